#!/usr/bin/env python3
"""GPU box: forward + backward of the training-mode MLP through ops.mlp_f64 (csrc/mlp_grad.hip) next to what a user has without it:
torch autograd of the same nn.Sequential on the same device in float64.  R = 64 x 512 rows (the rows of one frame of configs[1]), the
three BN stacks (kenc 4-32-64-128-128, denc 33-64-128-128, layer 128+128-256-128 with two sources) and the bare 128 -> 384
convolution: the median over windows of HIP-event time per call, after warm-up (also of the forward and the backward alone,
ops.mlp_f64_forward / ops.mlp_f64_backward with every gradient asked for), and the peak of torch.cuda.max_memory_allocated above
the inputs for both.  One JSON line per stack, with the ratios the conditions of DESIGN section 7.7 are stated on.

    python tools/mlp_grad_time.py [--windows 7] [--per-window 3] [--rows 32768]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import mlp_grad_ref as R  # noqa: E402
from mdgat_matcher_amd import ops  # noqa: E402

DEV = 'cuda:0'


def window(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / k


def median_ms(fn, windows, per_window):
    fn()
    torch.cuda.synchronize()
    return statistics.median(window(fn, per_window) for _ in range(windows))


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--per-window', type=int, default=3)
    ap.add_argument('--rows', type=int, default=64 * 512)
    args = ap.parse_args()
    for stack in ('kenc', 'denc', 'layer', 'conv384'):
        x, p, dout = R.gpu_case(stack, args.rows)
        seq = R.torch_stack(p, True).to(DEV)
        mod = seq[0] if len(p['W']) == 1 else seq
        xd, g = torch.from_numpy(x).to(DEV).requires_grad_(), torch.from_numpy(dout).to(DEV)
        gt = g.t().contiguous()[None]
        split = 128 if stack == 'layer' else 0
        srcs = [xd] if not split else [xd.detach()[:, :split].contiguous().requires_grad_(), xd.detach()[:, split:].contiguous().requires_grad_()]
        xt = xd.detach().t().contiguous()[None].requires_grad_()           # torch's own layout [1, C, R]: no transposes in its time

        def ours():
            mod.zero_grad(set_to_none=True)
            for s in srcs:
                s.grad = None
            ops.mlp_f64(mod, *srcs).backward(g)

        def theirs():
            mod.zero_grad(set_to_none=True)
            xt.grad = None
            mod(xt).backward(gt)

        def clear():          # "above the inputs": no gradient of an earlier call is alive when the base is read
            mod.zero_grad(set_to_none=True)
            xt.grad = None
            for s in srcs:
                s.grad = None

        raw = [t.detach() for t in srcs] + [None] * (2 - len(srcs))
        saved = ops.mlp_f64_forward(mod, *raw)[1]
        rec = {'stack': stack, 'rows': args.rows,
               'forward_ms': round(median_ms(lambda: ops.mlp_f64_forward(mod, *raw), args.windows, args.per_window), 4),
               'backward_ms': round(median_ms(lambda: ops.mlp_f64_backward(mod, *raw, saved, g), args.windows, args.per_window), 4),
               'mlp_f64_ms': round(median_ms(ours, args.windows, args.per_window), 4),
               'torch_ms': round(median_ms(theirs, args.windows, args.per_window), 4)}
        clear()
        rec['mlp_f64_peak_mb'] = round(peak_extra(ours) / 2 ** 20, 1)
        clear()
        rec['torch_peak_mb'] = round(peak_extra(theirs) / 2 ** 20, 1)
        rec['time_ratio'] = round(rec['mlp_f64_ms'] / rec['torch_ms'], 3)
        rec['time_limit'] = 1.0 if stack in ('kenc', 'denc') else 1.3
        rec['ok'] = bool(rec['time_ratio'] <= rec['time_limit'] and rec['mlp_f64_peak_mb'] <= rec['torch_peak_mb'])
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
