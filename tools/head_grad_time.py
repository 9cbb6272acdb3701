#!/usr/bin/env python3
"""GPU box: the matching head (ops.match_head) and its backward (ops.match_head_backward, csrc/head_grad.hip) next to what a user
has without them: torch autograd, on the same device and inputs, through the two reference lines in fp64
(tests/test_head_grad_ref.py::torch_head), forward + backward.  64 pairs of 512 and 8 pairs of 2048: the median over windows of
HIP-event time per call, after warm-up, the peak of torch.cuda.max_memory_allocated above the inputs, the backward's fp64 matrix
work (FLOP and the rate it ran at) and the largest difference between the two sets of gradients.  One JSON line per shape.

    python tools/head_grad_time.py [--windows 7] [--per-window 3] [--no-torch]
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
from mdgat_matcher_amd import _lib, ops  # noqa: E402

DEV = 'cuda:0'
SHAPES = ((64, 512, 512), (8, 2048, 2048))


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
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def backward_flop(B, N, M):
    """The recomputed projections, dmd of both frames, ddesc of both frames, dW."""
    return 2.0 * B * 128 * (3 * 128 * (N + M) + 2 * N * M)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--per-window', type=int, default=3)
    ap.add_argument('--no-torch', action='store_true')
    a = ap.parse_args()
    from test_head_grad_ref import random_inputs, torch_head
    lib = _lib.load()
    for B, N, M in SHAPES:
        d0, d1, W, b, G = [torch.from_numpy(x).to(DEV) for x in random_inputs(B, N, M, N)]
        fwd = lambda: ops.match_head(d0, d1, W, b)                      # noqa: E731
        bwd = lambda: ops.match_head_backward(d0, d1, W, b, G)          # noqa: E731
        r = {'B': B, 'N': N, 'M': M, 'forward_ms': round(median_ms(fwd, a.windows, a.per_window), 3),
             'backward_ms': round(median_ms(bwd, a.windows, a.per_window), 3)}
        fl = backward_flop(B, N, M)
        r.update(backward_gflop=round(fl / 1e9, 2), backward_tflops=round(fl / r['backward_ms'] / 1e9, 2),
                 dscores_mb=round(G.numel() * 8 / 2 ** 20, 1), workspace_mb=round(lib.mdgat_match_head_workspace_bytes(B, N, M) / 2 ** 20, 1),
                 forward_peak_extra_mb=round(peak_extra(fwd) / 2 ** 20, 1), backward_peak_extra_mb=round(peak_extra(bwd) / 2 ** 20, 1))
        if not a.no_torch:
            def torch_step():
                t = [x.detach().requires_grad_() for x in (d0, d1, W, b)]
                (torch_head(*t) * G).sum().backward()
                return [x.grad for x in t]

            def torch_fwd():
                with torch.no_grad():
                    return torch_head(d0, d1, W, b)
            try:
                r['torch_forward_ms'] = round(median_ms(torch_fwd, a.windows, a.per_window), 3)
                r['torch_autograd_peak_extra_mb'] = round(peak_extra(torch_step) / 2 ** 20, 1)
                r['torch_autograd_fwd_bwd_ms'] = round(median_ms(torch_step, a.windows, a.per_window), 3)
                ref, got = torch_step(), bwd()
                r['max_abs_diff_vs_torch'] = max(float((x - y).abs().max()) for x, y in zip(ref, got))
                del ref, got
            except torch.OutOfMemoryError as e:
                r['torch_autograd'] = f'out of memory: {str(e)[:80]}'
            torch.cuda.empty_cache()
        print(json.dumps(r), flush=True)
        del d0, d1, W, b, G
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
