#!/usr/bin/env python3
"""GPU box: the backward of the fp64 attention (ops.attention_f64_backward, csrc/attention_grad.hip) next to its forward
(ops.attention_f64, same shape, same form) and next to what a user has without it: torch autograd on the same device through a torch
transcription of the oracle's attention / dynamic_attention, forward + backward.  Shapes: 64 pairs of 512, full and topk = 128,
self and cross; 8 pairs of 2048, topk = 64.  Per shape one JSON line: the median over windows of HIP-event time per call, after
warm-up, the peak of torch.cuda.max_memory_allocated above the inputs, the backward's fp64 matrix work (FLOP of the seven products
of the formulas and the rate it ran at) and the largest difference between the two gradients.

Every shape is timed by a child process of its own under `timeout`; the first one that fails ends the run.

    python tools/attention_grad_time.py [--windows 7] [--per-window 3] [--no-torch] [--seconds 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
#         B,  N,    M,    cross, k
SHAPES = ((64, 512, 512, False, 0), (64, 512, 512, True, 0), (64, 512, 512, False, 128), (64, 512, 512, True, 128), (8, 2048, 2048, False, 64))


def torch_attention(qkv, N, M, cross, k):
    """The oracle's attention / dynamic_attention (top-k, softmax over the kept logits, scatter) on the library's layout."""
    import torch
    B = qkv.shape[0]
    fr = ((0, N), (N, N + M))
    out = []
    for side in range(2):
        lo, hi = fr[side]
        slo, shi = fr[1 - side] if cross else fr[side]
        q, kk, v = qkv[:, lo:hi, 0].permute(0, 2, 1, 3), qkv[:, slo:shi, 1].permute(0, 2, 1, 3), qkv[:, slo:shi, 2].permute(0, 2, 1, 3)
        logits = q @ kk.transpose(-1, -2) / 32 ** 0.5
        if k > 0:
            top = logits.topk(k, dim=3, largest=True, sorted=True)
            prob = torch.zeros_like(logits).scatter(3, top.indices, torch.softmax(top.values, dim=-1))
        else:
            prob = torch.softmax(logits, dim=-1)
        out.append((prob @ v).permute(0, 2, 1, 3).reshape(B, hi - lo, 128))
    return torch.cat(out, dim=1)


def one(idx, a):
    import torch
    sys.path.insert(0, ROOT)
    from mdgat_matcher_amd import _lib, ops

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def median_ms(fn):
        fn()
        torch.cuda.synchronize()
        return statistics.median(window(fn, a.per_window) for _ in range(a.windows))

    def peak_extra(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del out
        return peak

    B, N, M, cross, k = SHAPES[idx]
    gen = torch.Generator(device=DEV).manual_seed(N + k)
    qkv = torch.randn(B, N + M, 3, 4, 32, dtype=torch.float64, device=DEV, generator=gen) * 1.3
    dmsg = torch.randn(B, N + M, 128, dtype=torch.float64, device=DEV, generator=gen)
    _, sel = ops._attention_f64_values(qkv, N, M, cross, k, k > 0)
    fwd = lambda: ops.attention_f64(qkv, N, M, cross, topk=k)                                   # noqa: E731
    bwd = lambda: ops.attention_f64_backward(qkv, N, M, cross, dmsg, k, sel)                    # noqa: E731
    r = {'B': B, 'N': N, 'M': M, 'cross': cross, 'topk': k, 'forward_ms': round(median_ms(fwd), 3), 'backward_ms': round(median_ms(bwd), 3)}
    fl = 7 * 2.0 * B * 4 * 32 * 2 * N * M
    r.update(backward_over_forward=round(r['backward_ms'] / r['forward_ms'], 2), backward_gflop=round(fl / 1e9, 1),
             backward_tflops=round(fl / r['backward_ms'] / 1e9, 2),
             workspace_mb=round(_lib.load().mdgat_attention_backward_workspace_bytes(B, N, M) / 2 ** 20, 2),
             selection_mb=round((sel.numel() * 4 if sel is not None else 0) / 2 ** 20, 1),
             forward_peak_extra_mb=round(peak_extra(fwd) / 2 ** 20, 1), backward_peak_extra_mb=round(peak_extra(bwd) / 2 ** 20, 1))
    if not a.no_torch:
        def torch_step():
            x = qkv.detach().requires_grad_()
            (torch_attention(x, N, M, cross, k) * dmsg).sum().backward()
            return x.grad
        try:
            r['torch_autograd_peak_extra_mb'] = round(peak_extra(torch_step) / 2 ** 20, 1)
            r['torch_autograd_fwd_bwd_ms'] = round(median_ms(torch_step), 3)
            r['max_abs_diff_vs_torch'] = float((torch_step() - bwd()).abs().max())
        except torch.OutOfMemoryError as e:
            r['torch_autograd'] = f'out of memory: {str(e)[:80]}'
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--per-window', type=int, default=3)
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--seconds', type=int, default=240, help='time limit of one shape')
    ap.add_argument('--one', type=int, default=-1, help='(internal) time shape number ONE in this process')
    a = ap.parse_args()
    if a.one >= 0:
        return one(a.one, a)
    for i in range(len(SHAPES)):
        cmd = ['timeout', '-k', '10', str(a.seconds), sys.executable, os.path.abspath(__file__), '--one', str(i), '--windows', str(a.windows),
               '--per-window', str(a.per_window)] + (['--no-torch'] if a.no_torch else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f'shape {SHAPES[i]} ended with status {rc}: nothing further is started', flush=True)
            sys.exit(rc)


if __name__ == '__main__':
    main()
