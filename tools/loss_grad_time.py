#!/usr/bin/env python3
"""GPU box: the backward of the matching loss (ops.matching_loss_backward, csrc/loss_grad.hip) next to the forward
(ops.matching_loss) of the same build, and next to what a user has without it: torch autograd, on the same device and inputs,
through a torch transcription of the loss (tests/test_loss_grad_ref.py::torch_pair_losses), forward + backward.  fp64 Z at 64 pairs
of 512 and 8 pairs of 2048, every method: the median over windows of HIP-event time per call, after warm-up, and the peak of
torch.cuda.max_memory_allocated above the inputs.  Asserts that the HIP path's peak extra memory is dZ plus the
mdgat_loss_backward_workspace_bytes workspace (and the few bytes of the call's bookkeeping).  One JSON line per shape and method.

    python tools/loss_grad_time.py [--windows 7] [--per-window 3] [--no-torch]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from loss_ref import GT_PATTERNS, gt_batch  # noqa: E402
from mdgat_matcher_amd import _lib, ops  # noqa: E402

DEV = 'cuda:0'
SHAPES = ((64, 512), (8, 2048))
METHODS = ('superglue', 'triplet_loss', 'gap_loss')


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--per-window', type=int, default=3)
    ap.add_argument('--no-torch', action='store_true')
    a = ap.parse_args()
    from test_loss_grad_ref import torch_pair_losses
    lib = _lib.load()
    for B, N in SHAPES:
        gen = torch.Generator().manual_seed(0)
        s = ((torch.rand(B, N, N, generator=gen, dtype=torch.float64) * 2 - 1) * 15).to(DEV)
        Z = ops.sinkhorn_f64(s, 0.0, 20)
        del s
        g0, g1 = gt_batch([GT_PATTERNS[b % len(GT_PATTERNS)] for b in range(B)], N, N, seed=N)
        t0, t1 = torch.from_numpy(g0).to(DEV), torch.from_numpy(g1).to(DEV)
        d = torch.full((B,), 1.0 / B, dtype=torch.float64, device=DEV)
        for meth in METHODS:
            fwd = lambda: ops.matching_loss(Z, t0, t1, meth, 0.5)                      # noqa: E731
            bwd = lambda: ops.matching_loss_backward(Z, t0, t1, meth, 0.5, d)          # noqa: E731
            r = {'B': B, 'N': N, 'M': N, 'method': meth, 'forward_ms': round(median_ms(fwd, a.windows, a.per_window), 3),
                 'backward_ms': round(median_ms(bwd, a.windows, a.per_window), 3)}
            ws = lib.mdgat_loss_backward_workspace_bytes(B, N, N)
            dz = Z.numel() * 8
            peak = peak_extra(bwd)
            # dZ + the workspace; the caching allocator rounds each of the two up to its 2 MiB granule, and dloss, the bad word and the
            # int64 gts (no copies when they are int64 already) to 512 bytes
            assert peak <= dz + ws + 2 * (2 << 20) + 16 * 512 + 2 * t0.numel() * 8, (peak, dz, ws)
            r.update(dZ_mb=round(dz / 2 ** 20, 1), workspace_mb=round(ws / 2 ** 20, 1), backward_peak_extra_mb=round(peak / 2 ** 20, 1))
            if not a.no_torch:
                def torch_step():
                    z = Z.detach().requires_grad_()
                    torch_pair_losses(z, t0, t1, meth, 0.5).mean().backward()
                    return z.grad
                try:
                    r['torch_autograd_peak_extra_mb'] = round(peak_extra(torch_step) / 2 ** 20, 1)
                    r['torch_autograd_fwd_bwd_ms'] = round(median_ms(torch_step, a.windows, 1), 3)
                    ref, got = torch_step(), bwd()
                    r['max_abs_diff_vs_torch'] = float((ref - got).abs().max())
                    del ref, got
                except torch.OutOfMemoryError as e:
                    r['torch_autograd'] = f'out of memory: {str(e)[:80]}'
                torch.cuda.empty_cache()
            print(json.dumps(r), flush=True)
        del Z
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
