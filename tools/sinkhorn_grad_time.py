#!/usr/bin/env python3
"""GPU box: the fp64 Sinkhorn's forward (ops.sinkhorn_f64) against its backward (ops.sinkhorn_backward, csrc/sinkhorn_grad.hip) at
BASELINE configs[1]'s shape (64 pairs of 512, T = 100) and configs[4]'s (8 pairs of 2048, T = 200): the median over windows of
HIP-event time per call, after warm-up, the two alternating.  Prints one JSON line per shape.

    python tools/sinkhorn_grad_time.py [--windows 7] [--per-window 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgat_matcher_amd import _lib, ops  # noqa: E402

DEV = 'cuda:0'
SHAPES = ((64, 512, 100), (8, 2048, 200))


def window(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--per-window', type=int, default=3)
    a = ap.parse_args()
    for B, N, T in SHAPES:
        gen = torch.Generator().manual_seed(0)
        s = ((torch.rand(B, N, N, generator=gen, dtype=torch.float64) * 2 - 1) * 4).to(DEV)
        dZ = torch.randn(B, N + 1, N + 1, generator=gen, dtype=torch.float64).to(DEV)
        fwd = lambda: ops.sinkhorn_f64(s, 1.0, T)                # noqa: E731
        bwd = lambda: ops.sinkhorn_backward(s, 1.0, T, dZ)       # noqa: E731
        for fn in (fwd, bwd):
            fn()
        torch.cuda.synchronize()
        tf, tb = [], []
        for _ in range(a.windows):
            tf.append(window(fwd, a.per_window))
            tb.append(window(bwd, a.per_window))
        ws = _lib.load().mdgat_sinkhorn_backward_workspace_bytes(B, N, N, T)
        print(json.dumps({'B': B, 'N': N, 'M': N, 'iters': T, 'forward_ms': round(statistics.median(tf), 3),
                          'backward_ms': round(statistics.median(tb), 3), 'backward_over_forward': round(statistics.median(tb) / statistics.median(tf), 2),
                          'backward_workspace_mb': round(ws / 2 ** 20, 1), 'windows': a.windows, 'per_window': a.per_window}), flush=True)


if __name__ == '__main__':
    main()
