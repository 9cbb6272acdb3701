#!/usr/bin/env python3
"""GPU box: what the evaluation loss (csrc/loss.hip) adds to a forward at BASELINE configs[1] (B=64, N=M=512, L=9, S=100), in both
arithmetic modes and for every loss method: the median over windows of HIP-event time of the forward with the loss on and off,
after warm-up, alternating the two.  The loss kernels' own time: run `--trace` (a few loss-on forwards, nothing timed) under
`rocprofv3 --kernel-trace --stats`.

    python tools/loss_time.py [--windows 7] [--per-window 4] [--trace]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgat_matcher_amd import MDGAT, synth  # noqa: E402

DEV = 'cuda:0'
B, N, L, S = 64, 512, 9, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--per-window', type=int, default=4)
    ap.add_argument('--trace', action='store_true')
    a = ap.parse_args()
    d = synth.make_batch(B, N, N, device=DEV)
    gen = torch.Generator().manual_seed(0)
    d['gt_matches0'] = torch.randint(-1, N, (B, N), generator=gen).to(DEV)
    d['gt_matches1'] = torch.randint(-1, N, (B, N), generator=gen).to(DEV)
    args = (d['keypoints0'], d['scores0'], d['descriptors0'], d['keypoints1'], d['scores1'], d['descriptors1'])
    for arith in ('fp64', 'fp32'):
        for method in ('triplet_loss', 'gap_loss', 'superglue'):
            net = MDGAT(synth.default_config(L=L, sinkhorn_iterations=S, arithmetic=arith, loss_method=method)).double()
            net.load_state_dict(synth.make_state_dict(L=L, seed=0))
            net = net.eval().to(DEV)
            req = net._loss_request(d, d['keypoints0'], d['keypoints1'])
            with torch.no_grad():
                if a.trace:
                    for _ in range(3):
                        net._run(*args, loss=req)
                    torch.cuda.synchronize()
                    print(f'{arith} {method}: traced 3 loss-on forwards')
                    continue
                for _ in range(2):
                    net._run(*args)
                    net._run(*args, loss=req)
                torch.cuda.synchronize()
                times = {False: [], True: []}
                for _ in range(a.windows):
                    for on in (False, True):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.per_window):
                            net._run(*args, loss=req if on else None)
                        e1.record()
                        torch.cuda.synchronize()
                        times[on].append(e0.elapsed_time(e1) / a.per_window)
            med = {on: sorted(v)[len(v) // 2] for on, v in times.items()}
            spread = {on: (min(v), max(v)) for on, v in times.items()}
            print(f'{arith} {method}: off {med[False]:.3f} ms (range {spread[False][0]:.3f}-{spread[False][1]:.3f}), on {med[True]:.3f} ms '
                  f'(range {spread[True][0]:.3f}-{spread[True][1]:.3f}), overhead {med[True] - med[False]:+.3f} ms = '
                  f'{100 * (med[True] / med[False] - 1):+.2f} %', flush=True)
            del net


if __name__ == '__main__':
    main()
