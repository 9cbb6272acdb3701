#!/usr/bin/env python3
"""GPU box: what training straight from a resident bank of raw records costs next to the training step itself.
64 pairs of 512 keypoints out of a bank of synthetic frames of 600-900 records each, whose saliencies are drawn so that some frames keep
more than 512 records (truncation) and some fewer (padding); L = 9, 100 Sinkhorn iterations, triplet loss.  Three measurements, each in a
fresh process of its own, the clocks left as they are: the median and min .. max of seven one-step windows after a warm-up step, in
HIP-event time and in wall time (a host stall shows in the second only).

  a  ``training_forward`` + backward on a batch that already lies on the device (the batch ``training_batch_frames`` made, beforehand):
     the step as it was, the floor
  b  ``training_forward_frames`` + backward from the bank: the same step with the assembly and the ground truth inside the clock
  c  ``training_batch_frames`` alone: the assemble launch, the ground-truth launch, the upload of the chunk's counts and starts and the
     read of the status words

No threshold is set here.  One JSON line per measurement and one with b - a next to c.

    python tools/train_frames_time.py [--pairs 64] [--n 512] [--L 9] [--iters 100] [--windows 7]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = 'cuda:0'


def make_bank(pairs, n, seed=3):
    """2 * pairs frames of 600-900 records; per frame the share of salient records is drawn so that the kept count lies on either side of n"""
    import numpy as np
    from mdgat_matcher_amd import ops
    rs = np.random.RandomState(seed)
    frames = []
    for _ in range(2 * pairs):
        m = int(rs.randint(600, 901))
        r = rs.standard_normal((m, 37)).astype(np.float32)
        r[:, :3] *= np.array([30.0, 30.0, 3.0], dtype=np.float32)
        r[:, 4:] = np.abs(r[:, 4:]) * 50
        share = rs.uniform(0.3, 0.95)
        r[:, 3] = np.where(rs.uniform(size=m) < share, rs.uniform(10.5, 30.0, m), rs.uniform(0.0, 10.0, m)).astype(np.float32)
        frames.append(r)
    kept = [int((f[:, 3] > 10).sum()) for f in frames]
    return ops.pack_frames(frames, DEV), kept


def child(args):
    import torch
    from mdgat_matcher_amd import MDGAT, synth
    torch.backends.cuda.matmul.allow_tf32 = False
    net = MDGAT(synth.default_config(L=args.L, sinkhorn_iterations=args.iters)).double()
    net.load_state_dict(synth.make_state_dict(L=args.L, seed=1))
    net = net.to(DEV).train()
    bank, kept = make_bank(args.pairs, args.n)
    idx0, idx1 = list(range(0, 2 * args.pairs, 2)), list(range(1, 2 * args.pairs, 2))
    opts = dict(max_keypoints=args.n, gt_threshold=1.5)           # (identity transforms: synthetic frames share one sensor frame)
    resident = net.training_batch_frames(bank, idx0, idx1, None, None, **opts)
    torch.cuda.synchronize()

    def step():
        if args.side == 'c':
            return net.training_batch_frames(bank, idx0, idx1, None, None, **opts)['rep']
        net.zero_grad(set_to_none=True)
        if args.side == 'a':
            out = net.training_forward({k: (v.clone() if k.startswith('gt_') else v) for k, v in resident.items()})
        else:
            out = net.training_forward_frames(bank, idx0, idx1, None, None, **opts)
        loss = out['loss'].mean()
        loss.backward()
        return loss
    res = step()                                             # warm-up
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        res = step()
        e1.record()
        e1.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(e0.elapsed_time(e1))
    r = lambda x: round(x, 3)          # noqa: E731
    print(json.dumps({'side': args.side, 'pairs': args.pairs, 'n': args.n, 'L': args.L, 'iters': args.iters,
                      'frames_truncated': sum(k > args.n for k in kept), 'frames_padded': sum(k < args.n for k in kept),
                      'ms': r(statistics.median(ev)), 'min_ms': r(min(ev)), 'max_ms': r(max(ev)),
                      'wall_ms': r(statistics.median(wall)), 'wall_min_ms': r(min(wall)), 'wall_max_ms': r(max(wall)),
                      'result': float(res.detach().double().sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--L', type=int, default=9)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--side', choices=('a', 'b', 'c'), default=None)
    ap.add_argument('--child-timeout', type=float, default=150.0)
    args = ap.parse_args()
    if args.side is not None:
        return child(args)
    recs = {}
    for side in ('a', 'b', 'c'):             # a fresh process each; a child that fails or runs out of time ends the run (check=True)
        cmd = [sys.executable, os.path.abspath(__file__), '--side', side] + [f'--{k}={getattr(args, k)}' for k in ('pairs', 'n', 'L', 'iters', 'windows')]
        out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout, check=True).stdout
        line = [ln for ln in out.splitlines() if ln.startswith('{')][-1]
        print(line, flush=True)
        recs[side] = json.loads(line)
    a, b, c = recs['a'], recs['b'], recs['c']
    print(json.dumps({'b_minus_a_ms': round(b['ms'] - a['ms'], 3), 'c_ms': c['ms'], 'spread_of_a_ms': round(a['max_ms'] - a['min_ms'], 3),
                      'b_minus_a_wall_ms': round(b['wall_ms'] - a['wall_ms'], 3), 'c_wall_ms': c['wall_ms'],
                      'same_loss': a['result'] == b['result']}))


if __name__ == '__main__':
    main()
