#!/usr/bin/env python3
"""GPU box: what the descriptor encoders cost.  One forward (``MDGAT.match``) at 64 pairs of 512 keypoints, L = 9, 100 Sinkhorn
iterations, for a float64 module (the exact mode) and a float32 one, and one training step (``training_forward`` +
``loss.mean().backward()``, tools/train_step_time.py's method) per descriptor.  Every measurement runs in a fresh process; HIP-event
time per call, median over windows of ``--reps`` calls after a warm-up window.  One JSON line per measurement (DESIGN section 10.6
records them).  Copied into the tree of another commit it measures that commit's 'FPFH' for an A/B on the same box.

    python tools/descriptor_time.py [--descriptors FPFH FPFH_gloabal FPFH_only] [--what exact fp32 train]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = 'cuda:0'


def child(args):
    import torch
    from mdgat_matcher_amd import MDGAT, synth
    d, what = args.descriptors[0], args.what[0]
    kw = {} if d == 'FPFH' else {'descriptor': d}          # (the default descriptor also runs on a build from before the argument)
    cfg = synth.default_config(L=args.L, sinkhorn_iterations=args.iters, **kw)
    net = MDGAT(cfg).to(torch.float32 if what == 'fp32' else torch.float64)
    net.load_state_dict(synth.make_state_dict(L=args.L, seed=args.seed, **kw))
    net = net.to(DEV).train(what == 'train')
    data = synth.make_batch(args.pairs, args.n, args.n, device=DEV)
    if what == 'train':
        def call():
            net.zero_grad(set_to_none=True)
            net.training_forward({k: v.clone() for k, v in data.items()})['loss'].mean().backward()
        reps = 1
    else:
        a = [data[k].to(net.bin_score.dtype) for k in ('keypoints0', 'descriptors0', 'keypoints1', 'descriptors1', 'scores0', 'scores1')]

        def call():
            with torch.no_grad():
                net.match(*a)
        reps = args.reps
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / reps)
    fallback = bool(net.check(DEV)['sinkhorn_fallback']) if what != 'train' else False
    print(json.dumps({'descriptor': d, 'what': what, 'tree': os.path.basename(ROOT), 'pairs': args.pairs,
                      'n': args.n, 'L': args.L, 'iters': args.iters, 'ms': round(statistics.median(times), 3), 'min_ms': round(min(times), 3),
                      'max_ms': round(max(times), 3), 'seed': args.seed, 'sinkhorn_fallback': fallback}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--descriptors', nargs='+', default=['FPFH', 'FPFH_gloabal', 'FPFH_only'])
    ap.add_argument('--what', nargs='+', default=['exact', 'fp32', 'train'], choices=('exact', 'fp32', 'train'))
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--L', type=int, default=9)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--child-timeout', type=float, default=200.0)
    args = ap.parse_args()
    if args.child:
        return child(args)
    for what in args.what:
        for d in args.descriptors:
            cmd = [sys.executable, os.path.abspath(__file__), '--child', '--descriptors', d, '--what', what] + \
                  [f'--{k}={getattr(args, k)}' for k in ('pairs', 'n', 'L', 'iters', 'reps', 'windows', 'seed')]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout, check=True).stdout
            print([ln for ln in out.splitlines() if ln.startswith('{')][-1], flush=True)


if __name__ == '__main__':
    main()
