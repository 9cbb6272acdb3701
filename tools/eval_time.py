#!/usr/bin/env python3
"""GPU box: what the evaluation scripts' per-pair metrics cost next to the forward they follow, at B=64 pairs of N=M=512 keypoints
(BASELINE configs[1]: L=9, S=100) and at one pair of 256 (test.py's shape), wall-clock on the host with the device synchronised at
both ends of a window, the median of 7 windows after warm-up:

  (a) ops.evaluate_matches on the forward's device outputs plus the ONE device-to-host copy of the table (what EvalMeter.update does)
  (b) the scripts' host loop: the literal restatement (tests/eval_ref.py: test.py:212-311, comprehensions and numpy SVD included),
      with its per-tensor .cpu().numpy() copies from the device, over the same pairs
  (c) the forward alone, in both arithmetics

Each step runs in a child process of its own under a time limit (a step that fails or runs out of time ends the tool).

    python tools/eval_time.py [--windows 7] [--timeout 240]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

DEV = 'cuda:0'
L, S = 9, 100
SHAPES = ((64, 512), (1, 256))
STEPS = ('a', 'b', 'c-fp64', 'c-fp32')


def _inputs(B, N):
    """A forward's outputs (fp32-class path; the metrics do not care which arithmetic matched) and ground truth of the usual density."""
    import torch
    from mdgat_matcher_amd import MDGAT, synth
    d = synth.make_batch(B, N, N, device=DEV)
    net = MDGAT(synth.default_config(L=L, sinkhorn_iterations=S, arithmetic='fp32')).double()
    net.load_state_dict(synth.make_state_dict(L=L, seed=0))
    net = net.eval().to(DEV)
    with torch.no_grad():
        out = net(d)
    gen = torch.Generator().manual_seed(0)
    gt0 = torch.stack([torch.randperm(N, generator=gen) for _ in range(B)])
    gt1 = torch.argsort(gt0, dim=1)
    drop = torch.rand((B, N), generator=gen) < 0.4
    for b in range(B):
        gt1[b, gt0[b, drop[b]]] = -1
    gt0[drop] = -1
    pred = {**d, **out, 'gt_matches0': gt0.to(DEV), 'gt_matches1': gt1.to(DEV),
            'T_gt': torch.eye(4, dtype=torch.float64, device=DEV).repeat(B, 1, 1), 'idx0': list(range(B))}
    return pred


def _windows(fn, windows, per_window, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(per_window):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / per_window * 1e3)
    return sorted(ts)


def step(name, B, N, windows):
    import torch
    from mdgat_matcher_amd import MDGAT, ops, synth
    if name.startswith('c-'):
        arith = name[2:]
        d = synth.make_batch(B, N, N, device=DEV)
        net = MDGAT(synth.default_config(L=L, sinkhorn_iterations=S, arithmetic=arith)).double()
        net.load_state_dict(synth.make_state_dict(L=L, seed=0))
        net = net.eval().to(DEV)
        args = (d['keypoints0'], d['scores0'], d['descriptors0'], d['keypoints1'], d['scores1'], d['descriptors1'])
        with torch.no_grad():
            ts = _windows(lambda: net._run(*args), windows, 4)
    elif name == 'a':
        p = _inputs(B, N)

        def fn():
            m, _, _ = ops.evaluate_matches(p['matches0'], p['matches1'], p['gt_matches0'], p['gt_matches1'], p['keypoints0'], p['keypoints1'],
                                           T_gt=p['T_gt'])
            return m.cpu()
        ts = _windows(fn, windows, 8)
    else:
        import eval_ref as E
        p = _inputs(B, N)
        p['matching_scores0'] = p['matching_scores0'].double()

        def fn():
            meter = E.TestPyMeter()
            for b in range(B):
                E.test_py_pair(p, b, meter)
        ts = _windows(fn, windows, 1, warmup=1)
    print(json.dumps({'step': name, 'pairs': B, 'keypoints': N, 'ms_median': ts[len(ts) // 2], 'ms_min': ts[0], 'ms_max': ts[-1],
                      'windows': windows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--timeout', type=int, default=240)
    ap.add_argument('--step', choices=STEPS)
    ap.add_argument('--pairs', type=int)
    ap.add_argument('--keypoints', type=int)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.pairs, a.keypoints, a.windows)
    res = {}
    for B, N in SHAPES:
        for name in STEPS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', name, '--pairs', str(B), '--keypoints', str(N),
                                '--windows', str(a.windows)], timeout=a.timeout, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                sys.exit(f'step {name} at {B} x {N} ended with status {r.returncode}: stopping')
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            res[(B, N, name)] = json.loads(line)['ms_median']
    for B, N in SHAPES:
        a_, b_, c64, c32 = (res[(B, N, s)] for s in STEPS)
        print(f'{B} x {N}: (a) {a_:.3f} ms = {100 * a_ / c64:.2f} % of the exact forward ({c64:.3f} ms), {100 * a_ / c32:.2f} % of the '
              f'fp32-class one ({c32:.3f} ms); (b) {b_:.1f} ms = {b_ / a_:.0f} x (a)')


if __name__ == '__main__':
    main()
