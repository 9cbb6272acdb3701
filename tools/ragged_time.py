#!/usr/bin/env python3
"""Exact mode, pairs of different sizes: one pair per call against one ragged call ("Ragged batches").

64 pairs, L = 9, 100 Sinkhorn iterations, the default k schedule, counts drawn by seed uniformly from [--lo, --hi] per frame.
In one process, alternating, after warming all:
  (a) 64 single-pair ``forward`` calls (what test.py's batch_size=1 loop does),
  (b) one ``forward_ragged`` of the 64, packed once outside the clock (``ops.pack_ragged``),
  (b') the same on the LIST of per-pair dicts, as INTEGRATION.md's loop calls it: packing inside the clock,
  (c) for scale, ``forward`` on 64 uniform pairs of the largest count.
Device-synchronised host clock; the median of --windows windows and their spread (min .. max)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgat_matcher_amd import MDGAT, ops, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--lo', type=int, default=128)
    ap.add_argument('--hi', type=int, default=256)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--profile', action='store_true', help='per-stage times of one ragged call (mdgat_profile)')
    a = ap.parse_args()
    dev = 'cuda:0'
    L = 9
    cfg = synth.default_config(L=L, sinkhorn_iterations=100)
    net = MDGAT(cfg).double()
    net.load_state_dict(synth.make_state_dict(L=L, seed=1))
    net = net.eval().to(dev)
    rs = np.random.RandomState(a.seed)
    counts = [(int(rs.randint(a.lo, a.hi + 1)), int(rs.randint(a.lo, a.hi + 1))) for _ in range(a.pairs)]
    pairs = [{k: v.to(dev) for k, v in synth.make_batch(1, n, m, first_pair=b).items()} for b, (n, m) in enumerate(counts)]
    packed = ops.pack_ragged(pairs)
    Np, Mp = max(n for n, _ in counts), max(m for _, m in counts)
    uniform = synth.make_batch(a.pairs, Np, Mp, device=dev)

    def run_a():
        for p in pairs:
            net(p)

    def run_b():
        net.forward_ragged(packed)

    def run_b_list():
        net.forward_ragged(pairs)

    def run_c():
        net(uniform)

    legs = {'a_single_pair_calls': run_a, 'b_forward_ragged': run_b, 'b_list_with_packing': run_b_list, 'c_uniform_largest': run_c}
    times = {k: [] for k in legs}
    with torch.no_grad():
        for fn in legs.values():
            fn(); fn()
        torch.cuda.synchronize()
        for _ in range(a.windows):
            for name, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        prof = None
        if a.profile:
            net.profile(dev, True)
            run_b()
            torch.cuda.synchronize()
            prof = {k: v for k, v in net.profile(dev, False).items() if v[1]}
    med = {k: float(np.median(v)) for k, v in times.items()}
    # the work of the ragged batch relative to the uniform one: attention and Sinkhorn scale with N_b M_b (and N_b^2 + M_b^2), the
    # row-wise launches with N_b + M_b; both ratios are given
    quad = sum(n * n + m * m + 2 * n * m for n, m in counts) / (a.pairs * (Np + Mp) ** 2)
    lin = sum(n + m for n, m in counts) / (a.pairs * (Np + Mp))
    res = {'pairs': a.pairs, 'counts': [a.lo, a.hi], 'Np': Np, 'Mp': Mp, 'windows': a.windows,
           'ms_median': med, 'ms_min_max': {k: [float(min(v)), float(max(v))] for k, v in times.items()},
           'ms_per_pair': {k: v / a.pairs for k, v in med.items()},
           'ratio_a_over_b': med['a_single_pair_calls'] / med['b_forward_ragged'],
           'ratio_a_over_b_list': med['a_single_pair_calls'] / med['b_list_with_packing'],
           'work_ragged_over_uniform': {'quadratic': quad, 'linear': lin},
           'b_over_c': med['b_forward_ragged'] / med['c_uniform_largest']}
    if prof:
        res['profile_ms_launches'] = prof
    print(json.dumps(res))


if __name__ == '__main__':
    main()
