#!/usr/bin/env python3
"""Pairs of different sizes: one pair per call against one ragged call, in the exact mode and on the fp32-class path ("Ragged
batches").

64 pairs, L = 9, 100 Sinkhorn iterations, the default k schedule, counts drawn by seed uniformly from [--lo, --hi] per frame.
In one process, alternating, after warming all:
  (a) 64 single-pair ``forward`` calls (what test.py's batch_size=1 loop does),
  (b) one ``forward_ragged`` of the 64, packed once outside the clock (``ops.pack_ragged``),
  (b') the same on the LIST of per-pair dicts, as INTEGRATION.md's loop calls it: packing inside the clock,
  (c) for scale, ``forward`` on 64 uniform pairs of the largest count,
  (d) one ``match_frames_ragged`` of the 64 out of a bank of their 128 frames' raw float32 records, uploaded once outside the clock
      (``ops.pack_frames``): decode, normalisation and padding on the device,
  (d') the same with ``ops.pack_frames`` - the concatenation of the host records and the upload - inside the clock.
(The records are the pairs' own arrays narrowed to float32, so (d) re-normalises FPFH rows that are already normalised: the same work as
on loader records, results equal to (b)'s to float32 rounding of the inputs.)
The fp32-class legs, in the same run (a float32 module with config['ragged_arithmetic'] = 'module'):
  (f32 b) one ``forward_ragged`` of the 64, packed beforehand; (f32 b') the same with ``ops.pack_ragged`` inside the clock;
  (f32 a) 64 single-pair fp32-class ``forward`` calls; (f32 c) the uniform fp32-class batch of the slot size;
  (f32 d) one ``match_frames_ragged`` of the 64 out of the bank uploaded beforehand (the encoder kernel reads the records itself);
  (f32 d') the same with ``ops.pack_frames`` and the upload inside the clock;
  (f32 b split) / (f32 d split) (f32 b) and (f32 d) on a module with config['ragged_sinkhorn_fp32'] = 'split': the split form of the fp32
      Sinkhorn, one launch per iteration, a pair's rows over ceil(Np / 128) workgroups;
  (f32 gloabal) for the record, ``forward_ragged`` of the packed 64 on a float32 'FPFH_gloabal' module (its encoders in fp64).
Device-synchronised host clock; the median of --windows windows and their spread (min .. max).

Ranges beyond the register-resident fp64 Sinkhorn (575 keypoints): ``--ragged_sinkhorn auto`` (or ``streaming``) builds the exact module
with that config key, and the ranges ``--lo 512 --hi 1024`` and ``--lo 1024 --hi 2048`` then run the exact legs on the streaming fp64
Sinkhorn with per-pair counts.  Its K workspace follows the SLOT (35.6 MB per pair at 2048; 16 pairs: 570 MB), so --pairs defaults to 16
and 8 there, 64 below.  The fp32-class ragged forward holds 512 keypoints per frame; for larger ranges - up to 2048 - its modules are built
with config['ragged_slots_fp32'] = 'wide', and the default and the split Sinkhorn run side by side as below (the bank legs and the
pooled descriptor's as well).

``--per_op``: instead of all the above, the streaming ragged per-op launch (``ops.sinkhorn_f64(..., counts=, form='streaming')``, 100
iterations) on the counts (40, 1200), (1100, 40), (40, 33), (64, 64) in their slots of 1100 x 1200, against the uniform streaming launch
of four pairs of the slot size, and the same with the four repeated eight times (32 pairs: beyond the launch-latency floor of the 201
launches): small pairs in large slots must cost less than the slot."""
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
    ap.add_argument('--pairs', type=int, default=None, help='default: 64 up to 575 keypoints, 16 up to 1024, 8 beyond')
    ap.add_argument('--ragged_sinkhorn', choices=['resident', 'auto', 'streaming'], default='resident',
                    help="config['ragged_sinkhorn'] of the exact module; counts beyond 575 need 'auto' or 'streaming'")
    ap.add_argument('--per_op', action='store_true', help='the streaming ragged Sinkhorn launch against the uniform one of the slot size')
    ap.add_argument('--lo', type=int, default=128)
    ap.add_argument('--hi', type=int, default=256)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--profile', action='store_true', help='per-stage times of one ragged call (mdgat_profile)')
    ap.add_argument('--split_only', action='store_true', help="only (f32 b), (f32 d) and their 'split' twins: the two forms of the fp32 Sinkhorn side by side")
    a = ap.parse_args()
    dev = 'cuda:0'
    if a.per_op:
        return per_op(dev, a.windows)
    if a.pairs is None:
        a.pairs = 64 if a.hi <= MDGAT.RAGGED_MAX_KEYPOINTS else 16 if a.hi <= 1024 else 8
    if a.hi > MDGAT.RAGGED_MAX_KEYPOINTS and a.ragged_sinkhorn == 'resident':
        ap.error(f'counts up to {a.hi} are beyond the register-resident fp64 Sinkhorn ({MDGAT.RAGGED_MAX_KEYPOINTS}): --ragged_sinkhorn auto')
    with_f32 = a.hi <= MDGAT.RAGGED_FP32_WIDE_MAX_KEYPOINTS
    wide = {'ragged_slots_fp32': 'wide'} if a.hi > MDGAT.RAGGED_FP32_MAX_KEYPOINTS else {}
    L = 9
    cfg = synth.default_config(L=L, sinkhorn_iterations=100)
    net = MDGAT({**cfg, 'ragged_sinkhorn': a.ragged_sinkhorn}).double()
    net.load_state_dict(synth.make_state_dict(L=L, seed=1))
    net = net.eval().to(dev)
    net32 = MDGAT({**cfg, **wide, 'ragged_arithmetic': 'module'})
    net32.load_state_dict(synth.make_state_dict(L=L, seed=1))
    net32 = net32.float().eval().to(dev)
    net32s = MDGAT({**cfg, **wide, 'ragged_arithmetic': 'module', 'ragged_sinkhorn_fp32': 'split'})
    net32s.load_state_dict(synth.make_state_dict(L=L, seed=1))
    net32s = net32s.float().eval().to(dev)
    net32g = MDGAT({**cfg, **wide, 'ragged_arithmetic': 'module', 'descriptor': 'FPFH_gloabal'})
    net32g.load_state_dict(synth.make_state_dict(L=L, seed=1, descriptor='FPFH_gloabal'))
    net32g = net32g.float().eval().to(dev)
    rs = np.random.RandomState(a.seed)
    counts = [(int(rs.randint(a.lo, a.hi + 1)), int(rs.randint(a.lo, a.hi + 1))) for _ in range(a.pairs)]
    pairs = [{k: v.to(dev) for k, v in synth.make_batch(1, n, m, first_pair=b).items()} for b, (n, m) in enumerate(counts)]
    packed = ops.pack_ragged(pairs)
    Np, Mp = max(n for n, _ in counts), max(m for _, m in counts)
    uniform = synth.make_batch(a.pairs, Np, Mp, device=dev)
    # the frames as np.fromfile(...).reshape(-1, 37) would give them: host float32 records, frame 0 and frame 1 of every pair
    frames = [torch.cat([p['keypoints' + f][0], p['scores' + f][0][:, None], p['descriptors' + f][0]], -1).float().cpu().numpy() for p in pairs for f in '01']
    idx0, idx1 = list(range(0, 2 * a.pairs, 2)), list(range(1, 2 * a.pairs, 2))
    bank = ops.pack_frames(frames, dev)

    def run_a():
        for p in pairs:
            net(p)

    def run_b():
        net.forward_ragged(packed)

    def run_b_list():
        net.forward_ragged(pairs)

    def run_c():
        net(uniform)

    def run_d():
        net.match_frames_ragged(bank, idx0, idx1)

    def run_d_pack():
        net.match_frames_ragged(ops.pack_frames(frames, dev), idx0, idx1)

    def run_a32():
        for p in pairs:
            net32(p)

    legs = {'a_single_pair_calls': run_a, 'b_forward_ragged': run_b, 'b_list_with_packing': run_b_list, 'c_uniform_largest': run_c,
            'd_match_frames_ragged': run_d, 'd_with_pack_frames': run_d_pack,
            'f32_a_single_pair_calls': run_a32, 'f32_b_forward_ragged': lambda: net32.forward_ragged(packed),
            'f32_b_list_with_packing': lambda: net32.forward_ragged(pairs), 'f32_c_uniform_largest': lambda: net32(uniform),
            'f32_d_match_frames_ragged': lambda: net32.match_frames_ragged(bank, idx0, idx1),
            'f32_d_with_pack_frames': lambda: net32.match_frames_ragged(ops.pack_frames(frames, dev), idx0, idx1),
            'f32_b_split_forward_ragged': lambda: net32s.forward_ragged(packed),
            'f32_d_split_match_frames_ragged': lambda: net32s.match_frames_ragged(bank, idx0, idx1),
            'f32_gloabal_forward_ragged': lambda: net32g.forward_ragged(packed)}
    if not with_f32:
        legs = {k: v for k, v in legs.items() if not k.startswith('f32_')}
    if a.split_only:
        if not with_f32:
            ap.error('--split_only: the fp32-class ragged forward holds 2048 keypoints per frame')
        legs = {k: legs[k] for k in ('f32_b_forward_ragged', 'f32_b_split_forward_ragged', 'f32_d_match_frames_ragged', 'f32_d_split_match_frames_ragged')}
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
        prof = prof_d = prof32 = prof32_d = prof32s = None
        if a.profile:
            if with_f32:
                net32s.profile(dev, True)
                net32s.forward_ragged(packed)
                torch.cuda.synchronize()
                prof32s = {k: v for k, v in net32s.profile(dev, False).items() if v[1]}
                net32.profile(dev, True)
                net32.forward_ragged(packed)
                torch.cuda.synchronize()
                prof32 = {k: v for k, v in net32.profile(dev, True).items() if v[1]}
                net32.match_frames_ragged(bank, idx0, idx1)
                torch.cuda.synchronize()
                prof32_d = {k: v for k, v in net32.profile(dev, False).items() if v[1]}
        if a.profile and not a.split_only:
            net.profile(dev, True)
            run_b()
            torch.cuda.synchronize()
            prof = {k: v for k, v in net.profile(dev, True).items() if v[1]}
            run_d()
            torch.cuda.synchronize()
            prof_d = {k: v for k, v in net.profile(dev, False).items() if v[1]}
    med = {k: float(np.median(v)) for k, v in times.items()}
    # the work of the ragged batch relative to the uniform one: attention and Sinkhorn scale with N_b M_b (and N_b^2 + M_b^2), the
    # row-wise launches with N_b + M_b; both ratios are given
    quad = sum(n * n + m * m + 2 * n * m for n, m in counts) / (a.pairs * (Np + Mp) ** 2)
    lin = sum(n + m for n, m in counts) / (a.pairs * (Np + Mp))
    res = {'pairs': a.pairs, 'counts': [a.lo, a.hi], 'Np': Np, 'Mp': Mp, 'windows': a.windows, 'ragged_sinkhorn': a.ragged_sinkhorn,
           'ms_median': med, 'ms_min_max': {k: [float(min(v)), float(max(v))] for k, v in times.items()},
           'ms_per_pair': {k: v / a.pairs for k, v in med.items()}}
    if with_f32:
        res['f32_split_over_pair'] = {'b': med['f32_b_split_forward_ragged'] / med['f32_b_forward_ragged'],
                                      'd': med['f32_d_split_match_frames_ragged'] / med['f32_d_match_frames_ragged']}
    if prof32s:
        res['profile_ms_launches_f32_b_split'] = prof32s
    if a.split_only:
        if prof32:
            res['profile_ms_launches_f32_b'] = prof32
        print(json.dumps(res))
        return
    res.update({
           'ratio_a_over_b': med['a_single_pair_calls'] / med['b_forward_ragged'],
           'ratio_a_over_b_list': med['a_single_pair_calls'] / med['b_list_with_packing'],
           'work_ragged_over_uniform': {'quadratic': quad, 'linear': lin},
           'b_over_c': med['b_forward_ragged'] / med['c_uniform_largest'],
           'd_over_b': med['d_match_frames_ragged'] / med['b_forward_ragged'],
           'd_pack_over_b_list': med['d_with_pack_frames'] / med['b_list_with_packing'],
           'pairs_per_s': {k: 1e3 * a.pairs / v for k, v in med.items()}})
    if with_f32:
        res.update({'f32_ratio_a_over_b': med['f32_a_single_pair_calls'] / med['f32_b_forward_ragged'],
                    'f32_b_over_c': med['f32_b_forward_ragged'] / med['f32_c_uniform_largest'],
                    'f32_b_over_exact_b': med['f32_b_forward_ragged'] / med['b_forward_ragged'],
                    'f32_d_over_b': med['f32_d_match_frames_ragged'] / med['f32_b_forward_ragged'],
                    'f32_d_pack_over_b_list': med['f32_d_with_pack_frames'] / med['f32_b_list_with_packing']})
    if prof:
        res['profile_ms_launches'] = prof
        res['profile_ms_launches_d'] = prof_d
    if prof32:
        res['profile_ms_launches_f32_b'] = prof32
        res['profile_ms_launches_f32_d'] = prof32_d
    print(json.dumps(res))


def per_op(dev, windows):
    for reps in (1, 8):
        per_op_case(dev, windows, reps)


def per_op_case(dev, windows, reps):
    from mdgat_matcher_amd import _lib
    counts = ((40, 1200), (1100, 40), (40, 33), (64, 64)) * reps
    Np, Mp, iters = max(n for n, _ in counts), max(m for _, m in counts), 100
    rs = np.random.RandomState(0)
    s = torch.from_numpy(rs.standard_normal((len(counts), Np, Mp)) * 3.0).to(dev)
    cnt = ([n for n, _ in counts], [m for _, m in counts])
    cnt = {'counts0_host': torch.tensor(cnt[0], dtype=torch.int32), 'counts1_host': torch.tensor(cnt[1], dtype=torch.int32)}
    cnt.update(counts0=cnt['counts0_host'].to(dev), counts1=cnt['counts1_host'].to(dev))
    alone = [s[b:b + 1, :n, :m].contiguous() for b, (n, m) in enumerate(counts)]
    lib = _lib.load()
    legs = {'stream_ragged': lambda: ops.sinkhorn_f64(s, 1.0, iters, counts=cnt, form='streaming'),
            'uniform_streaming_slot_size': lambda: ops.sinkhorn_f64(s, 1.0, iters),
            'pairs_alone_streaming': lambda: [ops.sinkhorn_f64(x, 1.0, iters) for x in alone]}
    times = {k: [] for k in legs}
    prev = lib.mdgat_set_f64_sinkhorn_form(1)
    try:
        for fn in legs.values():
            fn(); fn()
        for _ in range(windows):
            for name, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
    finally:
        lib.mdgat_set_f64_sinkhorn_form(prev)
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({'per_op': 'sinkhorn_f64', 'counts': counts, 'Np': Np, 'Mp': Mp, 'iters': iters, 'windows': windows, 'ms_median': med,
                      'ms_min_max': {k: [float(min(v)), float(max(v))] for k, v in times.items()},
                      'ragged_over_uniform': med['stream_ragged'] / med['uniform_streaming_slot_size']}))


if __name__ == '__main__':
    main()
