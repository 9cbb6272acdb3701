"""Ragged chunks straight from raw frame records on a float32 module, and the pooled descriptor in ragged batches:
config['ragged_arithmetic'] = 'module' (mdgat_forward_frames_ragged on an fp32 handle - the encoder kernel's bank form - and the ragged plan
of the fp64 handle that runs the encoders alone).

Contracts.  (a) / (b): match_frames_ragged(bank, idx0, idx1, normalize) is bit for bit forward_ragged(ops.assemble_frames_ragged(bank, idx0,
idx1, normalize)) on the same module - every key, every dtype and Z.  (c): a pair's bits do not depend on its position or companions in equal
slots.  (d): the pooled descriptor gives the reference's results to fp32-class rounding.  (e): evaluate_frames_ragged's ground truth is a
float64 module's, its metrics evaluate_ragged's on the assembled chunk.

Against the fp64 reference the split is tests/ragged_decided.py's, the decided pairs written down here and recomputed on the CPU:

    loader chunk (tests/golden/aux_loader.npz), 'FPFH', k = [], seed 1: arg-max margins 3.12e-4, 2.62e-5, 3.43e-4 - pairs 0 and 2 decided
    pooled fixture (tests/golden/desc_gloabal_ragged.npz), k = []: margins 1.2e-2, 8.8e-4, 6.1e-4, 9.0e-3 - all four decided"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import descriptor_ref as DR  # noqa: E402
import ragged_decided as RD  # noqa: E402
import train_ref as T  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from mdgat_matcher_amd import MDGAT, _lib, ops, synth  # noqa: E402
from oracle import mdgat_oracle as O  # noqa: E402
from parity_util import PLAIN_FRAC, PLAIN_MAX, Z_TOL, near_tie_mismatches  # noqa: E402

DEV = 'cuda:0'
ARRAYS = ('keypoints0', 'scores0', 'descriptors0', 'keypoints1', 'scores1', 'descriptors1')
KEYS = ('matches0', 'matches1', 'matching_scores0', 'matching_scores1', 'loss')
SMALL = ((1, 1), (1, 5), (5, 1), (16, 16), (3, 70))
SET_A = ((40, 33), (17, 64), (65, 48))
SET_M = ((130, 256), (200, 130), (512, 384))
LOADER_DECIDED = (0, 2)


def _cfg(L, k, iters=20, descriptor='FPFH', **over):
    return synth.default_config(L=L, k=k, sinkhorn_iterations=iters, descriptor=descriptor, **{'ragged_arithmetic': 'module', **over})


@functools.lru_cache(maxsize=None)
def _net(L=2, k=(), seed=1, dtype=torch.float32, descriptor='FPFH'):
    net = MDGAT(_cfg(L, list(k), descriptor=descriptor)).to(dtype)
    net.load_state_dict(synth.make_state_dict(L=L, seed=seed, descriptor=descriptor))
    net = net.to(dtype).eval().to(DEV)
    assert net.exact() == (dtype == torch.float64) and net._ragged_module() == (dtype == torch.float32)
    return net


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(os.path.join(GOLDEN, 'aux_loader.npz')))


@functools.lru_cache(maxsize=None)
def _loader_chunk():
    """one bank of the fixture's six frames and the chunk of its three pairs (200 x 168, 256 x 256, 97 x 130: slots of 256 x 256)"""
    g = _golden()
    n = int(g['n_items'])
    frames = [g[f'item{j}_rec{f}'] for j in range(n) for f in (0, 1)]
    return ops.pack_frames(frames, DEV), list(range(0, 2 * n, 2)), list(range(1, 2 * n, 2))


def _loader_pairs(device=DEV):
    """the reference loader's per-pair dicts (a leading axis of 1)"""
    g = _golden()
    return [{k: torch.from_numpy(g[f'item{j}_{k}'])[None].to(device) for k in ARRAYS} for j in range(int(g['n_items']))]


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)


def _record(k, s, f):
    return np.concatenate([k, s[:, None], f], axis=1).astype(np.float32)


def _synth_frames(counts):
    """the frames of synth's pairs as float32 records: frame 0 of pair b at 2 b, frame 1 at 2 b + 1"""
    frames = []
    for b, (n, m) in enumerate(counts):
        k0, s0, f0, k1, s1, f1 = synth.make_pair(n, m, b)
        frames += [_record(k0, s0, f0), _record(k1, s1, f1)]
    return frames


def _bank_equals_packed(net, bank, idx0, idx1, normalize, what):
    """contracts (a) and (b); returns the bank call's per-pair dicts"""
    got = net.match_frames_ragged(bank, idx0, idx1, normalize=normalize, return_Z=True)
    ref = net.forward_ragged(ops.assemble_frames_ragged(bank, idx0, idx1, normalize=normalize), return_Z=True)
    assert len(got) == len(idx0) == len(ref)
    for b in range(len(idx0)):
        assert set(got[b]) == set(KEYS) | {'Z'}
        _same(got[b], ref[b], (what, 'normalize', normalize, b))
    return got


# ---------------------------------------------------------------------------------------------------- 1. the smallest shapes
@functools.lru_cache(maxsize=None)
def _small_frames():
    """The frames of SMALL's five pairs in a shuffled bank with spare frames in between (so no start but one is zero and a pair's records
    have strangers directly before and behind them); the one-keypoint frame 0 of pair 0 is also frame 0 of pair 1.  Returns (frames, idx0,
    idx1, spare indices) - host arrays."""
    per_pair = []
    for b, (n, m) in enumerate(SMALL):
        k0, s0, f0, k1, s1, f1 = synth.make_pair(n, m, b)
        per_pair.append((_record(k0, s0, f0), _record(k1, s1, f1)))
    rs = np.random.RandomState(7)
    spare = [rs.standard_normal((r, 37)).astype(np.float32) for r in (9, 33, 2)]
    layout = [('s', 0), (3, 1), (4, 0), (0, 1), ('s', 1), (2, 0), (1, 1), (4, 1), (0, 0), ('s', 2), (3, 0), (2, 1)]      # position -> (pair, side) or a spare
    frames = [spare[i] if p == 's' else per_pair[p][i] for p, i in layout]
    where = {(p, i): pos for pos, (p, i) in enumerate(layout) if p != 's'}
    where[(1, 0)] = where[(0, 0)]
    idx0 = [where[(b, 0)] for b in range(len(SMALL))]
    idx1 = [where[(b, 1)] for b in range(len(SMALL))]
    spares = [pos for pos, (p, _) in enumerate(layout) if p == 's']
    assert [(frames[i].shape[0], frames[j].shape[0]) for i, j in zip(idx0, idx1)] == list(SMALL)
    return frames, idx0, idx1, spares


@pytest.mark.parametrize('descriptor', ['FPFH', 'FPFH_only'])
def test_smallest_shapes_from_a_shuffled_bank(descriptor):
    """slots of 16 x 70, R = 430: two encoder workgroups, mostly padded rows, pair and frame boundaries inside a wave; and the pair (1, 1)
    alone, R = 2: one partial wave with clamped lanes"""
    net = _net(descriptor=descriptor)
    frames, idx0, idx1, _ = _small_frames()
    bank = ops.pack_frames(frames, DEV)
    assert min(int(bank['starts'][i]) for i in idx0[1:] + idx1) > 0
    for normalize in (True, False):
        got = _bank_equals_packed(net, bank, idx0, idx1, normalize, descriptor)
        for b, (n, m) in enumerate(SMALL):
            assert tuple(got[b]['matches0'].shape) == (1, n) and tuple(got[b]['Z'].shape) == (1, n + 1, m + 1) and got[b]['Z'].dtype == torch.float32
            assert got[b]['matching_scores0'].dtype in (torch.float32, torch.int64) and torch.isfinite(got[b]['Z']).all()
        _bank_equals_packed(net, bank, idx0[:1], idx1[:1], normalize, (descriptor, 'the pair (1, 1) alone'))
    net.check(DEV)


# ---------------------------------------------------------------------------------------------------- 2. several workgroups, dynamic layers
@pytest.mark.parametrize('name', ['A', 'M'])
def test_several_workgroups_of_real_rows_and_dynamic_layers(name):
    counts, L, k, subsets = {'A': (SET_A, 2, (8, None, 8, None), ([2, 0, 1], [2, 1])), 'M': (SET_M, 1, (64, None), ([2, 0, 1], [1, 2], [2, 0]))}[name]
    net = _net(L, k)
    bank = ops.pack_frames(_synth_frames(counts), DEV)
    idx0, idx1 = [0, 2, 4], [1, 3, 5]
    ref = _bank_equals_packed(net, bank, idx0, idx1, True, name)
    _bank_equals_packed(net, bank, idx0, idx1, False, name)
    # (c) the chunk permuted, and pairs next to the one(s) that set the slots: the same slots, the same bits per pair
    for order in subsets:
        got = net.match_frames_ragged(bank, [idx0[i] for i in order], [idx1[i] for i in order], return_Z=True)
        for i, p in enumerate(order):
            _same(got[i], ref[p], (name, order, p))
    net.check(DEV)


# ---------------------------------------------------------------------------------------------------- 3. nothing outside a pair is read
@pytest.mark.parametrize('poison', [float('nan'), 1e30])
def test_records_outside_the_chunk_are_never_read(poison):
    net = _net()
    frames, idx0, idx1, spares = _small_frames()
    clean = ops.pack_frames(frames, DEV)
    ref = net.match_frames_ragged(clean, idx0, idx1, return_Z=True)
    starts, counts = clean['starts'].tolist(), clean['counts'].tolist()
    spare = dict(clean)
    rec = clean['records'].clone()
    for s in spares:                                       # every record no pair points at - rows directly before and behind pairs' own among them
        rec[starts[s]:starts[s] + counts[s]] = poison
    rec[starts[spares[1]] + 3] = 1.0
    rec[starts[spares[1]] + 3, 4:] = 0                     # ... and an all-zero FPFH row
    spare['records'] = rec
    used = set(idx0) | set(idx1)
    assert sorted(used | set(spares)) == list(range(len(frames))) and all(s - 1 in used or s + 1 in used for s in spares)
    got = net.match_frames_ragged(spare, idx0, idx1, return_Z=True)
    net.check(DEV)                                         # the guard is not raised
    for b in range(len(SMALL)):
        _same(got[b], ref[b], b)
    if poison != poison:
        # the same poison in a record a pair uses, and an all-zero FPFH row there: refused by the guard, and the next clean call works
        def poisoned(frame, row, what):
            bank = dict(clean)
            r = clean['records'].clone()
            if what == 'nan':
                r[starts[frame] + row, 20] = float('nan')
            else:
                r[starts[frame] + row, 4:] = 0
            bank['records'] = r
            return bank
        for frame, row, what in ((idx1[4], 69, 'nan'), (idx0[3], 0, 'zero_row'), (idx0[0], 0, 'nan')):
            with pytest.raises(RuntimeError):
                net.match_frames_ragged(poisoned(frame, row, what), idx0, idx1)
            again = net.match_frames_ragged(clean, idx0, idx1, return_Z=True)
            net.check(DEV)
            for b in range(len(SMALL)):
                _same(again[b], ref[b], (what, b))
        # (without the normalisation an all-zero FPFH row is a row like any other)
        net.match_frames_ragged(poisoned(idx0[3], 0, 'zero_row'), idx0, idx1, normalize=False)
    net.check(DEV)


# ---------------------------------------------------------------------------------------------------- 4. the reference loader's records
def _check_pair(out, ref, ref_Z, decided, what):
    """one pair of a ragged call against the fp64 reference on the pair alone, by the split of tests/ragged_decided.py"""
    m0, m1 = out['matches0'].cpu(), out['matches1'].cpu()
    Z = out['Z'].cpu().double()
    ref_m0, ref_m1 = (torch.as_tensor(np.asarray(ref[k])).long().reshape(m.shape) for k, m in (('matches0', m0), ('matches1', m1)))
    err = (Z - torch.as_tensor(np.asarray(ref_Z)).double().reshape(Z.shape)).abs()
    es = [(out[k].cpu().double() - torch.as_tensor(np.asarray(ref[k])).double().reshape(out[k].shape)).abs() for k in ('matching_scores0', 'matching_scores1')]
    same = [m0 == ref_m0, m1 == ref_m1]
    worst_s = max([float(e[s].max()) for e, s in zip(es, same) if s.any()] + [0.0])
    print(f'{what}: decided {decided}; max |Z - reference| = {float(err.max()):.3e}, entries beyond 1e-4 {float((err > Z_TOL).double().mean()):.2e}, '
          f'scores {worst_s:.3e}, matches differing {int((~same[0]).sum() + (~same[1]).sum())}')
    if decided:
        assert same[0].all() and same[1].all(), what
        assert float(err.max()) < Z_TOL and worst_s < Z_TOL, (what, float(err.max()), worst_s)
        return
    assert float(err.max()) < PLAIN_MAX and float((err > Z_TOL).double().mean()) < PLAIN_FRAC, (what, float(err.max()))
    assert worst_s < PLAIN_MAX, (what, worst_s)
    near_tie_mismatches(out['Z'], out['matches0'], out['matches1'], ref_m0.numpy(), ref_m1.numpy(), tol=Z_TOL)


def test_from_the_reference_loaders_records_to_the_matches():
    net = _net()
    bank, idx0, idx1 = _loader_chunk()
    got = _bank_equals_packed(net, bank, idx0, idx1, True, 'loader')
    # the yardstick of the bits: the reference loader's own arrays
    ref = net.forward_ragged(_loader_pairs(), return_Z=True)
    for j in range(3):
        _same(got[j], ref[j], ('the loader\'s arrays', j))
    # ... and of the values: the oracle on every pair alone
    sd, cfg = synth.make_state_dict(L=2, seed=1), _cfg(2, [])
    oracle = [RD.oracle_pair(sd, cfg, p) for p in _loader_pairs('cpu')]
    print([(f'{gap:.2e}', f'{margin:.2e}') for _, _, gap, margin in oracle])
    assert tuple(j for j, (_, _, gap, margin) in enumerate(oracle) if RD.decided(gap, margin)) == LOADER_DECIDED
    for j, (out, cap, _, _) in enumerate(oracle):
        _check_pair(got[j], out, cap['Z'], j in LOADER_DECIDED, f'loader pair {j}')
    # the fixture's other net (dynamic layers; no pair of it is decided): the bits alone
    other = _net(2, (32, None, 16, None), 4)
    _bank_equals_packed(other, bank, idx0, idx1, True, 'loader, seed 4')
    net.check(DEV), other.check(DEV)


# ---------------------------------------------------------------------------------------------------- 5. the pooled descriptor
def _margin(Z):
    """the smallest margin between the two best candidates of any arg-max of the extraction (ragged_decided.oracle_pair's)"""
    Z = torch.as_tensor(Z).double()
    n, m = Z.shape[0] - 1, Z.shape[1] - 1
    out = float('inf')
    if m >= 1:
        r = Z[:n].topk(2, dim=1).values
        out = min(out, float((r[:, 0] - r[:, 1]).min()))
    if n >= 1:
        c = Z[:, :m].topk(2, dim=0).values
        out = min(out, float((c[0] - c[1]).min()))
    return out


def test_the_pooled_descriptor_against_the_reference():
    g = dict(np.load(T.golden_path(GOLDEN, DR.RAGGED_FILE)))
    net = MDGAT(DR.config('gap_loss', 'FPFH_gloabal', k=[], ragged_arithmetic='module')).to(torch.float32)
    net.load_state_dict(DR.initial_state('FPFH_gloabal'))
    net = net.to(torch.float32).to(DEV).eval()
    assert not net.exact() and net._handle_f64() and net._ragged_module()
    nb = len(DR.RAGGED_COUNTS)
    margins = [_margin(g[f'p{i}:Z'][0]) for i in range(nb)]
    print('margins', [f'{x:.2e}' for x in margins])
    assert min(margins) >= Z_TOL                           # no dynamic layer and every arg-max decided: all four pairs are decided
    assert int(g['visible'][g['visible'] >= 0].min()) >= 8          # a pool over the padded rows would change at least 8 channels per short frame
    pairs = [{k: torch.from_numpy(g[f'p{i}:in:{k}'].copy()).float().to(DEV) for k in ARRAYS} for i in range(nb)]
    assert [(p['keypoints0'].shape[1], p['keypoints1'].shape[1]) for p in pairs] == list(DR.RAGGED_COUNTS)
    got = net.forward_ragged(pairs, return_Z=True)
    for i, o in enumerate(got):
        assert o['Z'].dtype == torch.float32 and o['matching_scores0'].dtype == torch.float32
        ref = {'matches0': g[f'p{i}:matches0'], 'matches1': g[f'p{i}:matches1'], 'matching_scores0': g[f'p{i}:mscores0'], 'matching_scores1': g[f'p{i}:mscores1']}
        _check_pair(o, ref, g[f'p{i}:Z'], True, f'pooled pair {i} {DR.RAGGED_COUNTS[i]}')
    # (b) out of a bank of float32 records built from the same inputs
    frames = []
    for p in pairs:
        frames += [torch.cat([p[f'keypoints{f}'][0], p[f'scores{f}'][0, :, None], p[f'descriptors{f}'][0]], dim=1).cpu() for f in (0, 1)]
    bank = ops.pack_frames(frames, DEV)
    idx0, idx1 = list(range(0, 2 * nb, 2)), list(range(1, 2 * nb, 2))
    via_bank = _bank_equals_packed(net, bank, idx0, idx1, False, 'pooled')
    for i in range(nb):
        _same(via_bank[i], got[i], ('the pairs themselves', i))
    net.check(DEV)


def test_the_pooled_descriptor_with_dynamic_layers():
    """The oracle has no pooled encoder: the yardstick is a float64 module's forward_ragged (held to the reference by
    tests/test_gpu_descriptors.py), with the bounds for pairs that may hold flipped near ties."""
    net, net64 = _net(2, (8, None, 8, None), descriptor='FPFH_gloabal'), _net(2, (8, None, 8, None), dtype=torch.float64, descriptor='FPFH_gloabal')
    assert net._handle_f64() and not net.exact() and net64.exact()
    pairs = [{k: v.to(DEV) for k, v in synth.make_batch(1, n, m, first_pair=b).items()} for b, (n, m) in enumerate(SET_A)]
    got = net.forward_ragged(pairs, return_Z=True)
    # (c)
    for order in ([2, 0, 1], [2, 1]):
        moved = net.forward_ragged(ops.pack_ragged([pairs[i] for i in order]), return_Z=True)
        for i, p in enumerate(order):
            _same(moved[i], got[p], (order, p))
    # (b)
    bank = ops.pack_frames(_synth_frames(SET_A), DEV)
    _bank_equals_packed(net, bank, [0, 2, 4], [1, 3, 5], True, 'pooled, dynamic')
    ref = net64.forward_ragged(pairs, return_Z=True)
    for b, (o, r) in enumerate(zip(got, ref)):
        assert tuple(o['Z'].shape) == (1, SET_A[b][0] + 1, SET_A[b][1] + 1)
        _check_pair(o, {k: r[k].cpu() for k in KEYS[:4]}, r['Z'].cpu(), False, f'pooled, dynamic, pair {b}')
    net.check(DEV), net64.check(DEV)


# ---------------------------------------------------------------------------------------------------- 6. the evaluation
def _loader_poses():
    g = _golden()
    tr = [O.frame_transforms(g[f'item{j}_pose0'], g[f'item{j}_pose1'], g['T_cam0_velo']) for j in range(3)]
    return tuple(torch.from_numpy(np.stack([t[i] for t in tr])) for i in range(3))


@pytest.mark.parametrize('mutual', [False, True])
def test_evaluate_frames_ragged_on_a_float32_module(mutual):
    g = _golden()
    net, net64 = _net(), _net(dtype=torch.float64)
    bank, idx0, idx1 = _loader_chunk()
    prefix = 'mutual_' if mutual else ''
    T0, T1, T_gt = _loader_poses()
    opts = dict(T_gt=T_gt, gt_threshold=float(g['threshold']), gt_mutual=mutual)
    got = net.evaluate_frames_ragged(bank, idx0, idx1, T0, T1, **opts)
    exact = net64.evaluate_frames_ragged(bank, idx0, idx1, T0, T1, **opts)
    assert set(got) == {'pairs', 'metrics', 'T', 'gt_matches0', 'gt_matches1', 'rep'}
    for k in ('gt_matches0', 'gt_matches1', 'rep'):        # they depend on the keypoints only
        assert got[k].dtype == exact[k].dtype and torch.equal(got[k], exact[k]), k
    for j in range(3):
        for f in '01':
            want = g[f'item{j}_{prefix}gt_matches{f}'].astype(np.int64)
            have = got[f'gt_matches{f}'][j].cpu().numpy()
            assert np.array_equal(have[:len(want)], want) and (have[len(want):] == -1).all(), (j, f)
        assert int(got['rep'][j]) == int(g[f'item{j}_{prefix}rep']), j
    packed = dict(ops.assemble_frames_ragged(bank, idx0, idx1), gt_matches0=got['gt_matches0'], gt_matches1=got['gt_matches1'], T_gt=T_gt.to(DEV))
    ref = net.evaluate_ragged(packed)
    assert got['metrics'].cpu().numpy().tobytes() == ref['metrics'].cpu().numpy().tobytes()
    assert got['T'].cpu().numpy().tobytes() == ref['T'].cpu().numpy().tobytes()
    for j in range(3):
        _same(got['pairs'][j], ref['pairs'][j], j)
    assert ops.EvalMeter().update(got).registration().keys() == ops.EvalMeter().update(ref).registration().keys()
    net.check(DEV), net64.check(DEV)


def test_fpfh_only_takes_its_true_keypoints_from_the_bank():
    g = _golden()
    net = _net(descriptor='FPFH_only')
    bank, idx0, idx1 = _loader_chunk()
    T0, T1, T_gt = _loader_poses()
    opts = dict(T_gt=T_gt, gt_threshold=float(g['threshold']))
    ref = net.evaluate_frames_ragged(bank, idx0, idx1, T0, T1, **opts)
    Z = net.match_frames_ragged(bank, idx0, idx1, return_Z=True)
    scaled = dict(bank)
    scaled['records'] = bank['records'].clone()
    scaled['records'][:, :3] *= 3
    got = net.evaluate_frames_ragged(scaled, idx0, idx1, T0, T1, **opts)
    Z3 = net.match_frames_ragged(scaled, idx0, idx1, return_Z=True)
    for j in range(3):
        _same(got['pairs'][j], ref['pairs'][j], j)         # no match moves
        _same(Z3[j], Z[j], j)                              # ... and no Z
        for f in '01':                                     # the unscaled bank's ground truth is the fixture's: the true keypoints were read
            want = g[f'item{j}_gt_matches{f}'].astype(np.int64)
            assert np.array_equal(ref[f'gt_matches{f}'][j].cpu().numpy()[:len(want)], want), (j, f)
    a = ops.assemble_frames_ragged(scaled, idx0, idx1, normalize=False)
    g0, g1, rep = ops.gt_matches(a['keypoints0_f32'], a['keypoints1_f32'], T0, T1, threshold=float(g['threshold']), counts=a)
    assert torch.equal(got['gt_matches0'], g0) and torch.equal(got['gt_matches1'], g1) and torch.equal(got['rep'], rep)
    assert not torch.equal(got['gt_matches0'], ref['gt_matches0'])          # (the scaled keypoints match differently: the check is not vacuous)
    net.check(DEV)


# ---------------------------------------------------------------------------------------------------- 7. an exact module beside it
def test_an_exact_module_in_the_same_process_keeps_its_bits():
    lib = _lib.load()
    prev = lib.mdgat_set_f64_attention_form(0)
    try:
        net64, net32 = _net(2, (8, None, 8, None), dtype=torch.float64), _net(2, (8, None, 8, None))
        bank = ops.pack_frames(_synth_frames(SET_A), DEV)
        idx0, idx1 = [0, 2, 4], [1, 3, 5]
        alone = net64.match_frames_ragged(bank, idx0, idx1, return_Z=True)
        first = net32.match_frames_ragged(bank, idx0, idx1, return_Z=True)
        between = net64.match_frames_ragged(bank, idx0, idx1, return_Z=True)
        second = net32.match_frames_ragged(bank, idx0, idx1, return_Z=True)
        after = net64.match_frames_ragged(bank, idx0, idx1, return_Z=True)
        for b in range(3):
            _same(between[b], alone[b], b)
            _same(after[b], alone[b], b)
            _same(second[b], first[b], b)
            assert alone[b]['matching_scores0'].dtype == torch.float64 and first[b]['matching_scores0'].dtype == torch.float32
        net64.check(DEV), net32.check(DEV)
    finally:
        lib.mdgat_set_f64_attention_form(prev)


# ---------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_on_the_device():
    net = _net(2, (32, None, 16, None), 4)
    rs = np.random.RandomState(3)
    frames = [rs.standard_normal((n, 37)).astype(np.float32) for n in (513, 40, 20, 64)]
    bank = ops.pack_frames(frames, DEV)
    f16 = MDGAT(_cfg(2, [32, None, 16, None], attention_dtype='f16')).float().eval().to(DEV)
    with pytest.raises(NotImplementedError, match="attention_dtype='fp32'"):
        f16.match_frames_ragged(bank, [3], [1])
    with pytest.raises(ValueError, match='pair 1 has 513 x 40 keypoints: ragged batches hold at most 512 per frame'):
        net.match_frames_ragged(bank, [3, 0], [1, 1])
    with pytest.raises(ValueError, match='pair 0 has 40 x 20 keypoints: fewer than a dynamic layer keeps'):
        net.match_frames_ragged(bank, [1], [2])
    # a start beyond the bank, at the C entry on the fp32 handle: refused on the host copies before anything is enqueued, naming the pair
    lib = _lib.load()
    counts, starts = ops.frames_chunk(bank, [3, 1], [1, 3])
    R = int(bank['records'].shape[0])
    bad1 = starts[1].clone()
    bad1[1] = R - int(counts[1][1]) + 1                    # its last record lies one row past the bank's end
    args, dc, ds = ops._frames_args(bank, counts, (starts[0], bad1))
    B, Np, Mp = 2, 64, 64
    st = net._state_for(torch.device(DEV))
    assert not st.f64
    m0, m1 = (torch.full((B, P), -7, dtype=torch.int64, device=DEV) for P in (Np, Mp))
    s0, s1 = (torch.full((B, P), -7.0, dtype=torch.float32, device=DEV) for P in (Np, Mp))
    with torch.cuda.device(DEV):
        ws = torch.empty(lib.mdgat_workspace_bytes(st.handle, B, Np, Mp), dtype=torch.uint8, device=DEV)
        rc = lib.mdgat_forward_frames_ragged(st.handle, B, Np, Mp, *args, 1, m0.data_ptr(), m1.data_ptr(), s0.data_ptr(), s1.data_ptr(), None, None, None,
                                             ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.ERR_BAD_ARG and 'pair 1' in _lib.last_error() and 'outside the bank' in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    assert (m0 == -7).all() and (m1 == -7).all() and (s0 == -7).all() and (s1 == -7).all()          # nothing was launched
    assert len(net.match_frames_ragged(bank, [3, 1], [1, 3])) == 2          # (and the module still runs)
    net.check(DEV)
