"""Ragged chunks straight from raw frame records: ops.pack_frames / assemble_frames_ragged / gt_matches(counts=) and
MDGAT.match_frames_ragged / evaluate_frames_ragged.  The yardsticks are the reference loader's own outputs (tests/golden/aux_loader.npz),
the paths that existed before (forward_ragged on the loader's arrays, match_frames on each pair alone, evaluate_ragged) - bit for bit, with
the attention form pinned as in tests/test_gpu_ragged_forward.py - and the CPU oracle for the ground-truth matcher."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mdgat_matcher_amd import MDGAT, _lib, ops, synth  # noqa: E402
from oracle import mdgat_oracle as O  # noqa: E402

DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ARRAYS = ('keypoints0', 'scores0', 'descriptors0', 'keypoints1', 'scores1', 'descriptors1')
KEYS = ('matches0', 'matches1', 'matching_scores0', 'matching_scores1', 'loss')
SMALL = ((1, 1), (1, 5), (5, 1), (16, 16), (3, 70))


@pytest.fixture(autouse=True)
def _pinned_attention_form():
    lib = _lib.load()
    prev = lib.mdgat_set_f64_attention_form(0)
    yield
    lib.mdgat_set_f64_attention_form(prev)


def _make_net(L, k, iters, seed, dtype=torch.float64, descriptor='FPFH'):
    cfg = synth.default_config(L=L, k=k, sinkhorn_iterations=iters, descriptor=descriptor)
    net = MDGAT(cfg).to(dtype)
    net.load_state_dict(synth.make_state_dict(L=L, seed=seed, descriptor=descriptor))
    return net.to(dtype).eval().to(DEV)


@functools.lru_cache(maxsize=None)
def _loader_net():
    """the net of test_f64_records_in_equal_the_reference_loaders_arrays"""
    return _make_net(2, [32, None, 16, None], 20, 4)


@functools.lru_cache(maxsize=None)
def _small_net():
    return _make_net(2, [], 20, 1)


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


def _loader_pairs(prefix=''):
    """the reference loader's per-pair dicts (a leading axis of 1), on the device"""
    g = _golden()
    return [{k: torch.from_numpy(g[f'item{j}_{prefix}{k}'])[None].to(DEV) for k in ARRAYS} for j in range(int(g['n_items']))]


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)


def _same_as_tuple(d, tup, what):
    """a per-pair dict of match_frames_ragged (with Z) against match_frames' tuple for the pair alone (a leading axis of 1)"""
    m0, m1, s0, s1, Z = tup
    assert torch.equal(d['matches0'], m0) and torch.equal(d['matches1'], m1), what
    # (a pair that matched nothing carries INTEGER zeros in the dict; the kernels zeroed the float scores too)
    assert torch.equal(d['matching_scores0'].double(), s0.double()) and torch.equal(d['matching_scores1'].double(), s1.double()), what
    assert torch.equal(d['Z'], Z), what


# ---------------------------------------------------------------------------------------------------- 1. the reference loader's outputs
def test_assemble_frames_ragged_equals_the_reference_loaders_arrays():
    g = _golden()
    bank, idx0, idx1 = _loader_chunk()
    a = ops.assemble_frames_ragged(bank, idx0, idx1)
    assert tuple(a['keypoints0'].shape) == (3, 256, 3) and tuple(a['descriptors1'].shape) == (3, 256, 33) and tuple(a['scores0'].shape) == (3, 256)
    assert int(a['range_violation'].item()) == 0
    for j in range(3):
        for f in '01':
            n = int(g[f'item{j}_rec{f}'].shape[0])
            assert int(a[f'counts{f}_host'][j]) == n and int(a[f'counts{f}'][j]) == n
            for key in ('keypoints', 'scores', 'descriptors'):
                got = a[key + f][j]
                assert got.dtype == torch.float64
                assert _bits(got[:n]) == g[f'item{j}_{key}{f}'].tobytes(), (j, key + f)
                assert not np.frombuffer(_bits(got[n:]), dtype=np.uint8).any(), (j, key + f, 'beyond the counts')
            kp = a[f'keypoints{f}_f32'][j]
            assert kp.dtype == torch.float32 and _bits(kp[:n]) == np.ascontiguousarray(g[f'item{j}_rec{f}'][:, :3]).tobytes()
            assert not np.frombuffer(_bits(kp[n:]), dtype=np.uint8).any()
    # normalisation off: the records' own FPFH rows, widened
    raw = ops.assemble_frames_ragged(bank, idx0, idx1, normalize=False)
    assert _bits(raw['descriptors1'][2, :130]) == g['item2_rec1'][:, 4:].astype(np.float64).tobytes()


# ---------------------------------------------------------------------------------------------------- 2. against the existing paths
def test_match_frames_ragged_equals_forward_ragged_and_match_frames():
    g = _golden()
    net = _loader_net()
    bank, idx0, idx1 = _loader_chunk()
    got = net.match_frames_ragged(bank, idx0, idx1, return_Z=True)
    ref = net.forward_ragged(_loader_pairs(), return_Z=True)
    assert len(got) == 3
    for j in range(3):
        assert set(got[j]) == set(KEYS) | {'Z'}
        _same(got[j], ref[j], ('forward_ragged', j))
        r0, r1 = (torch.from_numpy(g[f'item{j}_rec{f}'])[None].to(DEV) for f in (0, 1))
        _same_as_tuple(got[j], net.match_frames(r0, r1, return_scores=True), ('match_frames', j))
    net.check(DEV)


# ---------------------------------------------------------------------------------------------------- 3. the evaluation, end to end
@pytest.mark.parametrize('mutual', [False, True])
def test_evaluate_frames_ragged_equals_the_reference_and_evaluate_ragged(mutual):
    g = _golden()
    net = _loader_net()
    bank, idx0, idx1 = _loader_chunk()
    prefix = 'mutual_' if mutual else ''
    tr = [O.frame_transforms(g[f'item{j}_pose0'], g[f'item{j}_pose1'], g['T_cam0_velo']) for j in range(3)]
    T0, T1, T_gt = (torch.from_numpy(np.stack([t[i] for t in tr])) for i in range(3))
    got = net.evaluate_frames_ragged(bank, idx0, idx1, T0, T1, T_gt=T_gt, gt_threshold=float(g['threshold']), gt_mutual=mutual)
    assert set(got) == {'pairs', 'metrics', 'T', 'gt_matches0', 'gt_matches1', 'rep'}
    assert tuple(got['gt_matches0'].shape) == (3, 256) and tuple(got['gt_matches1'].shape) == (3, 256) and got['gt_matches0'].dtype == torch.int64
    pairs = _loader_pairs(prefix)
    for j, p in enumerate(pairs):
        for f in '01':
            want = g[f'item{j}_{prefix}gt_matches{f}'].astype(np.int64)
            have = got[f'gt_matches{f}'][j].cpu().numpy()
            assert np.array_equal(have[:len(want)], want), (j, f)
            assert (have[len(want):] == -1).all(), (j, f)
            p[f'gt_matches{f}'] = torch.from_numpy(want)[None].to(DEV)
        assert int(got['rep'][j]) == int(g[f'item{j}_{prefix}rep']), j
        p['T_gt'] = T_gt[j:j + 1].to(DEV)
    ref = net.evaluate_ragged(pairs)
    assert _bits(got['metrics']) == _bits(ref['metrics']) and _bits(got['T']) == _bits(ref['T'])
    for j in range(3):
        _same(got['pairs'][j], ref['pairs'][j], j)
    a, b = ops.EvalMeter().update(got), ops.EvalMeter().update(ref)
    assert a.registration().keys() == b.registration().keys()


# ---------------------------------------------------------------------------------------------------- 4. the smallest shapes
def _record(k, s, f):
    return np.concatenate([k, s[:, None], f], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _small_frames():
    """The frames of SMALL's five pairs in a shuffled bank with spare frames in between; the one-keypoint frame 0 of pair 0 is also
    frame 0 of pair 1.  Returns (frames, idx0, idx1, spare indices) - host arrays."""
    per_pair = []
    for b, (n, m) in enumerate(SMALL):
        k0, s0, f0, k1, s1, f1 = synth.make_pair(n, m, b)
        per_pair.append((_record(k0, s0, f0), _record(k1, s1, f1)))
    rs = np.random.RandomState(7)
    spare = [rs.standard_normal((r, 37)).astype(np.float32) for r in (9, 33, 2)]
    # position in the bank -> frame: (pair, side), or a spare
    layout = [('s', 0), (3, 1), (4, 0), (0, 1), ('s', 1), (2, 0), (1, 1), (4, 1), (0, 0), ('s', 2), (3, 0), (2, 1)]
    frames = [spare[i] if p == 's' else per_pair[p][i] for p, i in layout]
    where = {(p, i): pos for pos, (p, i) in enumerate(layout) if p != 's'}
    where[(1, 0)] = where[(0, 0)]
    idx0 = [where[(b, 0)] for b in range(len(SMALL))]
    idx1 = [where[(b, 1)] for b in range(len(SMALL))]
    spares = [pos for pos, (p, _) in enumerate(layout) if p == 's']
    assert [(frames[i].shape[0], frames[j].shape[0]) for i, j in zip(idx0, idx1)] == list(SMALL)
    return frames, idx0, idx1, spares


def test_match_frames_ragged_smallest_shapes_from_a_shuffled_bank():
    net = _small_net()
    frames, idx0, idx1, _ = _small_frames()
    bank = ops.pack_frames(frames, DEV)
    got = net.match_frames_ragged(bank, idx0, idx1, return_Z=True)
    for b, (i, j) in enumerate(zip(idx0, idx1)):
        r0, r1 = torch.from_numpy(frames[i])[None].to(DEV), torch.from_numpy(frames[j])[None].to(DEV)
        _same_as_tuple(got[b], net.match_frames(r0, r1, return_scores=True), ('match_frames', b))
        alone = net.match_frames_ragged(bank, [i], [j], return_Z=True)[0]
        _same(got[b], alone, ('alone', b))
        assert tuple(got[b]['matches0'].shape) == (1, SMALL[b][0]) and tuple(got[b]['Z'].shape) == (1, SMALL[b][0] + 1, SMALL[b][1] + 1)
    net.check(DEV)


@pytest.mark.parametrize('mutual', [False, True])
def test_gt_matches_with_counts_equals_the_oracle_per_pair(mutual):
    """SMALL plus 300 x 257: rows beyond one stride of the kernel's 256 threads.  The keypoints beyond a pair's counts are NaN: not read."""
    counts = SMALL + ((300, 257),)
    B, Np, Mp = len(counts), max(n for n, _ in counts), max(m for _, m in counts)
    rs = np.random.RandomState(11)
    k0 = np.full((B, Np, 3), np.nan, dtype=np.float32)
    k1 = np.full((B, Mp, 3), np.nan, dtype=np.float32)
    T0, T1 = np.tile(np.eye(4), (B, 1, 1)), np.tile(np.eye(4), (B, 1, 1))
    for b, (n, m) in enumerate(counts):
        k0[b, :n] = rs.uniform(-3, 3, (n, 3))
        k1[b, :m] = rs.uniform(-3, 3, (m, 3))
        for T in (T0, T1):
            th = 0.3 * rs.standard_normal()
            T[b, :3, :3] = [[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]
            T[b, :3, 3] = 0.5 * rs.standard_normal(3)
    d0, d1 = torch.from_numpy(k0).to(DEV), torch.from_numpy(k1).to(DEV)
    cases = [(torch.from_numpy(T0), torch.from_numpy(T1))] + ([(None, None)] if not mutual else [])      # identity transforms once
    for t0, t1 in cases:
        g0, g1, rep = ops.gt_matches(d0, d1, t0, t1, threshold=1.0, mutual=mutual, counts=([n for n, _ in counts], [m for _, m in counts]))
        assert tuple(g0.shape) == (B, Np) and tuple(g1.shape) == (B, Mp)
        g0, g1, rep = g0.cpu().numpy(), g1.cpu().numpy(), rep.cpu().numpy()
        for b, (n, m) in enumerate(counts):
            w0, w1, wr = O.gt_matches(k0[b, :n], k1[b, :m], None if t0 is None else T0[b], None if t1 is None else T1[b], threshold=1.0,
                                      mutual=mutual)
            assert np.array_equal(g0[b, :n], w0) and np.array_equal(g1[b, :m], w1) and int(rep[b]) == wr, (b, mutual)
            assert (g0[b, n:] == -1).all() and (g1[b, m:] == -1).all(), b
    assert (g0[5] >= 0).sum() > 0          # (the cases are not vacuous: the large pair has matches)


# ---------------------------------------------------------------------------------------------------- 5. nothing outside a pair is read
def test_records_outside_the_chunk_are_never_read():
    net = _small_net()
    frames, idx0, idx1, spares = _small_frames()
    clean = ops.pack_frames(frames, DEV)
    ref = net.match_frames_ragged(clean, idx0, idx1, return_Z=True)
    starts, counts = clean['starts'].tolist(), clean['counts'].tolist()

    def poisoned(frame, row, what):
        bank = dict(clean)
        rec = clean['records'].clone()
        r = starts[frame] + row
        if what == 'nan':
            rec[r, 20] = float('nan')
        elif what == 'all_nan':
            rec[starts[frame]:starts[frame] + counts[frame]] = float('nan')
        else:
            rec[r, 4:] = 0
        bank['records'] = rec
        return bank

    spare = dict(clean)
    rec = clean['records'].clone()
    for s in spares:
        rec[starts[s]:starts[s] + counts[s]] = float('nan')
    rec[starts[spares[1]] + 3] = 1.0
    rec[starts[spares[1]] + 3, 4:] = 0                     # an all-zero FPFH row in a frame no pair points at
    spare['records'] = rec
    got = net.match_frames_ragged(spare, idx0, idx1, return_Z=True)
    net.check(DEV)
    for b in range(len(SMALL)):
        _same(got[b], ref[b], b)
    # the same poison in a frame a pair uses: refused, and the next clean call works
    for frame, row, what in ((idx1[4], 69, 'nan'), (idx0[3], 0, 'zero_row'), (idx0[0], 0, 'nan')):
        with pytest.raises(RuntimeError):
            net.match_frames_ragged(poisoned(frame, row, what), idx0, idx1)
        again = net.match_frames_ragged(clean, idx0, idx1, return_Z=True)
        net.check(DEV)
        for b in range(len(SMALL)):
            _same(again[b], ref[b], (what, b))
    # the assemble entry's own guard word
    assert int(ops.assemble_frames_ragged(spare, idx0, idx1)['range_violation'].item()) == 0
    assert int(ops.assemble_frames_ragged(poisoned(idx0[3], 15, 'zero_row'), idx0, idx1)['range_violation'].item()) == 1
    assert int(ops.assemble_frames_ragged(poisoned(idx0[3], 15, 'zero_row'), idx0, idx1, normalize=False)['range_violation'].item()) == 0


# ---------------------------------------------------------------------------------------------------- 6. uniform counts
def test_match_frames_ragged_uniform_counts_give_match_frames_bits():
    net = _loader_net()
    data = synth.make_batch(5, 200, 168, device=DEV)
    rec0 = torch.cat([data['keypoints0'], data['scores0'][..., None], data['descriptors0']], -1).float()
    rec1 = torch.cat([data['keypoints1'], data['scores1'][..., None], data['descriptors1']], -1).float()
    bank = ops.pack_frames([r for r in rec0] + [r for r in rec1], DEV)
    got = net.match_frames_ragged(bank, list(range(5)), list(range(5, 10)), return_Z=True)
    whole = net.match_frames(rec0, rec1, return_scores=True)
    for b in range(5):
        _same_as_tuple(got[b], tuple(t[b:b + 1] for t in whole), b)
    net.check(DEV)


# ---------------------------------------------------------------------------------------------------- 7. refusals
def test_frames_ragged_refusals():
    net = _loader_net()
    rs = np.random.RandomState(3)
    frames = [rs.standard_normal((n, 37)).astype(np.float32) for n in (576, 40, 20, 64, 0)]
    bank = ops.pack_frames(frames, DEV)
    with pytest.raises(ValueError, match='pair 1 has 576 x 40 keypoints: ragged batches hold at most 575'):
        net.match_frames_ragged(bank, [3, 0], [1, 1])
    with pytest.raises(ValueError, match='pair 0 has 40 x 20 keypoints: fewer than a dynamic layer keeps'):
        net.match_frames_ragged(bank, [1], [2])
    with pytest.raises(NotImplementedError, match='exact mode only'):
        _make_net(2, [32, None, 16, None], 20, 4, dtype=torch.float32).match_frames_ragged(bank, [3], [1])
    # an empty frame in a chunk: the early-out dict from the matcher, nothing to evaluate
    got = net.match_frames_ragged(bank, [3, 4, 1], [1, 3, 4])
    both = net.match_frames_ragged(bank, [3], [1])[0]
    _same(got[0], both, 'the pair next to the empty ones')
    for b, (n, m) in ((1, (0, 64)), (2, (40, 0))):
        early = net({'keypoints0': torch.zeros(1, n, 3, dtype=torch.float64, device=DEV), 'keypoints1': torch.zeros(1, m, 3, dtype=torch.float64, device=DEV)})
        assert got[b]['skip_train'] is True and early['skip_train'] is True
        _same({k: v for k, v in got[b].items() if k != 'skip_train'}, {k: v for k, v in early.items() if k != 'skip_train'}, ('early-out', b))
    with pytest.raises(ValueError, match='empty frame'):
        net.evaluate_frames_ragged(bank, [3, 4], [1, 3], None, None)
    # a start beyond the bank, at the C entries themselves: refused on the host copies before anything is enqueued, naming the pair
    lib = _lib.load()
    counts, starts = ops.frames_chunk(bank, [3, 1], [1, 3])
    R = int(bank['records'].shape[0])
    bad1 = starts[1].clone()
    bad1[1] = R - int(counts[1][1]) + 1                    # its last record lies one row past the bank's end
    args, dc, ds = ops._frames_args(bank, counts, (starts[0], bad1))
    B, Np, Mp = 2, 64, 64
    st = net._state_for(torch.device(DEV))
    m0, m1 = (torch.full((B, P), -7, dtype=torch.int64, device=DEV) for P in (Np, Mp))
    s0, s1 = (torch.zeros((B, P), dtype=torch.float32, device=DEV) for P in (Np, Mp))
    with torch.cuda.device(DEV):
        ws = torch.empty(lib.mdgat_workspace_bytes(st.handle, B, Np, Mp), dtype=torch.uint8, device=DEV)
        rc = lib.mdgat_forward_frames_ragged(st.handle, B, Np, Mp, *args, 1, m0.data_ptr(), m1.data_ptr(), s0.data_ptr(), s1.data_ptr(), None, None, None,
                                             ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.ERR_BAD_ARG and 'pair 1' in _lib.last_error() and 'outside the bank' in _lib.last_error()
    torch.cuda.synchronize()
    assert (m0 == -7).all() and (m1 == -7).all()          # nothing was launched
    neg0 = starts[0].clone()
    neg0[0] = -1
    args, dc, ds = ops._frames_args(bank, counts, (neg0, starts[1]))
    in4 = torch.zeros((B, Np + Mp, 4), dtype=torch.float64, device=DEV)
    in33 = torch.zeros((B, Np + Mp, 33), dtype=torch.float64, device=DEV)
    with torch.cuda.device(DEV):
        rc = lib.mdgat_assemble_frames_f64_ragged(B, Np, Mp, *args, 1, in4.data_ptr(), in33.data_ptr(), None, None, None,
                                                  torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.ERR_BAD_ARG and 'pair 0' in _lib.last_error()
    net.check(DEV)


# ---------------------------------------------------------------------------------------------------- 8. the other two descriptors
@pytest.mark.parametrize('descriptor', ['FPFH_only', 'FPFH_gloabal'])
def test_match_frames_ragged_with_the_other_descriptors(descriptor):
    net = _make_net(2, [8, None, 8, None], 20, 1, descriptor=descriptor)
    frames = []
    for b, (n, m) in enumerate(((40, 33), (17, 64), (65, 48))):
        k0, s0, f0, k1, s1, f1 = synth.make_pair(n, m, b)
        frames += [_record(k0, s0, f0), _record(k1, s1, f1)]
    bank = ops.pack_frames(frames, DEV)
    idx0, idx1 = [0, 2, 4], [1, 3, 5]
    got = net.match_frames_ragged(bank, idx0, idx1, return_Z=True)
    ref = net.forward_ragged(ops.assemble_frames_ragged(bank, idx0, idx1), return_Z=True)
    for b in range(3):
        _same(got[b], ref[b], (descriptor, b))
    net.check(DEV)
    ev = net.evaluate_frames_ragged(bank, idx0, idx1, None, None, gt_threshold=1.5)
    g0, g1, rep = ops.gt_matches(*(torch.from_numpy(np.stack([np.pad(frames[i][:, :3], ((0, P - len(frames[i])), (0, 0))) for i in idx])).to(DEV)
                                   for idx, P in ((idx0, 65), (idx1, 64))), threshold=1.5, counts=([40, 17, 65], [33, 64, 48]))
    assert torch.equal(ev['gt_matches0'], g0) and torch.equal(ev['gt_matches1'], g1) and torch.equal(ev['rep'], rep)
    for b in range(3):
        _same(ev['pairs'][b], {k: got[b][k] for k in KEYS}, (descriptor, 'evaluate', b))
