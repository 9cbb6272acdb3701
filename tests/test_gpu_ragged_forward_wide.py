"""MDGAT.forward_ragged and its siblings with config['ragged_sinkhorn'] = 'auto' / 'streaming': the exact-mode forward on pairs of
different sizes of up to 2048 keypoints in one call, the fp64 tail on the STREAMING Sinkhorn with per-pair counts.  The yardstick is
net.forward on every pair ALONE under mdgat_set_f64_sinkhorn_form(1) - bit for bit, dtypes included - with the attention form pinned to 0
as in tests/test_gpu_ragged_forward.py."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mdgat_matcher_amd import MDGAT, _lib, ops, synth  # noqa: E402
from parity_util import Z_TOL  # noqa: E402

DEV = 'cuda:0'
SET_A = ((40, 33), (17, 64), (64, 17), (65, 48), (8, 8), (31, 32), (33, 97))        # tests/test_gpu_ragged_forward.py's
SET_W = ((600, 40), (40, 610), (64, 64), (530, 100))
# X: the dynamic attention's limit.  The small pair is 129 x 129: k = 128 refuses anything smaller (torch.topk raises in the reference), and
# 128 x 128 is the documented exception to bit identity.
SET_X = ((2048, 130), (130, 2048), (129, 129))
# E1 / E2: the first slots the register-resident Sinkhorn does not take with counts - 576 rows (which that kernel holds, but the ragged limit
# is 575 for both frames) and 576 columns (which it does not)
SET_E1 = ((576, 40), (64, 64))
SET_E2 = ((575, 576), (40, 33))
# counts, L, k, Sinkhorn iterations
SETS = {'A': (SET_A, 2, [8, None, 8, None], 20), 'W': (SET_W, 1, [16, None], 10), 'X': (SET_X, 1, [128, None], 3),
        'E1': (SET_E1, 1, [16, None], 10), 'E2': (SET_E2, 1, [16, None], 10)}
MODES = {0: ('triplet_loss', False), 1: ('triplet_loss', True), 2: ('superglue', False), 3: ('superglue', True)}      # mdgat_extract_mode
KEYS = ('matches0', 'matches1', 'matching_scores0', 'matching_scores1', 'loss')


@pytest.fixture(autouse=True)
def _pinned_attention_form():
    lib = _lib.load()
    prev = lib.mdgat_set_f64_attention_form(0)
    yield
    lib.mdgat_set_f64_attention_form(prev)


class _form1:
    """the uniform forward's fp64 Sinkhorn on the streaming form"""
    def __enter__(self):
        self.prev = _lib.load().mdgat_set_f64_sinkhorn_form(1)

    def __exit__(self, *exc):
        _lib.load().mdgat_set_f64_sinkhorn_form(self.prev)


@functools.lru_cache(maxsize=None)
def _net(name, mode=0, ragged_sinkhorn=None, match_threshold=0.05):
    counts, L, k, iters = SETS[name]
    loss_method, mutual = MODES[mode]
    cfg = synth.default_config(L=L, k=k, sinkhorn_iterations=iters, loss_method=loss_method, mutual_check=mutual, match_threshold=match_threshold)
    if ragged_sinkhorn is not None:
        cfg['ragged_sinkhorn'] = ragged_sinkhorn
    net = MDGAT(cfg).double()
    net.load_state_dict(synth.make_state_dict(L=L, seed=1))
    net = net.eval().to(DEV)
    assert net.exact() and net._extract_mode() == mode
    return net


@functools.lru_cache(maxsize=None)
def _pairs(name):
    """the per-pair dicts of a set as a batch_size=1 loader yields them (a leading axis of 1), on the device"""
    return tuple({k: v.to(DEV) for k, v in synth.make_batch(1, n, m, first_pair=b).items()} for b, (n, m) in enumerate(SETS[name][0]))


def _forward_alone(net, p):
    with torch.no_grad():
        out = dict(net(p))
        out['Z'] = net.match(p['keypoints0'], p['descriptors0'], p['keypoints1'], p['descriptors1'], p['scores0'], p['scores1'], return_scores=True)[4]
    return out


@functools.lru_cache(maxsize=None)
def _alone(name, mode=0, form1=True):
    """net.forward and Z of match(..., return_scores=True) on every pair of the set alone - under Sinkhorn form 1, or in the default forms -
    computed once, never modified.  (The module without the key: a uniform call does not look at it.)"""
    net = _net(name, mode)
    if form1:
        with _form1():
            return tuple(_forward_alone(net, p) for p in _pairs(name))
    return tuple(_forward_alone(net, p) for p in _pairs(name))


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


@pytest.mark.parametrize('mode', [0, 1, 2, 3])
def test_streaming_on_set_A_equals_forward_on_every_pair_alone_under_form_1(mode):
    net = _net('A', mode, 'streaming')
    got = net.forward_ragged(list(_pairs('A')), return_Z=True)
    for b, alone in enumerate(_alone('A', mode)):
        assert set(got[b]) == set(KEYS) | {'Z'}
        _same(got[b], alone, ('A', mode, b))
    net.check(DEV)


def test_auto_on_set_A_has_the_bits_of_a_module_without_the_key():
    """slots within 575 keypoints, the form not forced: 'auto' runs the register-resident Sinkhorn as before"""
    pairs = list(_pairs('A'))
    got = _net('A', 0, 'auto').forward_ragged(pairs, return_Z=True)
    ref = _net('A', 0).forward_ragged(pairs, return_Z=True)
    for b in range(len(pairs)):
        _same(got[b], ref[b], b)


def test_auto_on_set_A_under_sinkhorn_form_1_runs_the_streaming_form():
    """'auto' with the form forced to 1: slots within 575 run the streaming form with the counts - the bits of every pair alone under form
    1 - where a module without the key refuses the batch as before"""
    pairs = list(_pairs('A'))
    with _form1():
        got = _net('A', 0, 'auto').forward_ragged(pairs, return_Z=True)
        with pytest.raises(RuntimeError, match='register-resident'):
            _net('A', 0).forward_ragged(pairs)
    for b, alone in enumerate(_alone('A')):
        _same(got[b], alone, ('A', b))


@pytest.mark.parametrize('name', ['E1', 'E2'])
def test_auto_at_the_first_slots_beyond_the_resident_form(name):
    """Slots of 576 x 64 and 575 x 576 as the FIRST call of a module (its workspace is sized by mdgat_workspace_bytes for this very call):
    the workspace holds the streaming form's K, and every pair is bit for bit forward on the pair alone under form 1."""
    counts = SETS[name][0]
    net = _net(name, 0, 'auto')
    Np, Mp = max(n for n, _ in counts), max(m for _, m in counts)
    lib = _lib.load()
    st = net._state_for(torch.device(DEV))
    assert lib.mdgat_workspace_bytes(st.handle, len(counts), Np, Mp) > lib.mdgat_sinkhorn_f64_stream_ragged_workspace_bytes(len(counts), Np, Mp)
    got = net.forward_ragged(list(_pairs(name)), return_Z=True)
    for b, alone in enumerate(_alone(name)):
        _same(got[b], alone, (name, b))
    net.check(DEV)


@functools.lru_cache(maxsize=None)
def _auto_W(mode=0, match_threshold=0.05):
    return tuple(_net('W', mode, 'auto', match_threshold).forward_ragged(list(_pairs('W')), return_Z=True))


def test_auto_on_set_W_equals_forward_on_every_pair_alone():
    """Slots of 600 x 610.  Bit for bit against each pair alone under Sinkhorn form 1; against the pair alone in the default forms (the
    three pairs within 575 x 575 then run the register-resident Sinkhorn: other summation orders) matches identical and Z within
    parity_util.Z_TOL."""
    got = _auto_W()
    for b, alone in enumerate(_alone('W')):
        _same(got[b], alone, ('W', b))
    for b, alone in enumerate(_alone('W', 0, False)):
        assert torch.equal(got[b]['matches0'], alone['matches0']) and torch.equal(got[b]['matches1'], alone['matches1']), b
        err = (got[b]['Z'].double() - alone['Z'].double()).abs().max().item()
        print(f'set W pair {b}: max |Z ragged (streaming) - Z alone (default forms)| (float32 outputs) = {err:.3e}')
        assert err < Z_TOL, (b, err)
    _net('W', 0, 'auto').check(DEV)


def test_auto_on_set_W_against_the_reference_held_pairs(golden_dir):
    """tests/golden/ragged_wide_pairs.npz - the reference's own outputs, one pair per call: matches identical in every extraction variant
    the reference runs on the pair; Z within parity_util.Z_TOL; the matching scores within 1e-6, the bound of
    tests/test_gpu_ragged_forward.py's reference-held test."""
    g = np.load(os.path.join(golden_dir, 'ragged_wide_pairs.npz'))
    assert [tuple(int(x) for x in r) for r in g['pairs']] == [tuple(c) for c in SET_W[:3]]
    tags = {'default': 0, 'mutual': 1, 'sg': 2, 'sgmutual': 3}
    for tag, mode in tags.items():
        got = _auto_W(mode, 0.2)           # (the fixture's config: the default threshold; the whole set in its slots of 600 x 610)
        for b in range(3):
            if f'p{b}_{tag}_matches0' not in g.files:
                continue
            o = got[b]
            assert np.array_equal(o['matches0'].cpu().numpy(), g[f'p{b}_{tag}_matches0']), (tag, b)
            assert np.array_equal(o['matches1'].cpu().numpy(), g[f'p{b}_{tag}_matches1']), (tag, b)
            es = max(np.abs(o['matching_scores0'].cpu().double().numpy() - g[f'p{b}_{tag}_mscores0']).max(),
                     np.abs(o['matching_scores1'].cpu().double().numpy() - g[f'p{b}_{tag}_mscores1']).max())
            ez = np.abs(o['Z'].cpu().double().numpy() - g[f'p{b}_Z']).max()
            print(f'{tag} pair {b}: max |Z - reference| = {ez:.2e}, scores {es:.2e}')
            assert ez < Z_TOL and es < 1e-6, (tag, b, ez, es)


def test_auto_on_set_X_equals_forward_on_every_pair_alone_under_form_1():
    """slots of 2048 x 2048: the limit of the dynamic attention (k = 128 of 2048 keys), 64 row slabs and 17 column chunks of the Sinkhorn"""
    net = _net('X', 0, 'auto')
    got = net.forward_ragged(list(_pairs('X')), return_Z=True)
    for b, alone in enumerate(_alone('X')):
        _same(got[b], alone, ('X', b))
    net.check(DEV)


def _with_gt(pairs):
    out = []
    for b, p in enumerate(pairs):
        rs = np.random.RandomState(100 + b)
        th = 0.05 * rs.standard_normal()
        T = np.eye(4)
        T[:3, :3] = [[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]
        T[:3, 3] = 0.3 * rs.standard_normal(3)
        T = torch.from_numpy(T)[None].to(DEV)
        g0, g1, _ = ops.gt_matches(p['keypoints0'], p['keypoints1'], T1=T, threshold=1.5)
        out.append({**p, 'gt_matches0': g0, 'gt_matches1': g1, 'T_gt': T})
    return out


def test_evaluate_ragged_on_set_W_equals_evaluate_on_every_pair_alone():
    pairs = _with_gt(_pairs('W'))
    with torch.no_grad():
        got = _net('W', 0, 'auto').evaluate_ragged(pairs)
        with _form1():
            alone = [_net('W').evaluate(p) for p in pairs]
    assert tuple(got['metrics'].shape) == (len(pairs), len(ops.EvalColumns))
    for b, a in enumerate(alone):
        assert _bits(got['metrics'][b]) == _bits(a['metrics'][0]) and _bits(got['T'][b]) == _bits(a['T'][0]), b      # (NaN columns included)
        _same(got['pairs'][b], {k: a[k] for k in KEYS}, b)


def _record(k, s, f):
    return np.concatenate([k, s[:, None], f], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _W_bank():
    """set W as raw records: a bank of its eight frames, frame 0 of pair b at 2 b, frame 1 at 2 b + 1"""
    frames = []
    for b, (n, m) in enumerate(SET_W):
        k0, s0, f0, k1, s1, f1 = synth.make_pair(n, m, b)
        frames += [_record(k0, s0, f0), _record(k1, s1, f1)]
    return tuple(frames), ops.pack_frames(frames, DEV), list(range(0, 8, 2)), list(range(1, 8, 2))


def test_match_frames_ragged_on_set_W_equals_match_frames_on_every_pair_alone():
    frames, bank, idx0, idx1 = _W_bank()
    net = _net('W', 0, 'auto')
    got = net.match_frames_ragged(bank, idx0, idx1, return_Z=True)
    for b, (i, j) in enumerate(zip(idx0, idx1)):
        r0, r1 = torch.from_numpy(frames[i])[None].to(DEV), torch.from_numpy(frames[j])[None].to(DEV)
        with _form1():
            m0, m1, s0, s1, Z = _net('W').match_frames(r0, r1, return_scores=True)
        d = got[b]
        assert tuple(d['matches0'].shape) == (1, SET_W[b][0]) and tuple(d['Z'].shape) == (1, SET_W[b][0] + 1, SET_W[b][1] + 1)
        assert torch.equal(d['matches0'], m0) and torch.equal(d['matches1'], m1), b
        assert torch.equal(d['matching_scores0'].double(), s0.double()) and torch.equal(d['matching_scores1'].double(), s1.double()), b
        assert torch.equal(d['Z'], Z), b
    net.check(DEV)


def test_evaluate_frames_ragged_on_set_W_equals_evaluate_ragged_of_the_assembled_chunk():
    _, bank, idx0, idx1 = _W_bank()
    net = _net('W', 0, 'auto')
    B = len(SET_W)
    rs = np.random.RandomState(3)
    T0, T1 = np.tile(np.eye(4), (B, 1, 1)), np.tile(np.eye(4), (B, 1, 1))
    for b in range(B):
        th = 0.05 * rs.standard_normal()
        T1[b, :3, :3] = [[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]
        T1[b, :3, 3] = 0.3 * rs.standard_normal(3)
    T0, T1 = torch.from_numpy(T0), torch.from_numpy(T1)
    T_gt = torch.linalg.inv(T1) @ T0
    got = net.evaluate_frames_ragged(bank, idx0, idx1, T0, T1, T_gt=T_gt, gt_threshold=1.5)
    assert tuple(got['gt_matches0'].shape) == (B, 600) and tuple(got['gt_matches1'].shape) == (B, 610)
    chunk = dict(ops.assemble_frames_ragged(bank, idx0, idx1))
    chunk.update(gt_matches0=got['gt_matches0'], gt_matches1=got['gt_matches1'], T_gt=T_gt.to(DEV))
    ref = net.evaluate_ragged(chunk)
    assert _bits(got['metrics']) == _bits(ref['metrics']) and _bits(got['T']) == _bits(ref['T'])
    for b in range(B):
        _same(got['pairs'][b], ref['pairs'][b], b)
    assert (got['gt_matches0'] >= 0).any()


@pytest.mark.parametrize('poison', [float('nan'), 1e300])
def test_padding_reaches_nothing(poison):
    """The padded tails of every input of set W hold NaN / 1e300 instead of zeros: the same bits, and no range or finiteness guard trips."""
    net, pairs = _net('W', 0, 'auto'), list(_pairs('W'))
    packed = ops.pack_ragged(pairs)
    ref = _auto_W()
    bad = dict(packed)
    for f, cnt in (('0', packed['counts0_host']), ('1', packed['counts1_host'])):
        for key in ('keypoints', 'scores', 'descriptors'):
            t = packed[key + f].clone()
            for b, c in enumerate(cnt.tolist()):
                t[b, c:] = poison
            bad[key + f] = t
    got = net.forward_ragged(bad, return_Z=True)
    net.check(DEV)
    for b in range(len(pairs)):
        _same(got[b], ref[b], b)


def test_refusals():
    """'auto' refuses a frame of 2049 keypoints, naming 2048 - the module before anything touches a device, the library for a caller
    that goes past the module's check; the same module without the key refuses 576 as before."""
    auto, plain = _net('W', 0, 'auto'), _net('W')
    h = lambda n, m: (torch.tensor([n], dtype=torch.int32), torch.tensor([m], dtype=torch.int32))      # noqa: E731
    with pytest.raises(ValueError, match='pair 0 has 2049 x 64 keypoints: ragged batches hold at most 2048 per frame'):
        auto._ragged_counts_checked(*h(2049, 64), 2049, 64)
    with pytest.raises(ValueError, match='pair 0 has 576 x 64 keypoints: ragged batches hold at most 575 per frame'):
        plain._ragged_counts_checked(*h(576, 64), 576, 64)
    big = {k: v.to(DEV) for k, v in synth.make_batch(1, 2049, 64, first_pair=0).items()}
    with pytest.raises(ValueError, match='2048'):
        auto.forward_ragged([big])
    mid = {k: v.to(DEV) for k, v in synth.make_batch(1, 576, 64, first_pair=0).items()}
    with pytest.raises(ValueError, match='575'):
        plain.forward_ragged([mid])
    # the library's own refusal: the module's check stepped over
    packed = ops.pack_ragged([big])
    check = MDGAT._ragged_counts_checked
    try:
        MDGAT._ragged_counts_checked = lambda self, *a: None
        with pytest.raises(RuntimeError, match='at most 2048 keypoints per frame'):
            auto.forward_ragged(packed)
        with pytest.raises(RuntimeError, match='at most 575 keypoints per frame'):
            plain.forward_ragged(ops.pack_ragged([mid]))
    finally:
        MDGAT._ragged_counts_checked = check
