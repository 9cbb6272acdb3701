"""MDGAT.forward_ragged / evaluate_ragged: the exact-mode forward on pairs of different sizes in one call of the library.  The yardstick
is net.forward on every pair ALONE (what the evaluation scripts run today): bit for bit, dtypes included, with the attention form pinned
(mdgat_set_f64_attention_form(0): a pair's bits then do not depend on the batch it travels in)."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mdgat_matcher_amd import MDGAT, _lib, ops, synth  # noqa: E402
from parity_util import Z_TOL  # noqa: E402

DEV = 'cuda:0'
F64_TOL = 1e-11
SET_A = ((40, 33), (17, 64), (64, 17), (65, 48), (8, 8), (31, 32), (33, 97))
SET_B = ((530, 100), (100, 540), (575, 575), (64, 64))
SET_C = ((1, 1), (1, 5), (5, 1), (16, 16), (3, 70))
# counts, L, k, Sinkhorn iterations
SETS = {'A': (SET_A, 2, [8, None, 8, None], 20), 'B': (SET_B, 1, [16, None], 10), 'C': (SET_C, 2, [], 20)}
MODES = {0: ('triplet_loss', False), 1: ('triplet_loss', True), 2: ('superglue', False), 3: ('superglue', True)}      # mdgat_extract_mode
KEYS = ('matches0', 'matches1', 'matching_scores0', 'matching_scores1', 'loss')


@pytest.fixture(autouse=True)
def _pinned_attention_form():
    lib = _lib.load()
    prev = lib.mdgat_set_f64_attention_form(0)
    yield
    lib.mdgat_set_f64_attention_form(prev)


@functools.lru_cache(maxsize=None)
def _net(name, mode=0, bin_score=1.0, match_threshold=0.05):
    counts, L, k, iters = SETS[name]
    loss_method, mutual = MODES[mode]
    cfg = synth.default_config(L=L, k=k, sinkhorn_iterations=iters, loss_method=loss_method, mutual_check=mutual, match_threshold=match_threshold)
    net = MDGAT(cfg).double()
    net.load_state_dict(synth.make_state_dict(L=L, seed=1, bin_score=bin_score))
    net = net.eval().to(DEV)
    assert net.exact() and net._extract_mode() == mode
    return net


@functools.lru_cache(maxsize=None)
def _pairs(name):
    """the per-pair dicts of a set as a batch_size=1 loader yields them (a leading axis of 1), on the device"""
    return tuple({k: v.to(DEV) for k, v in synth.make_batch(1, n, m, first_pair=b).items()} for b, (n, m) in enumerate(SETS[name][0]))


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize('mode', [0, 1, 2, 3])
@pytest.mark.parametrize('name', ['A', 'C'])
def test_forward_ragged_equals_forward_on_every_pair_alone(name, mode):
    net, pairs = _net(name, mode), _pairs(name)
    with torch.no_grad():
        got = net.forward_ragged(list(pairs), return_Z=True)
        for b, p in enumerate(pairs):
            alone = net(p)
            Z = net.match(p['keypoints0'], p['descriptors0'], p['keypoints1'], p['descriptors1'], p['scores0'], p['scores1'], return_scores=True)[4]
            assert set(got[b]) == set(KEYS) | {'Z'}
            _same({k: got[b][k] for k in KEYS}, alone, (name, mode, b))
            assert torch.equal(got[b]['Z'], Z), (name, mode, b)
    net.check(DEV)


def test_forward_ragged_against_the_reference_held_pairs(golden_dir):
    """Set A' in one call against tests/golden/ragged_pairs.npz - the reference's own outputs, one pair per call: matches identical in
    every extraction variant the reference runs on the pair; Z within parity_util.Z_TOL; the matching scores within 1e-6, the bound
    tests/test_gpu_f64.py applies to reference-held pairs with the fp64 tail."""
    g = np.load(os.path.join(golden_dir, 'ragged_pairs.npz'))
    pairs = list(_pairs('A')[:5])
    assert [tuple(int(x) for x in r) for r in g['pairs']] == [tuple(c) for c in SET_A[:5]]
    tags = {'default': 0, 'mutual': 1, 'sg': 2, 'sgmutual': 3}
    for tag, mode in tags.items():
        held = [b for b in range(5) if f'p{b}_{tag}_matches0' in g.files]
        with torch.no_grad():
            got = _net('A', mode, 1.0, 0.2).forward_ragged([pairs[b] for b in held], return_Z=True)      # (the fixture's config: the default threshold)
        for o, b in zip(got, held):
            assert np.array_equal(o['matches0'].cpu().numpy(), g[f'p{b}_{tag}_matches0']), (tag, b)
            assert np.array_equal(o['matches1'].cpu().numpy(), g[f'p{b}_{tag}_matches1']), (tag, b)
            es = max(np.abs(o['matching_scores0'].cpu().double().numpy() - g[f'p{b}_{tag}_mscores0']).max(),
                     np.abs(o['matching_scores1'].cpu().double().numpy() - g[f'p{b}_{tag}_mscores1']).max())
            ez = np.abs(o['Z'].cpu().double().numpy() - g[f'p{b}_Z']).max()
            print(f'{tag} pair {b}: max |Z - reference| = {ez:.2e}, scores {es:.2e}')
            assert ez < Z_TOL and es < 1e-6, (tag, b, ez, es)


def test_forward_ragged_applies_the_nothing_matched_rule_per_pair():
    """A bin score of 32 leaves the 8 x 8 pair of set A without a match (the oracle's count; its neighbours keep 1 to 4): that pair alone
    gets the reference's INTEGER zero scores (mdgat.py:464-467), as when it is the only pair of a call."""
    net, pairs = _net('A', 0, 32.0), _pairs('A')
    with torch.no_grad():
        got = net.forward_ragged(list(pairs))
        for b, p in enumerate(pairs):
            _same(got[b], net(p), b)
    kinds = [g['matching_scores0'].dtype for g in got]
    assert kinds[4] == torch.int64 and (got[4]['matches0'] == -1).all() and not got[4]['matching_scores1'].any()
    assert kinds.count(torch.float64) >= 1


def test_forward_ragged_uniform_counts_order_and_packed_input():
    net = _net('A')
    data = synth.make_batch(3, 65, 48, first_pair=2, device=DEV)
    pairs = [{k: v[b:b + 1] for k, v in data.items()} for b in range(3)]
    with torch.no_grad():
        m0, m1, s0, s1, Z = net.match(data['keypoints0'], data['descriptors0'], data['keypoints1'], data['descriptors1'], data['scores0'],
                                      data['scores1'], return_scores=True)
        got = net.forward_ragged(pairs, return_Z=True)
        for b in range(3):          # uniform counts: the bits of the stacked batch
            assert torch.equal(got[b]['matches0'], m0[b:b + 1]) and torch.equal(got[b]['matches1'], m1[b:b + 1])
            assert torch.equal(got[b]['matching_scores0'], s0[b:b + 1].double()) and torch.equal(got[b]['matching_scores1'], s1[b:b + 1].double())
            assert torch.equal(got[b]['Z'], Z[b:b + 1])
        ragged = list(_pairs('A'))
        ref = net.forward_ragged(ragged, return_Z=True)
        perm = [3, 6, 0, 5, 1, 4, 2]
        shuffled = net.forward_ragged(ops.pack_ragged([ragged[i] for i in perm]), return_Z=True)      # (a packed batch as input)
        for i, p in enumerate(perm):
            _same(shuffled[i], ref[p], (i, p))


@pytest.mark.parametrize('poison', [float('nan'), 1e300])
def test_forward_ragged_padding_reaches_nothing(poison):
    """The padded tails of every input hold NaN / 1e300 instead of zeros: the same bits, and no range or finiteness guard trips."""
    net, pairs = _net('A'), list(_pairs('A'))
    packed = ops.pack_ragged(pairs)
    with torch.no_grad():
        ref = net.forward_ragged(packed, return_Z=True)
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


def test_forward_ragged_empty_frame_gets_the_early_out():
    net, pairs = _net('A'), list(_pairs('A'))
    empty = {k: v.clone() for k, v in pairs[2].items()}
    for k in ('keypoints1', 'scores1', 'descriptors1'):
        empty[k] = empty[k][:, :0]
    with torch.no_grad():
        ref = net.forward_ragged(pairs)
        got = net.forward_ragged(pairs[:2] + [empty] + pairs[3:])
        early = net(empty)
    assert got[2]['skip_train'] is True
    _same({k: v for k, v in got[2].items() if k != 'skip_train'}, {k: v for k, v in early.items() if k != 'skip_train'}, 'early-out')
    for b in (0, 1, 3, 4, 5, 6):
        _same(got[b], ref[b], b)


def test_forward_ragged_beyond_512_keys():
    """Set B: the dynamic kernel of more than 512 keys serves the whole batch, the 64 x 64 and the small-frame pairs alone run the other
    instantiation: matches identical, Z within the fp64 kernels' rounding.  The forward hands out the float32 rounding of its fp64 Z: a
    difference of 1e-11 in fp64 moves that rounding by one float32 step at the most - 2e-6 at |Z| < 32 - and 2e-6 is the bound
    tests/test_gpu_f64.py puts on the same output (entries of larger magnitude, up to ~50 here, then have to be identical)."""
    net, pairs = _net('B'), _pairs('B')
    with torch.no_grad():
        got = net.forward_ragged(list(pairs), return_Z=True)
        for b, p in enumerate(pairs):
            m0, m1, s0, s1, Z = net.match(p['keypoints0'], p['descriptors0'], p['keypoints1'], p['descriptors1'], p['scores0'], p['scores1'],
                                          return_scores=True)
            assert torch.equal(got[b]['matches0'], m0) and torch.equal(got[b]['matches1'], m1), b
            err = (got[b]['Z'].double() - Z.double()).abs().max().item()
            print(f'set B pair {b}: max |Z ragged - Z alone| (float32 outputs) = {err:.3e}')
            assert err <= 2e-6, (b, err)
    net.check(DEV)


def test_forward_ragged_default_attention_form():
    """The attention form left to the launch size (the default): the matches are those of the pairs alone."""
    lib = _lib.load()
    net, pairs = _net('A'), _pairs('A')
    prev = lib.mdgat_set_f64_attention_form(-1)
    try:
        with torch.no_grad():
            got = net.forward_ragged(list(pairs))
            for b, p in enumerate(pairs):
                alone = net(p)
                assert torch.equal(got[b]['matches0'], alone['matches0']) and torch.equal(got[b]['matches1'], alone['matches1']), b
    finally:
        lib.mdgat_set_f64_attention_form(prev)


def test_evaluate_ragged_equals_evaluate_on_every_pair_alone():
    net = _net('A')
    pairs = []
    for b, p in enumerate(_pairs('A')):
        rs = np.random.RandomState(100 + b)
        th = 0.05 * rs.standard_normal()
        T = np.eye(4)
        T[:3, :3] = [[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]
        T[:3, 3] = 0.3 * rs.standard_normal(3)
        T = torch.from_numpy(T)[None].to(DEV)
        g0, g1, _ = ops.gt_matches(p['keypoints0'], p['keypoints1'], T1=T, threshold=1.5)
        pairs.append({**p, 'gt_matches0': g0, 'gt_matches1': g1, 'T_gt': T})
    with torch.no_grad():
        got = net.evaluate_ragged(pairs)
        alone = [net.evaluate(p) for p in pairs]
    assert tuple(got['metrics'].shape) == (len(pairs), len(ops.EvalColumns))
    for b, a in enumerate(alone):
        # (bit for bit, NaN columns included: compared as bytes)
        assert got['metrics'][b].cpu().numpy().tobytes() == a['metrics'][0].cpu().numpy().tobytes(), b
        assert got['T'][b].cpu().numpy().tobytes() == a['T'][0].cpu().numpy().tobytes(), b
        _same(got['pairs'][b], {k: a[k] for k in KEYS}, b)
    one, many = ops.EvalMeter(), ops.EvalMeter()
    one.update(got)
    for a in alone:
        many.update(a)
    for x, y in ((one.registration(), many.registration()),):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(np.asarray(x[k], dtype=np.float64), np.asarray(y[k], dtype=np.float64), equal_nan=True), k
    a, b = one.test_py(), many.test_py()
    for k in a:
        if k not in ('fail_rate', 'baned_data_rate'):          # (divided by the number of update calls, which differs by design)
            assert np.array_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64), equal_nan=True), k


def test_forward_ragged_refusals_on_the_device():
    net, pairs = _net('A'), list(_pairs('A'))
    lib = _lib.load()
    prev = lib.mdgat_set_f64_sinkhorn_form(1)
    try:
        with pytest.raises(RuntimeError, match='register-resident'):
            net.forward_ragged(pairs)
    finally:
        lib.mdgat_set_f64_sinkhorn_form(prev)
    cfg = synth.default_config(L=2, k=[8, None, 8, None], sinkhorn_iterations=20, sinkhorn_arithmetic='fp32')
    off = MDGAT(cfg).double()
    off.load_state_dict(synth.make_state_dict(L=2, seed=1))
    off = off.eval().to(DEV)
    with pytest.raises(RuntimeError, match='register-resident'):
        off.forward_ragged(pairs)
