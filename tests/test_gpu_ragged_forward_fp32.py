"""MDGAT.forward_ragged / evaluate_ragged on a float32 module with config['ragged_arithmetic'] = 'auto': the fp32-class forward on pairs
of different sizes in one call of the library (mdgat_forward_ragged).

The yardstick is the fp64 reference on every pair ALONE - the reference's own outputs where tests/golden/ragged_pairs.npz holds them, the
oracle elsewhere - split as tests/ragged_decided.py describes: a DECIDED pair (the oracle's smallest top-k gap >= 4e-5 and its smallest
arg-max margin on Z >= Z_TOL) must give the reference's matches and its Z and scores within Z_TOL; on the others the bounds parity_util
puts on outputs with flipped near ties hold (PLAIN_MAX, PLAIN_FRAC) and a differing match is a near tie by the path's own Z.  Which pairs
are decided is written down here (DECIDED) and checked against the helper on the CPU:

    set A   gaps 6.8e-5, 2.5e-4, 1.0e-5, 5.1e-5, none (8 x 8: k = all keys), 1.6e-4, 2.1e-4; margins >= 9.3e-4: only (64, 17) is undecided
    set C   no dynamic layer, margins >= 1.7e-2: all decided
    mid     gaps 6.5e-6, 5.3e-5, 9.9e-6, 9.9e-6; margins 3.6e-4, 4.0e-4, 2.9e-3, 6.7e-6: (130, 256) is the decided pair"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mdgat_matcher_amd import MDGAT, _lib, ops, synth  # noqa: E402
from parity_util import PLAIN_FRAC, PLAIN_MAX, Z_TOL, near_tie_mismatches  # noqa: E402
import ragged_decided as RD  # noqa: E402

DEV = 'cuda:0'
SET_A = ((40, 33), (17, 64), (64, 17), (65, 48), (8, 8), (31, 32), (33, 97))
SET_C = ((1, 1), (1, 5), (5, 1), (16, 16), (3, 70))
SET_M = ((300, 500), (130, 256), (200, 130), (512, 384))
# counts, L, k, Sinkhorn iterations
SETS = {'A': (SET_A, 2, [8, None, 8, None], 20), 'C': (SET_C, 2, [], 20), 'M': (SET_M, 1, [64, None], 20)}
DECIDED = {'A': (0, 1, 3, 4, 5, 6), 'C': (0, 1, 2, 3, 4), 'M': (1,)}
MODES = {0: ('triplet_loss', False), 1: ('triplet_loss', True), 2: ('superglue', False), 3: ('superglue', True)}      # mdgat_extract_mode
KEYS = ('matches0', 'matches1', 'matching_scores0', 'matching_scores1', 'loss')


def _cfg(name, mode=0, match_threshold=0.2):
    _, L, k, iters = SETS[name]
    loss_method, mutual = MODES[mode]
    return synth.default_config(L=L, k=k, sinkhorn_iterations=iters, loss_method=loss_method, mutual_check=mutual, match_threshold=match_threshold)


@functools.lru_cache(maxsize=None)
def _net(name, mode=0, bin_score=1.0, exact=False):
    net = MDGAT({**_cfg(name, mode), 'ragged_arithmetic': 'auto'})
    net.load_state_dict(synth.make_state_dict(L=SETS[name][1], seed=1, bin_score=bin_score))
    net = (net.double() if exact else net.float()).eval().to(DEV)
    assert net.exact() == exact and net._ragged_fp32() == (not exact) and net._extract_mode() == mode
    return net


@functools.lru_cache(maxsize=None)
def _pairs(name, device=DEV):
    """the per-pair dicts of a set as a batch_size=1 loader yields them (a leading axis of 1)"""
    return tuple({k: v.to(device) for k, v in synth.make_batch(1, n, m, first_pair=b).items()} for b, (n, m) in enumerate(SETS[name][0]))


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """the oracle on every pair of the set alone, once: (outputs, Z, smallest top-k gap, smallest arg-max margin) per pair"""
    sd = synth.make_state_dict(L=SETS[name][1], seed=1)
    out = []
    for p in _pairs(name, 'cpu'):
        ref, cap, gap, margin = RD.oracle_pair(sd, _cfg(name), p)
        out.append((ref, cap['Z'], gap, margin))
    return tuple(out)


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)


def _check_pair(out, ref_m0, ref_m1, ref_s0, ref_s1, ref_Z, decided, what):
    """one pair of a ragged call against the fp64 reference on the pair alone, by the split of the module docstring; returns the indices
    (frame 0, frame 1) whose match differs as a near tie"""
    m0, m1 = out['matches0'].cpu(), out['matches1'].cpu()
    Z = out['Z'].cpu().double()
    ref_m0, ref_m1 = (torch.as_tensor(np.asarray(t)).long().reshape(m.shape) for t, m in ((ref_m0, m0), (ref_m1, m1)))
    ref_Z = torch.as_tensor(np.asarray(ref_Z)).double().reshape(Z.shape)
    err = (Z - ref_Z).abs()
    es = [(out[k].cpu().double() - torch.as_tensor(np.asarray(r)).double().reshape(out[k].shape)).abs()
          for k, r in (('matching_scores0', ref_s0), ('matching_scores1', ref_s1))]
    same = [m0 == ref_m0, m1 == ref_m1]
    worst_s = max([float(e[s].max()) for e, s in zip(es, same) if s.any()] + [0.0])
    print(f'{what}: decided {decided}; max |Z - reference| = {float(err.max()):.3e}, entries beyond 1e-4 {float((err > Z_TOL).double().mean()):.2e}, '
          f'scores {worst_s:.3e}, matches differing {int((~same[0]).sum() + (~same[1]).sum())}')
    if decided:
        assert same[0].all() and same[1].all(), what
        assert float(err.max()) < Z_TOL and worst_s < Z_TOL, (what, float(err.max()), worst_s)
        return set(), set()
    assert float(err.max()) < PLAIN_MAX and float((err > Z_TOL).double().mean()) < PLAIN_FRAC, (what, float(err.max()))
    assert worst_s < PLAIN_MAX, (what, worst_s)
    flips = near_tie_mismatches(out['Z'], out['matches0'], out['matches1'], ref_m0.numpy(), ref_m1.numpy(), tol=Z_TOL)
    return {i for side, _, i, _, _, _ in flips if side == 0}, {i for side, _, i, _, _, _ in flips if side == 1}


def test_the_decided_pairs_are_the_ones_written_down():
    for name in SETS:
        got = tuple(b for b, (_, _, gap, margin) in enumerate(_oracle(name)) if RD.decided(gap, margin))
        print(name, [(f'{gap:.2e}', f'{margin:.2e}') for _, _, gap, margin in _oracle(name)])
        assert got == DECIDED[name], (name, got)
    assert sum(b in DECIDED['A'] for b in range(5)) >= 4          # of the five reference-held pairs


def test_forward_ragged_against_the_reference_held_pairs(golden_dir):
    """Set A's first five pairs in one call against tests/golden/ragged_pairs.npz - the reference's own outputs, one pair per call, in every
    extraction variant it holds for the pair.  The near ties a variant other than the default may differ in are those of the default
    one (every variant reads the same arg-maxes): the indices it flags and their partners."""
    g = np.load(os.path.join(golden_dir, 'ragged_pairs.npz'))
    pairs = list(_pairs('A')[:5])
    assert [tuple(int(x) for x in r) for r in g['pairs']] == [tuple(c) for c in SET_A[:5]]
    flagged = {}
    for tag, mode in {'default': 0, 'mutual': 1, 'sg': 2, 'sgmutual': 3}.items():
        held = [b for b in range(5) if f'p{b}_{tag}_matches0' in g.files]
        with torch.no_grad():
            got = _net('A', mode).forward_ragged([pairs[b] for b in held], return_Z=True)
        for o, b in zip(got, held):
            ref = [g[f'p{b}_{tag}_{k}'] for k in ('matches0', 'matches1', 'mscores0', 'mscores1')]
            if tag == 'default' or b in DECIDED['A']:
                flagged[b] = _check_pair(o, *ref, g[f'p{b}_Z'], b in DECIDED['A'], f'{tag} pair {b} {SET_A[b]}')
                continue
            # an undecided pair in another variant: Z as in the default one; a match may differ where the default variant met a near tie
            f0, f1 = flagged[b]
            err = (o['Z'].cpu().double().numpy() - g[f'p{b}_Z']).__abs__()
            assert err.max() < PLAIN_MAX and (err > Z_TOL).mean() < PLAIN_FRAC, (tag, b, err.max())
            m0, m1 = o['matches0'].cpu().numpy(), o['matches1'].cpu().numpy()
            for i in np.nonzero(m0[0] != ref[0].reshape(-1))[0]:
                assert i in f0 or {int(m0[0, i]), int(ref[0].reshape(-1)[i])} & f1, (tag, b, 0, int(i))
            for j in np.nonzero(m1[0] != ref[1].reshape(-1))[0]:
                assert j in f1 or {int(m1[0, j]), int(ref[1].reshape(-1)[j])} & f0, (tag, b, 1, int(j))


@pytest.mark.parametrize('name', ['A', 'C', 'M'])
def test_forward_ragged_against_the_oracle_on_every_pair(name):
    net, pairs = _net(name), _pairs(name)
    with torch.no_grad():
        got = net.forward_ragged(list(pairs), return_Z=True)
    net.check(DEV)
    for b, (o, (ref, Z, _, _)) in enumerate(zip(got, _oracle(name))):
        n, m = SETS[name][0][b]
        assert set(o) == set(KEYS) | {'Z'} and tuple(o['Z'].shape) == (1, n + 1, m + 1) and o['Z'].dtype == torch.float32
        assert o['matches0'].dtype == torch.int64 and tuple(o['matches0'].shape) == (1, n) and tuple(o['matches1'].shape) == (1, m)
        _check_pair(o, ref['matches0'], ref['matches1'], ref['matching_scores0'], ref['matching_scores1'], Z, b in DECIDED[name],
                    f'set {name} pair {b} ({n} x {m})')


def test_forward_ragged_returns_what_forward_returns_for_the_pair():
    """keys, dtypes and shapes of forward on the pair alone - and the reference's INTEGER zero scores for a pair that matched nothing: a bin
    score of 32 leaves the 8 x 8 pair of set A without a match (the oracle's count; its neighbours keep 1 to 4)"""
    for bin_score in (1.0, 32.0):
        net, pairs = _net('A', 0, bin_score), _pairs('A')
        with torch.no_grad():
            got = net.forward_ragged(list(pairs))
            for b, p in enumerate(pairs):
                alone = net(p)
                assert got[b].keys() == alone.keys(), b
                for k in alone:
                    assert got[b][k].dtype == alone[k].dtype and got[b][k].shape == alone[k].shape, (bin_score, b, k)
                if bin_score == 1.0 and b in DECIDED['A']:       # (both are the oracle's there)
                    assert torch.equal(got[b]['matches0'], alone['matches0']) and torch.equal(got[b]['matches1'], alone['matches1']), b
        if bin_score == 32.0:
            kinds = [g['matching_scores0'].dtype for g in got]
            assert kinds[4] == torch.int64 and (got[4]['matches0'] == -1).all() and not got[4]['matching_scores1'].any()
            assert kinds.count(torch.float32) >= 1


def test_results_do_not_depend_on_position_or_companions():
    """Equal slots (65 x 97: pairs 3 and 6 set them): a permutation, a subset and a packed batch as input give every pair the same bits."""
    net, pairs = _net('A'), list(_pairs('A'))
    with torch.no_grad():
        ref = net.forward_ragged(pairs, return_Z=True)
        for order in ([3, 6, 0, 5, 1, 4, 2], [6, 2, 3]):
            got = net.forward_ragged(ops.pack_ragged([pairs[i] for i in order]), return_Z=True)
            for i, p in enumerate(order):
                _same(got[i], ref[p], (order, p))


@pytest.mark.parametrize('poison', [float('nan'), 1e300])
def test_padding_reaches_nothing(poison):
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
        assert torch.isfinite(got[b]['Z']).all()


def test_an_empty_frame_gets_the_early_out():
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


def test_evaluate_ragged_equals_evaluate_matches_on_every_pairs_own_outputs():
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
        fwd = net.forward_ragged(pairs)
    assert tuple(got['metrics'].shape) == (len(pairs), len(ops.EvalColumns))
    for b, p in enumerate(pairs):
        _same(got['pairs'][b], fwd[b], b)
        metrics, T, _ = ops.evaluate_matches(fwd[b]['matches0'], fwd[b]['matches1'], p['gt_matches0'], p['gt_matches1'], p['keypoints0'],
                                             p['keypoints1'], T_gt=p['T_gt'])
        # (bit for bit, NaN columns included: compared as bytes)
        assert got['metrics'][b].cpu().numpy().tobytes() == metrics[0].cpu().numpy().tobytes(), b
        assert got['T'][b].cpu().numpy().tobytes() == T[0].cpu().numpy().tobytes(), b


def test_an_exact_module_in_the_same_process_keeps_its_own_bits():
    """an exact-mode module that carries the key too runs its own ragged forward, before and after an fp32-class one"""
    lib = _lib.load()
    prev = lib.mdgat_set_f64_attention_form(0)
    try:
        net64, net32, pairs = _net('A', exact=True), _net('A'), list(_pairs('A'))
        with torch.no_grad():
            before = net64.forward_ragged(pairs, return_Z=True)
            net32.forward_ragged(pairs)
            after = net64.forward_ragged(pairs, return_Z=True)
            for b, p in enumerate(pairs):
                _same(before[b], after[b], b)
                _same({k: before[b][k] for k in KEYS}, net64(p), b)
                assert before[b]['matching_scores0'].dtype == torch.float64
    finally:
        lib.mdgat_set_f64_attention_form(prev)


def test_refusals_on_the_device():
    net, pairs = _net('A'), list(_pairs('A'))
    with pytest.raises(ValueError, match='at most 512 per frame'):
        net.forward_ragged(pairs + [{k: v.to(DEV) for k, v in synth.make_batch(1, 513, 16).items()}])
    with pytest.raises(ValueError, match='fewer than a dynamic layer keeps'):
        net.forward_ragged(pairs + [{k: v.to(DEV) for k, v in synth.make_batch(1, 7, 16).items()}])
    with torch.no_grad():
        assert len(net.forward_ragged(pairs)) == len(pairs)          # (and the module still runs)
