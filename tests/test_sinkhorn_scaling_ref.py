"""tests/sinkhorn_scaling_ref.py - the float32 restatement of sinkhorn_scaling_kernel - against the fp64 oracle, and the conditions that
make FOLD_CASES a test of the kernel's fold branches: no device.

What a GPU test cannot see without counters in the kernel's iteration loop is established here, on the CPU: each fold case is NOT handed to
the streaming kernel (its smallest entry keeps 4 octaves to the range flag: v_exp_f32's rounding is 2^-22 relative), the fold kinds it
claims fire, and with the folds off the factor passes 2^44 - 4 octaves beyond the kernel's threshold, so the kernel folds too, whatever
iteration its own rounding picks.  The planted mistakes show that these inputs are sensitive to exactly the terms a fold has to update."""
import functools

import numpy as np
import pytest
import torch

import sinkhorn_forms as S
import sinkhorn_scaling_ref as R
from oracle import mdgat_oracle as O

MARGIN_KMIN = 2.0 ** -96          # 4 octaves above the range flag (2^-100)
MARGIN_LOG = 44.0                 # 4 octaves beyond the fold thresholds (2^40, 2^-40)


def _oracle(s, alpha, iters):
    return O.log_optimal_transport(torch.from_numpy(np.asarray(s, dtype=np.float64)), alpha, iters).numpy()


@functools.lru_cache(maxsize=None)
def _fold_case(name):
    """(scores [3, N, M], oracle Z, restatement Z, reports, reports with the folds off) of a fold case's batch."""
    alpha, iters, _, form, _ = R.FOLD_CASES[name][5:]
    s = R.fold_batch(name)
    from_k = form == 'scaling<false,4>'
    Z, rep = R.batch(s, alpha, iters, from_k=from_k)
    _, rep0 = R.batch(s, alpha, iters, fold=False, from_k=from_k)
    return s, _oracle(s, alpha, iters), Z, rep, rep0


@pytest.mark.parametrize('N,M', list(S.CLUSTER_CASES))
def test_restatement_vs_oracle_on_the_form_cases(N, M):
    s = R.form_batch(N, M)
    ref = _oracle(s, R.FORM_ALPHA, R.FORM_ITERS)
    Z, rep = R.batch(s, R.FORM_ALPHA, R.FORM_ITERS, from_k=S.CLUSTER_CASES[N, M][0] == 'scaling<false,4>')
    err = float(np.abs(Z - ref).max())
    print(f'{N} x {M}: restatement vs oracle {err:.2e} (bar {R.bar(ref):.2e})')
    assert np.isfinite(Z).all() and err < R.bar(ref)
    # plain Gaussian scores: nothing folds, nothing is flagged - these cases test the forms, not the folds
    assert not any(r['flagged'] for r in rep) and not any(R.fired(r) for r in rep)


@pytest.mark.parametrize('name', list(R.FOLD_CASES))
def test_restatement_vs_oracle_on_the_fold_cases(name):
    s, ref, Z, rep, _ = _fold_case(name)
    err = float(np.abs(Z - ref).max())
    print(f'{name}: restatement vs oracle {err:.2e} (bar {R.bar(ref):.2e})')
    assert np.isfinite(Z).all() and err < R.bar(ref)
    # both epilogues (the scores recovered from K, the scores read again) hold the bar
    alpha, iters = R.FOLD_CASES[name][5:7]
    for from_k in (False, True):
        Z2, _ = R.scaling(s[0], alpha, iters, from_k=from_k)
        assert np.abs(Z2 - ref[0]).max() < R.bar(ref), from_k


@pytest.mark.parametrize('name', list(R.FOLD_CASES))
def test_fold_cases_hold_their_conditions(name):
    claims, form, (GR, GC) = R.FOLD_CASES[name][7:]
    N, M = R.FOLD_CASES[name][:2]
    s, _, _, rep, rep0 = _fold_case(name)
    for b in (0, 2):                                   # the two fold pairs of the batch
        r, r0 = rep[b], rep0[b]
        what = f'{name} pair {b}: kmin 2^{np.log2(r["kmin"]):.1f}, folds {r["folds"]}, without folds {r0["maxlog"]}'
        # (1) the scaling form keeps the pair: 4 octaves of margin to the range flag
        assert not r['flagged'] and r['kmin'] >= MARGIN_KMIN, what
        # (2) the claimed folds fire
        assert set(claims) <= R.fired(r), what
        # (3) ... and must: left alone the factor goes 4 octaves beyond the threshold
        for kind in claims:
            assert r0['maxlog'][kind] > MARGIN_LOG, what
        assert not R.fired(r0)
    # the plain pair between them (scores spread four times as wide): under a hot-column case's bin score it folds nothing; under the
    # lopsided cases' bin score of -55 it is beyond the range test, so those batches mix pairs the cluster kernel keeps with one it hands on
    assert rep[1]['flagged'] == R.middle_pair_flagged(name) == name.startswith('lopsided')
    assert rep[1]['flagged'] or not R.fired(rep[1])
    # the shape reaches the instantiation the case is meant for
    p = S.plan(3, N, M)
    assert (p.scaling, p.GR, p.GC) == (form, GR, GC)


def test_fold_cases_reach_every_kind_in_every_instantiation():
    for form in S.SCALING:
        kinds = set()
        for name, c in R.FOLD_CASES.items():
            if c[8] == form:
                kinds |= set(c[7])
        assert kinds == set(R.KINDS), form
    # <false, 4> with and without partners; the column fold in slab 0 only and in the last slab only
    assert {c[9] for c in R.FOLD_CASES.values() if c[8] == 'scaling<false,4>'} == {(1, 1), (2, 1)}
    for name, slab in (('hot-40x513-c3', 0), ('hot-40x513-c512', 1)):
        for b in (0, 2):
            assert {sl for _, sl in _fold_case(name)[3][b]['folds']['col']} == {slab}, name
    # the hot column in a lane's first register, and in the last valid column of a ragged lane (M = 65: lane 8 holds column 64 alone)
    assert R.FOLD_CASES['hot-513x40-c0'][2] == (0,) and R.FOLD_CASES['hot-130x65-c64'][2] == (64,)


def test_the_denormal_reread_is_reached():
    """In the '-cold' cases an entry of K ends below 2^-126 in an unflagged pair - what the <false, 4> epilogue's re-read is for - and
    without the re-read Z is not finite.  No other fold case has such an entry."""
    for name in R.FOLD_CASES:
        s, ref, Z, rep, _ = _fold_case(name)
        for b in (0, 2):
            assert (rep[b]['denormal'] >= 1) == (name in R.DENORMAL_CASES), (name, b, rep[b]['denormal'])
    for name in R.DENORMAL_CASES:
        assert R.FOLD_CASES[name][8] == 'scaling<false,4>'
        s, ref, _, _, _ = _fold_case(name)
        alpha, iters = R.FOLD_CASES[name][5:7]
        r, c, _ = R.FOLD_CASES[name][4]
        Zbad, _ = R.scaling(s[0], alpha, iters, no_reread=True)
        assert not np.isfinite(Zbad[r, c]) and np.isfinite(np.delete(Zbad.ravel(), r * Zbad.shape[1] + c)).all()


# which fold cases each planted mistake must break: the hot-column cases fold columns and rows, the lopsided ones the dustbins
_HOT = [n for n in R.FOLD_CASES if n.startswith('hot')]
_LOP = [n for n in R.FOLD_CASES if n.startswith('lopsided')]
# (kr matters through the OTHER columns of the folding slab, whose kr aN is not small beside their column sum; in hot-40x513-c512 the
# folding slab holds the hot column alone, whose column sum dwarfs kr aN: that case cannot see a lost kr)
PLANTED = {'drop_kr': [n for n in _HOT if n != 'hot-40x513-c512'], 'drop_v0': _HOT + _LOP, 'drop_kbr': _HOT, 'drop_kc': _LOP}
WIDE = 100.0                      # "misses the bar by a wide factor"


@pytest.mark.parametrize('mistake', list(PLANTED))
def test_planted_mistakes_miss_the_bar(mistake):
    small = [n for n in R.FOLD_CASES if R.FOLD_CASES[n][0] * R.FOLD_CASES[n][1] <= 30000]
    hit = []
    for name in small:
        s, ref, _, _, _ = _fold_case(name)
        alpha, iters = R.FOLD_CASES[name][5:7]
        Zbad, _ = R.scaling(s[0], alpha, iters, **{mistake: True})
        err = float(np.abs(Zbad - ref[0]).max()) if np.isfinite(Zbad).all() else float('inf')
        print(f'{mistake} on {name}: {err:.2e} (bar {R.bar(ref):.2e})')
        if err > WIDE * R.bar(ref):
            hit.append(name)
        else:
            assert err < R.bar(ref), (mistake, name, err)      # a case the term does not enter: unchanged, not merely close
    assert hit == [n for n in small if n in PLANTED[mistake]], (mistake, hit)


# ---- the suite's earlier inputs reach no fold ----
@pytest.mark.parametrize('N,M,iters', [(1, 1, 3), (3, 200, 10), (130, 65, 25), (256, 256, 20), (300, 513, 30), (700, 900, 10), (64, 64, 0)])
def test_the_inputs_of_test_sinkhorn_vs_oracle_fold_nothing(N, M, iters):
    s = np.random.RandomState(N * 3 + M).standard_normal((3, N, M)) * 4.0
    _, rep = R.batch(s, 0.7, iters)
    _, rep0 = R.batch(s, 0.7, iters, fold=False)
    for r, r0 in zip(rep, rep0):
        assert not r['flagged'] and not R.fired(r)
        assert max(r0['maxlog'].values()) < 40 - 20, r0['maxlog']        # ... by more than 20 octaves


@pytest.mark.parametrize('N,M,iters,scale', [(512, 128, 7, 30.0), (512, 512, 3, 40.0), (300, 200, 20, 25.0), (1024, 512, 5, 30.0)])
def test_the_inputs_of_test_sinkhorn_wide_dynamic_range_are_flagged(N, M, iters, scale):
    """Every pair of every case is beyond the range test: what that test compares with the oracle is the streaming kernel's result
    (tests/test_gpu_ops.py asserts so through the launch counters and the bit-equality with the streaming kernel).  No fold either."""
    s = np.random.RandomState(N + M + iters).standard_normal((2, N, M)) * scale + 50.0
    _, rep = R.batch(s, 0.37, iters)
    for r in rep:
        assert r['flagged'] and not R.fired(r)
