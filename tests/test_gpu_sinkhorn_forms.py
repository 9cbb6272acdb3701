"""Every instantiation the fp32 Sinkhorn launchers reach, at the smallest shape that reaches it, against the fp64 oracle on every entry -
and the scaling kernel's four fold branches, which no earlier input reached (tests/test_sinkhorn_scaling_ref.py establishes on the CPU
that the inputs used here do, without raising the range flag).  The form is asserted around every call: before from the plan
(mdgat_sinkhorn_plan), afterwards from the launch counters (sinkhorn_forms.watch).

Measured on an MI355X (max |Z - oracle|; the bar is 1e-4 max(1, |ref|max / 100)):
  scaling<false,4>   GR 1 (64 x 64) 4.9e-6, GR 2 (130 x 65) 6.4e-6, GR 4 (390 x 24) 6.1e-6
  scaling<false,16>  GR 5 (513 x 40) 4.8e-6, GR 16 (2048 x 8) 5.5e-6
  scaling<true,16>   GR 1 GC 2 (40 x 513) 4.3e-6, GR 2 GC 3 (130 x 1030) 5.3e-6, GR 1 GC 4 (20 x 1540) 4.9e-6
  stream<1,16> 8.2e-6, <2,16> 4.7e-6, <4,16> 5.3e-6, <8,16> 7.3e-6, <16,8> 5.1e-6, <32,8> 5.6e-6 (M = 1025), 5.7e-6 (M = 2048)
  fold cases, <false,4>:  hot-64x64-c3 7.0e-6, hot-64x64-c3-cold 6.8e-6, lopsided-128x40 9.0e-6, hot-130x65-c64 6.6e-6,
                          hot-130x65-every7th 8.2e-6, hot-130x65-c3-cold 7.6e-6, lopsided-130x65 9.4e-6
              <false,16>: hot-513x40-c0 6.6e-6, lopsided-513x40 1.2e-5
              <true,16>:  hot-40x513-c3 6.9e-6, hot-40x513-c512 5.0e-6, lopsided-1030x513 1.1e-5
  (the streaming kernel on the fold cases: 3.7e-6 ... 1.5e-5).  The denormal re-read of the <false,4> epilogue is reached by the two
  '-cold' cases (tests/test_sinkhorn_scaling_ref.py: one entry of K below 2^-126 in an unflagged pair); no defect was found.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sinkhorn_forms as S  # noqa: E402
import sinkhorn_scaling_ref as R  # noqa: E402
from extract_ref import check_extraction, pick_threshold  # noqa: E402
from mdgat_matcher_amd import ops  # noqa: E402
from oracle import mdgat_oracle as O  # noqa: E402

DEV = 'cuda:0'
WORST = {}        # what the last test of the file prints: largest error per form and per fold case


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _oracle(s, alpha, iters):
    return O.log_optimal_transport(torch.as_tensor(s).double().cpu(), alpha, iters)


def _err(Z, ref, what):
    assert torch.isfinite(Z).all(), what
    err = float((Z.cpu().double() - ref).abs().max())
    bar = R.bar(ref.numpy())
    print(f'{what}: max |Z - oracle| = {err:.3e} (bar {bar:.2e})')
    return err, bar


def _note(key, err):
    WORST[key] = max(WORST.get(key, 0.0), err)


def _sinkhorn(s, alpha, iters, streaming=False, what=''):
    """ops.sinkhorn with the form asserted: the plan before the call, the counters after it.  Returns (Z, plan)."""
    B, N, M = s.shape
    p = S.plan(B, N, M, cus=_cus(), workspace=not streaming)
    with S.watch() as w:
        Z = ops.sinkhorn(s, alpha, iters, streaming=streaming)
    S.assert_launched(w, p, what or (B, N, M, streaming))
    return Z, p


# -------------------------------------------------------------------------------------- (a) every form against the oracle
@pytest.mark.parametrize('N,M', list(S.CLUSTER_CASES))
def test_scaling_forms_vs_oracle(N, M):
    name, GR, GC = S.CLUSTER_CASES[N, M]
    s = torch.from_numpy(R.form_batch(N, M, S.FORMS_BATCH))
    ref = _oracle(s, R.FORM_ALPHA, R.FORM_ITERS)
    Z, p = _sinkhorn(s.to(DEV), R.FORM_ALPHA, R.FORM_ITERS, what=name)
    assert (p.path, p.scaling, p.GR, p.GC) == (S.CLUSTER, name, GR, GC) and p.stream != 'none'
    err, bar = _err(Z, ref, f'{name} GR={GR} GC={GC} {N} x {M}')
    _note(f'{name} GR={GR} GC={GC} ({N} x {M})', err)
    assert err < bar
    # the cluster kernel's own result was kept: the gated streaming kernel behind it left at once
    Zs, ps = _sinkhorn(s.to(DEV), R.FORM_ALPHA, R.FORM_ITERS, streaming=True)
    assert ps.stream == p.stream and not torch.equal(Z, Zs)


@pytest.mark.parametrize('N,M', list(S.STREAM_CASES))
def test_streaming_forms_vs_oracle(N, M):
    name = S.STREAM_CASES[N, M]
    s = torch.from_numpy(R.form_batch(N, M, S.FORMS_BATCH))
    ref = _oracle(s, R.FORM_ALPHA, R.FORM_ITERS)
    Z, p = _sinkhorn(s.to(DEV), R.FORM_ALPHA, R.FORM_ITERS, streaming=True, what=name)
    assert (p.path, p.stream) == (S.STREAMING, name)
    err, bar = _err(Z, ref, f'{name} {N} x {M}')
    _note(f'{name} (M = {M})', err)
    assert err < bar


# -------------------------------------------------------------------------- (b) the fold cases through every scaling instantiation
@functools.lru_cache(maxsize=None)
def _fold_run(name):
    """A fold case's batch [fold pair, plain pair, fold pair] through the cluster kernel and the streaming kernel, and the oracle: computed
    once, never modified."""
    alpha, iters, _, form, (GR, GC) = R.FOLD_CASES[name][5:]
    s = torch.from_numpy(R.fold_batch(name))
    Z, p = _sinkhorn(s.to(DEV), alpha, iters, what=name)
    assert (p.scaling, p.GR, p.GC) == (form, GR, GC)
    Zs, _ = _sinkhorn(s.to(DEV), alpha, iters, streaming=True, what=name)
    return s, _oracle(s, alpha, iters), Z, Zs


@pytest.mark.parametrize('name', list(R.FOLD_CASES))
def test_fold_cases_vs_oracle(name):
    """Z of the cluster call within the bar of the oracle on every entry, the fold pairs' Z the scaling form's own."""
    s, ref, Z, Zs = _fold_run(name)
    err, bar = _err(Z, ref, f'{name} [{R.FOLD_CASES[name][8]}]')
    _note(f'fold case {name} [{R.FOLD_CASES[name][8]}]', float((Z[[0, 2]].cpu().double() - ref[[0, 2]]).abs().max()))
    assert err < bar
    # the scaling form's own result was kept for the fold pairs (they are not flagged: the restatement, 4 octaves of margin); the plain
    # pair between them is, under the lopsided cases' bin score, beyond the range test and was redone by the streaming kernel
    for b in (0, 2):
        assert not torch.equal(Z[b], Zs[b]), b
    assert torch.equal(Z[1], Zs[1]) == R.middle_pair_flagged(name)
    # the streaming kernel on the same inputs, for the record
    err_s, _ = _err(Zs, ref, f'{name} [streaming]')
    assert err_s < bar


@pytest.mark.parametrize('name', list(R.FOLD_CASES))
def test_fold_cases_equal_the_pair_alone(name):
    """Partners take every fold decision alike, and nothing a pair folds reaches the next pair: each pair of the batch, bit for bit, is
    what it is alone."""
    alpha, iters = R.FOLD_CASES[name][5:7]
    s, _, Z, _ = _fold_run(name)
    for b in range(3):
        alone, _ = _sinkhorn(s[b:b + 1].to(DEV), alpha, iters, what=(name, b))
        assert torch.equal(alone[0], Z[b]), (name, b)


@pytest.mark.parametrize('name', list(R.FOLD_CASES))
def test_fold_cases_fused_extraction(name):
    """The fused arg-max reads the epilogue's registers: all four modes against the rules applied to the Z the same call returned, which is
    the Z of ops.sinkhorn."""
    alpha, iters = R.FOLD_CASES[name][5:7]
    s, _, Z, _ = _fold_run(name)
    B, N, M = s.shape
    p = S.plan(B, N, M, cus=_cus())
    thr_inner = pick_threshold(Z.cpu())
    for mode in range(4):
        thr = 0.2 if mode < 2 else thr_inner
        with S.watch() as w:
            m0, m1, s0, s1, Zx = ops.sinkhorn_extract(s.to(DEV), alpha, iters, mode=mode, match_threshold=thr, want_Z=True)
        S.assert_launched(w, p, (name, mode), extract=True)
        assert torch.equal(Zx, Z), (name, mode)
        check_extraction(Zx, m0, m1, s0, s1, mode, thr)


# ----------------------------------------------------------------------------------------------- (c) state carried between pairs
@pytest.mark.parametrize('B,hot,other', [(66, 'hot-64x64-c3', 'hot-64x64-c3-cold'), (34, 'hot-130x65-c64', 'hot-130x65-every7th'),
                                       (66, 'hot-130x65-c64', 'hot-130x65-every7th')])
def test_a_fold_pair_leaves_nothing_to_the_next_pair_of_its_workgroup(B, hot, other):
    """More pairs than groups in flight (64 at most): groups 0 and 1 run two pairs each - a fold pair then a plain one, and a plain one
    then a fold pair.  Every pair equals itself alone, bit for bit.  (34 pairs of 130 x 65 have a group each on a 256-CU part - the
    plan says so; that case checks 34 concurrent groups, the one of 66 the carried state.)"""
    N, M = R.FOLD_CASES[hot][:2]
    alpha, iters = R.FOLD_CASES[hot][5:7]
    assert R.FOLD_CASES[other][:2] == (N, M) and R.FOLD_CASES[other][5:7] == (alpha, iters)      # (one bin score per call)
    s = (np.random.RandomState(B).standard_normal((B, N, M)) * 3.0).astype(np.float32)
    s[0], s[B - 1] = R.fold_scores(hot), R.fold_scores(other, seed=4)
    s[1], s[B - 2] = R.plain_scores(N, M, seed=6), R.plain_scores(N, M, seed=7)
    s = torch.from_numpy(s).to(DEV)
    Z, p = _sinkhorn(s, alpha, iters)
    if B == 66:
        # pair b runs in group b % 64: group 0 the fold pair 0 then the plain pair 64, group 1 the plain pair 1 then the fold pair 65
        assert p.ngroups == 64 and (B - 2) % p.ngroups == 0 and (B - 1) % p.ngroups == 1
    assert torch.isfinite(Z).all()
    for b in (0, 1, B - 2, B - 1, B // 2):
        alone, _ = _sinkhorn(s[b:b + 1].contiguous(), alpha, iters)
        assert torch.equal(alone[0], Z[b]), b
    Zs = ops.sinkhorn(s, alpha, iters, streaming=True)
    assert bool((Z != Zs).flatten(1).any(1).all())                       # no pair was redone
    assert (Z - Zs).abs().max() < 1e-4


# ------------------------------------------------------------------------------------------------------------------- (e) the figures
def test_zz_print_the_largest_errors():
    for k in sorted(WORST):
        print(f'{k}: {WORST[k]:.2e}')
