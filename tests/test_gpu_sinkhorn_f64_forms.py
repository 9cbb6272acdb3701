"""Every form of the fp64 Sinkhorn (csrc/sinkhorn_f64.hip: sinkhorn_f64_kernel<8, false | true>, and the streaming form's
sinkhorn_f64_wide_iter_kernel / _final_kernel<5 | 9 | 17, false | true>) at the smallest shapes that reach it and each end of it, with the
launch counters (mdgat_sinkhorn_f64_launches) as witnesses of what ran: around every group of calls exactly the index the case names
moves, by one per op call.  The tables, and why each case is there: tests/sinkhorn_f64_forms.py; tests/test_sinkhorn_f64_plan.py holds
them to the plan and shows on the oracle alone that no arg-max of any case is a near tie, so nothing below leaves out a row, a column
or a case.

Uniform cases: the checks of tests/test_gpu_f64.py::_sinkhorn_f64_case itself - Z within 1e-12 of the oracle's log_optimal_transport,
the four extraction modes equal to ops.extract of the oracle's Z, scores within 1e-6, Z32 within that function's bound.
Ragged cases on the streaming form: the yardstick of tests/test_gpu_ragged_sinkhorn_stream.py - every pair's block of Z, Z32, the matches
and the scores of all four modes have the BITS of the pair run alone under mdgat_set_f64_sinkhorn_form(1), the rest of every slot is
fixed - and every pair within 1e-12 of the oracle."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import sinkhorn_f64_forms as S  # noqa: E402
from mdgat_matcher_amd import ops  # noqa: E402
from oracle import mdgat_oracle as O  # noqa: E402
from test_gpu_f64 import _sinkhorn_f64_case  # noqa: E402

DEV = 'cuda:0'
STREAM = dict(form='streaming')
CALLS_PER_CASE = 5      # _sinkhorn_f64_case: ops.sinkhorn_f64 once, ops.sinkhorn_f64_extract once per mode


@pytest.mark.parametrize('c', S.UNIFORM_CASES, ids=lambda c: f'{S.NAMES[c.index]}-{c.B}x{c.N}x{c.M}-it{c.iters}')
def test_uniform_case_runs_its_form_and_agrees_with_the_oracle(c):
    with S.forced(c.form), S.watch() as w:
        assert S.plan(c.N, c.M, form=0)[0] == c.index                                  # (form 0: the current setting)
        _sinkhorn_f64_case(c.B, c.N, c.M, c.iters, S.UNIFORM_ALPHA, S.SCALE)
    assert w.ran() == {c.index: CALLS_PER_CASE}, (c, {S.NAMES[i]: n for i, n in w.ran().items()})


# ---------------------------------------------------------------------------------------------------- ragged, the streaming form
@functools.lru_cache(maxsize=None)
def _alone(name):
    """every pair of the set run alone under form 1: Z (fp64) and, per extraction mode, (m0, m1, s0, s1, Z32) - computed once, never
    modified; each pair's five calls must run the uniform streaming instantiation of its OWN size"""
    r = S.RAGGED_SETS[name]
    s = S.ragged_scores(r)
    out = []
    with S.forced(1):
        for b, (n, m) in enumerate(r.pairs):
            sb = s[b:b + 1, :n, :m].contiguous().to(DEV)
            with S.watch() as w:
                Z = ops.sinkhorn_f64(sb, r.alpha, r.iters)
                ex = [ops.sinkhorn_f64_extract(sb, r.alpha, r.iters, mode=mode, match_threshold=S.THR, want_Z=True) for mode in range(4)]
            assert w.ran() == {S.decide(n, m, form=1)[0]: 5}, (name, b, w.ran())
            out.append((Z, ex))
    return s, out


def _check_against_alone(name, s):
    r = S.RAGGED_SETS[name]
    _, alone = _alone(name)
    cnt = ([n for n, _ in r.pairs], [m for _, m in r.pairs])
    sd = s.to(DEV)
    with S.watch() as w:
        Z = ops.sinkhorn_f64(sd, r.alpha, r.iters, counts=cnt, **STREAM)
        ex = [ops.sinkhorn_f64_extract(sd, r.alpha, r.iters, mode=mode, match_threshold=S.THR, want_Z=True, counts=cnt, **STREAM) for mode in range(4)]
    assert w.ran() == {r.index: 5}, (name, {S.NAMES[i]: n for i, n in w.ran().items()})
    for b, (n, m) in enumerate(r.pairs):
        assert torch.equal(Z[b, :n + 1, :m + 1], alone[b][0][0]), (name, b)
        rest = Z[b].clone()
        rest[:n + 1, :m + 1] = 0
        assert not rest.any(), (name, b)
    for mode in range(4):
        m0, m1, s0, s1, Z32 = ex[mode]
        for b, (n, m) in enumerate(r.pairs):
            a0, a1, as0, as1, aZ = alone[b][1][mode]
            assert torch.equal(m0[b, :n], a0[0]) and torch.equal(m1[b, :m], a1[0]), (name, mode, b)
            assert torch.equal(s0[b, :n], as0[0]) and torch.equal(s1[b, :m], as1[0]), (name, mode, b)
            assert (m0[b, n:] == -1).all() and (m1[b, m:] == -1).all() and not s0[b, n:].any() and not s1[b, m:].any(), (name, mode, b)
            assert torch.equal(Z32[b, :n + 1, :m + 1], aZ[0]), (name, mode, b)
            rest = Z32[b].clone()
            rest[:n + 1, :m + 1] = 0
            assert not rest.any(), (name, mode, b)
    return Z, ex


@pytest.mark.parametrize('name', list(S.RAGGED_SETS))
def test_ragged_set_runs_the_slots_form_and_equals_every_pair_alone(name):
    """... while the small pairs alone ran <5>: the batch's instantiation follows the slot, a pair's bits do not."""
    r = S.RAGGED_SETS[name]
    s, _ = _alone(name)
    assert S.STREAM_5 in {S.decide(n, m, form=1)[0] for n, m in r.pairs} and r.index in (S.RAGGED_9, S.RAGGED_17)
    Z, ex = _check_against_alone(name, s)
    Z = Z.cpu()
    for b, (n, m) in enumerate(r.pairs):
        Zr = O.log_optimal_transport(s[b:b + 1, :n, :m], torch.tensor(r.alpha, dtype=torch.float64), r.iters)
        err = (Z[b:b + 1, :n + 1, :m + 1] - Zr).abs().max().item()
        print(f'{name} pair {b} ({n} x {m}): max|Z - oracle| = {err:.3e}')
        assert err < 1e-12, (name, b, err)
    if r.low is not None:       # the pair 40 below the bin score: nothing of it matched, all its scores zero - its neighbours keep theirs
        for mode in (0, 1):
            m0, m1, s0, s1, _ = ex[mode]
            assert (m0[r.low] == -1).all() and not s0[r.low].any() and not s1[r.low].any()
            assert (m0[0] >= 0).any() and s1[0].any()


@pytest.mark.parametrize('poison', [float('nan'), float('inf'), 1e300])
def test_ragged_nine_chunk_slots_never_read_beyond_a_pairs_counts(poison):
    _check_against_alone('V9', S.ragged_scores(S.RAGGED_SETS['V9'], fill=poison))


# ------------------------------------------------------------------------------------------------------ ragged, the resident form
def test_resident_ragged_at_its_limit_runs_its_form():
    """Slots of 575 x 575, the most the resident form takes with counts: index 1 and no other (the numerics of this form:
    tests/test_gpu_ragged_sinkhorn.py); Z within 1e-12 of the oracle on every pair, the rest of every slot zero."""
    r = S.RESIDENT_RAGGED_SET
    s = S.ragged_scores(r)
    cnt = ([n for n, _ in r.pairs], [m for _, m in r.pairs])
    with S.watch() as w:
        Z = ops.sinkhorn_f64(s.to(DEV), r.alpha, r.iters, counts=cnt).cpu()
        ops.sinkhorn_f64_extract(s.to(DEV), r.alpha, r.iters, counts=cnt)
    assert w.ran() == {S.RESIDENT_RAGGED: 2}, w.ran()
    for b, (n, m) in enumerate(r.pairs):
        Zr = O.log_optimal_transport(s[b:b + 1, :n, :m], torch.tensor(r.alpha, dtype=torch.float64), r.iters)
        assert (Z[b:b + 1, :n + 1, :m + 1] - Zr).abs().max().item() < 1e-12, b
        rest = Z[b].clone()
        rest[:n + 1, :m + 1] = 0
        assert not rest.any(), b
