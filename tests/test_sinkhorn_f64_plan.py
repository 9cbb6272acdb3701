"""Which form a call of the fp64 Sinkhorn runs (csrc/sinkhorn_f64.hip: sinkhorn_f64_plan, exported as mdgat_sinkhorn_f64_plan) as a pure
function: no device.  Holds the plan to the Python restatement (tests/sinkhorn_f64_forms.py: decide) at both sides of every limit, holds
the case tables of tests/test_gpu_sinkhorn_f64_forms.py to the forms they name, checks that the tables leave no form and no end of a
streaming bucket without a case, and - with the oracle alone - that the seeded inputs of every case have no near tie, so that the
extraction asserts of the GPU tests need leave out no row, no column and no case."""
import functools
import itertools

import pytest
import torch

import extract_ref
import sinkhorn_f64_forms as S
from oracle import mdgat_oracle as O

SWEEP_N = (1, 31, 32, 33, 575, 576, 577, 2175, 2176)
SWEEP_M = (1, 126, 127, 128, 511, 512, 513, 574, 575, 576, 639, 640, 1023, 1024, 1151, 1152, 2175, 2176)


def test_the_plan_is_the_restatement_at_both_sides_of_every_limit():
    seen = set()
    for N, M, ragged, mode, form, history in itertools.product(SWEEP_N, SWEEP_M, (0, 1), (0, 1, 2), (-1, 1), (0, 1)):
        got = S.plan(N, M, ragged, mode, form, history)
        assert got == S.decide(N, M, ragged, mode, form, history), (N, M, ragged, mode, form, history, got)
        seen.add(got[0])
    assert seen == set(range(len(S.NAMES))) | {-1}, sorted(seen)


def test_the_restatement_worked_by_hand():
    assert S.decide(576, 575) == (S.RESIDENT, 18, 0) and S.decide(577, 575) == (S.STREAM_5, 19, 5) and S.decide(576, 576) == (S.STREAM_5, 18, 5)
    assert S.decide(576, 575, form=1) == (S.STREAM_5, 18, 5) and S.decide(1, 1, form=1) == (S.STREAM_5, 1, 1)
    assert [S.decide(40, M)[0::2] for M in (639, 640, 1151, 1152, 2175)] == [(S.STREAM_5, 5), (S.STREAM_9, 6), (S.STREAM_9, 9), (S.STREAM_17, 10), (S.STREAM_17, 17)]
    assert S.decide(2175, 1) == (S.STREAM_5, 68, 1) and S.decide(2176, 1)[0] == -1 and S.decide(1, 2176)[0] == -1 and S.decide(0, 5)[0] == -1
    # with counts: mode 0 the resident form or none, 2 the streaming one, 1 whichever holds the slots
    assert S.decide(575, 575, True, 0) == (S.RESIDENT_RAGGED, 18, 0) and S.decide(576, 575, True, 0)[0] == -1 and S.decide(575, 575, True, 0, form=1)[0] == -1
    assert S.decide(575, 575, True, 2) == (S.RAGGED_5, 18, 5) and S.decide(70, 1151, True, 2) == (S.RAGGED_9, 3, 9) and S.decide(70, 1151, True, 0)[0] == -1
    assert S.decide(575, 575, True, 1)[0] == S.RESIDENT_RAGGED and S.decide(576, 575, True, 1)[0] == S.RAGGED_5 and S.decide(575, 575, True, 1, form=1)[0] == S.RAGGED_5
    # the history run: always streaming, never with counts
    assert S.decide(64, 64, history=True) == (S.HISTORY_5, 2, 1) and S.decide(64, 640, history=True)[0] == S.HISTORY_9 and S.decide(64, 1152, history=True)[0] == S.HISTORY_17
    assert S.decide(64, 64, True, 2, history=True) == (-1, 0, 0) and S.decide(2176, 64, history=True)[0] == -1


def test_any_other_form_value_is_the_current_setting():
    lib = S._lib()
    prev = lib.mdgat_set_f64_sinkhorn_form(-1)
    try:
        for setting in (-1, 1):
            lib.mdgat_set_f64_sinkhorn_form(setting)
            for N, M, ragged, mode in itertools.product((33, 576, 577), (64, 575, 640), (0, 1), (0, 1, 2)):
                for other in (0, -2, 2, 17):
                    assert S.plan(N, M, ragged, mode, other) == S.plan(N, M, ragged, mode, setting), (setting, N, M, ragged, mode, other)
                assert S.plan(N, M, ragged, mode, -setting) == S.decide(N, M, ragged, mode, -setting)      # an explicit form overrides it
    finally:
        lib.mdgat_set_f64_sinkhorn_form(prev)


def test_the_outputs_are_optional():
    lib = S._lib()
    assert lib.mdgat_sinkhorn_f64_plan(40, 640, 0, 0, -1, 0, None, None) == S.STREAM_9
    assert lib.mdgat_sinkhorn_f64_plan(40, 2176, 0, 0, -1, 0, None, None) < 0


def test_f64_kernel_is_the_restatement():
    assert extract_ref.f64_kernel(575, 575) == ('resident', 18) and extract_ref.f64_kernel(96, 96, 1) == ('streaming', 5, 3)
    assert extract_ref.f64_kernel(10, 640) == ('streaming', 9, 1) and extract_ref.f64_kernel(2176, 8) is None
    assert extract_ref.GAP_MIN == S.MARGIN_MIN


# ---------------------------------------------------------------------------------------------------------------- the case tables
def _ragged_sets():
    return list(S.RAGGED_SETS.items()) + [('R', S.RESIDENT_RAGGED_SET)]


def test_every_case_plans_to_the_index_it_names():
    assert len({c[:5] for c in S.UNIFORM_CASES}) == len(S.UNIFORM_CASES)
    for c in S.UNIFORM_CASES:
        assert S.plan(c.N, c.M, form=c.form)[0] == c.index, c
        assert 0 <= c.iters <= 10 and c.form in (-1, 1), c
    for name, r in S.RAGGED_SETS.items():
        assert S.plan(*S.slot(r.pairs), True, 2)[0] == r.index and 3 <= r.iters <= 10, name
        # alone under form 1 the pairs run the uniform instantiation of their own size
        assert all(S.plan(n, m, form=1)[0] in (S.STREAM_5, S.STREAM_9, S.STREAM_17) for n, m in r.pairs), name
    r = S.RESIDENT_RAGGED_SET
    assert S.plan(*S.slot(r.pairs), True, 0) == (S.RESIDENT_RAGGED, 18, 0) and S.slot(r.pairs) == (S.RAGGED_LIMIT, S.RAGGED_LIMIT)
    for name, (sl, index) in S.STREAM_SETS_ELSEWHERE.items():
        assert S.plan(*sl, True, 2)[0] == index, name
    for N, M, index in S.history_cases():
        assert S.plan(N, M, history=True)[0] == index and index >= S.HISTORY_5, (N, M)


def test_the_sets_elsewhere_are_those_of_their_module():
    import test_gpu_ragged_sinkhorn_stream as T
    assert set(T.SETS) == set(S.STREAM_SETS_ELSEWHERE)
    for name, (counts, _, _) in T.SETS.items():
        assert S.slot(counts) == S.STREAM_SETS_ELSEWHERE[name][0], name


def _reached():
    """{index: the chunk counts of the cases that run it}"""
    reached = {}
    for c in S.UNIFORM_CASES:
        reached.setdefault(c.index, set()).add(S.decide(c.N, c.M, form=c.form)[2])
    for _, r in _ragged_sets():
        reached.setdefault(r.index, set()).add(S.decide(*S.slot(r.pairs), True, 0 if r.index == S.RESIDENT_RAGGED else 2)[2])
    for sl, index in S.STREAM_SETS_ELSEWHERE.values():
        reached.setdefault(index, set()).add(S.decide(*sl, True, 2)[2])
    for N, M, index in S.history_cases():
        reached.setdefault(index, set()).add(S.decide(N, M, history=True)[2])
    return reached


def test_the_tables_reach_all_eleven_forms_and_both_ends_of_every_bucket():
    reached = _reached()
    assert set(reached) == set(range(len(S.NAMES))), [S.NAMES[i] for i in set(range(len(S.NAMES))) - set(reached)]
    for bucket, (lo, hi) in enumerate(S.BUCKETS):
        assert {lo, hi} <= reached[S.STREAM_5 + bucket], (S.NAMES[S.STREAM_5 + bucket], sorted(reached[S.STREAM_5 + bucket]))
        assert all(lo <= n <= hi for i in (S.STREAM_5, S.RAGGED_5, S.HISTORY_5) for n in reached[i + bucket]), bucket
    # with counts: <9> at six and at nine chunks, <17> at ten and at seventeen
    assert {6, 9} <= reached[S.RAGGED_9] and {10, 17} <= reached[S.RAGGED_17]
    # the seams, each from both sides, on the uniform form
    Ms = {c.M for c in S.UNIFORM_CASES if c.index in (S.STREAM_5, S.STREAM_9, S.STREAM_17)}
    assert {127, 128, 639, 640, 1024, 1151, 1152, 2175} <= Ms
    # the limits, each with the other side tiny; the resident kernel's 576 rows at one column and at 575
    shapes = {(c.N, c.M) for c in S.UNIFORM_CASES}
    assert {(2175, 1), (1, 2175), (576, 1), (576, 575), (1, 575)} <= shapes
    assert any(c.iters == 0 and c.index == S.STREAM_9 for c in S.UNIFORM_CASES)


def test_every_ragged_set_fills_its_slot_and_reaches_every_lower_bucket():
    for name, r in S.RAGGED_SETS.items():
        sl = S.slot(r.pairs)
        assert sl in r.pairs, name
        own = {S.decide(n, m, form=1)[0] - S.STREAM_5 for n, m in r.pairs}
        assert own == set(range(r.index - S.RAGGED_5 + 1)), (name, own)
        assert r.low is None or r.pairs[r.low] != sl
    assert S.RAGGED_SETS['V9'].low is not None
    # the chunk counts the sets are there for
    assert S.decide(*S.slot(S.RAGGED_SETS['V9'].pairs), True, 2)[2] == 9 and S.decide(*S.slot(S.RAGGED_SETS['V6'].pairs), True, 2)[2] == 6
    assert S.decide(*S.slot(S.RAGGED_SETS['V10'].pairs), True, 2)[2] == 10


# ------------------------------------------------------------------------------- the inputs leave the extraction nothing to excuse
@functools.lru_cache(maxsize=None)
def _oracle(key):
    """the oracle's Z of a uniform case, or of every pair of a ragged set (computed once)"""
    if isinstance(key, S.Uniform):
        return [O.log_optimal_transport(S.uniform_scores(key), torch.tensor(S.UNIFORM_ALPHA, dtype=torch.float64), key.iters)]
    r = dict(_ragged_sets())[key]
    s = S.ragged_scores(r)
    return [O.log_optimal_transport(s[b:b + 1, :n, :m], torch.tensor(r.alpha, dtype=torch.float64), r.iters) for b, (n, m) in enumerate(r.pairs)]


def test_the_uniform_scores_are_those_the_gpu_check_forms(monkeypatch):
    """tests/test_gpu_f64.py::_sinkhorn_f64_case, which the GPU cases call, seeds its own scores: what it hands the oracle must be what
    the margins below were taken on."""
    import test_gpu_f64 as T

    class Seen(Exception):
        pass

    def grab(s, alpha, iters):
        raise Seen(s, float(alpha), iters)

    monkeypatch.setattr(T.O, 'log_optimal_transport', grab)
    for c in S.UNIFORM_CASES:
        with pytest.raises(Seen) as seen:
            T._sinkhorn_f64_case(c.B, c.N, c.M, c.iters, S.UNIFORM_ALPHA, S.SCALE)
        s, alpha, iters = seen.value.args
        assert torch.equal(s, S.uniform_scores(c)) and (alpha, iters) == (S.UNIFORM_ALPHA, c.iters), c


@pytest.mark.parametrize('key', list(S.UNIFORM_CASES) + [name for name, _ in _ragged_sets()], ids=str)
def test_no_arg_max_of_any_case_is_a_near_tie(key):
    """The smallest margin between the two best candidates of any arg-max the four extraction modes take exceeds 1e-9 in the oracle's
    Z (the kernels agree with it to 1e-12), no two best candidates are equal as fp32 numbers (the device's extract kernel on the
    rounded Z is the uniform cases' reference), and no exp(maximum) lies within 1e-5 of the threshold."""
    for Zr in _oracle(key):
        m64, m32, thr = S.margins(Zr)
        print(f'{key}: {tuple(Zr.shape)}: margin {m64:.3e}, of the fp32 rounding {m32:.3e}, from the threshold {thr:.3e}')
        assert m64 > S.MARGIN_MIN and m32 > 0 and thr > 1e-5, (key, tuple(Zr.shape), m64, m32, thr)


def test_the_pushed_pair_matches_nothing_beside_pairs_that_do():
    r = S.RAGGED_SETS['V9']
    matched = [bool((extract_ref.oracle_extract(Zr, 0, S.THR)[0] >= 0).any()) for Zr in _oracle('V9')]
    assert not matched[r.low] and matched[r.low - 1] and matched[0], matched
