"""The fp64 attention launcher's choice of instantiation (csrc/f64.hip: attention_f64_plan_index, exported as mdgat_attention_f64_plan) as a
pure function: no device.  Pins the launches of tests/test_gpu_attention_f64_forms.py to the instantiations they name, the edges of the
rule, and the whole rule against its restatement below."""
import itertools

import pytest

import attention_f64_forms as F
import attention_f64_rows as R


def test_the_cases_of_the_gpu_tests_reach_their_instantiations():
    for case in R.CASES:
        ragged = case.counts is not None
        cmin = min(min(c) for c in case.counts) if ragged else 0
        want = (F.KEEP_TAP, F.KEEP) if max(case.N, case.M) <= 512 else (F.RECOMPUTE_TAP, F.RECOMPUTE)
        for cus in (32, 256, 304):
            for form in (-1, 0, 1):         # (the form setting concerns full attention only)
                got = tuple(F.plan(case.B, case.N, case.M, case.k, tap, ragged, cmin, form, cus) for tap in (True, False))
                assert got == want, (case.id, cus, form, got)
    # the pairs of the ragged cases alone: the same instantiation exactly when the pair's and the batch's larger frame are on one side of 512
    assert F.plan(1, 300, 100, 32, True) == F.KEEP_TAP and F.plan(1, 520, 40, 32, True) == F.RECOMPUTE_TAP
    assert F.plan(1, 64, 64, 32, True) == F.KEEP_TAP and F.plan(1, 64, 64, 40, True) == F.KEEP_TAP
    assert F.plan(1, 40, 40, 40, True) == F.FULL16        # alone, k = N = M is full attention


def test_edges_at_256_and_512_keys():
    # (256 / 257 keys: which search a frame gets INSIDE the kernel and where its histograms live; the instantiation is the same)
    for n in (256, 257, 512):
        assert F.plan(2, n, n, 32, True) == F.KEEP_TAP and F.plan(2, n, n, 32, False) == F.KEEP
        assert F.plan(2, n, 40, 32, False) == F.KEEP and F.plan(2, 40, n, 32, False) == F.KEEP
    for n in (513, 2048):
        assert F.plan(2, n, n, 32, True) == F.RECOMPUTE_TAP and F.plan(2, n, n, 32, False) == F.RECOMPUTE
        assert F.plan(2, n, 40, 32, False) == F.RECOMPUTE and F.plan(2, 40, n, 32, False) == F.RECOMPUTE
    # a ragged batch follows its padded sizes, not its counts
    assert F.plan(4, 513, 512, 32, True, True, 40) == F.RECOMPUTE_TAP and F.plan(4, 512, 512, 32, True, True, 40) == F.KEEP_TAP


def test_k_equal_to_both_sizes_is_full_attention_unless_ragged():
    for n in (40, 512, 600):
        assert F.plan(2, n, n, n, True) in (F.FULL16, F.FULL32, F.SOLO)
        assert F.plan(2, n, n, n, True) == F.plan(2, n, n, 0, False)
        assert F.plan(2, n, n, n, True, True, n) == (F.KEEP_TAP if n <= 512 else F.RECOMPUTE_TAP)
        assert F.plan(2, n, n, n, False, True, n) == (F.KEEP if n <= 512 else F.RECOMPUTE)
    assert F.plan(2, 64, 40, 40, False) == F.KEEP        # k equals ONE size only: dynamic (keep-all on the frame of 40)


def test_full_attention_forms_at_256_cus_worked_by_hand():
    """40 x 40: one 128-query group and two 32-query tiles per unit, B groups of eight units.  One wave per 32 queries from 8 B >= 4 x 256
    workgroups on: B >= 128.  Below that 16 queries per workgroup while 16 B < 2 x 256: B < 32."""
    want = {1: F.FULL16, 4: F.FULL16, 31: F.FULL16, 32: F.FULL32, 127: F.FULL32, 128: F.SOLO, 500: F.SOLO}
    for B, w in want.items():
        assert F.plan(B, 40, 40) == w, B
    assert F.full_attention_batches(40, 40, 256) == (4, 32, 128)
    # 512 x 512: four groups, sixteen tiles: solo from 32 pairs on, 16 queries below 4 pairs
    want = {1: F.FULL16, 3: F.FULL16, 4: F.FULL32, 31: F.FULL32, 32: F.SOLO}
    for B, w in want.items():
        assert F.plan(B, 512, 512) == w, B
    # every partition size has three batches for the GPU test
    for cus in (32, 64, 128, 256, 304):
        assert None not in F.full_attention_batches(40, 40, cus), cus


def test_forced_forms():
    for B, n in itertools.product((1, 4, 32, 128, 500), (40, 512, 2048)):
        assert F.plan(B, n, n, form=1) == F.SOLO
        assert F.plan(B, n, n, form=0) in (F.FULL16, F.FULL32)
        assert F.plan(B, n, n, form=0) == (F.FULL16 if 8 * ((n + 31) // 32) * B < 512 else F.FULL32)
        assert F.plan(B, n, n, form=-2) == F.plan(B, n, n, form=-1)       # (anything else: by launch size)


def test_no_launch_and_refusals():
    assert F.plan(0, 40, 40) == -1 and F.plan(2, 0, 40) == -1 and F.plan(2, 40, 0) == -1 and F.plan(2, 40, 40, cus=0) == -1
    assert F.plan(2, 64, 40, 41) == -2                                   # k above the smaller frame: torch.topk raises
    assert F.plan(2, 64, 64, 41, True, True, 40) == -2                   # ... above the smallest count of a ragged batch
    assert F.plan(2, 64, 64, 8, True, True, 0) == -2 and F.plan(2, 64, 40, 8, True, True, 41) == -2       # counts outside the slots
    assert F.plan(2, 2049, 40, 8) == -3 and F.plan(2, 2049, 2049) in (F.FULL16, F.FULL32, F.SOLO)         # 2048 keys: dynamic layers only


def _restated(B, N, M, topk, tap, ragged, cnt_min, form, cus):
    """The rule as include/mdgat_hip.h and the comments of launch_attention_f64 state it, in Python"""
    if B <= 0 or N <= 0 or M <= 0 or cus <= 0:
        return -1
    if ragged and not 1 <= cnt_min <= min(N, M):
        return -2
    if topk > (cnt_min if ragged else min(N, M)):
        return -2
    nk = max(N, M)
    if nk > 2048 and topk > 0:
        return -3
    if topk > 0 and (ragged or not (topk == N == M)):
        return (F.KEEP_TAP if nk <= 512 else F.RECOMPUTE_TAP) + (0 if tap else 1)
    groups = (B * 8 + 7) // 8
    if form == 1 or (form != 0 and 8 * ((nk + 127) // 128) * groups >= 4 * cus):
        return F.SOLO
    return F.FULL16 if 8 * ((nk + 31) // 32) * groups < 2 * cus else F.FULL32


@pytest.mark.parametrize('cus', (32, 64, 128, 256, 304))
def test_plan_is_the_stated_rule(cus):
    seen = set()
    sizes = (1, 16, 40, 128, 256, 257, 512, 513, 1030, 2048, 2049)
    for B, N, M, topk, form in itertools.product((0, 1, 2, 4, 31, 32, 33, 127, 128, 1000), sizes, sizes, (0, 1, 16, 40, 512, 513), (-1, 0, 1)):
        for tap, ragged, cmin in ((0, 0, 0), (1, 0, 0), (1, 1, min(N, M)), (0, 1, 16), (0, 1, 0)):
            got = F.plan(B, N, M, topk, tap, ragged, cmin, form, cus)
            assert got == _restated(B, N, M, topk, tap, ragged, cmin, form, cus), (B, N, M, topk, tap, ragged, cmin, form)
            seen.add(got)
    assert seen == set(range(-3, 7)), sorted(seen)
