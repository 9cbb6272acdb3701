"""The fp64 attention launcher's plan (csrc/f64.hip: attention_f64_plan) as a pure function: no device.  Its choice of instantiation,
exported as mdgat_attention_f64_plan: pins the launches of tests/test_gpu_attention_f64_forms.py to the instantiations they name, the
edges of the rule, and the whole rule against its restatement below.  Its launch geometry, exported as mdgat_attention_f64_geometry:
queries per workgroup, tiles, grid and LDS bytes against their restatement, a table worked by hand, and the device's LDS limit."""
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


def _sweep():
    sizes = (1, 16, 40, 128, 256, 257, 512, 513, 1030, 2048, 2049)
    for B, N, M, topk, form in itertools.product((0, 1, 2, 4, 31, 32, 33, 127, 128, 1000), sizes, sizes, (0, 1, 16, 40, 512, 513), (-1, 0, 1)):
        for tap, ragged, cmin in ((0, 0, 0), (1, 0, 0), (1, 1, min(N, M)), (0, 1, 16), (0, 1, 0)):
            yield B, N, M, topk, tap, ragged, cmin, form


@pytest.mark.parametrize('cus', (32, 64, 128, 256, 304))
def test_plan_is_the_stated_rule(cus):
    seen = set()
    for B, N, M, topk, tap, ragged, cmin, form in _sweep():
        got = F.plan(B, N, M, topk, tap, ragged, cmin, form, cus)
        assert got == _restated(B, N, M, topk, tap, ragged, cmin, form, cus), (B, N, M, topk, tap, ragged, cmin, form)
        seen.add(got)
    assert seen == set(range(-3, 7)), sorted(seen)


# ---- the launch the index stands for (mdgat_attention_f64_geometry) ----
A_LIST, ROWSEL_BYTES, RS_HIST_INTS, RQ_HIST_INTS = 32, 16, 320, 272        # f64.hip, row_search.hpp
LDS_LIMIT = 160 * 1024                                                     # of a workgroup on the device
QUERIES = {F.FULL16: 16, F.FULL32: 32, F.SOLO: 128, F.KEEP_TAP: 16, F.KEEP: 16, F.RECOMPUTE_TAP: 16, F.RECOMPUTE: 16}


def _restated_lds(idx, N, M, ragged, cnt_min):
    """The carve of the kernel's LDS (attn_lds in f64.hip), in bytes"""
    if idx == F.SOLO:
        return 256 * 8                                      # the exponential's table
    qt, nk_max, nk_min = QUERIES[idx], max(N, M), cnt_min if ragged else min(N, M)
    out = 4 * qt * 32 * 8                                   # the four waves' output partials
    head = (256 + 4 * qt + 4 * qt) * 8                      # the table, the row maxima and sums per wave
    if idx in (F.FULL16, F.FULL32):
        return head + out
    pitch = (nk_max + 63) // 64 * 64 + 4                    # of a row's rounding image, in floats
    if nk_max > 512:
        hist = 4 * RS_HIST_INTS                             # one row per wave
    else:                                                   # four rows per wave: in the rows' own images where the shortest is long enough
        hist = 16 if (nk_min + 63) // 64 * 64 + 4 >= RQ_HIST_INTS else 16 * RQ_HIST_INTS
    lists = qt * A_LIST * (8 + 4) + qt * 4 + qt * ROWSEL_BYTES
    return head + lists + hist * 4 + max(out, qt * pitch * 4)   # (the images are dead when the partials are written)


@pytest.mark.parametrize('cus', (32, 64, 128, 256, 304))
def test_geometry_has_the_plans_index_and_is_the_restated_launch(cus):
    worst = 0
    for B, N, M, topk, tap, ragged, cmin, form in _sweep():
        args = (B, N, M, topk, tap, ragged, cmin, form, cus)
        idx, queries, tiles, wgs, lds = F.geometry(*args)
        assert idx == F.plan(*args), args
        if idx < 0:
            assert (queries, tiles, wgs, lds) == (0, 0, 0, 0), args
            continue
        want_tiles = -(-max(N, M) // QUERIES[idx])
        assert (queries, tiles, wgs) == (QUERIES[idx], want_tiles, 8 * want_tiles * B), args
        assert lds == _restated_lds(idx, N, M, ragged, cmin), args
        assert lds <= LDS_LIMIT, args
        worst = max(worst, lds)
    assert worst == 145984                                  # 2048 keys, one row per wave: the largest launch there is


def test_geometry_worked_by_hand():
    """256 CUs.  Full attention: 2048 + 1088 q bytes at q queries per workgroup, the table alone for solo.  Dynamic (16 queries): 9536 bytes
    of table, row statistics, tie lists and RowSel; the histograms - 17408 (16 x 272 ints, a region of their own: a frame of at most 256
    keys), 64 (in the images: every frame beyond 256) or 5120 (4 x 320, beyond 512 keys); and the larger of the output partials (16384) and
    the rounding images, 64 (round64(keys) + 4)."""
    table = (
        # call                                                    index         queries tiles workgroups LDS
        (dict(B=1, N=40, M=40),                                   F.FULL16,        16,    3,     24,   19456),
        (dict(B=32, N=40, M=40),                                  F.FULL32,        32,    2,    512,   36864),
        (dict(B=128, N=40, M=40),                                 F.SOLO,         128,    1,   1024,    2048),
        (dict(B=2, N=40, M=40, topk=16),                          F.KEEP,          16,    3,     48,   43328),      # 9536 + 17408 + 16384
        (dict(B=2, N=300, M=40, topk=16),                         F.KEEP,          16,   19,    304,   47680),      # 9536 + 17408 + 64 x 324
        (dict(B=2, N=300, M=300, topk=16),                        F.KEEP,          16,   19,    304,   30336),      # 9536 + 64 + 20736
        (dict(B=2, N=512, M=512, topk=32, tap=True),              F.KEEP_TAP,      16,   32,    512,   42624),      # 9536 + 64 + 64 x 516
        (dict(B=4, N=512, M=512, topk=32, ragged=True, cnt_min=40), F.KEEP,        16,   32,   1024,   59968),      # 9536 + 17408 + 33024
        (dict(B=1, N=513, M=40, topk=16),                         F.RECOMPUTE,     16,   33,    264,   51776),      # 9536 + 5120 + 64 x 580
        (dict(B=1, N=2048, M=2048, topk=32),                      F.RECOMPUTE,     16,  128,   1024,  145984),      # 9536 + 5120 + 64 x 2052
        # the histograms' place: both frames at 256 keys - a region of their own; at 257 - in the rounding images
        (dict(B=2, N=256, M=256, topk=32),                        F.KEEP,          16,   16,    256,   43584),      # 9536 + 17408 + 64 x 260
        (dict(B=2, N=257, M=257, topk=32),                        F.KEEP,          16,   17,    272,   30336),      # 9536 + 64 + 64 x 324
    )
    for call, *want in table:
        assert list(F.geometry(cus=256, **call)) == want, call


def test_geometry_outputs_may_be_null():
    lib = F._lib()
    assert lib.mdgat_attention_f64_geometry(2, 40, 40, 16, 0, 0, 0, -1, 256, None, None, None, None) == F.KEEP
    assert F.geometry(2, 64, 40, 41) == (-2, 0, 0, 0, 0) and F.geometry(2, 2049, 40, 8) == (-3, 0, 0, 0, 0) and F.geometry(0, 40, 40) == (-1, 0, 0, 0, 0)
