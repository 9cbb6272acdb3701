"""The fp32-class attention launcher's choice for a RAGGED batch (csrc/attention.hip: attention_plan with counts, exported as
mdgat_attention_ragged_plan) as a pure function: no device.  Pins a table worked by hand from the rules a ragged launch follows - the form
from the slots alone; any topk > 0 dynamic, k == N == M included; never the stream or topk16 kernels; slots beyond 512 keypoints only with
`wide` - and properties over a sweep of B against the uniform plan (tests/test_attention_plan.py)."""
import pytest

import attention_forms as A
from test_attention_plan import _KS, _SHAPES, _base

NONE = ('none', 0, 0)
# (B, Np, Mp, topk) -> (name, split, tiles) without the tap; a dynamic case is pinned with it too: the ,TAP form, the same geometry
# units = 8 B (pair x frame x head); attention_kernel: split = min(ceil(512 / units), qtiles), tiles of 256 queries (128: dyn<16>)
NARROW = [
    ((2, 40, 100, 0), ('full<4>', 1, 1)),                # 4 key blocks; 1 tile
    ((2, 300, 500, 64), ('dyn<16>', 4, 1)),              # 16 key blocks; 4 tiles of 128, ceil(512 / 16) = 32 -> 4
    ((64, 300, 500, 64), ('dyn<16>', 1, 4)),             # ceil(512 / 512) = 1
    ((24, 300, 500, 64), ('dyn<16>', 3, 2)),             # ceil(512 / 192) = 3
    ((2, 512, 512, 0), ('full<8>', 2, 1)),               # not the stream kernel: it takes no counts; 2 tiles of 256
    ((2, 512, 512, 128), ('dyn<16>', 4, 1)),             # not topk16<512>
    ((2, 256, 256, 64), ('dyn<8>', 1, 1)),               # not topk16<256>; 8 key blocks, 1 tile of 256
    ((2, 64, 64, 64), ('dyn<4>', 1, 1)),                 # k == N == M stays dynamic: a pair may have fewer keys than its slot
    ((2, 40, 56, 57), ('dyn<4>', 1, 1)),                 # k against the counts is the caller's check, not the plan's
    ((2, 200, 130, 64), ('dyn<8>', 1, 1)),
    ((2, 33, 31, 0), ('full<4>', 1, 1)),
    ((2, 257, 130, 0), ('full<8>', 2, 1)),
    ((63, 300, 500, 0), ('full<8>', 2, 1)),              # ceil(512 / 504) = 2
    ((64, 300, 500, 0), ('full<8>', 1, 2)),
    ((0, 64, 64, 0), NONE),                              # an empty batch
    ((2, 0, 64, 0), NONE),
    ((2, 64, 64, -1), NONE),
]
# the slots only `wide` takes: refused without it
BEYOND = [
    ((2, 513, 100, 0), ('full<8,windowed>', 3, 1)),      # 17 key blocks: a workgroup per tile of 256, ceil(513 / 256) = 3
    ((1, 700, 600, 100), ('wide<4>', 11, 1)),            # 22 key blocks: passes of 64 queries, ceil(700 / 64) = 11
    ((2, 513, 40, 8), ('wide<4>', 9, 1)),                # ceil(513 / 64)
    ((9, 1024, 1024, 128), ('wide<4>', 16, 1)),          # 32 key blocks: still four waves per tile
    ((1, 1025, 40, 8), ('wide<8>', 33, 1)),              # 33 key blocks: passes of 32 queries, ceil(1025 / 32) = 33
    ((1, 1500, 520, 64), ('wide<8>', 47, 1)),            # ceil(1500 / 32)
    ((1, 2048, 2048, 64), ('wide<8>', 64, 1)),
    ((1, 2048, 2048, 0), ('full<8,windowed>', 8, 1)),
    ((64, 600, 700, 0), ('full<8,windowed>', 3, 1)),     # whatever B is
]
REFUSED = [(1, 2049, 100, 0), (1, 100, 2049, 8)]         # beyond MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS


def _check(case, want, wide):
    B, Np, Mp, k = case
    for tap in (False, True):
        form, split, tiles = A.ragged_plan(B, Np, Mp, k, tap, wide)
        name = want[0] + ',TAP' if tap and want[0] in A.DYN else want[0]
        assert (A.name(form), split, tiles) == (name, *want[1:]), (case, tap, wide)


@pytest.mark.parametrize('case,want', NARROW, ids=[f'{c[0]}x{c[1]}x{c[2]}-k{c[3]}' for c, _ in NARROW])
def test_pinned_cases_within_512(case, want):
    _check(case, want, wide=False)
    _check(case, want, wide=True)       # ... run the same thing with the opt-in


@pytest.mark.parametrize('case,want', BEYOND, ids=[f'{c[0]}x{c[1]}x{c[2]}-k{c[3]}' for c, _ in BEYOND])
def test_pinned_cases_beyond_512(case, want):
    _check(case, NONE, wide=False)
    _check(case, want, wide=True)


def test_pinned_refusals():
    for case in REFUSED:
        _check(case, NONE, wide=False)
        _check(case, NONE, wide=True)


def test_properties_over_a_sweep_of_the_batch():
    assert all(max(s) <= 2048 for s in _SHAPES)
    seen = set()
    for Np, Mp in _SHAPES:
        narrow = max(Np, Mp) <= 512
        for k in _KS:
            for tap in (False, True):
                first = A.ragged_plan(1, Np, Mp, k, tap, True)[0]
                for B in range(1, 131):
                    form, split, tiles = A.ragged_plan(B, Np, Mp, k, tap, True)
                    what = f'B={B} {Np}x{Mp} k={k} tap={tap}: {A.name(form)} {split}/{tiles}'
                    # from the slots alone: never B
                    assert form == first and 0 <= form < 23, what
                    seen.add(form)
                    # only forms whose kernel has a RAGGED instantiation; dynamic whenever k > 0; the tap's twin where there is one
                    base = _base(form)
                    assert base in A.RAGGED and (base in A.DYN) == (k > 0) and (',TAP' in A.NAMES[form]) == (tap and k > 0), what
                    assert (base in A.RAGGED_WIDE_ONLY) == (not narrow), what
                    # without the opt-in: the same within 512 x 512, refused beyond
                    assert A.ragged_plan(B, Np, Mp, k, tap, False) == ((form, split, tiles) if narrow else (-1, 0, 0)), what
                    # the uniform launch's geometry for the slots, wherever that launch runs a kernel with a RAGGED instantiation
                    uform, usplit, utiles = A.plan(B, Np, Mp, k, tap)
                    if uform >= 0 and _base(uform) in A.RAGGED:
                        assert (split, tiles) == (usplit, utiles), what
                        assert form == uform or k == Np == Mp, what
    assert {_base(f) for f in seen} == set(A.RAGGED) and len(seen) == 13, sorted(seen)
