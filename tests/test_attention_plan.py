"""The fp32-class attention launcher's choice of instantiation and launch geometry (csrc/attention.hip: attention_plan, exported as
mdgat_attention_plan) as a pure function: no device.  Pins a table worked by hand - every geometry tests/test_gpu_attention_geometry.py
runs, the benchmark's shapes, the thresholds on B where the split changes - and properties over a sweep of B."""
import pytest

import attention_forms as A

# (B, N, M, topk, tap) -> (name, split, tiles)
# units = 8 B (pair x frame x head); attention_kernel: qsplit = min(ceil(512 / units), qtiles), tiles of 256 queries (128: dyn<16>);
# topk16: qsplit = min(ceil(512 / units), qmax), qmax = 4 (256 keys from B = 16 on: 2), 32 (16) tiles of 16 queries
TABLE = [
    # ---- the geometries of tests/test_gpu_attention_geometry.py ----
    ((64, 300, 500, 0, False), ('full<8>', 1, 2)),                  # 2 tiles of 256; ceil(512 / 512) = 1
    ((64, 300, 500, 64, False), ('dyn<16>', 1, 4)),                 # 4 tiles of 128
    ((64, 300, 500, 64, True), ('dyn<16>,TAP', 1, 4)),
    ((40, 300, 500, 64, False), ('dyn<16>', 2, 2)),                 # ceil(512 / 320) = 2
    ((40, 300, 500, 64, True), ('dyn<16>,TAP', 2, 2)),
    ((24, 300, 500, 64, False), ('dyn<16>', 3, 2)),                 # ceil(512 / 192) = 3: workgroup 0 walks tiles 0 and 3
    ((24, 300, 500, 64, True), ('dyn<16>,TAP', 3, 2)),
    ((64, 512, 512, 128, False), ('topk16<512>', 1, 32)),           # (the benchmark's shape)
    ((64, 512, 512, 128, True), ('topk16<512>,TAP', 1, 32)),
    ((64, 512, 512, 64, False), ('topk16<512>', 1, 32)),            # (the benchmark's other k)
    ((64, 512, 512, 64, True), ('topk16<512>,TAP', 1, 32)),
    ((40, 512, 512, 128, False), ('topk16<512>', 2, 16)),
    ((40, 512, 512, 64, True), ('topk16<512>,TAP', 2, 16)),
    ((24, 512, 512, 128, False), ('topk16<512>', 3, 11)),           # ceil(32 / 3) = 11: the last part is cut short at 10 tiles
    ((24, 512, 512, 64, True), ('topk16<512>,TAP', 3, 11)),
    ((64, 256, 256, 128, False), ('topk16<256>', 1, 16)),
    ((64, 256, 256, 128, True), ('topk16<256>,TAP', 1, 16)),
    ((16, 256, 256, 128, False), ('topk16<256>', 2, 8)),
    ((16, 256, 256, 128, True), ('topk16<256>,TAP', 2, 8)),
    ((9, 700, 600, 100, False), ('wide<4>', 11, 1)),                # ceil(700 / 64) passes, one workgroup each
    ((9, 700, 600, 100, True), ('wide<4>,TAP', 11, 1)),
    ((9, 512, 448, 0, False), ('stream', 4, 1)),                    # 512 / 128
    ((9, 600, 700, 0, False), ('full<8,windowed>', 3, 1)),          # ceil(700 / 256)
    # ... and the same pairs alone (the batch-independence check runs them at B = 1)
    ((1, 300, 500, 0, False), ('full<8>', 2, 1)),
    ((1, 300, 500, 64, False), ('dyn<16>', 4, 1)),
    ((1, 300, 500, 64, True), ('dyn<16>,TAP', 4, 1)),
    ((1, 512, 512, 128, False), ('topk16<512>', 4, 8)),
    ((1, 512, 512, 64, True), ('topk16<512>,TAP', 4, 8)),
    ((1, 256, 256, 128, False), ('topk16<256>', 4, 4)),
    ((1, 256, 256, 128, True), ('topk16<256>,TAP', 4, 4)),
    ((1, 700, 600, 100, False), ('wide<4>', 11, 1)),
    ((1, 512, 448, 0, False), ('stream', 4, 1)),
    ((1, 600, 700, 0, False), ('full<8,windowed>', 3, 1)),
    # ---- 64 x 256 x 256 ----
    ((64, 256, 256, 0, False), ('stream', 2, 1)),
    ((64, 256, 256, 64, False), ('topk16<256>', 1, 16)),
    # ---- k == N == M: full attention, with or without the tap ----
    ((2, 64, 64, 64, True), ('stream', 1, 1)),
    ((3, 100, 100, 100, False), ('full<4>', 1, 1)),
    ((3, 100, 100, 100, True), ('full<4>', 1, 1)),
    ((64, 300, 300, 300, False), ('full<8>', 1, 2)),
    ((2, 513, 513, 512, False), ('wide<4>', 9, 1)),                 # (k one below: dynamic)
    # ---- both frames multiples of 64: the streamed kernel whatever B is ----
    ((1, 512, 512, 0, False), ('stream', 4, 1)),
    ((22, 512, 512, 0, False), ('stream', 4, 1)),
    ((64, 512, 512, 0, False), ('stream', 4, 1)),
    ((130, 128, 320, 0, False), ('stream', 3, 1)),
    ((64, 2048, 1344, 0, False), ('stream', 16, 1)),
    ((64, 64, 64, 0, False), ('stream', 1, 1)),
    # ---- more than 512 keys, full: the windowed form, one tile per workgroup ----
    ((2, 600, 700, 0, False), ('full<8,windowed>', 3, 1)),
    ((64, 2048, 1300, 0, False), ('full<8,windowed>', 8, 1)),
    ((1, 2100, 2100, 0, False), ('full<8,windowed>', 9, 1)),
    # ---- refusals ----
    ((1, 2100, 2100, 8, False), ('none', 0, 0)),                    # top-k over more than 2048 keys
    ((1, 2049, 100, 8, True), ('none', 0, 0)),
    ((1, 2048, 2048, 64, False), ('wide<8>', 64, 1)),
    ((2, 40, 56, 57, False), ('none', 0, 0)),                       # k > both frames
    ((2, 40, 56, 41, False), ('none', 0, 0)),                       # k > the smaller frame
    ((2, 40, 56, 40, False), ('dyn<4>', 1, 1)),
    ((0, 64, 64, 0, False), ('none', 0, 0)),
    ((2, 0, 64, 0, False), ('none', 0, 0)),
    ((2, 64, 64, -1, False), ('none', 0, 0)),
    # ---- the thresholds on B: the 512-key form ----
    ((21, 512, 512, 128, False), ('topk16<512>', 4, 8)),            # ceil(512 / 168) = 4
    ((22, 512, 512, 128, False), ('topk16<512>', 3, 11)),           # ceil(512 / 176) = 3
    ((31, 512, 512, 128, False), ('topk16<512>', 3, 11)),           # ceil(512 / 248) = 3
    ((32, 512, 512, 128, False), ('topk16<512>', 2, 16)),
    ((63, 512, 512, 128, False), ('topk16<512>', 2, 16)),           # ceil(512 / 504) = 2
    ((64, 512, 512, 128, False), ('topk16<512>', 1, 32)),
    ((512, 512, 512, 128, False), ('topk16<512>', 1, 32)),
    # ---- ... the 256-key form: at most 256 / 128 = 2 once 16 B units fill 256 workgroups ----
    ((15, 256, 256, 128, False), ('topk16<256>', 4, 4)),
    ((16, 256, 256, 128, False), ('topk16<256>', 2, 8)),
    ((63, 256, 256, 128, False), ('topk16<256>', 2, 8)),
    ((64, 256, 256, 128, False), ('topk16<256>', 1, 16)),
    # ---- ... attention_kernel: the second tile of a workgroup ----
    ((21, 300, 500, 64, False), ('dyn<16>', 4, 1)),
    ((22, 300, 500, 64, False), ('dyn<16>', 3, 2)),
    ((63, 300, 500, 0, False), ('full<8>', 2, 1)),
    ((64, 300, 500, 0, False), ('full<8>', 1, 2)),
    # ---- the other kernels, and the tap's effect on the choice ----
    ((2, 40, 100, 8, False), ('dyn<4>', 1, 1)),
    ((2, 40, 100, 8, True), ('dyn<4>,TAP', 1, 1)),
    ((2, 200, 130, 64, False), ('dyn<8>', 1, 1)),
    ((2, 200, 130, 64, True), ('dyn<8>,TAP', 1, 1)),
    ((2, 1024, 1024, 128, True), ('wide<4>,TAP', 16, 1)),
    ((1, 1500, 520, 64, False), ('wide<8>', 47, 1)),                # ceil(1500 / 32)
    ((1, 1500, 520, 64, True), ('wide<8>,TAP', 47, 1)),
    ((2, 33, 31, 0, False), ('full<4>', 1, 1)),
    ((2, 257, 130, 0, False), ('full<8>', 2, 1)),
]

# mode 1 (F16): (B, N, M, topk, tap) -> name
TABLE_F16 = [
    ((64, 512, 512, 128, False), 'topk16<512>,FAST'), ((64, 512, 512, 128, True), 'topk16<512>,TAP,FAST'),
    ((64, 256, 256, 128, False), 'topk16<256>,FAST'), ((64, 256, 256, 128, True), 'topk16<256>,TAP,FAST'),
    ((64, 512, 512, 0, False), 'stream,FAST'),
    # no FAST form: the split-f16 kernel
    ((64, 300, 500, 0, False), 'full<8>'), ((64, 300, 500, 64, True), 'dyn<16>,TAP'), ((2, 1024, 1024, 128, False), 'wide<4>'),
]


@pytest.mark.parametrize('case,want', TABLE, ids=[f'{c[0]}x{c[1]}x{c[2]}-k{c[3]}{"-tap" if c[4] else ""}' for c, _ in TABLE])
def test_pinned_cases(case, want):
    form, split, tiles = A.plan(*case)
    assert (A.name(form), split, tiles) == want


def test_pinned_cases_f16():
    for case, want in TABLE_F16:
        form, split, tiles = A.plan(*case, mode=1)
        assert A.name(form) == want, case
        # the geometry is the split-f16 launch's
        assert (split, tiles) == A.plan(*case)[1:], case
        assert A.SPLIT_TWIN.get(form, form) == A.plan(*case)[0], case


def test_names_and_indices():
    assert len(A.NAMES) == 23 and len(set(A.NAMES)) == 23
    assert A.NAMES[0] == 'stream' and A.NAMES[8] == 'topk16<512>' and A.NAMES[15] == 'topk16<512>,TAP' and A.NAMES[20] == 'topk16<512>,FAST'
    assert A.index('topk16<256>') == 7 and A.index('topk16<256>', tap=True) == 14 and A.index('full<8>', tap=True) == 2
    assert A.MODE0 == tuple(range(18))
    assert A.SPLIT_TWIN == {18: 0, 19: 7, 20: 8, 21: 14, 22: 15}
    assert A.counts().shape == (23,)        # (readable without a device)


_SHAPES = [(64, 64), (40, 56), (128, 96), (200, 130), (257, 130), (256, 256), (300, 500), (500, 300), (512, 512), (512, 448), (513, 513), (600, 700),
           (1024, 1024), (1500, 520), (130, 2048), (2048, 2048)]
_KS = (0, 1, 30, 64, 128)


def _base(form):
    return A.NAMES[form].replace(',FAST', '').replace(',TAP', '')


def test_properties_over_a_sweep_of_the_batch():
    seen = set()
    for N, M in _SHAPES:
        qmax = max(N, M)
        for k in _KS:
            for tap in (False, True):
                for mode in (0, 1):
                    for B in range(1, 131):
                        form, split, tiles = A.plan(B, N, M, k, tap, mode)
                        what = f'B={B} {N}x{M} k={k} tap={tap} mode={mode}: {A.name(form)} {split}/{tiles}'
                        if k > min(N, M):
                            assert (form, split, tiles) == (-1, 0, 0), what
                            continue
                        assert 0 <= form < 23, what
                        seen.add(form)
                        assert (form in A.MODE0) == (mode == 0 or form not in A.SPLIT_TWIN), what
                        base = _base(form)
                        assert (k > 0 and not (k == N == M)) == (base in A.DYN), what
                        assert (',TAP' in A.NAMES[form]) == (tap and base in A.DYN), what
                        qtiles = -(-qmax // A.TILE_QUERIES[base])
                        assert split >= 1 and tiles >= 1, what
                        # every query tile of the larger frame has a workgroup, and no workgroup is without a tile
                        assert split * tiles >= qtiles and split * (tiles - 1) < qtiles, what
                        if B <= 3:
                            # THE GAP tests/test_gpu_attention_geometry.py closes: at the batch sizes of tests/test_gpu_ops.py no
                            # workgroup walks a second tile - in the 16-query kernels no WAVE does (a tile per wave of the workgroup)
                            assert tiles <= A.WAVES16 if base.startswith('topk16') else tiles == 1, what
    assert seen == set(range(23)), sorted(seen)


def test_the_split_only_falls_with_the_batch():
    for N, M in _SHAPES:
        for k in (0, 64):
            if k > min(N, M):
                continue
            last = None
            for B in range(1, 131):
                form, split, tiles = A.plan(B, N, M, k)
                if last is not None:
                    assert form == last[0] and split <= last[1] and tiles >= last[2], (B, N, M, k)
                last = (form, split, tiles)
