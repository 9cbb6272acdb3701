"""The fp32-class layer launcher's choice of instantiation and launch geometry (csrc/layer.hip: layer_plan, exported as mdgat_layer_plan)
as a pure function of the launch and the mdgat_set_layer_split_tiles value: no device.  Pins both sides of the two thresholds under every
split setting, the V^T store path of every family, the grid, every case tests/test_gpu_layer_forms.py runs, and - over a brute-force
sweep - that the 14 indices of the table and no others are reached."""
import itertools

import pytest

import layer_forms as LF

MODES = [(0, 1), (0, 2), (1, 1), (1, 2)]        # (do_mlp, mode3)


@pytest.fixture()
def split_tiles():
    """set(tiles) for the test; the value found is put back afterwards."""
    lib = LF._lib()
    prev = lib.mdgat_set_layer_split_tiles(-1)
    try:
        yield lib.mdgat_set_layer_split_tiles
    finally:
        lib.mdgat_set_layer_split_tiles(prev)


# R = 8192 | 8193: 64 | 65 tiles of 128 keypoints, 16384 | 16385: 128 | 129
@pytest.mark.parametrize('setting,want', [
    (None, {8192: 'split', 8193: 'NW=4', 16384: 'NW=4', 16385: 'NW=8'}),          # the default: split up to 64 tiles
    (0, {1: 'NW=4', 8192: 'NW=4', 8193: 'NW=4', 16384: 'NW=4', 16385: 'NW=8'}),   # never split
    (1 << 20, {8192: 'split', 8193: 'split', 16384: 'split', 16385: 'split'}),    # always
    (-1, {8192: 'split', 8193: 'NW=4', 16384: 'NW=4', 16385: 'NW=8'}),            # back to the default
    (100, {12800: 'split', 12801: 'NW=4', 16384: 'NW=4', 16385: 'NW=8'}),         # a threshold of one's own
    (200, {16385: 'split', 25600: 'split', 25601: 'NW=8'}),                       # ... beyond the 64-keypoint family: it is never reached
])
def test_both_sides_of_each_threshold(split_tiles, setting, want):
    if setting is not None:
        split_tiles(7)                  # (so that -1 has something to undo)
        split_tiles(setting)
    for R, fam in want.items():
        for do_mlp, mode3 in MODES:
            for N, M in ((128, 128), (61, 66)):
                form, wg, kp, vs = LF.plan(R, N, M, do_mlp, mode3)
                assert LF.family(LF.name(form)) == fam, (setting, R, N, M, do_mlp, mode3, LF.name(form))
                assert kp == LF.KEYPOINTS[fam] and wg == -(-R // kp)


def test_set_returns_the_previous_value_and_negative_restores_the_default(split_tiles):
    assert split_tiles(5) == LF.SPLIT_TILES_DEFAULT
    assert split_tiles(-3) == 5
    assert split_tiles(0) == LF.SPLIT_TILES_DEFAULT
    assert split_tiles(-1) == 0


# (N, M) -> V^T store path by family
V_STORE = {(128, 128): {'split': 4, 'NW=4': 16, 'NW=8': 128}, (48, 64): {'split': 4, 'NW=4': 16, 'NW=8': 16},
           (60, 56): {'split': 4, 'NW=4': 4, 'NW=8': 4}, (61, 66): {'split': 1, 'NW=4': 1, 'NW=8': 1},
           # one frame decides: the coarser of the two
           (128, 64): {'split': 4, 'NW=4': 16, 'NW=8': 16}, (256, 384): {'split': 4, 'NW=4': 16, 'NW=8': 128}, (128, 4): {'split': 4, 'NW=4': 4, 'NW=8': 4},
           (16, 3): {'split': 1, 'NW=4': 1, 'NW=8': 1}}
# family -> (mdgat_set_layer_split_tiles value, R)
REACH = {'split': (1 << 20, 20000), 'NW=4': (0, 16384), 'NW=8': (0, 16385)}


@pytest.mark.parametrize('fam', ['split', 'NW=4', 'NW=8'])
def test_vw_and_v_store(split_tiles, fam):
    tiles, R = REACH[fam]
    split_tiles(tiles)
    for (N, M), want in V_STORE.items():
        for do_mlp, mode3 in MODES:
            form, wg, kp, vs = LF.plan(R, N, M, do_mlp, mode3)
            nm = LF.name(form)
            assert LF.family(nm) == fam
            # VW holds only for NW = 8, q | k | v, and N, M both multiples of 128
            vw = int(fam == 'NW=8' and mode3 == 1 and N % 128 == 0 and M % 128 == 0)
            assert nm == LF.form_name(fam, do_mlp, mode3, vw), (fam, N, M, do_mlp, mode3, nm)
            assert vs == (want[fam] if mode3 == 1 else 0), (fam, N, M, do_mlp, mode3, vs)
            assert (vs == 128) == bool(vw)


def test_no_launch():
    for R in (0, -1, -128):
        assert LF.plan(R, 64, 64, 1, 1) == (-1, 0, 0, 0)
    assert LF.name(-1) == 'none'


def test_names_and_indices():
    assert len(LF.NAMES) == 14 and len(set(LF.NAMES)) == 14
    assert LF.NAMES[1] == 'split<0,2>' and LF.NAMES[5] == 'layer<0,2,0,4>' and LF.NAMES[10] == 'layer<0,2,0,8>' and LF.NAMES[12] == 'layer<1,1,1,8>'
    assert LF.counts().shape == (14,)       # (readable without a device)
    assert LF.SPLIT_TILES_DEFAULT == 64 and LF.TILE64_TILES == 128


def test_brute_force_sweep_reaches_the_14_forms_and_no_other(split_tiles):
    seen = set()
    Rs = [1, 31, 32, 33, 64, 65, 127, 128, 129, 8191, 8192, 8193, 16383, 16384, 16385, 16637, 40000]
    NM = [1, 3, 4, 12, 16, 48, 61, 64, 128, 256]
    for tiles in (None, 0, 1, 1 << 20):
        split_tiles(-1 if tiles is None else tiles)
        thr = LF.SPLIT_TILES_DEFAULT if tiles is None else tiles
        for R, N, M, (do_mlp, mode3) in itertools.product(Rs, NM, NM, MODES):
            form, wg, kp, vs = LF.plan(R, N, M, do_mlp, mode3)
            what = f'tiles={tiles} R={R} {N}x{M} <{do_mlp},{mode3}>: {LF.name(form)} {wg} x {kp}, v_store {vs}'
            assert 0 <= form < 14, what
            seen.add(form)
            # the family by the launch size alone, the instantiation within it by the arguments
            t = -(-R // 128)
            fam = 'split' if t <= thr else 'NW=4' if t <= LF.TILE64_TILES else 'NW=8'
            vw = int(fam == 'NW=8' and mode3 == 1 and (N | M) % 128 == 0)
            assert LF.name(form) == LF.form_name(fam, do_mlp, mode3, vw), what
            # every keypoint row has a workgroup, and no workgroup is without one
            assert kp == LF.KEYPOINTS[fam] and wg == -(-R // kp) and (wg - 1) * kp < R <= wg * kp, what
            run = 16 if (N | M) % 16 == 0 else 4 if (N | M) % 4 == 0 else 1
            assert vs == (0 if mode3 != 1 else 128 if vw else min(run, 4) if fam == 'split' else run), what
    assert seen == set(range(14)), sorted(seen)


def test_mode3_other_than_1_is_final_proj():
    """launch_layer reads `mode3 != 1` as final_proj; the plan agrees for any value."""
    for mode3 in (0, 2, 3, -1):
        assert LF.plan(16385, 128, 128, 1, mode3) == LF.plan(16385, 128, 128, 1, 2)
        assert LF.plan(100, 61, 66, 0, mode3) == LF.plan(100, 61, 66, 0, 2)


@pytest.mark.parametrize('case', LF.CASES, ids=LF.case_id)
def test_cases_of_the_gpu_test(split_tiles, case):
    fam, how, B, n, m, v_store = case
    R = B * (n + m)
    with LF.forced(how):
        got = [LF.plan(R, n, m, do_mlp, mode3) for do_mlp, mode3 in ((0, 1), (1, 1), (1, 2))]
        assert LF.forward_plan(B, n, m, 1) == LF.case_forms(case)
    vw = int(v_store == 128)
    assert [LF.name(g[0]) for g in got] == [LF.form_name(fam, 0, 1, vw), LF.form_name(fam, 1, 1, vw), LF.form_name(fam, 1, 2)]
    assert [g[3] for g in got] == [v_store, v_store, 0]
    assert all(g[1:3] == (-(-R // LF.KEYPOINTS[fam]), LF.KEYPOINTS[fam]) for g in got)
    if fam == 'NW=8':
        assert R > 128 * LF.TILE64_TILES and R - 128 * LF.TILE64_TILES <= 2 * (n + m)  # within two pairs of the smallest batch that reaches the family
        assert R % 128 != 0 or (n | m) % 128 == 0                                   # a partial last tile wherever the shape allows one
    else:
        assert -(-R // 64) <= 6 and (R % 64 != 0 or (n, m) == (128, 128))


@pytest.mark.parametrize('case', LF.CASES_F64, ids=LF.case_id)
def test_cases_of_the_gpu_test_final_proj_only(split_tiles, case):
    fam, how, B, n, m = case
    with LF.forced(how):
        # every layer in fp64 (first = 2 L): the one fp32-class layer launch is <0,2,...>
        assert LF.forward_plan(B, n, m, 1, first=2) == {LF.form_name(fam, 0, 2): 1}


def test_the_two_case_tables_reach_every_form(split_tiles):
    seen = set()
    for c in LF.CASES:
        seen |= set(LF.case_forms(c))
    seen |= {LF.form_name(c[0], 0, 2) for c in LF.CASES_F64}
    assert seen == set(LF.NAMES)
