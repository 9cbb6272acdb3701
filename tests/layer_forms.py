"""The 14 instantiations launch_layer (csrc/layer.hip, csrc/layer_split.hip) can reach, as the tests name them, and the two symbols that
make the launcher's choice observable: mdgat_layer_plan (the choice and its launch geometry as a pure function of the launch and the
current mdgat_set_layer_split_tiles value; no device) and mdgat_layer_launches (launches so far by index).  The table of indices:
include/mdgat_hip.h.

split<DO_MLP,MODE3> (0-3): layer_split_kernel, 32 keypoints per workgroup; layer<DO_MLP,MODE3,VW,NW>: layer_kernel with 64 (NW = 4: 4-7)
or 128 (NW = 8: 8-13) keypoints per workgroup.  DO_MLP 0: projection only; MODE3 1: q | k | v of the next layer, 2: final_proj."""
import ctypes as C

import numpy as np

SPLIT = ('split<0,1>', 'split<0,2>', 'split<1,1>', 'split<1,2>')
NW4 = ('layer<0,1,0,4>', 'layer<0,2,0,4>', 'layer<1,1,0,4>', 'layer<1,2,0,4>')
NW8 = ('layer<0,1,0,8>', 'layer<0,1,1,8>', 'layer<0,2,0,8>', 'layer<1,1,0,8>', 'layer<1,1,1,8>', 'layer<1,2,0,8>')
NAMES = SPLIT + NW4 + NW8
FAMILIES = {'split': SPLIT, 'NW=4': NW4, 'NW=8': NW8}
KEYPOINTS = {'split': 32, 'NW=4': 64, 'NW=8': 128}      # per workgroup
SPLIT_TILES_DEFAULT = 64                                # mdgat_set_layer_split_tiles(-1)
TILE64_TILES = 128                                      # launches of more 128-keypoint tiles: NW = 8
# mdgat_set_layer_split_tiles value that forces a family on a launch of any size the tests run (None: the default dispatch)
FORCE = {'split': 1 << 20, 'whole': 0, 'default': None}


# The cases of tests/test_gpu_layer_forms.py - the smallest launch that reaches every form, with Npad != N where the path allows it -
# as (family, how it is forced, B, n, m, V^T store path of its q | k | v launches).  tests/test_layer_plan.py holds every one of them to
# the plan, so the table cannot rot.  R = B (n + m) rows in one launch; tiles = ceil(R / 128).
CASES = [
    # NW = 8 by the default dispatch: more than 128 tiles
    ('NW=8', 'default', 65, 128, 128, 128),     # R = 16640, 130 tiles: the gather buffers (VW)
    ('NW=8', 'default', 147, 48, 64, 16),       # 16464, 129: Npad 64 != 48; the last tile has 80 rows (three empty waves); workgroups straddle pairs
    ('NW=8', 'default', 142, 60, 56, 4),        # 16472, 129: waves straddle the frame boundary; the last wave is half valid
    ('NW=8', 'default', 131, 61, 66, 1),        # 16637, 130: odd P = 127, every workgroup straddles pairs; the last tile has 125 rows
    # NW = 4 with the split kernel off: at most 6 workgroups of 64 keypoints, the last one partial
    ('NW=4', 'whole', 1, 128, 128, 16),         # (no VW at NW = 4: whole 32-byte row pieces)
    ('NW=4', 'whole', 3, 48, 64, 16),
    ('NW=4', 'whole', 3, 60, 56, 4),
    ('NW=4', 'whole', 3, 61, 66, 1),
    # the split kernel, forced (the default dispatch reaches it too at these sizes)
    ('split', 'split', 3, 60, 56, 4),
    ('split', 'split', 3, 61, 66, 1),
]
# ... and of the projection-only final_proj launch <0,2,...> that only the exact mode with every layer in fp64 issues
CASES_F64 = [('NW=8', 'default', 131, 61, 66), ('NW=4', 'whole', 3, 61, 66), ('split', 'split', 3, 61, 66)]


def case_id(c):
    return f'{c[0]}-{c[2]}x{c[3]}x{c[4]}'


def case_forms(c, L=1):
    """{name: launches} a tapped fp32-class forward of L layers of case c is there for: <0,1>, 2 L - 1 times <1,1>, <1,2>."""
    fam, vw = c[0], int(c[5] == 128)
    want = {form_name(fam, 0, 1, vw): 1, form_name(fam, 1, 2): 1}
    if L > 0:
        want[form_name(fam, 1, 1, vw)] = 2 * L - 1
    return want


def family(name):
    return next(f for f, names in FAMILIES.items() if name in names)


def form_name(fam, do_mlp, mode3, vw=0):
    """The name of instantiation <do_mlp, mode3(, vw, NW)> of a family."""
    return f'split<{do_mlp},{mode3}>' if fam == 'split' else f'layer<{do_mlp},{mode3},{vw},{4 if fam == "NW=4" else 8}>'


def _lib():
    from mdgat_matcher_amd import _lib
    return _lib.load()


def plan(R, N, M, do_mlp, mode3):
    """(form, workgroups, keypoints per workgroup, v_store) launch_layer chooses for R rows of pairs of N + M keypoints under the current
    mdgat_set_layer_split_tiles value: the index (-1: no launch), the grid, and the V^T store path (0 none, 1, 4, 16, 128)."""
    wg, kp, vs = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    form = _lib().mdgat_layer_plan(R, N, M, do_mlp, mode3, C.byref(wg), C.byref(kp), C.byref(vs))
    return form, wg.value, kp.value, vs.value


def name(i):
    return 'none' if i < 0 else NAMES[i]


def forward_plan(B, n, m, L, first=0):
    """{name: launches} of one fp32-class forward of B pairs of n x m keypoints that runs unsliced (a tapped run): one projection-only
    launch in front of layer `first` (final_proj when first == 2 L: every layer in fp64), then one launch per layer from `first` on."""
    R, want = B * (n + m), {}
    launches = [(0, 2 if first == 2 * L else 1)] + [(1, 1 if i + 1 < 2 * L else 2) for i in range(first, 2 * L)]
    for do_mlp, mode3 in launches:
        nm = name(plan(R, n, m, do_mlp, mode3)[0])
        want[nm] = want.get(nm, 0) + 1
    return want


class forced:
    """``with forced('split' | 'whole' | 'default'):`` - every launch inside on layer_split_kernel / on layer_kernel / by the default
    threshold; the previous mdgat_set_layer_split_tiles value comes back on the way out."""

    def __init__(self, how):
        self.tiles = FORCE[how]

    def __enter__(self):
        self.prev = _lib().mdgat_set_layer_split_tiles(-1 if self.tiles is None else self.tiles)
        return self

    def __exit__(self, *exc):
        _lib().mdgat_set_layer_split_tiles(self.prev)


def counts():
    buf = (C.c_uint64 * len(NAMES))()
    _lib().mdgat_layer_launches(buf)
    return np.array(list(buf), dtype=np.int64)


class watch:
    """``with watch() as w: ...`` - afterwards w.delta[i] = launches of instantiation i in between (as numpy int64 [14])."""

    def __enter__(self):
        self.before = counts()
        self.delta = None
        return self

    def __exit__(self, *exc):
        self.delta = counts() - self.before

    def launched(self):
        return {NAMES[i]: int(n) for i, n in enumerate(self.delta) if n}


def assert_launched(w, want, what):
    """The watched region launched exactly ``want`` - {name or index: times}, or one name or index for a single launch - and no other."""
    if not isinstance(want, dict):
        want = {want: 1}
    want = {(NAMES[k] if isinstance(k, (int, np.integer)) else k): n for k, n in want.items()}
    assert w.launched() == want, f'{what}: wanted {want}, launched {w.launched()}'
