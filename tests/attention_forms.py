"""The 23 instantiations launch_attention (csrc/attention.hip, csrc/attention_stream.hip) can reach, as the tests name them, and the
symbols that make the launcher's choice observable: mdgat_attention_plan and, for a ragged batch, mdgat_attention_ragged_plan (the choice
and its launch geometry as a pure function; no device) and mdgat_attention_launches (launches so far by index).  The table of indices: include/mdgat_hip.h.

mode 0 (split-f16): 0 stream, 1-3 the full forms of attention_kernel, 4-10 the dynamic kernels, 11-17 their TAP twins (a selection buffer
is passed); mode 1 (F16): 18-22 the FAST twins of the kernels that have one (stream, topk16 and its TAP twin)."""
import ctypes as C

import numpy as np

FULL = ('stream', 'full<4>', 'full<8>', 'full<8,windowed>')
DYN = ('dyn<4>', 'dyn<8>', 'dyn<16>', 'topk16<256>', 'topk16<512>', 'wide<4>', 'wide<8>')
FAST = ('stream,FAST', 'topk16<256>,FAST', 'topk16<512>,FAST', 'topk16<256>,TAP,FAST', 'topk16<512>,TAP,FAST')
NAMES = FULL + DYN + tuple(n + ',TAP' for n in DYN) + FAST
MODE0 = tuple(range(len(FULL) + 2 * len(DYN)))       # the indices a split-f16 launch can reach
# queries of one tile (wide kernels: of one workgroup pass), by the kernel's name without its TAP / FAST suffixes
TILE_QUERIES = {'stream': 128, 'full<4>': 256, 'full<8>': 256, 'full<8,windowed>': 256, 'dyn<4>': 256, 'dyn<8>': 256, 'dyn<16>': 128,
                'topk16<256>': 16, 'topk16<512>': 16, 'wide<4>': 64, 'wide<8>': 32}
WAVES16 = 8                                          # waves of a topk16 workgroup: each claims 16-query tiles from the workgroup's counter
# FAST index -> the split-f16 index of the same kernel
SPLIT_TWIN = {NAMES.index(f): NAMES.index(f[:-len(',FAST')]) for f in FAST}


def index(name, tap=False):
    """The index of ``name``; tap: of its TAP twin where it has one (the full forms have none: a tap run launches the same kernel)."""
    return NAMES.index(name + ',TAP' if tap and name in DYN else name)


def _lib():
    from mdgat_matcher_amd import _lib
    return _lib.load()


def plan(B, N, M, topk=0, tap=False, mode=0):
    """(form, split, tiles) launch_attention chooses: the index (-1: no launch), the workgroups that share the query tiles of one
    (pair, frame, head), and the most query tiles one of them walks."""
    split, tiles = C.c_int(-7), C.c_int(-7)
    form = _lib().mdgat_attention_plan(B, N, M, topk, int(tap), mode, C.byref(split), C.byref(tiles))
    return form, split.value, tiles.value


# the forms whose kernel has a RAGGED instantiation (a call with counts); WIDE_ONLY: those only a slot beyond 512 keypoints reaches
RAGGED = ('full<4>', 'full<8>', 'full<8,windowed>', 'dyn<4>', 'dyn<8>', 'dyn<16>', 'wide<4>', 'wide<8>')
RAGGED_WIDE_ONLY = ('full<8,windowed>', 'wide<4>', 'wide<8>')


def ragged_plan(B, Np, Mp, topk=0, tap=False, wide=False):
    """(form, split, tiles) launch_attention chooses for a ragged batch in slots of Np x Mp (mdgat_attention_ragged_plan): the index is the
    uniform sibling's, the kernel its RAGGED instantiation."""
    split, tiles = C.c_int(-7), C.c_int(-7)
    form = _lib().mdgat_attention_ragged_plan(B, Np, Mp, topk, int(tap), int(wide), C.byref(split), C.byref(tiles))
    return form, split.value, tiles.value


def name(i):
    return 'none' if i < 0 else NAMES[i]


def counts():
    buf = (C.c_uint64 * len(NAMES))()
    _lib().mdgat_attention_launches(buf)
    return np.array(list(buf), dtype=np.int64)


class watch:
    """``with watch() as w: ...`` - afterwards w.delta[i] = launches of instantiation i in between (as numpy int64 [23])."""

    def __enter__(self):
        self.before = counts()
        self.delta = None
        return self

    def __exit__(self, *exc):
        self.delta = counts() - self.before

    def launched(self):
        return {NAMES[i]: int(n) for i, n in enumerate(self.delta) if n}


def assert_launched(w, want, what, times=1):
    """The watched region launched instantiation ``want`` (an index or a name) exactly ``times`` times, and no other."""
    want = NAMES[want] if isinstance(want, (int, np.integer)) else want
    assert w.launched() == {want: times}, f'{what}: wanted {times} x {want}, launched {w.launched()}'
