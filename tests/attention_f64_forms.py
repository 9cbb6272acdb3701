"""The seven instantiations of attention_f64_kernel (csrc/f64.hip) as the tests name them, and the three symbols that make the launcher's
plan (attention_f64_plan) observable: mdgat_attention_f64_plan (the choice as a pure function; no device), mdgat_attention_f64_geometry
(the same with the launch it stands for: queries per workgroup, tiles, grid, LDS bytes) and mdgat_attention_f64_launches (launches so
far by index)."""
import ctypes as C

import numpy as np

NAMES = ('full16', 'full32', 'keep+tap', 'keep', 'recompute+tap', 'recompute', 'solo')
FULL16, FULL32, KEEP_TAP, KEEP, RECOMPUTE_TAP, RECOMPUTE, SOLO = range(7)


def _lib():
    from mdgat_matcher_amd import _lib
    return _lib.load()


def plan(B, N, M, topk=0, tap=False, ragged=False, cnt_min=0, form=-1, cus=256):
    """The index launch_attention_f64 chooses (negative: no launch)"""
    return _lib().mdgat_attention_f64_plan(B, N, M, topk, int(tap), int(ragged), cnt_min, form, cus)


def geometry(B, N, M, topk=0, tap=False, ragged=False, cnt_min=0, form=-1, cus=256):
    """(index, queries per workgroup, query tiles per unit, workgroups, LDS bytes) of that launch; the four are 0 where there is none"""
    q, t, w, lds = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_size_t(1)
    idx = _lib().mdgat_attention_f64_geometry(B, N, M, topk, int(tap), int(ragged), cnt_min, form, cus, C.byref(q), C.byref(t), C.byref(w), C.byref(lds))
    return idx, q.value, t.value, w.value, lds.value


def counts():
    buf = (C.c_uint64 * len(NAMES))()      # MDGAT_ATTENTION_F64_FORMS
    _lib().mdgat_attention_f64_launches(buf)
    return np.array(list(buf), dtype=np.int64)


class watch:
    """``with watch() as w: ...`` - afterwards w.delta[i] = launches of instantiation i in between (numpy int64 [7])"""

    def __enter__(self):
        self.before = counts()
        self.delta = None
        return self

    def __exit__(self, *exc):
        self.delta = counts() - self.before

    def launched(self):
        return {NAMES[i]: int(n) for i, n in enumerate(self.delta) if n}


def cu_count(device=0):
    import torch
    return torch.cuda.get_device_properties(device).multi_processor_count


def full_attention_batches(N, M, cus):
    """Batch sizes that the automatic form sends to full16, full32 and solo on a device of `cus` compute units: 4 pairs (or fewer, on a
    small partition) and the smallest batches that reach the other two (None: none below 4096 pairs).  256 CUs, 40 x 40: 4, 32, 128."""
    first = {}
    for B in range(1, 4097):
        first.setdefault(plan(B, N, M, cus=cus), B)
    small = next((B for B in (4, 2, 1) if plan(B, N, M, cus=cus) == FULL16), None)
    return small, first.get(FULL32), first.get(SOLO)
