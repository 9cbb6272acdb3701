"""The seven forms a layer tail or the encoder launch of the exact mode takes (csrc/layer_f64.hip, and the one-product-per-launch branches
of csrc/api.hip), as the tests name them, and the two symbols that make the launchers' choice observable: mdgat_layer_f64_plan (the choice
and its grid as a pure function; no device unless cus <= 0) and mdgat_layer_f64_launches (tails / encoders so far by form).  The table of
indices: include/mdgat_hip.h."""
import collections
import ctypes as C

import numpy as np

NAMES = ('tail-gemms', 'tail<1>', 'tail<2>', 'tail-cluster', 'encoder<1>', 'encoder<2>', 'encoder-gemms')
TAIL_GEMMS, TAIL16, TAIL32, CLUSTER, ENC16, ENC32, ENC_GEMMS = range(7)
MODES = (0, 1, 2, 16, 32)               # what mdgat_set_f64_layer_fusion distinguishes
CASE_CUS = 256                          # the device the shapes of CASES are written for
ORACLE_MAX_ROWS = 1100                  # cases up to this many rows are also held to the CPU oracle

# The cases of tests/test_gpu_layer_f64_forms.py: the smallest launches that reach every form and every edge of it on a device of CASE_CUS
# compute units.  One case = one tapped forward (unsliced: every launch has R = B (n + m) rows) of an exact-mode network of L layers with
# the top-k schedule k under mdgat_set_f64_layer_fusion(mode).  tail 'auto': the fp64 tail - all 2 L layers in fp64, so the encoder launch
# and 2 L layer tails, the last of them without a next q | k | v (w3f == nullptr) and writing the fp32 x.  tail 'fp32'
# (sinkhorn_arithmetic): the fp32-class kernels take over behind the last layer with a k (csrc/api.hip: f64_layer_count) and READ that
# fp32 x, so a wrong hand-over shows in every later stage.  `tail_form` / `encoder_form`: what the case is there for, at CASE_CUS;
# tests/test_layer_f64_plan.py holds every row to the plan, so the table cannot rot.  alone: the case also runs its pair 0 alone.
Case = collections.namedtuple('Case', 'id B n m mode L k tail tail_form encoder_form alone')
_K = [16, None, 8, None]
CASES = [
    # nblk = 64 = CUs / 4 blocks: the largest clustered launch, 8 whole groups of 8 clusters
    Case('cluster_full', 1, 512, 512, 1, 2, _K, 'auto', CLUSTER, ENC16, False),
    # one block more: one workgroup per block
    Case('cluster_over', 1, 512, 528, 1, 2, _K, 'auto', TAIL16, ENC16, False),
    # nblk = 34 (34 % 8 = 2: the grid holds 40 clusters, six return at once), R % 16 = 3 (clamped tile rows, guarded stores)
    Case('cluster_ragged', 3, 100, 77, 1, 2, _K, 'auto', CLUSTER, ENC16, True),
    # a single partial block
    Case('cluster_one', 1, 5, 3, 1, 2, [2, None, 1, None], 'auto', CLUSTER, ENC16, False),
    # ceil(R / 32) = 512 = 2 CUs: the first launch the default rule gives 32 rows per workgroup ...
    Case('tail32_auto', 64, 128, 128, 1, 2, _K, 'auto', TAIL32, ENC32, True),
    # ... and one block fewer
    Case('tail16_below', 64, 128, 127, 1, 2, _K, 'auto', TAIL16, ENC16, False),
    # R % 32 = 13: the last workgroup's second row block lies wholly beyond R
    Case('tail32_half', 5, 33, 40, 32, 2, _K, 'auto', TAIL32, ENC32, True),
    Case('tail16_forced', 5, 33, 40, 16, 2, _K, 'auto', TAIL16, ENC16, False),
    # mode 2 where mode 1 clusters
    Case('no_cluster', 1, 512, 512, 2, 2, _K, 'auto', TAIL16, ENC16, False),
    # the hand-over: layers 0 .. 2 in fp64 (k of layer 2 is the last), layer 2's tail with w3f == nullptr writes the x layer 3 reads
    Case('last_layer_cluster', 2, 70, 64, 1, 2, _K, 'fp32', CLUSTER, ENC16, False),
    Case('last_layer_16', 2, 70, 64, 2, 2, _K, 'fp32', TAIL16, ENC16, False),
    Case('last_layer_32', 2, 70, 64, 32, 2, _K, 'fp32', TAIL32, ENC32, False),
    # no layer with a k: the encoder launch itself hands over (no q | k | v, the fp32 x written); no tail form runs
    Case('encoders_only', 3, 70, 64, 1, 1, [], 'fp32', None, ENC16, False),
    Case('encoders_only_32', 3, 70, 64, 32, 1, [], 'fp32', None, ENC32, False),
]


def f64_layers(case):
    """How many leading layers a case runs in fp64 (csrc/api.hip: Path::first): all with the fp64 tail, else through the last one with a k."""
    if case.tail == 'auto':
        return 2 * case.L
    return max((i + 1 for i, k in enumerate(case.k) if k), default=0)


def _lib():
    from mdgat_matcher_amd import _lib
    return _lib.load()


def plan(R, encoder=False, has_hid=True, chained=True, mode=1, cus=CASE_CUS):
    """(form, workgroups, rows per workgroup) of a launch of R rows (form -1: none)"""
    wg, rows = C.c_int(-7), C.c_int(-7)
    form = _lib().mdgat_layer_f64_plan(R, int(encoder), int(has_hid), int(chained), mode, cus, C.byref(wg), C.byref(rows))
    return form, wg.value, rows.value


def case_forms(case, cus=CASE_CUS, mode=None, chained=True):
    """{form index: times} the forward of a case runs under `mode` (default: its own) on a device of `cus` compute units."""
    R, mode = case.B * (case.n + case.m), case.mode if mode is None else mode
    want = {plan(R, True, mode=mode, cus=cus, chained=chained)[0]: 1}
    if f64_layers(case):
        want[plan(R, False, mode=mode, cus=cus, chained=chained)[0]] = f64_layers(case)
    return want


def counts():
    buf = (C.c_uint64 * len(NAMES))()
    _lib().mdgat_layer_f64_launches(buf)
    return np.array(list(buf), dtype=np.int64)


class watch:
    """``with watch() as w: ...`` - afterwards w.delta[i] = tails / encoders run in form i in between (numpy int64 [7])"""

    def __enter__(self):
        self.before = counts()
        self.delta = None
        return self

    def __exit__(self, *exc):
        self.delta = counts() - self.before

    def launched(self):
        return {i: int(n) for i, n in enumerate(self.delta) if n}


def named(forms):
    return {NAMES[i]: n for i, n in sorted(forms.items())}


class fusion:
    """``with fusion(mode):`` - mdgat_set_f64_layer_fusion(mode) inside, the default setting behind it"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        _lib().mdgat_set_f64_layer_fusion(self.mode)
        return self

    def __exit__(self, *exc):
        _lib().mdgat_set_f64_layer_fusion(-1)


def cu_count(device=0):
    import torch
    return torch.cuda.get_device_properties(device).multi_processor_count
