"""The 13 instantiations the fp32 Sinkhorn launcher (csrc/sinkhorn.hip: launch_sinkhorn, with or without per-pair counts) can reach, as the tests
name them, and the two symbols that make their choices observable: mdgat_sinkhorn_plan (the path, the instantiations and the launch
parameters as a pure function; no device) and mdgat_sinkhorn_launches (launches so far by index).  The table of indices: include/mdgat_hip.h.

0-2 the scaling (cluster) kernel, 3-8 the streaming kernel launched on its own, 9-12 its RAGGED twins; two more counters keep
``assert_launched`` exact: 13 a streaming kernel gated behind a cluster launch (which one: the plan's streaming index), 14 extract_kernel."""
import ctypes as C
from collections import namedtuple

import numpy as np

SCALING = ('scaling<false,4>', 'scaling<false,16>', 'scaling<true,16>')
STREAM = ('stream<1,16>', 'stream<2,16>', 'stream<4,16>', 'stream<8,16>', 'stream<16,8>', 'stream<32,8>')
RAGGED = tuple(n + ',RAGGED' for n in STREAM[:4])
NAMES = SCALING + STREAM + RAGGED + ('gated', 'extract')
INSTANTIATIONS = NAMES[:13]
GATED, EXTRACT = 'gated', 'extract'
CLUSTER, STREAMING, NONE = 0, 1, -1          # the plan's path
CUS = 256                                    # compute units of the part the kernels are written for (the plan's default here)

# The smallest shapes that reach each form (tests/test_gpu_sinkhorn_forms.py runs them, tests/test_sinkhorn_plan.py pins their plans)
# cluster: (N, M) -> (name, GR, GC)
CLUSTER_CASES = {
    (64, 64): ('scaling<false,4>', 1, 1),         # one workgroup: no exchange
    (130, 65): ('scaling<false,4>', 2, 1),        # two row slabs, a ragged column lane
    (390, 24): ('scaling<false,4>', 4, 1),
    (513, 40): ('scaling<false,16>', 5, 1),
    (2048, 8): ('scaling<false,16>', 16, 1),
    (40, 513): ('scaling<true,16>', 1, 2),
    (130, 1030): ('scaling<true,16>', 2, 3),
    (20, 1540): ('scaling<true,16>', 1, 4),
}
# streaming (no workspace): (N, M) -> name; each M also with N = 1 and N = 17
_STREAM_M = {64: 'stream<1,16>', 65: 'stream<2,16>', 129: 'stream<4,16>', 257: 'stream<8,16>', 513: 'stream<16,8>', 1025: 'stream<32,8>',
             2048: 'stream<32,8>'}
STREAM_CASES = {(n, m): nm for m, nm in _STREAM_M.items() for n in ((5 if m == 2048 else 3), 1, 17)}
FORMS_BATCH = 3                              # pairs per call in the tests of the forms

Plan = namedtuple('Plan', 'path scaling stream GR GC ngroups xcd_map grid cooperative')


def _lib():
    from mdgat_matcher_amd import _lib
    return _lib.load()


def name(i):
    return 'none' if i < 0 else NAMES[i]


def workspace_bytes(B, N, M):
    return int(_lib().mdgat_sinkhorn_workspace_bytes(B, N, M))


def plan(B, N, M, cus=CUS, workspace=True, fallback=True, ragged=False, ws_addr=None, ws_bytes=None):
    """What the launchers choose for B pairs of N x M, with the instantiations by name.  workspace: one of the size the library asks for
    at a 256-byte aligned address is passed (ws_addr / ws_bytes: another address or size; the address is never dereferenced)."""
    out = (C.c_int32 * 8)(*([-7] * 8))
    if ws_addr is None:
        ws_addr = 4096 if workspace else None
    if ws_bytes is None:
        ws_bytes = workspace_bytes(B, N, M) if workspace else 0
    path = _lib().mdgat_sinkhorn_plan(B, N, M, cus, ws_addr, ws_bytes, int(fallback), int(ragged), out)
    w = list(out)
    return Plan(path, name(w[0]), name(w[1]), w[2], w[3], w[4], bool(w[5]), w[6], bool(w[7]))


def counts():
    buf = (C.c_uint64 * len(NAMES))()
    _lib().mdgat_sinkhorn_launches(buf)
    return np.array(list(buf), dtype=np.int64)


class watch:
    """``with watch() as w: ...`` - afterwards w.delta[i] = launches of index i in between (as numpy int64 [15])."""

    def __enter__(self):
        self.before = counts()
        self.delta = None
        return self

    def __exit__(self, *exc):
        self.delta = counts() - self.before

    def launched(self):
        return {NAMES[i]: int(n) for i, n in enumerate(self.delta) if n}


def expected(p, times=1, extract=False):
    """What one call with plan ``p`` launches, ``times`` times: the cluster form and the gated kernel behind it, or the streaming form."""
    want = {}
    if p.path == CLUSTER:
        want[p.scaling] = times
        if p.stream != 'none':
            want[GATED] = times
    elif p.path == STREAMING:
        want[p.stream] = times
    if extract:
        want[EXTRACT] = times
    return want


def assert_launched(w, want, what, times=1, extract=False):
    """The watched region launched exactly ``want`` and nothing else.  want: a Plan (what ``expected`` derives from it), a name (that
    index ``times`` times) or a dict {name: launches}."""
    if isinstance(want, Plan):
        want = expected(want, times, extract)
    elif isinstance(want, str):
        want = {want: times}
    assert w.launched() == want, f'{what}: wanted {want}, launched {w.launched()}'
