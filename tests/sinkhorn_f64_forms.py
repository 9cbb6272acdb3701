"""The eleven forms a call of the fp64 Sinkhorn runs (csrc/sinkhorn_f64.hip; the table of indices: include/mdgat_hip.h), as the tests name
them; the launcher's decision restated in Python (``decide``: the one restatement - extract_ref.f64_kernel calls it); the two symbols that
make the decision observable - mdgat_sinkhorn_f64_plan (a pure function; no device) and mdgat_sinkhorn_f64_launches (calls so far by form);
and the case tables of tests/test_gpu_sinkhorn_f64_forms.py, every case with the index it claims.  tests/test_sinkhorn_f64_plan.py (CPU)
holds the plan to the restatement and the tables to the plan, so neither can rot."""
import collections
import ctypes as C

import numpy as np
import torch

NAMES = ('resident', 'resident-ragged', 'stream<5>', 'stream<9>', 'stream<17>', 'stream-ragged<5>', 'stream-ragged<9>', 'stream-ragged<17>',
         'history<5>', 'history<9>', 'history<17>')
RESIDENT, RESIDENT_RAGGED, STREAM_5, STREAM_9, STREAM_17, RAGGED_5, RAGGED_9, RAGGED_17, HISTORY_5, HISTORY_9, HISTORY_17 = range(11)
NC2 = {STREAM_5: 5, STREAM_9: 9, STREAM_17: 17, RAGGED_5: 5, RAGGED_9: 9, RAGGED_17: 17, HISTORY_5: 5, HISTORY_9: 9, HISTORY_17: 17}
BUCKETS = ((1, 5), (6, 9), (10, 17))    # the chunk counts (128 columns each, the dustbin column included) an instantiation <5 | 9 | 17> holds
RESIDENT_ROWS, RESIDENT_COLUMNS = 576, 575      # the register-resident kernel: 18 slabs of 32 rows, nine columns per lane less the dustbin
RAGGED_LIMIT = 575                      # MDGAT_RAGGED_MAX_KEYPOINTS: with counts, the resident form takes one limit for both frames
STREAM_LIMIT = 2175                     # 17 chunks of 128 columns less the dustbin; the rows' dustbin is a column of the backward's operand

MARGIN_MIN = 1e-9                       # extract_ref.GAP_MIN: a decision between candidates further apart than this is the oracle's
THR = 0.01                              # the match threshold of tests/test_gpu_f64.py::_sinkhorn_f64_case and of the ragged streaming tests
SCALE = 3.0                             # scores are standard normal times this


def decide(N, M, ragged=False, ragged_mode=0, form=-1, history=False):
    """(index, row slabs, column chunks) of a call in slots of N x M keypoints; ``ragged``: with counts, under ``ragged_mode`` as
    mdgat_set_ragged_sinkhorn takes it (0: the resident form or none, 2: the streaming form, 1: the resident form where mode 0 has it and
    the streaming one elsewhere); ``form``: -1 or 1 as mdgat_set_f64_sinkhorn_form takes them; ``history``: the backward's history run.
    (-1, 0, 0): no form holds the call, or history with counts."""
    resident_ok = N >= 1 and 1 <= M <= RESIDENT_COLUMNS and N <= RESIDENT_ROWS
    stream_ok = 1 <= N <= STREAM_LIMIT and 1 <= M <= STREAM_LIMIT
    if history and ragged:
        return -1, 0, 0
    resident = resident_ok and (not ragged or N <= RAGGED_LIMIT) and form != 1
    if resident and not (ragged and ragged_mode == 2):
        streaming = False
    elif stream_ok and not (ragged and ragged_mode == 0):
        streaming = True
    else:
        return -1, 0, 0
    slabs = -(-N // 32)
    if not streaming and not history:       # (the history run streams at every size)
        return (RESIDENT_RAGGED if ragged else RESIDENT), slabs, 0
    chunks = -(-(M + 1) // 128)
    bucket = next(i for i, (_, hi) in enumerate(BUCKETS) if chunks <= hi)
    return (HISTORY_5 if history else RAGGED_5 if ragged else STREAM_5) + bucket, slabs, chunks


# ------------------------------------------------------------------------------------------------------------------ the case tables
# Uniform calls (B, N, M, iterations, form, index): form 1 = under mdgat_set_f64_sinkhorn_form(1).  Each is held to the checks of
# tests/test_gpu_f64.py::_sinkhorn_f64_case on that function's own seeded scores (``uniform_scores``), bin score 1.0.
Uniform = collections.namedtuple('Uniform', 'B N M iters form index')
UNIFORM_CASES = (
    # resident: 18 full slabs (the most rows, one beyond the ragged limit) against one column and against the most columns; one row;
    # one full slab and one row more
    Uniform(1, 576, 1, 5, -1, RESIDENT), Uniform(1, 576, 575, 4, -1, RESIDENT), Uniform(2, 1, 575, 5, -1, RESIDENT),
    Uniform(1, 32, 64, 10, -1, RESIDENT), Uniform(1, 33, 64, 10, -1, RESIDENT),
    # <5>: the dustbin the last column of chunk 1 | alone in chunk 2; one row, one column; five full chunks (639 | 640)
    Uniform(2, 33, 127, 6, 1, STREAM_5), Uniform(2, 33, 128, 6, 1, STREAM_5), Uniform(1, 1, 1, 5, 1, STREAM_5), Uniform(1, 40, 639, 4, 1, STREAM_5),
    # <9>: the dustbin alone in chunk 6; alone in chunk 9; the last column of chunk 9 (1151 | 1152); and no iteration
    Uniform(1, 40, 640, 4, 1, STREAM_9), Uniform(1, 40, 1024, 3, 1, STREAM_9), Uniform(1, 40, 1151, 5, 1, STREAM_9), Uniform(1, 33, 900, 0, 1, STREAM_9),
    # <17>: the dustbin alone in chunk 10; one row and 17 chunks
    Uniform(1, 40, 1152, 4, 1, STREAM_17), Uniform(1, 1, 2175, 3, -1, STREAM_17),
    # 68 slabs, the most, against ONE chunk - which is <5>: the instantiation follows the columns alone
    Uniform(1, 2175, 1, 3, -1, STREAM_5),
)
UNIFORM_ALPHA = 1.0

# Ragged batches on the streaming form (ops' form='streaming'): the slot picks the instantiation, the pairs alone under form 1 pick their own
Ragged = collections.namedtuple('Ragged', 'pairs iters alpha low index')      # low: the pair pushed 40 below the bin score (or None)
RAGGED_SETS = {
    # slots of 70 x 1151: nine chunks, the dustbin of the filling pair their last column; pairs of six, five, nine and one chunk beside it
    'V9': Ragged(((70, 1151), (33, 640), (40, 639), (64, 1024), (8, 8), (1, 1)), 5, 0.7, 4, RAGGED_9),
    # slots of 33 x 640: six chunks, the dustbin alone in the last
    'V6': Ragged(((33, 640), (32, 127), (1, 5)), 3, 0.7, None, RAGGED_9),
    # slots of 40 x 1152: ten chunks, <17> at its fewest
    'V10': Ragged(((40, 1152), (40, 1151), (8, 8)), 4, 1.0, None, RAGGED_17),
}
# ... and on the resident form, at its limit
RESIDENT_RAGGED_SET = Ragged(((575, 8), (8, 575), (33, 33)), 5, 1.0, None, RESIDENT_RAGGED)
# The forms whose cases live elsewhere, (slot, index): the sets of tests/test_gpu_ragged_sinkhorn_stream.py, which asserts these indices ...
STREAM_SETS_ELSEWHERE = {'S': ((130, 128), RAGGED_5), 'S0': ((130, 128), RAGGED_5), 'T': ((1100, 1200), RAGGED_17), 'U': ((2175, 2175), RAGGED_17)}


def history_cases():
    """... and the history runs of tests/test_gpu_sinkhorn_grad.py::test_fp64_reverse_variants: (N, M, index)"""
    from sinkhorn_grad_ref import VARIANT_CASES
    return [(N, M, decide(N, M, history=True)[0]) for _, N, M, _ in VARIANT_CASES]


def slot(pairs):
    return max(n for n, _ in pairs), max(m for _, m in pairs)


def uniform_scores(c):
    """the scores tests/test_gpu_f64.py::_sinkhorn_f64_case forms for the case"""
    rs = np.random.RandomState(c.N + 3 * c.M + c.iters)
    return torch.from_numpy(rs.standard_normal((c.B, c.N, c.M)) * SCALE)


def ragged_scores(r, fill=0.0, seed=5):
    """[B, Np, Mp] scores of a ragged set, ``fill`` beyond every pair's counts; pair ``low`` lies 40 below, so that it matches nothing
    beside pairs that do"""
    Np, Mp = slot(r.pairs)
    rs = np.random.RandomState(seed)
    s = np.full((len(r.pairs), Np, Mp), fill)
    for b, (n, m) in enumerate(r.pairs):
        s[b, :n, :m] = rs.standard_normal((n, m)) * SCALE - (40.0 if b == r.low else 0.0)
    return torch.from_numpy(s)


# ------------------------------------------------------------------------------------- what the extraction asserts rest on (CPU, oracle)
def margins(Zr):
    """Of the oracle's fp64 Z [B, n+1, m+1]: (the smallest margin between the two best candidates of any arg-max the four extraction modes
    take - rows over all columns and over the inner ones, columns over all rows and over the inner ones; the same of Z rounded to fp32,
    which the device's extract kernel decides on when it serves as the reference; the smallest relative distance of exp(an inner maximum)
    from THR, which the superglue branches compare with)."""
    n, m = Zr.shape[1] - 1, Zr.shape[2] - 1
    out = []
    for Z in (Zr, Zr.float().double()):
        worst = float('inf')
        for t, dim in ((Z[:, :n, :], 2), (Z[:, :n, :m], 2), (Z[:, :, :m], 1), (Z[:, :n, :m], 1)):
            if t.shape[dim] >= 2:
                top = t.topk(2, dim=dim).values
                worst = min(worst, float((top.select(dim, 0) - top.select(dim, 1)).min()))
        out.append(worst)
    inner = Zr[:, :n, :m]
    e = torch.cat([inner.max(2).values.flatten(), inner.max(1).values.flatten()]).exp()
    out.append(float(((e - THR).abs() / THR).min()))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------- the two symbols
def _lib():
    from mdgat_matcher_amd import _lib
    return _lib.load()


def plan(N, M, ragged=False, ragged_mode=0, form=-1, history=False):
    """mdgat_sinkhorn_f64_plan -> (index, slabs, chunks); form: -1, 1, or anything else for the current setting"""
    slabs, chunks = C.c_int(-7), C.c_int(-7)
    index = _lib().mdgat_sinkhorn_f64_plan(N, M, int(ragged), ragged_mode, form, int(history), C.byref(slabs), C.byref(chunks))
    return index, slabs.value, chunks.value


def counts():
    buf = (C.c_uint64 * len(NAMES))()
    _lib().mdgat_sinkhorn_f64_launches(buf)
    return np.array(list(buf), dtype=np.int64)


class watch:
    """``with watch() as w: ...`` - afterwards w.ran() = {form index: calls run in it in between}"""

    def __enter__(self):
        self.before = counts()
        self.delta = None
        return self

    def __exit__(self, *exc):
        self.delta = counts() - self.before

    def ran(self):
        return {i: int(n) for i, n in enumerate(self.delta) if n}


class forced:
    """``with forced(form):`` - mdgat_set_f64_sinkhorn_form(form) inside, the previous setting behind it"""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.prev = _lib().mdgat_set_f64_sinkhorn_form(self.form)
        return self

    def __exit__(self, *exc):
        _lib().mdgat_set_f64_sinkhorn_form(self.prev)
