"""Yardstick, input builders and dispatch mirrors for the match extraction (models/mdgat.py:441-483) - every kernel that decides an
arg-max: extract_kernel, the epilogue of sinkhorn_scaling_kernel, the slab merges, the two fp64 Sinkhorn forms.  CPU, torch float64.

The reference is ``oracle.extract_matches`` applied in fp64.  Its dustbin-mutual branch (mdgat.py:469-478) works for any batch size:
it gathers per pair, where the reference indexes with ``[0]`` and so is right for B = 1 only.  The batch-wide all-dustbin rule
(465-467: no frame-0 keypoint of the WHOLE batch matched -> all scores zero) is the reference's and is kept.

Every rule under test is about equal values or a boundary - first maximal index, the dustbin (last index) loses a tie, a strict
threshold, "nothing matched anywhere" - so the builders here PLANT exact ties and boundary values; tests/test_extract_ref.py checks on
the oracle alone that they are there, tests/test_gpu_extract.py runs the kernels on them."""
import math

import numpy as np
import torch

import sinkhorn_f64_forms
from oracle import mdgat_oracle as O

MODES = {0: ('triplet_loss', False), 1: ('triplet_loss', True), 2: ('superglue', False), 3: ('superglue', True)}    # mdgat_extract_mode
SCORE_TOL = 1e-6          # the device's expf against fp64 exp of the same number, values <= 1 (test_extract_golden's bound)
GAP_MIN = 1e-9            # fp64 kernels against the oracle's Z: a decision between candidates further apart than this is the oracle's
                          # (the oracle-to-kernel bound on Z is 1e-12: tests/test_gpu_f64.py::_sinkhorn_f64_case)
THR_MARGIN = 1e-4         # relative distance kept between a threshold and every exp(max) it judges (far above expf's 1e-6)


def f32(x) -> float:
    """The float the C ABI's ``float match_threshold`` receives."""
    return float(np.float32(x))


def oracle_extract(Z, mode: int, thr: float):
    lm, mc = MODES[mode]
    return O.extract_matches(Z.detach().cpu().double(), lm, mc, thr)


def check_extraction(Z, m0, m1, s0, s1, mode: int, thr: float) -> float:
    """The matches a kernel returned against ``extract_matches`` in fp64 on the Z (any float dtype, any device) they were decided on:
    every index equal - no row or column is left out - and the scores within SCORE_TOL.  Returns the largest score error."""
    r0, r1, rs0, rs1 = oracle_extract(Z, mode, thr)
    m0, m1 = m0.cpu(), m1.cpu()
    bad0, bad1 = (m0 != r0).nonzero(), (m1 != r1).nonzero()
    assert m0.dtype == torch.int64 and m1.dtype == torch.int64
    assert bad0.numel() == 0, f'mode {mode}: matches0 differs at {bad0[:4].tolist()}: got {m0[tuple(bad0[0])].item()}, want {r0[tuple(bad0[0])].item()}'
    assert bad1.numel() == 0, f'mode {mode}: matches1 differs at {bad1[:4].tolist()}: got {m1[tuple(bad1[0])].item()}, want {r1[tuple(bad1[0])].item()}'
    e0 = (s0.cpu().double() - rs0).abs().max().item()
    e1 = (s1.cpu().double() - rs1).abs().max().item()
    assert e0 <= SCORE_TOL and e1 <= SCORE_TOL, f'mode {mode}: scores off by {e0:.3e} / {e1:.3e}'
    return max(e0, e1)


def naive_extract(Z, mode: int, thr: float):
    """mdgat.py:441-483 as plain loops (first maximal index by a strict compare in ascending order), the yardstick's yardstick."""
    Z = Z.double()
    B, n, m = Z.shape[0], Z.shape[1] - 1, Z.shape[2] - 1
    inner = mode >= 2
    ncol, nrow = (m, n) if inner else (m + 1, n + 1)
    i0 = [[0] * n for _ in range(B)]
    i1 = [[0] * m for _ in range(B)]
    for b in range(B):
        for i in range(n):
            best = 0
            for j in range(1, ncol):
                if Z[b, i, j] > Z[b, i, best]:
                    best = j
            i0[b][i] = best
        for j in range(m):
            best = 0
            for i in range(1, nrow):
                if Z[b, i, j] > Z[b, best, j]:
                    best = i
            i1[b][j] = best
    m0 = torch.full((B, n), -1, dtype=torch.int64)
    m1 = torch.full((B, m), -1, dtype=torch.int64)
    s0 = torch.zeros(B, n, dtype=torch.float64)
    s1 = torch.zeros(B, m, dtype=torch.float64)
    any_valid0 = any(i0[b][i] < m for b in range(B) for i in range(n))
    for b in range(B):
        e0 = [math.exp(Z[b, i, i0[b][i]]) for i in range(n)]
        e1 = [math.exp(Z[b, i1[b][j], j]) for j in range(m)]
        for i in range(n):
            j = i0[b][i]
            if mode < 2:
                if j < m:
                    m0[b, i] = j
                    if any_valid0 and (mode == 0 or i1[b][j] == i):
                        s0[b, i] = e0[i]
            elif mode == 2:
                if e0[i] > thr:
                    m0[b, i], s0[b, i] = j, e0[i]
            else:
                if i1[b][j] == i:
                    s0[b, i] = e0[i]
                    if e0[i] > thr:
                        m0[b, i] = j
        for j in range(m):
            i = i1[b][j]
            if mode < 2:
                if i < n:
                    m1[b, j] = i
                    if any_valid0 and (mode == 0 or i0[b][i] == j):
                        s1[b, j] = e1[j]
            elif mode == 2:
                if e1[j] > thr:
                    m1[b, j], s1[b, j] = i, e1[j]
            else:
                if i0[b][i] == j:
                    s1[b, j] = float(s0[b, i])
                    if int(m0[b, i]) >= 0:
                        m1[b, j] = i
    return m0, m1, s0, s1


def pick_threshold(Z, margin: float = THR_MARGIN) -> float:
    """A match threshold for the superglue branches taken from the Z under test: the midpoint of the two neighbours, in the sorted
    exp(row max) and exp(column max) of the inner block, that lie nearest the median and are at least ``margin`` relative apart.  Both
    sides are populated and no value is within margin / 2 of the threshold.  All values equal: half of that value."""
    Zi = Z.detach().cpu().double()[:, :-1, :-1]
    e = torch.cat([Zi.max(2).values.flatten(), Zi.max(1).values.flatten()]).exp().sort().values
    k = e.numel() // 2
    for d in range(e.numel()):
        for i in (k - 1 - d, k + d):
            if 0 <= i < e.numel() - 1 and float(e[i + 1] - e[i]) >= margin * float(e[i + 1]):
                return f32(0.5 * float(e[i] + e[i + 1]))
    return f32(0.5 * float(e[0]))


def ambiguous(Zr, mode: int, gap: float = GAP_MIN) -> int:
    """Rows and columns of the oracle's fp64 Z whose two best candidates are neither exactly equal (a planted tie: first index) nor
    more than ``gap`` apart - the ones a kernel with its own fp64 rounding (1e-12 on Z) may decide differently."""
    n, m = Zr.shape[1] - 1, Zr.shape[2] - 1
    rows = Zr[:, :n, :m] if mode >= 2 else Zr[:, :n, :]
    cols = Zr[:, :n, :m] if mode >= 2 else Zr[:, :, :m]
    cnt = 0
    for t, dim in ((rows, 2), (cols, 1)):
        if t.shape[dim] < 2:
            continue
        top = t.topk(2, dim=dim).values
        d = top.select(dim, 0) - top.select(dim, 1)
        cnt += int(((d > 0) & (d <= gap)).sum())
    return cnt


# ---------------------------------------------------------------------------------------------------------------- dispatch mirrors
def sk_tiling(N, M):
    """csrc/sinkhorn.hip sk_tiling: row slabs of 128 rows (8 waves x 16 rows), column slabs of 512 columns (64 lanes x 8 columns)."""
    return (N + 127) // 128, (M + 511) // 512


def scaling_kernel(N, M):
    """launch_scaling's choice of sinkhorn_scaling_kernel<TWO_D, GMAX>."""
    GR, GC = sk_tiling(N, M)
    if N > 2048 or M > 2048:
        return None
    return ('true', 16) if GC > 1 else ('false', 16) if GR > 4 else ('false', 4)


def streaming_kernel(N, M):
    """launch_streaming's choice of sinkhorn_kernel<NC, NW>."""
    for lim, nc, nw in ((64, 1, 16), (128, 2, 16), (256, 4, 16), (512, 8, 16)):
        if M <= lim:
            return nc, nw
    if M <= 1024 and N <= 4096:
        return 16, 8
    if M <= 2048 and N <= 4096:
        return 32, 8
    return None


def f64_kernel(N, M, form: int = -1):
    """csrc/sinkhorn_f64.hip sinkhorn_f64_form (a uniform call) and the streaming form's NC2: ('resident', row slabs of 32) or ('streaming', NC2, slabs)."""
    index, slabs, _ = sinkhorn_f64_forms.decide(N, M, form=form)      # (the one restatement of the decision, counts and history included)
    if index < 0:
        return None
    return ('resident', slabs) if index == sinkhorn_f64_forms.RESIDENT else ('streaming', sinkhorn_f64_forms.NC2[index], slabs)


def sk_wave(i):
    """(row slab, wave) that owns row i in the cluster kernel."""
    return i // 128, (i % 128) // 16


def sk_lane(j):
    """(column slab, lane) that owns column j in the cluster kernel."""
    return j // 512, (j % 512) // 8


def f64_streaming_wave(i):
    """(row slab, wave) of row i in the streaming fp64 form: the rows of a 32-row slab interleave over its eight waves."""
    return i // 32, (i % 32) % 8


# ------------------------------------------------------------------------------------------------------------------- planted Z
# base values lie in [-12, -1); every plant lies in (-1, 0), on rows and columns no other plant uses: a planted value is the maximum
# of its row and of its column.  THR is the threshold the superglue branches run with: the plants pass, the base does not.
THR = 0.5
EXTRACT_SHAPES = [(1, 1, 1), (3, 9, 7), (2, 64, 64), (2, 130, 2048), (2, 2048, 130), (1, 2048, 2048), (5, 600, 700), (2, 1, 300), (2, 300, 1),
                  (1, 2048, 1), (1, 17, 2048), (2, 2048, 64)]


def planted_Z(B, N, M, seed, zero_maxima=False):
    """Random fp32 Z [B, N+1, M+1] with ties and boundary values planted, and the list of what was planted:
    ('row_tie', r, c1, c2) equal row maxima, c1 < c2 (in different 64-column strides and lanes of extract_kernel's row scan if M allows);
    ('col_tie', c, r1, r2) equal column maxima at rows that different waves own;
    ('row_bin_tie', r, c) / ('col_bin_tie', c, r): an inner entry equal to the dustbin entry - the inner one must win;
    ('row_bin', r) / ('col_bin', c): the dustbin strictly larger;
    ('thr_above', r, c) / ('thr_below', r, c): exp(max) THR_MARGIN relative either side of THR;
    ('stolen', a, b, c): rows a and b both point at column c, which points at b; ('mutual', r, c): a pair that point at each other;
    ('zero', r, c) with ``zero_maxima``: Z = 0 as the maximum (exp = 1 exactly: not above a threshold of 1.0), ('above1', r, c): 1e-3.
    Plants that do not fit a small shape are left out."""
    g = torch.Generator().manual_seed(seed)
    Z = -1.0 - 11.0 * torch.rand(B, N + 1, M + 1, generator=g)
    rows = torch.randperm(N, generator=g).tolist()
    cols = torch.randperm(M, generator=g).tolist()
    plants = []

    def take(lst, k=1):
        if len(lst) < k:
            return None
        out = [lst.pop() for _ in range(k)]
        return out if k > 1 else out[0]

    def take_where(lst, ok):
        for x in lst:
            if ok(x):
                lst.remove(x)
                return x
        return None

    # equal row maxima: once in different lanes and strides, once in one lane (strides apart)
    for same_lane in (False, True):
        c1 = take(cols)
        if c1 is None:
            break
        c2 = take_where(cols, lambda c: c // 64 != c1 // 64 and (c % 64 == c1 % 64) == same_lane) if M > 64 else take(cols)
        r = take(rows)
        if c2 is None or r is None:
            break
        c1, c2 = min(c1, c2), max(c1, c2)
        Z[:, r, c1] = Z[:, r, c2] = -0.5
        plants.append(('row_tie', r, c1, c2))
    # equal column maxima at rows of different waves (rows i and i + 16 k + r)
    r1 = take(rows)
    if r1 is not None:
        r2 = take_where(rows, lambda r: r % 16 != r1 % 16) if N > 16 else take(rows)
        c = take(cols)
        if r2 is not None and c is not None:
            r1, r2 = min(r1, r2), max(r1, r2)
            Z[:, r1, c] = Z[:, r2, c] = -0.45
            plants.append(('col_tie', c, r1, r2))
    for kind, val in (('row_bin_tie', -0.25), ('col_bin_tie', -0.3), ('thr_above', math.log(THR * (1 + THR_MARGIN))),
                      ('thr_below', math.log(THR * (1 - THR_MARGIN))), ('mutual', -0.05)) + ((('zero', 0.0), ('above1', 1e-3)) if zero_maxima else ()):
        r, c = take(rows), take(cols)
        if r is None or c is None:
            continue
        Z[:, r, c] = val
        if kind == 'row_bin_tie':
            Z[:, r, M] = val
            plants.append((kind, r, c))
        elif kind == 'col_bin_tie':
            Z[:, N, c] = val
            plants.append((kind, c, r))
        else:
            plants.append((kind, r, c))
    r = take(rows)
    if r is not None:
        Z[:, r, M] = -0.1
        plants.append(('row_bin', r))
    c = take(cols)
    if c is not None:
        Z[:, N, c] = -0.1
        plants.append(('col_bin', c))
    ab, c = take(rows, 2), take(cols)
    if ab is not None and c is not None:
        Z[:, ab[0], c], Z[:, ab[1], c] = -0.3, -0.2
        plants.append(('stolen', ab[0], ab[1], c))
    return Z, plants


# ------------------------------------------------------------------------------------------------------------- planted scores
# (B, N, M) of the fp32 Sinkhorn + extraction cases; tests/test_extract_ref.py holds what they must cover
SK_SHAPES = [(3, 100, 300), (1, 128, 512), (3, 512, 512), (70, 400, 257), (2, 70, 60), (2, 300, 100),        # <false, 4>
             (1, 513, 200), (3, 900, 512), (1, 2048, 130),                                                   # <false, 16>
             (1, 300, 513), (3, 200, 700), (1, 130, 2048), (2, 700, 1100), (1, 2048, 2048)]                  # <true, 16>
SK_ITERS = 20
# (B, N, M, iters, form) of the fp64 cases: form 1 = mdgat_set_f64_sinkhorn_form(1), the streaming form on frames the resident one holds
F64_CASES = [(2, 96, 96, 50, -1), (2, 96, 96, 50, 1), (1, 575, 575, 20, -1), (2, 200, 130, 30, -1), (2, 200, 130, 30, 1),
             (1, 576, 300, 20, -1), (1, 300, 576, 20, -1), (2, 575, 575, 20, 1), (1, 1100, 900, 20, -1),
             (1, 2175, 130, 20, -1), (1, 130, 2175, 20, -1)]
# the rows / columns that builder A makes equal: 'waves' - other wave, other lane, one slab; 'slabs' - first and last slab;
# 'interleave' - ra < rb with ra in a HIGHER wave of the streaming fp64 form (rows 7 and 8 of a slab), columns 64 apart
TIE_VARIANTS = ('waves', 'slabs', 'interleave')


def tie_positions(N, M, variant):
    """(ra, rb, ca, cb), ra < rb and ca < cb."""
    if variant == 'waves':
        ra, rb, ca, cb = 5, min(55, N - 1), 3, min(60, M - 1)
    elif variant == 'slabs':
        ra, rb, ca, cb = 5, N - 2, 3, M - 1
    else:
        ra, rb, ca, cb = 7, 8, 3, min(67, M - 1)
    assert 0 <= ra < rb < N and 0 <= ca < cb < M, (N, M, variant)
    return ra, rb, ca, cb


def _randn(B, N, M, seed, dtype):
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.standard_normal((B, N, M))).to(dtype)


def scores_A(B, N, M, variant, seed=0, dtype=torch.float32):
    """Normal scores x 3 with row rb a copy of row ra and column cb a copy of column ca, the four crossing entries raised to 20: rows ra
    and rb get the same potential and so do the two columns, and the four equal entries of Z are the maxima of their rows and columns.
    Row ra must pick column ca, column ca row ra - and so must row rb and column cb."""
    ra, rb, ca, cb = tie_positions(N, M, variant)
    s = _randn(B, N, M, seed + 7 * N + M, dtype) * 3
    s[:, rb, :] = s[:, ra, :]
    s[:, :, cb] = s[:, :, ca]
    for r in (ra, rb):
        for c in (ca, cb):
            s[:, r, c] = 20.0
    return s, (ra, rb, ca, cb)


# builder B: constant scores - every inner entry of Z ties.  'inner' (bin = c - 12): the inner entries are the maxima of every row
# (N <= M) and of every column (M <= N) - column 0 / row 0 must win across all lanes, waves and slabs - while the longer frame's surplus
# mass goes to the dustbin; 'dustbin' (bin = c + 2) sends everything to the dustbin; the superglue branches pick index 0 on both sides
# either way.  'border' runs NO iteration with bin = c = -10: Z is the coupling matrix itself, every row and column ties its inner entries
# WITH its dustbin entry.
CONST_SCORE = 0.5
BORDER_SCORE = -10.0      # ('border': Z = score + log(N + M) stays below 0, so that its exp is within the score bound's range)
CONST_KINDS = {'inner': (CONST_SCORE, CONST_SCORE - 12.0, None), 'dustbin': (CONST_SCORE, CONST_SCORE + 2.0, None),
               'border': (BORDER_SCORE, BORDER_SCORE, 0)}                                                   # score, bin_score, iterations


def scores_B(B, N, M, dtype=torch.float32, value=CONST_SCORE):
    return torch.full((B, N, M), value, dtype=dtype)


def bin_score_C(N, M):
    """Builder C's bin score: with normal scores x 3, between 10 % and 90 % of the keypoints of the SHORTER frame prefer the dustbin
    (of the longer frame at most min(N, M) keypoints can carry inner mass at all, so no bin score brings its share below
    1 - min / max).  Fitted to the bin score at which half of them do, for frames from 60 to 2175 keypoints."""
    return 1.0 + 2.4 * math.sqrt(math.log(max(N, M) / min(N, M)))


def dustbin_share_C(Z):
    """Share of the shorter frame's keypoints (rows if N <= M) whose arg-max is the dustbin."""
    n, m = Z.shape[1] - 1, Z.shape[2] - 1
    if n <= m:
        return (Z[:, :n, :].argmax(2) == m).double().mean().item()
    return (Z[:, :, :m].argmax(1) == n).double().mean().item()


def scores_C(B, N, M, seed=0, dtype=torch.float32):
    return _randn(B, N, M, seed + 3 * N + 5 * M + 1, dtype) * 3


def wide_range_scores(B, N, M, wide, seed=0):
    """The builder of test_sinkhorn_range_fallback_is_per_pair: pairs ``wide`` spread over ~250 units, beyond the scaling form's range."""
    s = _randn(B, N, M, seed + B + N + M, torch.float32) * 3
    for w in wide:
        s[w] = s[w] * 14 + 50.0
    return s


# ------------------------------------------------------------------------------------------------------------- all-dustbin rule
ALLDUST_SHAPE = (96, 24)      # N = 4 M: with a bin score between the two fixed-point ratios rows prefer the dustbin, columns do not
ALLDUST_BIN = 0.0 - 0.5 * (math.log(96) + math.log(24))


def alldust_scores(B, kind, which=0, seed=0):
    """[B, 96, 24] scores and the bin score for the batch-wide rule: 'none' - no row of any pair prefers an inner column while every
    column prefers an inner row (so matching_scores1 is NOT zero before the rule is applied); 'one' - the same, but row 11 of pair
    ``which`` is raised above its dustbin; 'all' - every pair matches plenty."""
    N, M = ALLDUST_SHAPE
    s = _randn(B, N, M, seed + 11 * B, torch.float32) * 0.05
    if kind == 'all':
        return s * 60, ALLDUST_BIN
    if kind == 'one':
        s[which, 11, 5] += 6.0
    return s, ALLDUST_BIN


def alldust_Z(B, kind, which=0, seed=0, N=40, M=50):
    """The same three kinds as a planted Z for ops.extract: dustbin column -0.1 (every row's maximum), dustbin row -20."""
    g = torch.Generator().manual_seed(seed + B)
    Z = -1.0 - 11.0 * torch.rand(B, N + 1, M + 1, generator=g)
    if kind != 'all':
        Z[:, :N, M] = -0.1
        Z[:, N, :] = -20.0
    if kind == 'one':
        Z[which, 11, 5] = -0.05
    return Z
