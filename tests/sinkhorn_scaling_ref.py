"""The arithmetic of sinkhorn_scaling_kernel (csrc/sinkhorn.hip) for ONE pair, restated in numpy float32 on the CPU, with a report of what
the kernel cannot be asked about without touching its iteration loop: whether the pair is handed to the streaming kernel (the range flag),
which of the four folds fired and when, and how far a scaling factor would have gone without them.

Written from the kernel and from the model's log_optimal_transport (mdgat.py:279-308).  The steps are the kernel's: scores in base-2 log
units, the row maximum (bin score included) absorbed, K = exp2(s + u0) kept for all iterations, the range test kmin < 2^-100, the
a / b iteration with the dustbin row and column in closed form, the four folds at the kernel's thresholds - the column fold decided per
512-column slab, the dustbin column bM, the dustbin row aN, single rows - and the epilogue: lg2(K) + dU + dV with the re-read of
entries below the smallest normal (the <false, 4> kernel, ``from_k=True``), or the scores read again (the other two).  What it does NOT
restate: the order of the sums (numpy's pairwise sums for the wave and slab reductions) and the last bit of v_rcp_f32 / v_exp_f32 /
v_log_f32 (numpy's correctly rounded float32 division, exp2 and log2).  Both are 2^-22 relative effects on a factor: a fold whose factor
passes its threshold by octaves fires in the kernel as well, possibly an iteration earlier or later.

The planted mistakes (keyword arguments) are the ones a fold can make without any existing test noticing: four drop one of the updates
that keep K, the border entries and the absorbed potentials consistent, the fifth drops the epilogue's re-read.

THE DENORMAL RE-READ is reached: in the '-cold' cases of FOLD_CASES one entry of the hot column lies 63 units below the rest of its row -
2^-91 of the row maximum, 9 octaves inside the range test - and the column fold (factor below 2^-40) takes it under 2^-126.  Families
tried that reach none: a hot column alone (one or several, any position), lopsided dustbins (bin score -55 ... -62, up to 200
iterations), both together (the bin score then flags the pair)."""
import math

import numpy as np

F = np.float32
LOG2E = F(1.4426950408889634)
LN2 = F(0.6931471805599453)
RANGE_HI = F(2.0 ** 40)
RANGE_LO = F(2.0 ** -40)
FLAG_BELOW = F(2.0 ** -100)       # the range test: an entry of K (or a dustbin-column entry) below this hands the pair to the streaming kernel
MIN_NORMAL = F(1.17549435e-38)    # 2^-126: the epilogue re-reads the score of an entry of K below it
SLAB = 512                        # columns of one workgroup: the column fold is decided per slab
KINDS = ('col', 'bM', 'aN', 'row')


def _out(x):
    """not (RANGE_LO < x < RANGE_HI), as the kernel writes it: NaN counts as out of range."""
    return ~((x > RANGE_LO) & (x < RANGE_HI))


def _lg2(x):
    with np.errstate(divide='ignore'):
        return np.log2(x, dtype=F)


def scaling(scores, alpha, iters, fold=True, from_k=True, drop_kr=False, drop_v0=False, drop_kbr=False, drop_kc=False, no_reread=False):
    """One pair: scores [N, M], bin score ``alpha``.  Returns (Z [N+1, M+1] float32, report).

    report: 'flagged' (the pair would be redone by the streaming kernel), 'kmin' (the smallest entry the range test sees),
    'folds' {kind: [iterations in which it fired]} for 'col' (once per slab and iteration: entries (iteration, slab)), 'bM', 'aN', 'row'
    (entries (iteration, number of rows)), 'denormal' (entries of K below 2^-126 when the epilogue reads them), 'maxlog' {kind: the
    largest |log2| the factor reached} - the factor a fold=False run lets grow.

    fold=False: no fold is taken.  Planted mistakes: drop_kr - the column fold without kr *= b; drop_v0 - without v0 += lg2 b; drop_kbr -
    the row fold without kbr *= a; drop_kc - the aN fold without kc *= aN; no_reread - the <false, 4> epilogue without its re-read, lg2 of an
    entry below 2^-126 being -inf as v_log_f32 returns it."""
    s = np.ascontiguousarray(scores, dtype=F)
    N, M = s.shape
    alpha2 = F(F(alpha) * LOG2E)
    norm = F(-math.log(N + M))
    mu = F(1.0) / F(N + M)
    muN = F(M) / F(N + M)
    nu, nuM = mu, F(N) / F(N + M)
    with np.errstate(under='ignore', over='ignore', invalid='ignore', divide='ignore'):
        S2 = s * LOG2E
        mrow = np.maximum(S2.max(axis=1), alpha2)
        u0 = -mrow
        K = np.exp2(S2 - mrow[:, None], dtype=F)
        kb = np.exp2(alpha2 + u0, dtype=F)                  # dustbin-column entries
        a = np.ones(N, F)
        kmin = F(min(K.min(), kb.min()))
        u0N, aN = F(-alpha2), F(1)
        v0, kr, b = np.zeros(M, F), np.ones(M, F), np.ones(M, F)
        v0M, kc, bM = F(0), F(1), F(1)
        folds = {k: [] for k in KINDS}
        maxlog = {k: 0.0 for k in KINDS}

        def see(kind, x):
            x = np.atleast_1d(x)
            v = np.abs(np.log2(x.astype(np.float64)))
            maxlog[kind] = max(maxlog[kind], float(np.nanmax(v)) if np.isfinite(v).any() else float('inf'))

        for it in range(iters):
            # row update (mdgat.py:283)
            psum = (K * b[None, :]).sum(axis=1, dtype=F)
            pd = F((kr * b).sum(dtype=F))
            aN = muN / F(kc * bM + pd)
            a = mu / (kb * bM + psum)
            dsum = F((kb * a).sum(dtype=F))
            # column update (mdgat.py:284)
            q = (K * a[:, None]).sum(axis=0, dtype=F)
            b = nu / (kr * aN + q)
            bM = nuM / F(kc * aN + dsum)
            see('col', b), see('bM', bM), see('aN', aN), see('row', a)
            if not fold:
                continue
            for j0 in range(0, M, SLAB):
                sl = slice(j0, min(j0 + SLAB, M))
                if _out(b[sl]).any():
                    K[:, sl] *= b[sl][None, :]
                    if not drop_v0:
                        v0[sl] += _lg2(b[sl])
                    if not drop_kr:
                        kr[sl] *= b[sl]
                    b[sl] = F(1)
                    folds['col'].append((it, j0 // SLAB))
            if _out(bM):
                kb = kb * bM
                kc = F(kc * bM)
                v0M = F(v0M + _lg2(bM))
                bM = F(1)
                folds['bM'].append(it)
            if _out(aN):
                kr = kr * aN
                if not drop_kc:
                    kc = F(kc * aN)
                u0N = F(u0N + _lg2(aN))
                aN = F(1)
                folds['aN'].append(it)
            rows = _out(a)
            if rows.any():
                K[rows] *= a[rows][:, None]
                if not drop_kbr:
                    kb[rows] *= a[rows]
                u0[rows] += _lg2(a[rows])
                a[rows] = F(1)
                folds['row'].append((it, int(rows.sum())))

        # epilogue: Z = couplings + u + v - norm, natural-log units
        ran = iters > 0
        VM = F(v0M + _lg2(bM)) if ran else F(0)
        U = (u0 + _lg2(a)) if ran else np.zeros(N, F)
        V = (v0 + _lg2(b)) if ran else np.zeros(M, F)
        UN = F(u0N + _lg2(aN)) if ran else F(0)
        under = ~(K >= MIN_NORMAL)
        reread = (S2 + U[:, None] + V[None, :]) * LN2 - norm
        if from_k:
            dU, dV = U - u0, V - v0
            z = (_lg2(K) + dU[:, None] + dV[None, :]) * LN2 - norm
            z = np.where(under, F(-np.inf) if no_reread else reread, z)
        else:
            z = reread
        Z = np.empty((N + 1, M + 1), F)
        Z[:N, :M] = z
        Z[:N, M] = (alpha2 + U + VM) * LN2 - norm
        Z[N, :M] = (alpha2 + UN + V) * LN2 - norm
        Z[N, M] = (alpha2 + UN + VM) * LN2 - norm
    report = {'flagged': bool(kmin < FLAG_BELOW), 'kmin': float(kmin), 'folds': folds, 'denormal': int(under.sum()), 'maxlog': maxlog}
    return Z, report


def bar(ref):
    """The project's bar on Z against the fp64 oracle (tests/test_gpu_ops.py::test_sinkhorn_wide_dynamic_range)."""
    return 1e-4 * max(1.0, float(np.abs(np.asarray(ref)).max()) / 100)


# ---- inputs that reach the folds without raising the range flag ----
# name: (N, M, hot columns, shift, cold entry (row, column, units below the rest of its row) or None, bin score, iterations,
#        the fold kinds the case claims, the scaling instantiation and (GR, GC) it is meant for)
# A hot column (every row's maximum sits in it) drives its b down and every a up, 55 units = 79 octaves apart: the column fold and the row
# fold.  A bin score 55 below the scores with more rows than columns drives bM and aN apart: the two dustbin folds.  The cold entry sits
# in the hot column 63 units below the rest of its row (2^-91 after the row maximum is absorbed, 9 octaves inside the range test): the
# column fold takes it below 2^-126, which is what the re-read of the <false, 4> epilogue is for.
FOLD_CASES = {
    'hot-64x64-c3':        (64, 64, (3,), 55.0, None, 1.0, 20, ('col', 'row'), 'scaling<false,4>', (1, 1)),
    'hot-64x64-c3-cold':   (64, 64, (3,), 55.0, (5, 3, 63.0), 1.0, 20, ('col', 'row'), 'scaling<false,4>', (1, 1)),
    'lopsided-128x40':     (128, 40, (), 0.0, None, -55.0, 100, ('bM', 'aN'), 'scaling<false,4>', (1, 1)),
    'hot-130x65-c64':      (130, 65, (64,), 55.0, None, 1.0, 20, ('col', 'row'), 'scaling<false,4>', (2, 1)),   # a ragged lane's last valid column
    'hot-130x65-every7th': (130, 65, tuple(range(0, 65, 7)), 55.0, None, 1.0, 20, ('col', 'row'), 'scaling<false,4>', (2, 1)),
    'hot-130x65-c3-cold':  (130, 65, (3,), 55.0, (129, 3, 63.0), 1.0, 20, ('col', 'row'), 'scaling<false,4>', (2, 1)),
    'lopsided-130x65':     (130, 65, (), 0.0, None, -55.0, 100, ('bM', 'aN'), 'scaling<false,4>', (2, 1)),
    'hot-513x40-c0':       (513, 40, (0,), 55.0, None, 1.0, 20, ('col', 'row'), 'scaling<false,16>', (5, 1)),      # the first lane
    'lopsided-513x40':     (513, 40, (), 0.0, None, -55.0, 100, ('bM', 'aN'), 'scaling<false,16>', (5, 1)),
    'hot-40x513-c3':       (40, 513, (3,), 55.0, None, 1.0, 20, ('col', 'row'), 'scaling<true,16>', (1, 2)),       # slab 0 folds, slab 1 does not
    'hot-40x513-c512':     (40, 513, (512,), 55.0, None, 1.0, 20, ('col', 'row'), 'scaling<true,16>', (1, 2)),     # the last slab only
    'lopsided-1030x513':   (1030, 513, (), 0.0, None, -55.0, 100, ('bM', 'aN'), 'scaling<true,16>', (9, 2)),
}
FOLD_SEEDS = (3, 4)               # the two fold pairs of fold_batch
DENORMAL_CASES = ('hot-64x64-c3-cold', 'hot-130x65-c3-cold')


def fold_scores(name, seed=3):
    """The scores [N, M] (float32) of a fold case."""
    N, M, hot, shift, cold, *_ = FOLD_CASES[name]
    s = np.random.RandomState(seed).standard_normal((N, M)).astype(F)
    if hot:
        s[:, list(hot)] += F(shift)
    if cold:
        r, c, below = cold
        s[r, c] = np.delete(s[r], c).max() - F(below)
    return s


def plain_scores(N, M, seed=5):
    return (np.random.RandomState(seed).standard_normal((N, M)) * 4.0).astype(F)


def fold_batch(name):
    """The batch the GPU tests run a fold case in: [the case (seed 3), a plain Gaussian pair, the case (seed 4)]."""
    N, M = FOLD_CASES[name][:2]
    return np.stack([fold_scores(name, FOLD_SEEDS[0]), plain_scores(N, M), fold_scores(name, FOLD_SEEDS[1])])


def middle_pair_flagged(name):
    """Whether the plain pair of fold_batch(name) is beyond the range test (tests/test_sinkhorn_scaling_ref.py checks it): a bin score of
    -55 lies more than 100 octaves below the row maxima of scores spread four times as wide."""
    return FOLD_CASES[name][5] < -50


# the inputs of the per-form comparison with the oracle (tests/test_gpu_sinkhorn_forms.py (a))
FORM_ALPHA, FORM_ITERS = 0.7, 20


def form_batch(N, M, B=3):
    return (np.random.RandomState(N * 3 + M).standard_normal((B, N, M)) * 4.0).astype(F)


def fired(report):
    """The fold kinds that fired at least once."""
    return {k for k in KINDS if report['folds'][k]}


def batch(scores, alpha, iters, **kw):
    """scaling() over a batch [B, N, M]: (Z [B, N+1, M+1], [report per pair])."""
    out = [scaling(s, alpha, iters, **kw) for s in np.asarray(scores)]
    return np.stack([z for z, _ in out]), [r for _, r in out]
