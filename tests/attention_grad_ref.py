"""fp64 restatement of attention / dynamic_attention (models/mdgat.py:190-210) and of their gradient, the yardstick of
csrc/attention_grad.hip.  numpy, no autograd.

Library layout: qkv [B, N + M, 3, 4, 32] (q | k | v, head, dim), message and dmsg [B, N + M, 128] (channel = head * 32 + dim); rows
0 .. N - 1 are frame 0, the rest frame 1.  The queries of a frame read the keys and values of their SOURCE: the frame itself, or the
other frame in a cross layer.  ``masks`` = (mask0 [B, 4, N, keys of frame 0's source], mask1 [B, 4, M, keys of frame 1's source]),
True where the row kept the key (``ops.topk_sel_to_masks``); None = every key.  Per (pair, frame, head), s = 1 / sqrt(32):

    S = s Q K^T,   P = softmax of S over the kept keys of each row, exactly 0 elsewhere,   O = P V

and with G = dL/dO:

    D_i = sum_d G_id O_id,   dP = G V^T,   dS_ij = P_ij (dP_ij - D_i)
    dQ = s dS K,   dK = s dS^T Q,   dV = P^T G

The selection is not differentiated (the reference gathers, softmaxes and scatters: autograd sends exactly 0 to the other logits).
A row that keeps no key - no forward writes one, but the selection is an input of the backward - has P = 0 throughout: no message,
dQ = 0, nothing sent to dK and dV, and a tolerance of 0.

The error bound (``tolerances``), derived as head_grad_ref derives its own: a dot product of length K in fp64, in any order, with or
without FMA, is off by at most K u sum|a_k b_k| to first order, u = 2^-53, and the formulas rerun on absolute values give the
magnitudes.  With |Q|, |K|, |V|, |G| the absolute values, P the probabilities themselves and n_i the number of keys row i kept:

    A_S  = s |Q||K|^T           e_S = 32 u A_S                                  (a logit's absolute error)
    rel_i = 2 max over the kept j of e_S(i, j) + n_i u                          (the RELATIVE error of row i of P: a logit error e
                                                                                  moves exp(S - max) by a factor e^e and the
                                                                                  normalising sum by at most as much again; the sum
                                                                                  itself has n_i terms)
    A_dP = |G||V|^T             A_D_i = sum_j P_ij A_dP_ij                      (dP: length 32; D: length 32)
    A_dS = P (A_dP + A_D)       e_dS = A_dS (2 rel_i + (32 + 32) u)             (P appears in front and inside D)
    dQ:  s (e_dS + n_i u A_dS) |K|            closing product over the keys
    dK:  s (e_dS + nq u A_dS)^T |Q|           closing product over the queries
    dV:  (P (rel_i + nq u))^T |G|

Tolerance per entry: 4 x that - a factor 2 for the two implementations compared, 2 for the first-order truncation."""
import os

import numpy as np

SCALE = 1.0 / np.sqrt(32.0)
U = 2.0 ** -53
#         case,                   B, N,  M,  cross, k
CASES = (('full_self_n48',        1, 48, 48, False, 0),
         ('full_cross_n40m56',    1, 40, 56, True,  0),
         ('dyn_self_n48_k16',     1, 48, 48, False, 16),
         ('dyn_cross_n40m56_k16', 1, 40, 56, True,  16),
         ('dyn_self_n48_k1',      1, 48, 48, False, 1),
         ('dyn_cross_n40m56_k1',  1, 40, 56, True,  1),
         ('dyn_cross_b2_n20m28_k16', 2, 20, 28, True, 16))
GOLDEN_FILES = tuple('attention_grad_' + c[0] for c in CASES)


def _scale(dtype):
    """1 / sqrt(32) in ``dtype`` (fp64: SCALE itself)."""
    return SCALE if dtype == np.float64 else 1 / np.sqrt(np.dtype(dtype).type(32))


def _sides(N, M, cross):
    """(query rows, source rows) of frame 0 and of frame 1."""
    f = (slice(0, N), slice(N, N + M))
    return ((f[0], f[1 if cross else 0]), (f[1], f[0 if cross else 1]))


def _heads(x):
    """[B, n, 4, 32] -> [B, 4, n, 32]"""
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1, 3)))


def _softmax(S, mask):
    """Over the kept keys of each row, exactly 0 elsewhere.  A row that keeps no key has P = 0 throughout (no message, no gradient);
    every other row goes through the same operations on the same values as if there were no such row."""
    if mask is not None:
        S = np.where(mask, S, -np.inf)
    mx = S.max(axis=-1, keepdims=True)
    e = np.exp(S - np.where(np.isfinite(mx), mx, 0.0))          # (an empty row: exp(-inf - 0) = 0)
    l = e.sum(axis=-1, keepdims=True)
    return e / np.where(l > 0, l, 1.0)


def _check(qkv, N, M, dtype=np.float64):
    qkv = np.asarray(qkv, dtype=dtype)
    assert qkv.ndim == 5 and qkv.shape[1] == N + M and qkv.shape[2:] == (3, 4, 32), qkv.shape
    return qkv


def logits(qkv, N, M, cross, dtype=np.float64):
    """(S of frame 0's queries [B, 4, N, keys], S of frame 1's), in ``dtype``."""
    qkv = _check(qkv, N, M, dtype)
    return tuple(_scale(qkv.dtype) * (_heads(qkv[:, qs, 0]) @ np.swapaxes(_heads(qkv[:, ks, 1]), -1, -2)) for qs, ks in _sides(N, M, cross))


def probabilities(qkv, N, M, cross, masks=None, dtype=np.float64):
    """(P of frame 0's queries [B, 4, N, keys], P of frame 1's)."""
    return tuple(_softmax(S, None if masks is None else np.asarray(masks[side], dtype=bool))
                 for side, S in enumerate(logits(qkv, N, M, cross, dtype)))


def forward(qkv, N, M, cross, masks=None):
    """message [B, N + M, 128]."""
    qkv = _check(qkv, N, M)
    B = qkv.shape[0]
    msg = np.zeros((B, N + M, 128))
    for (qs, ks), P in zip(_sides(N, M, cross), probabilities(qkv, N, M, cross, masks)):
        O = P @ _heads(qkv[:, ks, 2])
        msg[:, qs] = np.transpose(O, (0, 2, 1, 3)).reshape(B, -1, 128)
    return msg


def _backward(qkv, N, M, cross, dmsg, Ps, mode='grad', e_in=None, e_dmsg=None):
    """mode 'grad': the gradient formulas.  On absolute values: 'mag' the magnitude of every entry (dS = P (dP + D)), 'err' the error
    propagation of the module docstring; ``e_in`` / ``e_dmsg`` (err only): absolute errors the inputs qkv / dmsg arrive with."""
    B = qkv.shape[0]
    out = np.zeros_like(qkv)
    SCALE = _scale(qkv.dtype)
    for (qs, ks), P in zip(_sides(N, M, cross), Ps):
        Q, K, V = _heads(qkv[:, qs, 0]), _heads(qkv[:, ks, 1]), _heads(qkv[:, ks, 2])
        G = _heads(dmsg[:, qs].reshape(B, -1, 4, 32))
        nq = Q.shape[2]
        T = lambda x: np.swapaxes(x, -1, -2)                    # noqa: E731
        dP = G @ T(V)
        if mode == 'grad':
            D = (G * (P @ V)).sum(axis=-1, keepdims=True)
            dS = P * (dP - D)
            dQ, dK, dV = SCALE * (dS @ K), SCALE * (T(dS) @ Q), T(P) @ G
        elif mode == 'mag':
            dS = P * (dP + (P * dP).sum(axis=-1, keepdims=True))
            dQ, dK, dV = SCALE * (dS @ K), SCALE * (T(dS) @ Q), T(P) @ G
        else:
            kept = P > 0
            n_i = kept.sum(axis=-1, keepdims=True)
            e_S = 32 * U * SCALE * (Q @ T(K))
            x_dP = 0.0
            if e_in is not None:
                eQ, eK, eV = _heads(e_in[:, qs, 0]), _heads(e_in[:, ks, 1]), _heads(e_in[:, ks, 2])
                e_S = e_S + SCALE * (eQ @ T(K) + Q @ T(eK))
                x_dP = G @ T(eV)
            if e_dmsg is not None:
                x_dP = x_dP + _heads(e_dmsg[:, qs].reshape(B, -1, 4, 32)) @ T(V)
            rel = 2 * np.where(kept, e_S, 0.0).max(axis=-1, keepdims=True) + n_i * U
            A_dS = P * (dP + (P * dP).sum(axis=-1, keepdims=True))
            e_dS = A_dS * (2 * rel + 64 * U) + P * (x_dP + (P * x_dP).sum(axis=-1, keepdims=True))
            dQ = SCALE * ((e_dS + n_i * U * A_dS) @ K)
            dK = SCALE * (T(e_dS + nq * U * A_dS) @ Q)
            dV = T(P * (rel + nq * U)) @ G
            if e_in is not None:
                dQ, dK = dQ + SCALE * (A_dS @ eK), dK + SCALE * (T(A_dS) @ eQ)
            if e_dmsg is not None:
                dV = dV + T(P) @ _heads(e_dmsg[:, qs].reshape(B, -1, 4, 32))
        out[:, qs, 0] += np.transpose(dQ, (0, 2, 1, 3))
        out[:, ks, 1] += np.transpose(dK, (0, 2, 1, 3))
        out[:, ks, 2] += np.transpose(dV, (0, 2, 1, 3))
    return out


def backward(qkv, N, M, cross, dmsg, masks=None):
    """dqkv [B, N + M, 3, 4, 32]."""
    qkv = _check(qkv, N, M)
    dmsg = np.asarray(dmsg, dtype=np.float64)
    assert dmsg.shape == (qkv.shape[0], N + M, 128), dmsg.shape
    return _backward(qkv, N, M, cross, dmsg, probabilities(qkv, N, M, cross, masks))


def tolerances(qkv, N, M, cross, dmsg, masks=None):
    """Per entry of dqkv, 4 x the first-order error of the module docstring."""
    qkv = _check(qkv, N, M)
    return 4.0 * _backward(np.abs(qkv), N, M, cross, np.abs(np.asarray(dmsg, dtype=np.float64)), probabilities(qkv, N, M, cross, masks), mode='err')


def topk_masks(qkv, N, M, cross, k):
    """The index sets of ``logits.topk(k)`` on the fp64 logits as masks, and the smallest gap between a row's k-th and (k + 1)-th
    largest logit (inf when every key is kept)."""
    qkv = _check(qkv, N, M)
    masks, gap = [], np.inf
    for qs, ks in _sides(N, M, cross):
        S = SCALE * (_heads(qkv[:, qs, 0]) @ np.swapaxes(_heads(qkv[:, ks, 1]), -1, -2))
        order = np.argsort(-S, axis=-1, kind='stable')
        mask = np.zeros(S.shape, dtype=bool)
        np.put_along_axis(mask, order[..., :k], True, axis=-1)
        masks.append(mask)
        if k < S.shape[-1]:
            srt = np.take_along_axis(S, order, axis=-1)
            gap = min(gap, float((srt[..., k - 1] - srt[..., k]).min()))
    return tuple(masks), gap


def backward_longdouble(qkv, N, M, cross, dmsg, masks=None):
    """``backward``, every operation in np.longdouble (x87 extended where the platform has it): dqkv as longdouble."""
    qkv = _check(qkv, N, M, np.longdouble)
    dmsg = np.asarray(dmsg, dtype=np.longdouble)
    assert dmsg.shape == (qkv.shape[0], N + M, 128), dmsg.shape
    return _backward(qkv, N, M, cross, dmsg, probabilities(qkv, N, M, cross, masks, np.longdouble))


def masks_to_words(masks, B, N, M, cross, pad=0):
    """The inverse of ``ops.topk_sel_to_masks``: int32 words [B][4][N + M][W], W = ceil(max(N, M) / 32), bit j of word w = key
    32 w + j of the row's source frame.  ``pad`` (0 or 1) is the value of every bit that addresses no key: the bits at or beyond the
    source's size in its last used word, and every higher word of the row."""
    W = (max(N, M) + 31) // 32
    bits = np.full((B, 4, N + M, W * 32), bool(pad))
    nk = (M, N) if cross else (N, M)
    for side, rows in enumerate((slice(0, N), slice(N, N + M))):
        m = np.asarray(masks[side], dtype=bool)
        assert m.shape == (B, 4, rows.stop - rows.start, nk[side]), (m.shape, side)
        bits[:, :, rows, :nk[side]] = m
    words = (bits.reshape(B, 4, N + M, W, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=-1)
    return words.astype(np.uint32).view(np.int32)


LAZY_NEG, LAZY_TAU = -1e300, 8.0


def lazy_trace(qkv, N, M, cross, masks=None):
    """The decisions of the lazy softmax reference in walk 1 of ag_row_kernel, emulated on the fp64 logits (the decisions only, not the
    kernel's arithmetic).  A wave is 16 consecutive queries of a 64-query tile; lane (query, g), g = 0 .. 3, owns the keys
    16 jb + g + 4 r, r = 0 .. 3, of key block jb; keys past the frame and keys the row did not keep never count.  Every lane starts
    from m = mthr = -1e300; in a block where ANY lane of the wave has its block maximum above its own mthr, EVERY lane of the wave
    sets m = max(m, its block maximum) and mthr = m + 8, rescaling its sums by exp(old m - new m).  (The lanes of a last wave's
    missing queries run too, as the kernel's do: on logits of 0 under the selection of the frame's last query.  They can trigger a
    wave's update and are counted nowhere.)

    Returns a dict of [2, 4] arrays (side, head), over all pairs: ``blocks`` the number of wave-blocks in which some lane that already
    held a kept key rescaled by a factor below 1, ``factor`` the smallest such factor (1.0 if none), ``apart`` the largest distance
    between the references of a row's quarters at the end (quarters that kept a key; 0.0 if no row has two)."""
    out = {'blocks': np.zeros((2, 4), dtype=np.int64), 'factor': np.ones((2, 4)), 'apart': np.zeros((2, 4))}
    for side, S in enumerate(logits(qkv, N, M, cross)):
        B, _, nq, nk = S.shape
        keep = np.ones(S.shape, dtype=bool) if masks is None else np.asarray(masks[side], dtype=bool)
        nw, nblk = (nq + 15) // 16, (nk + 15) // 16
        # [B, 4, wave, query of the wave, key block, r, g]: the missing queries of the last wave, the missing keys of the last block
        Sp = np.zeros((B, 4, nw * 16, nblk * 16))
        Kp = np.zeros(Sp.shape, dtype=bool)
        Sp[:, :, :nq, :nk], Kp[:, :, :nq, :nk] = S, keep
        Kp[:, :, nq:, :nk] = keep[:, :, nq - 1:nq]
        real = (np.arange(nw * 16) < nq).reshape(nw, 16, 1)
        lm_all = np.where(Kp, Sp, LAZY_NEG).reshape(B, 4, nw, 16, nblk, 4, 4).max(axis=5)      # [B, 4, wave, query, block, g]
        m = np.full((B, 4, nw, 16, 4), LAZY_NEG)
        mthr = m.copy()
        has = np.zeros(m.shape, dtype=bool)
        for jb in range(nblk):
            lm = lm_all[..., jb, :]
            fire = (lm > mthr).any(axis=(3, 4), keepdims=True)
            mnew = np.where(fire, np.maximum(m, lm), m)
            shrink = has & real & (mnew > m)
            out['blocks'][side] += shrink.any(axis=(3, 4)).sum(axis=(0, 2))
            fac = np.where(shrink, np.exp(np.where(shrink, m - mnew, 0.0)), 1.0)
            out['factor'][side] = np.minimum(out['factor'][side], fac.min(axis=(0, 2, 3, 4)))
            mthr = np.where(fire, mnew + LAZY_TAU, mthr)
            m = mnew
            has |= lm > LAZY_NEG
        two = real[..., 0] & (has.sum(axis=-1) >= 2)
        apart = np.where(has, m, -np.inf).max(axis=-1) - np.where(has, m, np.inf).min(axis=-1)
        out['apart'][side] = np.where(two, apart, 0.0).max(axis=(0, 2, 3))
    return out


# ---- seeded inputs that reach what Gaussian inputs of unit scale do not: (qkv [B, N + M, 3, 4, 32], dmsg [B, N + M, 128]) ----
def _unit_heads(rs):
    u = rs.standard_normal((4, 32))
    return u / np.linalg.norm(u, axis=-1, keepdims=True)


def _frames(N, M):
    return (slice(0, N), slice(N, N + M))


def gauss(B, N, M, seed, scale):
    """Standard normal; q and k times ``scale``: logits of standard deviation scale^2."""
    rs = np.random.RandomState(seed)
    qkv, dmsg = rs.standard_normal((B, N + M, 3, 4, 32)), rs.standard_normal((B, N + M, 128))
    qkv[:, :, :2] *= scale
    return qkv, dmsg


def ramp(B, N, M, seed, peak=200.0):
    """Noise 0.3 N(0, 1); the k of key j gets a t_j u_head, t rising linearly from -1 to 1 along the frame's keys, the q of query i
    gets +- a c_i u_head (+ for even i, - for odd i, c_i in [0.5, 1]), u_head a unit vector per head, a = sqrt(peak sqrt(32)): the
    logit of (i, j) is +- peak c_i t_j plus noise.  Even rows rise along the keys - the reference moves block after block - and odd
    rows fall: the first block holds the mass and later terms run down toward exp(-2 peak)."""
    rs = np.random.RandomState(seed)
    qkv, dmsg = 0.3 * rs.standard_normal((B, N + M, 3, 4, 32)), rs.standard_normal((B, N + M, 128))
    u, a = _unit_heads(rs), np.sqrt(peak * np.sqrt(32.0))
    for fr in _frames(N, M):
        n = fr.stop - fr.start
        c = rs.uniform(0.5, 1.0, (B, n)) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        qkv[:, fr, 0] += a * c[:, :, None, None] * u
        qkv[:, fr, 1] += a * np.linspace(-1.0, 1.0, n)[None, :, None, None] * u
    return qkv, dmsg


def _spiked(B, N, M, seed, peak, keys):
    rs = np.random.RandomState(seed)
    qkv, dmsg = 1.3 * rs.standard_normal((B, N + M, 3, 4, 32)), rs.standard_normal((B, N + M, 128))
    u, a = _unit_heads(rs), np.sqrt(peak * np.sqrt(32.0))
    qkv[:, :, 0] += a * u
    for fr in _frames(N, M):
        qkv[:, fr, 1][:, keys(fr.stop - fr.start)] += a * u
    return qkv, dmsg


def lastkey(B, N, M, seed, peak=150.0):
    """1.3 N(0, 1), every q plus a u_head and only the LAST key of each frame plus a u_head (a = sqrt(peak sqrt(32))): the dominant
    logit, about ``peak``, arrives in the final key block."""
    return _spiked(B, N, M, seed, peak, lambda n: slice(n - 1, n))


def quarter(B, N, M, seed, peak=120.0):
    """As ``lastkey``, but the keys j = 2 (mod 4) of each frame get a u_head: one lane quarter of every row holds all the mass."""
    return _spiked(B, N, M, seed, peak, lambda n: slice(2, n, 4))


def alternate_rows(dmsg, e=20):
    """dmsg with its rows scaled by 2^e (even rows) and 2^-e (odd rows)."""
    return dmsg * np.where(np.arange(dmsg.shape[1]) % 2 == 0, 2.0 ** e, 2.0 ** -e)[None, :, None]


def varied_masks(B, N, M, cross, seed):
    """Row (row + head) % 6 = 0 .. 5 keeps 0, 1, 2, nk / 2, nk - 1, nk keys of its source's nk, drawn at random."""
    rs = np.random.RandomState(seed)
    masks = []
    for nq, nk in zip((N, M), (M, N) if cross else (N, M)):
        counts = np.array([0, 1, 2, nk // 2, nk - 1, nk])[(np.arange(nq)[None, :] + np.arange(4)[:, None]) % 6]
        masks.append(np.argsort(rs.random_sample((B, 4, nq, nk)), axis=-1) < np.minimum(counts, nk)[None, :, :, None])
    return tuple(masks)


def last_block_masks(B, N, M, cross):
    """Every row keeps the keys of its source's last block of 16 (keys >= 16 floor((nk - 1) / 16)) and no other."""
    return tuple(np.broadcast_to(np.arange(nk) >= 16 * ((nk - 1) // 16), (B, 4, nq, nk)).copy()
                 for nq, nk in zip((N, M), (M, N) if cross else (N, M)))


def constant_masks(B, N, M, cross, value):
    return tuple(np.full((B, 4, nq, nk), bool(value)) for nq, nk in zip((N, M), (M, N) if cross else (N, M)))


FAMILIES = {'gauss_2m12': (gauss, {'scale': 2.0 ** -12}), 'gauss_1.3': (gauss, {'scale': 1.3}), 'gauss_4': (gauss, {'scale': 4.0}),
            'gauss_6': (gauss, {'scale': 6.0}), 'ramp': (ramp, {}), 'lastkey': (lastkey, {}), 'quarter': (quarter, {})}
HARD = ('gauss_4', 'gauss_6', 'ramp', 'lastkey', 'quarter')          # the reference of walk 1 must be seen to move
TINY_FACTOR = ('gauss_6', 'ramp', 'lastkey')                         # ... by a factor below 1e-20 somewhere
#             family,  B, N, M, cross, k
LOGIT_CASES = tuple((f, B, N, M, cross, k) for f in ('gauss_2m12', 'gauss_4', 'gauss_6', 'ramp', 'lastkey', 'quarter')
                    for (B, N, M, cross) in ((2, 49, 65, True), (2, 49, 65, False), (1, 130, 70, True)) for k in (0, 8, 17))
#                 family,  B, N, M, cross
SELECTION_CASES = tuple((f, 2, N, M, cross) for f in ('gauss_1.3', 'gauss_6') for (N, M, cross) in ((49, 65, True), (65, 49, False)))
SELECTION_KINDS = ('varied', 'last_block', 'none', 'all')
SINGLE_CASES = tuple(('gauss_1.3', 3, N, M, cross, k) for (N, M) in ((1, 1), (1, 70), (65, 1)) for cross in (False, True) for k in (0, 1))
INVARIANCE_CASES = (('gauss_4', 2, 49, 65, True, 8), ('gauss_4', 2, 65, 49, False, 0))


def family_inputs(family, B, N, M, cross):
    """The seeded (qkv, dmsg) of a case: one seed per (family, shape, direction)."""
    fn, kw = FAMILIES[family]
    return fn(B, N, M, seed=1000 * sorted(FAMILIES).index(family) + 7 * N + 3 * M + B + int(cross), **kw)


def selection_masks(kind, B, N, M, cross):
    if kind == 'varied':
        return varied_masks(B, N, M, cross, seed=N + 2 * M + int(cross))
    if kind == 'last_block':
        return last_block_masks(B, N, M, cross)
    return constant_masks(B, N, M, cross, kind == 'all')


def worst_fraction(got, want, tol):
    """max over the entries of |got - want| / tol (0 / 0 counts as 0, x / 0 as inf)."""
    got, want, tol = [np.asarray(x, dtype=np.float64) for x in (got, want, tol)]
    assert got.shape == want.shape == tol.shape, (got.shape, want.shape, tol.shape)
    if got.size == 0:
        return 0.0
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(err == 0.0, 0.0, err / tol)
    return float(frac.max())


def load_golden(golden_dir, case):
    """One case of tests/golden/attention_grad_<case>.npz (tools/make_goldens_attention_grad.py): a dict with ``meta`` = [B, N, M,
    cross, k], ``qkv``, ``dmsg``, ``msg``, ``dqkv`` and, for k > 0, ``masks`` (a tuple of two boolean arrays)."""
    with np.load(os.path.join(golden_dir, f'attention_grad_{case}.npz')) as z:
        g = {k: z[k] for k in z.files}
    B, N, M, cross, k = (int(v) for v in g['meta'])
    if k > 0:
        nk = (M, N) if cross else (N, M)
        g['masks'] = tuple(np.unpackbits(g.pop(f'mask{i}_bits'))[:B * 4 * n * nk[i]].reshape(B, 4, n, nk[i]).astype(bool)
                           for i, n in enumerate((N, M)))
    else:
        g['masks'] = None
    return g


# ---- the attention inside the reference's MultiHeadedAttention.forward (models/mdgat.py:223-237), one direction of a cross layer ----
# The reference's view(B, 32, 4, -1) sends channel c of a projection to (dim = c // 4, head = c % 4); the library's channel is
# head * 32 + dim (pack.py).  PERM[library channel] = reference channel.
PERM = (np.arange(32)[None, :] * 4 + np.arange(4)[:, None]).reshape(-1)
MHA_FILES = ('attention_grad_mha_inputs', 'attention_grad_mha_grads')
MHA_GRADS = ('dx', 'dsource', 'dWq', 'dbq', 'dWk', 'dbk', 'dWv', 'dbv', 'dWm', 'dbm')


def mha_qkv(x, source, w):
    """x [B, n, 128], source [B, m, 128] point-major, w: the reference's 'Wq', 'bq', ... 'Wm', 'bm' ([128, 128] / [128]) ->
    (desc [B, n + m, 128], qkv [B, n + m, 3, 4, 32] in the library's layout)."""
    desc = np.concatenate([x, source], axis=1)
    qkv = np.stack([desc @ w['W' + c][PERM].T + w['b' + c][PERM] for c in 'qkv'], axis=2)
    return desc, qkv.reshape(desc.shape[0], desc.shape[1], 3, 4, 32)


def mha_forward(x, source, w, masks, attention=forward):
    """merge(attention(proj(x), proj(source), proj(source))) [B, n, 128]: frame 0 of a cross layer."""
    n, m = x.shape[1], source.shape[1]
    msg = attention(mha_qkv(x, source, w)[1], n, m, True, masks)[:, :n]
    return msg @ w['Wm'][:, PERM].T + w['bm']


def mha_backward(x, source, w, dout, masks, attention=forward, attention_backward=backward):
    """The gradients MHA_GRADS of sum(out * dout), the 1x1 convolutions composed in numpy around the attention's two directions."""
    B, n, m = x.shape[0], x.shape[1], source.shape[1]
    desc, qkv = mha_qkv(x, source, w)
    msg = attention(qkv, n, m, True, masks)[:, :n]
    dmsg = np.concatenate([dout @ w['Wm'][:, PERM], np.zeros((B, m, 128))], axis=1)
    dqkv = attention_backward(qkv, n, m, True, dmsg, masks).reshape(B, n + m, 3, 128)
    g = {'dWm': np.zeros((128, 128)), 'dbm': dout.sum(axis=(0, 1))}
    g['dWm'][:, PERM] = dout.reshape(-1, 128).T @ msg.reshape(-1, 128)
    ddesc = np.zeros_like(desc)
    for i, c in enumerate('qkv'):
        d = dqkv[:, :, i]
        dW, db = np.zeros((128, 128)), np.zeros(128)
        dW[PERM], db[PERM] = d.reshape(-1, 128).T @ desc.reshape(-1, 128), d.sum(axis=(0, 1))
        g['dW' + c], g['db' + c] = dW, db
        ddesc += d @ w['W' + c][PERM]
    g['dx'], g['dsource'] = ddesc[:, :n], ddesc[:, n:]
    return g


def mha_tolerances(x, source, w, dout, masks):
    """The composed bound, by the rules of the module docstring: the projections (length 128) hand the attention a qkv that is off by
    128 u (|desc||W|^T + |b|) and a dmsg off by 128 u |dout||Wm|; ``_backward`` carries both through the attention ('err' mode) next
    to its own error; the closing convolutions add (their length) u (magnitude) and pass the incoming error through |W| / |desc|:
    dW_c: (n + m) rows, ddesc: 3 x 128, dWm: B n rows on |dout|^T |msg| plus |dout|^T e_msg with e_msg = (rel_i + n_i u) P|V| + P e_V,
    rel_i from the logits' own and inherited error as in ``_backward``.  Times 4, as everywhere."""
    B, n, m = x.shape[0], x.shape[1], source.shape[1]
    desc, qkv = mha_qkv(x, source, w)
    aw = {k: np.abs(v) for k, v in w.items()}
    adesc, adout = np.abs(desc), np.abs(dout)
    _, aqkv = mha_qkv(np.abs(x), np.abs(source), aw)
    e_in = 128 * U * aqkv
    admsg = np.concatenate([adout @ aw['Wm'][:, PERM], np.zeros((B, m, 128))], axis=1)
    e_dmsg = 128 * U * admsg
    Ps = probabilities(qkv, n, m, True, masks)
    e = _backward(aqkv, n, m, True, admsg, Ps, mode='err', e_in=e_in, e_dmsg=e_dmsg).reshape(B, n + m, 3, 128)
    A = _backward(aqkv, n, m, True, admsg, Ps, mode='mag').reshape(B, n + m, 3, 128)
    t = {}
    e_desc = np.zeros_like(desc)
    for i, c in enumerate('qkv'):
        dW, db = np.zeros((128, 128)), np.zeros(128)
        dW[PERM] = (e[:, :, i] + (n + m) * U * A[:, :, i]).reshape(-1, 128).T @ adesc.reshape(-1, 128)
        db[PERM] = (e[:, :, i] + (n + m) * U * A[:, :, i]).sum(axis=(0, 1))
        t['dW' + c], t['db' + c] = 4 * dW, 4 * db
        e_desc += (e[:, :, i] + 3 * 128 * U * A[:, :, i]) @ aw['W' + c][PERM]
    t['dx'], t['dsource'] = 4 * e_desc[:, :n], 4 * e_desc[:, n:]
    Q, K, V = _heads(aqkv[:, :n, 0]), _heads(aqkv[:, n:, 1]), _heads(aqkv[:, n:, 2])
    eQ, eK, eV = _heads(e_in[:, :n, 0]), _heads(e_in[:, n:, 1]), _heads(e_in[:, n:, 2])
    kept = Ps[0] > 0
    n_i = kept.sum(axis=-1, keepdims=True)
    e_S = SCALE * (32 * U * (Q @ np.swapaxes(K, -1, -2)) + eQ @ np.swapaxes(K, -1, -2) + Q @ np.swapaxes(eK, -1, -2))
    rel = 2 * np.where(kept, e_S, 0.0).max(axis=-1, keepdims=True) + n_i * U
    unheads = lambda o: np.transpose(o, (0, 2, 1, 3)).reshape(B, n, 128)          # noqa: E731
    amsg, e_msg = unheads(Ps[0] @ V), unheads((rel + n_i * U) * (Ps[0] @ V) + Ps[0] @ eV)
    t['dWm'] = np.zeros((128, 128))
    t['dWm'][:, PERM] = 4 * (adout.reshape(-1, 128).T @ (B * n * U * amsg + e_msg).reshape(-1, 128))
    t['dbm'] = 4 * B * n * U * adout.sum(axis=(0, 1))
    return t


def load_mha(golden_dir):
    """tests/golden/attention_grad_mha_{inputs,grads}.npz as one dict: 'x', 'source' (point-major), 'w' (the weights), 'dout', 'out',
    'k', 'masks' (frame 0's from the reference, frame 1's - which receives no gradient - the top-k of its own logits), the MHA_GRADS."""
    g = {}
    for name in MHA_FILES:
        with np.load(os.path.join(golden_dir, name + '.npz')) as z:
            g.update({k: z[k] for k in z.files})
    B, n, m, k = (int(v) for v in g['meta'])
    g['w'] = {k2: g.pop(k2) for k2 in ('Wq', 'bq', 'Wk', 'bk', 'Wv', 'bv', 'Wm', 'bm')}
    mask0 = np.unpackbits(g.pop('mask0_bits'))[:B * 4 * n * m].reshape(B, 4, n, m).astype(bool)
    own, _ = topk_masks(mha_qkv(g['x'], g['source'], g['w'])[1], n, m, True, k)
    g['masks'], g['k'] = (mask0, own[1]), k
    return g
