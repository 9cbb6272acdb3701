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


def _sides(N, M, cross):
    """(query rows, source rows) of frame 0 and of frame 1."""
    f = (slice(0, N), slice(N, N + M))
    return ((f[0], f[1 if cross else 0]), (f[1], f[0 if cross else 1]))


def _heads(x):
    """[B, n, 4, 32] -> [B, 4, n, 32]"""
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1, 3)))


def _softmax(S, mask):
    if mask is not None:
        S = np.where(mask, S, -np.inf)
    e = np.exp(S - S.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def _check(qkv, N, M):
    qkv = np.asarray(qkv, dtype=np.float64)
    assert qkv.ndim == 5 and qkv.shape[1] == N + M and qkv.shape[2:] == (3, 4, 32), qkv.shape
    return qkv


def probabilities(qkv, N, M, cross, masks=None):
    """(P of frame 0's queries [B, 4, N, keys], P of frame 1's)."""
    qkv = _check(qkv, N, M)
    out = []
    for side, (qs, ks) in enumerate(_sides(N, M, cross)):
        Q, K = _heads(qkv[:, qs, 0]), _heads(qkv[:, ks, 1])
        out.append(_softmax(SCALE * (Q @ np.swapaxes(K, -1, -2)), None if masks is None else np.asarray(masks[side], dtype=bool)))
    return tuple(out)


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
