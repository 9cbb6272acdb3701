"""fp64 restatement of the matching head (models/mdgat.py:397, 430-431) and of its gradient, the yardstick of csrc/head_grad.hip.
numpy, no autograd.

Library layout, point-major: desc0 [B, N, 128], desc1 [B, M, 128], W [128 out, 128 in], b [128], s = 1 / sqrt(128).

    md0 = desc0 W^T + b,  md1 = desc1 W^T + b,  scores[z] = s md0[z] md1[z]^T                         [B, N, M]

and with G = dL/dscores:

    dmd0[z] = s G[z] md1[z]           dmd1[z] = s G[z]^T md0[z]
    ddesc0  = dmd0 W                  ddesc1  = dmd1 W
    dW[c, k] = sum over every point p of every pair, both frames, of dmd[p, c] desc[p, k]
    db[c]    = the same sum of dmd[p, c]

The error bound (``tolerances``), derived: a dot product of length K in fp64, in any order, with or without FMA, is off by at most
K u sum|a_k b_k| to first order, u = 2^-53.  The same formulas run on absolute values give the magnitude A of every entry
(|md| = |desc||W|^T + |b|, |dmd| = s|G||md|, |ddesc| = |dmd||W|, |dW| = sum |dmd|^T|desc|, |db| = sum |dmd|), and K is the sum of the
contraction lengths on the way to the entry: scores 128 + 128; ddesc0 128 + M + 128; ddesc1 128 + N + 128; dW and db
128 + max(N, M) + B (N + M).  Tolerance per entry: 4 K u A - a factor 2 for the two implementations compared, 2 for the first-order
truncation; an output rounded to float32 adds 2^-24 |value|."""
import os

import numpy as np

D = 128
SCALE = 1.0 / np.sqrt(128.0)
U = 2.0 ** -53
GOLDEN_FILES = ('head_grad', 'head_grad_n64_superglue', 'head_grad_n64_triplet_loss', 'head_grad_n64_gap_loss', 'head_grad_n48m64_gap_loss')


def _f64(*xs):
    return [np.asarray(x, dtype=np.float64) for x in xs]


def _weight(W):
    W = np.asarray(W, dtype=np.float64)
    return W.reshape(D, D) if W.ndim == 3 else W


def project(desc, W, b):
    return desc @ _weight(W).T + np.asarray(b, dtype=np.float64)


def forward(desc0, desc1, W, b):
    """scores [B, N, M]."""
    desc0, desc1 = _f64(desc0, desc1)
    return SCALE * (project(desc0, W, b) @ project(desc1, W, b).transpose(0, 2, 1))


def backward(desc0, desc1, W, b, G):
    """(ddesc0 [B, N, 128], ddesc1 [B, M, 128], dW [128, 128], db [128])."""
    desc0, desc1, G = _f64(desc0, desc1, G)
    W = _weight(W)
    md0, md1 = project(desc0, W, b), project(desc1, W, b)
    dmd0 = SCALE * (G @ md1)
    dmd1 = SCALE * (G.transpose(0, 2, 1) @ md0)
    dW = dmd0.reshape(-1, D).T @ desc0.reshape(-1, D) + dmd1.reshape(-1, D).T @ desc1.reshape(-1, D)
    db = dmd0.sum(axis=(0, 1)) + dmd1.sum(axis=(0, 1))
    return dmd0 @ W, dmd1 @ W, dW, db


def magnitudes(desc0, desc1, W, b, G=None):
    """The formulas on absolute values: {'scores', and with G 'ddesc0', 'ddesc1', 'dW', 'db'} -> the magnitude A of every entry."""
    d0, d1 = [np.abs(x) for x in _f64(desc0, desc1)]
    W, b = np.abs(_weight(W)), np.abs(np.asarray(b, dtype=np.float64))
    out = {'scores': forward(d0, d1, W, b)}
    if G is not None:
        out['ddesc0'], out['ddesc1'], out['dW'], out['db'] = backward(d0, d1, W, b, np.abs(np.asarray(G, dtype=np.float64)))
    return out


def contraction_lengths(B, N, M):
    red = D + max(N, M) + B * (N + M)
    return {'scores': D + D, 'ddesc0': D + M + D, 'ddesc1': D + N + D, 'dW': red, 'db': red}


def tolerances(desc0, desc1, W, b, G=None):
    """Per entry 4 K u A, for the names of ``magnitudes``."""
    B, N, M = np.shape(desc0)[0], np.shape(desc0)[1], np.shape(desc1)[1]
    K = contraction_lengths(B, N, M)
    return {k: 4.0 * K[k] * U * A for k, A in magnitudes(desc0, desc1, W, b, G).items()}


def worst_fraction(got, want, tol, out_eps=0.0):
    """max over the entries of (|got - want| - out_eps |want|) / tol (0 / 0 counts as 0, x / 0 as inf)."""
    got, want, tol = _f64(got, want, tol)
    assert got.shape == want.shape == tol.shape, (got.shape, want.shape, tol.shape)
    if got.size == 0:
        return 0.0
    err = np.maximum(np.abs(got - want) - out_eps * np.abs(want), 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(err == 0.0, 0.0, err / tol)
    return float(frac.max())


def load_golden(golden_dir):
    """The arrays of tests/golden/head_grad*.npz (tools/make_goldens_head_grad.py) as one dict."""
    out = {}
    for name in GOLDEN_FILES:
        with np.load(os.path.join(golden_dir, name + '.npz')) as z:
            out.update({k: z[k] for k in z.files})
    return out
