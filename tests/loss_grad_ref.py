"""fp64 restatement of the GRADIENT of MDGAT's three losses with respect to Z, the yardstick of csrc/loss_grad.hip: the derivative of
tests/loss_ref.py::pair_losses written out in numpy, no autograd.

``pair_grads(Z, gt0, gt1, method, gamma, dloss)`` -> dZ [B, n+1, m+1] = sum_b dloss[b] d pair_losses[b] / dZ, with the conventions of torch
autograd on the reference's code (models/mdgat.py:486-594):

* torch.clamp(x, min=0) passes the gradient where x >= 0 (an exact 0 is active, NaN is not);
* t(z) = -log(exp(z)) is differentiated literally: a gradient g on t becomes (-g / e) * e on z, e = exp(z) - -g to an ulp where e is
  normal, -+inf where 1 / e overflows, NaN where e == 0, also for g == 0.  gap passes every entry of Z[:n] and of Z[:, :m] through t,
  triplet only the positives and the hard negatives;
* gap repeats a positive against its partners BEFORE applying t: its gradient is count x (-w / e) * e over the active partners,
  (-0 / e) * e when none is active;
* arg-max ties (triplet): the lowest index, the rule of this library (np.argmax); torch.topk leaves the choice open.
* a gt index outside [-1, m] / [-1, n]: the pair's dZ is NaN throughout.

``clamp_margin`` / ``triplet_top_gap`` measure how close the inputs come to the only places where two correct implementations may
differ discretely."""
import numpy as np

from loss_ref import _pos, clamp0, t


def dt_dz(g, z):
    with np.errstate(all='ignore'):
        e = np.exp(z)
        return (-np.asarray(g, dtype=np.float64) / e) * e


def _gt_ok(g0, g1, n, m, method):
    ok = np.all((g0 >= -1) & (g0 <= m))
    if method != 'superglue':
        ok = ok and np.all((g1 >= -1) & (g1 <= n))
    return bool(ok)


def _masks(n, m, p0, p1):
    keep_r = np.ones((n, m + 1), dtype=bool)
    keep_r[np.arange(n), p0] = False
    keep_c = np.ones((n + 1, m), dtype=bool)
    keep_c[p1, np.arange(m)] = False
    return keep_r, keep_c


def _positive(count, w, z):
    """count x dt_dz(w) for count > 0, dt_dz(0) for none"""
    with np.errstate(all='ignore'):
        return np.where(count > 0, count * dt_dz(w, z), dt_dz(np.zeros_like(z), z))


def _gap_parts(z, p0, p1, gamma):
    """The clamp arguments of gap's two halves with where they come from: (X_r [n, m+1], keep_r), (X_c [n, m], (pi, pj), (vi, vj))."""
    n, m = z.shape[0] - 1, z.shape[1] - 1
    keep_r, keep_c = _masks(n, m, p0, p1)
    tz = t(z)
    with np.errstate(invalid='ignore'):
        X_r = tz[np.arange(n), p0][:, None] - tz[:n, :] + gamma
        pi, pj = np.nonzero(~keep_c)                      # P, row-major
        vi, vj = np.nonzero(keep_c)                       # V, row-major, n x m
        vi, vj = vi.reshape(n, m), vj.reshape(n, m)
        X_c = tz[pi, pj][None, :] - tz[vi, vj] + gamma
    return X_r, keep_r, X_c, (pi, pj), (vi, vj)


def _triplet_parts(z, p0, p1):
    n, m = z.shape[0] - 1, z.shape[1] - 1
    keep_r, keep_c = _masks(n, m, p0, p1)
    neg_r = np.where(keep_r, z[:n, :], -np.inf).argmax(axis=1)      # lowest index on ties
    neg_c = np.where(keep_c, z[:, :m], -np.inf).argmax(axis=0)
    return keep_r, keep_c, neg_r, neg_c


def pair_grads(Z, gt0, gt1, method, gamma=0.5, dloss=None):
    Z = np.asarray(Z, dtype=np.float64)
    B, n, m = Z.shape[0], Z.shape[1] - 1, Z.shape[2] - 1
    dloss = np.ones(B) if dloss is None else np.asarray(dloss, dtype=np.float64).reshape(B)
    out = np.zeros_like(Z)
    rows, cols = np.arange(n), np.arange(m)
    for b in range(B):
        z, g, d = Z[b], dloss[b], out[b]
        g0, g1 = np.asarray(gt0[b], dtype=np.int64), np.asarray(gt1[b], dtype=np.int64)
        if not _gt_ok(g0, g1, n, m, method):
            d[:] = np.nan
            continue
        p0, p1 = _pos(g0, m), _pos(g1, n)
        with np.errstate(all='ignore'):
            if method == 'superglue':
                un = g1 == -1
                w = -g / (un.sum() + m)
                d[rows, p0] = w
                d[n, cols[un]] = w
            elif method == 'triplet_loss':
                _, _, neg_r, neg_c = _triplet_parts(z, p0, p1)
                w = g / (n + m)
                w_r = np.where(t(z[rows, p0]) - t(z[rows, neg_r]) + gamma >= 0, w, 0.0)
                w_c = np.where(t(z[p1, cols]) - t(z[neg_c, cols]) + gamma >= 0, w, 0.0)
                d[rows, p0] += dt_dz(w_r, z[rows, p0])              # (each index list has no repeats: += is safe)
                d[rows, neg_r] += dt_dz(-w_r, z[rows, neg_r])
                d[p1, cols] += dt_dz(w_c, z[p1, cols])
                d[neg_c, cols] += dt_dz(-w_c, z[neg_c, cols])
            elif method == 'gap_loss':
                X_r, keep_r, X_c, (pi, pj), (vi, vj) = _gap_parts(z, p0, p1, gamma)
                act = keep_r & (X_r >= 0)
                w_r = g / (n * (np.where(keep_r, clamp0(X_r), 0.0).sum(axis=1) + 1))
                row = dt_dz(np.where(act, -w_r[:, None], 0.0), z[:n, :])
                row[rows, p0] = _positive(act.sum(axis=1), w_r, z[rows, p0])
                d[:n, :] += row
                act = X_c >= 0
                w_c = g / (m * (clamp0(X_c).sum(axis=0) + 1))
                d[vi, vj] += dt_dz(np.where(act, -w_c[None, :], 0.0), z[vi, vj])
                d[pi, pj] += _positive(act.sum(axis=0), w_c, z[pi, pj])
            else:
                raise ValueError(method)
    return out


def clamp_margin(Z, gt0, gt1, method, gamma=0.5):
    """The smallest |clamp argument| over the batch (inf for superglue, which has none): a gradient computed in another order of
    operations may flip the activity of a term whose argument is this close to 0."""
    Z = np.asarray(Z, dtype=np.float64)
    n, m = Z.shape[1] - 1, Z.shape[2] - 1
    best = np.inf
    rows, cols = np.arange(n), np.arange(m)
    for z, g0, g1 in zip(Z, gt0, gt1):
        p0, p1 = _pos(np.asarray(g0, dtype=np.int64), m), _pos(np.asarray(g1, dtype=np.int64), n)
        with np.errstate(all='ignore'):
            if method == 'triplet_loss':
                _, _, neg_r, neg_c = _triplet_parts(z, p0, p1)
                xs = [t(z[rows, p0]) - t(z[rows, neg_r]) + gamma, t(z[p1, cols]) - t(z[neg_c, cols]) + gamma]
            elif method == 'gap_loss':
                X_r, keep_r, X_c, _, _ = _gap_parts(z, p0, p1, gamma)
                xs = [X_r[keep_r], X_c]
            else:
                continue
            for x in xs:
                x = np.abs(x[np.isfinite(x)])
                if x.size:
                    best = min(best, float(x.min()))
    return best


def triplet_top_gap(Z, gt0, gt1):
    """The smallest difference between the two largest non-positive entries of a row / column over the batch (inf where a row or
    column has only one): triplet's choice of negative is open below it."""
    Z = np.asarray(Z, dtype=np.float64)
    n, m = Z.shape[1] - 1, Z.shape[2] - 1
    best = np.inf
    for z, g0, g1 in zip(Z, gt0, gt1):
        p0, p1 = _pos(np.asarray(g0, dtype=np.int64), m), _pos(np.asarray(g1, dtype=np.int64), n)
        keep_r, keep_c = _masks(n, m, p0, p1)
        for v in (np.where(keep_r, z[:n, :], -np.inf), np.where(keep_c, z[:, :m], -np.inf).T):
            if v.shape[1] < 2:
                continue
            top = np.sort(v, axis=1)[:, -2:]
            with np.errstate(invalid='ignore'):
                gap = top[:, 1] - top[:, 0]
            gap = gap[np.isfinite(gap)]
            if gap.size:
                best = min(best, float(gap.min()))
    return best


def tolerance(n, m, dZ_b):
    """|difference| allowed between two fp64 evaluations of one pair's dZ in different summation orders: every entry is a sum of at
    most max(n, m) + 2 terms of one sign pattern and each weight holds one sum S of at most max(n, m) + 1 non-negative terms."""
    fin = np.abs(dZ_b[np.isfinite(dZ_b)])
    return 4 * (n + m + 2) * 2.0 ** -53 * (float(fin.max()) if fin.size else 0.0)


def golden_dloss(g, case, meth):
    """dloss [B] of a case of tests/golden/loss_grad.npz: the reference's loss is the mean over pairs for superglue / triplet (one weight), [B] for gap."""
    B = int(g[f'{case}_meta'][0])
    w = g[f'{case}_{meth}_w']
    return np.asarray(w, dtype=np.float64) if meth == 'gap_loss' else np.full(B, float(w) / B)
