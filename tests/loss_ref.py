"""fp64 restatement of MDGAT's three losses (models/mdgat.py:486-594) in row / column form, the yardstick of csrc/loss.hip.

Z [B, n+1, m+1] (row n: dustbin row, column m: dustbin column), gt0 [B, n] / gt1 [B, m] with -1 = dustbin.  t(z) = -log(exp(z))
literally, as the reference applies it: -z where exp(z) is a normal number, imprecise in its subnormal band (below about -708.4)
and +inf below about -745.1.  ``pair_losses`` gives one value per pair: superglue / triplet the pair's ratio / mean (the
reference's loss is their mean), gap the pair's loss (the reference returns that vector)."""
import numpy as np


def t(z):
    with np.errstate(divide='ignore', over='ignore', under='ignore'):
        return -np.log(np.exp(z))


def clamp0(x):
    return np.where(x < 0, 0.0, x)          # torch.clamp(min=0) keeps NaN


def _pos(gt, dust):
    g = np.asarray(gt, dtype=np.int64)
    return np.where(g == -1, dust, g)


def pair_losses(Z, gt0, gt1, method, gamma=0.5):
    Z = np.asarray(Z, dtype=np.float64)
    B, n, m = Z.shape[0], Z.shape[1] - 1, Z.shape[2] - 1
    out = np.empty(B)
    for b in range(B):
        z = Z[b]
        g1 = np.asarray(gt1[b], dtype=np.int64)
        p0, p1 = _pos(gt0[b], m), _pos(g1, n)
        rows, cols = np.arange(n), np.arange(m)
        pos_r = z[rows, p0]                              # Z[i, gt0(i)]
        pos_c = z[p1, cols]                              # Z[gt1(j), j]
        if method == 'superglue':
            tp = pos_r.sum()
            un = g1 == -1                                # only a literal -1 counts
            tn = z[n, cols[un]].sum()
            out[b] = (-tp - tn) / (un.sum() + m)
            continue
        keep_r = np.ones((n, m + 1), dtype=bool)
        keep_r[rows, p0] = False                         # row i: the columns j != gt0(i)
        keep_c = np.ones((n + 1, m), dtype=bool)
        keep_c[p1, cols] = False                         # column j: the rows i != gt1(j)
        if method == 'triplet_loss':
            neg_r = np.where(keep_r, z[:n, :], -np.inf).max(axis=1)
            neg_c = np.where(keep_c, z[:, :m], -np.inf).max(axis=0)
            terms = np.concatenate([clamp0(t(pos_r) - t(neg_r) + gamma), clamp0(t(pos_c) - t(neg_c) + gamma)])
            out[b] = terms.mean()
        elif method == 'gap_loss':
            tz = t(z)
            row = np.where(keep_r, clamp0(t(pos_r)[:, None] - tz[:n, :] + gamma), 0.0).sum(axis=1)
            # The column half is not per column of Z.  The reference lists the m positives Z[gt1(j), j] and the n m other entries of
            # Z[:, :m] each in ROW-MAJOR order and lays the second list out as an n x m matrix V: term c pairs the c-th positive in
            # that order with column c of V.  (Per column of Z only when every positive lies in the dustbin row: positives' rows that
            # increase with j put P in column order, but V's entries still shift by the positives taken out before them.)
            P = tz[:, :m][~keep_c]                       # t of the positives, row-major
            V = tz[:, :m][keep_c].reshape(n, m)          # t of the others, row-major, n x m
            col = clamp0(P[None, :] - V + gamma).sum(axis=0)
            out[b] = (np.mean(2 * np.log(row + 1)) + np.mean(2 * np.log(col + 1))) / 2
        else:
            raise ValueError(method)
    return out


def module_loss(Z, gt0, gt1, method, gamma=0.5):
    """What the reference's forward returns as 'loss': 0-d mean for superglue / triplet, [B] for gap."""
    v = pair_losses(Z, gt0, gt1, method, gamma)
    return v if method == 'gap_loss' else np.float64(v.mean())


# ---- ground-truth patterns for the kernel tests (tests/test_gpu_loss.py) ----
GT_PATTERNS = ('partial', 'reversed', 'all_dustbin', 'non_injective', 'explicit_dustbin')


def gt_pattern(name, n, m, rs):
    """(gt0 [n], gt1 [m]) int64 of one pair.  rs: a numpy RandomState.
    partial:          a random partial matching (3/5 of min(n, m) pairs), the rest -1;
    reversed:         the first min(n, m) rows and columns matched in reverse (gt1[j] = k - 1 - j): the positives' rows fall with j,
                      so gap's row-major P is the columns backwards;
    all_dustbin:      every gt -1: all positives in the dustbin row / column;
    non_injective:    gt1 sends the first half of the columns to row 0 and the rest to row n // 2 (one row holds >= m / 2 positives),
                      gt0 random in [-1, m);
    explicit_dustbin: partial, with about half of the unmatched entries given as the dustbin index itself (m in gt0, n in gt1)."""
    g0 = np.full(n, -1, dtype=np.int64)
    g1 = np.full(m, -1, dtype=np.int64)
    if name in ('partial', 'explicit_dustbin'):
        k = max(1, 3 * min(n, m) // 5)
        rows, cols = rs.permutation(n)[:k], rs.permutation(m)[:k]
        g0[rows], g1[cols] = cols, rows
        if name == 'explicit_dustbin':
            g0[(g0 == -1) & (rs.rand(n) < 0.5)] = m
            g1[(g1 == -1) & (rs.rand(m) < 0.5)] = n
    elif name == 'reversed':
        k = min(n, m)
        g0[:k] = np.arange(k - 1, -1, -1)
        g1[:k] = np.arange(k - 1, -1, -1)
    elif name == 'non_injective':
        g1[:] = n // 2
        g1[:m // 2] = 0
        g0[:] = rs.randint(-1, m, n)
    elif name != 'all_dustbin':
        raise ValueError(name)
    return g0, g1


def gt_batch(names, n, m, seed):
    """gt0 [B, n], gt1 [B, m]: pair b gets pattern names[b]."""
    rs = np.random.RandomState(seed)
    pairs = [gt_pattern(p, n, m, rs) for p in names]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
