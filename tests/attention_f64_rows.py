"""Inputs for fp64 dynamic attention (csrc/f64.hip) whose logit rows have a chosen shape, and the cases built from them
(tests/test_attention_f64_rows.py proves on the CPU which branches of the row select they reach; tests/test_gpu_attention_f64_forms.py
runs them).

A unit is (pair, frame, head).  Head 0 of every frame is the control: dense random q and K, bell-shaped rows.  In heads 1 - 3 the queries
are ONE-HOT within the head, q[r] = c_r e_d: logit[r, j] = c_r K[j, d] / sqrt(32) is a single nonzero term, so column d of the unit's keys
IS the shape of row r, and two keys that agree in column d have bitwise equal logits in the kernel and in any reference.  Columns 0 - 7 of a
unit's keys hold the eight shapes of COLUMNS (below, in units of the logit at c = 1); row r reads column r % 8 with the factor c_r of
`pattern`: both signs (a negative c_r reverses the row: outliers above become outliers below, the left tail the right one), the
magnitudes 2^-30, 2^-12, 1 and 16 (powers of two: the shape is the same to the bit at every scale; |logit| <= 256 everywhere), and
c_r = 0 - a constant row, every logit zero, all keys tied.  Rows r % 16 == 7 of the dense units are constant as well.

Ties are planted by rank, for both signs where the frame has room:
  dup     more than 32 EXACT copies of one value straddling the k-th place (36 - 40; beyond 32 fp32-tied candidates the kernel keeps the
          lowest keys, which is the fp64 ranking only when the fp64 values are equal too), and max(40, k + 8) copies of the smallest value -
          for a negative c_r the tie group that holds the row maximum;
  list32  32 values 1.5 (1 + i 1e-10), i = 0 .. 31, straddling the k-th place: one fp32 value, 32 fp64 values - the list at its capacity;
          on random keys, one of them the frame's last (the ragged last block);
  list2   the (k+1)-th value a copy of the k-th moved by 1e-10 of itself."""
import functools

import numpy as np
import torch

SQRT32 = 32 ** 0.5
MAGS = (2.0 ** -30, 2.0 ** -12, 1.0, 16.0)
COLUMNS = ('normal', 'out', 'tail', 'bimodal', 'narrow', 'dup', 'list32', 'list2')
PATTERNS = 9
DENSE_CONST_EVERY, DENSE_CONST_AT = 16, 7


def pattern(r):
    """row r of a one-hot unit -> (column, pattern index, c_r)"""
    d = r % 8
    p = (r // 8 + 3 * d) % PATTERNS
    if p == 8:
        return d, p, 0.0
    return d, p, (1.0 if p % 2 == 0 else -1.0) * MAGS[p // 2]


def _straddle(k, g, nk):
    """first rank (from the top, 0-based) of a group of g equal-ish values that holds places k and k + 1"""
    return int(np.clip(k - g // 2, max(0, k + 1 - g), min(k - 1, nk - g)))


def list32_mirrored(nk, k):
    """does a frame of nk keys have room for the second list32 group, the one a negative c_r brings to the k-th place?"""
    return nk >= 2 * (_straddle(k, 32, nk) + 32) + 8


def _place(vals, nk, rs, last=None):
    """vals by rank -> by key, on a random permutation; rank `last` goes to the frame's last key"""
    perm = rs.permutation(nk)
    if last is not None:
        i = int(np.nonzero(perm == nk - 1)[0][0])
        perm[i], perm[last] = perm[last], perm[i]
    out = np.empty(nk)
    out[perm] = vals
    return out


def column(name, nk, k, rs):
    """One shape: nk logits at c = 1.  k: the launch's top-k (< nk)"""
    n = rs.standard_normal(nk)
    if name == 'normal':
        return 1.3 * n
    if name == 'out':                  # three outliers 48 bulk deviations up, on keys both searches sample
        v = 0.25 * n
        v[:3] = (12.0, 12.5, 11.5)
        return v
    if name == 'tail':
        t = -np.exp(1.5 * n)
        return t * (16.0 / np.abs(t).max())
    if name == 'bimodal':
        hi = rs.permutation(nk) < max(1, nk // 10)
        return np.where(hi, 5.0, -5.0) + 0.3 * n
    if name == 'narrow':               # c = -16: all logits in -200 +- 10
        return 12.5 + 0.6 * rs.uniform(-1.0, 1.0, nk)
    vals = np.sort(1.3 * n)[::-1].copy()
    if name == 'dup':
        g = min(40, nk - 4)
        a = _straddle(k, g, nk)
        vals[a:a + g] = vals[a]
        g2 = max(40, k + 8)
        if a + g + g2 + 2 <= nk:
            vals[nk - g2:] = vals[nk - g2]
        return _place(vals, nk, rs, last=a)
    if name == 'list32':
        a = _straddle(k, 32, nk)
        grp = 1.5 * (1.0 + 1e-10 * np.arange(31, -1, -1))
        mirrored = list32_mirrored(nk, k)
        low = nk - a - 32 - (a + 32 if mirrored else 0)
        parts = [np.sort(rs.uniform(2.0, 4.0, a))[::-1], grp, np.sort(rs.uniform(-1.0, 1.0, low))[::-1]]
        if mirrored:
            parts += [-grp[::-1], np.sort(rs.uniform(-4.0, -2.0, a))[::-1]]
        return _place(np.concatenate(parts), nk, rs, last=a + 7)
    if name == 'list2':
        vals += 8.0                    # (bell-shaped around 8: no k-th value near zero, where 1e-10 of it would vanish beside the row's largest)
        vals[k] = vals[k - 1] - abs(vals[k - 1]) * 1e-10
        if nk - k - 1 > k + 1:
            vals[nk - k - 1] = vals[nk - k] + abs(vals[nk - k]) * 1e-10
        return _place(vals, nk, rs)
    raise KeyError(name)


def make_pair(n, m, k, cross, seed):
    """-> qkv [n + m, 3, 4, 32] float64 (numpy) of one pair.  k: the launch's top-k; a frame of at most k keys gets the shapes for nk - 1"""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((n + m, 3, 4, 32)) * 1.3
    lo = (0, n)
    cnt = (n, m)
    for side in range(2):
        src = 1 - side if cross else side
        nq, nk = cnt[side], cnt[src]
        q = x[lo[side]:lo[side] + nq, 0]
        kk = x[lo[src]:lo[src] + nk, 1]
        q[DENSE_CONST_AT::DENSE_CONST_EVERY, 0] = 0.0
        for h in (1, 2, 3):
            if nk < 40:                # (no room for the planted groups: dense, like head 0)
                q[DENSE_CONST_AT::DENSE_CONST_EVERY, h] = 0.0
                continue
            for d, name in enumerate(COLUMNS):
                kk[:, h, d] = column(name, nk, min(k, nk - 1), rs) * SQRT32
            q[:, h] = 0.0
            for r in range(nq):
                d, _, c = pattern(r)
                q[r, h, d] = c
    return x


def one_hot(nk):
    return nk >= 40


class Case:
    """One launch: B pairs in slots of N x M (ragged: `counts` = the pairs' own sizes, NaN in the padding)"""

    def __init__(self, name, N, M, k, cross, B=None, counts=None, seed=0):
        self.name, self.N, self.M, self.k, self.cross, self.counts = name, N, M, k, cross, counts
        self.B = len(counts) if counts else B
        self.seed = seed

    @property
    def id(self):
        return f'{self.name}-k{self.k}-{"cross" if self.cross else "self"}'

    def pair_counts(self):
        return self.counts if self.counts else ((self.N, self.M),) * self.B

    def pair_seed(self, b):
        return 1000 * self.seed + 10 * b + int(self.cross)

    @functools.lru_cache(maxsize=None)
    def qkv(self):
        """[B, N + M, 3, 4, 32] float64, read-only for every test that shares it"""
        x = np.full((self.B, self.N + self.M, 3, 4, 32), np.nan)
        for b, (n, m) in enumerate(self.pair_counts()):
            p = make_pair(n, m, self.k, self.cross, self.pair_seed(b))
            x[b, :n] = p[:n]
            x[b, self.N:self.N + m] = p[n:]
        return torch.from_numpy(x)

    def units(self):
        """(b, side, head, query rows (lo, n), key rows (lo, n)) of every unit"""
        for b, (n, m) in enumerate(self.pair_counts()):
            cnt, lo = (n, m), (0, self.N)
            for side in range(2):
                src = 1 - side if self.cross else side
                for h in range(4):
                    yield b, side, h, (lo[side], cnt[side]), (lo[src], cnt[src])

    @functools.lru_cache(maxsize=None)
    def reference(self):
        """{(b, side): (logits [4, nq, nk] as the oracle forms them, kept [4, nq, nk] bool)}: the top k of every row under the total order
        (fp64 logit descending, key ascending) - torch.topk's keys wherever those are specified, the lowest keys among exact ties"""
        x = self.qkv()
        out = {}
        for b, side, h, (ql, nq), (kl, nk) in self.units():
            if h:
                continue
            q = x[b, ql:ql + nq, 0].permute(2, 1, 0)[None]          # [1, dh, H, n]: the oracle's layout
            kk = x[b, kl:kl + nk, 1].permute(2, 1, 0)[None]
            logits = (torch.einsum('bdhn,bdhm->bhnm', q, kk) / 32 ** 0.5)[0]
            order = torch.sort(logits, dim=-1, descending=True, stable=True).indices[..., :min(self.k, nk)]
            kept = torch.zeros_like(logits, dtype=torch.bool).scatter_(-1, order, True)
            out[b, side] = (logits, kept)
        return out


# the smallest launches that reach each search form and both ways a row is loaded (a whole row nk == 16 NV, or a guarded one)
SHAPES = (('128x100', 128, 100, 16, 2),        # quad<8> whole / guarded, the histograms in a region of their own
          ('256x130', 256, 130, 32, 2),        # quad<16> whole / guarded
          ('512x257', 512, 257, 64, 2),        # quad<32>, the histogram inside the row's rounding image
          ('520x40', 520, 40, 32, 1),          # row<16>, and row<8> on 40 keys
          ('1030x40', 1030, 40, 32, 1),        # row<32>
          ('520x500', 520, 500, 32, 1),        # row<8> on a frame whose size fits the launch's zq: the seeded start
          ('128x100', 128, 100, 1, 2), ('128x100', 128, 100, 99, 2), ('520x40', 520, 40, 1, 1), ('520x40', 520, 40, 39, 1))
RAGGED = (('raggedA', ((300, 100), (100, 300), (512, 257), (128, 128)), (32,)),             # at most 512 keys, the smallest count <= 256
          ('raggedB', ((520, 40), (40, 520), (600, 600), (64, 64)), (32, 40)))              # beyond 512; k = 40 = a pair's own count

UNIFORM_CASES = tuple(Case(name, N, M, k, cross, B=B, seed=i + 1) for i, (name, N, M, k, B) in enumerate(SHAPES) for cross in (False, True))
RAGGED_CASES = tuple(Case(name, max(n for n, _ in counts), max(m for _, m in counts), k, cross, counts=counts, seed=20 + i)
                     for i, (name, counts, ks) in enumerate(RAGGED) for k in ks for cross in (False, True))
CASES = UNIFORM_CASES + RAGGED_CASES
