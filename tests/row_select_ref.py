"""A numpy model of the two row selects of the fp64 dynamic attention kernel (csrc/row_search.hpp: topk_quad_search, four rows per wave,
frames of at most 512 keys; topk_row_search, one row per wave, beyond) and of the tie rule csrc/f64.hip builds on them (RowSel).  It
runs on the fp32 roundings of a row's fp64 logits and says which way the search takes on that row - it decides nothing about the
result: the k-th largest is the k-th largest whichever way it is found.  tests/test_attention_f64_rows.py uses it to prove that the
inputs of tests/attention_f64_rows.py reach every branch of either search in every instantiation.

Modelled: the sampling of the moments (quad: registers i % 2 == 0 of keys s + 16 i, scaled by 2 / nk; row: i % 4 == 0 of keys lane + 64 i,
4 / nk), zq as the launcher computes it from the launch's largest key count, where the select starts (the quad's base aligned to its digit
position), the restart from the minimum, and the levels of the radix select.  The device sums the moments in another order than numpy
does: `analyse` therefore also says whether the start's class survives moving the start by +- 0.05 deviations."""
import math

import numpy as np

A_LIST = 32                # f64.hip
RQ_START_BELOW = 0.25      # row_search.hpp: topk_quad_search starts this far below mean + zq sd
RS_START_BELOW = 1.0       # topk_row_search
FORMS = ('quad<8>', 'quad<16>', 'quad<32>', 'row<8>', 'row<16>', 'row<32>')
STARTS = ('seeded', 'restart', 'from_min')
TIES = ('mode0', 'mode1', 'list2', 'list32')

_f32 = np.float32


def normal_quantile_upper(p):
    """f64_normal_quantile_upper of f64.hip (Abramowitz-Stegun 26.2.23), as the float the kernel receives"""
    if p <= 0.0:
        return _f32(8.0)
    if p >= 1.0:
        return _f32(-8.0)
    upper = p < 0.5
    pp = p if upper else 1.0 - p
    t = math.sqrt(-2.0 * math.log(pp))
    x = t - (2.515517 + 0.802853 * t + 0.010328 * t * t) / (1.0 + 1.432788 * t + 0.189269 * t * t + 0.001308 * t * t * t)
    return _f32(x if upper else -x)


def zq_of(k, nk_max):
    return normal_quantile_upper((k - 0.5) / nk_max)


def search_form(nk, nk_max):
    """The search a frame of nk keys gets in a launch whose largest (padded) frame has nk_max keys"""
    if nk_max <= 512:
        return 'quad<8>' if nk <= 128 else 'quad<16>' if nk <= 256 else 'quad<32>'
    return 'row<8>' if nk <= 512 else 'row<16>' if nk <= 1024 else 'row<32>'


def f2ord(f):
    """monotone image of float32 values in the unsigned integers (as int64 arrays, for overflow-free arithmetic)"""
    b = np.asarray(f, dtype=_f32).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, (~b) & 0xffffffff, b | 0x80000000)


def _clz32(x):
    return 32 - int(x).bit_length()


def _moments(row, nk, quad):
    idx = np.arange(nk)
    sampled = (idx // 16) % 2 == 0 if quad else (idx // 64) % 4 == 0
    g = row[sampled]
    g = np.where(g > _f32(-3.0e38), g, _f32(0))
    s1 = g.sum(dtype=_f32)
    s2 = (g * g).sum(dtype=_f32)
    inv_n = _f32(2.0 if quad else 4.0) / _f32(nk)
    mu = s1 * inv_n
    sd = np.sqrt(np.maximum(s2 * inv_n - mu * mu, _f32(0)))
    return _f32(mu), _f32(sd)


def _quad_range(lo, omx):
    h = 24 - _clz32((omx - lo) | 0xff)
    b = lo & ~((1 << h) - 1)
    if ((omx - b) >> h) >= 256:
        h += 1
        b = lo & ~((1 << h) - 1)
    return b, h


def _start(o, omn, omx, mu, sd, zq, below, quad, k):
    """-> (class, base, shift, values at or above the unaligned start)"""
    cand = int(f2ord(_f32(mu + (_f32(zq) - _f32(below)) * sd)))
    n_cand = int((o >= cand).sum())
    if quad:
        if cand < omx:
            base, sh = _quad_range(cand, omx)
            if int((o >= base).sum()) < k:
                b2, s2 = _quad_range(1, omx)
                return 'restart', b2, s2, int((o >= base).sum())
            return 'seeded', base, sh, n_cand
        base, sh = _quad_range(omn, omx)
        return 'from_min', base, sh, len(o)
    if omn < cand < omx:
        if n_cand < k:
            return 'restart', omn, 24 - _clz32((omx - omn) | 0xff), n_cand
        return 'seeded', cand, 24 - _clz32((omx - cand) | 0xff), n_cand
    return 'from_min', omn, 24 - _clz32((omx - omn) | 0xff), len(o)


def analyse(row32, k, zq, form):
    """row32: the fp32 roundings of one row's logits (the frame's own keys only); form: one of FORMS.  -> dict:
    start (STARTS), robust (the class survives +- 0.05 sd and has the margin in values the tests ask for), levels, exit ('single' |
    'digits'), narrow (the last level had fewer than 256 digits), mode (0, 1, 2), list (tied candidates in mode 2), thr, c_gt, c_ge,
    tie (TIES or None)"""
    quad = form.startswith('quad')
    row = np.asarray(row32, dtype=_f32) + _f32(0)          # (-0.0 counts as +0.0)
    nk = len(row)
    assert 0 < k < nk
    o = f2ord(row)
    omn, omx = int(o.min()), int(o.max())
    mu, sd = _moments(row, nk, quad)
    below = RQ_START_BELOW if quad else RS_START_BELOW
    start, base, sh, n_at = _start(o, omn, omx, mu, sd, zq, below, quad, k)
    moved = {_start(o, omn, omx, mu, sd, zq, below + d, quad, k)[0] for d in (-0.05, 0.05)}
    robust = moved == {start}
    if start == 'seeded':
        robust = robust and n_at >= k + max(2, k // 8)
    elif start == 'restart':
        robust = robust and n_at <= k // 2
    above, width, levels = 0, 256, 0
    while True:
        levels += 1
        if quad:
            d = ((o >> sh) - (base >> sh)) & 0xffffffff
            play = d < width
        else:
            d = (o - base) >> sh
            play = (o >= base) & (d < width)
        hist = np.bincount(d[play], minlength=256)
        assert above + int(hist.sum()) >= k, 'the model restarts on the first level only'
        from_top = above + np.cumsum(hist[::-1])[::-1]             # values in play in this bin and above it
        b = int(np.nonzero(from_top >= k)[0][-1])
        ceq = int(hist[b])
        above = int(from_top[b]) - ceq
        base += b << sh
        narrow = width < 256
        if sh == 0:
            how = 'digits'
            break
        if ceq == 1:
            how = 'single'
            base = int(o[play & (d == b)].max())
            break
        width = 256 if sh >= 8 else 1 << sh
        sh = sh - 8 if sh > 8 else 0
    c_gt, c_ge = above, above + ceq
    assert c_gt == int((o > base).sum()) and c_ge == int((o >= base).sum()) and c_gt < k <= c_ge, 'the model selects the k-th largest'
    mode = 0 if c_ge == k else 2 if ceq <= A_LIST else 1
    tie = 'mode0' if mode == 0 else 'mode1' if mode == 1 else 'list2' if ceq == 2 else 'list32' if ceq == A_LIST else None
    return dict(start=start, robust=robust, levels=levels, exit=how, narrow=narrow, mode=mode, list=ceq if mode == 2 else 0,
                thr=base, c_gt=c_gt, c_ge=c_ge, tie=tie)
