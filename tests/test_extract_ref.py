"""CPU checks of the extraction yardstick (tests/extract_ref.py): the oracle's tie rules against plain loops, every input builder of
tests/test_gpu_extract.py against what it claims to plant (in the oracle's fp64 Z), and the shape lists against mirrors of the
launchers' kernel choice."""
import math

import pytest
import torch

from extract_ref import (ALLDUST_SHAPE, CONST_KINDS, EXTRACT_SHAPES, F64_CASES, GAP_MIN, SK_ITERS, SK_SHAPES, THR, THR_MARGIN,
                         TIE_VARIANTS, alldust_Z, alldust_scores, ambiguous, bin_score_C, check_extraction, dustbin_share_C, f32, f64_kernel,
                         f64_streaming_wave, naive_extract, oracle_extract, pick_threshold, planted_Z, scaling_kernel, scores_A, scores_B,
                         scores_C, sk_lane, sk_tiling, sk_wave, streaming_kernel, tie_positions, wide_range_scores)
from oracle import mdgat_oracle as O


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:2], b[:2])) and all(float((x.double() - y.double()).abs().max()) < 1e-15 and torch.equal(x == 0, y == 0) for x, y in zip(a[2:], b[2:]))


# ------------------------------------------------------------------------------------------------- (a) the oracle's tie behaviour
@pytest.mark.parametrize('mode', range(4))
def test_oracle_ties_against_plain_loops(mode):
    """extract_matches on small matrices with planted ties against a double loop with a strict compare: first index in rows and in
    columns, a dustbin entry that ties with an inner one loses, and exp(v) == threshold is not a match."""
    g = torch.Generator().manual_seed(mode)
    for B, n, m in ((1, 1, 1), (1, 4, 6), (3, 6, 4), (2, 5, 5)):
        Z = -1.0 - torch.rand(B, n + 1, m + 1, generator=g, dtype=torch.float64)
        if n > 3 and m > 3:
            Z[:, 1, 1] = Z[:, 1, 3] = -0.5                      # row tie
            Z[:, 0, 2] = Z[:, 3, 2] = -0.4                      # column tie
            Z[:, 2, 0] = Z[:, 2, m] = -0.3                      # inner ties with the dustbin column
            Z[:, 3, 3] = Z[:, n, 3] = -0.2                      # inner ties with the dustbin row
            Z[0, 0, 0] = math.log(0.5)                          # exp == threshold
        for thr in (0.5, 0.2):
            assert _same(oracle_extract(Z, mode, thr), naive_extract(Z, mode, thr)), (B, n, m, thr)
    Zc = torch.zeros(2, 6, 5, dtype=torch.float64)              # everything ties, the dustbins included: index 0 on both sides
    r = oracle_extract(Zc, mode, 0.5)
    assert _same(r, naive_extract(Zc, mode, 0.5)) and (r[0][:, 0] == 0).all() and (r[1][:, 0] == 0).all()
    if mode != 3:                                               # (3: only row 0 and column 0 point at each other)
        assert (r[0] == 0).all() and (r[1] == 0).all()
    assert (oracle_extract(Zc, 2, 1.0)[0] == -1).all()          # exp(0) == 1.0 is not above a threshold of 1.0
    assert (oracle_extract(Zc, 2, f32(1.0 - 1e-6))[0] == 0).all()


def test_oracle_tie_rules_one_by_one():
    Z = torch.full((1, 4, 4), -5.0, dtype=torch.float64)
    Z[0, 0, 1] = Z[0, 0, 2] = -1.0                              # row 0: columns 1 and 2 tie -> 1
    Z[0, 1, 0] = Z[0, 2, 0] = -1.5                              # column 0: rows 1 and 2 tie -> 1
    Z[0, 2, 3] = -1.5                                           # row 2: column 0 ties with the dustbin -> 0
    Z[0, 3, 2] = -1.0                                           # column 2: row 0 ties with the dustbin -> 0
    m0, m1, s0, s1 = oracle_extract(Z, 0, 0.2)
    assert m0[0].tolist() == [1, 0, 0] and m1[0].tolist() == [1, 0, 0]
    Z[0, 2, 3] = -1.4                                           # the dustbin strictly larger
    assert oracle_extract(Z, 0, 0.2)[0][0].tolist() == [1, 0, -1]
    m0, m1, s0, s1 = oracle_extract(Z, 2, math.exp(-1.0))       # strict threshold: exp(-1) is not above exp(-1)
    assert m0[0].tolist() == [-1, -1, -1] and s0.abs().max() == 0
    none = alldust_Z(3, 'none')
    for mode in (0, 1):
        m0, m1, s0, s1 = oracle_extract(none, mode, 0.2)
        assert (m0 == -1).all() and (m1 >= 0).all() and s0.abs().max() == 0 and s1.abs().max() == 0       # the batch-wide rule
        m0, m1, s0, s1 = oracle_extract(alldust_Z(3, 'one', 1), mode, 0.2)
        assert int((m0 >= 0).sum()) == 1 and int(m0[1, 11]) == 5 and (s1[0] > 0).any() == (mode == 0)


def test_check_extraction_catches_one_wrong_entry():
    Z, _ = planted_Z(2, 9, 7, 0)
    r = [t.clone() for t in oracle_extract(Z, 0, THR)]
    check_extraction(Z, *r, 0, THR)
    r[1][1, 3] = (r[1][1, 3] + 1) % 9
    with pytest.raises(AssertionError, match='matches1'):
        check_extraction(Z, *r, 0, THR)
    r = [t.clone() for t in oracle_extract(Z, 0, THR)]
    r[2][0, 0] += 2e-6
    with pytest.raises(AssertionError, match='scores'):
        check_extraction(Z, *r, 0, THR)


# ------------------------------------------------------------------------------------------------- (b) the builders
@pytest.mark.parametrize('B,N,M', EXTRACT_SHAPES)
def test_planted_Z_holds_its_plants(B, N, M):
    Z, plants = planted_Z(B, N, M, seed=N + M, zero_maxima=True)
    assert Z.dtype == torch.float32
    kinds = {p[0] for p in plants}
    if min(N, M) >= 60:
        assert kinds == {'row_tie', 'col_tie', 'row_bin_tie', 'col_bin_tie', 'row_bin', 'col_bin', 'thr_above', 'thr_below', 'stolen', 'mutual',
                         'zero', 'above1'}
    rmax, cmax = Z[:, :N, :].max(2).values, Z[:, :, :M].max(1).values
    i0, i1 = Z[:, :N, :].argmax(2), Z[:, :, :M].argmax(1)
    for p in plants:
        k = p[0]
        if k == 'row_tie':
            _, r, c1, c2 = p
            assert c1 < c2 and (Z[:, r, c1] == Z[:, r, c2]).all() and (Z[:, r, c1] == rmax[:, r]).all() and (i0[:, r] == c1).all()
            if M > 64:
                assert c1 // 64 != c2 // 64
        elif k == 'col_tie':
            _, c, r1, r2 = p
            assert r1 < r2 and (Z[:, r1, c] == Z[:, r2, c]).all() and (Z[:, r1, c] == cmax[:, c]).all() and (i1[:, c] == r1).all()
            if N > 16:
                assert r1 % 16 != r2 % 16                      # extract_kernel's row scan: rows i, i + 16, ... belong to one wave
        elif k == 'row_bin_tie':
            _, r, c = p
            assert (Z[:, r, c] == Z[:, r, M]).all() and (Z[:, r, c] == rmax[:, r]).all() and (i0[:, r] == c).all()
        elif k == 'col_bin_tie':
            _, c, r = p
            assert (Z[:, r, c] == Z[:, N, c]).all() and (Z[:, r, c] == cmax[:, c]).all() and (i1[:, c] == r).all()
        elif k == 'row_bin':
            assert (i0[:, p[1]] == M).all()
        elif k == 'col_bin':
            assert (i1[:, p[1]] == N).all()
        elif k in ('thr_above', 'thr_below'):
            _, r, c = p
            e = Z[:, r, c].double().exp()
            assert (i0[:, r] == c).all() and (i1[:, c] == r).all()
            assert ((e > THR * (1 + 0.9 * THR_MARGIN)) if k == 'thr_above' else (e < THR * (1 - 0.9 * THR_MARGIN))).all()
        elif k == 'stolen':
            _, a, b, c = p
            assert (i0[:, a] == c).all() and (i0[:, b] == c).all() and (i1[:, c] == b).all()
        elif k == 'mutual':
            assert (i0[:, p[1]] == p[2]).all() and (i1[:, p[2]] == p[1]).all()
        elif k == 'zero':
            assert (Z[:, p[1], p[2]] == 0).all() and (i0[:, p[1]] == p[2]).all() and math.exp(0.0) == 1.0
        elif k == 'above1':
            assert (i0[:, p[1]] == p[2]).all()
    if min(N, M) >= 60:
        for mode in (2, 3):                                    # both sides of the threshold are populated
            m0 = oracle_extract(Z, mode, THR)[0]
            assert (m0 >= 0).any() and (m0 < 0).any()


def _oracle_Z(s, bin_score, iters, pairs=(0, -1)):
    idx = sorted({p % s.shape[0] for p in pairs})
    return O.log_optimal_transport(s[idx].double(), torch.tensor(float(bin_score), dtype=torch.float64), iters)


def _check_A(Z, pos, exact):
    ra, rb, ca, cb = pos
    v = Z[:, ra, ca]
    rest = Z.clone()
    for r in (ra, rb):
        for c in (ca, cb):
            # the four entries tie - exactly where the oracle's Z is the reference (the fp64 cases).  torch's logsumexp does not reduce
            # every row in the same order, so at some shapes duplicated rows come out an ulp apart: the fp32 cases, which compare a
            # kernel with its OWN Z and assert there that the entries are bit-equal, only need the structure
            assert torch.equal(Z[:, r, c], v) if exact else float((Z[:, r, c] - v).abs().max()) < 1e-13
            rest[:, r, c] = -math.inf
    for r in (ra, rb):                                         # ... and are the maxima of their rows and columns, by a margin
        assert (rest[:, r, :].max(1).values < v - 1e-3).all()
    for c in (ca, cb):
        assert (rest[:, :, c].max(1).values < v - 1e-3).all()
    if not exact:
        return
    for mode in range(4):
        m0, m1, _, _ = oracle_extract(Z, mode, pick_threshold(Z))
        assert (m0[:, ra] == ca).all() and (m1[:, ca] == ra).all()
        if mode != 3:                                          # (3: row rb and column cb are not pointed back at)
            assert (m0[:, rb] == ca).all() and (m1[:, cb] == ra).all()


@pytest.mark.parametrize('B,N,M', SK_SHAPES)
def test_score_builders_fp32_cases(B, N, M):
    """Builders A, B, C at the fp32 shapes, on the oracle's fp64 Z (first and last pair of a batch)."""
    for variant in TIE_VARIANTS[:2]:
        s, pos = scores_A(B, N, M, variant)
        _check_A(_oracle_Z(s, 1.0, SK_ITERS), pos, exact=False)
    s = scores_C(B, N, M)
    share = dustbin_share_C(_oracle_Z(s, bin_score_C(N, M), SK_ITERS))
    assert 0.1 <= share <= 0.9, share
    _check_B(B, N, M, torch.float32)


def _check_B(B, N, M, dtype):
    for kind, (value, bin_score, iters) in CONST_KINDS.items():
        s = scores_B(1, N, M, dtype, value)
        Z = _oracle_Z(s, bin_score, SK_ITERS if iters is None else iters)
        assert (Z[:, :N, :M] == Z[:, :1, :1]).all()            # every inner entry ties
        i0, i1 = Z[:, :N, :].argmax(2), Z[:, :, :M].argmax(1)
        if kind == 'dustbin':
            assert (i0 == M).all() and (i1 == N).all()
        elif kind == 'inner':                                  # the shorter frame's side picks index 0 with the dustbin in the running
            assert (i0 == 0).all() if N <= M else (i1 == 0).all()
        else:
            assert (i0 == 0).all() and (i1 == 0).all()
        assert (Z[:, :N, :M].argmax(2) == 0).all() and (Z[:, :N, :M].argmax(1) == 0).all()      # the superglue branches: index 0 on both sides
        if kind == 'border':
            assert (Z == Z[:, :1, :1]).all() and float(Z.max()) < 0        # ... with the dustbins as well


@pytest.mark.parametrize('B,N,M,iters,form', [c for c in F64_CASES if c[4] != 1])
def test_score_builders_fp64_cases(B, N, M, iters, form):
    """The fp64 cases: the plants of builder A tie exactly and are the maxima, and NO row or column of any committed seed is left
    out of the index comparison (two best candidates equal, or more than GAP_MIN apart)."""
    alpha = torch.tensor(1.0, dtype=torch.float64)
    for variant in TIE_VARIANTS:
        s, pos = scores_A(B, N, M, variant, dtype=torch.float64)
        Z = O.log_optimal_transport(s, alpha, iters)
        _check_A(Z, pos, exact=True)
        assert [ambiguous(Z, mode) for mode in (0, 2)] == [0, 0], variant
    s = scores_C(B, N, M, dtype=torch.float64)
    Z = O.log_optimal_transport(s, torch.tensor(bin_score_C(N, M), dtype=torch.float64), iters)
    assert 0.1 <= dustbin_share_C(Z) <= 0.9
    assert [ambiguous(Z, mode) for mode in (0, 2)] == [0, 0]
    _check_B(B, N, M, torch.float64)
    assert GAP_MIN == 1e-9


def test_alldust_builders():
    N, M = ALLDUST_SHAPE
    for B in (1, 3, 70):
        for kind, which in [('none', 0), ('all', 0)] + [('one', w) for w in sorted({0, B // 2, B - 1})]:
            s, bin_score = alldust_scores(B, kind, which)
            Z = O.log_optimal_transport(s.double(), torch.tensor(bin_score, dtype=torch.float64), SK_ITERS)
            rows = (Z[:, :N, :].argmax(2) < M).sum(1)
            cols = (Z[:, :, :M].argmax(1) < N).sum(1)
            assert (cols > 0).all()                            # matching_scores1 is not zero by itself
            if kind == 'none':
                assert int(rows.sum()) == 0
            elif kind == 'one':
                assert int(rows.sum()) == 1 and int(rows[which]) == 1 and int(Z[which, 11, :].argmax()) == 5
            else:
                assert (rows > 0).all()
            Zp = alldust_Z(B, kind, which)
            rows = (Zp[:, :-1, :].argmax(2) < Zp.shape[2] - 1).sum(1)
            assert kind == 'all' or (Zp[:, :, :-1].argmax(1) < Zp.shape[1] - 1).all()
            assert int(rows.sum()) == (0 if kind == 'none' else 1 if kind == 'one' else int(rows.sum())) and (kind != 'all' or (rows > 0).all())


def test_pick_threshold_separates():
    Z, _ = planted_Z(2, 64, 64, 1)
    thr = pick_threshold(Z)
    e = torch.cat([Z[:, :-1, :-1].max(2).values.flatten(), Z[:, :-1, :-1].max(1).values.flatten()]).double().exp()
    assert (e > thr).any() and (e < thr).any() and ((e - thr).abs() >= 0.4 * THR_MARGIN * thr).all() and thr == f32(thr)
    assert pick_threshold(torch.zeros(1, 4, 4)) == 0.5


# ------------------------------------------------------------------------------------------------- (c) the shape lists
def test_dispatch_mirrors():
    assert sk_tiling(1, 1) == (1, 1) and sk_tiling(128, 512) == (1, 1) and sk_tiling(129, 513) == (2, 2) and sk_tiling(2048, 2048) == (16, 4)
    assert scaling_kernel(512, 512) == ('false', 4) and scaling_kernel(513, 512) == ('false', 16) and scaling_kernel(1, 513) == ('true', 16)
    assert scaling_kernel(2049, 4) is None
    assert [streaming_kernel(9, M) for M in (64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049)] == \
        [(1, 16), (2, 16), (2, 16), (4, 16), (4, 16), (8, 16), (8, 16), (16, 8), (16, 8), (32, 8), (32, 8), None]
    assert f64_kernel(575, 575) == ('resident', 18) and f64_kernel(576, 575)[0] == 'resident' and f64_kernel(577, 575)[0] == 'streaming'
    assert f64_kernel(575, 576)[0] == 'streaming' and f64_kernel(96, 96, 1) == ('streaming', 5, 3)
    assert f64_kernel(10, 639)[1] == 5 and f64_kernel(10, 640)[1] == 9 and f64_kernel(10, 1151)[1] == 9 and f64_kernel(10, 1152)[1] == 17
    assert f64_kernel(2175, 2175) == ('streaming', 17, 68) and f64_kernel(2176, 8) is None and f64_kernel(8, 2176) is None


def test_shape_lists_reach_every_kernel_form():
    sk = {(N, M) for _, N, M in SK_SHAPES}
    assert {scaling_kernel(N, M) for N, M in sk} == {('false', 4), ('false', 16), ('true', 16)}
    GR4 = {sk_tiling(N, M)[0] for N, M in sk if scaling_kernel(N, M) == ('false', 4)}
    assert {1, 4} <= GR4
    assert {N for N, M in sk if scaling_kernel(N, M) == ('false', 16)} >= {513, 900, 2048}
    assert {M for N, M in sk if scaling_kernel(N, M) == ('true', 16)} >= {513, 700, 2048} and (2048, 2048) in sk
    assert {sk_tiling(N, M)[0] for N, M in sk} >= {1, 16} and {sk_tiling(N, M)[1] for N, M in sk} >= {1, 4}
    assert {N % 128 for N, M in sk} >= {0, 1} and any(1 < N % 128 < 127 for N, M in sk)            # the last row slab: one row, some, full
    assert {M % 512 for N, M in sk} >= {0, 1} and any(1 < M % 512 < 511 for N, M in sk)
    assert {B for B, _, _ in SK_SHAPES} >= {1, 3, 70}
    assert {streaming_kernel(N, M) for N, M in sk} == {(1, 16), (2, 16), (4, 16), (8, 16), (16, 8), (32, 8)}
    # builder A's ties: other wave of one slab and other slab (rows); other lane of one slab and other slab (columns)
    rows, cols = set(), set()
    for N, M in sk:
        for variant in TIE_VARIANTS[:2]:
            ra, rb, ca, cb = tie_positions(N, M, variant)
            (sa, wa), (sb, wb) = sk_wave(ra), sk_wave(rb)
            rows.add('slab' if sa != sb else 'wave' if wa != wb else 'same')
            (ta, la), (tb, lb) = sk_lane(ca), sk_lane(cb)
            cols.add('slab' if ta != tb else 'lane' if la != lb else 'same')
            if variant == 'slabs':
                assert (sa != sb) == (sk_tiling(N, M)[0] > 1) and (ta != tb) == (sk_tiling(N, M)[1] > 1)
    assert rows >= {'slab', 'wave'} and cols >= {'slab', 'lane'}
    # the extraction from a Z in memory
    ex = {(B, N, M) for B, N, M in EXTRACT_SHAPES}
    assert ex >= {(1, 1, 1), (3, 9, 7), (2, 64, 64), (2, 130, 2048), (2, 2048, 130), (1, 2048, 2048), (5, 600, 700)}
    assert any(N == 1 for _, N, _ in ex) and any(M == 1 for _, _, M in ex)
    assert {min(N, M) for _, N, M in ex if max(N, M) == 2048} >= {1, 17, 64, 130}
    # the fp64 forms
    forms = {f64_kernel(N, M, form)[:2] if f64_kernel(N, M, form)[0] == 'streaming' else ('resident',) for _, N, M, _, form in F64_CASES}
    assert forms == {('resident',), ('streaming', 5), ('streaming', 9), ('streaming', 17)}
    assert {(N, M) for _, N, M, _, form in F64_CASES if form != 1} >= {(575, 575), (576, 300), (300, 576), (2175, 130), (130, 2175)}
    assert all(it <= 20 for _, N, M, it, _ in F64_CASES if max(N, M) > 576)
    for _, N, M, _, form in F64_CASES:
        ra, rb, _, _ = tie_positions(N, M, 'interleave')
        (sa, wa), (sb, wb) = f64_streaming_wave(ra), f64_streaming_wave(rb)
        assert ra < rb and sa == sb and wa > wb                 # the smaller row in the HIGHER wave
        ra, rb, _, _ = tie_positions(N, M, 'slabs')
        assert ra // 32 != rb // 32


def test_wide_range_builder_is_the_range_fallback_tests():
    s = wide_range_scores(5, 64, 64, (1,))
    assert float(s[1].max() - s[1].min()) > 200 and float(s[0].max() - s[0].min()) < 40
