"""Match extraction (models/mdgat.py:441-483) in every kernel that decides an arg-max, on inputs with planted ties and boundary
values (tests/extract_ref.py; tests/test_extract_ref.py shows on the CPU that the plants are there):
extract_kernel scanning a Z in memory, the epilogue of sinkhorn_scaling_kernel in its three instantiations with the slab merge in
extract_kernel, redone pairs, the batch-wide all-dustbin rule in its ticket and its deferred form, and the two fp64 Sinkhorn forms.
The fp32 kernels are compared with the rules applied in fp64 to the Z they returned themselves (the epilogue arg-maxes the registers
it stores), the fp64 kernels with the oracle's fp64 Z."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from extract_ref import (ALLDUST_SHAPE, CONST_KINDS, EXTRACT_SHAPES, F64_CASES, SCORE_TOL, SK_ITERS, SK_SHAPES, THR, TIE_VARIANTS,  # noqa: E402
                         alldust_Z, alldust_scores, ambiguous, bin_score_C, check_extraction, dustbin_share_C, pick_threshold,
                         planted_Z, scores_A, scores_B, scores_C, wide_range_scores)
from mdgat_matcher_amd import MDGAT, _lib, ops, synth  # noqa: E402
from oracle import mdgat_oracle as O  # noqa: E402

DEV = 'cuda:0'
WORST = {'score': 0.0}      # the largest score error seen (printed by the last test of the file)


def _note(err):
    WORST['score'] = max(WORST['score'], err)


# -------------------------------------------------------------------------------------------- extract_kernel on a Z in memory
@pytest.mark.parametrize('B,N,M', EXTRACT_SHAPES)
def test_extract_planted_Z(B, N, M):
    """ops.extract on a random Z with equal row maxima in different lanes and strides, equal column maxima, inner entries equal to the
    dustbin entry, a dustbin strictly larger, exp(max) 1e-4 either side of the threshold and rows that point at a column which points
    elsewhere - in all four branches."""
    Z, plants = planted_Z(B, N, M, seed=N + M)
    for mode in range(4):
        _note(check_extraction(Z, *ops.extract(Z.to(DEV), mode, THR), mode, THR))
    # the plants, by name (check_extraction has compared every row and column already)
    m0, m1, _, _ = ops.extract(Z.to(DEV), _lib.EXTRACT_DUSTBIN, THR)
    t0, t1, _, _ = ops.extract(Z.to(DEV), _lib.EXTRACT_THRESHOLD, THR)
    for p in plants:
        if p[0] == 'row_tie':
            assert (m0[:, p[1]] == p[2]).all() and (t0[:, p[1]] == p[2]).all()
        elif p[0] == 'col_tie':
            assert (m1[:, p[1]] == p[2]).all() and (t1[:, p[1]] == p[2]).all()
        elif p[0] in ('row_bin_tie', 'col_bin_tie'):
            assert ((m0 if p[0] == 'row_bin_tie' else m1)[:, p[1]] == p[2]).all()
        elif p[0] in ('row_bin', 'col_bin'):
            assert ((m0 if p[0] == 'row_bin' else m1)[:, p[1]] == -1).all()
        elif p[0] == 'thr_above':
            assert (t0[:, p[1]] == p[2]).all() and (t1[:, p[2]] == p[1]).all()
        elif p[0] == 'thr_below':
            assert (t0[:, p[1]] == -1).all() and (t1[:, p[2]] == -1).all()


@pytest.mark.parametrize('B,N,M', [(3, 20, 16), (2, 64, 64), (2, 130, 2048), (5, 600, 700)])
def test_extract_threshold_is_strict(B, N, M):
    """Z = 0 as a maximum: expf(0) == 1 is not above a threshold of 1.0 - and 1e-3 is."""
    Z, plants = planted_Z(B, N, M, seed=N + M, zero_maxima=True)
    zero = [p for p in plants if p[0] == 'zero'][0]
    above = [p for p in plants if p[0] == 'above1'][0]
    for mode in (2, 3):
        m0, m1, s0, s1 = ops.extract(Z.to(DEV), mode, 1.0)
        _note(check_extraction(Z, m0, m1, s0, s1, mode, 1.0))
        assert (m0[:, zero[1]] == -1).all() and (m1[:, zero[2]] == -1).all()
        assert (m0[:, above[1]] == above[2]).all() and int((m0 >= 0).sum()) == B
    for mode in range(4):
        _note(check_extraction(Z, *ops.extract(Z.to(DEV), mode, THR), mode, THR))


# ------------------------------------------------------------------------- the fused epilogue and the streaming kernel + scan
def _run_sk(s, bin_score, iters, streaming, modes=range(4), want_Z_false_too=True):
    """ops.sinkhorn_extract in every branch against the rules applied to the Z it returned; the same call without Z must give the
    same matches (the cluster kernel then stores no Z at all).  Returns the Z of the first mode."""
    d = s.to(DEV)
    Z0 = None
    for mode in modes:
        thr = 0.2
        if mode >= 2:
            thr = pick_threshold(Z0 if Z0 is not None else ops.sinkhorn_extract(d, bin_score, iters, mode=mode, want_Z=True, streaming=streaming)[4])
        m0, m1, s0, s1, Z = ops.sinkhorn_extract(d, bin_score, iters, mode=mode, match_threshold=thr, want_Z=True, streaming=streaming)
        Z = Z.cpu()
        assert torch.isfinite(Z).all()
        if Z0 is None:
            Z0 = Z
        assert torch.equal(Z, Z0)                                      # (what the threshold was taken from)
        _note(check_extraction(Z, m0, m1, s0, s1, mode, thr))
        if want_Z_false_too and not streaming:
            n0, n1, t0, t1 = ops.sinkhorn_extract(d, bin_score, iters, mode=mode, match_threshold=thr)
            assert torch.equal(n0, m0) and torch.equal(n1, m1) and torch.equal(t0, s0) and torch.equal(t1, s1)
    return Z0


@pytest.mark.parametrize('streaming', [False, True])
@pytest.mark.parametrize('B,N,M', SK_SHAPES)
def test_sinkhorn_extract_duplicated_rows_and_columns(B, N, M, streaming):
    """Builder A: two equal rows and two equal columns whose four crossing entries are the maxima.  The entries must come out
    bit-equal, and row ra and column ca - the first of the equal maxima - must win, across waves, lanes and slabs."""
    for variant in TIE_VARIANTS[:2]:
        s, (ra, rb, ca, cb) = scores_A(B, N, M, variant)
        Z = _run_sk(s, 1.0, SK_ITERS, streaming)
        for r in (ra, rb):
            for c in (ca, cb):
                assert torch.equal(Z[:, r, c], Z[:, ra, ca]), (variant, r, c)
        for mode in (0, 2):
            m0, m1, _, _ = ops.sinkhorn_extract(s.to(DEV), 1.0, SK_ITERS, mode=mode, match_threshold=1e-6, streaming=streaming)
            assert (m0[:, ra] == ca).all() and (m0[:, rb] == ca).all() and (m1[:, ca] == ra).all() and (m1[:, cb] == ra).all(), (variant, mode)


@pytest.mark.parametrize('streaming', [False, True])
@pytest.mark.parametrize('B,N,M', SK_SHAPES)
def test_sinkhorn_extract_constant_scores(B, N, M, streaming):
    """Builder B: every inner entry ties.  Index 0 wins on both sides in the superglue branches, and in the dustbin branches wherever the
    dustbin is smaller; with no iteration and bin score == score the dustbin ties as well and still loses; a large bin score wins."""
    for kind, (value, bin_score, iters) in CONST_KINDS.items():
        s = scores_B(B, N, M, value=value)
        iters = SK_ITERS if iters is None else iters
        Z = _run_sk(s, bin_score, iters, streaming, want_Z_false_too=(kind == 'inner'))
        for mode in range(3):
            m0, m1, _, _ = ops.sinkhorn_extract(s.to(DEV), bin_score, iters, mode=mode, match_threshold=1e-30, streaming=streaming)
            if mode == 2:
                assert (m0 == 0).all() and (m1 == 0).all(), kind
            elif kind == 'dustbin':
                assert (m0 == -1).all() and (m1 == -1).all()
            elif kind == 'inner':
                assert (m0 == 0).all() if N <= M else (m1 == 0).all()
        if kind == 'border' and (Z == Z[:, :1, :1]).all():              # (a form whose Z ties bit for bit: index 0, not the dustbin)
            m0, m1, _, _ = ops.sinkhorn_extract(s.to(DEV), bin_score, iters, mode=0, streaming=streaming)
            assert (m0 == 0).all() and (m1 == 0).all()


@pytest.mark.parametrize('streaming', [False, True])
@pytest.mark.parametrize('B,N,M', SK_SHAPES)
def test_sinkhorn_extract_natural_dustbin_share(B, N, M, streaming):
    """Builder C: normal scores and a bin score for which 10 % to 90 % of the shorter frame's keypoints prefer the dustbin, so that the
    compare with the dustbin column / row decides on natural data."""
    Z = _run_sk(scores_C(B, N, M), bin_score_C(N, M), SK_ITERS, streaming)
    assert 0.1 <= dustbin_share_C(Z.double()) <= 0.9


# ------------------------------------------------------------------------------------------------------------- redone pairs
@pytest.mark.parametrize('B,N,M,wide', [(5, 512, 512, (1,)), (9, 300, 400, (0, 7)), (3, 1024, 700, (2,)), (66, 512, 512, (13, 40))])
def test_sinkhorn_extract_redone_pairs(B, N, M, wide):
    """Pairs beyond the scaling form's range are redone by the streaming kernel; the extraction takes THEIR matches from a scan of
    that Z and the other pairs' from the fused bests - each against the Z the call returned.  Builder A's ties sit in a redone and in
    a kept pair of the same launch."""
    s = wide_range_scores(B, N, M, wide)
    ra, rb, ca, cb = 5, min(N - 2, 200), 3, M - 1
    kept = [b for b in range(B) if b not in wide][0]
    for b in (wide[0], kept):
        scale = 14 if b in wide else 1
        s[b, ra, :] -= 12.0 * scale                                     # (no other row or column has ITS maximum in the planted ones:
        s[b, :, ca] -= 12.0 * scale                                     # a wide pair's rows put nearly all their mass on one entry)
        s[b, rb, :] = s[b, ra, :]
        s[b, :, cb] = s[b, :, ca]
        top = float(s[b].max()) + 8.0 * scale
        for r in (ra, rb):
            for c in (ca, cb):
                s[b, r, c] = top
    Z = _run_sk(s, 0.8, SK_ITERS, False)
    Zs = ops.sinkhorn(s.to(DEV), 0.8, SK_ITERS, streaming=True).cpu()
    for b in range(B):
        assert torch.equal(Z[b], Zs[b]) == (b in wide), b              # redone pairs carry the streaming kernel's Z, the others do not
    for b in (wide[0], kept):
        for r in (ra, rb):
            for c in (ca, cb):
                assert Z[b, r, c] == Z[b, ra, ca]
    m0, m1, _, _ = ops.sinkhorn_extract(s.to(DEV), 0.8, SK_ITERS)
    for b in (wide[0], kept):
        assert int(m0[b, ra]) == ca and int(m0[b, rb]) == ca and int(m1[b, ca]) == ra and int(m1[b, cb]) == ra


@pytest.mark.parametrize('B,N,M', [(3, 512, 512), (70, 300, 512), (2, 1024, 700), (1, 2048, 2048)])
def test_sinkhorn_extract_after_a_lost_partner(B, N, M, monkeypatch):
    """MDGAT_SK_FORCE_FALLBACK=1: the whole launch is redone and every pair's matches come from the scan of the streaming kernel's Z."""
    s, (ra, rb, ca, cb) = scores_A(B, N, M, 'slabs')
    Zs = ops.sinkhorn(s.to(DEV), 1.0, SK_ITERS, streaming=True).cpu()
    monkeypatch.setenv('MDGAT_SK_FORCE_FALLBACK', '1')
    try:
        Z = _run_sk(s, 1.0, SK_ITERS, False)
        m0, m1, _, _ = ops.sinkhorn_extract(s.to(DEV), 1.0, SK_ITERS)
        torch.cuda.synchronize()
    finally:
        monkeypatch.delenv('MDGAT_SK_FORCE_FALLBACK')
    assert torch.equal(Z, Zs)
    assert (m0[:, ra] == ca).all() and (m0[:, rb] == ca).all() and (m1[:, ca] == ra).all() and (m1[:, cb] == ra).all()


# --------------------------------------------------------------------------------------------------------- all-dustbin rule
def _alldust_cases(B):
    return [('none', 0), ('all', 0)] + [('one', w) for w in sorted({0, B // 2, B - 1})]


@pytest.mark.parametrize('B', [1, 3, 70])
def test_alldust_rule_extract(B):
    """mdgat.py:465-467 through ops.extract: no pair matches -> every score zero; exactly one pair - first, middle, last - matches one
    row -> the scores of ALL pairs stay; all match."""
    for kind, which in _alldust_cases(B):
        Z = alldust_Z(B, kind, which)
        for mode in (0, 1):
            m0, m1, s0, s1 = ops.extract(Z.to(DEV), mode, 0.2)
            _note(check_extraction(Z, m0, m1, s0, s1, mode, 0.2))
            assert ((s0 == 0).all() and (s1 == 0).all()) == (kind == 'none'), (kind, which, mode)
            if kind == 'one':
                assert int((m0 >= 0).sum()) == 1 and int(m0[which, 11]) == 5
                if mode == 0:
                    assert all((s1[b] > 0).any() for b in range(B))


@pytest.mark.parametrize('streaming', [False, True])
@pytest.mark.parametrize('B', [1, 3, 70])
def test_alldust_rule_sinkhorn_extract(B, streaming):
    """The same through ops.sinkhorn_extract: the cluster path applies the rule with a ticket word inside extract_kernel - the last
    workgroup to finish zeroes the scores only if NO workgroup before it matched anything."""
    N, M = ALLDUST_SHAPE
    for kind, which in _alldust_cases(B):
        s, bin_score = alldust_scores(B, kind, which)
        for mode in (0, 1):
            m0, m1, s0, s1, Z = ops.sinkhorn_extract(s.to(DEV), bin_score, SK_ITERS, mode=mode, want_Z=True, streaming=streaming)
            _note(check_extraction(Z, m0, m1, s0, s1, mode, 0.2))
            assert ((s0 == 0).all() and (s1 == 0).all()) == (kind == 'none'), (kind, which, mode)
            assert (m1 >= 0).any()
            if kind == 'none':
                assert (m0 == -1).all()
            if kind == 'one':
                assert int((m0 >= 0).sum()) == 1 and int(m0[which, 11]) == 5
                if mode == 0:
                    assert all((s1[b] > 0).any() for b in range(B))


SPARSE_BIN_SCORE = 20.0      # (measured: 0.5 % of the keypoints match, in 121 of the 130 pairs)


@pytest.mark.parametrize('mode', ['dustbin', 'dustbin_mutual'])
def test_alldust_rule_deferred_in_a_sliced_batch(mode):
    """130 pairs of 512 run as slices, the rule applied by extract_alldust_fixup after the last one.  With a bin score for which fewer
    than 1 % of the keypoints match - and more than none - the matches are few and far between, and no score may be zeroed."""
    B, n = 130, 512
    cfg = synth.default_config(L=2, k=[128, None, 64, None], sinkhorn_iterations=10)
    cfg.update({'dustbin': {}, 'dustbin_mutual': {'mutual_check': True}}[mode])
    net = MDGAT({**cfg, 'arithmetic': 'fp32'}).double()            # the fp32-class path: fused arg-maxes, the rule deferred to the fix-up
    net.load_state_dict(synth.make_state_dict(L=2, seed=5, bin_score=SPARSE_BIN_SCORE))
    net = net.to(DEV).eval()
    data = synth.make_batch(B, n, n, device=DEV)
    with torch.no_grad():
        m0, m1, s0, s1, Z = net.match(data['keypoints0'], data['descriptors0'], data['keypoints1'], data['descriptors1'],
                                      data['scores0'], data['scores1'], return_scores=True)
    torch.cuda.synchronize()
    share = (m0 >= 0).double().mean().item()
    print(f'matched share {share:.5f}, pairs with a match {int((m0 >= 0).any(1).sum())} of {B}')
    assert 0 < share < 0.01
    _note(check_extraction(Z, m0, m1, s0, s1, 1 if mode == 'dustbin_mutual' else 0, 0.2))
    assert (s0 > 0).any()


# -------------------------------------------------------------------------------------------------------------- fp64 kernels
def _run_f64(s, bin_score, iters, planted=None):
    """ops.sinkhorn_f64_extract in every branch against the rules applied to the ORACLE's fp64 Z.  No row or column is left out: the
    two best candidates of each are equal (planted) or more than 1e-9 apart (tests/test_extract_ref.py, for these very inputs)."""
    Zr = O.log_optimal_transport(s, torch.tensor(float(bin_score), dtype=torch.float64), iters)
    thr = pick_threshold(Zr)
    d = s.to(DEV)
    for mode in range(4):
        assert ambiguous(Zr, mode) == 0
        m0, m1, s0, s1 = ops.sinkhorn_f64_extract(d, bin_score, iters, mode=mode, match_threshold=thr)
        _note(check_extraction(Zr, m0, m1, s0, s1, mode, thr))
    if planted:
        ra, rb, ca, cb = planted
        Z = ops.sinkhorn_f64(d, bin_score, iters).cpu()
        assert (Z - Zr).abs().max().item() < 1e-12
        for r in (ra, rb):
            for c in (ca, cb):
                assert torch.equal(Z[:, r, c], Z[:, ra, ca]), (r, c)       # a planted tie ties in the kernel as well
    return Zr


@pytest.mark.parametrize('B,N,M,iters,form', F64_CASES)
def test_sinkhorn_f64_extract_planted(B, N, M, iters, form):
    """Builders A (rows in other waves, in other slabs, and - for the streaming form, whose rows interleave over the waves - the smaller
    row in the higher wave), B and C through the resident and the streaming fp64 Sinkhorn."""
    lib = _lib.load()
    prev = lib.mdgat_set_f64_sinkhorn_form(form)
    try:
        for variant in TIE_VARIANTS:
            s, pos = scores_A(B, N, M, variant, dtype=torch.float64)
            _run_f64(s, 1.0, iters, planted=pos)
            ra, rb, ca, cb = pos
            for mode in (0, 2):
                m0, m1, _, _ = ops.sinkhorn_f64_extract(s.to(DEV), 1.0, iters, mode=mode, match_threshold=1e-6)
                assert (m0[:, ra] == ca).all() and (m0[:, rb] == ca).all() and (m1[:, ca] == ra).all() and (m1[:, cb] == ra).all(), (variant, mode)
        Zr = _run_f64(scores_C(B, N, M, dtype=torch.float64), bin_score_C(N, M), iters)
        assert 0.1 <= dustbin_share_C(Zr) <= 0.9
        for kind, (value, bin_score, it) in CONST_KINDS.items():
            s = scores_B(B, N, M, torch.float64, value)
            it = iters if it is None else it
            for mode in range(3):
                m0, m1, s0, s1 = ops.sinkhorn_f64_extract(s.to(DEV), bin_score, it, mode=mode, match_threshold=1e-30)
                Z = ops.sinkhorn_f64(s.to(DEV), bin_score, it).cpu()
                _note(check_extraction(Z, m0, m1, s0, s1, mode, 1e-30))       # (everything ties: the kernel's own fp64 Z)
                if mode == 2 or kind == 'border':
                    assert (m0 == 0).all() and (m1 == 0).all(), (kind, mode)
                elif kind == 'dustbin':
                    assert (m0 == -1).all() and (m1 == -1).all()
    finally:
        lib.mdgat_set_f64_sinkhorn_form(prev)


def test_report_largest_score_error():
    print(f'largest matching-score error seen in this file: {WORST["score"]:.3e} (bound {SCORE_TOL:.0e})')
    assert WORST['score'] <= SCORE_TOL
