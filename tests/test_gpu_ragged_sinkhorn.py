"""Ragged batches through the fp64 Sinkhorn and its match extraction (ops.sinkhorn_f64 / sinkhorn_f64_extract with counts=): pairs of
different sizes in padded slots of one launch.  The yardstick is the pair run ALONE through the same ops: bit for bit."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mdgat_matcher_amd import _lib, ops  # noqa: E402
from oracle import mdgat_oracle as O  # noqa: E402

DEV = 'cuda:0'
# counts that straddle the kernel's tiling: 32-row slabs (Np = 65: three slabs, pairs of at most 32 rows leave two of them empty), 64-column lanes
SET_A = ((40, 33), (17, 64), (64, 17), (65, 48), (8, 8), (31, 32), (33, 97))
SET_B = ((530, 100), (100, 540), (575, 575), (64, 64))          # the register-resident form's limit
SET_C = ((1, 1), (1, 5), (5, 1), (16, 16), (3, 70))
SETS = {'A': (SET_A, 20, 0.7), 'B': (SET_B, 10, 1.0), 'C': (SET_C, 20, 0.4), 'A0': (SET_A, 0, 0.7)}      # counts, iterations, bin score
THR = 0.01


def _scores(counts, fill=0.0, seed=5):
    """[B, Np, Mp] random scores, `fill` beyond every pair's counts; pair 1 of sets with more than two pairs is pushed far below the bin
    score, so that it matches nothing next to pairs that do."""
    Np, Mp = max(n for n, _ in counts), max(m for _, m in counts)
    rs = np.random.RandomState(seed)
    s = np.full((len(counts), Np, Mp), fill)
    for b, (n, m) in enumerate(counts):
        s[b, :n, :m] = rs.standard_normal((n, m)) * 3.0 - (40.0 if b == 1 and len(counts) > 2 else 0.0)
    return torch.from_numpy(s)


@functools.lru_cache(maxsize=None)
def _alone(name):
    """every pair of the set run alone: Z (fp64) and, per extraction mode, (m0, m1, s0, s1, Z32) - computed once, never modified"""
    counts, iters, alpha = SETS[name]
    s = _scores(counts)
    out = []
    for b, (n, m) in enumerate(counts):
        sb = s[b:b + 1, :n, :m].contiguous().to(DEV)
        Z = ops.sinkhorn_f64(sb, alpha, iters)
        ex = [ops.sinkhorn_f64_extract(sb, alpha, iters, mode=mode, match_threshold=THR, want_Z=True) for mode in range(4)]
        out.append((Z, ex))
    return s, out


def _check_against_alone(name, s, counts_arg=None):
    counts, iters, alpha = SETS[name]
    _, alone = _alone(name)
    cnt = counts_arg if counts_arg is not None else ([n for n, _ in counts], [m for _, m in counts])
    Z = ops.sinkhorn_f64(s.to(DEV), alpha, iters, counts=cnt)
    for b, (n, m) in enumerate(counts):
        assert torch.equal(Z[b, :n + 1, :m + 1], alone[b][0][0]), (name, b)
        rest = Z[b].clone()
        rest[:n + 1, :m + 1] = 0
        assert not rest.any(), (name, b)
    for mode in range(4):
        m0, m1, s0, s1, Z32 = ops.sinkhorn_f64_extract(s.to(DEV), alpha, iters, mode=mode, match_threshold=THR, want_Z=True, counts=cnt)
        for b, (n, m) in enumerate(counts):
            a0, a1, as0, as1, aZ = alone[b][1][mode]
            assert torch.equal(m0[b, :n], a0[0]) and torch.equal(m1[b, :m], a1[0]), (name, mode, b)
            assert torch.equal(s0[b, :n], as0[0]) and torch.equal(s1[b, :m], as1[0]), (name, mode, b)
            assert (m0[b, n:] == -1).all() and (m1[b, m:] == -1).all() and not s0[b, n:].any() and not s1[b, m:].any(), (name, mode, b)
            assert torch.equal(Z32[b, :n + 1, :m + 1], aZ[0]), (name, mode, b)
    return Z


@pytest.mark.parametrize('name', ['A', 'B', 'C', 'A0'])
def test_ragged_sinkhorn_equals_every_pair_alone_and_the_oracle(name):
    """Z[b, :N_b+1, :M_b+1], the matches and the scores of all four extraction modes: the bits of the pair run alone; the rest of every
    slot fixed (Z 0, matches -1, scores 0); Z within 1e-12 of the oracle's log_optimal_transport (the bound of tests/test_gpu_f64.py)."""
    counts, iters, alpha = SETS[name]
    s, _ = _alone(name)
    Z = _check_against_alone(name, s).cpu()
    for b, (n, m) in enumerate(counts):
        Zr = O.log_optimal_transport(s[b:b + 1, :n, :m], torch.tensor(alpha, dtype=torch.float64), iters)
        assert (Z[b:b + 1, :n + 1, :m + 1] - Zr).abs().max().item() < 1e-12, (name, b)


def test_ragged_sinkhorn_applies_the_nothing_matched_rule_per_pair():
    """Pair 1 of set A sits 40 below the bin score: nothing of it is matched and ALL its scores are zero (mdgat.py:465-467, as when it is
    the only pair of a call), while its neighbours in the launch keep theirs."""
    counts, iters, alpha = SETS['A']
    s, _ = _alone('A')
    for mode in (_lib.EXTRACT_DUSTBIN, _lib.EXTRACT_DUSTBIN_MUTUAL):
        m0, m1, s0, s1 = ops.sinkhorn_f64_extract(s.to(DEV), alpha, iters, mode=mode, counts=([n for n, _ in counts], [m for _, m in counts]))
        assert (m0[1] == -1).all() and not s0[1].any() and not s1[1].any()
        assert (m0[0] >= 0).any() and s1[0].any() and (m0[3] >= 0).any() and s1[3].any()


@pytest.mark.parametrize('poison', [float('nan'), float('inf'), 1e300])
def test_ragged_sinkhorn_never_reads_beyond_a_pairs_counts(poison):
    counts, _, _ = SETS['A']
    _check_against_alone('A', _scores(counts, fill=poison))


def test_ragged_sinkhorn_order_and_packed_counts():
    """Permuting the pairs permutes the results (every pair still equals itself alone); a pack_ragged-style dict serves as counts."""
    counts, iters, alpha = SETS['A']
    s, alone = _alone('A')
    perm = [4, 2, 6, 0, 5, 1, 3]
    h0 = torch.tensor([counts[p][0] for p in perm], dtype=torch.int32)
    h1 = torch.tensor([counts[p][1] for p in perm], dtype=torch.int32)
    packed = {'counts0': h0.to(DEV), 'counts1': h1.to(DEV), 'counts0_host': h0, 'counts1_host': h1}
    Z = ops.sinkhorn_f64(s[perm].to(DEV), alpha, iters, counts=packed)
    m0 = ops.sinkhorn_f64_extract(s[perm].to(DEV), alpha, iters, counts=packed)[0]
    for i, p in enumerate(perm):
        n, m = counts[p]
        assert torch.equal(Z[i, :n + 1, :m + 1], alone[p][0][0]) and torch.equal(m0[i, :n], alone[p][1][0][0][0])


@pytest.mark.parametrize('B,N,M,iters', [(3, 65, 48, 20), (2, 575, 575, 5), (9, 64, 64, 0)])
def test_ragged_sinkhorn_with_uniform_counts_equals_the_uniform_entry(B, N, M, iters):
    s = torch.from_numpy(np.random.RandomState(N + M).standard_normal((B, N, M)) * 3.0).to(DEV)
    cnt = ([N] * B, [M] * B)
    assert torch.equal(ops.sinkhorn_f64(s, 0.5, iters, counts=cnt), ops.sinkhorn_f64(s, 0.5, iters))
    for mode in range(4):
        got = ops.sinkhorn_f64_extract(s, 0.5, iters, mode=mode, match_threshold=THR, want_Z=True, counts=cnt)
        ref = ops.sinkhorn_f64_extract(s, 0.5, iters, mode=mode, match_threshold=THR, want_Z=True)
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), mode


def test_ragged_sinkhorn_refusals():
    """Checked on the host copies before anything is launched, naming the first offending pair."""
    s = torch.zeros(3, 16, 16, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match='pair 1'):
        ops.sinkhorn_f64(s, 1.0, 2, counts=([16, 0, 0], [16, 16, 16]))
    with pytest.raises(RuntimeError, match='pair 2'):
        ops.sinkhorn_f64_extract(s, 1.0, 2, counts=([16, 16, 16], [16, 16, 17]))
    with pytest.raises(RuntimeError, match='575'):
        ops.sinkhorn_f64(torch.zeros(1, 8, 576, dtype=torch.float64, device=DEV), 1.0, 2, counts=([8], [8]))
    with pytest.raises(RuntimeError, match='575'):          # (one limit for both frames, although the kernel holds 576 rows)
        ops.sinkhorn_f64_extract(torch.zeros(1, 576, 8, dtype=torch.float64, device=DEV), 1.0, 2, counts=([8], [8]))
    with pytest.raises(ValueError, match='3 entries'):
        ops.sinkhorn_f64(s, 1.0, 2, counts=([16, 16], [16, 16]))
    with pytest.raises(RuntimeError, match='forward only'):
        ops.sinkhorn_f64(s.clone().requires_grad_(), 1.0, 2, counts=([16] * 3, [16] * 3))
    lib = _lib.load()
    prev = lib.mdgat_set_f64_sinkhorn_form(1)
    try:
        with pytest.raises(RuntimeError, match='streaming'):
            ops.sinkhorn_f64(s, 1.0, 2, counts=([16] * 3, [16] * 3))
    finally:
        lib.mdgat_set_f64_sinkhorn_form(prev)
