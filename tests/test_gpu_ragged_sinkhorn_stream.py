"""Ragged batches through the STREAMING form of the fp64 Sinkhorn and its match extraction (ops.sinkhorn_f64 / sinkhorn_f64_extract with
counts= and form='streaming'): pairs of different sizes in padded slots of up to 2175 keypoints.  The yardstick is the pair run ALONE
through the same ops under mdgat_set_f64_sinkhorn_form(1) - the uniform streaming form - bit for bit."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sinkhorn_f64_forms as F  # noqa: E402
from mdgat_matcher_amd import _lib, ops  # noqa: E402
from oracle import mdgat_oracle as O  # noqa: E402

DEV = 'cuda:0'
# S: counts on both sides of the 32-row slabs and of the 128-column chunk edge (m + 1 = 128 against 129), in slots of 130 x 128 where most
# pairs leave slabs and chunks empty
SET_S = ((40, 33), (33, 127), (32, 128), (65, 48), (8, 8), (1, 1), (1, 5), (130, 3))
# T: the slot picks the 17-chunk instantiation while three of the pairs alone pick the 5-chunk one; 1100 rows are 35 slabs
SET_T = ((40, 1200), (1100, 40), (40, 33), (64, 64))
# U: the limits - 68 slabs, 17 chunks
SET_U = ((2175, 8), (8, 2175), (16, 16))
SETS = {'S': (SET_S, 20, 0.7), 'S0': (SET_S, 0, 0.7), 'T': (SET_T, 3, 1.0), 'U': (SET_U, 2, 1.0)}      # counts, iterations, bin score
THR = 0.01
STREAM = dict(form='streaming')


def _scores(counts, fill=0.0, seed=5):
    """[B, Np, Mp] random scores, `fill` beyond every pair's counts; pair 1 is pushed far below the bin score, so that it matches nothing
    next to pairs that do (the construction of tests/test_gpu_ragged_sinkhorn.py)."""
    Np, Mp = max(n for n, _ in counts), max(m for _, m in counts)
    rs = np.random.RandomState(seed)
    s = np.full((len(counts), Np, Mp), fill)
    for b, (n, m) in enumerate(counts):
        s[b, :n, :m] = rs.standard_normal((n, m)) * 3.0 - (40.0 if b == 1 and len(counts) > 2 else 0.0)
    return torch.from_numpy(s)


class _form1:
    """the uniform entries on the streaming form"""
    def __enter__(self):
        self.prev = _lib.load().mdgat_set_f64_sinkhorn_form(1)

    def __exit__(self, *exc):
        _lib.load().mdgat_set_f64_sinkhorn_form(self.prev)


@functools.lru_cache(maxsize=None)
def _alone(name):
    """every pair of the set run alone under form 1: Z (fp64) and, per extraction mode, (m0, m1, s0, s1, Z32) - computed once, never modified"""
    counts, iters, alpha = SETS[name]
    s = _scores(counts)
    out = []
    with _form1():
        for b, (n, m) in enumerate(counts):
            sb = s[b:b + 1, :n, :m].contiguous().to(DEV)
            Z = ops.sinkhorn_f64(sb, alpha, iters)
            ex = [ops.sinkhorn_f64_extract(sb, alpha, iters, mode=mode, match_threshold=THR, want_Z=True) for mode in range(4)]
            out.append((Z, ex))
    return s, out


def _check_against_alone(name, s):
    counts, iters, alpha = SETS[name]
    _, alone = _alone(name)
    cnt = ([n for n, _ in counts], [m for _, m in counts])
    sd = s.to(DEV)
    with F.watch() as w:
        Z = ops.sinkhorn_f64(sd, alpha, iters, counts=cnt, **STREAM)
    # the instantiation follows the slot (tests/sinkhorn_f64_forms.py: S <5, true>, T and U <17, true>)
    assert w.ran() == {F.STREAM_SETS_ELSEWHERE[name][1]: 1}, (name, w.ran())
    for b, (n, m) in enumerate(counts):
        assert torch.equal(Z[b, :n + 1, :m + 1], alone[b][0][0]), (name, b)
        rest = Z[b].clone()
        rest[:n + 1, :m + 1] = 0
        assert not rest.any(), (name, b)
    for mode in range(4):
        m0, m1, s0, s1, Z32 = ops.sinkhorn_f64_extract(sd, alpha, iters, mode=mode, match_threshold=THR, want_Z=True, counts=cnt, **STREAM)
        for b, (n, m) in enumerate(counts):
            a0, a1, as0, as1, aZ = alone[b][1][mode]
            assert torch.equal(m0[b, :n], a0[0]) and torch.equal(m1[b, :m], a1[0]), (name, mode, b)
            assert torch.equal(s0[b, :n], as0[0]) and torch.equal(s1[b, :m], as1[0]), (name, mode, b)
            assert (m0[b, n:] == -1).all() and (m1[b, m:] == -1).all() and not s0[b, n:].any() and not s1[b, m:].any(), (name, mode, b)
            assert torch.equal(Z32[b, :n + 1, :m + 1], aZ[0]), (name, mode, b)
            rest = Z32[b].clone()
            rest[:n + 1, :m + 1] = 0
            assert not rest.any(), (name, mode, b)
    return Z


@pytest.mark.parametrize('name', ['S', 'S0', 'T', 'U'])
def test_stream_ragged_sinkhorn_equals_every_pair_alone_under_form_1(name):
    """Z[b, :N_b+1, :M_b+1], Z32, the matches and the scores of all four extraction modes: the bits of the pair run alone through the
    uniform streaming form; the rest of every slot fixed (Z 0, matches -1, scores 0)."""
    s, _ = _alone(name)
    _check_against_alone(name, s)


@pytest.mark.parametrize('name', ['S', 'T'])
def test_stream_ragged_sinkhorn_against_the_oracle(name):
    """Z within 1e-12 of the oracle's log_optimal_transport: the bound tests/test_gpu_f64.py holds the uniform streaming form to."""
    counts, iters, alpha = SETS[name]
    s, _ = _alone(name)
    Z = ops.sinkhorn_f64(s.to(DEV), alpha, iters, counts=([n for n, _ in counts], [m for _, m in counts]), **STREAM).cpu()
    for b, (n, m) in enumerate(counts):
        Zr = O.log_optimal_transport(s[b:b + 1, :n, :m], torch.tensor(alpha, dtype=torch.float64), iters)
        err = (Z[b:b + 1, :n + 1, :m + 1] - Zr).abs().max().item()
        print(f'{name} pair {b} ({n} x {m}): max|Z - oracle| = {err:.3e}')
        assert err < 1e-12, (name, b, err)


@pytest.mark.parametrize('poison', [float('nan'), float('inf'), 1e300])
def test_stream_ragged_sinkhorn_never_reads_beyond_a_pairs_counts(poison):
    counts, _, _ = SETS['S']
    _check_against_alone('S', _scores(counts, fill=poison))


def test_stream_ragged_sinkhorn_applies_the_nothing_matched_rule_per_pair():
    """Pair 1 of set S sits 40 below the bin score: nothing of it is matched and ALL its scores are zero (mdgat.py:465-467, as when it is
    the only pair of a call), while its neighbours in the launch keep theirs."""
    counts, iters, alpha = SETS['S']
    s, _ = _alone('S')
    for mode in (_lib.EXTRACT_DUSTBIN, _lib.EXTRACT_DUSTBIN_MUTUAL):
        m0, m1, s0, s1 = ops.sinkhorn_f64_extract(s.to(DEV), alpha, iters, mode=mode, counts=([n for n, _ in counts], [m for _, m in counts]), **STREAM)
        assert (m0[1] == -1).all() and not s0[1].any() and not s1[1].any()
        assert (m0[0] >= 0).any() and s1[0].any() and (m0[3] >= 0).any() and s1[3].any()


def test_stream_ragged_sinkhorn_order_and_packed_counts():
    """Permuting the pairs permutes the results (every pair still equals itself alone); a pack_ragged-style dict serves as counts."""
    counts, iters, alpha = SETS['S']
    s, alone = _alone('S')
    perm = [4, 2, 6, 0, 7, 5, 1, 3]
    h0 = torch.tensor([counts[p][0] for p in perm], dtype=torch.int32)
    h1 = torch.tensor([counts[p][1] for p in perm], dtype=torch.int32)
    packed = {'counts0': h0.to(DEV), 'counts1': h1.to(DEV), 'counts0_host': h0, 'counts1_host': h1}
    Z = ops.sinkhorn_f64(s[perm].to(DEV), alpha, iters, counts=packed, **STREAM)
    m0, m1 = ops.sinkhorn_f64_extract(s[perm].to(DEV), alpha, iters, counts=packed, **STREAM)[:2]
    for i, p in enumerate(perm):
        n, m = counts[p]
        assert torch.equal(Z[i, :n + 1, :m + 1], alone[p][0][0]), p
        assert torch.equal(m0[i, :n], alone[p][1][0][0][0]) and torch.equal(m1[i, :m], alone[p][1][0][1][0]), p


@pytest.mark.parametrize('B,N,M,iters', [(3, 65, 48, 20), (2, 130, 200, 3), (9, 64, 64, 0), (1, 600, 40, 2)])
def test_stream_ragged_sinkhorn_with_uniform_counts_equals_the_uniform_entry_under_form_1(B, N, M, iters):
    s = torch.from_numpy(np.random.RandomState(N + M).standard_normal((B, N, M)) * 3.0).to(DEV)
    cnt = ([N] * B, [M] * B)
    with _form1():
        refZ = ops.sinkhorn_f64(s, 0.5, iters)
        refs = [ops.sinkhorn_f64_extract(s, 0.5, iters, mode=mode, match_threshold=THR, want_Z=True) for mode in range(4)]
    assert torch.equal(ops.sinkhorn_f64(s, 0.5, iters, counts=cnt, **STREAM), refZ)
    for mode in range(4):
        got = ops.sinkhorn_f64_extract(s, 0.5, iters, mode=mode, match_threshold=THR, want_Z=True, counts=cnt, **STREAM)
        assert all(torch.equal(a, b) for a, b in zip(got, refs[mode])), mode


def test_stream_ragged_sinkhorn_refusals():
    """Checked on the host before anything is launched: the slot limit of 2175, then the counts, naming the first offending pair."""
    s = torch.zeros(3, 16, 16, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match='pair 1'):
        ops.sinkhorn_f64(s, 1.0, 2, counts=([16, 0, 0], [16, 16, 16]), **STREAM)
    with pytest.raises(RuntimeError, match='pair 2'):
        ops.sinkhorn_f64_extract(s, 1.0, 2, counts=([16, 16, 16], [16, 16, 17]), **STREAM)
    with pytest.raises(RuntimeError, match='padded sizes 8 x 2176: the streaming form holds at most 2175'):
        ops.sinkhorn_f64(torch.zeros(1, 8, 2176, dtype=torch.float64, device=DEV), 1.0, 2, counts=([8], [8]), **STREAM)
    with pytest.raises(RuntimeError, match='padded sizes 2176 x 8: the streaming form holds at most 2175'):
        ops.sinkhorn_f64_extract(torch.zeros(1, 2176, 8, dtype=torch.float64, device=DEV), 1.0, 2, counts=([8], [8]), **STREAM)
    with pytest.raises(ValueError, match='3 entries'):
        ops.sinkhorn_f64(s, 1.0, 2, counts=([16, 16], [16, 16]), **STREAM)
    with pytest.raises(RuntimeError, match='forward only'):
        ops.sinkhorn_f64(s.clone().requires_grad_(), 1.0, 2, counts=([16] * 3, [16] * 3), **STREAM)
    with pytest.raises(RuntimeError, match='forward only'):
        ops.sinkhorn_f64_extract(s.clone().requires_grad_(), 1.0, 2, counts=([16] * 3, [16] * 3), **STREAM)
    with pytest.raises(ValueError, match='needs counts'):
        ops.sinkhorn_f64(s, 1.0, 2, **STREAM)
    with pytest.raises(ValueError, match="expected None or 'streaming'"):
        ops.sinkhorn_f64(s, 1.0, 2, counts=([16] * 3, [16] * 3), form='resident')
