"""Ragged batches through the fp32 streaming Sinkhorn and its match extraction (ops.sinkhorn / ops.sinkhorn_extract with counts=): pairs of
different sizes in padded slots of one launch, in slots that select each of the kernel's four column widths (64: NC = 1, 256: NC = 4,
512: NC = 8; set A's 65 x 97: NC = 2).  The yardstick is the pair run ALONE through the streaming kernel (streaming=True) - which picks
its width from the pair's own M - bit for bit, and the oracle within the bound of test_gpu_ops.py::test_sinkhorn_vs_oracle.  The scores
beyond every pair's counts are NaN."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sinkhorn_forms as SF  # noqa: E402
from mdgat_matcher_amd import _lib, ops  # noqa: E402
from oracle import mdgat_oracle as O  # noqa: E402

DEV = 'cuda:0'
Z_ORACLE_TOL = 1e-4     # test_gpu_ops.py::test_sinkhorn_vs_oracle
THR = 0.01
# name -> (counts, iterations, bin score, scale and offset of the random scores)
SETS = {
    's64': (((40, 33), (17, 64), (64, 17), (1, 1), (1, 5), (5, 1)), 20, 0.7, 4.0, 0.0),
    's256': (((200, 130), (130, 256), (65, 48)), 20, 0.7, 4.0, 0.0),
    's512': (((300, 500), (512, 512), (64, 64)), 100, 0.7, 4.0, 0.0),
    # set A of the exact mode's tests under a bin score of 32: with these scores the oracle leaves the 8 x 8 pair - and no other - without a match
    'A32': (((40, 33), (17, 64), (64, 17), (65, 48), (8, 8), (31, 32), (33, 97)), 20, 32.0, 3.0, 27.0),
}
UNMATCHED = {'A32': 4}
# the RAGGED instantiation each set's slots select (from the padded M alone): one of the four per set
RAGGED_FORM = {'s64': 'stream<1,16>,RAGGED', 'A32': 'stream<2,16>,RAGGED', 's256': 'stream<4,16>,RAGGED', 's512': 'stream<8,16>,RAGGED'}


def _cnt(counts):
    return [n for n, _ in counts], [m for _, m in counts]


def _scores(name, order=None, fill=float('nan')):
    """[B, Np, Mp] float64 scores, `fill` beyond every pair's counts; a pair's scores follow from its own sizes alone, wherever it stands"""
    counts, _, _, scale, offset = SETS[name]
    Np, Mp = max(n for n, _ in counts), max(m for _, m in counts)
    order = range(len(counts)) if order is None else order
    s = np.full((len(order), Np, Mp), fill)
    for i, b in enumerate(order):
        n, m = counts[b]
        s[i, :n, :m] = np.random.RandomState(5 + 1000 * n + m).standard_normal((n, m)) * scale + offset
    return torch.from_numpy(s)


@functools.lru_cache(maxsize=None)
def _alone(name):
    """every pair of the set run alone through the streaming kernel: Z and, per extraction mode, (m0, m1, s0, s1, Z) - computed once, never
    modified"""
    counts, iters, alpha, _, _ = SETS[name]
    s = _scores(name)
    out = []
    for b, (n, m) in enumerate(counts):
        sb = s[b:b + 1, :n, :m].contiguous().to(DEV)
        Z = ops.sinkhorn(sb, alpha, iters, streaming=True)
        ex = [ops.sinkhorn_extract(sb, alpha, iters, mode=mode, match_threshold=THR, want_Z=True, streaming=True) for mode in range(4)]
        out.append((Z, ex))
    return s, out


@pytest.mark.parametrize('name', list(SETS))
def test_ragged_sinkhorn_equals_every_pair_alone_and_the_oracle(name):
    """Z[b, :N_b+1, :M_b+1]: the bits of the pair alone, whatever column width the slot selects; the rest of the slot 0; the oracle's
    log_optimal_transport within 1e-4."""
    counts, iters, alpha, _, _ = SETS[name]
    s, alone = _alone(name)
    p = SF.plan(len(counts), s.shape[1], s.shape[2], ragged=True)
    assert p.path == SF.STREAMING and p.stream == RAGGED_FORM[name] and sorted(RAGGED_FORM.values()) == sorted(SF.RAGGED)
    with SF.watch() as w:
        Z = ops.sinkhorn(s.to(DEV), alpha, iters, counts=_cnt(counts))
    SF.assert_launched(w, p, name)
    for b, (n, m) in enumerate(counts):
        assert torch.equal(Z[b, :n + 1, :m + 1], alone[b][0][0]), (name, b)
        rest = Z[b].clone()
        rest[:n + 1, :m + 1] = 0
        assert not rest.any(), (name, b)
        Zr = O.log_optimal_transport(s[b:b + 1, :n, :m], torch.tensor(alpha, dtype=torch.float64), iters)
        err = (Z[b:b + 1, :n + 1, :m + 1].cpu().double() - Zr).abs().max().item()
        print(f'{name} pair {b} ({n} x {m}): max |Z - oracle| = {err:.3e}')
        assert err < Z_ORACLE_TOL, (name, b, err)


@pytest.mark.parametrize('name', list(SETS))
def test_ragged_extraction_equals_every_pair_alone(name):
    """All four extraction modes: matches, scores and Z are the bits of the pair alone (streaming=True), with the nothing-matched rule of
    mdgat.py:465-467 applied per pair; beyond the counts matches are -1 and scores 0."""
    counts, iters, alpha, _, _ = SETS[name]
    s, alone = _alone(name)
    for mode in range(4):
        for want_Z in (True, False):
            with SF.watch() as w:
                got = ops.sinkhorn_extract(s.to(DEV), alpha, iters, mode=mode, match_threshold=THR, want_Z=want_Z, counts=_cnt(counts))
            SF.assert_launched(w, {RAGGED_FORM[name]: 1, SF.EXTRACT: 1}, (name, mode, want_Z))
            m0, m1, s0, s1 = got[:4]
            for b, (n, m) in enumerate(counts):
                a0, a1, as0, as1, aZ = alone[b][1][mode]
                assert torch.equal(m0[b, :n], a0[0]) and torch.equal(m1[b, :m], a1[0]), (name, mode, b)
                assert torch.equal(s0[b, :n], as0[0]) and torch.equal(s1[b, :m], as1[0]), (name, mode, b)
                assert (m0[b, n:] == -1).all() and (m1[b, m:] == -1).all() and not s0[b, n:].any() and not s1[b, m:].any(), (name, mode, b)
                if want_Z:
                    assert torch.equal(got[4][b, :n + 1, :m + 1], aZ[0]), (name, mode, b)


def test_the_nothing_matched_rule_is_applied_per_pair():
    """Bin score 32 on set A: the oracle matches nothing in the 8 x 8 pair - all of that pair's scores are zero, as when it is the only pair
    of a call - and something in every other pair, whose scores stay; the matches are the oracle's."""
    counts, iters, alpha, _, _ = SETS['A32']
    s = _scores('A32')
    for mode, mutual in ((_lib.EXTRACT_DUSTBIN, False), (_lib.EXTRACT_DUSTBIN_MUTUAL, True)):
        m0, m1, s0, s1 = ops.sinkhorn_extract(s.to(DEV), alpha, iters, mode=mode, counts=_cnt(counts))
        for b, (n, m) in enumerate(counts):
            Zr = O.log_optimal_transport(s[b:b + 1, :n, :m], torch.tensor(alpha, dtype=torch.float64), iters)
            r0, r1, rs0, rs1 = O.extract_matches(Zr, 'triplet_loss', mutual, 0.2)
            assert bool((r0 >= 0).any()) == (b != UNMATCHED['A32']), b          # (what the set is here for)
            assert torch.equal(m0[b, :n].cpu(), r0[0].long()) and torch.equal(m1[b, :m].cpu(), r1[0].long()), (mode, b)
            if b == UNMATCHED['A32']:
                assert not s0[b].any() and not s1[b].any()
            else:
                assert s1[b, :m].any() and (s0[b, :n].cpu().double() - rs0[0].double()).abs().max() < 1e-4 \
                    and (s1[b, :m].cpu().double() - rs1[0].double()).abs().max() < 1e-4, (mode, b)


def test_ragged_sinkhorn_order_and_packed_counts():
    """Permuting the pairs permutes the results (every pair still equals itself alone); a pack_ragged-style dict serves as counts."""
    counts, iters, alpha, _, _ = SETS['s64']
    _, alone = _alone('s64')
    perm = [4, 2, 5, 0, 1, 3]
    h0 = torch.tensor([counts[p][0] for p in perm], dtype=torch.int32)
    h1 = torch.tensor([counts[p][1] for p in perm], dtype=torch.int32)
    packed = {'counts0': h0.to(DEV), 'counts1': h1.to(DEV), 'counts0_host': h0, 'counts1_host': h1}
    s = _scores('s64', order=perm, fill=1e300)
    Z = ops.sinkhorn(s.to(DEV), alpha, iters, counts=packed)
    m0 = ops.sinkhorn_extract(s.to(DEV), alpha, iters, counts=packed)[0]
    for i, p in enumerate(perm):
        n, m = counts[p]
        assert torch.equal(Z[i, :n + 1, :m + 1], alone[p][0][0]) and torch.equal(m0[i, :n], alone[p][1][0][0][0])


def test_ragged_sinkhorn_refusals():
    """Checked on the host copies before anything is launched, naming the first offending pair."""
    s = torch.zeros(3, 16, 16, device=DEV)
    with pytest.raises(RuntimeError, match='mdgat_sinkhorn_ragged: pair 1'):
        ops.sinkhorn(s, 1.0, 2, counts=([16, 0, 0], [16, 16, 16]))
    with pytest.raises(RuntimeError, match='mdgat_sinkhorn_extract_ragged: pair 2'):
        ops.sinkhorn_extract(s, 1.0, 2, counts=([16, 16, 16], [16, 16, 17]))
    with pytest.raises(RuntimeError, match='at most 512'):
        ops.sinkhorn(torch.zeros(1, 8, 513, device=DEV), 1.0, 2, counts=([8], [8]))
    with pytest.raises(RuntimeError, match='at most 512'):
        ops.sinkhorn_extract(torch.zeros(1, 513, 8, device=DEV), 1.0, 2, counts=([8], [8]))
    with pytest.raises(ValueError, match='3 entries'):
        ops.sinkhorn(s, 1.0, 2, counts=([16, 16], [16, 16]))
