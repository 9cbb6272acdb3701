"""Ragged batches in WIDE slots through the fp32 Sinkhorn and its match extraction: ops.sinkhorn / ops.sinkhorn_extract with counts= and
wide=True (mdgat_sinkhorn_ragged_wide, mdgat_sinkhorn_extract_ragged_wide), on the one-workgroup kernel and on the split form.

Slots (the scores beyond every pair's counts are NaN; every call runs with its outputs and its workspace prefilled with 0xFF: NaN):
    nc16   520 x 544    sinkhorn_kernel<16, 8, RAGGED>; split: 5 slabs, NC = 16, 8 waves
    nc32   1040 x 1056  sinkhorn_kernel<32, 8, RAGGED>; split: 9 slabs, NC = 32, 8 waves
    cols   65 x 600     few rows, wide columns: one slab, so split=True keeps the one-workgroup kernel and its bits
    rows   600 x 65     the old <2, 16, RAGGED> in a slot of 600 rows; split: G = 5 slabs with NC = 2 (the 16-slab instantiation, 16 waves)
    big    2048 x 2048  one pair of 1500 x 2048; split: 16 slabs of which the pair's rows fill 12
    U      600 x 65     bin score 32: the oracle leaves the 8 x 8 pair - and no other - without a match

The one-workgroup form is held to the pair run ALONE through the uniform streaming kernel (streaming=True), bit for bit, and to the oracle
within Z_TOL.  The split form merges its column sums in another order: it is held to the oracle and to the default form within Z_TOL, and to
the default form's matches wherever the oracle decides them (an arg-max margin of at least Z_TOL; see _decided)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sinkhorn_forms as SF  # noqa: E402
from mdgat_matcher_amd import _lib, ops  # noqa: E402
from oracle import mdgat_oracle as O  # noqa: E402
from parity_util import Z_TOL  # noqa: E402
from prefilled import prefilled  # noqa: E402

DEV = 'cuda:0'
THR = 0.01
ITERS = 20
# name -> (slot, counts, bin score, scale and offset of the random scores)
SETS = {
    'nc16': ((520, 544), ((520, 544), (130, 513), (64, 70), (513, 64)), 0.7, 4.0, 0.0),
    'nc32': ((1040, 1056), ((1040, 1056), (90, 1025), (300, 70)), 0.7, 4.0, 0.0),
    'cols': ((65, 600), ((65, 600), (17, 513), (64, 64)), 0.7, 4.0, 0.0),
    'rows': ((600, 65), ((600, 65), (513, 17), (100, 65), (129, 33)), 0.7, 4.0, 0.0),
    'big': ((2048, 2048), ((1500, 2048),), 0.7, 4.0, 0.0),
    'U': ((600, 65), ((600, 65), (8, 8), (130, 33)), 32.0, 3.0, 27.0),
}
UNMATCHED = {'U': 1}
SK16, SK32, ITER, FINISH = ops.RAGGED_WIDE_LAUNCHES[:4]
# what one default-form call launches: the wide counter, or the old RAGGED instantiation's name (mdgat_sinkhorn_launches)
ONE_WORKGROUP = {'nc16': SK16, 'nc32': SK32, 'cols': SK16, 'rows': 'stream<2,16>,RAGGED', 'big': SK32, 'U': 'stream<2,16>,RAGGED'}
SLABS = {name: (slot[0] + 127) // 128 for name, (slot, *_) in SETS.items()}


def _cnt(counts):
    return [n for n, _ in counts], [m for _, m in counts]


def _scores(name, order=None, fill=float('nan')):
    """[B, Np, Mp] float64 scores in the set's slot, `fill` beyond every pair's counts; a pair's scores follow from its own sizes alone"""
    (Np, Mp), counts, _, scale, offset = SETS[name]
    order = range(len(counts)) if order is None else order
    s = np.full((len(order), Np, Mp), fill)
    for i, b in enumerate(order):
        n, m = counts[b]
        s[i, :n, :m] = np.random.RandomState(5 + 1000 * n + m).standard_normal((n, m)) * scale + offset
    return torch.from_numpy(s)


class watch:
    """both counter sets around a region: ``launched()`` = {name: launches} of mdgat_sinkhorn_launches and mdgat_ragged_wide_launches"""

    def __enter__(self):
        self.sf = SF.watch().__enter__()
        self.before = ops.ragged_wide_launches()
        return self

    def __exit__(self, *exc):
        self.sf.__exit__(*exc)
        after = ops.ragged_wide_launches()
        self.wide = {k: after[k] - self.before[k] for k in after if after[k] != self.before[k]}

    def launched(self):
        return {**self.sf.launched(), **self.wide}


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """per pair: the oracle's Z [n+1, m+1] (fp64, CPU) - computed once, never modified"""
    _, counts, alpha, _, _ = SETS[name]
    s = _scores(name)
    return [O.log_optimal_transport(s[b:b + 1, :n, :m], torch.tensor(alpha, dtype=torch.float64), ITERS)[0] for b, (n, m) in enumerate(counts)]


@functools.lru_cache(maxsize=None)
def _alone(name):
    """every pair of the set run alone through the uniform streaming kernel: Z and, per extraction mode, (m0, m1, s0, s1, Z)"""
    _, counts, alpha, _, _ = SETS[name]
    s = _scores(name)
    out = []
    for b, (n, m) in enumerate(counts):
        sb = s[b:b + 1, :n, :m].contiguous().to(DEV)
        Z = ops.sinkhorn(sb, alpha, ITERS, streaming=True)
        out.append((Z, [ops.sinkhorn_extract(sb, alpha, ITERS, mode=mode, match_threshold=THR, want_Z=True, streaming=True) for mode in range(4)]))
    return out


@functools.lru_cache(maxsize=None)
def _default(name):
    """the set through the wide entries' default form, under 0xFF: Z and, per mode, (m0, m1, s0, s1, Z); with what each call launched"""
    _, counts, alpha, _, _ = SETS[name]
    s = _scores(name).to(DEV)
    with prefilled('ones'):
        with watch() as wz:
            Z = ops.sinkhorn(s, alpha, ITERS, counts=_cnt(counts), wide=True)
        ex = []
        for mode in range(4):
            with watch() as we:
                ex.append(ops.sinkhorn_extract(s, alpha, ITERS, mode=mode, match_threshold=THR, want_Z=True, counts=_cnt(counts), wide=True))
        torch.cuda.synchronize()
    return Z, ex, wz.launched(), we.launched()


@functools.lru_cache(maxsize=None)
def _split(name):
    _, counts, alpha, _, _ = SETS[name]
    s = _scores(name).to(DEV)
    with prefilled('ones') as p:
        with watch() as wz:
            Z = ops.sinkhorn(s, alpha, ITERS, counts=_cnt(counts), wide=True, split=True)
        ex = []
        for mode in range(4):
            for want_Z in (True, False):
                with watch() as we:
                    got = ops.sinkhorn_extract(s, alpha, ITERS, mode=mode, match_threshold=THR, want_Z=want_Z, counts=_cnt(counts), wide=True, split=True)
                if want_Z:
                    ex.append(got)
                else:
                    for a, b in zip(got, ex[-1][:4]):            # (Z in the workspace or in the caller's buffer: the same matches)
                        assert torch.equal(a, b), (name, mode)
        torch.cuda.synchronize()
    return Z, ex, wz.launched(), we.launched(), p.scratch_bytes


# ---------------------------------------------------------------------------------------------------- the one-workgroup form
@pytest.mark.parametrize('name', list(SETS))
def test_one_workgroup_form_equals_every_pair_alone_and_the_oracle(name):
    (Np, Mp), counts, _, _, _ = SETS[name]
    Z, ex, launched_z, launched_ex = _default(name)
    assert launched_z == {ONE_WORKGROUP[name]: 1} and launched_ex == {ONE_WORKGROUP[name]: 1, SF.EXTRACT: 1}, (launched_z, launched_ex)
    assert tuple(Z.shape) == (len(counts), Np + 1, Mp + 1)
    alone = _alone(name)
    for b, (n, m) in enumerate(counts):
        assert torch.equal(Z[b, :n + 1, :m + 1], alone[b][0][0]), (name, b)
        rest = Z[b].clone()
        rest[:n + 1, :m + 1] = 0
        assert not rest.any(), (name, b)                      # (NaN counts as something)
        err = (Z[b, :n + 1, :m + 1].cpu().double() - _oracle(name)[b]).abs().max().item()
        print(f'{name} pair {b} ({n} x {m}): max |Z - oracle| = {err:.3e}')
        assert err < Z_TOL, (name, b, err)
        for mode in range(4):
            m0, m1, s0, s1, Zx = ex[mode]
            a0, a1, as0, as1, aZ = alone[b][1][mode]
            assert torch.equal(m0[b, :n], a0[0]) and torch.equal(m1[b, :m], a1[0]), (name, mode, b)
            assert torch.equal(s0[b, :n], as0[0]) and torch.equal(s1[b, :m], as1[0]), (name, mode, b)
            assert (m0[b, n:] == -1).all() and (m1[b, m:] == -1).all() and not s0[b, n:].any() and not s1[b, m:].any(), (name, mode, b)
            assert torch.equal(Zx[b], Z[b]), (name, mode, b)


# ---------------------------------------------------------------------------------------------------- the split form
def _decided(Zr, n, m, mode):
    """From the oracle's Z alone: the rows and the columns whose arg-max (over the range extraction `mode` scans) leads the runner-up by
    at least Z_TOL and, in the threshold modes, whose best probability is at least Z_TOL away from the threshold (|d exp(z)| <= |dz| for
    z <= 0).  Below that margin two forms that are each within Z_TOL of the oracle may order two candidates differently."""
    inner = mode >= 2
    rows = Zr[:n, :m] if inner else Zr[:n, :m + 1]
    cols = Zr[:n, :m] if inner else Zr[:n + 1, :m]
    def margin(t, dim):
        if t.shape[dim] < 2:
            return torch.full((t.shape[1 - dim],), float('inf'), dtype=t.dtype), t.max(dim=dim).values
        top = t.topk(2, dim=dim).values
        return (top.select(dim, 0) - top.select(dim, 1)), top.select(dim, 0)
    gr, br = margin(rows, 1)
    gc, bc = margin(cols, 0)
    okr, okc = gr >= Z_TOL, gc >= Z_TOL
    if inner:
        okr &= (br.exp() - THR).abs() >= Z_TOL
        okc &= (bc.exp() - THR).abs() >= Z_TOL
    return okr, okc


@pytest.mark.parametrize('name', [n for n in SETS if n != 'cols'])
def test_split_form_against_the_oracle_and_the_default_form(name):
    """Z within Z_TOL of the oracle and of the default form; the default form's matches on every row and column the oracle decides
    (_decided), which the test asserts - from the oracle alone - to be more than 99 in 100 of each pair's; 0 over the rest of the slot;
    the launches counted; the workspace asked for holds a Z and the scratch, and the 0xFF fill reached an allocation of that size."""
    (Np, Mp), counts, _, _, _ = SETS[name]
    B, G = len(counts), SLABS[name]
    Z, ex, launched_z, launched_ex, scratch = _split(name)
    assert launched_z == {ITER: ITERS, FINISH: 1} and launched_ex == {ITER: ITERS, FINISH: 1, SF.EXTRACT: 1}, (launched_z, launched_ex)
    need = _lib.load().mdgat_sinkhorn_ragged_wide_workspace_bytes(B, Np, Mp)
    assert need >= 4 * B * ((Np + 1) * (Mp + 1) + 2 * G * Mp * 2 + 2 * (Np + 1)) and scratch >= need, (need, scratch)
    Zd, exd, _, _ = _default(name)
    worst_o = worst_d = 0.0
    for b, (n, m) in enumerate(counts):
        rest = Z[b].clone()
        rest[:n + 1, :m + 1] = 0
        assert not rest.any(), (name, b)
        err = (Z[b, :n + 1, :m + 1].cpu().double() - _oracle(name)[b]).abs().max().item()
        err_d = (Z[b].double() - Zd[b].double()).abs().max().item()
        worst_o, worst_d = max(worst_o, err), max(worst_d, err_d)
        print(f'{name} pair {b} ({n} x {m}): max |Z - oracle| = {err:.3e}, max |Z - default form| = {err_d:.3e}')
        assert err < Z_TOL and err_d < Z_TOL, (name, b, err, err_d)
        for mode in range(4):
            m0, m1, s0, s1, Zx = ex[mode]
            d0, d1 = exd[mode][0], exd[mode][1]
            assert torch.equal(Zx[b], Z[b]), (name, mode, b)
            assert (m0[b, n:] == -1).all() and (m1[b, m:] == -1).all() and not s0[b, n:].any() and not s1[b, m:].any(), (name, mode, b)
            okr, okc = _decided(_oracle(name)[b], n, m, mode)
            if mode == _lib.EXTRACT_THRESHOLD_MUTUAL:      # a row's match depends on its column's arg-max as well: the pair as a whole
                if not (okr.all() and okc.all()):
                    print(f'{name} pair {b} mode {mode}: undecided ({int((~okr).sum())} rows, {int((~okc).sum())} columns)')
                    continue
            okr, okc = okr.to(DEV), okc.to(DEV)
            assert torch.equal(m0[b, :n][okr], d0[b, :n][okr]) and torch.equal(m1[b, :m][okc], d1[b, :m][okc]), (name, mode, b)
            assert okr.float().mean() > 0.99 and okc.float().mean() > 0.99, (name, mode, b)          # (from the oracle alone: the check is not empty)
    print(f'{name}: largest |dZ| against the oracle {worst_o:.3e}, against the default form {worst_d:.3e}')


def test_a_slot_of_one_slab_keeps_the_one_workgroup_kernel():
    Z, ex, launched_z, launched_ex, _ = _split('cols')
    Zd, exd, _, _ = _default('cols')
    assert launched_z == {SK16: 1} and launched_ex == {SK16: 1, SF.EXTRACT: 1}
    assert torch.equal(Z, Zd)
    for mode in range(4):
        for a, b in zip(ex[mode], exd[mode]):
            assert torch.equal(a, b), mode


@pytest.mark.parametrize('name,orders', [('nc16', ([3, 0, 2, 1], [0, 2], [1])), ('nc32', ([2, 1, 0], [1])), ('rows', ([1, 3, 0, 2], [3]))])
@pytest.mark.parametrize('split', [False, True])
def test_bits_do_not_depend_on_position_or_companions(name, orders, split):
    """permutations and subsets in the same slot (the slot is the set's whatever the pairs), the padding 1e300 instead of NaN"""
    _, counts, alpha, _, _ = SETS[name]
    ref = (_split(name) if split else _default(name))[0]
    for order in orders:
        s = _scores(name, order=order, fill=1e300).to(DEV)
        with prefilled('ones'):
            Z = ops.sinkhorn(s, alpha, ITERS, counts=_cnt([counts[b] for b in order]), wide=True, split=split)
        for i, b in enumerate(order):
            assert torch.equal(Z[i], ref[b]), (name, order, b)


# ---------------------------------------------------------------------------------------------------- both forms
@pytest.mark.parametrize('split', [False, True])
def test_the_nothing_matched_rule_is_applied_per_pair(split):
    """Bin score 32: the oracle matches nothing in the 8 x 8 pair - all of that pair's scores are zero - and something in every other pair,
    whose scores stay; the matches are the oracle's."""
    _, counts, alpha, _, _ = SETS['U']
    ex = (_split('U') if split else _default('U'))[1]
    for mode, mutual in ((_lib.EXTRACT_DUSTBIN, False), (_lib.EXTRACT_DUSTBIN_MUTUAL, True)):
        m0, m1, s0, s1, _ = ex[mode]
        for b, (n, m) in enumerate(counts):
            r0, r1, rs0, rs1 = O.extract_matches(_oracle('U')[b][None], 'triplet_loss', mutual, 0.2)
            assert bool((r0 >= 0).any()) == (b != UNMATCHED['U']), b          # (what the set is here for)
            okr, okc = _decided(_oracle('U')[b], n, m, mode)
            assert torch.equal(m0[b, :n].cpu()[okr], r0[0].long()[okr]) and torch.equal(m1[b, :m].cpu()[okc], r1[0].long()[okc]), (mode, b)
            if b == UNMATCHED['U']:
                assert okr.all() and okc.all() and not s0[b].any() and not s1[b].any()
            else:
                assert s1[b, :m].any() and s0[b, :n].any(), (mode, b)


def test_narrow_slots_run_what_they_run_without_the_switch():
    """a slot within 512 x 512 through the wide entries: the old RAGGED instantiation, counted where it was, and the old entries' bits"""
    import test_gpu_ragged_sinkhorn_fp32 as RS
    counts, iters, alpha, _, _ = RS.SETS['s256']
    s = RS._scores('s256').to(DEV)
    with watch() as w:
        Z = ops.sinkhorn(s, alpha, iters, counts=RS._cnt(counts), wide=True)
    assert w.launched() == {RS.RAGGED_FORM['s256']: 1}
    assert torch.equal(Z, ops.sinkhorn(s, alpha, iters, counts=RS._cnt(counts)))
    got = ops.sinkhorn_extract(s, alpha, iters, mode=1, match_threshold=THR, counts=RS._cnt(counts), wide=True)
    for a, b in zip(got, ops.sinkhorn_extract(s, alpha, iters, mode=1, match_threshold=THR, counts=RS._cnt(counts))):
        assert torch.equal(a, b)


def test_refusals():
    s = torch.zeros(2, 600, 16, device=DEV)
    with pytest.raises(RuntimeError, match='mdgat_sinkhorn_ragged_wide: pair 1 has 601 x 16 keypoints'):
        ops.sinkhorn(s, 1.0, 2, counts=([600, 601], [16, 16]), wide=True)
    with pytest.raises(RuntimeError, match='mdgat_sinkhorn_extract_ragged_wide: pair 0'):
        ops.sinkhorn_extract(s, 1.0, 2, counts=([600, 600], [0, 16]), wide=True, split=True)
    with pytest.raises(RuntimeError, match='padded sizes 8 x 2049: fp32 ragged batches hold at most 2048 keypoints per frame'):
        ops.sinkhorn(torch.zeros(1, 8, 2049, device=DEV), 1.0, 2, counts=([8], [8]), wide=True)
    with pytest.raises(RuntimeError, match='at most 512'):
        ops.sinkhorn(s, 1.0, 2, counts=([600, 600], [16, 16]))
    with pytest.raises(ValueError, match='need counts'):
        ops.sinkhorn(s, 1.0, 2, wide=True)
    with pytest.raises(ValueError, match='needs wide=True'):
        ops.sinkhorn(s, 1.0, 2, counts=([600, 600], [16, 16]), split=True)
    assert torch.isfinite(ops.sinkhorn(s, 1.0, 2, counts=([600, 17], [16, 16]), wide=True, split=True)).all()
