"""fp64 attention (csrc/f64.hip) at every instantiation and every branch of its row select, against the oracle.

Dynamic attention: the inputs of tests/attention_f64_rows.py - rows with outliers, tails, two modes, a narrow negative band, constant rows,
masses of exact duplicates and fp32-tied lists of 2 and of 32 at the k-th place - at the smallest launches that reach each search form
(tests/test_attention_f64_rows.py proves on the CPU which branches they reach).  The reference selection is the top k of every row under
the total order (fp64 logit descending, key ascending): torch.topk's keys wherever those are specified, and this library's documented rule
on exact ties; the reference message is the oracle's dynamic_attention with that selection forced.  EVERY row is compared, the tied ones at
the full F64_TOL: under the rule the choice is determined.  The launch without the selection tap - what a forward runs - must return the
same message bits, and the launch counters (mdgat_attention_f64_launches) must show the two intended instantiations and no other.

Full attention: the automatic choice between 16 queries, 32 queries and one wave per 32 queries, at three batch sizes taken from
mdgat_attention_f64_plan for the device's CU count."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_f64_forms as F  # noqa: E402
import attention_f64_rows as R  # noqa: E402
from mdgat_matcher_amd import _lib, ops  # noqa: E402
from oracle import mdgat_oracle as O  # noqa: E402

DEV = 'cuda:0'
F64_TOL = 1e-11         # as tests/test_gpu_f64.py: the fp64 kernels against torch fp64 on the same operands (summation order only)


def _to_lib(msg):
    b, dh, h, n = msg.shape
    return msg.permute(0, 3, 2, 1).reshape(b, n, h * dh)


def _launched(w):
    return {i: int(n) for i, n in enumerate(w.delta) if n}


def _against_the_oracle(case, msg, masks):
    """every row of every pair: the kept keys equal the reference selection, the message is within F64_TOL of the oracle's on that selection;
    rows and masks beyond a pair's counts are zero"""
    x = case.qkv()
    worst, wrong = 0.0, 0
    for (b, side), (logits, kept) in case.reference().items():
        (ql, nq), (kl, nk) = next((q, k) for bb, s, h, q, k in case.units() if (bb, s, h) == (b, side, 0))
        got = masks[side][b, :, :nq, :nk]
        bad = int((got ^ kept).any(-1).sum())
        q, kk, v = (x[b, lo:lo + n, i].permute(2, 1, 0)[None] for lo, n, i in ((ql, nq, 0), (kl, nk, 1), (kl, nk, 2)))
        ref, _ = O.dynamic_attention(q, kk, v, min(case.k, nk), forced=kept[None])
        err = (msg[b, ql:ql + nq] - _to_lib(ref)[0]).abs().max().item()
        print(f'{case.id} pair {b} frame {side} ({nq} queries x {nk} keys): {bad} rows select other keys, max |msg - oracle| = {err:.3e}')
        wrong += bad
        worst = max(worst, err)
        rest = masks[side][b].clone()
        rest[:, :nq, :nk] = False
        assert not rest.any(), (b, side)
    assert wrong == 0, f'{wrong} rows keep other keys than the reference'
    assert worst < F64_TOL, worst
    for b, (n, m) in enumerate(case.pair_counts()):
        assert not msg[b, n:case.N].any() and not msg[b, case.N + m:].any(), b


def _run(case):
    """the case with and without the selection tap -> (msg, masks) on the CPU; asserts the two instantiations and equal message bits"""
    x = case.qkv().to(DEV)
    cnt = dict(counts=([n for n, _ in case.counts], [m for _, m in case.counts])) if case.counts else {}
    with F.watch() as w:
        msg, masks = ops.attention_f64(x, case.N, case.M, case.cross, topk=case.k, return_selection=True, **cnt)
        plain = ops.attention_f64(x, case.N, case.M, case.cross, topk=case.k, **cnt)
    tap = F.KEEP_TAP if max(case.N, case.M) <= 512 else F.RECOMPUTE_TAP
    assert _launched(w) == {tap: 1, tap + 1: 1}, (w.launched(), F.NAMES[tap])
    assert torch.equal(plain, msg), f'without the tap: max difference {(plain - msg).abs().max().item():.3e}'
    return msg.cpu(), [m.cpu() for m in masks]


@pytest.mark.parametrize('case', R.UNIFORM_CASES, ids=lambda c: c.id)
def test_dynamic_attention_f64_selects_and_sums_like_the_oracle(case):
    msg, masks = _run(case)
    _against_the_oracle(case, msg, masks)


@pytest.mark.parametrize('case', R.RAGGED_CASES, ids=lambda c: c.id)
def test_ragged_dynamic_attention_f64_against_the_oracle_and_the_pair_alone(case):
    """Per pair against the oracle (NaN in the padding), and against the pair alone: the same bits wherever both launches run the same
    instantiation - the larger frame of the pair and of the batch on the same side of 512 keys, and k below the pair's counts (alone,
    k = N_b = M_b is full attention) - and within F64_TOL otherwise; the kept keys are the same always."""
    msg, masks = _run(case)
    _against_the_oracle(case, msg, masks)
    x = case.qkv()
    cus = F.cu_count()
    for b, (n, m) in enumerate(case.pair_counts()):
        alone = torch.cat([x[b:b + 1, :n], x[b:b + 1, case.N:case.N + m]], 1).to(DEV)
        with F.watch() as w:
            amsg, amasks = ops.attention_f64(alone, n, m, case.cross, topk=case.k, return_selection=True)
        want = F.plan(1, n, m, case.k, True, cus=cus)
        assert _launched(w) == {want: 1}, (b, w.launched(), F.NAMES[want])
        same = want == (F.KEEP_TAP if max(case.N, case.M) <= 512 else F.RECOMPUTE_TAP)
        assert same == ((max(n, m) <= 512) == (max(case.N, case.M) <= 512) and not (case.k == n and case.k == m))
        mine = torch.cat([msg[b:b + 1, :n], msg[b:b + 1, case.N:case.N + m]], 1)
        err = (mine - amsg.cpu()).abs().max().item()
        print(f'{case.id} pair {b} ({n} x {m}): max |ragged - alone| = {err:.3e} (same instantiation: {same})')
        assert torch.equal(mine, amsg.cpu()) if same else err < F64_TOL, (b, err)
        nk = (m, n) if case.cross else (n, m)
        assert torch.equal(masks[0][b, :, :n, :nk[0]], amasks[0][0].cpu()) and torch.equal(masks[1][b, :, :m, :nk[1]], amasks[1][0].cpu()), b


@pytest.mark.parametrize('cross', [False, True])
def test_full_attention_f64_under_the_automatic_form(cross):
    """40 x 40 keypoints at the three batch sizes mdgat_attention_f64_plan gives for this device (256 CUs: 4, 32 and 128 pairs): 16 queries
    per workgroup, 32 queries, one wave per 32 queries - each against the oracle, with the instantiation asserted."""
    lib = _lib.load()
    cus = F.cu_count()
    batches = F.full_attention_batches(40, 40, cus)
    assert None not in batches, (cus, batches)
    prev = lib.mdgat_set_f64_attention_form(-1)
    try:
        for B, want in zip(batches, (F.FULL16, F.FULL32, F.SOLO)):
            rs = np.random.RandomState(B + cross)
            qkv = torch.from_numpy(rs.standard_normal((B, 80, 3, 4, 32)) * 1.3)
            with F.watch() as w:
                out = ops.attention_f64(qkv.to(DEV), 40, 40, cross).cpu()
            assert _launched(w) == {want: 1}, (B, cus, w.launched(), F.NAMES[want])
            for lo, slo in ((0, 40 if cross else 0), (40, 0 if cross else 40)):
                q, k, v = (qkv[:, a:a + 40, i].permute(0, 3, 2, 1) for a, i in ((lo, 0), (slo, 1), (slo, 2)))
                err = (out[:, lo:lo + 40] - _to_lib(O.attention(q, k, v)[0])).abs().max().item()
                print(f'B={B} cross={cross} {F.NAMES[want]} frame at {lo}: max |msg - oracle| = {err:.3e}')
                assert err < F64_TOL, (B, err)
    finally:
        lib.mdgat_set_f64_attention_form(prev)
