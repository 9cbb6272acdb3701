"""Ragged batches in WIDE slots through the fp32-class attention kernels (ops.attention with counts= and wide=True: mdgat_attention_ragged_wide),
self and cross, full and k = 64, with and without the selection tap:

    w4      544 x 520     wide<4> (17 key blocks), the windowed kernel    (544, 520), (70, 300), (513, 64), (256, 512)
    w8      1056 x 1040   wide<8> (33 key blocks)                         (1056, 1040), (90, 1030), (1025, 70), (768, 1024)
    whole4  1024 x 1024   the per-pair `whole` under NW = 4               (1024, 1024), (1000, 1024)
    whole8  2048 x 2048   the per-pair `whole` under NW = 8               (2048, 2048), (1500, 2047)

Pairs of 64 and 70 keys leave NW - 1 waves of a tile without a key; the key counts are on and off multiples of 256, 32 and 8.  The padding rows
of q, k and v hold NaN.  The yardstick is tests/test_gpu_ragged_attention_fp32.py's: the fp64 torch attention on each pair's own rows, its
message bound (1e-5), exactly k kept keys per row, all inside the pair's counts; the selection is torch.topk's on every row whose fp64 gap
between the k-th and the (k+1)-th logit is at least parity_util.GAP_EPS - the exempt rows are decided from the fp64 logits alone and asserted,
from them alone, to be under 1 % of the rows."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mdgat_matcher_amd import ops  # noqa: E402
from oracle import mdgat_oracle as O  # noqa: E402
from parity_util import GAP_EPS  # noqa: E402
from test_gpu_ragged_attention_fp32 import MSG_TOL, _lib_msg  # noqa: E402

DEV = 'cuda:0'
K = 64
EXEMPT_FRAC = 0.01
SETS = {
    'w4': ((544, 520), ((544, 520), (70, 300), (513, 64), (256, 512))),
    'w8': ((1056, 1040), ((1056, 1040), (90, 1030), (1025, 70), (768, 1024))),
    'whole4': ((1024, 1024), ((1024, 1024), (1000, 1024))),
    'whole8': ((2048, 2048), ((2048, 2048), (1500, 2047))),
}
WINDOWED, WIDE4, WIDE4_TAP, WIDE8, WIDE8_TAP = ops.RAGGED_WIDE_LAUNCHES[4:]
DYNAMIC = {'w4': WIDE4, 'w8': WIDE8, 'whole4': WIDE4, 'whole8': WIDE8}
CASES = [(name, k) for name in SETS for k in (0, K)]


def _qkv(name, order=None, seed=11, fill=float('nan')):
    """[B, Np + Mp, 3, 4, 32]: pair b's frames at rows 0 .. N_b and Np .. Np + M_b, `fill` everywhere else; a pair's rows follow from its own
    sizes and the seed alone, wherever it stands"""
    (Np, Mp), counts = SETS[name]
    order = range(len(counts)) if order is None else order
    x = np.full((len(order), Np + Mp, 3, 4, 32), fill)
    for i, b in enumerate(order):
        n, m = counts[b]
        rs = np.random.RandomState(seed + 1000 * n + m)
        x[i, :n] = rs.standard_normal((n, 3, 4, 32)) * 1.3
        x[i, Np:Np + m] = rs.standard_normal((m, 3, 4, 32)) * 1.3
    return torch.from_numpy(x)


@functools.lru_cache(maxsize=None)
def _reference(name, cross, k):
    """Per pair and side, computed once on the CPU in fp64 and never modified: the oracle's message rows [n, 128], and for the dynamic case the
    kept keys of torch.topk on the fp64 logits [H, n, keys] with the exempt rows [H, n] (a k-th gap below GAP_EPS)."""
    (Np, Mp), counts = SETS[name]
    qkv = _qkv(name, seed=11 + cross)
    out = []
    for b, (n, m) in enumerate(counts):
        frames = (qkv[b, :n], qkv[b, Np:Np + m])
        sides = []
        for side in (0, 1):
            src = frames[1 - side if cross else side]
            q = frames[side][:, 0].permute(2, 1, 0)[None]          # [1, dh, H, nq]
            kk, v = src[:, 1].permute(2, 1, 0)[None], src[:, 2].permute(2, 1, 0)[None]
            if not k:
                sides.append((_lib_msg(O.attention(q, kk, v)[0]), None, None))
                continue
            logits = torch.einsum('bdhn,bdhm->bhnm', q, kk)[0] / 32 ** 0.5       # [H, nq, nk]
            nk = logits.shape[-1]
            keep = torch.zeros_like(logits, dtype=torch.bool).scatter_(2, logits.topk(k, dim=2).indices, True)
            if k < nk:
                top = logits.topk(k + 1, dim=2).values
                near = (top[..., k - 1] - top[..., k]) < GAP_EPS
            else:
                near = torch.zeros(logits.shape[:2], dtype=torch.bool)
            sides.append((_lib_msg(O.dynamic_attention(q, kk, v, k)[0]), keep, near))
        out.append(sides)
    return qkv, out


def _run(name, qkv, order, cross, k, tap):
    """ops.attention on the ragged batch; the wide counters show the instantiation the slots select, launched once, and no other"""
    (Np, Mp), counts = SETS[name]
    cnt = ([counts[b][0] for b in order], [counts[b][1] for b in order])
    want = WINDOWED if not k else {WIDE4: WIDE4_TAP, WIDE8: WIDE8_TAP}[DYNAMIC[name]] if tap else DYNAMIC[name]
    before = ops.ragged_wide_launches()
    got = ops.attention(qkv.to(DEV), Np, Mp, cross, topk=k, return_selection=tap, counts=cnt, wide=True)
    after = ops.ragged_wide_launches()
    assert {n: after[n] - before[n] for n in after if after[n] != before[n]} == {want: 1}, (name, k, tap)
    return got


@pytest.mark.parametrize('cross', [False, True])
@pytest.mark.parametrize('name,k', CASES)
def test_against_the_oracle_on_every_pairs_own_rows(name, k, cross):
    (Np, Mp), counts = SETS[name]
    qkv, ref = _reference(name, cross, k)
    order = list(range(len(counts)))
    msg = _run(name, qkv, order, cross, k, tap=False).cpu()
    masks = None
    if k:
        tapped, masks = _run(name, qkv, order, cross, k, tap=True)
        masks = [t.cpu() for t in masks]
        tapped = tapped.cpu()
    assert torch.isfinite(msg).all()
    rows = exempt = 0
    for b, (n, m) in enumerate(counts):
        assert not msg[b, n:Np].any() and not msg[b, Np + m:].any(), b          # the rows beyond the pair's counts are exactly 0 (their inputs are NaN)
        for side, (lo, c) in enumerate(((0, n), (Np, m))):
            want, keep, near = ref[b][side]
            err = (msg[b, lo:lo + c].double() - want).abs().reshape(c, 4, 32).amax(2)                   # [c, H]
            if not k:
                print(f'{name} cross={cross} full pair {b} ({n} x {m}) side {side}: max |msg - oracle| = {err.max():.3e}')
                assert err.max() < MSG_TOL, (b, side, float(err.max()))
                continue
            nk = keep.shape[-1]
            sel = masks[side][b, :, :c]                                           # [H, c, slot keys]
            assert (sel.sum(-1) == k).all(), (b, side)                            # exactly k kept keys per row
            assert not sel[..., nk:].any(), (b, side)                             # none beyond the pair's counts
            assert not masks[side][b, :, c:].any(), (b, side)                     # no tap word beyond its queries
            ok = ~near                                                            # [H, c]
            assert torch.equal(sel[..., :nk][ok], keep[ok]), (b, side)            # torch.topk's selection wherever the fp64 gap decides
            rows += near.numel()
            exempt += int(near.sum())
            okr = ok.permute(1, 0)                                                # [c, H]
            worst = float(err[okr].max()) if okr.any() else 0.0
            print(f'{name} cross={cross} k={k} pair {b} ({n} x {m}) side {side}: max |msg - oracle| = {worst:.3e}, exempt rows {int(near.sum())} of {near.numel()}')
            assert worst < MSG_TOL, (b, side, worst)
            # the tapped instantiation gives the untapped one's message bits (an exact tie at the k-th place - it can only be among the exempt
            # rows - is broken before the pass there and corrected after it here: to rounding)
            a, t = msg[b, lo:lo + c].reshape(c, 4, 32), tapped[b, lo:lo + c].reshape(c, 4, 32)
            assert torch.equal(a[okr], t[okr]), (b, side)
            assert (a - t).abs().max() < 1e-6, (b, side)
        if k:
            assert not tapped[b, n:Np].any() and not tapped[b, Np + m:].any(), b
    if k:
        print(f'{name} cross={cross} k={k}: {exempt} exempt rows of {rows}')
        assert exempt < EXEMPT_FRAC * rows           # (from the fp64 logits alone)


@pytest.mark.parametrize('name,k', [c for c in CASES if c[0] in ('w4', 'w8')])
def test_a_pairs_rows_do_not_depend_on_its_position_or_companions(name, k):
    """the same slots: the same bits under a permutation of the batch and in subsets of it (another batch size), the padding 1e300 instead of NaN"""
    counts = SETS[name][1]
    base = _run(name, _qkv(name, seed=12), list(range(len(counts))), True, k, tap=False)
    for order in ([3, 2, 1, 0], [1, 3], [2]):
        got = _run(name, _qkv(name, order=order, seed=12, fill=1e300), order, True, k, tap=False)
        for i, b in enumerate(order):
            assert torch.equal(got[i], base[b]), (order, b)


def test_narrow_slots_run_what_they_run_without_the_switch():
    import attention_forms as AF
    import test_gpu_ragged_attention_fp32 as RA
    counts = RA._counts('s256', 64)
    Np, Mp = RA._slots('s256')
    qkv = RA._qkv(counts, Np, Mp, 11).to(DEV)
    cnt = ([n for n, _ in counts], [m for _, m in counts])
    for k in (0, 64):
        before = ops.ragged_wide_launches()
        with AF.watch() as w:
            got = ops.attention(qkv, Np, Mp, True, topk=k, counts=cnt, wide=True)
        AF.assert_launched(w, AF.index(RA.SETS['s256'][3] if k else RA.SETS['s256'][2]), f'narrow slot, k={k}')
        assert ops.ragged_wide_launches() == before
        assert torch.equal(got, ops.attention(qkv, Np, Mp, True, topk=k, counts=cnt))


def test_refusals():
    """Checked on the host copies before the launch, naming the first offending pair; the old entry keeps its limit."""
    qkv = torch.zeros(2, 600 + 20, 3, 4, 32, device=DEV)
    with pytest.raises(RuntimeError, match='mdgat_attention_ragged_wide: pair 1: k=8 exceeds'):
        ops.attention(qkv, 600, 20, False, topk=8, counts=([600, 20], [20, 7]), wide=True)
    with pytest.raises(RuntimeError, match='mdgat_attention_ragged_wide: pair 0 has 601 x 20'):
        ops.attention(qkv, 600, 20, True, counts=([601, 20], [20, 20]), wide=True)
    with pytest.raises(RuntimeError, match='at most 2048 keypoints'):
        ops.attention(torch.zeros(1, 2049 + 20, 3, 4, 32, device=DEV), 2049, 20, False, counts=([20], [20]), wide=True)
    with pytest.raises(RuntimeError, match='at most 512 keypoints'):
        ops.attention(qkv, 600, 20, False, counts=([600, 20], [20, 20]))
    with pytest.raises(ValueError, match='needs counts'):
        ops.attention(qkv, 600, 20, False, wide=True)
