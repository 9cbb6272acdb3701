"""Ragged batches through the fp32-class attention kernel (ops.attention with counts=): pairs of different sizes in padded slots of one
launch, self and cross, full and dynamic, on count sets that reach every ragged instantiation of attention_kernel - full<4>, full<8>,
dyn<4>, dyn<8>, dyn<16> and the TAP twins of the three dynamic ones (read from the launch counters).

The yardstick is tests/test_gpu_ops.py's own: the fp64 torch attention (the oracle) on the pair's OWN q/k/v rows, with that file's bounds
(test_attention_full, test_attention_topk): 1e-5 on the messages; a dynamic row whose k-th and (k+1)-th largest fp64 logits are closer than
5e-6 may keep the other key, and fewer than 2e-3 of all rows are such near ties.  The padding rows of every input hold NaN."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_forms as AF  # noqa: E402
from mdgat_matcher_amd import ops  # noqa: E402
from oracle import mdgat_oracle as O  # noqa: E402

DEV = 'cuda:0'
MSG_TOL = 1e-5          # test_gpu_ops.py: test_attention_full, test_attention_topk
NEAR_TIE = 5e-6         # ... a k-th gap of the fp64 logits below this is not resolved in fp32
NEAR_TIE_FRAC = 2e-3

# name -> (count set, the k of its dynamic cases, the full and the dynamic instantiation its slots select)
SETS = {
    's128': (((40, 100), (100, 40), (128, 128), (8, 8), (33, 97), (1, 5)), (8,), 'full<4>', 'dyn<4>'),
    's256': (((200, 130), (130, 256), (256, 200), (64, 64)), (64,), 'full<8>', 'dyn<8>'),       # (64, 64): k = the pair's whole key count
    's512': (((300, 500), (500, 300), (512, 512), (65, 48)), (48, 64), 'full<8>', 'dyn<16>'),   # k = 48: all keys of (65, 48)'s frame 1
}
CASES = [(name, k) for name, (_, ks, _, _) in SETS.items() for k in (0, *ks)]


def _counts(name, k):
    """the pairs of the set that have k keys in both frames (torch.topk raises on the others, and so does the entry)"""
    return tuple(c for c in SETS[name][0] if min(c) >= max(k, 1))


def _qkv(counts, Np, Mp, seed, fill=float('nan')):
    """[B, Np + Mp, 3, 4, 32]: pair b's frames at rows 0 .. N_b and Np .. Np + M_b, `fill` everywhere else; a pair's rows follow from its
    own sizes and the seed alone, wherever it stands"""
    x = np.full((len(counts), Np + Mp, 3, 4, 32), fill)
    for b, (n, m) in enumerate(counts):
        rs = np.random.RandomState(seed + 1000 * n + m)
        x[b, :n] = rs.standard_normal((n, 3, 4, 32)) * 1.3
        x[b, Np:Np + m] = rs.standard_normal((m, 3, 4, 32)) * 1.3
    return torch.from_numpy(x)


def _slots(name):
    counts = SETS[name][0]
    return max(n for n, _ in counts), max(m for _, m in counts)


def _lib_msg(ref):
    """reference message [1, dh, H, n] -> library rows [n, H * dh]"""
    return ref.permute(0, 3, 2, 1).reshape(ref.shape[3], -1)


@functools.lru_cache(maxsize=None)
def _reference(name, cross, k):
    """Per pair and side, computed once on the CPU in fp64 and never modified: the oracle's message rows [n, 128], and for a dynamic case
    the kept keys of torch.topk on the fp64 logits [H, n, keys] with the near-tie rows [H, n]."""
    counts = _counts(name, k)
    Np, Mp = _slots(name)
    qkv = _qkv(counts, Np, Mp, 11 + cross)
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
                near = (top[..., k - 1] - top[..., k]) < NEAR_TIE
            else:
                near = torch.zeros(logits.shape[:2], dtype=torch.bool)
            sides.append((_lib_msg(O.dynamic_attention(q, kk, v, k)[0]), keep, near))
        out.append(sides)
    return counts, qkv, out


def _run(name, counts, qkv, cross, k, tap):
    """ops.attention on the ragged batch, with the instantiation the slots select read from the launch counters"""
    Np, Mp = _slots(name)
    cnt = ([n for n, _ in counts], [m for _, m in counts])
    want = AF.index(SETS[name][3], tap=tap) if k else AF.index(SETS[name][2])
    with AF.watch() as w:
        got = ops.attention(qkv.to(DEV), Np, Mp, cross, topk=k, return_selection=tap, counts=cnt)
    AF.assert_launched(w, want, f'ragged {name} k={k} tap={tap}')
    return got


@pytest.mark.parametrize('cross', [False, True])
@pytest.mark.parametrize('name,k', CASES)
def test_ragged_attention_against_the_oracle_on_every_pair(name, k, cross):
    counts, qkv, ref = _reference(name, cross, k)
    Np, Mp = _slots(name)
    msg = _run(name, counts, qkv, cross, k, tap=False)
    masks = None
    if k:
        tapped, masks = _run(name, counts, qkv, cross, k, tap=True)
        masks = [t.cpu() for t in masks]
        tapped = tapped.cpu()
    msg = msg.cpu()
    assert torch.isfinite(msg).all()
    rows = near_rows = 0
    for b, (n, m) in enumerate(counts):
        # padding: the rows beyond the pair's counts are exactly 0 (their inputs are NaN)
        assert not msg[b, n:Np].any() and not msg[b, Np + m:].any(), b
        for side, (lo, c) in enumerate(((0, n), (Np, m))):
            want, keep, near = ref[b][side]
            got = msg[b, lo:lo + c].double()
            err = (got - want).abs().reshape(c, 4, 32).amax(2)                   # [c, H]
            if not k:
                print(f'{name} cross={cross} full pair {b} ({n} x {m}) side {side}: max |msg - oracle| = {err.max():.3e}')
                assert err.max() < MSG_TOL, (b, side, float(err.max()))
                continue
            nk = keep.shape[-1]
            sel = masks[side][b, :, :c]                                           # [H, c, slot keys]
            assert (sel.sum(-1) == k).all(), (b, side)                            # exactly k kept keys per row
            assert not sel[..., nk:].any(), (b, side)                             # none beyond the pair's counts
            assert not masks[side][b, :, c:].any(), (b, side)                     # no mask beyond its queries
            ok = ~near                                                            # [H, c]
            assert torch.equal(sel[..., :nk][ok], keep[ok]), (b, side)            # torch.topk's selection outside near ties
            rows += near.numel()
            near_rows += int(near.sum())
            okr = ok.permute(1, 0)                                                # [c, H]
            worst = float(err[okr].max()) if okr.any() else 0.0
            print(f'{name} cross={cross} k={k} pair {b} ({n} x {m}) side {side}: max |msg - oracle| = {worst:.3e}, near ties {int(near.sum())} of {near.numel()}')
            assert worst < MSG_TOL, (b, side, worst)
            # tap: the tapped instantiation gives the untapped one's bits; an exact tie at the k-th place (it can only be among the near
            # ties) is broken before the pass there and corrected after it here - to rounding
            a, t = msg[b, lo:lo + c].reshape(c, 4, 32), tapped[b, lo:lo + c].reshape(c, 4, 32)
            assert torch.equal(a[okr], t[okr]), (b, side)
            assert (a - t).abs().max() < 1e-6, (b, side)
        if k:
            assert not tapped[b, n:Np].any() and not tapped[b, Np + m:].any(), b
    if k:
        print(f'{name} cross={cross} k={k}: {near_rows} near-tie rows of {rows}')
        assert near_rows < NEAR_TIE_FRAC * rows


@pytest.mark.parametrize('name,k', CASES)
def test_a_pairs_rows_do_not_depend_on_its_position_or_companions(name, k):
    """Equal slots: the same bits under a permutation of the batch and in a subset that keeps the largest pair (another batch size: another
    number of workgroups per (pair, frame, head))."""
    counts = _counts(name, k)
    Np, Mp = _slots(name)
    cross = True
    base = _run(name, counts, _qkv(counts, Np, Mp, 12), cross, k, tap=False)
    perm = list(reversed(range(len(counts))))
    # the subset: the pairs that set the slots, and the first other one
    keepers = sorted({max(range(len(counts)), key=lambda b: counts[b][0]), max(range(len(counts)), key=lambda b: counts[b][1])})
    subset = keepers + [b for b in range(len(counts)) if b not in keepers][:1]
    for order in (perm, subset):
        sub = tuple(counts[b] for b in order)
        assert (max(n for n, _ in sub), max(m for _, m in sub)) == (Np, Mp)
        got = _run(name, sub, _qkv(sub, Np, Mp, 12), cross, k, tap=False)
        for i, b in enumerate(order):
            assert torch.equal(got[i], base[b]), (order, b)


def test_ragged_attention_refusals():
    """Checked on the host copies before the launch, naming the first offending pair."""
    qkv = torch.zeros(2, 40, 3, 4, 32, device=DEV)
    with pytest.raises(RuntimeError, match='mdgat_attention_ragged: pair 1: k=8 exceeds'):
        ops.attention(qkv, 20, 20, False, topk=8, counts=([20, 20], [20, 7]))
    with pytest.raises(RuntimeError, match='pair 0 has 21 x 20'):
        ops.attention(qkv, 20, 20, True, counts=([21, 20], [20, 20]))
    with pytest.raises(RuntimeError, match='at most 512 keypoints'):
        ops.attention(torch.zeros(1, 513 + 20, 3, 4, 32, device=DEV), 513, 20, False, counts=([20], [20]))
