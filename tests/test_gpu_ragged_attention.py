"""Ragged batches through the fp64 attention kernels (ops.attention_f64 with counts=): pairs of different sizes in padded slots of one
launch, every instantiation - full attention in its split-key and one-wave-per-query-block forms, dynamic attention up to and beyond
512 keys, with the selection tap.  The yardstick is the pair run ALONE through the same op."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mdgat_matcher_amd import _lib, ops  # noqa: E402

DEV = 'cuda:0'
F64_TOL = 1e-11         # as tests/test_gpu_f64.py: fp64 kernels that differ in summation order only
SET_A = ((40, 33), (17, 64), (64, 17), (65, 48), (8, 8), (31, 32), (33, 97))          # 16-key blocks, 16 / 32-query tiles straddled
SET_B = ((530, 100), (100, 540), (575, 575), (64, 64))                                # the dynamic kernel beyond 512 keys
SETS = {'A': (SET_A, 8), 'B': (SET_B, 16)}


def _qkv(counts, fill, seed):
    """[B, Np + Mp, 3, 4, 32]: pair b's frames at rows 0 .. N_b and Np .. Np + M_b, `fill` everywhere else"""
    Np, Mp = max(n for n, _ in counts), max(m for _, m in counts)
    rs = np.random.RandomState(seed)
    x = np.full((len(counts), Np + Mp, 3, 4, 32), fill)
    for b, (n, m) in enumerate(counts):
        x[b, :n] = rs.standard_normal((n, 3, 4, 32)) * 1.3
        x[b, Np:Np + m] = rs.standard_normal((m, 3, 4, 32)) * 1.3
    return torch.from_numpy(x), Np, Mp


@pytest.mark.parametrize('kind', ['full0', 'full1', 'dynamic'])
@pytest.mark.parametrize('cross', [False, True])
@pytest.mark.parametrize('name', ['A', 'B'])
def test_ragged_attention_equals_every_pair_alone(name, cross, kind):
    """Pair b's message rows against ops.attention_f64 on pair b alone: the same bits wherever both launches run the same instantiation -
    full attention under either forced form; dynamic attention when the larger frame of the pair and of the batch are on the same side of
    512 keys and k is below the pair's counts (alone, k = N_b = M_b is full attention and runs the full-attention kernel) - and within
    1e-11 otherwise.  The kept keys are the same in every case; rows and masks beyond a pair's counts are zero; what the padding holds
    (zeros, NaN, 1e300) changes no bit."""
    counts, k = SETS[name]
    topk = k if kind == 'dynamic' else 0
    lib = _lib.load()
    qkv, Np, Mp = _qkv(counts, 0.0, 11 + cross)
    cnt = ([n for n, _ in counts], [m for _, m in counts])
    prev = lib.mdgat_set_f64_attention_form(1 if kind == 'full1' else 0)
    try:
        got = ops.attention_f64(qkv.to(DEV), Np, Mp, cross, topk=topk, return_selection=topk > 0, counts=cnt)
        msg, masks = got if topk else (got, None)
        for fill in (float('nan'), 1e300):
            again = ops.attention_f64(_qkv(counts, fill, 11 + cross)[0].to(DEV), Np, Mp, cross, topk=topk, return_selection=topk > 0, counts=cnt)
            assert torch.equal(again[0] if topk else again, msg), fill
            assert not topk or all(torch.equal(a, b) for a, b in zip(again[1], masks)), fill
        for b, (n, m) in enumerate(counts):
            x = torch.cat([qkv[b:b + 1, :n], qkv[b:b + 1, Np:Np + m]], 1).to(DEV)
            ref = ops.attention_f64(x, n, m, cross, topk=topk, return_selection=topk > 0)
            rmsg, rmasks = ref if topk else (ref, None)
            mine = torch.cat([msg[b:b + 1, :n], msg[b:b + 1, Np:Np + m]], 1)
            err = (mine - rmsg).abs().max().item()
            same = not topk or ((max(n, m) <= 512) == (max(Np, Mp) <= 512) and not (k == n and k == m))
            print(f'{name} cross={cross} {kind} pair {b} ({n} x {m}): max |ragged - alone| = {err:.3e} (same instantiation: {same})')
            assert torch.equal(mine, rmsg) if same else err < F64_TOL, (b, err)
            assert not msg[b, n:Np].any() and not msg[b, Np + m:].any(), b
            if topk:
                nk = (m, n) if cross else (n, m)
                assert torch.equal(masks[0][b, :, :n, :nk[0]], rmasks[0][0]) and torch.equal(masks[1][b, :, :m, :nk[1]], rmasks[1][0]), b
                for side, c in enumerate((n, m)):
                    rest = masks[side][b].clone()
                    rest[:, :c, :nk[side]] = False
                    assert not rest.any(), (b, side)
    finally:
        lib.mdgat_set_f64_attention_form(prev)


def test_ragged_attention_refusals():
    """Checked on the host copies before the launch, naming the first offending pair; no gradient through a ragged launch."""
    qkv = torch.zeros(2, 40, 3, 4, 32, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match='pair 1: k=8 exceeds'):
        ops.attention_f64(qkv, 20, 20, False, topk=8, counts=([20, 20], [20, 7]))
    with pytest.raises(RuntimeError, match='pair 0 has 21 x 20'):
        ops.attention_f64(qkv, 20, 20, True, counts=([21, 20], [20, 20]))
    with pytest.raises(RuntimeError, match='pair 1 has 20 x 0'):
        ops.attention_f64(qkv, 20, 20, True, counts=([20, 20], [20, 0]))
    with pytest.raises(RuntimeError, match='forward only'):
        ops.attention_f64(qkv.clone().requires_grad_(), 20, 20, False, counts=([20, 20], [20, 20]))
