"""csrc/attention_grad.hip where tests/test_gpu_attention_grad.py does not take it: logits up to |S| = 205 with a lazy softmax
reference that moves in most key blocks, selections that no forward wrote, frames of one point, and the invariances that hold bit for
bit.  The inputs, and the conditions they meet (how far the logits reach, that the reference of walk 1 does move - lazy_trace -, that
the restatement agrees with np.longdouble within half the bound), are in tests/attention_grad_ref.py and asserted on the CPU by
tests/test_attention_grad_ref.py.

Expected values and tolerance as in tests/test_gpu_attention_grad.py, whose helpers these tests use: the numpy restatement
R.backward within R.tolerances, every entry compared, none excluded, the worst fraction of the bound printed.

Measured on an MI355X (worst fraction of the bound per family): see DESIGN section 7.5."""
import numpy as np
import pytest
import torch

import attention_grad_ref as R
from test_gpu_attention_grad import _assert_within, _dev, _forward_selection, _ops

pytestmark = pytest.mark.gpu


def _name(B, N, M, cross):
    return f'{B}x{N}x{M}-{"cross" if cross else "self"}'


def _words(masks, B, N, M, cross, pad=0):
    return _dev(R.masks_to_words(masks, B, N, M, cross, pad).reshape(-1))


def _backward(qkv, N, M, cross, dmsg, topk=0, sel=None):
    return _ops().attention_f64_backward(_dev(qkv), N, M, cross, _dev(dmsg), topk, sel)


def _against_restatement(qkv, N, M, cross, dmsg, masks, got, what):
    return _assert_within(got.cpu().numpy(), R.backward(qkv, N, M, cross, dmsg, masks), R.tolerances(qkv, N, M, cross, dmsg, masks), what)


# ------------------------------------------------------------------------------------------------ (a) hard logits
@pytest.mark.parametrize('family,B,N,M,cross,k', R.LOGIT_CASES, ids=[f'{c[0]}-{_name(*c[1:5])}-k{c[5]}' for c in R.LOGIT_CASES])
def test_hard_logits_against_the_restatement(family, B, N, M, cross, k):
    """Every key, and the forward's own top-k selection (first asserted equal to the top-k of the fp64 logits); dmsg ~ N(0, 1), and the
    same with its rows scaled by 2^20 and 2^-20 in turn."""
    qkv, dmsg = R.family_inputs(family, B, N, M, cross)
    _, sel, masks = _forward_selection(_dev(qkv), N, M, cross, k)
    if k > 0:
        masks = tuple(m.cpu().numpy() for m in masks)
        own, gap = R.topk_masks(qkv, N, M, cross, k)
        for a, b in zip(masks, own):
            assert np.array_equal(a, b), f'{int((a ^ b).any(-1).sum())} rows selected unlike the top-k of the fp64 logits (gap {gap:.2e})'
    for rows, g in (('N(0,1)', dmsg), ('rows 2^+-20', R.alternate_rows(dmsg))):
        _against_restatement(qkv, N, M, cross, g, masks, _backward(qkv, N, M, cross, g, k, sel), f'{family} {_name(B, N, M, cross)} k={k} dmsg {rows}')


# ------------------------------------------------------------------------------------------------ (b) selections as inputs
@pytest.mark.parametrize('family,B,N,M,cross', R.SELECTION_CASES, ids=[f'{c[0]}-{_name(*c[1:])}' for c in R.SELECTION_CASES])
def test_selections_no_forward_wrote(family, B, N, M, cross):
    """The selection words are an input: rows that keep 0, 1, 2, nk / 2, nk - 1 and nk keys side by side, set bits where there is no
    key, the last partial key block alone, no key at all, every key."""
    qkv, dmsg = R.family_inputs(family, B, N, M, cross)
    what = f'{family} {_name(B, N, M, cross)}'
    # (i) per-row counts 0, 1, 2, nk / 2, nk - 1, nk
    masks = R.selection_masks('varied', B, N, M, cross)
    got = _backward(qkv, N, M, cross, dmsg, 1, _words(masks, B, N, M, cross))
    assert torch.isfinite(got).all()
    _against_restatement(qkv, N, M, cross, dmsg, masks, got, what + ' varied counts')
    empty_rows = 0
    for (qs, _), m in zip(R._sides(N, M, cross), masks):
        empty = ~m.any(axis=-1)                                                    # [B, 4, nq]
        assert (got[:, qs, 0].permute(0, 2, 1, 3).cpu().numpy()[empty] == 0.0).all()
        empty_rows += int(empty.sum())
    assert empty_rows > 0
    # (ii) the bits that address no key are not read
    padded = _backward(qkv, N, M, cross, dmsg, 1, _words(masks, B, N, M, cross, pad=1))
    assert torch.equal(padded, got)
    # (iii) only keys of the last, partial block
    masks = R.selection_masks('last_block', B, N, M, cross)
    for pad in (0, 1):
        _against_restatement(qkv, N, M, cross, dmsg, masks, _backward(qkv, N, M, cross, dmsg, 1, _words(masks, B, N, M, cross, pad)),
                             what + f' last block only, pad {pad}')
    # (iv) no key anywhere: exact zeros
    masks = R.selection_masks('none', B, N, M, cross)
    got = _backward(qkv, N, M, cross, dmsg, 1, _words(masks, B, N, M, cross))
    assert torch.equal(got, torch.zeros_like(got))
    # (v) every key, as a selection.  The masked kernels differ from the unmasked ones only in where a lane's keep bits come from (kept()
    # in the row pass, `keep` in the column pass); the arithmetic behind them is the same text, so the bits are those of topk = 0
    masks = R.selection_masks('all', B, N, M, cross)
    got = _backward(qkv, N, M, cross, dmsg, min(N, M), _words(masks, B, N, M, cross))
    _against_restatement(qkv, N, M, cross, dmsg, None, got, what + ' every key as a selection')
    full = _backward(qkv, N, M, cross, dmsg)
    print(f'{what}: every key as a selection gives the bits of topk = 0: {torch.equal(got, full)}')
    assert torch.equal(got, full)


# ------------------------------------------------------------------------------------------------ (c) one key, one query
@pytest.mark.parametrize('family,B,N,M,cross,k', R.SINGLE_CASES, ids=[f'{_name(*c[1:5])}-k{c[5]}' for c in R.SINGLE_CASES])
def test_frames_of_one_point(family, B, N, M, cross, k):
    """N = 1 and M = 1.  k = 1: every row keeps its best key (the top-1 of the fp64 logits, as selection words).  A row with one kept
    key has a constant softmax: its dq, and the dk of the frame its side reads, are 0 within the bound."""
    qkv, dmsg = R.family_inputs(family, B, N, M, cross)
    masks = R.topk_masks(qkv, N, M, cross, k)[0] if k > 0 else None
    got = _backward(qkv, N, M, cross, dmsg, k, _words(masks, B, N, M, cross) if k > 0 else None)
    _against_restatement(qkv, N, M, cross, dmsg, masks, got, f'{_name(B, N, M, cross)} k={k}')
    tol, got = R.tolerances(qkv, N, M, cross, dmsg, masks), got.cpu().numpy()
    seen = 0
    for (qs, ks), nk in zip(R._sides(N, M, cross), (M, N) if cross else (N, M)):
        if nk == 1 or k == 1:
            assert (np.abs(got[:, qs, 0]) <= tol[:, qs, 0]).all() and (np.abs(got[:, ks, 1]) <= tol[:, ks, 1]).all()
            seen += 1
    assert seen > 0
    assert np.abs(got[:, :, 2]).max() > 0


# ------------------------------------------------------------------------------------------------ (d) exact invariances
@pytest.mark.parametrize('family,B,N,M,cross,k', R.INVARIANCE_CASES, ids=[f'{c[0]}-{_name(*c[1:5])}-k{c[5]}' for c in R.INVARIANCE_CASES])
def test_invariances_hold_bit_for_bit(family, B, N, M, cross, k):
    """Powers of two scale every product and sum of the kernel exactly; heads and frames are units of the grid that share nothing."""
    ops = _ops()
    qkv, dmsg = R.family_inputs(family, B, N, M, cross)
    x, g = _dev(qkv), _dev(dmsg)
    _, sel, _ = _forward_selection(x, N, M, cross, k)
    run = lambda x, g, N=N, M=M, sel=sel: ops.attention_f64_backward(x, N, M, cross, g, k, sel)                      # noqa: E731
    base = run(x, g)
    assert torch.isfinite(base).all() and bool((base != 0).any())
    up, down = 2.0 ** 20, 2.0 ** -20
    # dmsg x 2^20
    assert torch.equal(run(x, g * up), base * up)
    # v x 2^-20: dq and dk scale, dv does not see v
    scaled = x.clone()
    scaled[:, :, 2] *= down
    got = run(scaled, g)
    assert torch.equal(got[:, :, :2], base[:, :, :2] * down) and torch.equal(got[:, :, 2], base[:, :, 2])
    # q x 2^7, k x 2^-7: the same logits bit for bit, so the selection words of the unscaled run stand
    scaled = x.clone()
    scaled[:, :, 0] *= 2.0 ** 7
    scaled[:, :, 1] *= 2.0 ** -7
    got = run(scaled, g)
    assert torch.equal(got[:, :, 0], base[:, :, 0] * 2.0 ** -7) and torch.equal(got[:, :, 1], base[:, :, 1] * 2.0 ** 7)
    assert torch.equal(got[:, :, 2], base[:, :, 2])
    # the four heads permuted in qkv, dmsg and the words
    perm = [2, 0, 3, 1]
    W = (max(N, M) + 31) // 32
    sel_p = sel.reshape(B, 4, N + M, W)[:, perm].contiguous().reshape(-1) if k > 0 else None
    got = run(x[:, :, :, perm].contiguous(), g.reshape(B, N + M, 4, 32)[:, :, perm].reshape(B, N + M, 128).contiguous(), sel=sel_p)
    assert torch.equal(got, base[:, :, :, perm])
    # the two frames swapped: rows, N <-> M, and the rows of the words
    swap = torch.cat([torch.arange(N, N + M), torch.arange(N)]).to(x.device)
    sel_s = sel.reshape(B, 4, N + M, W)[:, :, swap].contiguous().reshape(-1) if k > 0 else None
    got = run(x[:, swap].contiguous(), g[:, swap].contiguous(), N=M, M=N, sel=sel_s)
    assert torch.equal(got, base[:, swap])
