"""tests/attention_grad_ref.py - the numpy restatement of the fp64 attention's gradient and its derived error bound - against the
reference's own gradients (tests/golden/attention_grad_*.npz, tools/make_goldens_attention_grad.py) and against torch autograd
through the oracle's attention / dynamic_attention on further seeded shapes.  CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attention_grad_ref as R
from oracle import mdgat_oracle as O

CASE_NAMES = [c[0] for c in R.CASES]


def random_inputs(B, N, M, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((B, N + M, 3, 4, 32)) * 1.3, rs.standard_normal((B, N + M, 128))


def oracle_backward(qkv, N, M, cross, dmsg, k):
    """(message, dqkv, masks) by torch autograd through the oracle's functions, frame by frame, in the library's layout."""
    B = qkv.shape[0]
    x = torch.from_numpy(qkv).clone().requires_grad_()
    fr = ((0, N), (N, N + M))
    masks, parts = [], []
    for side in range(2):
        lo, hi = fr[side]
        slo, shi = fr[1 - side] if cross else fr[side]
        q, kk, v = (x[:, a:b, i].permute(0, 3, 2, 1) for a, b, i in ((lo, hi, 0), (slo, shi, 1), (slo, shi, 2)))
        if k > 0:
            rep = []
            out, _ = O.dynamic_attention(q, kk, v, k, report=rep)
            masks.append(rep[0]['own'].numpy())
        else:
            out, _ = O.attention(q, kk, v)
        parts.append((lo, hi, out.permute(0, 3, 2, 1).reshape(B, hi - lo, 128)))
    msg = torch.cat([p[2] for p in parts], dim=1)
    (msg * torch.from_numpy(dmsg)).sum().backward()
    return msg.detach().numpy(), x.grad.numpy(), tuple(masks) if k > 0 else None


@pytest.fixture(scope='module')
def goldens(golden_dir):
    return {c: R.load_golden(golden_dir, c) for c in CASE_NAMES}


def _args(g):
    B, N, M, cross, k = (int(v) for v in g['meta'])
    return (g['qkv'], N, M, bool(cross)), k


def test_fixture_holds_every_case(goldens):
    for (case, B, N, M, cross, k) in R.CASES:
        g = goldens[case]
        assert tuple(int(v) for v in g['meta']) == (B, N, M, int(cross), k)
        assert g['qkv'].shape == (B, N + M, 3, 4, 32) and g['dqkv'].shape == g['qkv'].shape
        assert g['dmsg'].shape == (B, N + M, 128) and g['msg'].shape == g['dmsg'].shape
        assert all(np.isfinite(g[n]).all() for n in ('qkv', 'dmsg', 'msg', 'dqkv'))
        if k > 0:
            assert all((m.sum(axis=-1) == k).all() for m in g['masks'])
            own, gap = R.topk_masks(g['qkv'], N, M, cross, k)
            assert gap >= 1e-9 and all(np.array_equal(a, b) for a, b in zip(own, g['masks']))
    assert {c[4] for c in R.CASES} == {False, True} and {c[5] for c in R.CASES} == {0, 1, 16}


@pytest.mark.parametrize('case', CASE_NAMES)
def test_backward_restates_the_references_gradients(goldens, case):
    g = goldens[case]
    a, k = _args(g)
    assert np.abs(R.forward(*a, g['masks']) - g['msg']).max() < 1e-13
    frac = R.worst_fraction(R.backward(*a, g['dmsg'], g['masks']), g['dqkv'], R.tolerances(*a, g['dmsg'], g['masks']))
    print(f'{case}: {frac:.2e} of the bound')
    assert frac <= 1.0


@pytest.mark.parametrize('B,N,M,cross,k', [(1, 1, 1, False, 0), (1, 5, 3, True, 2), (2, 17, 17, False, 16), (2, 33, 31, True, 0), (1, 64, 64, False, 63),
                                           (2, 100, 70, True, 70), (1, 130, 97, True, 8), (1, 257, 130, False, 0)])
def test_backward_is_what_autograd_takes_through_the_oracle(B, N, M, cross, k):
    qkv, dmsg = random_inputs(B, N, M, 1000 * N + 10 * M + k)
    msg, want, masks = oracle_backward(qkv, N, M, cross, dmsg, k)
    assert np.abs(R.forward(qkv, N, M, cross, masks) - msg).max() < 1e-12
    frac = R.worst_fraction(R.backward(qkv, N, M, cross, dmsg, masks), want, R.tolerances(qkv, N, M, cross, dmsg, masks))
    print(f'{frac:.2e} of the bound')
    assert frac <= 1.0


@pytest.mark.parametrize('case', ['dyn_self_n48_k16', 'dyn_cross_n40m56_k16', 'dyn_cross_b2_n20m28_k16'])
def test_the_bound_notices_one_swapped_key(goldens, case):
    """One kept key of one row swapped for the row's best key that was not kept: more than 100 x the tolerance away somewhere."""
    g = goldens[case]
    a, k = _args(g)
    qkv, N, M, cross = a
    masks = [m.copy() for m in g['masks']]
    side, b, h, row = 1, 0, 2, 3
    qs, ks = R._sides(N, M, cross)[side]
    S = R.SCALE * (qkv[b, qs, 0, h][row] @ qkv[b, ks, 1, h].T)
    kept = masks[side][b, h, row]
    worst_kept = np.where(kept, S, np.inf).argmin()
    best_other = np.where(kept, -np.inf, S).argmax()
    masks[side][b, h, row, worst_kept], masks[side][b, h, row, best_other] = False, True
    assert masks[side][b, h, row].sum() == k
    frac = R.worst_fraction(R.backward(*a, g['dmsg'], tuple(masks)), g['dqkv'], R.tolerances(*a, g['dmsg'], g['masks']))
    print(f'{case}: a swapped key is {frac:.2e} of the bound')
    assert frac > 100.0


@pytest.mark.parametrize('case', CASE_NAMES)
def test_the_bound_notices_a_relative_error_of_1e_6(goldens, case):
    g = goldens[case]
    a, k = _args(g)
    frac = R.worst_fraction(g['dqkv'] * (1.0 + 1e-6), g['dqkv'], R.tolerances(*a, g['dmsg'], g['masks']))
    assert frac > 1.0, frac


@pytest.mark.parametrize('case', ['dyn_self_n48_k1', 'dyn_cross_n40m56_k1'])
def test_one_kept_key_has_no_gradient_through_the_softmax(goldens, case):
    """k = 1: a one-element softmax is constant - dq is 0 (within the bound), and dk / dv rows of keys no query kept are exactly 0.0."""
    g = goldens[case]
    a, k = _args(g)
    qkv, N, M, cross = a
    tol = R.tolerances(*a, g['dmsg'], g['masks'])
    for d in (R.backward(*a, g['dmsg'], g['masks']), g['dqkv']):
        assert (np.abs(d[:, :, 0]) <= tol[:, :, 0]).all()
        seen = 0
        for (qs, ks), mask in zip(R._sides(N, M, cross), g['masks']):
            unkept = ~mask.any(axis=2)                       # [B, 4, keys]
            rows = np.transpose(d[:, ks, 1:], (0, 3, 1, 2, 4))   # [B, 4, keys, 2, 32]
            assert (rows[unkept] == 0.0).all()
            seen += int(unkept.sum())
        assert seen > 0
    assert np.abs(g['dqkv'][:, :, 2]).max() > 0


def test_tolerance_arithmetic_and_worst_fraction():
    qkv, dmsg = random_inputs(1, 9, 7, 5)
    tol = R.tolerances(qkv, 9, 7, True, dmsg)
    assert tol.shape == qkv.shape and (tol > 0).all()
    # twice the upstream gradient: twice the gradient, twice the bound
    assert np.allclose(R.tolerances(qkv, 9, 7, True, 2 * dmsg), 2 * tol, rtol=1e-12)
    assert np.allclose(R.backward(qkv, 9, 7, True, 2 * dmsg), 2 * R.backward(qkv, 9, 7, True, dmsg), rtol=1e-12, atol=0)
    # the closing products: dv's bound is (P (rel + nq u))^T |G| - at least 4 nq u |dv| (frame 0's rows: read by frame 1's 7 queries)
    Ps = R.probabilities(qkv, 9, 7, True)
    assert (tol[:, :, 2] >= 4 * 7 * R.U * np.abs(R.backward(qkv, 9, 7, True, dmsg))[:, :, 2] * (1 - 1e-12))[:, :9].all() and len(Ps) == 2
    assert R.worst_fraction(np.ones(3), np.ones(3), np.zeros(3)) == 0.0 and R.worst_fraction(np.ones(3), np.zeros(3), np.zeros(3)) == np.inf



# ---- the attention inside the reference's MultiHeadedAttention.forward: the channel convention and the convolutions around it ----
def test_composition_restates_the_references_multi_headed_attention(golden_dir):
    """The 1x1 convolutions composed in numpy around the restatement, channels permuted from the reference's dim * 4 + head to the
    library's head * 32 + dim: the module's output and all ten recorded gradients."""
    g = R.load_mha(golden_dir)
    a = (g['x'], g['source'], g['w'])
    assert g['k'] == 8 and g['x'].shape == (1, 40, 128) and g['source'].shape == (1, 56, 128)
    assert np.abs(R.mha_forward(*a, g['masks']) - g['out']).max() < 1e-12
    got, tol = R.mha_backward(*a, g['dout'], g['masks']), R.mha_tolerances(*a, g['dout'], g['masks'])
    for name in R.MHA_GRADS:
        frac = R.worst_fraction(got[name], g[name], tol[name])
        print(f'{name}: {frac:.2e} of the bound', end='; ')
        assert frac <= 1.0, (name, frac)
        assert np.abs(g[name]).max() > 0


def test_composition_notices_the_wrong_channel_convention(golden_dir, monkeypatch):
    """Only the permutation is varied - head * 32 + dim taken for the reference's own order, the recorded selection kept: the gradients
    leave the bound by orders of magnitude (with the right permutation the same call is inside it: the test above)."""
    g = R.load_mha(golden_dir)
    a = (g['x'], g['source'], g['w'])
    tol = R.mha_tolerances(*a, g['dout'], g['masks'])
    monkeypatch.setattr(R, 'PERM', np.arange(128))
    got = R.mha_backward(*a, g['dout'], g['masks'])
    assert min(R.worst_fraction(got[name], g[name], tol[name]) for name in ('dx', 'dsource', 'dWq', 'dWk', 'dWv', 'dWm')) > 100.0


def test_generator_check_reproduces_the_committed_files():
    """tools/make_goldens_attention_grad.py --check: the committed fixtures are what the reference computes.  Runs where the reference
    is (tools/make_goldens.py: REF); elsewhere there is nothing to compare against."""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
    sys.path.insert(0, tools)
    try:
        import make_goldens
    finally:
        sys.path.remove(tools)
    if not os.path.isfile(os.path.join(make_goldens.REF, 'models', 'mdgat.py')):
        pytest.skip('the reference is not on this machine')
    r = subprocess.run([sys.executable, os.path.join(tools, 'make_goldens_attention_grad.py'), '--check'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'OK' in r.stdout.splitlines()[-1]
