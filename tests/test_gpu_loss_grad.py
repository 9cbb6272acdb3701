"""The gradient of the matching loss on the device: csrc/loss_grad.hip through ops.matching_loss_backward and through autograd of
ops.matching_loss.  Expected values: the reference's own dZ / dscores / dalpha (tests/golden/loss_grad.npz,
tools/make_goldens_loss_grad.py) and the numpy restatement tests/loss_grad_ref.py (pinned to the reference and to torch autograd by
tests/test_loss_grad_ref.py).

Tolerance (loss_grad_ref.tolerance), derived: 4 (n + m + 2) 2^-53 max|dZ_b| per pair - every entry of dZ is a sum of at most
max(n, m) + 2 terms of one sign pattern and each weight holds one sum of at most max(n, m) + 1 non-negative terms.  For fp32 Z the
yardstick runs on the same rounded Z and the output's own fp32 rounding (2^-24 |dZ|) is added.  The kernel evaluates t(z) as -z where
exp(z) is normal and the yardstick literally, so a clamp argument within an ulp of 0 could be taken differently: every test counts the
yardstick's clamp arguments within 1e-9 of zero (and, for triplet, tied top entries) on its seeded inputs and asserts there are none."""
import os

import numpy as np
import pytest
import torch

from loss_grad_ref import clamp_margin, golden_dloss, pair_grads, tolerance, triplet_top_gap
from loss_ref import GT_PATTERNS, gt_batch
from sinkhorn_grad_ref import max_rel

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
METHODS = ('superglue', 'triplet_loss', 'gap_loss')


@pytest.fixture(scope='module')
def g(golden_dir):
    return np.load(os.path.join(golden_dir, 'loss_grad.npz'))


def _ops():
    from mdgat_matcher_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _backward(Z, g0, g1, meth, gamma, dloss):
    return _ops().matching_loss_backward(_dev(Z), _dev(g0), _dev(g1), meth, gamma, _dev(np.asarray(dloss, dtype=np.float64))).cpu().numpy()


def _assert_close(got, want, n, m, what, planted=False, out_eps=0.0):
    """Per pair within ``tolerance`` (+ out_eps |want| for an output rounded to fp32); planted: where ``want`` is finite, with
    identical isfinite masks.  Prints the worst |difference| / tolerance."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    worst = 0.0
    for b in range(want.shape[0]):
        fin = np.isfinite(want[b])
        if planted:
            np.testing.assert_array_equal(np.isfinite(got[b]), fin, err_msg=f'{what} pair {b}: isfinite')
        else:
            assert fin.all(), (what, b)
            assert np.isfinite(got[b]).all(), (what, b)
        tol = tolerance(n, m, want[b])
        err = np.abs(got[b][fin] - want[b][fin]) - out_eps * np.abs(want[b][fin])
        e = float(err.max(initial=0.0))
        worst = max(worst, e / tol if tol else (0.0 if e <= 0 else np.inf))
        assert e <= tol, f'{what} pair {b}: |diff| {e:.3e} > {tol:.3e}'
    print(f'{what}: {worst:.3f} of the tolerance', end='; ')


def _clear_of_choices(Z, g0, g1, meth, gamma=0.5):
    cm = clamp_margin(Z, g0, g1, meth, gamma)
    assert cm >= 1e-9, f'{meth}: a clamp argument of the seeded input lies within {cm:.3e} of zero'
    if meth == 'triplet_loss':
        tg = triplet_top_gap(Z, g0, g1)
        assert tg >= 1e-9, f'the two largest non-positive entries of a row / column of the seeded input are {tg:.3e} apart'


# ------------------------------------------------------------------------------------------------ 4: it is differentiable at all
@pytest.mark.parametrize('meth', METHODS)
def test_matching_loss_carries_a_grad_fn(g, meth):
    ops = _ops()
    Z = _dev(g['n64_Z']).requires_grad_()
    loss = ops.matching_loss(Z, _dev(g['n64_gt0']), _dev(g['n64_gt1']), meth, 0.5)
    assert loss.requires_grad and loss.grad_fn is not None
    assert loss.dtype == torch.float64 and tuple(loss.shape) == (2,)
    loss.mean().backward()
    assert Z.grad is not None and Z.grad.shape == Z.shape and Z.grad.dtype == Z.dtype
    assert torch.isfinite(Z.grad).all() and Z.grad.abs().max() > 0
    want = pair_grads(g['n64_Z'], g['n64_gt0'], g['n64_gt1'], meth, 0.5, np.full(2, 0.5))
    _assert_close(Z.grad.cpu().numpy(), want, 64, 64, f'autograd {meth}')


# ------------------------------------------------------------------------------------------------ 5 / 6: the reference's own dZ
@pytest.mark.parametrize('case', ['n64', 'n48m64', 'planted_sub', 'planted_inf'])
def test_kernel_reproduces_the_references_gradient(g, case):
    B, n, m = [int(x) for x in g[f'{case}_meta']]
    planted = case.startswith('planted')
    Z, g0, g1, gamma = g[f'{case}_Z'], g[f'{case}_gt0'], g[f'{case}_gt1'], float(g[f'{case}_gamma'])
    for meth in METHODS:
        if f'{case}_{meth}_dZ' not in g.files:
            continue
        if not planted:
            _clear_of_choices(Z, g0, g1, meth, gamma)
        dloss = golden_dloss(g, case, meth)
        got = _backward(Z, g0, g1, meth, gamma, dloss)
        _assert_close(got, g[f'{case}_{meth}_dZ'], n, m, f'{case} {meth} vs reference', planted)
        _assert_close(got, pair_grads(Z, g0, g1, meth, gamma, dloss), n, m, f'{case} {meth} vs restatement', planted)
        if not planted:
            Z32 = Z.astype(np.float32)
            _clear_of_choices(Z32.astype(np.float64), g0, g1, meth, gamma)
            got32 = _backward(Z32, g0, g1, meth, gamma, dloss)
            assert got32.dtype == np.float32
            _assert_close(got32, pair_grads(Z32.astype(np.float64), g0, g1, meth, gamma, dloss), n, m, f'{case} {meth} fp32', out_eps=2.0 ** -24)
    print()


# ------------------------------------------------------------------------------------------------ 5: the shapes it runs at
def _lp_Z(B, n, m, seed):
    """log-probabilities as the module's Z: the fp64 oracle's Sinkhorn of random scores (spread +-15, bin score 0, 20 iterations), on
    the CPU so that the seeded input - and with it the count of near-zero clamp arguments - does not depend on the device."""
    from oracle import mdgat_oracle as O
    gen = torch.Generator().manual_seed(seed)
    s = (torch.rand(B, n, m, generator=gen, dtype=torch.float64) * 2 - 1) * 15
    return O.log_optimal_transport(s, torch.tensor(0.0, dtype=torch.float64), 20).numpy()


def _check_shape(names, n, m, seed, methods):
    B = len(names)
    g0, g1 = gt_batch(names, n, m, seed=seed)
    Z = _lp_Z(B, n, m, seed)
    dloss = np.round(np.random.RandomState(seed).uniform(0.5, 2.0, B) * 256) / 256
    for meth in methods:
        for f32 in (False, True):
            # fp32 values are multiples of 2^-24 or coarser and so is gamma = 0.5: among millions of clamp arguments some are exactly 0.
            # The rounded Z is run with gamma = 0.3, which no such difference meets; the assertion below shows it.
            gamma = 0.3 if f32 else 0.5
            Zx = Z.astype(np.float32) if f32 else Z
            Z64 = Zx.astype(np.float64)
            _clear_of_choices(Z64, g0, g1, meth, gamma)
            got = _backward(Zx, g0, g1, meth, gamma, dloss)
            assert got.dtype == Zx.dtype
            want = pair_grads(Z64, g0, g1, meth, gamma, dloss)
            assert min(n, m) == 1 or all(np.abs(want[b]).max() > 0 for b in range(B))       # (one keypoint: every term may be inactive)
            _assert_close(got, want, n, m, f'{meth} {n}x{m} {"fp32" if f32 else "fp64"}', out_eps=2.0 ** -24 if f32 else 0.0)
    print()


@pytest.mark.parametrize('n', [1, 64, 257])
def test_kernel_square_frames(n):
    _check_shape(GT_PATTERNS, n, n, 7000 + n, METHODS)


@pytest.mark.parametrize('n,m', [(17, 33), (33, 17), (48, 64), (1, 5)])
def test_kernel_ragged_frames_gap(n, m):
    _check_shape(GT_PATTERNS, n, m, 7000 + 100 * n + m, ('gap_loss',))


def test_kernel_64_pairs_of_512():
    """BASELINE configs[1]'s shape; the gt patterns in turn."""
    _check_shape([GT_PATTERNS[b % len(GT_PATTERNS)] for b in range(64)], 512, 512, 7512, METHODS)


@pytest.mark.parametrize('names', [('partial', 'reversed'), ('all_dustbin', 'non_injective'), ('explicit_dustbin', 'partial')])
def test_kernel_2_pairs_of_2048(names):
    _check_shape(names, 2048, 2048, 9048 + GT_PATTERNS.index(names[0]), METHODS)


# ------------------------------------------------------------------------------------------------ 7: determinism
@pytest.mark.parametrize('meth', METHODS)
def test_a_pairs_gradient_does_not_depend_on_its_batch(meth):
    ops = _ops()
    n = 200
    names = [GT_PATTERNS[b % len(GT_PATTERNS)] for b in range(64)]
    g0, g1 = gt_batch(names, n, n, seed=37)
    gen = torch.Generator().manual_seed(37)
    Z = (-8 * torch.rand(64, n + 1, n + 1, generator=gen, dtype=torch.float64)).to(DEV)
    d = torch.rand(64, generator=gen, dtype=torch.float64).to(DEV) + 0.5
    t0, t1 = _dev(g0), _dev(g1)
    full = ops.matching_loss_backward(Z, t0, t1, meth, 0.5, d)
    alone = ops.matching_loss_backward(Z[37:38], t0[37:38], t1[37:38], meth, 0.5, d[37:38])
    assert torch.equal(alone[0], full[37])
    # the other pairs carry other weights, other gts and other Z
    d2 = d * 3
    d2[37] = d[37]
    t0b, t1b = t0.roll(1, 1).clone(), t1.roll(3, 1).clone()
    t0b[37], t1b[37] = t0[37], t1[37]
    Z2 = Z.flip(2).clone()
    Z2[37] = Z[37]
    other = ops.matching_loss_backward(Z2, t0b, t1b, meth, 0.5, d2)
    assert torch.equal(other[37], full[37])
    assert torch.equal(ops.matching_loss_backward(Z, t0, t1, meth, 0.5, d), full)


# ------------------------------------------------------------------------------------------------ 8: the forward is untouched
def _raw_loss(Z, g0, g1, meth):
    from mdgat_matcher_amd import _lib
    lib = _lib.load()
    B, N, M = Z.shape[0], Z.shape[1] - 1, Z.shape[2] - 1
    loss = torch.empty(B, dtype=torch.float64, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    need = lib.mdgat_loss_workspace_bytes(B, N, M)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    off = (-ws.data_ptr()) % 256
    fn = lib.mdgat_loss_f64 if Z.dtype == torch.float64 else lib.mdgat_loss
    _lib.check(fn(B, N, M, Z.data_ptr(), g0.data_ptr(), g1.data_ptr(), _lib.LOSS_METHODS[meth], 0.5, loss.data_ptr(), bad.data_ptr(),
                  ws.data_ptr() + off, need, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    return loss


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_forward_values_are_the_raw_abis(g, dtype):
    ops = _ops()
    for case in ('n64', 'n48m64'):
        Z = _dev(g[f'{case}_Z']).to(dtype)
        g0, g1 = _dev(g[f'{case}_gt0']).long(), _dev(g[f'{case}_gt1']).long()
        for meth in METHODS:
            if f'{case}_{meth}_dZ' not in g.files:
                continue
            raw = _raw_loss(Z, g0, g1, meth)
            with torch.no_grad():
                a = ops.matching_loss(Z.clone().requires_grad_(), g0, g1, meth, 0.5)
            b = ops.matching_loss(Z, g0, g1, meth, 0.5)
            c = ops.matching_loss(Z.clone().requires_grad_(), g0, g1, meth, 0.5)
            assert a.grad_fn is None and b.grad_fn is None and c.grad_fn is not None
            for v in (a, b, c):
                assert v.dtype == torch.float64 and torch.equal(v.detach(), raw)


# ------------------------------------------------------------------------------------------------ 9: scores -> Z -> loss -> backward
@pytest.mark.parametrize('case', ['n64', 'n48m64'])
def test_composition_reproduces_the_references_score_gradients(g, case):
    """Tolerance: what tests/test_gpu_sinkhorn_grad.py asserts for the fp64 Sinkhorn backward against the reference at T up to 100 and
    a spread of +-100: 1e-8 of max|g| for dscores, 1e-8 relative for dalpha (here T = 20)."""
    ops = _ops()
    B = int(g[f'{case}_meta'][0])
    for meth in METHODS:
        if f'{case}_{meth}_dscores' not in g.files:
            continue
        s = _dev(g[f'{case}_scores']).requires_grad_()
        al = torch.tensor(float(g[f'{case}_alpha']), dtype=torch.float64, device=DEV, requires_grad=True)
        Z = ops.log_optimal_transport(s, al, int(g[f'{case}_iters']))
        loss = ops.matching_loss(Z, _dev(g[f'{case}_gt0']), _dev(g[f'{case}_gt1']), meth, float(g[f'{case}_gamma']))
        w = _dev(np.asarray(g[f'{case}_{meth}_w'], dtype=np.float64))
        ((loss * w).sum() if meth == 'gap_loss' else loss.mean() * w).backward()
        e_s = max_rel(s.grad.cpu(), torch.from_numpy(g[f'{case}_{meth}_dscores']))
        ref_da = float(g[f'{case}_{meth}_dalpha'])
        e_a = abs(float(al.grad) - ref_da) / abs(ref_da)
        print(f'{case} {meth}: dscores {e_s:.2e} of max|g|, dalpha {e_a:.2e}', end='; ')
        assert e_s < 1e-8 and e_a < 1e-8, (meth, e_s, e_a)
    print()


# ------------------------------------------------------------------------------------------------ 10: error paths
def test_error_paths(g):
    ops = _ops()
    Z = _dev(g['n64_Z']).requires_grad_()
    g0, g1 = _dev(g['n64_gt0']).long(), _dev(g['n64_gt1']).long()
    bad0 = g0.clone()
    bad0[1, 5] = 65
    for meth in METHODS:
        with pytest.raises(IndexError):
            ops.matching_loss(Z, bad0, g1, meth)
        with pytest.raises(IndexError):
            ops.matching_loss_backward(Z.detach(), bad0, g1, meth, 0.5, torch.ones(2, dtype=torch.float64, device=DEV))
    Zr = _dev(g['n48m64_Z']).requires_grad_()
    r0, r1 = _dev(g['n48m64_gt0']), _dev(g['n48m64_gt1'])
    for meth in ('superglue', 'triplet_loss'):
        with pytest.raises(ValueError):
            ops.matching_loss(Zr, r0, r1, meth)
        with pytest.raises(ValueError):
            ops.matching_loss_backward(Zr.detach(), r0, r1, meth, 0.5, torch.ones(2, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        ops.matching_loss_backward(Z.detach(), g0, g1, 'gap_loss', 0.5, torch.ones(3, dtype=torch.float64, device=DEV))
    loss = ops.matching_loss(Z, g0, g1, 'gap_loss')
    gz, = torch.autograd.grad(loss.sum(), Z, create_graph=True)
    with pytest.raises(RuntimeError):
        gz.sum().backward()


def test_bad_pair_is_nan_and_raw_abi_refuses_bad_arguments(g):
    """Through the raw ABI: a bad gt index poisons its own pair only and sets the bad word; bad arguments are refused with a message."""
    from mdgat_matcher_amd import _lib
    lib = _lib.load()
    Z = _dev(g['n64_Z'])
    g0, g1 = _dev(g['n64_gt0']).long(), _dev(g['n64_gt1']).long()
    g1[1, 3] = -2
    B, N, M = 2, 64, 64
    d = torch.ones(B, dtype=torch.float64, device=DEV)
    dZ = torch.zeros_like(Z)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    need = lib.mdgat_loss_backward_workspace_bytes(B, N, M)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    off = (-ws.data_ptr()) % 256
    st = torch.cuda.current_stream().cuda_stream
    args = lambda meth, wsp, nbytes: (B, N, M, Z.data_ptr(), g0.data_ptr(), g1.data_ptr(), meth, 0.5, d.data_ptr(), dZ.data_ptr(),     # noqa: E731
                                      bad.data_ptr(), wsp, nbytes, st)
    assert lib.mdgat_loss_backward_f64(*args(_lib.LOSS_GAP, ws.data_ptr() + off, need)) == _lib.OK
    torch.cuda.synchronize()
    assert int(bad.item()) == 1 and torch.isnan(dZ[1]).all() and torch.isfinite(dZ[0]).all()
    bad.zero_()
    assert lib.mdgat_loss_backward_f64(*args(_lib.LOSS_SUPERGLUE, ws.data_ptr() + off, need)) == _lib.OK      # superglue reads gt1 through == -1 alone
    torch.cuda.synchronize()
    assert int(bad.item()) == 0 and torch.isfinite(dZ).all()
    assert lib.mdgat_loss_backward_f64(*args(_lib.LOSS_GAP, ws.data_ptr() + off, need - 1)) == _lib.ERR_BAD_ARG
    assert 'workspace' in _lib.last_error()
    assert lib.mdgat_loss_backward_f64(*args(_lib.LOSS_GAP, ws.data_ptr() + off + 8, need)) == _lib.ERR_BAD_ARG
    assert lib.mdgat_loss_backward_f64(*args(7, ws.data_ptr() + off, need)) == _lib.ERR_BAD_ARG
    assert lib.mdgat_loss_backward_f64(B, N, M, None, g0.data_ptr(), g1.data_ptr(), _lib.LOSS_GAP, 0.5, d.data_ptr(), dZ.data_ptr(), bad.data_ptr(),
                                       ws.data_ptr() + off, need, st) == _lib.ERR_BAD_ARG
    assert lib.mdgat_loss_backward_f64(B, N, M + 1, Z.data_ptr(), g0.data_ptr(), g1.data_ptr(), _lib.LOSS_TRIPLET, 0.5, d.data_ptr(), dZ.data_ptr(),
                                       bad.data_ptr(), ws.data_ptr() + off, need, st) == _lib.ERR_BAD_ARG
