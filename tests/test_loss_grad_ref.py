"""The numpy restatement of the losses' gradient (tests/loss_grad_ref.py) against the reference's own dZ (tests/golden/loss_grad.npz,
tools/make_goldens_loss_grad.py) and against torch autograd of a torch transcription of tests/loss_ref.py::pair_losses.  CPU only.

Tolerance (loss_grad_ref.tolerance), derived: every entry of dZ is a sum of at most max(n, m) + 2 terms of equal sign pattern and each
weight contains one sum S of at most max(n, m) + 1 non-negative terms, so two fp64 evaluations in different summation orders differ
by at most 4 (n + m + 2) 2^-53 max|dZ_b| per pair."""
import os

import numpy as np
import pytest
import torch

from loss_grad_ref import clamp_margin, golden_dloss, pair_grads, tolerance, triplet_top_gap
from loss_ref import GT_PATTERNS, gt_batch, pair_losses, t

METHODS = ('superglue', 'triplet_loss', 'gap_loss')
CASES = ('n64', 'n48m64', 'planted_sub', 'planted_inf')


@pytest.fixture(scope='module')
def g(golden_dir):
    return np.load(os.path.join(golden_dir, 'loss_grad.npz'))


def assert_grad_close(got, want, n, m, what, planted=False):
    """Per pair within ``tolerance``; planted: only where ``want`` is finite, with identical isfinite masks."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    worst = 0.0
    for b in range(want.shape[0]):
        fin = np.isfinite(want[b])
        if planted:
            np.testing.assert_array_equal(np.isfinite(got[b]), fin, err_msg=f'{what} pair {b}: isfinite')
        else:
            assert fin.all() and np.isfinite(got[b]).all(), (what, b)
        tol = tolerance(n, m, want[b])
        err = float(np.abs(got[b][fin] - want[b][fin]).max(initial=0.0))
        worst = max(worst, err / tol if tol else (0.0 if err == 0 else np.inf))
        assert err <= tol, f'{what} pair {b}: |diff| {err:.3e} > {tol:.3e}'
    return worst


@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_the_references_gradient(g, case):
    B, n, m = [int(x) for x in g[f'{case}_meta']]
    planted = case.startswith('planted')
    seen = 0
    for meth in METHODS:
        if f'{case}_{meth}_dZ' not in g.files:
            continue
        seen += 1
        want = g[f'{case}_{meth}_dZ']
        got = pair_grads(g[f'{case}_Z'], g[f'{case}_gt0'], g[f'{case}_gt1'], meth, float(g[f'{case}_gamma']), golden_dloss(g, case, meth))
        worst = assert_grad_close(got, want, n, m, f'{case} {meth}', planted)
        print(f'{case} {meth}: worst |diff| / tolerance {worst:.3f}, non-finite {int((~np.isfinite(want)).sum())}')
        assert np.abs(want[np.isfinite(want)]).max() > 0
        if planted and meth != 'superglue':
            assert (~np.isfinite(want)).any()               # the planted entries reach the literal t's non-finite gradients
    assert seen == (1 if case == 'n48m64' else 3)


def test_goldens_keep_clear_of_discrete_choices(g):
    for case in ('n64', 'n48m64'):
        for meth in METHODS:
            if f'{case}_{meth}_dZ' in g.files:
                assert clamp_margin(g[f'{case}_Z'], g[f'{case}_gt0'], g[f'{case}_gt1'], meth, float(g[f'{case}_gamma'])) >= 1e-9
        if case == 'n64':
            assert triplet_top_gap(g[f'{case}_Z'], g[f'{case}_gt0'], g[f'{case}_gt1']) >= 1e-9


# ---- torch autograd of a transcription of loss_ref.pair_losses -------------------------------------------------------------------
def torch_pair_losses(Z, gt0, gt1, method, gamma=0.5):
    """tests/loss_ref.py::pair_losses in torch, line for line, so that autograd differentiates it (on Z's device; tools/loss_grad_time.py
    times it there)."""
    dev = Z.device
    tt = lambda z: -torch.log(torch.exp(z))         # noqa: E731
    B, n, m = Z.shape[0], Z.shape[1] - 1, Z.shape[2] - 1
    out = []
    for b in range(B):
        z = Z[b]
        g1 = torch.as_tensor(gt1[b]).to(device=dev, dtype=torch.int64)
        g0 = torch.as_tensor(gt0[b]).to(device=dev, dtype=torch.int64)
        p0, p1 = torch.where(g0 == -1, m, g0), torch.where(g1 == -1, n, g1)
        rows, cols = torch.arange(n, device=dev), torch.arange(m, device=dev)
        pos_r, pos_c = z[rows, p0], z[p1, cols]
        if method == 'superglue':
            un = g1 == -1
            out.append((-pos_r.sum() - z[n, cols[un]].sum()) / (un.sum() + m))
            continue
        keep_r = torch.ones((n, m + 1), dtype=torch.bool, device=dev)
        keep_r[rows, p0] = False
        keep_c = torch.ones((n + 1, m), dtype=torch.bool, device=dev)
        keep_c[p1, cols] = False
        ninf = torch.tensor(-np.inf, dtype=z.dtype, device=dev)
        if method == 'triplet_loss':
            neg_r = torch.where(keep_r, z[:n, :], ninf).max(dim=1).values
            neg_c = torch.where(keep_c, z[:, :m], ninf).max(dim=0).values
            terms = torch.cat([torch.clamp(tt(pos_r) - tt(neg_r) + gamma, min=0), torch.clamp(tt(pos_c) - tt(neg_c) + gamma, min=0)])
            out.append(terms.mean())
        else:
            tz = tt(z)
            zero = torch.zeros((), dtype=z.dtype, device=dev)
            row = torch.where(keep_r, torch.clamp(tt(pos_r)[:, None] - tz[:n, :] + gamma, min=0), zero).sum(dim=1)
            P = tz[:, :m][~keep_c]
            V = tz[:, :m][keep_c].reshape(n, m)
            col = torch.clamp(P[None, :] - V + gamma, min=0).sum(dim=0)
            out.append((torch.mean(2 * torch.log(row + 1)) + torch.mean(2 * torch.log(col + 1))) / 2)
    return torch.stack(out)


def grid_Z(B, n, m, rs):
    """Z on the grid 2^-8 in [-8, 0]: with gamma = 0.5 the clamp arguments are differences of grid values wherever t(z) = -z exactly."""
    return -rs.randint(0, 8 * 256 + 1, (B, n + 1, m + 1)) / 256.0


def test_t_agrees_with_torch_on_the_grid():
    """The precondition of the comparison with autograd: numpy and torch evaluate t(z) = -log(exp(z)) to the same bits on every grid
    value, so both sides see the same clamp arguments and take the same discrete decisions (>= 0, arg-max)."""
    z = -np.arange(0, 8 * 256 + 1) / 256.0
    np.testing.assert_array_equal(t(z), (-torch.log(torch.exp(torch.from_numpy(z)))).numpy())


@pytest.mark.parametrize('method,n,m', [('superglue', 24, 24), ('triplet_loss', 24, 24), ('gap_loss', 24, 24), ('gap_loss', 17, 33),
                                        ('gap_loss', 33, 17), ('gap_loss', 1, 1), ('triplet_loss', 1, 1)])
def test_restatement_equals_autograd_on_the_grid(method, n, m):
    rs = np.random.RandomState(1000 * n + m)
    B = len(GT_PATTERNS)
    g0, g1 = gt_batch(GT_PATTERNS, n, m, seed=n + m)
    for _ in range(200):
        Z = grid_Z(B, n, m, rs)
        if method != 'triplet_loss' or triplet_top_gap(Z, g0, g1) > 0:
            break
    if method == 'triplet_loss':
        assert triplet_top_gap(Z, g0, g1) > 0           # no row / column with tied top non-positives: the arg-max is not open
    dloss = np.round(rs.uniform(0.5, 2.0, B) * 256) / 256
    zt = torch.from_numpy(Z).requires_grad_(True)
    loss = torch_pair_losses(zt, g0, g1, method, 0.5)
    np.testing.assert_allclose(loss.detach().numpy(), pair_losses(Z, g0, g1, method, 0.5), rtol=1e-13)
    (loss * torch.from_numpy(dloss)).sum().backward()
    got = pair_grads(Z, g0, g1, method, 0.5, dloss)
    assert_grad_close(got, zt.grad.numpy(), n, m, f'{method} {n}x{m}')
    if method == 'gap_loss' and n > 1:
        assert clamp_margin(Z, g0, g1, method, 0.5) == 0.0      # exact zeros occur: the >= 0 convention is exercised


def test_ties_take_the_lowest_index():
    """torch.topk leaves the choice among equals open; the restatement (and the kernel) take the lowest index."""
    n = m = 6
    Z = np.full((1, n + 1, m + 1), -4.0)
    g0 = np.array([[2, -1, -1, -1, -1, -1]])
    g1 = np.array([[-1, -1, 0, -1, -1, -1]])
    Z[0, 0, 2] = -3.0                                   # the mutual positive
    Z[0, 0, [4, 5]] = -2.0                              # row 0: columns 4 and 5 tie for the negative
    Z[0, [3, 5], 1] = -3.0                              # column 1: rows 3 and 5 tie
    d = pair_grads(Z, g0, g1, 'triplet_loss', 0.5)[0]
    w = 1.0 / (n + m)
    # every term here is active.  (0, 4) and (0, 5) are also the negatives of their own columns, (3, 1) and (5, 1) of their own rows: one
    # w each from those; the tied choice adds a second w to the LOWER index only
    np.testing.assert_allclose([d[0, 4], d[0, 5], d[3, 1], d[5, 1]], [2 * w, w, 2 * w, w], rtol=1e-15)


def test_bad_index_poisons_the_pair_only():
    rs = np.random.RandomState(3)
    Z = grid_Z(2, 5, 5, rs)
    g0 = rs.randint(-1, 5, (2, 5))
    g1 = rs.randint(-1, 5, (2, 5))
    g0[1, 2] = 7
    for meth in METHODS:
        d = pair_grads(Z, g0, g1, meth)
        assert np.isnan(d[1]).all() and np.isfinite(d[0]).all()


def test_literal_t_gradient():
    """(-g / e) * e: -g where e is normal, non-finite where 1 / e overflows or e == 0, 0 for g == 0 unless e == 0."""
    from loss_grad_ref import dt_dz
    assert abs(dt_dz(0.25, -3.0) + 0.25) < 1e-16
    assert np.isinf(dt_dz(0.25, -740.0)) and dt_dz(0.25, -740.0) < 0
    assert dt_dz(0.0, -740.0) == 0
    assert np.isnan(dt_dz(0.0, -750.0)) and np.isnan(dt_dz(0.25, -750.0))
