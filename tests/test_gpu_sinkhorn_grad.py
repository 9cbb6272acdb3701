"""The backward of log_optimal_transport (csrc/sinkhorn_grad.hip; ops.sinkhorn_backward, ops.log_optimal_transport and the drop-in
models.mdgat.log_optimal_transport) against the reference's autograd gradients (tests/golden/sk_grad.npz), against torch autograd
of the fp64 oracle on the CPU, and against the fp64 restatement (tests/sinkhorn_grad_ref.py) at the shapes of every kernel variant and
of training."""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

from loss_ref import gt_batch
import sinkhorn_f64_forms as F
from sinkhorn_grad_ref import REVERSE_VARIANTS, VARIANT_CASES, max_rel, oracle_grad, reverse_dispatch, sinkhorn_grad

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'


def _ops():
    from mdgat_matcher_amd import ops
    return ops


def _grads(scores, alpha, iters, dZ, arithmetic='auto'):
    """(dscores, dalpha) of ops.log_optimal_transport on the GPU for a given dZ."""
    s = scores.to(DEV).clone().requires_grad_(True)
    al = torch.tensor(float(alpha), dtype=scores.dtype, device=DEV, requires_grad=True)
    Z = _ops().log_optimal_transport(s, al, iters, arithmetic=arithmetic)
    Z.backward(dZ.to(device=DEV, dtype=Z.dtype))
    return s.grad.cpu(), al.grad.cpu()


def _check(ds, da, ref_ds, ref_da, tol):
    e_s = max_rel(ds, ref_ds)
    ref_da = torch.as_tensor(ref_da, dtype=torch.float64)
    e_a = abs(float(da) - float(ref_da)) / max(abs(float(ref_da)), 1e-300)
    print(f'dscores {e_s:.2e} of max|g|, dalpha {e_a:.2e}')
    assert torch.isfinite(ds).all() and math.isfinite(float(da))
    assert e_s < tol and e_a < tol, (e_s, e_a)


@pytest.mark.parametrize('case', ['b2n64m48', 'n120m180', 'n7m5'])
def test_fp64_against_reference_goldens(golden_dir, case):
    g = np.load(os.path.join(golden_dir, 'sk_grad.npz'))
    ds, da = _grads(torch.from_numpy(g[f'{case}_scores']), float(g[f'{case}_alpha']), int(g[f'{case}_iters']),
                    torch.from_numpy(g[f'{case}_dZ']))
    assert ds.dtype == torch.float64 and da.dtype == torch.float64 and da.shape == ()
    _check(ds, da, torch.from_numpy(g[f'{case}_dscores']), g[f'{case}_dalpha'], 1e-8)


# N != M, every T of the issue, a score spread of +-100, dustbin-heavy pairs (alpha above the scores), streaming-sized frames
@pytest.mark.parametrize('B,N,M,T,spread,alpha', [
    (2, 24, 40, 0, 3.0, 0.5),
    (2, 24, 40, 1, 3.0, 0.5),
    (2, 33, 20, 100, 100.0, 1.0),
    (1, 50, 70, 100, 2.0, 6.0),
    (1, 600, 130, 3, 5.0, 1.0),
    (1, 300, 700, 10, 4.0, 1.0),          # skg_reverse_kernel<9>: autograd, not the scaling form of the restatement
])
def test_fp64_against_oracle_autograd(B, N, M, T, spread, alpha):
    gen = torch.Generator().manual_seed(N * 131 + M * 7 + T)
    s = (torch.rand(B, N, M, generator=gen, dtype=torch.float64) * 2 - 1) * spread
    dZ = torch.randn(B, N + 1, M + 1, generator=gen, dtype=torch.float64)
    ds, da = _grads(s, alpha, T, dZ)
    ref_ds, ref_da = oracle_grad(s, alpha, T, dZ)
    _check(ds, da, ref_ds, ref_da, 1e-8)


def test_fp64_at_the_streaming_limit():
    N = M = 2175
    gen = torch.Generator().manual_seed(2175)
    s = (torch.rand(1, N, M, generator=gen, dtype=torch.float64) * 2 - 1) * 4.0
    dZ = torch.randn(1, N + 1, M + 1, generator=gen, dtype=torch.float64)
    ds, da = _grads(s, 1.0, 5, dZ)
    ref_ds, ref_da = oracle_grad(s, 1.0, 5, dZ)
    _check(ds, da, ref_ds, ref_da, 1e-8)


# ---- against the fp64 restatement (tests/sinkhorn_grad_ref.py) at the shapes and values the small cases above do not reach ----
def _check_pairs(ds, dbin, ref_ds, ref_da, tol):
    """d scores and every pair's d bin score of ops.sinkhorn_backward within tol of max|g| of the restatement's."""
    e_s, e_a = max_rel(ds, ref_ds), max_rel(dbin, ref_da)
    print(f'dscores {e_s:.2e} of max|g|, dalpha {e_a:.2e} of max|dalpha|')
    assert torch.isfinite(ds).all() and torch.isfinite(dbin).all()
    assert e_s < tol and e_a < tol, (e_s, e_a)


def _against_restatement(s, alpha, T, dZ):
    ds, dbin = _ops().sinkhorn_backward(s.to(DEV), alpha, T, dZ.to(DEV))
    ref_ds, ref_da = sinkhorn_grad(s, alpha, T, dZ)
    _check_pairs(ds.cpu(), dbin.cpu(), ref_ds, ref_da, 1e-8)


def _uniform(B, N, M, spread, gen):
    return (torch.rand(B, N, M, generator=gen, dtype=torch.float64) * 2 - 1) * spread


def _model_scores(B, N, M, seed, D=64):
    """Scores as the model forms them: the scaled dot product of descriptors (final_proj, / sqrt(D)), standard deviation 2: about +-10."""
    gen = torch.Generator().manual_seed(seed)
    d0 = torch.randn(B, D, N, generator=gen, dtype=torch.float64)
    d1 = torch.randn(B, D, M, generator=gen, dtype=torch.float64)
    return torch.einsum('bdn,bdm->bnm', d0, d1) / D ** .5 * 2.0


def _superglue_dZ(B, N, M, seed):
    """dL/dZ of the superglue loss (_superglue_loss below) for random partial matches: -1 / (unmatched columns + M) / B at every row's
    gt entry (the dustbin column for an unmatched row) and at the dustbin row of every unmatched column, zero elsewhere."""
    gt0, gt1 = (torch.from_numpy(g) for g in gt_batch(['partial'] * B, N, M, seed))
    Z = torch.zeros(B, N + 1, M + 1, dtype=torch.float64, requires_grad=True)
    _superglue_loss(Z, gt0, gt1).backward()
    assert int((Z.grad != 0).sum()) == B * N + int((gt1 == -1).sum())
    return Z.grad


@pytest.mark.parametrize('B,N,M,T', VARIANT_CASES)
def test_fp64_reverse_variants(B, N, M, T):
    """skg_reverse_kernel<5 / 9 / 17> with and without masked column pairs, and the history-writing streaming forward in each
    (the shape list and what it covers: sinkhorn_grad_ref.VARIANT_CASES, checked on the CPU by test_sinkhorn_grad_ref.py)."""
    print(f'M={M}: Mp, nc2, variant = {reverse_dispatch(M)}', end='; ')
    gen = torch.Generator().manual_seed(N * 7 + M * 131 + T)
    with F.watch() as w:
        _against_restatement(_uniform(B, N, M, 4.0, gen), 1.0, T, torch.randn(B, N + 1, M + 1, generator=gen, dtype=torch.float64))
    # the history run of the instantiation the columns name (tests/sinkhorn_f64_forms.py), and no other call of the fp64 Sinkhorn
    assert w.ran() == {F.HISTORY_5 + REVERSE_VARIANTS.index(reverse_dispatch(M)[2]): 1}, w.ran()


# a score spread of +-100, and dustbin-heavy pairs (alpha above every score), in <9> (900 columns: nc2 8) and <17> (1500: nc2 12)
@pytest.mark.parametrize('B,N,M,T,spread,alpha', [
    (1, 200, 900, 50, 100.0, 1.0),
    (1, 200, 900, 50, 2.0, 6.0),
    (2, 150, 1500, 30, 100.0, 1.0),
    (1, 150, 1500, 30, 2.0, 6.0),
])
def test_fp64_hard_values_in_the_wide_variants(B, N, M, T, spread, alpha):
    gen = torch.Generator().manual_seed(N + M + T + int(spread))
    _against_restatement(_uniform(B, N, M, spread, gen), alpha, T, torch.randn(B, N + 1, M + 1, generator=gen, dtype=torch.float64))


# BASELINE's training shapes: 64 pairs of 512 at T = 100 (eight of them here) and pairs of 2048 at T = 200
@pytest.mark.parametrize('B,N,T', [(8, 512, 100), (1, 2048, 200)])
@pytest.mark.parametrize('dz', ['dense', 'superglue'])
def test_fp64_at_production_shapes(B, N, T, dz):
    s = _model_scores(B, N, N, seed=N + T)
    if dz == 'dense':
        dZ = torch.randn(B, N + 1, N + 1, generator=torch.Generator().manual_seed(N), dtype=torch.float64)
    else:
        dZ = _superglue_dZ(B, N, N, seed=N)
    _against_restatement(s, 1.0, T, dZ)


def test_fp32_inputs_at_2048():
    s = _model_scores(1, 2048, 2048, seed=2048).to(torch.float32)
    dZ = torch.randn(1, 2049, 2049, generator=torch.Generator().manual_seed(1), dtype=torch.float32)
    x = s.to(DEV).requires_grad_(True)
    al = torch.tensor(1.0, dtype=torch.float32, device=DEV, requires_grad=True)
    Z = _ops().log_optimal_transport(x, al, 100)
    assert Z.dtype == torch.float32
    Z.backward(dZ.to(DEV))
    assert x.grad.dtype == torch.float32 and al.grad.dtype == torch.float32
    ref_ds, ref_da = sinkhorn_grad(s.double(), 1.0, 100, dZ.double())
    _check(x.grad.cpu().double(), al.grad.cpu().double(), ref_ds, ref_da.sum(), 1e-6)


@pytest.mark.parametrize('N,M', [(700, 900), (300, 1500)])
def test_wide_variants_are_bitwise_batch_independent(N, M):
    """<9> (900 columns) and <17> (1500): every pair of a batch of three alone gives its slice's bits."""
    gen = torch.Generator().manual_seed(N + M)
    S = _uniform(3, N, M, 20.0, gen).to(DEV)
    G = torch.randn(3, N + 1, M + 1, generator=gen, dtype=torch.float64).to(DEV)
    ds3, db3 = _ops().sinkhorn_backward(S, 1.5, 30, G)
    worst = 0.0
    for b in range(3):
        ds1, db1 = _ops().sinkhorn_backward(S[b:b + 1], 1.5, 30, G[b:b + 1])
        worst = max(worst, (ds1 - ds3[b:b + 1]).abs().max().item(), (db1 - db3[b:b + 1]).abs().max().item())
        assert torch.equal(ds1, ds3[b:b + 1]) and torch.equal(db1, db3[b:b + 1]), b
    print(f'max |alone - batch| = {worst:.1e}')


def test_gradcheck_scores_and_alpha():
    gen = torch.Generator().manual_seed(3)
    s = torch.randn(2, 3, 4, generator=gen, dtype=torch.float64).to(DEV).requires_grad_(True)
    al = torch.tensor(0.7, dtype=torch.float64, device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x, a: _ops().log_optimal_transport(x, a, 3), (s, al), eps=1e-6, atol=1e-7, rtol=1e-6)


def test_fp32_inputs_get_fp32_gradients():
    gen = torch.Generator().manual_seed(5)
    s = ((torch.rand(2, 40, 56, generator=gen) * 2 - 1) * 8).to(torch.float32)
    dZ = torch.randn(2, 41, 57, generator=gen, dtype=torch.float32)
    x = s.to(DEV).requires_grad_(True)
    al = torch.tensor(1.0, dtype=torch.float32, device=DEV, requires_grad=True)
    Z = _ops().log_optimal_transport(x, al, 50)
    assert Z.dtype == torch.float32
    Z.backward(dZ.to(DEV))
    assert x.grad.dtype == torch.float32 and al.grad.dtype == torch.float32 and al.grad.shape == ()
    ref_ds, ref_da = oracle_grad(s.double(), 1.0, 50, dZ.double())
    _check(x.grad.cpu().double(), al.grad.cpu().double(), ref_ds, ref_da, 1e-6)


def test_raw_entry_takes_expanded_dZ_and_python_alpha():
    gen = torch.Generator().manual_seed(9)
    s = torch.randn(2, 9, 7, generator=gen, dtype=torch.float64)
    dZ = torch.ones((), dtype=torch.float64).expand(2, 10, 8)              # what Z.sum().backward() hands over
    ds, dbin = _ops().sinkhorn_backward(s.to(DEV), 0.3, 20, dZ.to(DEV))
    assert ds.dtype == torch.float64 and dbin.shape == (2,)
    ref_ds, ref_da = oracle_grad(s, 0.3, 20, dZ.contiguous())
    _check(ds.cpu(), dbin.sum().cpu(), ref_ds, ref_da, 1e-8)
    x = s.to(DEV).requires_grad_(True)                                      # alpha a python float: no gradient for it, none asked
    _ops().log_optimal_transport(x, 0.3, 20).sum().backward()
    assert torch.equal(x.grad, ds)


@pytest.fixture()
def models_mdgat():
    """`import models.mdgat` the way the reference's scripts do, with <repo>/integration ahead on sys.path."""
    shim = os.path.join(ROOT, 'integration')
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == 'models' or k.startswith('models.')}
    sys.path.insert(0, shim)
    try:
        yield importlib.import_module('models.mdgat')
    finally:
        sys.path.remove(shim)
        for k in [k for k in sys.modules if k == 'models' or k.startswith('models.')]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_dropin_is_differentiable_with_an_unchanged_forward(models_mdgat):
    lot = models_mdgat.log_optimal_transport
    gen = torch.Generator().manual_seed(17)
    s = torch.randn(2, 30, 45, generator=gen, dtype=torch.float32) * 3
    alpha = torch.nn.Parameter(torch.tensor(1.0, device=DEV))
    with torch.no_grad():
        Z0 = lot(s.to(DEV), alpha, 100)
    x = s.to(DEV).requires_grad_(True)
    Z = lot(x, alpha, 100)
    assert Z.grad_fn is not None and Z0.grad_fn is None
    assert torch.equal(Z.detach(), Z0)
    Z.sum().backward()
    ref_ds, ref_da = oracle_grad(s.double(), 1.0, 100, torch.ones(2, 31, 46, dtype=torch.float64))
    _check(x.grad.cpu().double(), alpha.grad.cpu().double(), ref_ds, ref_da, 1e-6)
    x.grad, alpha.grad = None, None
    dZ = torch.randn(2, 31, 46, generator=gen, dtype=torch.float32)
    lot(x, alpha, 100).backward(dZ.to(DEV))
    ref_ds, ref_da = oracle_grad(s.double(), 1.0, 100, dZ.double())
    _check(x.grad.cpu().double(), alpha.grad.cpu().double(), ref_ds, ref_da, 1e-6)


def _superglue_loss(Z, gt0, gt1):
    """The reference's superglue loss (mdgat.py:487-510) on Z, vectorised: -(sum of Z at the gt of every row (-1: the dustbin column)
    + the dustbin row at every unmatched column) / (unmatched columns + m), averaged over the pairs."""
    b, n = gt0.shape
    m = gt1.shape[1]
    tp = Z[torch.arange(b, device=Z.device)[:, None], torch.arange(n, device=Z.device)[None], gt0].sum(1)
    un = (gt1 == -1)
    tn = (Z[:, -1, :m] * un).sum(1)
    return torch.mean((-tp - tn) / (un.sum(1) + m))


@pytest.mark.parametrize('dtype,tol', [(torch.float64, 1e-8), (torch.float32, 1e-5)])
def test_dropin_end_to_end_step_matches_the_cpu_oracle(models_mdgat, dtype, tol):
    from oracle import mdgat_oracle as O
    gen = torch.Generator().manual_seed(23)
    b, d, n, m = 2, 32, 24, 24
    d0 = torch.randn(b, d, n, generator=gen, dtype=torch.float64)
    d1 = torch.randn(b, d, m, generator=gen, dtype=torch.float64)
    gt0 = torch.randint(-1, m, (b, n), generator=gen)
    gt1 = torch.randint(-1, n, (b, m), generator=gen)

    def step(lot, dev, dtype):
        x0 = d0.to(device=dev, dtype=dtype).requires_grad_(True)
        x1 = d1.to(device=dev, dtype=dtype).requires_grad_(True)
        bin_score = torch.nn.Parameter(torch.tensor(1.0, device=dev, dtype=dtype))
        scores = torch.einsum('bdn,bdm->bnm', x0, x1) / d ** .5
        Z = lot(scores, bin_score, 100)
        loss = _superglue_loss(Z, gt0.to(dev), gt1.to(dev))
        loss.backward()
        return loss.detach().cpu().double(), x0.grad.cpu().double(), x1.grad.cpu().double(), bin_score.grad.cpu().double()

    got = step(models_mdgat.log_optimal_transport, DEV, dtype)
    ref = step(O.log_optimal_transport, 'cpu', torch.float64)
    assert abs(float(got[0] - ref[0])) < 1e-5
    for g, r in zip(got[1:], ref[1:]):
        print(f'{max_rel(g, r):.2e} of max|g|')
        assert max_rel(g, r) < tol, max_rel(g, r)


def test_a_pair_is_bitwise_the_same_alone_and_in_a_batch():
    gen = torch.Generator().manual_seed(31)
    s = (torch.rand(8, 70, 150, generator=gen, dtype=torch.float64) * 2 - 1) * 20
    dZ = torch.randn(8, 71, 151, generator=gen, dtype=torch.float64)
    S, G = s.to(DEV), dZ.to(DEV)
    ops = _ops()
    ds8, db8 = ops.sinkhorn_backward(S, 1.5, 40, G)
    ds8b, db8b = ops.sinkhorn_backward(S, 1.5, 40, G)
    ds1, db1 = ops.sinkhorn_backward(S[5:6], 1.5, 40, G[5:6])
    assert torch.equal(ds8, ds8b) and torch.equal(db8, db8b)
    assert torch.equal(ds8[5:6], ds1) and torch.equal(db8[5:6], db1)


def test_guards():
    ops = _ops()
    with pytest.raises(RuntimeError, match='2175'):
        ops.sinkhorn_backward(torch.zeros(1, 2176, 4, dtype=torch.float64, device=DEV), 1.0, 3,
                              torch.zeros(1, 2177, 5, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.sinkhorn_backward(torch.zeros(1, 4, 4, dtype=torch.float64), 1.0, 3, torch.zeros(1, 5, 5, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.log_optimal_transport(torch.zeros(1, 4, 4, dtype=torch.float64, requires_grad=True), 1.0, 3)
    with pytest.raises(ValueError, match='does not fit'):
        ops.sinkhorn_backward(torch.zeros(1, 4, 4, dtype=torch.float64, device=DEV), 1.0, 3,
                              torch.zeros(1, 4, 5, dtype=torch.float64, device=DEV))
    x = torch.zeros(1, 4, 4, dtype=torch.float64, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match='arithmetic'):
        ops.log_optimal_transport(x, 1.0, 3, arithmetic='bf16')
