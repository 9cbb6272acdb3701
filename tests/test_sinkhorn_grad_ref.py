"""The fp64 restatement of log_optimal_transport's gradient (tests/sinkhorn_grad_ref.py) against torch autograd of the oracle and
against the reference's own autograd gradients (tests/golden/sk_grad.npz, tools/make_goldens_grad.py).  CPU only."""
import os

import numpy as np
import pytest
import torch

from sinkhorn_grad_ref import REVERSE_VARIANTS, VARIANT_CASES, max_rel, oracle_grad, reverse_dispatch, sinkhorn_grad

CASES = ('b2n64m48', 'n120m180', 'n7m5')


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'sk_grad.npz'))


@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_the_reference(golden, case):
    g = golden
    ds, da = sinkhorn_grad(torch.from_numpy(g[f'{case}_scores']), float(g[f'{case}_alpha']), int(g[f'{case}_iters']),
                           torch.from_numpy(g[f'{case}_dZ']))
    assert max_rel(ds, torch.from_numpy(g[f'{case}_dscores'])) < 1e-10
    ref_a = float(g[f'{case}_dalpha'])
    assert abs(da.sum().item() - ref_a) <= 1e-10 * max(abs(ref_a), 1e-300)


@pytest.mark.parametrize('B,N,M,T,spread,alpha', [(2, 7, 5, 0, 3.0, 0.5), (2, 7, 5, 1, 3.0, 0.5), (1, 9, 13, 3, 1.0, 4.0),
                                                  (2, 24, 16, 50, 100.0, 1.0), (1, 16, 16, 100, 450.0, -2.0)])
def test_restatement_matches_oracle_autograd(B, N, M, T, spread, alpha):
    g = torch.Generator().manual_seed(B * 1000 + N * 10 + T)
    s = (torch.rand(B, N, M, generator=g, dtype=torch.float64) * 2 - 1) * spread
    dZ = torch.randn(B, N + 1, M + 1, generator=g, dtype=torch.float64)
    ds, da = sinkhorn_grad(s, alpha, T, dZ)
    ods, oda = oracle_grad(s, alpha, T, dZ)
    assert torch.isfinite(ds).all() and torch.isfinite(da).all()
    assert max_rel(ds, ods) < 1e-10
    assert abs(da.sum().item() - oda.item()) <= 1e-10 * max(abs(oda.item()), 1e-300)


def test_zero_iterations_is_the_identity_on_the_couplings():
    s = torch.randn(2, 4, 6, dtype=torch.float64)
    dZ = torch.randn(2, 5, 7, dtype=torch.float64)
    ds, da = sinkhorn_grad(s, 0.25, 0, dZ)
    assert torch.equal(ds, dZ[:, :4, :6])
    assert torch.allclose(da, dZ[:, 4, :].sum(1) + dZ[:, :4, 6].sum(1), rtol=0, atol=1e-14)


def test_reverse_dispatch_mirrors_the_launcher():
    assert reverse_dispatch(1) == (128, 1, 5)
    assert reverse_dispatch(639) == (640, 5, 5) and reverse_dispatch(640) == (768, 6, 9)
    assert reverse_dispatch(1151) == (1152, 9, 9) and reverse_dispatch(1152) == (1280, 10, 17)
    assert reverse_dispatch(2047) == (2048, 16, 17) and reverse_dispatch(2175) == (2176, 17, 17)
    with pytest.raises(ValueError):
        reverse_dispatch(2176)


def test_reverse_variant_cases_cover_every_path():
    """The shapes of the GPU's test_fp64_reverse_variants reach every skg_reverse_kernel instantiation with and without its masked
    column pairs, both sides of every switch, both tile-edge states of rows and columns, both slab states and both T parities."""
    Ms = {M for _, _, M, _ in VARIANT_CASES}
    paths = {(reverse_dispatch(M)[2], reverse_dispatch(M)[1] < reverse_dispatch(M)[2]) for M in Ms}
    assert paths == {(v, masked) for v in REVERSE_VARIANTS for masked in (False, True)}, paths
    # both sides of every switch (test_reverse_dispatch_mirrors_the_launcher): <5> | <9>, <9> | <17>, <17> masked | unmasked
    assert {639, 640, 1151, 1152, 2047, 2048} <= Ms
    assert {(N + 1) % 64 == 0 for _, N, _, _ in VARIANT_CASES} == {False, True}
    assert {(M + 1) % 64 == 0 for _, _, M, _ in VARIANT_CASES} == {False, True}
    assert {N % 32 == 0 for _, N, _, _ in VARIANT_CASES} == {False, True}
    assert {(2 * T) % 4 for _, _, _, T in VARIANT_CASES} == {0, 2}
    assert {1, 7, 20, 100, 200} <= {T for _, _, _, T in VARIANT_CASES}
    assert (1, 1, 2048) in {(B, N, M) for B, N, M, _ in VARIANT_CASES}
    assert (1, 2175, 1) in {(B, N, M) for B, N, M, _ in VARIANT_CASES}
    assert any(B > 1 for B, _, _, _ in VARIANT_CASES)
