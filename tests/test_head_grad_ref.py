"""tests/head_grad_ref.py - the numpy restatement of the matching head's gradient and its derived error bound - against the
reference's own gradients (tests/golden/head_grad*.npz, tools/make_goldens_head_grad.py) and against torch autograd through a
transcription of the two reference lines (models/mdgat.py:397, 430-431) on random fp64 inputs.  CPU only."""
import numpy as np
import pytest
import torch

import head_grad_ref as R

CASE_METHODS = (('n64', 'superglue'), ('n64', 'triplet_loss'), ('n64', 'gap_loss'), ('n48m64', 'gap_loss'))
GRADS = ('ddesc0', 'ddesc1', 'dW', 'db')


def torch_head(desc0, desc1, weight, bias):
    """The reference's two lines on point-major descriptors [B, N, 128] / [B, M, 128]: Conv1d(128, 128, 1) on both frames, then
    einsum('bdn,bdm->bnm') / 128 ** .5."""
    w = weight.reshape(128, 128, 1)
    md0 = torch.nn.functional.conv1d(desc0.transpose(1, 2), w, bias)
    md1 = torch.nn.functional.conv1d(desc1.transpose(1, 2), w, bias)
    return torch.einsum('bdn,bdm->bnm', md0, md1) / 128 ** .5


def random_inputs(B, N, M, seed, dtype=np.float64):
    """Seeded descriptors, final_proj and dscores of the size the network's are: (desc0, desc1, W, b, G)."""
    rs = np.random.RandomState(seed)
    f = lambda *s: rs.standard_normal(s).astype(dtype)        # noqa: E731
    return f(B, N, 128), f(B, M, 128), (f(128, 128) / np.sqrt(128.0)).astype(dtype), (0.1 * f(128)).astype(dtype), f(B, N, M)


@pytest.fixture(scope='module')
def g(golden_dir):
    return R.load_golden(golden_dir)


def test_fixture_holds_every_case(g):
    for case, (B, n, m) in (('n64', (2, 64, 64)), ('n48m64', (2, 48, 64))):
        assert tuple(int(x) for x in g[f'{case}_meta']) == (B, n, m)
        assert g[f'{case}_desc0'].shape == (B, n, 128) and g[f'{case}_desc1'].shape == (B, m, 128)
        assert g[f'{case}_W'].shape == (128, 128) and g[f'{case}_b'].shape == (128,) and g[f'{case}_scores'].shape == (B, n, m)
        assert int(g[f'{case}_iters']) == 20
    for case, meth in CASE_METHODS:
        for k in GRADS + ('dscores', 'dalpha', 'w'):
            assert np.isfinite(g[f'{case}_{meth}_{k}']).all()
        assert np.abs(g[f'{case}_{meth}_dW']).max() > 0 and np.abs(g[f'{case}_{meth}_db']).max() > 0


@pytest.mark.parametrize('case', ['n64', 'n48m64'])
def test_forward_restates_the_references_scores(g, case):
    a = [g[f'{case}_{k}'] for k in ('desc0', 'desc1', 'W', 'b')]
    frac = R.worst_fraction(R.forward(*a), g[f'{case}_scores'], R.tolerances(*a)['scores'])
    print(f'{case} scores: {frac:.2e} of the bound')
    assert frac <= 1.0


@pytest.mark.parametrize('case,meth', CASE_METHODS)
def test_backward_restates_the_references_gradients(g, case, meth):
    a = [g[f'{case}_{k}'] for k in ('desc0', 'desc1', 'W', 'b')] + [g[f'{case}_{meth}_dscores']]
    tol = R.tolerances(*a)
    for k, got in zip(GRADS, R.backward(*a)):
        frac = R.worst_fraction(got, g[f'{case}_{meth}_{k}'], tol[k])
        print(f'{case} {meth} {k}: {frac:.2e} of the bound', end='; ')
        assert frac <= 1.0, (k, frac)


@pytest.mark.parametrize('B,N,M', [(1, 1, 1), (1, 1, 5), (2, 17, 33), (2, 33, 17), (3, 64, 64), (2, 130, 97)])
def test_backward_is_what_autograd_takes_through_the_reference_lines(B, N, M):
    a = random_inputs(B, N, M, 100 * N + M)
    t = [torch.from_numpy(x).clone().requires_grad_() for x in a[:4]]
    scores = torch_head(*t)
    (scores * torch.from_numpy(a[4])).sum().backward()
    tol = R.tolerances(*a)
    assert R.worst_fraction(R.forward(*a[:4]), scores.detach().numpy(), tol['scores']) <= 1.0
    for k, got, ref in zip(GRADS, R.backward(*a), t):
        assert R.worst_fraction(got, ref.grad.numpy(), tol[k]) <= 1.0, k


def test_weight_in_the_conv1d_shape_and_tolerance_arithmetic():
    a = random_inputs(2, 9, 7, 5)
    b = (a[0], a[1], a[2].reshape(128, 128, 1), a[3], a[4])
    for x, y in zip(R.backward(*a), R.backward(*b)):
        assert np.array_equal(x, y)
    K = R.contraction_lengths(2, 9, 7)
    assert K == {'scores': 256, 'ddesc0': 128 + 7 + 128, 'ddesc1': 128 + 9 + 128, 'dW': 128 + 9 + 2 * 16, 'db': 128 + 9 + 2 * 16}
    tol, mag = R.tolerances(*a), R.magnitudes(*a)
    assert set(tol) == {'scores', 'ddesc0', 'ddesc1', 'dW', 'db'}
    for k in tol:
        assert np.array_equal(tol[k], 4.0 * K[k] * 2.0 ** -53 * mag[k]) and (mag[k] > 0).all()
    assert R.worst_fraction(np.ones(3), np.ones(3), np.zeros(3)) == 0.0 and R.worst_fraction(np.ones(3), np.zeros(3), np.zeros(3)) == np.inf
