"""The fp64 restatement of the losses (tests/loss_ref.py) against the reference's own loss values (tests/golden/loss_cases.npz,
tools/make_goldens_loss.py).  CPU only."""
import os

import numpy as np
import pytest
import torch

from loss_ref import module_loss, pair_losses, t

METHODS = ('superglue', 'triplet_loss', 'gap_loss')


@pytest.fixture(scope='module')
def cases(golden_dir):
    return np.load(os.path.join(golden_dir, 'loss_cases.npz'))


def _methods(g, case):
    return [m for m in METHODS if f'{case}_{m}_loss' in g.files]


def _oracle_Z(g, case):
    """Z of a case stored without it, from the fp64 oracle (pinned to the reference by test_oracle_golden.py)."""
    from mdgat_matcher_amd import synth
    from oracle import mdgat_oracle as O
    B, n, m, L, S, seed, first_pair = [int(x) for x in g[f'{case}_meta']]
    k = [None if x < 0 else int(x) for x in g[f'{case}_k']]
    cfg = synth.default_config(L=L, k=k, sinkhorn_iterations=S)
    cap = {}
    O.mdgat_forward(synth.make_state_dict(L=L, seed=seed), cfg, synth.make_batch(B, n, m, first_pair=first_pair), cap)
    return cap['Z'].numpy()


@pytest.mark.parametrize('case', ['n64', 'n48m64', 'b8n256'])
def test_restatement_reproduces_the_reference(cases, case):
    g = cases
    Z = g[f'{case}_Z'] if f'{case}_Z' in g.files else _oracle_Z(g, case)
    gamma = float(g[f'{case}_gamma'])
    for meth in _methods(g, case):
        want = g[f'{case}_{meth}_loss']
        got = module_loss(Z, g[f'{case}_gt0'], g[f'{case}_gt1'], meth, gamma)
        assert np.shape(got) == want.shape, (meth, np.shape(got), want.shape)
        assert np.all(np.isfinite(want))
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=f'{case} {meth}')


def test_fixture_has_real_ground_truth(cases):
    for case in ('n64', 'n48m64', 'b8n256'):
        g0, g1 = cases[f'{case}_gt0'], cases[f'{case}_gt1']
        assert g0.dtype == np.int16 and g1.dtype == np.int16
        assert 0.2 < (g0 >= 0).mean() < 0.8 and (g0 == -1).any() and (g1 == -1).any(), case


def test_in_place_rewrite_recorded(cases):
    """triplet and gap rewrite -1 to m / n in the caller's tensors; superglue leaves them alone."""
    g = cases
    for case in ('n64', 'n48m64'):
        n, m = int(g[f'{case}_meta'][1]), int(g[f'{case}_meta'][2])
        for meth in _methods(g, case):
            a0, a1 = g[f'{case}_{meth}_gt0_after'], g[f'{case}_{meth}_gt1_after']
            if meth == 'superglue':
                np.testing.assert_array_equal(a0, g[f'{case}_gt0'])
                np.testing.assert_array_equal(a1, g[f'{case}_gt1'])
            else:
                np.testing.assert_array_equal(a0, np.where(g[f'{case}_gt0'] == -1, m, g[f'{case}_gt0']))
                np.testing.assert_array_equal(a1, np.where(g[f'{case}_gt1'] == -1, n, g[f'{case}_gt1']))


@pytest.mark.parametrize('case', ['planted_sub', 'planted_inf'])
def test_planted_t_edge(cases, case):
    """Z entries in exp's subnormal band and below its underflow: the restatement applies t() as literally as the reference."""
    g = cases
    Z = g[f'{case}_Z']
    assert ((Z > -740) & (Z < -709)).any() and (Z < -745.2).any()
    gamma = float(g[f'{case}_gamma'])
    for meth in METHODS:
        want = np.asarray(g[f'{case}_{meth}_loss'])
        got = np.asarray(module_loss(Z, g[f'{case}_gt0'], g[f'{case}_gt1'], meth, gamma))
        np.testing.assert_array_equal(np.isinf(got), np.isinf(want), err_msg=f'{case} {meth}')
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{case} {meth}')
        fin = np.isfinite(want)
        np.testing.assert_allclose(got[fin], want[fin], rtol=1e-6, atol=0, err_msg=f'{case} {meth}')
    assert np.isinf(g['planted_inf_triplet_loss_loss']) and np.isinf(g['planted_inf_gap_loss_loss']).all()


def test_t_matches_torch():
    z = np.array([0.0, -1.5, -700.0, -708.5, -720.0, -740.0, -745.0, -745.2, -800.0])
    np.testing.assert_array_equal(t(z), (-torch.log(torch.from_numpy(z).exp())).numpy())


def test_pair_losses_shapes():
    rs = np.random.RandomState(0)
    Z = rs.standard_normal((3, 9, 9)) - 3
    g0 = rs.randint(-1, 8, (3, 8))
    g1 = rs.randint(-1, 8, (3, 8))
    for meth in METHODS:
        assert pair_losses(Z, g0, g1, meth).shape == (3,)
    assert np.ndim(module_loss(Z, g0, g1, 'triplet_loss')) == 0
