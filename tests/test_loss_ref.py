"""The fp64 restatement of the losses (tests/loss_ref.py) against the reference's own loss values (tests/golden/loss_cases.npz,
tools/make_goldens_loss.py).  CPU only."""
import os

import numpy as np
import pytest
import torch

from loss_ref import GT_PATTERNS, clamp0, gt_batch, module_loss, pair_losses, t

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


def _gap_per_column(Z, gt0, gt1, gamma=0.5):
    """gap_loss with its column half taken naively per column of Z (column j: its positive against the other rows of that column).  The
    reference's row-major reordering comes to this when every positive lies in the dustbin row (V is then the inner rows of Z, P the
    dustbin row in column order), not in general."""
    out = []
    for z, g0, g1 in zip(np.asarray(Z, dtype=np.float64), gt0, gt1):
        n, m = z.shape[0] - 1, z.shape[1] - 1
        p0, p1 = np.where(g0 == -1, m, g0), np.where(g1 == -1, n, g1)
        tz = t(z)
        keep_r = np.ones((n, m + 1), dtype=bool)
        keep_r[np.arange(n), p0] = False
        row = np.where(keep_r, clamp0(tz[np.arange(n), p0][:, None] - tz[:n] + gamma), 0.0).sum(axis=1)
        keep_c = np.ones((n + 1, m), dtype=bool)
        keep_c[p1, np.arange(m)] = False
        col = np.where(keep_c, clamp0(tz[p1, np.arange(m)][None, :] - tz[:, :m] + gamma), 0.0).sum(axis=0)
        out.append((np.mean(2 * np.log(row + 1)) + np.mean(2 * np.log(col + 1))) / 2)
    return np.array(out)


def test_gt_patterns_reach_gaps_reordering():
    """The gt patterns of the kernel tests (loss_ref.gt_pattern, tests/test_gpu_loss.py) at 511 x 511: a per-column column half is far
    from the reference's wherever the row-major reordering matters, P's order crosses the 256-column chunks of the kernel's stable
    ranking, one row holds >= 256 positives - and with every positive in the dustbin row the two forms agree."""
    from oracle import mdgat_oracle as O
    n = m = 511
    s = (torch.rand(len(GT_PATTERNS), n, m, generator=torch.Generator().manual_seed(511), dtype=torch.float64) * 2 - 1) * 15
    Z = O.log_optimal_transport(s, torch.tensor(0.0, dtype=torch.float64), 20).numpy()   # (as test_gpu_loss._lp_Z)
    g0, g1 = gt_batch(GT_PATTERNS, n, m, seed=511)
    ref = pair_losses(Z, g0, g1, 'gap_loss')
    naive = _gap_per_column(Z, g0, g1)
    assert np.all(np.isfinite(ref)) and np.all(ref > 0)
    for b, name in enumerate(GT_PATTERNS):
        p1 = np.where(g1[b] == -1, n, g1[b])
        order = np.argsort(p1, kind='stable')                      # the columns in P's (row-major) order
        crosses = bool(np.any(order // 256 != np.arange(m) // 256))
        rel = abs(naive[b] - ref[b]) / abs(ref[b])
        if name == 'all_dustbin':
            assert rel < 1e-12 and not crosses, (name, rel)
        else:
            assert rel > 1e-6, (name, rel)                          # the kernel tests hold the kernel to 1e-11
        if name in ('partial', 'reversed', 'explicit_dustbin'):
            assert crosses, name
        if name == 'non_injective':
            assert np.bincount(p1).max() >= 256
        if name == 'explicit_dustbin':
            assert (g0[b] == m).any() and (g0[b] == -1).any() and (g1[b] == n).any() and (g1[b] == -1).any()
