"""tests/golden/ragged_pairs.npz (tools/make_goldens_ragged.py: the reference itself, one pair per call) against the CPU oracle, pair by
pair, at the bounds of tests/test_oracle_golden.py: the fixture the ragged GPU tests lean on is what the reference computes."""
import os

import numpy as np
import pytest

from mdgat_matcher_amd import synth
from oracle import mdgat_oracle as O

TOL = 1e-9
VARIANTS = {'default': ('triplet_loss', False), 'mutual': ('triplet_loss', True), 'sg': ('superglue', False), 'sgmutual': ('superglue', True)}


@pytest.mark.parametrize('b', range(5))
def test_oracle_per_pair_equals_the_reference_held_ragged_pairs(golden_dir, b):
    g = np.load(os.path.join(golden_dir, 'ragged_pairs.npz'))
    L, S, seed = [int(x) for x in g['meta']]
    k = [None if x < 0 else int(x) for x in g['k']]
    n, m = [int(x) for x in g['pairs'][b]]
    sd = synth.make_state_dict(L=L, seed=seed)
    data = synth.make_batch(1, n, m, first_pair=b)
    held = [tag for tag in VARIANTS if f'p{b}_{tag}_matches0' in g.files]
    assert 'default' in held and 'mutual' in held and (n != m or len(held) == 4)
    for tag in held:
        loss_method, mutual = VARIANTS[tag]
        cap = {}
        out = O.mdgat_forward(sd, synth.default_config(L=L, k=k, sinkhorn_iterations=S, loss_method=loss_method, mutual_check=mutual), data, cap)
        if tag == 'default':
            assert cap['Z'].shape == (1, n + 1, m + 1) and np.abs(cap['Z'].numpy() - g[f'p{b}_Z']).max() < TOL
        np.testing.assert_array_equal(out['matches0'].numpy(), g[f'p{b}_{tag}_matches0'])
        np.testing.assert_array_equal(out['matches1'].numpy(), g[f'p{b}_{tag}_matches1'])
        np.testing.assert_allclose(out['matching_scores0'].numpy(), g[f'p{b}_{tag}_mscores0'], atol=TOL)
        np.testing.assert_allclose(out['matching_scores1'].numpy(), g[f'p{b}_{tag}_mscores1'], atol=TOL)
