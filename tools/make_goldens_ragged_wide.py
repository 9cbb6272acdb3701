#!/usr/bin/env python3
"""tests/golden/ragged_wide_pairs.npz: the REAL reference (fp64, CPU, imported unmodified as in tools/make_goldens.py) on three pairs of
different sizes, two of them beyond the 575 keypoints of the register-resident fp64 Sinkhorn, ONE PAIR PER CALL, as test.py runs them -
what MDGAT.forward_ragged must return for the same pairs in one call of a module with config['ragged_sinkhorn'] = 'auto'.

Pairs: the first three of set W of tests/test_gpu_ragged_forward_wide.py, (N_b, M_b) = (600, 40), (40, 610), (64, 64); L = 1,
k = [16, None], 10 Sinkhorn iterations; weights synth.make_state_dict(L=1, seed=1), pair b = synth.make_batch(1, N_b, M_b, first_pair=b).
Inputs are regenerated from these seeds; the file holds outputs only, laid out as tests/golden/ragged_pairs.npz: per pair Z and, per
extraction variant the reference can run on that pair (tools/make_goldens_ragged.py: N != M runs 'gap_loss' and has no superglue
variants), matches and scores.

Refused, as there: a fixture in which a top-k selection or a match arg-max is decided by less than 1e-9."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as G  # noqa: E402
from make_goldens_ragged import GAP, Refused, argmax_gap, topk_gaps  # noqa: E402
from mdgat_matcher_amd import synth  # noqa: E402

PAIRS = ((600, 40), (40, 610), (64, 64))
L, K, S, SEED = 1, [16, None], 10, 1


def main():
    M = G.import_reference()
    sd = synth.make_state_dict(L=L, seed=SEED)
    sched = [0 if k is None else k for k in K]
    arrays = {'pairs': np.array(PAIRS, dtype=np.int64), 'meta': np.array([L, S, SEED], dtype=np.int64),
              'k': np.array([-1 if x is None else x for x in K], dtype=np.int64)}
    for b, (n, m) in enumerate(PAIRS):
        data = synth.make_batch(1, n, m, first_pair=b)
        for tag, (loss_method, mutual) in G.VARIANTS.items():
            if n != m:
                if loss_method == 'superglue':
                    continue
                loss_method = 'gap_loss'
            cfg = synth.default_config(L=L, k=K, sinkhorn_iterations=S, loss_method=loss_method, mutual_check=mutual)
            net = G.build_ref_net(M, cfg, sd)
            seen, restore = topk_gaps(M)
            try:
                out, cap = G.run_ref(M, net, data, capture=False)
            finally:
                restore()
            assert len(seen) == 4 * L, len(seen)                 # two frames per layer
            if tag == 'default':
                for i, kk in enumerate(sched):
                    for logits in seen[2 * i:2 * i + 2]:
                        if kk and kk < logits.shape[-1]:
                            t = logits.topk(kk + 1, dim=-1).values
                            gap = float((t[..., kk - 1] - t[..., kk]).min())
                            if gap < GAP:
                                raise Refused(f'pair {b} layer {i}: a top-{kk} selection is decided by {gap:.3e}')
                arrays[f'p{b}_Z'] = cap['Z'].numpy()
            gap = argmax_gap(cap['Z'], loss_method == 'superglue')
            if gap < GAP:
                raise Refused(f'pair {b} {tag}: a match arg-max is decided by {gap:.3e}')
            for key, v in G.out_arrays(out, tag).items():
                arrays[f'p{b}_{key}'] = v
            print(f'pair {b} ({n} x {m}) {tag}: {int((out["matches0"] >= 0).sum())} matches, smallest arg-max gap {gap:.2e}')
    path = os.path.join(G.OUT, 'ragged_wide_pairs.npz')
    np.savez_compressed(path, **arrays)
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < (1 << 20), 'the fixture must stay under 1 MiB'


if __name__ == '__main__':
    main()
