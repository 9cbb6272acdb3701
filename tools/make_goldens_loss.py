#!/usr/bin/env python3
"""Generate tests/golden/loss_cases.npz: the reference's own evaluation loss (models/mdgat.py:486-594) on pairs with real ground
truth.  Runs where the reference exists (never on the GPU box); imports it unmodified through the device shim of make_goldens.py.

Pairs are synth.make_batch's correlated frames; their ground truth is oracle.gt_matches (load_data.py:238-285) at 0.5 m with
frame 1 taken back through the rigid motion synth.make_pair applied, so the re-observed keypoints match and the rest go to the
dustbin.  gt_matches are int16, as the loader gives them.  Per case ``<case>_`` (Z is the same for every loss method: the method
only selects the extraction branch):

* ``meta`` [B, n, m, L, S, seed, first_pair], ``k``, ``gamma``, ``gt0`` / ``gt1`` before the call, ``Z`` (not for ``b8n256``);
* per method ``<case>_<method>_loss`` (the reference's ``loss``: 0-d for superglue / triplet, [B] for gap) and
  ``<case>_<method>_gt0_after`` / ``_gt1_after`` (the reference rewrites -1 in place for triplet and gap).

Cases: ``n64`` (B=2, n=m=64, every method); ``n48m64`` (gap only: the other two raise on ragged pairs); ``b8n256`` (BASELINE
configs[0]: 8 pairs of 256, L=4, S=20; losses and gts only); ``planted_sub`` / ``planted_inf`` (one pair of 64 whose Z, as
log_optimal_transport returns it, is overwritten in places with values in the subnormal band of exp (-740 .. -709) and below
-745.2, where exp is 0 and -log(exp(z)) is +inf: pins the reference's literal t(z)).

    python tools/make_goldens_loss.py [--check]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_goldens as G  # noqa: E402
from mdgat_matcher_amd import synth  # noqa: E402
from oracle import mdgat_oracle as O  # noqa: E402

NAME = 'loss_cases'
METHODS = ('superglue', 'triplet_loss', 'gap_loss')
SMALL_K = [16, None, 16, None, 8, None, 8, None]
GAMMA = 0.5


def pair_motion(n, m, pair_index, base_seed=1234):
    """The rigid motion synth.make_pair applies to the re-observed keypoints (k1 = R k0 + t + noise), drawn the same way."""
    rs = np.random.RandomState(base_seed + 7919 * (pair_index + 1))
    rs.permutation(n)
    rs.permutation(m)
    th = 0.1 * rs.standard_normal()
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    t = rs.standard_normal(3)
    return R, t


def ground_truth(data, first_pair):
    """gt_matches0/1 [B, n] / [B, m] int16: frame 1 mapped back into frame 0's coordinates (T1 = inverse motion)."""
    B, n, m = data['keypoints0'].shape[0], data['keypoints0'].shape[1], data['keypoints1'].shape[1]
    g0, g1 = [], []
    for b in range(B):
        R, t = pair_motion(n, m, first_pair + b)
        T1 = np.eye(4)
        T1[:3, :3], T1[:3, 3] = R.T, -R.T @ t
        a0, a1, _ = O.gt_matches(data['keypoints0'][b].numpy(), data['keypoints1'][b].numpy(), None, T1, threshold=0.5)
        g0.append(a0)
        g1.append(a1)
    return torch.from_numpy(np.stack(g0).astype(np.int16)), torch.from_numpy(np.stack(g1).astype(np.int16))


def plant(Z, gt0, gt1, rs, inf):
    """Overwrite entries of one pair's Z: positives and negatives of some rows / columns in the subnormal band of exp, a few
    negatives below -745.2, and (inf) one row's positive below -745.2 as well."""
    Z = Z.clone()
    n, m = Z.shape[1] - 1, Z.shape[2] - 1
    p0 = [int(g) if g >= 0 else m for g in gt0[0]]
    p1 = [int(g) if g >= 0 else n for g in gt1[0]]
    for i in range(0, n, 5):
        Z[0, i, p0[i]] = rs.uniform(-740.0, -709.0)
        Z[0, i, (p0[i] + 1) % (m + 1)] = rs.uniform(-740.0, -709.0)
    for j in range(2, m, 7):
        Z[0, p1[j], j] = rs.uniform(-740.0, -709.0)
        Z[0, (p1[j] + 3) % (n + 1), j] = rs.uniform(-760.0, -745.2)
    Z[0, n, 1::9] = torch.from_numpy(rs.uniform(-740.0, -709.0, Z[0, n, 1::9].shape[0]))
    if inf:
        Z[0, 3, p0[3]] = -750.0
    return Z


def run(M, cfg, sd, data, gt0, gt1, planted=None):
    """The reference's forward with real gts; returns (loss, Z, gt0 after, gt1 after) - the dict it was given is its own copy."""
    net = G.build_ref_net(M, cfg, sd)
    d = {k: v.clone() for k, v in data.items()}
    d['gt_matches0'], d['gt_matches1'] = gt0.clone(), gt1.clone()
    orig = M.log_optimal_transport
    cap = {}

    def lot(scores, alpha, iters):
        Z = orig(scores, alpha, iters)
        if planted is not None:
            Z = planted(Z)
        cap['Z'] = Z.detach().clone()
        return Z
    M.log_optimal_transport = lot
    try:
        with torch.no_grad():
            out = net(d)
    finally:
        M.log_optimal_transport = orig
    return out['loss'].detach().numpy().astype(np.float64), cap['Z'].numpy(), d['gt_matches0'].numpy(), d['gt_matches1'].numpy()


def gen_case(M, arrays, case, B, n, m, L, S, k, methods, seed=0, first_pair=0, keep_Z=True, planted=None):
    sd = synth.make_state_dict(L=L, seed=seed)
    data = synth.make_batch(B, n, m, first_pair=first_pair)
    gt0, gt1 = ground_truth(data, first_pair)
    arrays[f'{case}_meta'] = np.array([B, n, m, L, S, seed, first_pair], dtype=np.int64)
    arrays[f'{case}_k'] = np.array([-1 if x is None else x for x in k], dtype=np.int64)
    arrays[f'{case}_gamma'] = np.array(GAMMA)
    arrays[f'{case}_gt0'], arrays[f'{case}_gt1'] = gt0.numpy(), gt1.numpy()
    plant_fn = None
    if planted is not None:
        plant_fn = lambda Z: plant(Z, gt0, gt1, np.random.RandomState(77), planted == 'inf')     # noqa: E731
    for meth in methods:
        cfg = synth.default_config(L=L, k=k, sinkhorn_iterations=S, loss_method=meth, triplet_loss_gamma=GAMMA)
        loss, Z, a0, a1 = run(M, cfg, sd, data, gt0, gt1, plant_fn)
        arrays[f'{case}_{meth}_loss'] = loss
        arrays[f'{case}_{meth}_gt0_after'], arrays[f'{case}_{meth}_gt1_after'] = a0, a1
        if keep_Z:
            arrays[f'{case}_Z'] = Z
    print(case, {meth: arrays[f'{case}_{meth}_loss'].tolist() for meth in methods},
          'matched rows', int((gt0 >= 0).sum()), 'of', gt0.numel())


def generate(M, out_dir):
    arrays = {}
    gen_case(M, arrays, 'n64', 2, 64, 64, 4, 20, SMALL_K, METHODS, first_pair=20)
    gen_case(M, arrays, 'n48m64', 2, 48, 64, 4, 20, SMALL_K, ('gap_loss',), first_pair=22)
    gen_case(M, arrays, 'b8n256', 8, 256, 256, 4, 20, synth.DEFAULT_K, METHODS, first_pair=30, keep_Z=False)
    gen_case(M, arrays, 'planted_sub', 1, 64, 64, 4, 20, SMALL_K, METHODS, first_pair=40, planted='sub')
    gen_case(M, arrays, 'planted_inf', 1, 64, 64, 4, 20, SMALL_K, METHODS, first_pair=41, planted='inf')
    np.savez_compressed(os.path.join(out_dir, NAME + '.npz'), **arrays)
    print('wrote', os.path.join(out_dir, NAME + '.npz'))


def main():
    check = '--check' in sys.argv[1:]
    torch.set_num_threads(synth.effective_cpu_count())
    M = G.import_reference()
    if not check:
        generate(M, G.OUT)
        return
    import shutil
    import tempfile
    tmp = tempfile.mkdtemp(prefix='mdgat_goldens_loss_')
    try:
        generate(M, tmp)
        bad = G.compare_dirs(tmp, G.OUT, [NAME])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for line in bad:
        print('MISMATCH', line)
    print(f'checked {NAME} against {G.OUT}: ' + ('OK' if not bad else f'{len(bad)} disagreements'))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
