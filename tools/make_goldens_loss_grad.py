#!/usr/bin/env python3
"""Generate tests/golden/loss_grad.npz: the gradient autograd takes through the reference's own loss code (models/mdgat.py:486-594),
in fp64 on the CPU.  Runs where the reference exists (never on the GPU box); imports it unmodified through the device shim of
make_goldens.py.

The reference's forward runs WITH grad on the pairs of make_goldens_loss.py (synth frames, real ground truth); its
log_optimal_transport is wrapped to retain the gradient of its input scores and of its output Z, and ``(loss * w).sum().backward()``
is called with seeded weights w of the loss's own shape (0-d for superglue / triplet, [B] for gap).  Per case ``<case>_``: ``meta``
[B, n, m], ``gamma``, ``gt0`` / ``gt1`` (before the call), ``Z``, ``scores``, ``alpha``, ``iters``; per method ``<case>_<method>_w``,
``_dZ`` and - not for the planted cases, whose Z is overwritten behind the Sinkhorn - ``_dscores`` / ``_dalpha``.  Only recorded inputs
and results.

Cases: ``n64`` (B=2, every method), ``n48m64`` (gap only), ``planted_sub`` / ``planted_inf`` (make_goldens_loss.plant: entries in the
subnormal band of exp and below -745.2; one pair each).

Two correct implementations may differ discretely only where a clamp argument is 0 or a triplet row / column has tied largest
non-positive entries.  The generator REFUSES to write if, outside the planted cases, a clamp argument lies within 1e-9 of zero or
such a pair of entries is closer than 1e-9.

    python tools/make_goldens_loss_grad.py [--check]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import make_goldens as G  # noqa: E402
import make_goldens_loss as GL  # noqa: E402
from loss_grad_ref import clamp_margin, triplet_top_gap  # noqa: E402
from mdgat_matcher_amd import synth  # noqa: E402

NAME = 'loss_grad'
MARGIN = 1e-9
#        case,          B, n,  m,  methods,           first_pair, planted
CASES = (('n64',         2, 64, 64, GL.METHODS,        20, None),
         ('n48m64',      2, 48, 64, ('gap_loss',),     22, None),
         ('planted_sub', 1, 64, 64, GL.METHODS,        40, 'sub'),
         ('planted_inf', 1, 64, 64, GL.METHODS,        41, 'inf'))
L, S = 4, 20


class Refused(Exception):
    pass


def run(M, cfg, sd, data, gt0, gt1, w, planted=None):
    """The reference's forward with grad and (loss * w).sum().backward(): (scores, alpha, iters, Z, dscores, dalpha, dZ) as numpy."""
    net = G.build_ref_net(M, cfg, sd)
    d = {k: v.clone() for k, v in data.items()}
    d['gt_matches0'], d['gt_matches1'] = gt0.clone(), gt1.clone()
    orig = M.log_optimal_transport
    cap = {}

    def lot(scores, alpha, iters):
        scores.retain_grad()
        if not alpha.is_leaf:
            alpha.retain_grad()
        Z = orig(scores, alpha, iters)
        if planted is not None:
            Z = planted(Z)
        Z.retain_grad()
        cap.update(scores=scores, alpha=alpha, iters=iters, Z=Z)
        return Z
    M.log_optimal_transport = lot
    try:
        out = net(d)
    finally:
        M.log_optimal_transport = orig
    loss = out['loss']
    assert tuple(loss.shape) == tuple(w.shape), (loss.shape, w.shape)
    (loss * torch.from_numpy(np.asarray(w))).sum().backward()
    f = lambda x: x.detach().numpy().astype(np.float64).copy()      # noqa: E731
    return (f(cap['scores']), f(cap['alpha']), int(cap['iters']), f(cap['Z']), f(cap['scores'].grad), f(cap['alpha'].grad), f(cap['Z'].grad))


def gen_case(M, arrays, case, B, n, m, methods, first_pair, planted, seed=0):
    sd = synth.make_state_dict(L=L, seed=seed)
    data = synth.make_batch(B, n, m, first_pair=first_pair)
    gt0, gt1 = GL.ground_truth(data, first_pair)
    plant_fn = None
    if planted is not None:
        plant_fn = lambda Z: GL.plant(Z, gt0, gt1, np.random.RandomState(77), planted == 'inf')     # noqa: E731
    rs = np.random.RandomState(1000 + first_pair)
    arrays[f'{case}_meta'] = np.array([B, n, m], dtype=np.int64)
    arrays[f'{case}_gamma'] = np.array(GL.GAMMA)
    arrays[f'{case}_gt0'], arrays[f'{case}_gt1'] = gt0.numpy(), gt1.numpy()
    for meth in methods:
        cfg = synth.default_config(L=L, k=GL.SMALL_K, sinkhorn_iterations=S, loss_method=meth, triplet_loss_gamma=GL.GAMMA)
        w = np.asarray(np.round(rs.uniform(0.5, 2.0, (B,) if meth == 'gap_loss' else ()) * 256) / 256)
        scores, alpha, iters, Z, dscores, dalpha, dZ = run(M, cfg, sd, data, gt0, gt1, w, plant_fn)
        if planted is None:
            for b in range(B):
                cm = clamp_margin(Z[b:b + 1], gt0.numpy()[b:b + 1], gt1.numpy()[b:b + 1], meth, GL.GAMMA)
                if cm < MARGIN:
                    raise Refused(f'{case} {meth} pair {b}: a clamp argument lies within {cm:.3e} of zero')
                tg = triplet_top_gap(Z[b:b + 1], gt0.numpy()[b:b + 1], gt1.numpy()[b:b + 1]) if meth == 'triplet_loss' else np.inf
                if tg < MARGIN:
                    raise Refused(f'{case} {meth} pair {b}: the two largest non-positive entries of a row / column are {tg:.3e} apart')
        for key, val in (('Z', Z), ('scores', scores), ('alpha', alpha), ('iters', np.int64(iters))):
            if f'{case}_{key}' in arrays:
                assert np.array_equal(arrays[f'{case}_{key}'], val), (case, meth, key)       # the method only selects the loss branch
            arrays[f'{case}_{key}'] = val
        arrays[f'{case}_{meth}_w'], arrays[f'{case}_{meth}_dZ'] = w, dZ
        if planted is None:
            arrays[f'{case}_{meth}_dscores'], arrays[f'{case}_{meth}_dalpha'] = dscores, dalpha
        print(case, meth, 'w', w.tolist(), 'max|dZ|', float(np.nanmax(np.abs(np.where(np.isfinite(dZ), dZ, 0.0)))),
              'non-finite', int((~np.isfinite(dZ)).sum()))


def generate(M, out_dir):
    arrays = {}
    for case in CASES:
        gen_case(M, arrays, *case)
    path = os.path.join(out_dir, NAME + '.npz')
    np.savez_compressed(path, **arrays)
    print(f'wrote {path} ({os.path.getsize(path)} bytes)')


def main():
    check = '--check' in sys.argv[1:]
    torch.set_num_threads(synth.effective_cpu_count())
    M = G.import_reference()
    try:
        if not check:
            generate(M, G.OUT)
            return
        import shutil
        import tempfile
        tmp = tempfile.mkdtemp(prefix='mdgat_goldens_loss_grad_')
        try:
            generate(M, tmp)
            bad = G.compare_dirs(tmp, G.OUT, [NAME])
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    except Refused as e:
        print('REFUSED:', e)
        sys.exit(2)
    for line in bad:
        print('MISMATCH', line)
    print(f'checked {NAME} against {G.OUT}: ' + ('OK' if not bad else f'{len(bad)} disagreements'))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
