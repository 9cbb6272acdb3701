#!/usr/bin/env python3
"""Generate tests/golden/head_grad*.npz: the gradients autograd takes through the reference's own matching head (models/mdgat.py:397
final_proj, 430-431 the score matrix) on the way back from its loss, in fp64 on the CPU.  Runs where the reference exists (never on
the GPU box); imports it unmodified through the device shim of make_goldens.py.

The reference's forward runs WITH grad on the pairs of make_goldens_loss.py (synth frames, real ground truth).  A forward hook on
``final_proj`` keeps its two inputs (the GNN's output descriptors of frame 0 and frame 1, ``retain_grad``), log_optimal_transport is
wrapped to retain the gradient of its input scores, and ``(loss * w).sum().backward()`` is called with seeded weights w of the loss's
own shape (0-d for superglue / triplet, [B] for gap).  Recorded per case ``<case>_``: ``meta`` [B, n, m], ``gamma``, ``gt0`` / ``gt1``,
``desc0`` [B, n, 128] / ``desc1`` [B, m, 128] (point-major, the library's layout: the reference's [B, 128, n] transposed), ``W``
[128, 128], ``b``, ``scores``, ``alpha``, ``iters``; per method ``<case>_<method>_`` ``w``, ``dscores``, ``ddesc0``, ``ddesc1``,
``dW``, ``db``, ``dalpha``.  Only recorded inputs and results.

Cases: ``n64`` (B=2, every method), ``n48m64`` (B=2, gap only); L = 4, S = 20.  The inputs of both go to head_grad.npz, each (case,
method)'s gradients to head_grad_<case>_<method>.npz (tests/head_grad_ref.py::load_golden reads them as one dict): a pair of 64
keypoints is 64 KB per descriptor array, and no committed file may exceed 1 MiB.

The generator REFUSES to write if a clamp argument of a loss lies within 1e-9 of zero or the two largest non-positive entries of a
triplet row / column are closer than 1e-9 (where two correct implementations may differ discretely), as make_goldens_loss_grad.py.

    python tools/make_goldens_head_grad.py [--check]
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
from head_grad_ref import GOLDEN_FILES  # noqa: E402
from loss_grad_ref import clamp_margin, triplet_top_gap  # noqa: E402
from mdgat_matcher_amd import synth  # noqa: E402

NAME = 'head_grad'
MARGIN = 1e-9
#        case,     B, n,  m,  methods,       first_pair
CASES = (('n64',    2, 64, 64, GL.METHODS,    20),
         ('n48m64', 2, 48, 64, ('gap_loss',), 22))
L, S = 4, 20


class Refused(Exception):
    pass


def run(M, cfg, sd, data, gt0, gt1, w):
    """The reference's forward with grad and (loss * w).sum().backward(): a dict of numpy float64 arrays."""
    net = G.build_ref_net(M, cfg, sd)
    d = {k: v.clone() for k, v in data.items()}
    d['gt_matches0'], d['gt_matches1'] = gt0.clone(), gt1.clone()
    orig = M.log_optimal_transport
    cap = {'desc': []}

    def keep_input(mod, inp):
        inp[0].retain_grad()
        cap['desc'].append(inp[0])
    hook = net.final_proj.register_forward_pre_hook(keep_input)

    def lot(scores, alpha, iters):
        scores.retain_grad()
        Z = orig(scores, alpha, iters)
        cap.update(scores=scores, iters=iters, Z=Z)
        return Z
    M.log_optimal_transport = lot
    try:
        out = net(d)
    finally:
        M.log_optimal_transport = orig
        hook.remove()
    loss = out['loss']
    assert tuple(loss.shape) == tuple(w.shape), (loss.shape, w.shape)
    assert len(cap['desc']) == 2
    (loss * torch.from_numpy(np.asarray(w))).sum().backward()
    f = lambda x: x.detach().numpy().astype(np.float64).copy()                         # noqa: E731
    pm = lambda x: np.ascontiguousarray(f(x).transpose(0, 2, 1))                        # noqa: E731  [B, 128, n] -> [B, n, 128]
    d0, d1 = cap['desc']
    fp = net.final_proj
    return {'desc0': pm(d0), 'desc1': pm(d1), 'W': f(fp.weight)[:, :, 0], 'b': f(fp.bias), 'scores': f(cap['scores']),
            'alpha': f(net.bin_score), 'iters': np.int64(cap['iters']), 'Z': f(cap['Z']),
            'dscores': f(cap['scores'].grad), 'ddesc0': pm(d0.grad), 'ddesc1': pm(d1.grad), 'dW': f(fp.weight.grad)[:, :, 0],
            'db': f(fp.bias.grad), 'dalpha': f(net.bin_score.grad)}


def gen_case(M, files, case, B, n, m, methods, first_pair, seed=0):
    sd = synth.make_state_dict(L=L, seed=seed)
    data = synth.make_batch(B, n, m, first_pair=first_pair)
    gt0, gt1 = GL.ground_truth(data, first_pair)
    rs = np.random.RandomState(1000 + first_pair)
    inputs = files[NAME]
    inputs[f'{case}_meta'] = np.array([B, n, m], dtype=np.int64)
    inputs[f'{case}_gamma'] = np.array(GL.GAMMA)
    inputs[f'{case}_gt0'], inputs[f'{case}_gt1'] = gt0.numpy(), gt1.numpy()
    for meth in methods:
        cfg = synth.default_config(L=L, k=GL.SMALL_K, sinkhorn_iterations=S, loss_method=meth, triplet_loss_gamma=GL.GAMMA)
        w = np.asarray(np.round(rs.uniform(0.5, 2.0, (B,) if meth == 'gap_loss' else ()) * 256) / 256)
        r = run(M, cfg, sd, data, gt0, gt1, w)
        Z = r.pop('Z')
        for b in range(B):
            cm = clamp_margin(Z[b:b + 1], gt0.numpy()[b:b + 1], gt1.numpy()[b:b + 1], meth, GL.GAMMA)
            if cm < MARGIN:
                raise Refused(f'{case} {meth} pair {b}: a clamp argument lies within {cm:.3e} of zero')
            tg = triplet_top_gap(Z[b:b + 1], gt0.numpy()[b:b + 1], gt1.numpy()[b:b + 1]) if meth == 'triplet_loss' else np.inf
            if tg < MARGIN:
                raise Refused(f'{case} {meth} pair {b}: the two largest non-positive entries of a row / column are {tg:.3e} apart')
        assert r['desc0'].shape == (B, n, 128) and r['desc1'].shape == (B, m, 128) and r['scores'].shape == (B, n, m)
        for key in ('desc0', 'desc1', 'W', 'b', 'scores', 'alpha', 'iters'):
            val = r.pop(key)
            if f'{case}_{key}' in inputs:
                assert np.array_equal(inputs[f'{case}_{key}'], val), (case, meth, key)       # the method only selects the loss branch
            inputs[f'{case}_{key}'] = val
        grads = files[f'{NAME}_{case}_{meth}'] = {f'{case}_{meth}_w': w}
        for key, val in r.items():
            grads[f'{case}_{meth}_{key}'] = val
        print(case, meth, 'w', w.tolist(), {k: float(np.abs(v).max()) for k, v in r.items()})


def generate(M, out_dir):
    files = {NAME: {}}
    for case in CASES:
        gen_case(M, files, *case)
    assert tuple(files) == GOLDEN_FILES, tuple(files)
    for name, arrays in files.items():
        path = os.path.join(out_dir, name + '.npz')
        np.savez_compressed(path, **arrays)
        print(f'wrote {path} ({os.path.getsize(path)} bytes)')
        assert os.path.getsize(path) < (1 << 20), path


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
        tmp = tempfile.mkdtemp(prefix='mdgat_goldens_head_grad_')
        try:
            generate(M, tmp)
            bad = G.compare_dirs(tmp, G.OUT, list(GOLDEN_FILES))
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
