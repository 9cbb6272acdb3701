#!/usr/bin/env python3
"""Generate tests/golden/sk_grad.npz: the gradient of the reference's own log_optimal_transport (models/mdgat.py:279-308), by torch
autograd in fp64 on the CPU.  Runs where the reference exists (never on the GPU box); imports it unmodified through the device shim
of make_goldens.py.

Per case ``<case>_``: ``scores`` [B, N, M], ``alpha`` (0-d), ``iters`` (0-d), ``dZ`` [B, N+1, M+1] (seeded), and the reference's
``dscores`` [B, N, M] and ``dalpha`` (0-d: the bin score is one parameter shared by the batch, mdgat.py:359-360).  Scores and dZ are
drawn on grids (multiples of 2^-6 and 2^-8) so that the inputs compress; the gradients are full fp64.

Cases: ``b2n64m48`` (T = 100, scores in +-100), ``n120m180`` (T = 50, a dustbin-heavy pair: alpha above most scores), ``n7m5``
(T = 3).

    python tools/make_goldens_grad.py [--check]
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

NAME = 'sk_grad'
CASES = (('b2n64m48', 2, 64, 48, 100, 100.0, 1.0, 11),
         ('n120m180', 1, 120, 180, 50, 3.0, 2.5, 12),
         ('n7m5', 1, 7, 5, 3, 2.0, 0.3, 13))


def gen(M):
    arrays = {}
    for name, B, n, m, T, spread, alpha, seed in CASES:
        rs = np.random.RandomState(seed)
        scores = np.round(rs.uniform(-spread, spread, (B, n, m)) * 64) / 64
        dZ = np.round(rs.standard_normal((B, n + 1, m + 1)) * 256) / 256
        s = torch.from_numpy(scores).requires_grad_(True)
        al = torch.tensor(alpha, dtype=torch.float64, requires_grad=True)
        Z = M.log_optimal_transport(s, al, T)
        (Z * torch.from_numpy(dZ)).sum().backward()
        arrays.update({f'{name}_scores': scores, f'{name}_alpha': np.float64(alpha), f'{name}_iters': np.int64(T), f'{name}_dZ': dZ,
                       f'{name}_dscores': s.grad.numpy(), f'{name}_dalpha': al.grad.numpy()})
    return arrays


def main():
    M = G.import_reference()
    arrays = gen(M)
    path = os.path.join(G.OUT, NAME + '.npz')
    if '--check' in sys.argv:
        old = np.load(path)
        bad = [k for k in arrays if k not in old.files or not np.allclose(arrays[k], old[k], rtol=1e-12, atol=0)]
        print('sk_grad: ' + ('OK' if not bad else 'differs in ' + ', '.join(bad)))
        sys.exit(1 if bad else 0)
    np.savez_compressed(path, **arrays)
    print(f'wrote {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    main()
