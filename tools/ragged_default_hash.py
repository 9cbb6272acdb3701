#!/usr/bin/env python3
"""One SHA-256 over the output bytes of the calls a change to the fp32 Sinkhorn must leave alone, for comparing two builds of the library
("The split form"):  python tools/ragged_default_hash.py [--lib path/to/libmdgat_hip.so]

Seeded, on one GPU: ``forward_ragged`` with Z of a float32 module WITHOUT config['ragged_sinkhorn_fp32'] on the two chunks of
tests/ragged_split_cases.py (slots 130 x 70 and 512 x 500, at 1, 2, 3, 20 and 100 iterations), ``ops.sinkhorn`` and
``ops.sinkhorn_extract`` with counts on the first chunk's slot, and a uniform ``forward`` of four pairs of 130 x 70.  Prints the digest of
every part and the digest over all of them."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from mdgat_matcher_amd import MDGAT, _lib, ops, synth  # noqa: E402


def leaves(x):
    if isinstance(x, torch.Tensor):
        yield x
    elif isinstance(x, dict):
        for k in sorted(x):
            yield from leaves(x[k])
    elif isinstance(x, (tuple, list)):
        for v in x:
            yield from leaves(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None, help='another build of libmdgat_hip.so (default: the package\'s own)')
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import ragged_split_cases as CASES
    dev = 'cuda:0'
    whole = hashlib.sha256()

    def add(name, out):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in leaves(out):
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
        whole.update(h.digest())
        print(f'{name}: {h.hexdigest()}')

    with torch.no_grad():
        for name in sorted(CASES.CHUNKS):
            for iters in CASES.ITERS[name]:
                net = MDGAT({**CASES.cfg(iters), 'ragged_arithmetic': 'auto'})
                net.load_state_dict(CASES.state_dict())
                net = net.float().eval().to(dev)
                add(f'forward_ragged {name} iters={iters}', net.forward_ragged(list(CASES.pairs(name, dev)), return_Z=True))
        counts = CASES.CHUNKS['A']
        rs = np.random.RandomState(7)
        s = torch.from_numpy(rs.standard_normal((len(counts), 130, 70)).astype(np.float32) * 3.0).to(dev)
        h0, h1 = (torch.tensor([c[f] for c in counts], dtype=torch.int32) for f in (0, 1))
        cnt = {'counts0_host': h0, 'counts1_host': h1, 'counts0': h0.to(dev), 'counts1': h1.to(dev)}
        add('ops.sinkhorn counts', ops.sinkhorn(s, 1.0, 20, counts=cnt))
        add('ops.sinkhorn_extract counts', ops.sinkhorn_extract(s, 1.0, 20, counts=cnt))
        net = MDGAT(CASES.cfg(20))
        net.load_state_dict(CASES.state_dict())
        net = net.float().eval().to(dev)
        out = net(synth.make_batch(4, 130, 70, device=dev))
        add('uniform forward', {k: v for k, v in out.items() if isinstance(v, torch.Tensor)})
    print(f'library {_lib.LIB_PATH}\nall: {whole.hexdigest()}')


if __name__ == '__main__':
    main()
