"""One SHA-256 over what a descriptor='FPFH' module computes on the recorded 'gap' training case (tests/golden/train_gap_io.npz): the
eval() ``forward`` and ``match`` outputs, then one train() ``training_forward`` with ``loss.mean().backward()`` - loss, matches, scores,
every gradient and every buffer.  tests/test_gpu_descriptors.py compares it with the digest recorded from the build before the
FPFH_gloabal / FPFH_only encoders were added: the default descriptor computes the same bits."""
import hashlib
import os

import numpy as np
import torch

import train_ref as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
INPUT_KEYS = ('keypoints0', 'scores0', 'descriptors0', 'keypoints1', 'scores1', 'descriptors1', 'gt_matches0', 'gt_matches1')


def fpfh_digest(device='cuda:0'):
    from mdgat_matcher_amd import MDGAT
    case = T.load(GOLDEN, 'gap')
    data = lambda: {k: torch.from_numpy(np.ascontiguousarray(case['data'][k])).to(device) for k in INPUT_KEYS}      # noqa: E731
    net = MDGAT(T.config('gap_loss')).double()
    net.load_state_dict(T.initial_state())
    net = net.to(device).eval()
    h = hashlib.sha256()

    def add(name, t):
        a = t.detach().cpu().contiguous().numpy()
        h.update(name.encode() + str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    d = data()
    with torch.no_grad():
        out = net(d)
        m = net.match(d['keypoints0'], d['descriptors0'], d['keypoints1'], d['descriptors1'], d['scores0'], d['scores1'], return_scores=True)
    torch.cuda.synchronize()
    for k in ('matches0', 'matches1', 'matching_scores0', 'matching_scores1'):
        add('forward:' + k, out[k])
    for i, t in enumerate(m):
        add(f'match:{i}', t)
    net.train()
    out = net.training_forward(data())
    out['loss'].mean().backward()
    torch.cuda.synchronize()
    for k in ('matches0', 'matches1', 'matching_scores0', 'matching_scores1', 'loss'):
        add('train:' + k, out[k])
    for k, p in net.named_parameters():
        add('grad:' + k, p.grad)
    for k, b in net.named_buffers():
        add('buf:' + k, b)
    return h.hexdigest()
