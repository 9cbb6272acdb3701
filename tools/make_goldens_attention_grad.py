#!/usr/bin/env python3
"""Generate tests/golden/attention_grad_<case>.npz: the gradients autograd takes through the reference's own ``attention`` and
``dynamic_attention`` (models/mdgat.py:190-210), in fp64 on the CPU.  Runs where the reference exists (never on the GPU box); imports
it unmodified through the device shim of make_goldens.py.

Per case (tests/attention_grad_ref.py::CASES: full and dynamic, self and cross, 48 x 48 and 40 x 56 keypoints, k in {1, 16}, one with
two pairs) seeded fp64 q, k, v = randn * 1.3 in the reference's [B, 32, 4, n] layout and a seeded dmsg; every frame's queries go
through the reference function against their source frame's keys and values, ``(message * dmsg).sum().backward()``.  Recorded, in
the LIBRARY's layout: ``meta`` = [B, N, M, cross, k], ``qkv`` [B, N + M, 3, 4, 32], ``dmsg`` and ``msg`` [B, N + M, 128] (channel =
head * 32 + dim), ``dqkv``, and for k > 0 the reference's own top-k index sets as bit-packed masks ``mask0_bits`` / ``mask1_bits``
(the support of the ``prob`` it returns).  Record 2 (``gen_mha``, attention_grad_mha_{inputs,grads}.npz): one case through the
reference's whole ``MultiHeadedAttention.forward`` (mdgat.py:223-237; seeded weights, dynamic, cross) with the gradients of x, source,
the three ``proj`` weights and biases and ``merge`` - it pins the channel convention (the reference's channel = dim * 4 + head, the
library's head * 32 + dim).  Only recorded inputs and results.  One file per case: a case is ~0.7 MB, and no committed
file may exceed 1 MiB.

The generator REFUSES to write if, in any row of a dynamic case, the k-th and (k + 1)-th largest logits are closer than 1e-9
(where two correct implementations may select differently), the margin the other generators use for discrete choices.

    python tools/make_goldens_attention_grad.py [--check]
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
import attention_grad_ref as R  # noqa: E402
from mdgat_matcher_amd import synth  # noqa: E402

MARGIN = 1e-9


class Refused(Exception):
    pass


def to_ref(x):
    """library rows [B, n, 4, 32] -> the reference's [B, 32, 4, n]"""
    return torch.from_numpy(np.ascontiguousarray(np.transpose(x, (0, 3, 2, 1)))).requires_grad_()


def from_ref(t):
    """[B, 32, 4, n] -> [B, n, 4, 32]"""
    return np.transpose(t.detach().numpy().astype(np.float64), (0, 3, 2, 1))


def gen_case(M, case, B, N, Mm, cross, k, seed):
    rs = np.random.RandomState(seed)
    qkv = rs.standard_normal((B, N + Mm, 3, 4, 32)) * 1.3
    dmsg = rs.standard_normal((B, N + Mm, 128))
    if k > 0:
        _, gap = R.topk_masks(qkv, N, Mm, cross, k)
        if gap < MARGIN:
            raise Refused(f'{case}: the k-th and (k + 1)-th largest logits of a row are {gap:.3e} apart')
    msg, dqkv, masks = np.zeros((B, N + Mm, 128)), np.zeros_like(qkv), []
    frames = (slice(0, N), slice(N, N + Mm))
    for side in (0, 1):
        qs, ks = frames[side], frames[1 - side if cross else side]
        q, kk, v = to_ref(qkv[:, qs, 0]), to_ref(qkv[:, ks, 1]), to_ref(qkv[:, ks, 2])
        out, prob = M.dynamic_attention(q, kk, v, k) if k > 0 else M.attention(q, kk, v)
        g = torch.from_numpy(np.ascontiguousarray(np.transpose(dmsg[:, qs].reshape(B, -1, 4, 32), (0, 3, 2, 1))))
        (out * g).sum().backward()
        msg[:, qs] = from_ref(out).reshape(B, -1, 128)
        dqkv[:, qs, 0] += from_ref(q.grad)
        dqkv[:, ks, 1] += from_ref(kk.grad)
        dqkv[:, ks, 2] += from_ref(v.grad)
        if k > 0:
            mask = prob.detach().numpy() > 0            # [B, 4, n, m]: the scattered softmax is positive exactly on the index set
            assert (mask.sum(axis=-1) == k).all(), case
            masks.append(mask)
    arrays = {'meta': np.array([B, N, Mm, int(cross), k], dtype=np.int64), 'qkv': qkv, 'dmsg': dmsg, 'msg': msg, 'dqkv': dqkv}
    for i, mask in enumerate(masks):
        arrays[f'mask{i}_bits'] = np.packbits(mask.reshape(-1))
    print(case, {n: float(np.abs(a).max()) for n, a in arrays.items() if a.dtype == np.float64})
    return arrays


def gen_mha(M, B=1, n=40, m=56, k=8, seed=4200):
    """Record 2: the reference's whole MultiHeadedAttention.forward (mdgat.py:223-237), dynamic, one direction of a cross layer:
    seeded module weights, x [B, 128, n], source [B, 128, m], (out * dout).sum().backward().  Recorded point-major (x, source, dout,
    out and their gradients transposed to [B, points, 128]); the weights and their gradients as the reference holds them, channel
    c = dim * 4 + head."""
    torch.manual_seed(seed)
    mha = M.MultiHeadedAttention(4, 128).double()
    mha.prob = []
    rs = np.random.RandomState(seed)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s))          # noqa: E731
    with torch.no_grad():
        for conv in list(mha.proj) + [mha.merge]:
            conv.weight.copy_((t(128, 128, 1) * (1.6 / np.sqrt(128.0))))
            conv.bias.copy_(t(128) * 0.1)
    x, source, dout = t(B, 128, n).requires_grad_(), t(B, 128, m).requires_grad_(), t(B, 128, n)
    q, kk = (l(v).view(B, 32, 4, -1) for l, v in zip(mha.proj[:2], (x, source)))
    srt = (torch.einsum('bdhn,bdhm->bhnm', q, kk) / 32 ** .5).detach().sort(dim=-1, descending=True).values
    gap = float((srt[..., k - 1] - srt[..., k]).min())
    if gap < MARGIN:
        raise Refused(f'mha: the k-th and (k + 1)-th largest logits of a row are {gap:.3e} apart')
    out = mha(x, source, k)
    (out * dout).sum().backward()
    mask = mha.prob[-1].detach().numpy() > 0
    assert mask.shape == (B, 4, n, m) and (mask.sum(axis=-1) == k).all()
    f = lambda v: v.detach().numpy().astype(np.float64).copy()                           # noqa: E731
    pm = lambda v: np.ascontiguousarray(f(v).transpose(0, 2, 1))                          # noqa: E731
    inputs = {'meta': np.array([B, n, m, k], dtype=np.int64), 'x': pm(x), 'source': pm(source), 'dout': pm(dout), 'out': pm(out),
              'mask0_bits': np.packbits(mask.reshape(-1))}
    grads = {'dx': pm(x.grad), 'dsource': pm(source.grad)}
    for c, conv in zip('qkvm', list(mha.proj) + [mha.merge]):
        inputs['W' + c], inputs['b' + c] = f(conv.weight)[:, :, 0], f(conv.bias)
        grads['dW' + c], grads['db' + c] = f(conv.weight.grad)[:, :, 0], f(conv.bias.grad)
    print('mha', {a: float(np.abs(v).max()) for a, v in grads.items()})
    return dict(zip(R.MHA_FILES, (inputs, grads)))


def generate(M, out_dir):
    for name, arrays in gen_mha(M).items():
        path = os.path.join(out_dir, name + '.npz')
        np.savez_compressed(path, **arrays)
        print(f'wrote {path} ({os.path.getsize(path)} bytes)')
        assert os.path.getsize(path) < (1 << 20), path
    for i, (case, B, N, Mm, cross, k) in enumerate(R.CASES):
        arrays = gen_case(M, case, B, N, Mm, cross, k, seed=4100 + i)
        path = os.path.join(out_dir, f'attention_grad_{case}.npz')
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
        tmp = tempfile.mkdtemp(prefix='mdgat_goldens_attention_grad_')
        try:
            generate(M, tmp)
            bad = G.compare_dirs(tmp, G.OUT, list(R.GOLDEN_FILES + R.MHA_FILES))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    except Refused as e:
        print('REFUSED:', e)
        sys.exit(2)
    for line in bad:
        print('MISMATCH', line)
    print(f'checked attention_grad against {G.OUT}: ' + ('OK' if not bad else f'{len(bad)} disagreements'))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
