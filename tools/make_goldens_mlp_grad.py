#!/usr/bin/env python3
"""Generate tests/golden/mlp_grad_<case>.npz: what the reference's own ``MLP`` stacks (models/mdgat.py:34-46) compute in
``.double().train()`` and what autograd takes through them, on the CPU.  Runs where the reference exists (never on the GPU box);
imports it unmodified through the device shim of make_goldens.py.

Cases (tests/mlp_grad_ref.py::GOLDEN_FILES):

* ``kenc``       ``KeypointEncoder(128, [32, 64, 128])`` called for frame 0 and then frame 1, as mdgat.py:392-393 does: the buffers move
                 twice.  2 pairs of 24 (frame 0) and 30 (frame 1) keypoints.
* ``denc``       ``DescriptorEncoder(128, [64, 128])``, likewise.
* ``denc_eval``  the same module in ``.eval()``: the running statistics stand in and do not move.
* ``layer``      ``AttentionalPropagation(128, 4).mlp`` on ``cat([x, message])``, one call of 2 x 26 points (two files: the weights alone
                 are 0.8 MB and no committed file may exceed 1 MiB).

* ``prop_self`` / ``prop_cross``  one whole ``AttentionalPropagation(128, 4).forward`` in training mode, called for frame 0 and then
                 frame 1 as ``AttentionalGNN.forward`` calls it (mdgat.py:259-276): self with ``k=None``, cross with ``k=8``; two pairs
                 of 20 x 28 points.  Both modes share the seeded weights (``mlp_grad_prop_weights_{attn,mlp}``); per mode the inputs,
                 douts, outputs, input gradients, top-k index sets (bit-packed) and the buffers afterwards (``_io``) and autograd's
                 parameter gradients (``_grads_attn``, ``_grads_mlp``).  The attention's weights are recorded as the reference holds them
                 (channel = dim * 4 + head).  ``_io`` also holds ``err_<quantity>``: the reference's own error per quantity, measured against
                 an evaluation of the layer in x86's 80-bit format (tests/mlp_grad_ref.py explains the bound built on it).  Refused as
                 well when a row's k-th and (k + 1)-th largest logits are closer than 1e-9.

Seeded: the weights (1.6 / sqrt(C_in) randn), gamma, beta and the running buffers (mlp_grad_ref.random_params), the inputs and a dout
per frame.  Recorded, arrays only, point-major (the reference's [B, C, P] transposed and flattened to rows): per frame ``x_f<i>``,
``dout_f<i>``, ``out_f<i>``, ``dx_f<i>``; the parameters ``W<l>``, ``b<l>``, ``gamma<l>``, ``beta<l>`` and the buffers BEFORE the calls
``rm<l>``, ``rv<l>``; ``eps``, ``momentum``; autograd's gradients of sum over the frames of ``(out * dout).sum()``: ``dW<l>``, ``db<l>``,
``dgamma<l>``, ``dbeta<l>``; the buffers afterwards ``rm_after<l>``, ``rv_after<l>``, ``nbt_after``.

The generator REFUSES to write a case whose ReLU is not decided: the smallest |z| of any BN layer must exceed its error bound
(mlp_grad_ref.relu_margin) by 1e3 in every frame.

    python tools/make_goldens_mlp_grad.py [--check]
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
import mlp_grad_ref as R  # noqa: E402
from mdgat_matcher_amd import synth  # noqa: E402

MARGIN = 1e3


class Refused(Exception):
    pass


def set_params(seq, p):
    convs = [m for m in seq if isinstance(m, torch.nn.Conv1d)]
    bns = [m for m in seq if isinstance(m, torch.nn.BatchNorm1d)]
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))          # noqa: E731
    with torch.no_grad():
        for l, c in enumerate(convs):
            c.weight.copy_(t(p['W'][l])[:, :, None])
            c.bias.copy_(t(p['b'][l]))
        for l, b in enumerate(bns):
            b.weight.copy_(t(p['gamma'][l]))
            b.bias.copy_(t(p['beta'][l]))
            b.running_mean.copy_(t(p['rm'][l]))
            b.running_var.copy_(t(p['rv'][l]))
            p['eps'][l], p['momentum'][l] = b.eps, b.momentum
    return convs, bns


def record(case, seq, call, xs, douts, p, training):
    """call(x_rows_as [B, P, K] tensor) -> the module's output [B, C, P]; xs: per frame [B, P, K]."""
    seq.double()
    seq.train(training)
    convs, bns = set_params(seq, p)
    arrays = {'n_conv': np.int64(len(convs)), 'n_frames': np.int64(len(xs)), 'training': np.int64(training),
              'eps': np.array(p['eps']), 'momentum': np.array(p['momentum'])}
    for l in range(len(convs)):
        arrays[f'W{l}'], arrays[f'b{l}'] = p['W'][l], p['b'][l]
    for l in range(len(bns)):
        for k in ('gamma', 'beta', 'rm', 'rv'):
            arrays[f'{k}{l}'] = np.array(p[k][l])
    q = {k: list(v) for k, v in p.items()}
    loss, ins = 0.0, []
    for i, (x, dout) in enumerate(zip(xs, douts)):
        margin = R.relu_margin(x.reshape(-1, x.shape[-1]), q, training)
        if margin < MARGIN:
            raise Refused(f'{case}: frame {i}: the smallest |z| is only {margin:.3e} x its bound')
        _, _, (q['rm'], q['rv']) = R.forward(x.reshape(-1, x.shape[-1]), q, training)
        xt = torch.from_numpy(x).requires_grad_()
        out = call(xt)                                                  # [B, C, P]
        loss = loss + (out * torch.from_numpy(np.ascontiguousarray(dout.transpose(0, 2, 1)))).sum()
        ins.append(xt)
        arrays[f'x_f{i}'] = x.reshape(-1, x.shape[-1])
        arrays[f'dout_f{i}'] = dout.reshape(-1, dout.shape[-1])
        arrays[f'out_f{i}'] = out.detach().numpy().transpose(0, 2, 1).reshape(-1, out.shape[1]).copy()
    loss.backward()
    for i, xt in enumerate(ins):
        arrays[f'dx_f{i}'] = xt.grad.numpy().reshape(-1, xt.shape[-1]).copy()
    f = lambda v: v.detach().numpy().astype(np.float64).copy()            # noqa: E731
    for l, c in enumerate(convs):
        arrays[f'dW{l}'], arrays[f'db{l}'] = f(c.weight.grad)[:, :, 0], f(c.bias.grad)
    for l, b in enumerate(bns):
        arrays[f'dgamma{l}'], arrays[f'dbeta{l}'] = f(b.weight.grad), f(b.bias.grad)
        arrays[f'rm_after{l}'], arrays[f'rv_after{l}'] = f(b.running_mean), f(b.running_var)
    arrays['nbt_after'] = np.array([int(b.num_batches_tracked) for b in bns], dtype=np.int64)
    print(case, {n: float(np.abs(a).max()) for n, a in arrays.items() if n.startswith(('out', 'dx', 'dW'))})
    return arrays


def cases(M):
    out = {}
    rs = np.random.RandomState(5100)
    frames = lambda k, c: ([rs.standard_normal((2, n, k)) for n in (24, 30)], [rs.standard_normal((2, n, c)) for n in (24, 30)])   # noqa: E731
    kenc = M.KeypointEncoder(128, [32, 64, 128])
    xs, douts = frames(4, 128)
    out['kenc'] = record('kenc', kenc.encoder, lambda x: kenc(x[:, :, :3], x[:, :, 3]), xs, douts, R.random_params(R.STACKS['kenc'], 5101), True)
    for case, training, seed in (('denc', True, 5102), ('denc_eval', False, 5103)):
        denc = M.DescriptorEncoder(128, [64, 128])
        xs, douts = frames(33, 128)
        out[case] = record(case, denc.encoder, lambda x: denc(x), xs, douts, R.random_params(R.STACKS['denc'], seed), training)
    layer = M.AttentionalPropagation(128, 4)
    x, msg, dout = rs.standard_normal((2, 26, 128)), rs.standard_normal((2, 26, 128)), rs.standard_normal((2, 26, 128))
    call = lambda xt: layer.mlp(torch.cat([xt[:, :, :128].transpose(1, 2), xt[:, :, 128:].transpose(1, 2)], dim=1))      # noqa: E731
    out['layer'] = record('layer', layer.mlp, call, [np.concatenate([x, msg], axis=2)], [dout], R.random_params(R.STACKS['layer'], 5104), True)
    return out


def prop_cases(M):
    """-> {file name: arrays} of the whole-layer records."""
    import attention_grad_ref as A
    B, n, m = 2, 20, 28
    torch.manual_seed(5200)
    layer = M.AttentionalPropagation(128, 4).double().train()
    rs = np.random.RandomState(5200)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s))          # noqa: E731
    convs = dict(zip('qkvm', list(layer.attn.proj) + [layer.attn.merge]))
    with torch.no_grad():
        for conv in convs.values():
            conv.weight.copy_(t(128, 128, 1) * (1.6 / np.sqrt(128.0)))
            conv.bias.copy_(t(128) * 0.1)
    p = R.random_params(R.STACKS['layer'], 5201)
    mlp_convs, bns = set_params(layer.mlp, p)
    f = lambda v: v.detach().numpy().astype(np.float64).copy()            # noqa: E731
    pm = lambda v: np.ascontiguousarray(f(v).transpose(0, 2, 1))           # noqa: E731
    w = {}
    for c, conv in convs.items():
        w['W' + c], w['b' + c] = f(conv.weight)[:, :, 0], f(conv.bias)
    files = {'mlp_grad_prop_weights_attn': dict(w),
             'mlp_grad_prop_weights_mlp': {'W0': p['W'][0], 'b0': p['b'][0], 'W1': p['W'][1], 'b1': p['b'][1], 'gamma0': p['gamma'][0],
                                           'beta0': p['beta'][0], 'rm0': np.array(p['rm'][0]), 'rv0': np.array(p['rv'][0]),
                                           'eps': np.array(p['eps']), 'momentum': np.array(p['momentum'])}}
    state = {k: v.clone() for k, v in layer.state_dict().items()}
    for mode, (cross, k) in R.PROP_MODES.items():
        layer.load_state_dict(state)
        layer.zero_grad(set_to_none=True)
        layer.attn.prob = []
        d0, d1 = t(B, 128, n).requires_grad_(), t(B, 128, m).requires_grad_()
        g0, g1 = t(B, 128, n), t(B, 128, m)
        if k > 0:
            own, gap = A.topk_masks(A.mha_qkv(pm(d0), pm(d1), w)[1], n, m, cross, k)
            if gap < 1e-9:
                raise Refused(f'prop_{mode}: the k-th and (k + 1)-th largest logits of a row are {gap:.3e} apart')
        out0 = layer(d0, d1 if cross else d0, k if k > 0 else None)
        out1 = layer(d1, d0 if cross else d1, k if k > 0 else None)
        ((out0 * g0).sum() + (out1 * g1).sum()).backward()
        io = {'desc0': pm(d0), 'desc1': pm(d1), 'dout0': pm(g0), 'dout1': pm(g1), 'out0': pm(out0), 'out1': pm(out1),
              'ddesc0': pm(d0.grad), 'ddesc1': pm(d1.grad), 'rm_after0': f(bns[0].running_mean), 'rv_after0': f(bns[0].running_var),
              'nbt_after': np.array([int(bns[0].num_batches_tracked)], dtype=np.int64)}
        masks = None
        if k > 0:
            masks = tuple(pr.detach().numpy() > 0 for pr in layer.attn.prob)
            assert all((mk.sum(axis=-1) == k).all() for mk in masks) and all(np.array_equal(a, b) for a, b in zip(masks, own))
            for i, mk in enumerate(masks):
                io[f'mask{i}_bits'] = np.packbits(mk.reshape(-1))
        ga = {}
        for c, conv in convs.items():
            ga['dW' + c], ga['db' + c] = f(conv.weight.grad)[:, :, 0], f(conv.bias.grad)
        gm = {'dW0': f(mlp_convs[0].weight.grad)[:, :, 0], 'db0': f(mlp_convs[0].bias.grad), 'dW1': f(mlp_convs[1].weight.grad)[:, :, 0],
              'db1': f(mlp_convs[1].bias.grad), 'dgamma0': f(bns[0].weight.grad), 'dbeta0': f(bns[0].bias.grad)}
        # the reference's own error, measured against an 80-bit evaluation (mlp_grad_ref: the section's comment), and the ReLU condition on it
        case = {'desc0': io['desc0'], 'desc1': io['desc1'], 'dout0': io['dout0'], 'dout1': io['dout1'], 'w': w, 'p': p, 'cross': cross, 'masks': masks}
        recorded = dict(io, **ga, **gm, rm0=io['rm_after0'], rv0=io['rv_after0'])
        err = R.prop_reference_error(case, recorded)
        margin = R.prop_relu_margin(case, err)
        if margin < MARGIN:
            raise Refused(f'prop_{mode}: the smallest |z| is only {margin:.3e} x its bound')
        for q, e in err.items():
            io['err_' + q] = np.float64(e)
        files.update(dict(zip(R.PROP_FILES[mode], (io, ga, gm))))
        rel = {q: e / max(float(np.abs(recorded[q]).max()), 1e-300) for q, e in err.items() if q in recorded}
        print(f'prop_{mode}: relu margin {margin:.2e}; err / max|value|:', {q: float(f'{v:.1e}') for q, v in rel.items()})
    return files


def generate(M, out_dir):
    for name, part in prop_cases(M).items():
        path = os.path.join(out_dir, name + '.npz')
        np.savez_compressed(path, **part)
        print(f'wrote {path} ({os.path.getsize(path)} bytes)')
        assert os.path.getsize(path) < (1 << 20), path
    for case, arrays in cases(M).items():
        names = R.GOLDEN_FILES[case]
        if len(names) == 1:
            parts = [arrays]
        else:           # inputs | gradients
            grad = lambda k: k.startswith(('dW', 'db', 'dgamma', 'dbeta', 'dx_'))      # noqa: E731
            parts = [{k: v for k, v in arrays.items() if not grad(k)}, {k: v for k, v in arrays.items() if grad(k)}]
        for name, part in zip(names, parts):
            path = os.path.join(out_dir, name + '.npz')
            np.savez_compressed(path, **part)
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
        tmp = tempfile.mkdtemp(prefix='mdgat_goldens_mlp_grad_')
        try:
            generate(M, tmp)
            bad = G.compare_dirs(tmp, G.OUT, list(R.ALL_FILES))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    except Refused as e:
        print('REFUSED:', e)
        sys.exit(2)
    for line in bad:
        print('MISMATCH', line)
    print(f'checked mlp_grad against {G.OUT}: ' + ('OK' if not bad else f'{len(bad)} disagreements'))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
