#!/usr/bin/env python3
"""Generate tests/golden/train_*.npz: one whole training step of the reference's own ``MDGAT`` (models/mdgat.py:369-603) -
``net.double().train()``, one forward, ``loss.mean().backward()`` (train.py:222, 234-245) - in fp64 on the CPU.  Runs where the reference
exists (never on the GPU box); imports it unmodified through the device shim of make_goldens.py.

The net (tests/train_ref.py: L = 1 - layer 0 self and full, layer 1 cross with k = 8 -, 20 Sinkhorn iterations) takes its weights from
``synth.make_state_dict(L, SEED)``, loaded after ``.double()``: the weights are not stored, the seed is.  The pairs are synth.make_batch's
with make_goldens_loss.ground_truth's gts.  Every array is stored under a prefixed name: ``in:<key>`` the inputs, ``r:<quantity>`` the
reference's result, ``e:<quantity>`` the measured error of that quantity (train_ref.reference_error), ``nbt:<buffer>`` the
num_batches_tracked afterwards; quantities are ``loss``, ``Z``, ``grad:<parameter>``, ``buf:<running_mean / running_var>``.

* ``gap``        2 pairs of 20 x 28, gap_loss: the inputs, loss, Z, matches and scores, every buffer (``train_gap_io``) and every
                 parameter's gradient (``train_gap_grads_enc``: kenc, denc, final_proj, bin_score; ``train_gap_grads_l<i>_attn`` /
                 ``_mlp``: the layers - the MLP weights of one layer alone are 0.8 MB and no committed file may exceed 1 MiB).
                 ``train_gap_step2``: after ``p -= 0.01 * grad`` on every parameter, a second step on the same inputs - the loss, the
                 gradients of ``denc`` and every buffer afterwards (``r2:`` / ``e2:``): the parameters and the buffers are read fresh
                 (in training mode a buffer shows in nothing but its own next value).
* ``superglue``, ``triplet``   2 pairs of 24 x 24: the inputs, loss, matches, scores, buffers and the gradients of kenc, denc,
                 final_proj and bin_score, one file each.

* the shape cases (train_ref.SHAPE_CASES: ``tiles``, ``one_pair``, ``square_triplet``, ``square_superglue``, ``wide``), each with its
                 own L and k list, three files each: ``train_shape_<case>_io`` (the inputs, meta, ``k`` with None written as 0, matches
                 and scores, ``nbt:``, the loss and every buffer, and ``e:`` of EVERY quantity), ``_z`` (Z) and ``_grads`` (every
                 gradient but the layers' convolution weights - q, k, v, merge and the two of the MLP, 1.3 MB per layer).  Those are
                 held by the tests to the float64 restatement, so the generator asserts that the restatement meets the reference
                 within the bound on every quantity, stored or not, and that its num_batches_tracked are the reference's.

The generator REFUSES a case in which a discrete decision is open: a dynamic layer's k-th and (k + 1)-th largest logits of a row
closer than 1e-9; a BatchNorm output |z| below 1e3 x the recorded error of that pre-activation; a triplet hard negative decided by
less than 1e-9 or a clamp argument within 1e-9 of zero; a match arg-max decided by less than 1e-5 (ops.extract reads Z rounded to
float32: 1e-9 would not decide it) or, for superglue, an exp(max) within 1e-4 relative of the threshold.

    python tools/make_goldens_train.py [--check]
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
import extract_ref as E  # noqa: E402
import loss_grad_ref as LG  # noqa: E402
import train_ref as T  # noqa: E402
from mdgat_matcher_amd import synth  # noqa: E402

RELU_MARGIN, TOPK_GAP, LOSS_GAP, MATCH_GAP, THR_MARGIN = 1e3, 1e-9, 1e-9, 1e-5, 1e-4


class Refused(Exception):
    pass


def ref_step(M, net, data):
    """One forward of the reference with grad and loss.mean().backward(): ``train_ref.flatten``'s dict plus matches and scores."""
    net.zero_grad(set_to_none=True)
    d = {k: v.clone() for k, v in data.items()}
    orig, cap = M.log_optimal_transport, {}

    def lot(scores, alpha, iters):
        cap['Z'] = orig(scores, alpha, iters)
        return cap['Z']
    M.log_optimal_transport = lot
    try:
        out = net(d)
    finally:
        M.log_optimal_transport = orig
    out['loss'].mean().backward()
    f = lambda v: v.detach().numpy().astype(np.float64).copy()            # noqa: E731
    res = {'loss': f(out['loss']), 'Z': f(cap['Z'])}
    for k, p in net.named_parameters():
        res['grad:' + k] = f(p.grad)
    nbt = {}
    for k, b in net.named_buffers():
        if k.endswith('num_batches_tracked'):
            nbt[k] = int(b)
        else:
            res['buf:' + k] = f(b)
    extra = {'matches0': out['matches0'].numpy().astype(np.int64), 'matches1': out['matches1'].numpy().astype(np.int64),
             'mscores0': f(out['matching_scores0']), 'mscores1': f(out['matching_scores1'])}
    return res, nbt, extra


def check_decided(case, method, mine, err_z, Z, gt0, gt1, mutual=False):
    if mine['topk_gap'] < TOPK_GAP:
        raise Refused(f'{case}: the k-th and (k + 1)-th largest logits of a row are {mine["topk_gap"]:.3e} apart')
    margin = min(float(np.abs(z).min()) / max(e, 1e-300) for z, e in zip(mine['z'], err_z))
    if margin < RELU_MARGIN:
        raise Refused(f'{case}: the smallest |z| is only {margin:.3e} x the error of its pre-activation')
    clamp = LG.clamp_margin(Z, gt0, gt1, method, T.GAMMA)
    if clamp < LOSS_GAP:
        raise Refused(f'{case}: a clamp argument lies {clamp:.3e} from zero')
    if method == 'triplet_loss' and LG.triplet_top_gap(Z, gt0, gt1) < LOSS_GAP:
        raise Refused(f'{case}: a triplet hard negative is decided by {LG.triplet_top_gap(Z, gt0, gt1):.3e}')
    mode = {('superglue', False): 2, ('superglue', True): 3}.get((method, mutual), 1 if mutual else 0)
    Zt = torch.from_numpy(Z)
    if E.ambiguous(Zt, mode, gap=MATCH_GAP):
        raise Refused(f'{case}: a match arg-max is decided by less than {MATCH_GAP}')
    if method == 'superglue':
        e = torch.cat([Zt[:, :-1, :-1].max(2).values.flatten(), Zt[:, :-1, :-1].max(1).values.flatten()]).exp()
        if float(((e - 0.2).abs() / 0.2).min()) < THR_MARGIN:
            raise Refused(f'{case}: an exp(max) lies within {THR_MARGIN} of the match threshold')
    return margin


def rel_sizes(err, want):
    """err / max|value| per quantity; not for the gradients that are zero in exact arithmetic (their value is rounding noise)."""
    return {k: e / max(float(np.abs(want[k]).max()), 1e-300) for k, e in err.items() if not k.endswith(T.ZERO_GRAD_BIASES)}


def gen_case(M, case):
    method, B, n, m, first = T.CASES[case]
    cfg = T.config(method)
    sd = T.initial_state()
    net = M.MDGAT(cfg).double().train()
    net.load_state_dict(sd, strict=True)
    data = synth.make_batch(B, n, m, first_pair=first)
    data['gt_matches0'], data['gt_matches1'] = GL.ground_truth(data, first)
    sd0 = T.numpy_state(net.state_dict())
    npdata = {k: v.numpy().copy() for k, v in data.items()}
    rec, nbt, extra = ref_step(M, net, data)
    err, mine, truth, err_z = T.reference_error(sd0, npdata, method, rec)
    margin = check_decided(case, method, mine, err_z, rec['Z'], npdata['gt_matches0'], npdata['gt_matches1'], cfg['mutual_check'])
    assert {k: int(v) for k, v in mine['after'].items() if k.endswith('num_batches_tracked')} == nbt
    rel = rel_sizes(err, rec)
    worst = max(rel, key=rel.get)
    print(f'{case}: relu margin {margin:.2e}, top-k gap {mine["topk_gap"]:.2e}; err / max|value|: median {np.median(list(rel.values())):.1e}, '
          f'loss {rel["loss"]:.1e}, Z {rel["Z"]:.1e}, worst {rel[worst]:.1e} at {worst}')
    meta = {'meta': np.array([B, n, m, T.L, T.ITERS, T.SEED, first], dtype=np.int64), 'k': np.array(T.K_LIST, dtype=np.int64),
            'gamma': np.float64(T.GAMMA), 'lr': np.float64(T.SGD_LR)}
    io = dict(meta, **{'in:' + k: v for k, v in npdata.items()}, **extra, **{'nbt:' + k: np.int64(v) for k, v in nbt.items()})
    keep = lambda names: {**{'r:' + k: rec[k] for k in names}, **{'e:' + k: np.float64(err[k]) for k in names}}        # noqa: E731
    grads = [k for k in rec if k.startswith('grad:')]
    io.update(keep(['loss'] + [k for k in rec if k.startswith('buf:')]))
    if case != 'gap':
        io.update(keep([k for k in grads if k[5:].startswith(T.ENC_PREFIXES)]))
        return {T.FILES[case][0]: io}
    io.update(keep(['Z']))
    files = {'train_gap_io': io, 'train_gap_grads_enc': keep([k for k in grads if k[5:].startswith(T.ENC_PREFIXES)])}
    for i in range(2 * T.L):
        for part in ('attn', 'mlp'):
            files[f'train_gap_grads_l{i}_{part}'] = keep([k for k in grads if k[5:].startswith(f'gnn.layers.{i}.{part}.')])
    assert sum(len(v) for v in files.values()) >= 2 * len(rec)
    # the second step: p -= lr * grad on every parameter, then the same inputs again
    with torch.no_grad():
        for p in net.parameters():
            p -= T.SGD_LR * p.grad
    rec2, _, _ = ref_step(M, net, data)
    mine2 = T.step(T.sgd(sd0, mine['grads'], mine['after']), npdata, method)
    sd_truth = T.sgd(sd0, truth['grads'], truth['after'])
    with T.R.precision(np.longdouble):
        truth2 = T.step(sd_truth, npdata, method, masks=mine2['masks'])
    if mine2['topk_gap'] < TOPK_GAP:
        raise Refused(f'{case} step 2: the k-th and (k + 1)-th largest logits of a row are {mine2["topk_gap"]:.3e} apart')
    names2 = ['loss'] + [k for k in grads if k[5:].startswith('denc.')] + [k for k in rec if k.startswith('buf:')]
    err2 = T.measure({k: rec2[k] for k in names2}, T.flatten(mine2), T.flatten(truth2))
    rel2 = rel_sizes(err2, rec2)
    print(f'{case} step 2: loss {float(rec["loss"].mean()):.6f} -> {float(rec2["loss"].mean()):.6f}; err / max|value|: loss {rel2["loss"]:.1e}, '
          f'worst {max(rel2.values()):.1e}')
    files['train_gap_step2'] = {**{'r2:' + k: rec2[k] for k in names2}, **{'e2:' + k: np.float64(err2[k]) for k in names2}}
    return files


def gen_shape_case(M, case):
    """One case of train_ref.SHAPE_CASES: the same recipe as ``gen_case`` with the case's own L and k list, every quantity measured
    (``e:``), and the reference's value (``r:``) of all of them but the layers' convolution weights.  For those the tests' expected
    value is the float64 restatement, so it is held here to the reference on EVERY quantity, stored or not."""
    method, B, n, m, L, k_list, first = T.case_spec(case)
    cfg = T.config(method, L=L, k=k_list)
    sd = T.initial_state(L=L)
    net = M.MDGAT(cfg).double().train()
    net.load_state_dict(sd, strict=True)
    data = synth.make_batch(B, n, m, first_pair=first)
    data['gt_matches0'], data['gt_matches1'] = GL.ground_truth(data, first)
    sd0 = T.numpy_state(net.state_dict())
    npdata = {k: v.numpy().copy() for k, v in data.items()}
    rec, nbt, extra = ref_step(M, net, data)
    err, mine, truth, err_z = T.reference_error(sd0, npdata, method, rec, L=L, k_list=k_list, iters=T.ITERS)
    assert set(err) == set(rec) == set(T.flatten(mine)), 'a quantity without a measured error'
    margin = check_decided(case, method, mine, err_z, rec['Z'], npdata['gt_matches0'], npdata['gt_matches1'], cfg['mutual_check'])
    assert {k: int(v) for k, v in mine['after'].items() if k.endswith('num_batches_tracked')} == nbt
    worst, where, _ = T.compare(T.flatten(mine), rec, err)
    assert worst <= 1.0, f'{case}: the restatement is {worst:.3g} x the bound from the reference at {where}'
    clamp = LG.clamp_margin(rec['Z'], npdata['gt_matches0'], npdata['gt_matches1'], method, T.GAMMA)
    rel = rel_sizes(err, rec)
    at = max(rel, key=rel.get)
    print(f'{case}: relu margin {margin:.2e}, top-k gap {mine["topk_gap"]:.2e}, clamp margin {clamp:.2e}'
          + (f', hard-negative gap {LG.triplet_top_gap(rec["Z"], npdata["gt_matches0"], npdata["gt_matches1"]):.2e}' if method == 'triplet_loss' else '')
          + f'; err / max|value|: median {np.median(list(rel.values())):.1e}, loss {rel["loss"]:.1e}, Z {rel["Z"]:.1e}, worst {rel[at]:.1e} at {at}; '
          f'restatement against the reference: {worst:.3f} of the bound at {where}')
    io = {'meta': np.array([B, n, m, L, T.ITERS, T.SEED, first], dtype=np.int64), 'k': np.array([0 if v is None else v for v in k_list], dtype=np.int64),
          'gamma': np.float64(T.GAMMA)}
    io.update({'in:' + k: v for k, v in npdata.items()}, **extra, **{'nbt:' + k: np.int64(v) for k, v in nbt.items()})
    io.update({'e:' + k: np.float64(e) for k, e in err.items()})
    io.update({'r:' + k: rec[k] for k in rec if k == 'loss' or k.startswith('buf:')})
    grads = {'r:' + k: rec[k] for k in rec if k.startswith('grad:') and T.shape_stored(k)}
    files = dict(zip(T.FILES[case], (io, {'r:Z': rec['Z']}, grads)))
    stored = sum(k.startswith('r:') for part in files.values() for k in part)
    assert len(rec) - stored == 2 * L * len(T.SHAPE_UNSTORED), (len(rec), stored)
    return files


def generate(M, out_dir):
    for case in list(T.CASES) + list(T.SHAPE_CASES):
        for name, part in (gen_case if case in T.CASES else gen_shape_case)(M, case).items():
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
        tmp = tempfile.mkdtemp(prefix='mdgat_goldens_train_')
        try:
            generate(M, tmp)
            bad = G.compare_dirs(tmp, G.OUT, list(T.ALL_FILES))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    except Refused as e:
        print('REFUSED:', e)
        sys.exit(2)
    for line in bad:
        print('MISMATCH', line)
    print(f'checked train against {G.OUT}: ' + ('OK' if not bad else f'{len(bad)} disagreements'))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
