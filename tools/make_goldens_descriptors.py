#!/usr/bin/env python3
"""Generate tests/golden/desc_*.npz: the reference's own ``MDGAT`` with ``descriptor='FPFH_gloabal'`` and ``'FPFH_only'``
(models/mdgat.py:156-174, 342-350, 389-393, 421-426) in fp64 on the CPU.  Runs where the reference exists (never on the GPU box);
imports it unmodified through the device shim of make_goldens.py.  Arrays and name lists only; the weights are not stored, the seed
is: ``synth.make_state_dict(L=1, seed=11, descriptor=...)``.  The net is tests/train_ref.py's: L = 1 (layer 0 self and full, layer 1
cross with k = 8), 20 Sinkhorn iterations.

* ``desc_<d>_eval``     ``net.double().eval()``, 2 pairs of 20 x 28 (gap_loss): the inputs, the encoder output per frame as the GNN
                        receives it (forward hooks: denc + kenc, or denc alone), its measured error ``enc_err``, Z, matches, scores, the
                        state dict's names and shapes.
* ``desc_gloabal_ragged``   eval, k = [] (a frame of 5 keypoints has no 8 keys), four pairs with counts (5, 9), (28, 20), (17, 28),
                        (9, 8), the reference run ONE PAIR AT A TIME: inputs, encoder outputs, Z, matches and scores per pair
                        (``p<i>:<name>``), and per frame the number of channels in which a padded row would win the pool (``visible``).
* ``desc_<d>_train_<case>_<i>``   ``net.double().train()``, tests/train_ref.py's 'gap' (2 pairs of 20 x 28) and 'triplet' (2 pairs of
                        24 x 24) inputs: one forward and ``loss.mean().backward()`` - loss, Z, matches, scores, every gradient, every
                        buffer, and ``e:<quantity>`` the measured error (tests/descriptor_ref.py: the 80-bit re-evaluation), spread over
                        numbered files of less than 1 MiB.

The generator REFUSES a case in which a discrete decision is open - every check of make_goldens_train.py - and additionally when
* a pooled channel's largest and second-largest entry differ by less than 1e-9 relative (which row wins a tie is unspecified);
* a frame has no pooled channel with a NEGATIVE maximum (a zero-initialised accumulator would then go unnoticed);
* in the ragged fixture, a frame shorter than its slot has fewer than 8 channels in which ``denc.encoder(0-row)`` exceeds the true
  maximum over the frame's own rows (a pool that forgets the counts would then go unnoticed).

    python tools/make_goldens_descriptors.py
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
import make_goldens_train as GT  # noqa: E402
import extract_ref as E  # noqa: E402
import descriptor_ref as DR  # noqa: E402
import train_ref as T  # noqa: E402
from mdgat_matcher_amd import synth  # noqa: E402

POOL_GAP, VISIBLE_MIN, PART_BYTES = 1e-9, 8, 900_000
Refused = GT.Refused


def ref_forward(M, net, data, grad=False):
    """One forward of the reference: (out, Z, [encoder output of frame 0, of frame 1] as [B, n, 128])."""
    cap = {'denc': [], 'kenc': []}
    hooks = [net.denc.register_forward_hook(lambda m, i, o: cap['denc'].append(o.detach().clone()))]
    if hasattr(net, 'kenc'):
        hooks.append(net.kenc.register_forward_hook(lambda m, i, o: cap['kenc'].append(o.detach().clone())))
    orig = M.log_optimal_transport

    def lot(scores, alpha, iters):
        cap['Z'] = orig(scores, alpha, iters)
        return cap['Z']
    M.log_optimal_transport = lot
    try:
        d = {k: v.clone() for k, v in data.items()}
        if grad:
            out = net(d)
        else:
            with torch.no_grad():
                out = net(d)
    finally:
        M.log_optimal_transport = orig
        for h in hooks:
            h.remove()
    enc = [(cap['denc'][f] + (cap['kenc'][f] if cap['kenc'] else 0)).transpose(1, 2).numpy().copy() for f in (0, 1)]
    return out, cap['Z'], enc


def out_arrays(out):
    f = lambda v: v.detach().numpy().astype(np.float64).copy()            # noqa: E731
    return {'matches0': out['matches0'].numpy().astype(np.int64), 'matches1': out['matches1'].numpy().astype(np.int64),
            'mscores0': f(out['matching_scores0']), 'mscores1': f(out['matching_scores1'])}


def check_pool(case, e_frames):
    """The pool's own conditions on e [B, n, 128] per frame."""
    for f, e in enumerate(e_frames):
        gap = DR.pool_gap(e)
        if gap < POOL_GAP:
            raise Refused(f'{case}: frame {f}: a pooled channel\'s two largest entries are {gap:.3e} apart (relative)')
        neg = (np.asarray(e, dtype=np.float64).max(axis=1) < 0).sum(axis=1)
        if int(neg.min()) < 1:
            raise Refused(f'{case}: frame {f}: a pair has no pooled channel with a negative maximum')


def pooled_e(sd, npdata):
    """denc.encoder's eval-mode output per frame [B, n, 128] (the restatement's: the reference does not expose it)."""
    p = T._mlp_p(sd, 'denc.encoder', 3)
    B = npdata['descriptors0'].shape[0]
    return [DR.R.forward(npdata[f'descriptors{f}'].reshape(-1, 33), p, training=False)[0].reshape(B, -1, 128) for f in (0, 1)]


def check_extract(case, Z, method='gap_loss', mutual=False):
    mode = {('superglue', False): 2, ('superglue', True): 3}.get((method, mutual), 1 if mutual else 0)
    if E.ambiguous(torch.from_numpy(Z), mode, gap=GT.MATCH_GAP):
        raise Refused(f'{case}: a match arg-max is decided by less than {GT.MATCH_GAP}')


def check_forward(case, sd0, npdata, descriptor, Z, k_list):
    """The open decisions of an eval() forward, on the restatement's float64 and 80-bit evaluations: the dynamic layer's selection,
    the ReLUs behind every BatchNorm, the pool."""
    mine = DR.step(sd0, npdata, 'gap_loss', descriptor, k_list=k_list, training=False)
    with DR.R.precision(np.longdouble):
        truth = DR.step(sd0, npdata, 'gap_loss', descriptor, k_list=k_list, training=False, masks=mine['masks'])
    if mine['topk_gap'] < GT.TOPK_GAP:
        raise Refused(f'{case}: the k-th and (k + 1)-th largest logits of a row are {mine["topk_gap"]:.3e} apart')
    margin = min(float(np.abs(a).min()) / max(float(np.abs(np.asarray(a, dtype=np.longdouble) - b).max()), 1e-300) for a, b in zip(mine['z'], truth['z']))
    if margin < GT.RELU_MARGIN:
        raise Refused(f'{case}: the smallest |z| is only {margin:.3e} x the error of its pre-activation')
    dz = float(np.abs(Z - np.asarray(mine['Z'], dtype=np.float64)).max())
    if dz > 1e-9:
        raise Refused(f'{case}: the restatement\'s Z is {dz:.3e} from the reference\'s')
    if descriptor == 'FPFH_gloabal':
        check_pool(case, mine['e'])
    print(f'{case}: relu margin {margin:.2e}, top-k gap {mine["topk_gap"]:.2e}, pool gap {mine["pool_gap"]:.2e}, max|Z - restatement| {dz:.1e}')


def gen_eval(M, descriptor):
    case = DR.eval_file(descriptor)
    method, B, n, m, first = T.CASES['gap']
    cfg = DR.config(method, descriptor)
    sd = DR.initial_state(descriptor)
    net = G.build_ref_net(M, cfg, sd)
    data = synth.make_batch(B, n, m, first_pair=first)
    data['gt_matches0'], data['gt_matches1'] = GL.ground_truth(data, first)
    npdata = {k: v.numpy().copy() for k, v in data.items()}
    out, Z, enc = ref_forward(M, net, data)
    Z = Z.detach().numpy().copy()
    sd0 = T.numpy_state(net.state_dict())
    enc_err, mine = DR.encoder_error(sd0, npdata, descriptor, enc)
    check_extract(case, Z)
    check_forward(case, sd0, npdata, descriptor, Z, T.K_LIST)
    names = list(net.state_dict().keys())
    print(f'{case}: encoder err {enc_err:.2e} (max|enc| {max(float(np.abs(e).max()) for e in enc):.2f}), {int((out["matches0"] >= 0).sum())} matches')
    return {case: dict({'in:' + k: v for k, v in npdata.items()}, enc0=enc[0], enc1=enc[1], enc_err=np.float64(enc_err), Z=Z, **out_arrays(out),
                       names=np.array(names), shapes=np.array([','.join(map(str, net.state_dict()[k].shape)) for k in names]),
                       meta=np.array([B, n, m, T.L, T.ITERS, DR.SEED, first], dtype=np.int64), k=np.array(T.K_LIST, dtype=np.int64))}


def gen_ragged(M):
    descriptor, case = 'FPFH_gloabal', DR.RAGGED_FILE
    cfg = synth.default_config(L=T.L, k=[], sinkhorn_iterations=T.ITERS, loss_method='gap_loss', triplet_loss_gamma=T.GAMMA, descriptor=descriptor)
    sd = DR.initial_state(descriptor)
    net = G.build_ref_net(M, cfg, sd)
    sd0 = T.numpy_state(net.state_dict())
    slots = (max(c[0] for c in DR.RAGGED_COUNTS), max(c[1] for c in DR.RAGGED_COUNTS))
    zero = np.asarray(DR.zero_row(T._mlp_p(sd0, 'denc.encoder', 3)), dtype=np.float64)
    arrays = {'counts': np.array(DR.RAGGED_COUNTS, dtype=np.int64), 'meta': np.array([T.L, T.ITERS, DR.SEED, DR.RAGGED_FIRST], dtype=np.int64)}
    visible = np.full((len(DR.RAGGED_COUNTS), 2), -1, dtype=np.int64)
    for i, (n, m) in enumerate(DR.RAGGED_COUNTS):
        data = synth.make_batch(1, n, m, first_pair=DR.RAGGED_FIRST + i)
        npdata = {k: v.numpy().copy() for k, v in data.items()}
        out, Z, enc = ref_forward(M, net, data)
        Z = Z.detach().numpy().copy()
        check_extract(f'{case} pair {i}', Z)
        check_forward(f'{case} pair {i}', sd0, npdata, descriptor, Z, [])
        e = pooled_e(sd0, npdata)
        for f in (0, 1):
            if (n, m)[f] < slots[f]:
                visible[i, f] = int((zero > np.asarray(e[f][0], dtype=np.float64).max(axis=0)).sum())
                if visible[i, f] < VISIBLE_MIN:
                    raise Refused(f'{case} pair {i} frame {f}: a padded row would win the pool in only {visible[i, f]} channels')
        arrays.update({f'p{i}:in:{k}': v for k, v in npdata.items()})
        arrays.update({f'p{i}:{k}': v for k, v in dict(out_arrays(out), Z=Z, enc0=enc[0], enc1=enc[1]).items()})
    arrays['visible'] = visible
    print(f'{case}: channels in which a padded row would win the pool, per pair and frame (-1: the frame fills its slot): {visible.tolist()}')
    return {case: arrays}


def gen_train(M, descriptor, case):
    method, B, n, m, first = T.CASES[case]
    cfg = DR.config(method, descriptor)
    sd = DR.initial_state(descriptor)
    net = M.MDGAT(cfg).double().train()
    net.load_state_dict(sd, strict=True)
    data = synth.make_batch(B, n, m, first_pair=first)
    data['gt_matches0'], data['gt_matches1'] = GL.ground_truth(data, first)
    sd0 = T.numpy_state(net.state_dict())
    npdata = {k: v.numpy().copy() for k, v in data.items()}
    rec, nbt, extra = GT.ref_step(M, net, data)
    err, mine, truth, err_z = DR.reference_error(sd0, npdata, method, descriptor, rec)
    name = f'{descriptor} {case}'
    margin = GT.check_decided(name, method, mine, err_z, rec['Z'], npdata['gt_matches0'], npdata['gt_matches1'], cfg['mutual_check'])
    if descriptor == 'FPFH_gloabal':
        check_pool(name, mine['e'])
    assert {k: int(v) for k, v in mine['after'].items() if k.endswith('num_batches_tracked')} == nbt
    assert set(T.flatten(mine)) == set(rec), set(T.flatten(mine)) ^ set(rec)
    rel = {k: e / max(float(np.abs(rec[k]).max()), 1e-300) for k, e in err.items() if not k.endswith(DR.zero_grad_biases(descriptor))}
    worst = max(rel, key=rel.get)
    print(f'{name}: relu margin {margin:.2e}, top-k gap {mine["topk_gap"]:.2e}, pool gap {mine["pool_gap"]:.2e}; err / max|value|: median '
          f'{np.median(list(rel.values())):.1e}, loss {rel["loss"]:.1e}, Z {rel["Z"]:.1e}, worst {rel[worst]:.1e} at {worst}')
    first_part = dict({'in:' + k: v for k, v in npdata.items()}, **extra, **{'nbt:' + k: np.int64(v) for k, v in nbt.items()},
                      meta=np.array([B, n, m, T.L, T.ITERS, DR.SEED, first], dtype=np.int64), k=np.array(T.K_LIST, dtype=np.int64),
                      gamma=np.float64(T.GAMMA))
    parts, size = [first_part], sum(v.nbytes for v in first_part.values())
    for k in sorted(rec, key=lambda k: (not k.startswith(('loss', 'Z', 'buf:')), k)):
        nb = rec[k].nbytes + 8
        if size + nb > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1]['r:' + k], parts[-1]['e:' + k] = rec[k], np.float64(err[k])
        size += nb
    return {f'desc_{DR.SHORT[descriptor]}_train_{case}_{i}': p for i, p in enumerate(parts)}


def main():
    torch.set_num_threads(synth.effective_cpu_count())
    M = G.import_reference()
    only = sys.argv[1:]
    jobs = [('eval', d) for d in DR.DESCRIPTORS] + [('ragged', None)] + [('train', (d, c)) for d in DR.DESCRIPTORS for c in DR.TRAIN_CASES]
    try:
        for kind, arg in jobs:
            if only and kind not in only:
                continue
            files = gen_eval(M, arg) if kind == 'eval' else gen_ragged(M) if kind == 'ragged' else gen_train(M, *arg)
            for name, part in files.items():
                path = os.path.join(G.OUT, name + '.npz')
                np.savez_compressed(path, **part)
                print(f'wrote {path} ({os.path.getsize(path)} bytes)')
                assert os.path.getsize(path) < (1 << 20), path
    except Refused as e:
        print('REFUSED:', e)
        sys.exit(2)


if __name__ == '__main__':
    main()
