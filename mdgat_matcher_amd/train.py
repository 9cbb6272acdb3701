"""The training-mode forward of the whole MDGAT (models/mdgat.py:369-603, descriptor='FPFH', 'FPFH_gloabal' or 'FPFH_only') in fp64, composed in Python from the
differentiable device primitives of ``ops``: ``mlp_f64_tensors`` (the encoders, q | k | v, merge, the layer MLP), ``attention_f64``,
``match_head``, ``log_optimal_transport``, ``extract`` and ``matching_loss``.  ``MDGAT.training_forward`` is the public entry.

What autograd records is one node per primitive; the parameters are read from the modules on every call (never from the packed
blobs), so ``loss.mean().backward()`` fills the ``.grad`` of the module's own parameters and ``optimizer.step()`` is seen by the
next call.  A layer's parameters serve both frames: autograd sums their gradients.

BatchNorm follows ``net.training``, called as the reference calls it: every encoder once per frame (frame 0 first), every layer's MLP
for frame 0 and then for frame 1 (mdgat.py:270-272) - statistics over one frame's B * N rows, the buffers moved twice per layer and
step.  q / k / v / merge have no BN and run once over the N + M points of both frames.

Layout: point-major, channel-last, from the inputs to the head; the descriptors of the two frames are kept as two contiguous tensors
[B, N, 128] and [B, M, 128].  The reference's head order of the attention channels (c = dim * 4 + head) against the kernels'
(head * 32 + dim) is a permutation of WEIGHTS - the rows of q / k / v, the columns of merge, gathered by torch indexing, which
carries the gradient back to the modules' weights - never of an activation.  q | k | v is one 128 -> 384 product whose output is the
attention's [B, N + M, 3, 4, 32] as it stands.  ``desc + delta`` and ``denc(...) + kenc(...)`` are the residual operand of the MLP's last
product.  Per layer two activation-sized copies remain, both forced by the per-frame BatchNorm: the two frames' descriptors are laid
side by side for the q | k | v product (``cat``), and the merged message is split into its frames' rows (contiguous per frame for
B > 1 only as a copy)."""
from __future__ import annotations

import torch

from . import _lib, ops

# kernel channel head * 32 + dim  <-  reference channel dim * 4 + head
_PERM = [(j % 32) * 4 + j // 32 for j in range(128)]


def _enc_parts(seq):
    mods = list(seq.children())
    convs, bns = mods[0::3], mods[1::3]
    return [c.weight for c in convs], [c.bias for c in convs], bns


def _layer(layer, d0, d1, cross, k, training, perm):
    """One AttentionalPropagation for both frames (mdgat.py:246-248, 261-274): (desc0 + delta0, desc1 + delta1)."""
    B, N, M = d0.shape[0], d0.shape[1], d1.shape[1]
    proj, merge = layer.attn.proj, layer.attn.merge
    wqkv = torch.stack([p.weight[:, :, 0] for p in proj])[:, perm].reshape(384, 128)
    bqkv = torch.stack([p.bias for p in proj])[:, perm].reshape(384)
    desc = torch.cat([d0, d1], dim=1)
    qkv = ops.mlp_f64_tensors(desc, [wqkv], [bqkv], training=training).view(B, N + M, 3, 4, 32)
    msg = ops.attention_f64(qkv, N, M, cross, topk=k)
    merged = ops.mlp_f64_tensors(msg, [merge.weight[:, :, 0][:, perm]], [merge.bias], training=training)
    m0, m1 = merged.split([N, M], dim=1)
    ws, bs, bns = _enc_parts(layer.mlp)
    # frame 0 first: the buffers move in the reference's order
    out0 = ops.mlp_f64_tensors(d0, ws, bs, bns, training, x1=m0.contiguous(), residual=d0)
    out1 = ops.mlp_f64_tensors(d1, ws, bs, bns, training, x1=m1.contiguous(), residual=d1)
    return out0, out1


def descriptors(net, kpts0, sigma0, fpfh0, kpts1, sigma1, fpfh1):
    """The encoders and the GNN: (desc0 [B, N, 128], desc1 [B, M, 128]) as ``final_proj`` receives them, point-major."""
    training = bool(net.training)
    descriptor = net.descriptor
    dw, db, dbn = _enc_parts(net.denc.encoder)
    if descriptor != 'FPFH_only':
        kw, kb, kbn = _enc_parts(net.kenc.encoder)
    if descriptor == 'FPFH_gloabal':
        gw, gb, gbn = _enc_parts(net.denc.encoder2)
    out = []
    for kpts, sigma, fpfh in ((kpts0, sigma0, fpfh0), (kpts1, sigma1, fpfh1)):        # mdgat.py:392-393: denc, then kenc, per frame
        enc = ops.mlp_f64_tensors(fpfh, dw, db, dbn, training)
        if descriptor == 'FPFH_gloabal':
            # DescriptorGloabalEncoder (mdgat.py:163-174): encoder2 over [e | the frame's maximum of e, repeated]; its BatchNorm sees this
            # frame's B * n rows
            g, _ = ops.frame_max_f64(enc)
            enc = ops.mlp_f64_tensors(enc, gw, gb, gbn, training, x1=g.unsqueeze(1).expand(-1, enc.shape[1], -1))
        if descriptor == 'FPFH_only':       # mdgat.py:421-426: denc alone
            out.append(enc)
            continue
        out.append(ops.mlp_f64_tensors(torch.cat([kpts, sigma.unsqueeze(-1)], dim=-1), kw, kb, kbn, training, residual=enc))
    d0, d1 = out
    perm = torch.tensor(_PERM, dtype=torch.int64, device=d0.device)
    sched = net._topk_schedule()
    for i, layer in enumerate(net.gnn.layers):
        d0, d1 = _layer(layer, d0, d1, bool(i % 2), sched[i], training, perm)
    return d0, d1


def training_forward(net, data):
    """See ``MDGAT.training_forward``."""
    kpts0, kpts1 = data['keypoints0'], data['keypoints1']
    if kpts0.shape[1] == 0 or kpts1.shape[1] == 0:      # mdgat.py:374-382
        shape0, shape1 = kpts0.shape[:-1], kpts1.shape[:-1]
        return {
            'matches0': kpts0.new_full(shape0, -1, dtype=torch.int)[0],
            'matches1': kpts1.new_full(shape1, -1, dtype=torch.int)[0],
            'matching_scores0': kpts0.new_zeros(shape0, dtype=torch.float64)[0],
            'matching_scores1': kpts1.new_zeros(shape1, dtype=torch.float64)[0],
            'skip_train': True,
        }
    if not kpts0.is_cuda:
        raise RuntimeError('mdgat_matcher_amd runs on MI355X (gfx950) only: inputs must be on a CUDA/HIP device; there is no CPU fallback')
    dev = kpts0.device
    if 'bin_score' not in net._parameters:
        raise NotImplementedError('training_forward on a DataParallel replica: multi-GPU training is out of scope (one device only)')
    if net.bin_score.dtype != torch.float64 or net.bin_score.device != dev:
        raise NotImplementedError(f'training_forward needs a float64 module on the inputs\' device ({dev}): call net.double().to(device) '
                                  f'(the module is {net.bin_score.dtype} on {net.bin_score.device}); the fp32-class path has no backward')
    method = _lib.LOSS_METHODS.get(net.loss_method)
    if method is None:
        raise ValueError(f"loss_method={net.loss_method!r}: the loss is defined for 'superglue', 'triplet_loss' and 'gap_loss'")
    keys = ('keypoints0', 'scores0', 'descriptors0', 'keypoints1', 'scores1', 'descriptors1')
    # ('FPFH_only' never reads the saliency, mdgat.py:421-426)
    ins = [None if net.descriptor == 'FPFH_only' and k.startswith('scores') else data[k].to(device=dev, dtype=torch.float64) for k in keys]
    if ins[2].shape[-1] != 33 or ins[5].shape[-1] != 33 or kpts0.shape[-1] != 3 or kpts1.shape[-1] != 3:
        raise ValueError('expected keypoints [B, N, 3] and 33-D FPFH descriptors [B, N, 33]')
    gt0, gt1 = data['gt_matches0'], data['gt_matches1']            # KeyError when absent, as in the reference (mdgat.py:438-439)
    B, N, M = kpts0.shape[0], kpts0.shape[1], kpts1.shape[1]
    if tuple(gt0.shape) != (B, N) or tuple(gt1.shape) != (B, M):
        raise ValueError(f'gt_matches0 {tuple(gt0.shape)} / gt_matches1 {tuple(gt1.shape)}: expected [{B}, {N}] / [{B}, {M}]')
    if method != _lib.LOSS_GAP and N != M:
        raise ValueError(f'loss_method={net.loss_method!r} needs frames of equal size (N={N}, M={M}): the reference\'s index '
                         "tensors do not broadcast otherwise; 'gap_loss' takes ragged pairs")
    with torch.cuda.device(dev):
        d0, d1 = descriptors(net, *ins)
        scores = ops.match_head(d0, d1, net.final_proj.weight, net.final_proj.bias)
        Z = ops.log_optimal_transport(scores, net.bin_score, int(net.config['sinkhorn_iterations']), arithmetic='fp64')
        # matches and loss from the same Z
        m0, m1, s0, s1 = ops.extract(Z.detach(), net._extract_mode(), float(net.config['match_threshold']))
        s0, s1 = s0.to(torch.float64), s1.to(torch.float64)
        # (copies: the loss keeps its gts for the backward, and the caller's are rewritten in place below)
        g0 = gt0.detach().to(device=dev, dtype=torch.int64, copy=True)
        g1 = gt1.detach().to(device=dev, dtype=torch.int64, copy=True)
        per_pair = ops.matching_loss(Z, g0, g1, net.loss_method, float(net.triplet_loss_gamma))     # IndexError for a gt out of range
        if method != _lib.LOSS_SUPERGLUE:
            # mdgat.py:519-520, 554-555 rewrite the caller's tensors in place (test.py:237-238 undoes it)
            gt0[gt0 == -1] = M
            gt1[gt1 == -1] = N
            if not bool((m0 >= 0).any()):               # mdgat.py:464-467: integer-zero scores when nothing matched
                s0, s1 = torch.zeros_like(m0), torch.zeros_like(m1)
        loss = per_pair if method == _lib.LOSS_GAP else per_pair.mean()
    return {'matches0': m0, 'matches1': m1, 'matching_scores0': s0, 'matching_scores1': s1, 'loss': loss}


def training_batch_frames(net, bank, idx0, idx1, T0, T1, T_gt=None, max_keypoints=512, gt_threshold=0.5, gt_mutual=None, min_saliency=10.0,
                          normalize=True):
    """See ``MDGAT.training_batch_frames``."""
    a = ops.assemble_frames_train(bank, idx0, idx1, max_keypoints, min_saliency=min_saliency, normalize=normalize)
    # the one read of the two device words: which frames kept no record, and whether a kept record was unusable
    words = torch.cat([a['status'].reshape(-1), a['range_violation']]).cpu()
    none = words[:-1].nonzero()
    if none.numel():
        w = int(none[0])
        b, f = w // 2, w % 2
        frame = int(torch.as_tensor((idx0, idx1)[f]).reshape(-1)[b])
        raise ValueError(f'pair {b}: frame {f} (frame {frame} of the bank) has no keypoint with saliency > {float(min_saliency):g}: the '
                         f"reference's loader does not terminate on it (load_data.py:198, `while kp1_num > len(kp1)` on an empty array)")
    if int(words[-1]):
        raise RuntimeError('training_batch_frames: a kept record of the chunk holds a non-finite word or an all-zero FPFH row (NaN '
                           'descriptors in the reference): the batch is invalid')
    mutual = net.mutual_check if gt_mutual is None else gt_mutual
    g0, g1, rep = ops.gt_matches(a['keypoints0_f32'], a['keypoints1_f32'], T0, T1, threshold=gt_threshold, mutual=bool(mutual))
    batch = {**a, 'gt_matches0': g0, 'gt_matches1': g1, 'rep': rep}
    if T_gt is not None:
        batch['T_gt'] = torch.as_tensor(T_gt).to(device=g0.device, dtype=torch.float64)
    return batch
