#!/usr/bin/env python3
"""GPU box: one training step - ``MDGAT.training_forward`` and ``loss.mean().backward()`` - next to what a user has without it: the
same step written in plain torch (the module's own nn.Conv1d / nn.BatchNorm1d layers, the oracle's attention and optimal transport,
float64 autograd) on the same device, with the same parameters and inputs.  64 pairs of 512 keypoints, L = 9, 100 Sinkhorn
iterations, k and the loss (triplet) as ``synth.default_config``.  Each side runs in a fresh process of its own; it reports the
median over windows of HIP-event time per step after a warm-up step, the peak of torch.cuda.max_memory_allocated above what was
allocated before the step (parameters and inputs), and its loss (the two must agree).  One JSON line per side and one with the ratios
(DESIGN section 7.8 records them; no ratio is a condition).

    python tools/train_step_time.py [--pairs 64] [--n 512] [--L 9] [--iters 100] [--windows 7]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = 'cuda:0'


def torch_step(net, data, O):
    """The reference's training forward (mdgat.py:369-546, FPFH, triplet) on the module's own torch layers: the loss, 0-d."""
    import torch
    B = data['keypoints0'].shape[0]
    d = []
    for f in (0, 1):
        kin = torch.cat([data[f'keypoints{f}'].transpose(1, 2), data[f'scores{f}'][:, None, :]], dim=1)
        d.append(net.denc.encoder(data[f'descriptors{f}'].transpose(1, 2)) + net.kenc.encoder(kin))
    sched = net._topk_schedule()

    def prop(layer, x, src, k):
        q, kk, v = [p(t).view(B, 32, 4, -1) for p, t in zip(layer.attn.proj, (x, src, src))]
        msg = O.attention(q, kk, v)[0] if k == 0 else O.dynamic_attention(q, kk, v, k)[0]
        return layer.mlp(torch.cat([x, layer.attn.merge(msg.contiguous().view(B, 128, -1))], dim=1))
    for i, layer in enumerate(net.gnn.layers):
        s0, s1 = (d[1], d[0]) if i % 2 else (d[0], d[1])
        delta0, delta1 = prop(layer, d[0], s0, sched[i]), prop(layer, d[1], s1, sched[i])
        d = [d[0] + delta0, d[1] + delta1]
    md0, md1 = net.final_proj(d[0]), net.final_proj(d[1])
    scores = torch.einsum('bdn,bdm->bnm', md0, md1) / 128 ** 0.5
    Z = O.log_optimal_transport(scores, net.bin_score, int(net.config['sinkhorn_iterations']))
    n, m = Z.shape[1] - 1, Z.shape[2] - 1
    g0, g1 = data['gt_matches0'].long(), data['gt_matches1'].long()
    p0, p1 = torch.where(g0 < 0, m, g0)[..., None], torch.where(g1 < 0, n, g1)[:, None, :]
    rows, cols = Z[:, :n, :], Z[:, :, :m]
    t = lambda z: -torch.log(torch.exp(z))          # noqa: E731
    x_r = t(rows.gather(2, p0)[..., 0]) - t(rows.scatter(2, p0, float('-inf')).amax(2))
    x_c = t(cols.gather(1, p1)[:, 0]) - t(cols.scatter(1, p1, float('-inf')).amax(1))
    return torch.clamp(torch.cat([x_r, x_c], dim=1) + float(net.triplet_loss_gamma), min=0).mean()


def child(args):
    import torch
    from mdgat_matcher_amd import MDGAT, synth
    from oracle import mdgat_oracle as O
    torch.backends.cuda.matmul.allow_tf32 = False
    net = MDGAT(synth.default_config(L=args.L, sinkhorn_iterations=args.iters)).double()
    net.load_state_dict(synth.make_state_dict(L=args.L, seed=1))
    net = net.to(DEV).train()
    data = synth.make_batch(args.pairs, args.n, args.n, device=DEV)

    def step():
        net.zero_grad(set_to_none=True)
        batch = {k: v.clone() for k, v in data.items()}
        loss = net.training_forward(batch)['loss'].mean() if args.side == 'ours' else torch_step(net, batch, O)
        loss.backward()
        return loss
    loss = step()                                           # warm-up
    torch.cuda.synchronize()
    net.zero_grad(set_to_none=True)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    times = []
    for _ in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = step()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    peak = torch.cuda.max_memory_allocated() - base
    gnorm = float(sum(p.grad.double().pow(2).sum() for p in net.parameters()).sqrt())
    print(json.dumps({'side': args.side, 'pairs': args.pairs, 'n': args.n, 'L': args.L, 'iters': args.iters, 'step_ms': round(statistics.median(times), 2),
                      'min_ms': round(min(times), 2), 'max_ms': round(max(times), 2), 'peak_mb': round(peak / 2 ** 20, 1),
                      'loss': float(loss.detach()), 'grad_norm': gnorm}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--L', type=int, default=9)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--side', choices=('ours', 'torch'), default=None)
    ap.add_argument('--child-timeout', type=float, default=280.0)
    args = ap.parse_args()
    if args.side is not None:
        return child(args)
    recs = {}
    for side in ('ours', 'torch'):                          # a fresh process each: neither sees the other's allocator or caches
        cmd = [sys.executable, os.path.abspath(__file__), '--side', side] + [f'--{k}={getattr(args, k)}' for k in ('pairs', 'n', 'L', 'iters', 'windows')]
        out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout, check=True).stdout
        line = [ln for ln in out.splitlines() if ln.startswith('{')][-1]
        print(line, flush=True)
        recs[side] = json.loads(line)
    a, b = recs['ours'], recs['torch']
    print(json.dumps({'time_ratio': round(a['step_ms'] / b['step_ms'], 3), 'memory_ratio': round(a['peak_mb'] / b['peak_mb'], 3),
                      'loss_difference': abs(a['loss'] - b['loss']), 'grad_norm_rel_difference': abs(a['grad_norm'] - b['grad_norm']) / b['grad_norm']}))


if __name__ == '__main__':
    main()
