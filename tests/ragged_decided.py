"""Which pairs the fp32-class arithmetic must reproduce to the literal bar (tests/test_gpu_ragged_forward_fp32.py), computed on the CPU
from the fp64 oracle alone.

The fp32-class forward carries logits to ~8e-6 (parity_util.GAP_EPS: 2e-5 bounds it) and Z to a few 1e-6.  Two things in the network are
discontinuous - the top-k selection of a dynamic layer and the arg-maxes of the extraction - and a pair whose oracle trajectory comes
close to neither is DECIDED: no rounding of that class can change a selection or a match, so Z, the scores and the matches must agree
with the oracle to the plain bars.  The other pairs get the bounds parity_util states for outputs with flipped near ties."""
import torch

from oracle import mdgat_oracle as O
from parity_util import GAP_EPS, Z_TOL

MIN_GAP = 2 * GAP_EPS       # 4e-5: twice the bound on the logit error, five times the worst fp32-class logit error on record


def oracle_pair(sd, cfg, data):
    """The oracle's forward of one pair (tensors with a leading axis of 1) -> (its outputs, its capture, the smallest gap between the k-th
    and the (k+1)-th largest logit over every row of every dynamic layer - inf without one -, the smallest margin between the two best
    candidates of any arg-max of the extraction: rows and columns of Z, dustbins included)."""
    cap = {}
    ref = O.mdgat_forward(sd, cfg, data, cap)
    sched = O.layer_topk_schedule(cfg['L'], cfg['k'])
    gap = float('inf')
    for i, k in enumerate(sched):
        if k is None:
            continue
        x = [cap[f'layer{i - 1}_desc{f}'] if i else cap[f'enc{f}'] for f in (0, 1)]
        for side in (0, 1):
            src = x[1 - side] if i & 1 else x[side]
            p = f'gnn.layers.{i}.attn'
            q = O._pointwise(sd[f'{p}.proj.0.weight'], sd[f'{p}.proj.0.bias'], x[side]).view(1, 32, 4, -1)
            kk = O._pointwise(sd[f'{p}.proj.1.weight'], sd[f'{p}.proj.1.bias'], src).view(1, 32, 4, -1)
            logits = torch.einsum('bdhn,bdhm->bhnm', q, kk) / 32 ** 0.5
            if k < logits.shape[-1]:
                top = logits.topk(k + 1, dim=3).values
                gap = min(gap, float((top[..., k - 1] - top[..., k]).min()))
    Z = cap['Z'][0]
    n, m = Z.shape[0] - 1, Z.shape[1] - 1
    margin = float('inf')
    if m >= 1:
        r = Z[:n].topk(2, dim=1).values
        margin = min(margin, float((r[:, 0] - r[:, 1]).min()))
    if n >= 1:
        c = Z[:, :m].topk(2, dim=0).values
        margin = min(margin, float((c[0] - c[1]).min()))
    return ref, cap, gap, margin


def decided(gap, margin):
    return gap >= MIN_GAP and margin >= Z_TOL
