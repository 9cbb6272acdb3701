"""The whole training step of MDGAT (models/mdgat.py:369-603, descriptor='FPFH', ``net.double().train()``; train.py:234-248's
``loss.mean().backward()``) restated in numpy, no autograd: the yardstick of ``MDGAT.training_forward``.

Composed from the restatements that pin the device primitives: ``mlp_grad_ref`` (the MLP with batch-statistics BatchNorm, its gradient and
buffer update; its ``_attention`` is ``attention_grad_ref``'s formulas) around this module's own forms of the head, the optimal
transport and the loss.  Those three are written out here once more because ``head_grad_ref``, ``sinkhorn_grad_ref`` and ``loss_ref`` /
``loss_grad_ref`` pin float64 in their code (``np.asarray(x, dtype=np.float64)``, torch float64) and the tolerance needs the step in x86's
80-bit format as well; tests/test_train_ref.py holds each of them to its pinned sibling in float64.  Everything runs in
``mlp_grad_ref``'s current precision (``with R.precision(np.longdouble):``).

Order of the calls, which is what BatchNorm sees: ``denc`` and ``kenc`` once per frame, frame 0 first; each layer's q / k / v / merge
once over both frames' points, then its MLP for frame 0 and for frame 1 - statistics over one frame's B * N rows, the buffers moved
twice per layer.  The top-k selection of a dynamic layer is decided on the float64 logits and handed to every precision as masks.

Tolerance (the method of mlp_grad_ref's section on the whole layer): the generator evaluates this restatement a second
time in 80-bit arithmetic and records per quantity err = the larger of max|the reference's float64 - that| and max|this restatement's
float64 - that|; a gradient that is zero in exact arithmetic (the biases in front of a BatchNorm, bk, bv, bm) gets the floor
4 u max|dW of the same convolution|.  A third float64 evaluation is held to 32 err: 2 for the two implementations compared, 16 for the
tail over summation orders.

``step(..., plant=...)`` plants the mistakes the bound must catch (PLANTS).  Two of them (TAIL_PLANTS) begin beyond one tile of a
kernel - the queries of a ragged last tile missing from dk and dv, the rows of a second slab missing from a dW - and change no bit of
the three small fixtures; the shape cases (SHAPE_CASES) are the ones that see them."""
import os

import numpy as np

import attention_grad_ref as A
import mlp_grad_ref as R

U = 2.0 ** -53
FACTOR = 32.0
PERM = A.PERM
EPS, MOMENTUM = 1e-5, 0.1               # nn.BatchNorm1d's defaults, which the reference's MLP takes
# the plants whose damage begins beyond one tile of a kernel: no-ops, bit for bit, on the three small fixtures (SHAPE_CASES shows them)
TAIL_PLANTS = ('tile_tail', 'second_slab')
TILE_QUERIES, SLAB_ROWS = 64, 512       # queries per workgroup of the attention backward's dk / dv pass; rows per slab of the dW kernel
PLANTS = ('joint_bn', 'frame_order', 'no_residual', 'cross_kv_grad', 'no_perm_merge', 'final_proj_entry', 'no_bin_grad') + TAIL_PLANTS
METHODS = ('superglue', 'triplet_loss', 'gap_loss')

# ---- the fixtures (tools/make_goldens_train.py) ----
#        case,        loss_method,    B, N,  M,  first_pair
CASES = {'gap':       ('gap_loss',     2, 20, 28, 40),
         'superglue': ('superglue',    2, 24, 24, 44),
         'triplet':   ('triplet_loss', 2, 24, 24, 44)}
L, K_LIST, ITERS, SEED, GAMMA = 1, [8], 20, 11, 0.5
SGD_LR = 0.01                            # the second step of the 'gap' case follows p -= SGD_LR * grad
ENC_PREFIXES = ('kenc.', 'denc.', 'final_proj.', 'bin_score')          # the gradients recorded for superglue / triplet
GAP_FILES = ('train_gap_io', 'train_gap_grads_enc', 'train_gap_grads_l0_attn', 'train_gap_grads_l0_mlp', 'train_gap_grads_l1_attn',
             'train_gap_grads_l1_mlp', 'train_gap_step2')
FILES = {'gap': GAP_FILES, 'superglue': ('train_superglue',), 'triplet': ('train_triplet',)}
# ---- the shape cases: a whole step past one tile of every kernel it composes (same generator, same seed, same iterations) ----
# Each carries its own network: L pairs of layers and the k list (None: full attention; topk_schedule gives the k of every layer).
#   tiles            2 and 3 query tiles of the attention backward with ragged 16-blocks (70 = 64 + 6, 180 = 11 x 16 + 4); 540 rows in
#                    frame 1 and 750 in q | k | v: a second, ragged slab of the dW kernel; layer 1 cross with k = 16, layer 2 self with
#                    k = 8, layer 3 cross and full; the residual gradient summed over four propagations
#   one_pair         B = 1: the merged message's frames are views at a storage offset, BatchNorm over one pair's rows; layer 0 self
#                    with k = 8, layer 1 cross and full
#   square_triplet, square_superglue    three 64-point tiles, the last with 2 points; the equal-size losses beyond one tile
#   wide             M + 1 > 640: the nine-chunk Sinkhorn backward with its history and the streaming forward inside a step; 11 key
#                    tiles against one query tile in the cross layer
#               case,               loss_method,    B, N,   M,   L, k list,               first_pair
SHAPE_CASES = {'tiles':            ('gap_loss',     3, 70,  180, 2, [None, 16, 8, None], 40),
               'one_pair':         ('gap_loss',     1, 33,  95,  1, [8, None],           41),
               'square_triplet':   ('triplet_loss', 2, 130, 130, 1, [None, 32],          44),
               'square_superglue': ('superglue',    2, 130, 130, 1, [None, 32],          44),
               'wide':             ('gap_loss',     1, 24,  650, 1, [8],                 46)}
# what a shape case stores of the reference's results (``r:``): the loss, Z, every buffer and every gradient but the layers' four
# convolution weights (0.5 + 0.8 MB per layer); those are held to this restatement in float64, which the generator holds to the
# reference.  Every quantity has its measured error (``e:``).
SHAPE_UNSTORED = ('attn.proj.0.weight', 'attn.proj.1.weight', 'attn.proj.2.weight', 'attn.merge.weight', 'mlp.0.weight', 'mlp.3.weight')
SHAPE_PARTS = ('io', 'z', 'grads')
FILES.update({case: tuple(f'train_shape_{case}_{part}' for part in SHAPE_PARTS) for case in SHAPE_CASES})
ALL_FILES = tuple(f for fs in FILES.values() for f in fs)


def shape_stored(quantity):
    """Whether a shape case stores the reference's value of this quantity of ``flatten``."""
    return not (quantity.startswith('grad:gnn.layers.') and quantity.endswith(SHAPE_UNSTORED))


def case_spec(case):
    """(loss_method, B, N, M, L, k list, first_pair) of a case of CASES or SHAPE_CASES."""
    if case in CASES:
        method, B, n, m, first = CASES[case]
        return method, B, n, m, L, list(K_LIST), first
    method, B, n, m, Lc, k, first = SHAPE_CASES[case]
    return method, B, n, m, Lc, list(k), first


def config(method, L=L, k=K_LIST, **over):
    from mdgat_matcher_amd import synth
    return synth.default_config(L=L, k=list(k), sinkhorn_iterations=ITERS, loss_method=method, triplet_loss_gamma=GAMMA, **over)


def _dt():
    return R._DT[0]


def _f(x):
    return R._f(x)


def numpy_state(sd):
    """A state dict (torch tensors or arrays) as float64 / int64 numpy arrays, DataParallel's prefix stripped."""
    out = {}
    for k, v in sd.items():
        a = v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)
        out[k[7:] if k.startswith('module.') else k] = a.copy()
    return out


def is_buffer(name):
    return name.endswith(('running_mean', 'running_var', 'num_batches_tracked'))


def param_names(sd):
    return [k for k in sd if not is_buffer(k)]


# ---- the MLP stacks, called once per frame ----
def _mlp_p(sd, prefix, n):
    p = {'W': [sd[f'{prefix}.{3 * l}.weight'][:, :, 0] for l in range(n)], 'b': [sd[f'{prefix}.{3 * l}.bias'] for l in range(n)]}
    for k, name in (('gamma', 'weight'), ('beta', 'bias'), ('rm', 'running_mean'), ('rv', 'running_var')):
        p[k] = [sd[f'{prefix}.{3 * l + 1}.{name}'] for l in range(n - 1)]
    p['eps'], p['momentum'] = [EPS] * (n - 1), [MOMENTUM] * (n - 1)
    return p


class _Stack:
    """One MLP of the state dict run over the frames' rows in call order; keeps what its backward needs and writes the buffers it
    leaves into ``after``."""

    def __init__(self, sd, prefix, n, after, zs):
        self.prefix, self.n, self.p, self.after, self.zs = prefix, n, _mlp_p(sd, prefix, n), after, zs
        self.nbt = [int(sd[f'{prefix}.{3 * l + 1}.num_batches_tracked']) for l in range(n - 1)]
        self.calls = []

    def forward(self, xs, joint=False, swap=False):
        """xs: the rows of frame 0 and of frame 1 -> their outputs.  ``joint``: one call over both frames' rows (a planted mistake);
        ``swap``: frame 1 called before frame 0 (another)."""
        groups = [np.concatenate(xs)] if joint else list(xs)
        order = list(range(len(groups)))[::-1] if swap else list(range(len(groups)))
        outs = [None] * len(groups)
        self.calls = [None] * len(groups)
        for g in order:
            out, cache, (rm, rv) = R.forward(groups[g], self.p)
            self.p = dict(self.p, rm=rm, rv=rv)
            self.nbt = [v + 1 for v in self.nbt]
            outs[g], self.calls[g] = out, cache
            self.zs.extend(c['z'] for c in cache[:-1])
        for l in range(self.n - 1):
            self.after[f'{self.prefix}.{3 * l + 1}.running_mean'] = self.p['rm'][l]
            self.after[f'{self.prefix}.{3 * l + 1}.running_var'] = self.p['rv'][l]
            self.after[f'{self.prefix}.{3 * l + 1}.num_batches_tracked'] = np.int64(self.nbt[l])
        if joint:
            cut = xs[0].shape[0]
            return [outs[0][:cut], outs[0][cut:]]
        return outs

    def backward(self, douts, grads, joint=False, slab_rows=None):
        """douts per frame -> dx per frame; the parameters' gradients are summed into ``grads``.  ``slab_rows`` (a planted mistake): a
        call of more rows than that forms the dW of its last convolution from the first ``slab_rows`` rows alone."""
        groups = [np.concatenate(douts)] if joint else list(douts)
        dxs = []
        for cache, dout in zip(self.calls, groups):
            g = R.backward(cache, self.p, dout)
            if slab_rows is not None and dout.shape[0] > slab_rows:
                g['dW'][-1] = _f(dout)[:slab_rows].T @ cache[-1]['A'][:slab_rows]
            dxs.append(g['dx'])
            for l in range(self.n):
                _add(grads, f'{self.prefix}.{3 * l}.weight', g['dW'][l][:, :, None])
                _add(grads, f'{self.prefix}.{3 * l}.bias', g['db'][l])
            for l in range(self.n - 1):
                _add(grads, f'{self.prefix}.{3 * l + 1}.weight', g['dgamma'][l])
                _add(grads, f'{self.prefix}.{3 * l + 1}.bias', g['dbeta'][l])
        if joint:
            cut = douts[0].shape[0]
            return [dxs[0][:cut], dxs[0][cut:]]
        return dxs


def _add(grads, name, v):
    grads[name] = v if name not in grads else grads[name] + v


# ---- the head, the optimal transport, the loss: in the current precision ----
def head_forward(d0, d1, W, b):
    """scores [B, N, M] = final_proj(d0) final_proj(d1)^T / sqrt(128) (mdgat.py:397, 430-431) and the projected descriptors."""
    W, b = _f(W).reshape(128, 128), _f(b)
    md0, md1 = _f(d0) @ W.T + b, _f(d1) @ W.T + b
    s = 1 / np.sqrt(_dt()(128))
    return s * (md0 @ np.swapaxes(md1, 1, 2)), (md0, md1, s)


def head_backward(d0, d1, W, st, G):
    """(ddesc0, ddesc1, dW [128, 128], db)"""
    md0, md1, s = st
    W, G = _f(W).reshape(128, 128), _f(G)
    dmd0, dmd1 = s * (G @ md1), s * (np.swapaxes(G, 1, 2) @ md0)
    dW = dmd0.reshape(-1, 128).T @ _f(d0).reshape(-1, 128) + dmd1.reshape(-1, 128).T @ _f(d1).reshape(-1, 128)
    return dmd0 @ W, dmd1 @ W, dW, dmd0.sum(axis=(0, 1)) + dmd1.sum(axis=(0, 1))


def _lse(x, axis):
    m = x.max(axis=axis, keepdims=True)
    return np.squeeze(m, axis) + np.log(np.exp(x - m).sum(axis=axis))


def sinkhorn_forward(scores, alpha, iters):
    """log_optimal_transport (mdgat.py:279-308) as the reference writes it, in log space: (Z [B, N+1, M+1], state)."""
    scores = _f(scores)
    B, N, M = scores.shape
    dt = _dt()
    C = np.full((B, N + 1, M + 1), dt(alpha), dtype=dt)
    C[:, :N, :M] = scores
    norm = -np.log(dt(N + M))
    log_mu = np.concatenate([np.full(N, norm), [np.log(dt(M)) + norm]]).astype(dt)
    log_nu = np.concatenate([np.full(M, norm), [np.log(dt(N)) + norm]]).astype(dt)
    u, v = np.zeros((B, N + 1), dtype=dt), np.zeros((B, M + 1), dtype=dt)
    us, vs = [], [v]
    for _ in range(int(iters)):
        u = log_mu - _lse(C + v[:, None, :], 2)
        v = log_nu - _lse(C + u[:, :, None], 1)
        us.append(u)
        vs.append(v)
    return C + u[:, :, None] + v[:, None, :] - norm, (C, log_mu, log_nu, us, vs)


def sinkhorn_backward(st, G):
    """The iterations walked backwards: (dscores [B, N, M], dalpha summed over the batch)."""
    C, log_mu, log_nu, us, vs = st
    G = _f(G)
    N, M = C.shape[1] - 1, C.shape[2] - 1
    gC, gu, gv = G.copy(), G.sum(axis=2), G.sum(axis=1)
    for t in range(len(us) - 1, -1, -1):
        x = C + us[t][:, :, None]                                   # v_t = log_nu - lse_i(C + u_t)
        P = np.exp(x - _lse(x, 1)[:, None, :]) * gv[:, None, :]
        gC -= P
        gu = gu - P.sum(axis=2)
        x = C + vs[t][:, None, :]                                   # u_t = log_mu - lse_j(C + v_{t-1})      (vs[0] = 0)
        P = np.exp(x - _lse(x, 2)[:, :, None]) * gu[:, :, None]
        gC -= P
        gv = -P.sum(axis=1)
        gu = np.zeros_like(gu)
    dalpha = gC[:, N, :].sum() + gC[:, :N, M].sum()
    return gC[:, :N, :M], dalpha


def _t(z):
    with np.errstate(divide='ignore', over='ignore', under='ignore'):
        return -np.log(np.exp(z))


def _dt_dz(g, z):
    with np.errstate(all='ignore'):
        e = np.exp(z)
        return (-_f(g) / e) * e


def _clamp0(x):
    return np.where(x < 0, 0, x)


def loss_pair(z, g0, g1, method, gamma, w=None):
    """One pair's loss (loss_ref.pair_losses) and, with the upstream weight ``w``, its gradient w dloss / dZ (loss_grad_ref.pair_grads),
    for gts inside their range and a Z on which exp does not underflow."""
    z = _f(z)
    n, m = z.shape[0] - 1, z.shape[1] - 1
    g0, g1 = np.asarray(g0, dtype=np.int64), np.asarray(g1, dtype=np.int64)
    p0, p1 = np.where(g0 == -1, m, g0), np.where(g1 == -1, n, g1)
    rows, cols = np.arange(n), np.arange(m)
    d = None if w is None else np.zeros_like(z)
    gamma = _dt()(gamma)
    if method == 'superglue':
        un = g1 == -1
        loss = (-z[rows, p0].sum() - z[n, cols[un]].sum()) / (un.sum() + m)
        if d is not None:
            d[rows, p0] = -w / (un.sum() + m)
            d[n, cols[un]] = -w / (un.sum() + m)
        return loss, d
    keep_r = np.ones((n, m + 1), dtype=bool)
    keep_r[rows, p0] = False
    keep_c = np.ones((n + 1, m), dtype=bool)
    keep_c[p1, cols] = False
    if method == 'triplet_loss':
        neg_r = np.where(keep_r, z[:n, :], -np.inf).argmax(axis=1)
        neg_c = np.where(keep_c, z[:, :m], -np.inf).argmax(axis=0)
        x_r = _t(z[rows, p0]) - _t(z[rows, neg_r]) + gamma
        x_c = _t(z[p1, cols]) - _t(z[neg_c, cols]) + gamma
        loss = np.concatenate([_clamp0(x_r), _clamp0(x_c)]).mean()
        if d is not None:
            wt = w / (n + m)
            w_r, w_c = np.where(x_r >= 0, wt, 0), np.where(x_c >= 0, wt, 0)
            d[rows, p0] += _dt_dz(w_r, z[rows, p0])
            d[rows, neg_r] += _dt_dz(-w_r, z[rows, neg_r])
            d[p1, cols] += _dt_dz(w_c, z[p1, cols])
            d[neg_c, cols] += _dt_dz(-w_c, z[neg_c, cols])
        return loss, d
    assert method == 'gap_loss', method
    tz = _t(z)
    X_r = tz[rows, p0][:, None] - tz[:n, :] + gamma
    pi, pj = np.nonzero(~keep_c)                      # the positives and the others of Z[:, :m], each row-major (loss_ref explains)
    vi, vj = np.nonzero(keep_c)
    vi, vj = vi.reshape(n, m), vj.reshape(n, m)
    X_c = tz[pi, pj][None, :] - tz[vi, vj] + gamma
    row, col = np.where(keep_r, _clamp0(X_r), 0).sum(axis=1), _clamp0(X_c).sum(axis=0)
    loss = (np.mean(2 * np.log(row + 1)) + np.mean(2 * np.log(col + 1))) / 2
    if d is not None:
        act = keep_r & (X_r >= 0)
        w_r = w / (n * (row + 1))
        g = _dt_dz(np.where(act, -w_r[:, None], 0), z[:n, :])
        g[rows, p0] = act.sum(axis=1) * _dt_dz(w_r, z[rows, p0])
        d[:n, :] += g
        act = X_c >= 0
        w_c = w / (m * (col + 1))
        d[vi, vj] += _dt_dz(np.where(act, -w_c[None, :], 0), z[vi, vj])
        d[pi, pj] += act.sum(axis=0) * _dt_dz(w_c, z[pi, pj])
    return loss, d


def loss_forward_backward(Z, gt0, gt1, method, gamma):
    """(the module's ``loss`` - 0-d for superglue / triplet, [B] for gap -, dZ of ``loss.mean()``)."""
    B = Z.shape[0]
    w = 1 / _dt()(B)
    pairs = [loss_pair(Z[b], gt0[b], gt1[b], method, gamma, w) for b in range(B)]
    per = np.array([p[0] for p in pairs], dtype=_dt())
    return (per if method == 'gap_loss' else per.mean()), np.stack([p[1] for p in pairs])


# ---- the step ----
def topk_schedule(L, k_list):
    n = len(k_list)
    return [0 if not (i > 2 * L - 1 - n) or k_list[i - 2 * L + n] is None else int(k_list[i - 2 * L + n]) for i in range(2 * L)]


def _whole_tiles(nq):
    """The planted 'tile_tail': of nq queries, how many still reach dk and dv - those of the whole tiles of TILE_QUERIES.  A frame of
    less than one tile has no ragged tail BEHIND a whole tile: its only tile is the one every kernel runs, so it is left alone (which is
    what makes the plant invisible to the small fixtures)."""
    return nq if nq < TILE_QUERIES else TILE_QUERIES * (nq // TILE_QUERIES)


def step(sd, data, method, gamma=GAMMA, L=L, k_list=K_LIST, iters=ITERS, masks=None, plant=None):
    """One forward and ``loss.mean().backward()`` in the current precision.

    sd: ``numpy_state`` of the module BEFORE the step; data: 'keypoints0/1' [B, N, 3], 'scores0/1', 'descriptors0/1' [B, N, 33],
    'gt_matches0/1'.  ``masks``: per layer the top-k masks to use (None: decided here on the float64 logits).
    Returns {'loss', 'Z', 'grads': {parameter name: gradient in the parameter's shape}, 'after': {buffer name: value after the
    step}, 'z': the BN inputs (list of arrays, for the ReLU condition), 'masks': per layer, 'topk_gap'}."""
    assert plant is None or plant in PLANTS, plant
    sd = dict(sd)
    if plant == 'final_proj_entry':
        W = sd['final_proj.weight'].copy()
        W[5, 7, 0] *= 1 + 1e-6
        sd['final_proj.weight'] = W
    grads, after, zs = {}, {}, []
    B, N, M = data['keypoints0'].shape[0], data['keypoints0'].shape[1], data['keypoints1'].shape[1]
    kin = [np.concatenate([_f(data[f'keypoints{f}']), _f(data[f'scores{f}'])[..., None]], axis=-1).reshape(-1, 4) for f in (0, 1)]
    din = [_f(data[f'descriptors{f}']).reshape(-1, 33) for f in (0, 1)]
    denc, kenc = _Stack(sd, 'denc.encoder', 3, after, zs), _Stack(sd, 'kenc.encoder', 4, after, zs)
    joint, swap = plant == 'joint_bn', plant == 'frame_order'
    de, ke = denc.forward(din, joint, swap), kenc.forward(kin, joint, swap)
    d = [(de[f] + ke[f]).reshape(B, -1, 128) for f in (0, 1)]
    sched = topk_schedule(L, k_list)
    layers, used_masks, topk_gap = [], [], np.inf
    for i in range(2 * L):
        pre, cross, k = f'gnn.layers.{i}', bool(i % 2), sched[i]
        w = {c: sd[f'{pre}.attn.proj.{j}.weight'][:, :, 0] for j, c in enumerate('qkv')}
        bq = {c: sd[f'{pre}.attn.proj.{j}.bias'] for j, c in enumerate('qkv')}
        Wm, bm = _f(sd[f'{pre}.attn.merge.weight'][:, :, 0]), _f(sd[f'{pre}.attn.merge.bias'])
        WmP = Wm if plant == 'no_perm_merge' else Wm[:, PERM]
        desc = np.concatenate(d, axis=1)
        qkv = np.stack([desc @ _f(w[c])[PERM].T + _f(bq[c])[PERM] for c in 'qkv'], axis=2).reshape(B, N + M, 3, 4, 32)
        mk = None
        if k > 0:
            if masks is not None:
                mk = masks[i]
            else:
                mk, gap = A.topk_masks(np.asarray(qkv, dtype=np.float64), N, M, cross, k)
                topk_gap = min(topk_gap, gap)
        used_masks.append(mk)
        msg, _ = R._attention(qkv, N, M, cross, mk)
        merged = msg @ WmP.T + bm
        mlp = _Stack(sd, f'{pre}.mlp', 2, after, zs)
        rows = (slice(0, N), slice(N, N + M))
        X = [np.concatenate([d[f], merged[:, rows[f]]], axis=2).reshape(-1, 256) for f in (0, 1)]
        delta = mlp.forward(X, joint, swap)
        layers.append({'pre': pre, 'cross': cross, 'mk': mk, 'w': w, 'WmP': WmP, 'desc': desc, 'qkv': qkv, 'msg': msg, 'mlp': mlp})
        d = [delta[f].reshape(B, -1, 128) + (0 if plant == 'no_residual' else d[f]) for f in (0, 1)]
    scores, hst = head_forward(d[0], d[1], sd['final_proj.weight'], sd['final_proj.bias'])
    Z, sst = sinkhorn_forward(scores, sd['bin_score'], iters)
    loss, dZ = loss_forward_backward(Z, data['gt_matches0'], data['gt_matches1'], method, gamma)
    # ---- backward ----
    dscores, dalpha = sinkhorn_backward(sst, dZ)
    grads['bin_score'] = np.zeros_like(dalpha) if plant == 'no_bin_grad' else dalpha
    g0, g1, dW, db = head_backward(d[0], d[1], sd['final_proj.weight'], hst, dscores)
    grads['final_proj.weight'], grads['final_proj.bias'] = dW[:, :, None], db
    dd = [g0, g1]
    for ly in reversed(layers):
        pre, mlp = ly['pre'], ly['mlp']
        dX = [v.reshape(B, -1, 256) for v in mlp.backward([g.reshape(-1, 128) for g in dd], grads, joint,
                                                          slab_rows=SLAB_ROWS if plant == 'second_slab' else None)]
        dmerged = np.concatenate([dX[0][..., 128:], dX[1][..., 128:]], axis=1)
        dd = [dX[f][..., :128] + (0 if plant == 'no_residual' else dd[f]) for f in (0, 1)]
        dWm = np.zeros((128, 128), dtype=_dt())
        prod = dmerged.reshape(-1, 128).T @ ly['msg'].reshape(-1, 128)
        if plant == 'no_perm_merge':
            dWm = prod
        else:
            dWm[:, PERM] = prod
        grads[f'{pre}.attn.merge.weight'], grads[f'{pre}.attn.merge.bias'] = dWm[:, :, None], dmerged.sum(axis=(0, 1))
        _, dqkv = R._attention(ly['qkv'], N, M, ly['cross'], ly['mk'], dmerged @ ly['WmP'], kv_queries=_whole_tiles if plant == 'tile_tail' else None)
        dqkv = dqkv.reshape(B, N + M, 3, 128)
        ddesc = np.zeros_like(ly['desc'])
        for j, c in enumerate('qkv'):
            dq = dqkv[:, :, j]
            dW, db = np.zeros((128, 128), dtype=_dt()), np.zeros(128, dtype=_dt())
            dW[PERM], db[PERM] = dq.reshape(-1, 128).T @ ly['desc'].reshape(-1, 128), dq.sum(axis=(0, 1))
            grads[f'{pre}.attn.proj.{j}.weight'], grads[f'{pre}.attn.proj.{j}.bias'] = dW[:, :, None], db
            if plant == 'cross_kv_grad' and ly['cross'] and c in 'kv':
                continue                # the planted mistake: a frame's gradient through the OTHER frame's queries is dropped
            ddesc = ddesc + dq @ _f(ly['w'][c])[PERM]
        dd = [dd[0] + ddesc[:, :N], dd[1] + ddesc[:, N:]]
    flat = [g.reshape(-1, 128) for g in dd]
    kenc.backward(flat, grads, joint)
    denc.backward(flat, grads, joint)
    return {'loss': loss, 'Z': Z, 'grads': grads, 'after': after, 'z': zs, 'masks': used_masks, 'topk_gap': topk_gap}


def sgd(sd, grads, after, lr=SGD_LR):
    """The state after ``p -= lr * grad`` on every parameter, with the buffers the step left (float64, as the module holds it)."""
    out = {}
    for k, v in sd.items():
        if k in grads:
            out[k] = np.asarray(_f(v) - lr * np.asarray(grads[k]).reshape(np.shape(v)), dtype=np.float64)
        else:
            out[k] = np.asarray(after[k], dtype=v.dtype) if k in after else v
    return out


# ---- the measured bound ----
ZERO_GRAD_BIASES = ('attn.proj.1.bias', 'attn.proj.2.bias', 'attn.merge.bias', 'mlp.0.bias', 'kenc.encoder.0.bias', 'kenc.encoder.3.bias',
                    'kenc.encoder.6.bias', 'denc.encoder.0.bias', 'denc.encoder.3.bias')


def flatten(res):
    """{'loss', 'Z', 'grad:<parameter>', 'buf:<float buffer>'} of a ``step`` result (or of a recorded one in the same form)."""
    q = {'loss': np.asarray(res['loss']), 'Z': res['Z']}
    q.update({'grad:' + k: v for k, v in res['grads'].items()})
    q.update({'buf:' + k: v for k, v in res['after'].items() if not k.endswith('num_batches_tracked')})
    return q


def measure(recorded, mine, truth):
    """{quantity: err}: per quantity of ``flatten`` the larger deviation of the reference's float64 result (``recorded``) and of this
    restatement's (``mine``) from the 80-bit evaluation ``truth``, with the floor of the gradients that are zero in exact arithmetic."""
    dev = lambda a, b: float(np.abs(np.asarray(a, dtype=np.longdouble).reshape(np.shape(b)) - b).max())          # noqa: E731
    err = {}
    for k, t in truth.items():
        if k not in recorded:
            continue
        err[k] = max(dev(recorded[k], t), dev(mine[k], t))
        if k.startswith('grad:') and k.endswith(ZERO_GRAD_BIASES):
            err[k] = max(err[k], 4.0 * U * float(np.abs(np.asarray(mine[k[:-4] + 'weight'], dtype=np.float64)).max()))
    return err


def reference_error(sd, data, method, recorded, **kw):
    """(err by quantity, this restatement's float64 result, the 80-bit one) for one step; ``recorded``: ``flatten`` of the reference's."""
    if np.finfo(np.longdouble).eps > 2.0 ** -60:
        raise RuntimeError('the measured bound needs an extended-precision long double (x86)')
    mine = step(sd, data, method, **kw)
    with R.precision(np.longdouble):
        truth = step(sd, data, method, masks=mine['masks'], **kw)
    err = measure(recorded, flatten(mine), flatten(truth))
    # the BN inputs: this restatement's error alone (the reference does not expose them), for the ReLU condition
    err_z = [float(np.abs(np.asarray(a, dtype=np.longdouble) - b).max()) for a, b in zip(mine['z'], truth['z'])]
    return err, mine, truth, err_z


def compare(got, want, err, names=None):
    """max over the quantities of max|got - want| / (32 err): (worst, where, {quantity: fraction})."""
    fr = {}
    for k in (names if names is not None else want):
        a, b = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        a = a.reshape(b.shape)
        diff = float(np.abs(a - b).max()) if b.size else 0.0
        fr[k] = 0.0 if diff == 0.0 else (np.inf if err[k] == 0.0 else diff / (FACTOR * err[k]))
    where = max(fr, key=fr.get)
    return fr[where], where, fr


# ---- fixtures ----
def load(golden_dir, case):
    """One recorded case: {'data': the inputs (numpy), 'want': ``flatten``-style dict of the reference's results, 'err': by quantity,
    'nbt': {buffer name: value after}, 'matches0/1', 'mscores0/1'; for 'gap' also 'step2': {'want', 'err'}}."""
    g = R.load_files(golden_dir, FILES[case])
    data = {k: g['in:' + k] for k in ('keypoints0', 'scores0', 'descriptors0', 'keypoints1', 'scores1', 'descriptors1', 'gt_matches0', 'gt_matches1')}
    want = {k[2:]: g[k] for k in g if k.startswith('r:')}
    err = {k[2:]: float(g[k]) for k in g if k.startswith('e:')}
    out = {'data': data, 'want': want, 'err': err, 'nbt': {k[4:]: int(g[k]) for k in g if k.startswith('nbt:')},
           'matches0': g['matches0'], 'matches1': g['matches1'], 'mscores0': g['mscores0'], 'mscores1': g['mscores1']}
    if case == 'gap':
        out['step2'] = {'want': {k[3:]: g[k] for k in g if k.startswith('r2:')}, 'err': {k[3:]: float(g[k]) for k in g if k.startswith('e2:')}}
    return out


def shape_want(c, res):
    """What a step of a shape case is held to: the reference's recorded value where the fixture ``c`` stores one, this restatement's
    float64 result ``res`` (which the generator held to the reference) for the layers' convolution weights."""
    mine = flatten(res)
    assert set(mine) == set(c['err']) and set(c['want']) <= set(mine)
    return {k: c['want'].get(k, v) for k, v in mine.items()}


def initial_state(seed=SEED, L=L):
    from mdgat_matcher_amd import synth
    return synth.make_state_dict(L, seed)


def golden_path(golden_dir, name):
    return os.path.join(golden_dir, name + '.npz')
