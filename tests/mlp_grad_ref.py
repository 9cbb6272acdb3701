"""fp64 restatement of the reference's ``MLP(channels)`` (models/mdgat.py:34-46) with BatchNorm in TRAINING mode, of its gradient and of
the running-buffer update: the yardstick of csrc/mlp_grad.hip.  numpy, no autograd.

Rows are points: x [R, K] (a second source is concatenated by the caller), W_l [C_l, C_in], b_l, and for every convolution but the last
gamma_l, beta_l, running mean / var, eps, momentum.  ``p`` is a dict of lists: 'W', 'b', 'gamma', 'beta', 'rm', 'rv', 'eps', 'momentum'.

    Y_l = A_{l-1} W_l^T + b_l
    mean = colmean(Y),  d = Y - mean,  var = colmean(d^2)  (two passes, biased),  invstd = 1 / sqrt(var + eps)
    yhat = d invstd,  z = gamma yhat + beta,  A_l = max(z, 0)
    rm' = (1 - m) rm + m mean,   rv' = (1 - m) rv + m var R / (R - 1)          (eval mode: mean = rm, var = rv, nothing moves)

and with dY_L = dout, from the last convolution to the first:

    db_l = colsum(dY_l),  dW_l = dY_l^T A_{l-1},  dA_{l-1} = dY_l W_l
    dz = dA [z > 0]  (zero is not positive),  dbeta = colsum(dz),  dgamma = colsum(dz yhat)
    dY_{l-1} = gamma invstd (dz - dbeta / R - yhat dgamma / R)                 (eval mode: gamma invstd dz)

The error bound (``tolerances``), derived as head_grad_ref derives its own: a dot product of length K in fp64, in any order, with or
without FMA, is off by at most K u sum|a_k b_k| to first order, u = 2^-53; the formulas rerun on absolute values give the magnitudes,
and an error an operand arrives with is carried through the same products.  Forward, per layer (e_X: absolute error of X):

    e_Y    = K u (|A||W|^T + |b|) + e_A |W|^T
    e_mean = colmean(e_Y) + R u colmean|Y|
    e_d    = e_Y + e_mean + u |d|
    e_var  = 2 colmean(|d| e_d) + R u var
    r_inv  = e_var / (2 (var + eps)) + 2 u                   the RELATIVE error of invstd.  With e_Y of the order K u (|mean| + std) and
                                                             |d| of the order std this is K u (1 + |mean| / std): a channel far from
                                                             zero loses the digits of its offset - the term BN brings
    e_yhat = e_d invstd + |yhat| (r_inv + u)
    e_z    = |gamma| e_yhat + 2 u (|gamma yhat| + |beta|)    = e_A of the next layer (max(., 0) is 1-Lipschitz); its magnitude
                                                             |A| <= |gamma||yhat| + |beta|
    eval mode: e_mean = 0, r_inv = 2 u (the running statistics are given)
    rm', rv': e_mean and e_var R / (R - 1) times m, plus 3 u of the magnitudes

Backward (e_G: the error dY_l arrives with; |.| magnitudes on absolute values; the mask is taken as decided - ``relu_margin`` is the
test's condition that it is):

    db: colsum(e_G) + R u colsum|G|             dW: e_G^T |A| + |G|^T e_A + R u |G|^T |A|
    e_dA = e_G |W| + C_out u |G||W|,  e_dz = e_dA [z > 0]
    dbeta: colsum(e_dz) + R u colsum|dz|        dgamma: colsum(e_dz |yhat| + |dz| e_yhat) + R u colsum|dz yhat|
    T = |dz| + colsum|dz| / R + |yhat| colsum|dz yhat| / R                                   the magnitude of the bracket
    e_dY = |gamma| invstd (e_dz + e_dbeta / R + e_yhat colsum|dz yhat| / R + |yhat| e_dgamma / R + 3 u T + T (r_inv + 2 u))
    eval mode: e_dY = |gamma| invstd (e_dz + |dz| (r_inv + 2 u))

r_inv multiplies yhat and, through yhat, dgamma and dY.  Tolerance per entry: 4 x the above - a factor 2 for the two implementations
compared, 2 for the first-order truncation."""
import os

import numpy as np

U = 2.0 ** -53
#  case -> the fixture files that hold it (tools/make_goldens_mlp_grad.py)
GOLDEN_FILES = {'kenc': ('mlp_grad_kenc',), 'denc': ('mlp_grad_denc',), 'denc_eval': ('mlp_grad_denc_eval',),
                'layer': ('mlp_grad_layer_inputs', 'mlp_grad_layer_grads')}
ALL_FILES = tuple(f for fs in GOLDEN_FILES.values() for f in fs)
STACKS = {'kenc': (4, 32, 64, 128, 128), 'denc': (33, 64, 128, 128), 'layer': (256, 256, 128), 'conv128': (128, 128), 'conv384': (128, 384), 'ragged': (8, 48, 80, 16)}


_DT = [np.float64]


def _f(x):
    return np.asarray(x, dtype=_DT[0])


class precision:
    """``with precision(np.longdouble):`` - the restatement runs in that type (x86's 80-bit format: u = 2^-64) instead of float64."""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.old, _DT[0] = _DT[0], self.dtype

    def __exit__(self, *exc):
        _DT[0] = self.old


def n_bn(p):
    return len(p['W']) - 1


def random_params(channels, seed, mean_shift=0.0):
    """Seeded parameters and buffers of MLP(channels): weights 1.6 / sqrt(C_in) randn (activations keep their scale), non-trivial
    gamma / beta and running statistics."""
    rs = np.random.RandomState(seed)
    p = {k: [] for k in ('W', 'b', 'gamma', 'beta', 'rm', 'rv', 'eps', 'momentum')}
    for l in range(1, len(channels)):
        p['W'].append(rs.standard_normal((channels[l], channels[l - 1])) * (1.6 / np.sqrt(channels[l - 1])))
        p['b'].append(rs.standard_normal(channels[l]) * 0.1 + mean_shift)
        if l < len(channels) - 1:
            p['gamma'].append(1.0 + 0.2 * rs.standard_normal(channels[l]))
            p['beta'].append(0.2 * rs.standard_normal(channels[l]))
            p['rm'].append(0.1 * rs.standard_normal(channels[l]))
            p['rv'].append(1.0 + 0.5 * rs.random_sample(channels[l]))
            p['eps'].append(1e-5)
            p['momentum'].append(0.1)
    return p


def forward(x, p, training=True, variance='two_pass', normalise_unbiased=False, running_biased=False):
    """(out [R, C_L], cache, (rm', rv')).  cache: per layer the dict of A (the layer's input), Y, mean, var, invstd, yhat, z.
    The keyword arguments plant the mistakes the tests must catch: ``variance='one_pass'`` forms E[y^2] - E[y]^2,
    ``normalise_unbiased`` divides by R - 1 in the normalisation, ``running_biased`` puts the biased variance into running_var."""
    A = _f(x)
    R = A.shape[0]
    cache, rm_new, rv_new = [], [], []
    L = len(p['W'])
    for l in range(L):
        Y = A @ _f(p['W'][l]).T + _f(p['b'][l])
        c = {'A': A, 'Y': Y}
        cache.append(c)
        if l == L - 1:
            return Y, cache, (rm_new, rv_new)
        if training:
            mean = Y.mean(axis=0)
            d = Y - mean
            var = (Y * Y).mean(axis=0) - mean * mean if variance == 'one_pass' else (d * d).mean(axis=0)
            m = p['momentum'][l]
            rm_new.append((1 - m) * _f(p['rm'][l]) + m * mean)
            rv_new.append((1 - m) * _f(p['rv'][l]) + m * (var if running_biased else var * R / (R - 1)))
            if normalise_unbiased:
                var = var * R / (R - 1)
        else:
            mean, var = _f(p['rm'][l]), _f(p['rv'][l])
            d = Y - mean
            rm_new.append(mean.copy())
            rv_new.append(var.copy())
        invstd = 1.0 / np.sqrt(var + p['eps'][l])
        yhat = d * invstd
        z = _f(p['gamma'][l]) * yhat + _f(p['beta'][l])
        c.update(mean=mean, var=var, invstd=invstd, yhat=yhat, z=z)
        A = np.maximum(z, 0.0)


def backward(cache, p, dout, training=True, drop_dgamma=False, mask_ge=False):
    """{'dx', 'dW': [...], 'db': [...], 'dgamma': [...], 'dbeta': [...]}.  ``drop_dgamma`` / ``mask_ge`` plant mistakes."""
    G = _f(dout)
    R = G.shape[0]
    L = len(p['W'])
    g = {'dW': [None] * L, 'db': [None] * L, 'dgamma': [None] * (L - 1), 'dbeta': [None] * (L - 1)}
    for l in range(L - 1, -1, -1):
        g['db'][l] = G.sum(axis=0)
        g['dW'][l] = G.T @ cache[l]['A']
        dA = G @ _f(p['W'][l])
        if l == 0:
            g['dx'] = dA
            return g
        c = cache[l - 1]
        dz = np.where(c['z'] >= 0.0 if mask_ge else c['z'] > 0.0, dA, 0.0)
        g['dbeta'][l - 1] = dz.sum(axis=0)
        g['dgamma'][l - 1] = (dz * c['yhat']).sum(axis=0)
        k = _f(p['gamma'][l - 1]) * c['invstd']
        if training:
            G = k * (dz - g['dbeta'][l - 1] / R - (0.0 if drop_dgamma else c['yhat'] * g['dgamma'][l - 1] / R))
        else:
            G = k * dz


def tolerances(x, p, dout=None, training=True):
    """Per entry 4 x the first-order error of the module docstring: {'out', 'z': [...] per BN layer, 'rm': [...], 'rv': [...]} and with
    dout {'dx', 'dW', 'db', 'dgamma', 'dbeta'}."""
    _, cache, _ = forward(x, p, training)
    R = np.shape(x)[0]
    L = len(p['W'])
    t = {'z': [], 'rm': [], 'rv': []}
    eA, mA = np.zeros_like(_f(x)), np.abs(_f(x))
    fw = []
    for l in range(L):
        aW, K = np.abs(_f(p['W'][l])), np.shape(p['W'][l])[1]
        eY = K * U * (mA @ aW.T + np.abs(_f(p['b'][l]))) + eA @ aW.T
        fw.append({'eA': eA, 'mA': mA})
        if l == L - 1:
            t['out'] = 4.0 * eY
            break
        c = cache[l]
        d = np.abs(c['Y'] - c['mean'])
        if training:
            e_mean = eY.mean(axis=0) + R * U * np.abs(c['Y']).mean(axis=0)
            e_d = eY + e_mean + U * d
            e_var = 2.0 * (d * e_d).mean(axis=0) + R * U * c['var']
            r_inv = e_var / (2.0 * (c['var'] + p['eps'][l])) + 2.0 * U
            m = p['momentum'][l]
            t['rm'].append(4.0 * (m * e_mean + 3.0 * U * ((1 - m) * np.abs(_f(p['rm'][l])) + m * np.abs(c['mean']))))
            t['rv'].append(4.0 * (m * e_var * R / (R - 1) + 3.0 * U * ((1 - m) * np.abs(_f(p['rv'][l])) + m * c['var'] * R / (R - 1))))
        else:
            e_d = eY + U * d
            r_inv = 2.0 * U * np.ones_like(c['var'])
            t['rm'].append(np.zeros_like(c['mean']))
            t['rv'].append(np.zeros_like(c['var']))
        ayhat, ag, ab = np.abs(c['yhat']), np.abs(_f(p['gamma'][l])), np.abs(_f(p['beta'][l]))
        e_yhat = e_d * c['invstd'] + ayhat * (r_inv + U)
        e_z = ag * e_yhat + 2.0 * U * (ag * ayhat + ab)
        t['z'].append(4.0 * e_z)
        fw[-1].update(e_yhat=e_yhat, r_inv=r_inv)
        eA, mA = e_z, ag * ayhat + ab
    if dout is None:
        return t
    G = np.abs(_f(dout))
    eG = np.zeros_like(G)
    t.update(dW=[None] * L, db=[None] * L, dgamma=[None] * (L - 1), dbeta=[None] * (L - 1))
    for l in range(L - 1, -1, -1):
        aW, Cout = np.abs(_f(p['W'][l])), np.shape(p['W'][l])[0]
        t['db'][l] = 4.0 * (eG.sum(axis=0) + R * U * G.sum(axis=0))
        t['dW'][l] = 4.0 * (eG.T @ fw[l]['mA'] + G.T @ fw[l]['eA'] + R * U * (G.T @ fw[l]['mA']))
        e_dA, m_dA = eG @ aW + Cout * U * (G @ aW), G @ aW
        if l == 0:
            t['dx'] = 4.0 * e_dA
            return t
        c, f = cache[l - 1], fw[l - 1]
        mask = c['z'] > 0.0
        e_dz, dz, ayhat = e_dA * mask, m_dA * mask, np.abs(c['yhat'])
        s1, s2 = dz.sum(axis=0), (dz * ayhat).sum(axis=0)
        e_dbeta = e_dz.sum(axis=0) + R * U * s1
        e_dgamma = (e_dz * ayhat + dz * f['e_yhat']).sum(axis=0) + R * U * s2
        t['dbeta'][l - 1], t['dgamma'][l - 1] = 4.0 * e_dbeta, 4.0 * e_dgamma
        k = np.abs(_f(p['gamma'][l - 1])) * c['invstd']
        if training:
            T = dz + s1 / R + ayhat * s2 / R
            eG = k * (e_dz + e_dbeta / R + f['e_yhat'] * s2 / R + ayhat * e_dgamma / R + 3.0 * U * T + T * (f['r_inv'] + 2.0 * U))
            G = k * T
        else:
            eG = k * (e_dz + dz * (f['r_inv'] + 2.0 * U))
            G = k * dz


def relu_margin(x, p, training=True):
    """The ReLU condition: min over every BN layer and entry of |z| / (the entry's bound).  Below 1 an entry is undecided - two correct
    implementations may mask differently; the tests ask for 1e3 of everything they feed the kernel."""
    _, cache, _ = forward(x, p, training)
    tz = tolerances(x, p, None, training)['z']
    worst = np.inf
    for c, tol in zip(cache, tz):
        with np.errstate(divide='ignore'):
            worst = min(worst, float((np.abs(c['z']) / tol).min()))
    return worst


def worst_fraction(got, want, tol):
    """max over the entries of |got - want| / tol (0 / 0 counts as 0, x / 0 as inf)."""
    got, want, tol = [_f(v) for v in (got, want, tol)]
    assert got.shape == want.shape == tol.shape, (got.shape, want.shape, tol.shape)
    if got.size == 0:
        return 0.0
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(err == 0.0, 0.0, err / tol)
    return float(frac.max())


def compare_grads(got, want, tol):
    """Worst fraction over a gradient dict ({'dx', 'dW': [...], ...}); names missing from ``got`` are skipped."""
    worst = 0.0
    for k, w in want.items():
        if k not in got or got[k] is None or k not in tol:
            continue
        if isinstance(w, list):
            for a, b, c in zip(got[k], w, tol[k]):
                worst = max(worst, worst_fraction(np.reshape(a, np.shape(b)), b, c))
        else:
            worst = max(worst, worst_fraction(got[k], w, tol[k]))
    return worst


# ---- the seeded inputs of the GPU tests (tests/test_gpu_mlp_grad.py), checked for the ReLU condition on the CPU ----
GPU_ROWS = (2, 17, 64, 65, 1000, 1024)
GPU_STACKS = ('kenc', 'denc', 'layer', 'conv128', 'conv384', 'ragged')


def gpu_case(stack, R, seed=None):
    """(x [R, K], params, dout [R, C_L]) of one GPU-test case; 'layer' splits x into two sources of 128 in the test."""
    ch = STACKS[stack]
    seed = 7000 + 31 * GPU_STACKS.index(stack) + R if seed is None else seed
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((R, ch[0]))
    return x, random_params(ch, seed + 1), rs.standard_normal((R, ch[-1]))


def offset_case(R=64, seed=7700):
    """The case whose channels sit at mean 1e4 with spread 1: a 16 -> 32 -> 16 stack whose first bias is 1e4."""
    rs = np.random.RandomState(seed)
    p = random_params((16, 32, 16), seed + 1)
    p['W'][0] = p['W'][0] / 1.6
    p['b'][0] = p['b'][0] + 1e4
    return rs.standard_normal((R, 16)), p, rs.standard_normal((R, 16))


def dead_constant_case(R=40, seed=7800):
    """A 16 -> 32 -> 16 stack in which channel 3 of the hidden layer is dead for the whole batch (z < 0 everywhere: gamma = 0,
    beta = -1) and channel 5 is constant (a zero weight row: var = 0)."""
    rs = np.random.RandomState(seed)
    p = random_params((16, 32, 16), seed + 1)
    p['gamma'][0][3], p['beta'][0][3] = 0.0, -1.0
    p['W'][0][5] = 0.0
    p['beta'][0][5] = 0.25
    return rs.standard_normal((R, 16)), p, rs.standard_normal((R, 16))


def torch_stack(p, training):
    """The equivalent torch nn.Sequential (float64, CPU) of the parameter dict ``p``: what autograd and the device ops are handed."""
    import torch
    mods = []
    L = len(p['W'])
    for l in range(L):
        c = torch.nn.Conv1d(p['W'][l].shape[1], p['W'][l].shape[0], 1).double()
        with torch.no_grad():
            c.weight.copy_(torch.from_numpy(p['W'][l])[:, :, None])
            c.bias.copy_(torch.from_numpy(p['b'][l]))
        mods.append(c)
        if l < L - 1:
            b = torch.nn.BatchNorm1d(p['W'][l].shape[0], eps=p['eps'][l], momentum=p['momentum'][l]).double()
            with torch.no_grad():
                b.weight.copy_(torch.from_numpy(p['gamma'][l]))
                b.bias.copy_(torch.from_numpy(p['beta'][l]))
                b.running_mean.copy_(torch.from_numpy(p['rm'][l]))
                b.running_var.copy_(torch.from_numpy(p['rv'][l]))
            mods += [b, torch.nn.ReLU()]
    return torch.nn.Sequential(*mods).train(training)


# ---- fixtures ----
def load_files(golden_dir, names):
    out = {}
    for name in names:
        with np.load(os.path.join(golden_dir, name + '.npz')) as z:
            out.update({k: z[k] for k in z.files})
    return out


def load_case(golden_dir, case):
    """One recorded MLP case: {'p': params with the buffers BEFORE the calls, 'training', 'frames': [(x, dout, out, dx), ...] in call
    order, 'grads': the parameters' gradients of sum over the frames of (out * dout).sum(), 'rm_after', 'rv_after', 'nbt_after'}."""
    g = load_files(golden_dir, GOLDEN_FILES[case])
    L = int(g['n_conv'])
    p = {'W': [g[f'W{l}'] for l in range(L)], 'b': [g[f'b{l}'] for l in range(L)]}
    for k in ('gamma', 'beta', 'rm', 'rv'):
        p[k] = [g[f'{k}{l}'] for l in range(L - 1)]
    p['eps'], p['momentum'] = [float(v) for v in g['eps']], [float(v) for v in g['momentum']]
    frames = [(g[f'x_f{i}'], g[f'dout_f{i}'], g[f'out_f{i}'], g[f'dx_f{i}']) for i in range(int(g['n_frames']))]
    grads = {'dW': [g[f'dW{l}'] for l in range(L)], 'db': [g[f'db{l}'] for l in range(L)],
             'dgamma': [g[f'dgamma{l}'] for l in range(L - 1)], 'dbeta': [g[f'dbeta{l}'] for l in range(L - 1)]}
    return {'p': p, 'training': bool(g['training']), 'frames': frames, 'grads': grads,
            'rm_after': [g[f'rm_after{l}'] for l in range(L - 1)], 'rv_after': [g[f'rv_after{l}'] for l in range(L - 1)],
            'nbt_after': [int(v) for v in g['nbt_after']]}


def run_case(case):
    """The restatement on a recorded case, frame after frame with the buffers moving: (outs, dxs, summed parameter gradients, final
    params, per-frame tolerances summed for the parameters)."""
    p = {k: list(v) for k, v in case['p'].items()}
    outs, dxs, tols = [], [], []
    total, ttotal = None, None
    for x, dout, _, _ in case['frames']:
        out, cache, (rm, rv) = forward(x, p, case['training'])
        g = backward(cache, p, dout, case['training'])
        t = tolerances(x, p, dout, case['training'])
        outs.append(out)
        dxs.append(g['dx'])
        tols.append(t)
        add = lambda a, b: b if a is None else {k: [u + v for u, v in zip(a[k], b[k])] for k in ('dW', 'db', 'dgamma', 'dbeta')}     # noqa: E731
        total, ttotal = add(total, g), add(ttotal, t)
        p['rm'], p['rv'] = rm, rv
    return outs, dxs, total, p, tols, ttotal


def buffer_tolerances(case):
    """The bound on the buffers after all frames: a frame's own bound, plus the earlier frames' carried through (1 - m)."""
    p = {k: list(v) for k, v in case['p'].items()}
    acc = None
    for x, _, _, _ in case['frames']:
        _, _, (rm, rv) = forward(x, p, case['training'])
        t = tolerances(x, p, None, case['training'])
        m = p['momentum']
        acc = (t['rm'], t['rv']) if acc is None else ([(1 - mm) * a + b for mm, a, b in zip(m, acc[0], t['rm'])],
                                                      [(1 - mm) * a + b for mm, a, b in zip(m, acc[1], t['rv'])])
        p['rm'], p['rv'] = rm, rv
    return acc


# ---- a whole AttentionalPropagation.forward in training mode (models/mdgat.py:239-248, called per frame as 259-276 do) ----
# Composed from this module's MLP and the formulas of tests/attention_grad_ref.py (A): q | k | v = bare convolutions of every row, the
# channels permuted to the library's head * 32 + dim (A.PERM); the attention of both frames at once; merge, a bare convolution of the
# message permuted back; then PER FRAME - the reference calls the layer once per frame, so the batch statistics are a frame's own and
# the buffers move twice, frame 0 first - the two-source MLP on [desc_f | merged_f].
#
# The bound of the composed layer is NOT the two modules' entrywise derivations stacked: carried on absolute values through six
# products, a softmax and a BN in a row they grow by an order of magnitude per stage, and the result exceeds the gradients themselves.
# It is the reference's own error, measured: the generator evaluates the layer a third time in x86's 80-bit format (u = 2^-64, 2048
# times finer: the truth as far as float64 can tell) and records, per quantity, err = the larger of max|torch's float64 - truth| and
# max|this restatement's float64 - truth| - two independent float64 evaluations, in different summation orders, of the same
# conditioning.  A first-order error is (the map's sensitivity) x (local roundings), the local rounding of a dot product is bounded
# by K u sum|a_k b_k| in any order, with or without FMA, so a third correct float64 evaluation differs from these two by a constant
# factor, not by an order in u.  Tolerance per quantity: 32 err - 2 for the two implementations compared, 16 for the tail over
# summation orders (the maximum over thousands of entries of two samples is already an upper-tail estimate).  That holds a gradient
# to about 1e-13 of its largest entry.  The true gradient of four biases is ZERO (bk: a softmax does not see a shift of its row; bv, bm and
# b0: the batch statistics remove a constant), so what is compared there is the rounding noise of column sums; every bias gradient
# gets the floor err >= 4 u max|dW of the same convolution| - the same column sums weighted by inputs of order 1.
PROP_MODES = {'self': (False, 0), 'cross': (True, 8)}                     # mode -> (cross, k)
PROP_WEIGHT_FILES = ('mlp_grad_prop_weights_attn', 'mlp_grad_prop_weights_mlp')
PROP_FILES = {m: tuple(f'mlp_grad_prop_{m}_{part}' for part in ('io', 'grads_attn', 'grads_mlp')) for m in PROP_MODES}
ALL_FILES = ALL_FILES + PROP_WEIGHT_FILES + tuple(f for fs in PROP_FILES.values() for f in fs)
PROP_ATTN_GRADS = ('dWq', 'dbq', 'dWk', 'dbk', 'dWv', 'dbv', 'dWm', 'dbm')
PROP_MLP_GRADS = ('dW0', 'db0', 'dW1', 'db1', 'dgamma0', 'dbeta0')
PROP_QUANTITIES = ('out0', 'out1', 'ddesc0', 'ddesc1') + PROP_ATTN_GRADS + PROP_MLP_GRADS + ('rm0', 'rv0')
PROP_FACTOR = 32.0


def _A():
    import attention_grad_ref as A
    return A


def _attention(qkv, N, M, cross, masks, dmsg=None, kv_queries=None):
    """(message [B, N + M, 128], dqkv or None) by attention_grad_ref's formulas, in the module's current precision.  ``kv_queries``
    plants a mistake (train_ref's 'tile_tail'): a function nq -> how many of a side's leading queries contribute to dk and dv."""
    A = _A()
    qkv = _f(qkv)
    B, s = qkv.shape[0], 1 / np.sqrt(_DT[0](32))
    msg = np.zeros((B, N + M, 128), dtype=_DT[0])
    dqkv = None if dmsg is None else np.zeros_like(qkv)
    T = lambda x: np.swapaxes(x, -1, -2)                                        # noqa: E731
    un = lambda o: np.transpose(o, (0, 2, 1, 3))                                # noqa: E731
    for side, (qs, ks) in enumerate(A._sides(N, M, cross)):
        Q, K, V = A._heads(qkv[:, qs, 0]), A._heads(qkv[:, ks, 1]), A._heads(qkv[:, ks, 2])
        S = s * (Q @ T(K))
        if masks is not None:
            S = np.where(masks[side], S, -np.inf)
        e = np.exp(S - S.max(axis=-1, keepdims=True))
        P = e / e.sum(axis=-1, keepdims=True)
        O = P @ V
        msg[:, qs] = un(O).reshape(B, -1, 128)
        if dmsg is not None:
            G = A._heads(_f(dmsg)[:, qs].reshape(B, -1, 4, 32))
            dS = P * (G @ T(V) - (G * O).sum(axis=-1, keepdims=True))
            dqkv[:, qs, 0] += un(s * (dS @ K))
            c = Q.shape[2] if kv_queries is None else kv_queries(Q.shape[2])
            dqkv[:, ks, 1] += un(s * (T(dS[:, :, :c]) @ Q[:, :, :c]))
            dqkv[:, ks, 2] += un(T(P[:, :, :c]) @ G[:, :, :c])
    return msg, dqkv


def prop_forward(desc0, desc1, w, p, cross, masks):
    """(out0 [B, N, 128], out1 [B, M, 128], state for ``prop_backward``, (rm, rv) after both frames)."""
    PERM = _A().PERM
    desc = np.concatenate([_f(desc0), _f(desc1)], axis=1)
    B, N, M = desc.shape[0], np.shape(desc0)[1], np.shape(desc1)[1]
    qkv = np.stack([desc @ _f(w['W' + c])[PERM].T + _f(w['b' + c])[PERM] for c in 'qkv'], axis=2).reshape(B, N + M, 3, 4, 32)
    msg, _ = _attention(qkv, N, M, cross, masks)
    merged = msg @ _f(w['Wm'])[:, PERM].T + _f(w['bm'])
    q = {k: list(v) for k, v in p.items()}
    outs, caches = [], []
    for rows in (slice(0, N), slice(N, N + M)):
        X = np.concatenate([desc[:, rows], merged[:, rows]], axis=2).reshape(-1, 256)
        out, cache, (rm, rv) = forward(X, q)
        outs.append(out.reshape(B, -1, 128))
        caches.append(cache)
        q = dict(q, rm=rm, rv=rv)
    return outs[0], outs[1], {'desc': desc, 'qkv': qkv, 'msg': msg, 'caches': caches}, (q['rm'], q['rv'])


def prop_backward(st, w, p, cross, masks, dout0, dout1, drop_dgamma=False, no_perm_back=False):
    """Flat dict of the gradients: 'ddesc0', 'ddesc1', PROP_ATTN_GRADS (as the reference holds them: channel = dim * 4 + head) and
    PROP_MLP_GRADS summed over the two frames.  ``drop_dgamma`` / ``no_perm_back`` (the message's gradient handed to the attention
    without the channel permutation) plant mistakes."""
    PERM = _A().PERM
    desc, qkv, msg = st['desc'], st['qkv'], st['msg']
    B, P = desc.shape[0], desc.shape[1]
    N = np.shape(dout0)[1]
    M = P - N
    ddesc, dmerged, mlp = np.zeros_like(desc), np.zeros_like(desc), None
    for rows, cache, dout in zip((slice(0, N), slice(N, P)), st['caches'], (dout0, dout1)):
        g = backward(cache, p, _f(dout).reshape(-1, 128), drop_dgamma=drop_dgamma)
        dX = g['dx'].reshape(B, -1, 256)
        ddesc[:, rows], dmerged[:, rows] = dX[..., :128], dX[..., 128:]
        part = {'dW0': g['dW'][0], 'db0': g['db'][0], 'dW1': g['dW'][1], 'db1': g['db'][1], 'dgamma0': g['dgamma'][0], 'dbeta0': g['dbeta'][0]}
        mlp = part if mlp is None else {k: mlp[k] + part[k] for k in part}
    out = dict(mlp, dWm=np.zeros((128, 128), dtype=_DT[0]), dbm=dmerged.sum(axis=(0, 1)))
    out['dWm'][:, PERM] = dmerged.reshape(-1, 128).T @ msg.reshape(-1, 128)
    Wm = _f(w['Wm'])
    _, dqkv = _attention(qkv, N, M, cross, masks, dmerged @ (Wm if no_perm_back else Wm[:, PERM]))
    dqkv = dqkv.reshape(B, P, 3, 128)
    for i, c in enumerate('qkv'):
        d = dqkv[:, :, i]
        dW, db = np.zeros((128, 128), dtype=_DT[0]), np.zeros(128, dtype=_DT[0])
        dW[PERM], db[PERM] = d.reshape(-1, 128).T @ desc.reshape(-1, 128), d.sum(axis=(0, 1))
        out['dW' + c], out['db' + c] = dW, db
        ddesc = ddesc + d @ _f(w['W' + c])[PERM]
    out['ddesc0'], out['ddesc1'] = ddesc[:, :N], ddesc[:, N:]
    return out


def prop_run(c, **planted):
    """Every quantity of PROP_QUANTITIES the restatement gives for a recorded (or to be recorded) case ``c`` ('desc0', 'desc1', 'w',
    'p', 'cross', 'masks', 'dout0', 'dout1'), plus 'z': the BN inputs of both frames, for the ReLU condition."""
    out0, out1, st, (rm, rv) = prop_forward(c['desc0'], c['desc1'], c['w'], c['p'], c['cross'], c['masks'])
    q = prop_backward(st, c['w'], c['p'], c['cross'], c['masks'], c['dout0'], c['dout1'], **planted)
    q.update(out0=out0, out1=out1, rm0=rm[0], rv0=rv[0], z=np.concatenate([cache[0]['z'] for cache in st['caches']]))
    return q


def prop_reference_error(c, recorded):
    """{quantity: err} as the section's comment defines it; ``recorded``: the reference's own float64 results by quantity.  'z': this
    restatement's alone (the reference does not expose it)."""
    if np.finfo(np.longdouble).eps > 2.0 ** -60:
        raise RuntimeError('the measured bound needs an extended-precision long double (x86)')
    with precision(np.longdouble):
        truth = prop_run(c)
    mine = prop_run(c)
    dev = lambda a, b: float(np.abs(np.asarray(a, dtype=np.longdouble) - b).max())          # noqa: E731
    err = {k: max(dev(recorded[k], truth[k]), dev(mine[k], truth[k])) for k in PROP_QUANTITIES}
    for k in PROP_QUANTITIES:           # the bias gradients' floor
        if k in ('dbq', 'dbk', 'dbv', 'dbm', 'db0', 'db1'):
            err[k] = max(err[k], 4.0 * U * float(np.abs(mine['dW' + k[2:]]).max()))
    err['z'] = dev(mine['z'], truth['z'])
    return err


def prop_compare(got, want, err, names=PROP_QUANTITIES):
    """Worst over the quantities of max|got - want| / (32 err); returns (worst, the quantity it was met at)."""
    worst = (0.0, '')
    for k in names:
        a, b = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        worst = max(worst, (float(np.abs(a - b).max()) / (PROP_FACTOR * err[k]), k))
    return worst


def prop_relu_margin(c, err):
    """min |z| over both frames' BN inputs / (32 err_z)."""
    return float(np.abs(prop_run(c)['z']).min()) / (PROP_FACTOR * err['z'])


def load_prop(golden_dir, mode):
    """One recorded layer call pair (tools/make_goldens_mlp_grad.py): the inputs of ``prop_run`` ('w': the attention's weights as the
    reference holds them, 'p': the MLP's parameters with the buffers BEFORE the calls, 'masks': None for full attention), 'k',
    'want': the reference's results by quantity, 'err': the measured reference error by quantity (and 'z'), 'nbt_after'."""
    g = load_files(golden_dir, PROP_WEIGHT_FILES + PROP_FILES[mode])
    cross, k = PROP_MODES[mode]
    B, N, M = g['desc0'].shape[0], g['desc0'].shape[1], g['desc1'].shape[1]
    p = {'W': [g['W0'], g['W1']], 'b': [g['b0'], g['b1']], 'gamma': [g['gamma0']], 'beta': [g['beta0']], 'rm': [g['rm0']], 'rv': [g['rv0']],
         'eps': [float(g['eps'][0])], 'momentum': [float(g['momentum'][0])]}
    masks = None
    if k > 0:
        nk = (M, N) if cross else (N, M)
        masks = tuple(np.unpackbits(g[f'mask{i}_bits'])[:B * 4 * n * nk[i]].reshape(B, 4, n, nk[i]).astype(bool) for i, n in enumerate((N, M)))
    want = {q: g[q] for q in PROP_QUANTITIES if q not in ('rm0', 'rv0')}
    want.update(rm0=g['rm_after0'], rv0=g['rv_after0'])
    return {'w': {k2: g[k2] for k2 in ('Wq', 'bq', 'Wk', 'bk', 'Wv', 'bv', 'Wm', 'bm')}, 'p': p, 'cross': cross, 'k': k, 'masks': masks,
            'desc0': g['desc0'], 'desc1': g['desc1'], 'dout0': g['dout0'], 'dout1': g['dout1'], 'want': want,
            'err': {q: float(g['err_' + q]) for q in PROP_QUANTITIES + ('z',)}, 'nbt_after': [int(v) for v in g['nbt_after']]}
