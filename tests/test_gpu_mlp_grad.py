"""The training-mode MLP on the device: ops.mlp_f64 (Conv1d(k=1), BatchNorm1d on the batch's own statistics, ReLU; csrc/mlp_grad.hip) and
its backward through autograd and through ops.mlp_f64_backward.  Expected values: the reference's own recorded results
(tests/golden/mlp_grad_*.npz, tools/make_goldens_mlp_grad.py) and the numpy restatement tests/mlp_grad_ref.py (pinned to the reference
and to torch autograd by tests/test_mlp_grad_ref.py).

Tolerance (mlp_grad_ref.tolerances), derived there: K u sum|a_k b_k| per product, carried through the layers on absolute values, with
the terms BN brings (the relative error of invstd grows with 1 + |mean| / std and multiplies yhat, dgamma and dY), times 4.  Every
input here has its ReLU decided by a factor 1e3 (tests/test_mlp_grad_ref.py asserts it on the CPU).  Every comparison prints the worst
|difference| / tolerance it met.  The two-source and behind-a-BatchNorm cases assert by the launch counters (tests/gemm_f64_forms.py)
which instantiation of gemm_f64_kernel each of their products ran."""
import numpy as np
import pytest
import torch

import gemm_f64_forms as F
import mlp_grad_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _ops():
    from mdgat_matcher_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _seq(p, training, bare=False):
    seq = R.torch_stack(p, training).to(DEV)
    return seq[0].train(training) if bare else seq


def _parts(seq):
    mods = [seq] if isinstance(seq, torch.nn.Conv1d) else list(seq)
    return [m for m in mods if isinstance(m, torch.nn.Conv1d)], [m for m in mods if isinstance(m, torch.nn.BatchNorm1d)]


def _grads(seq, xs):
    """The gradients that landed on the modules' own parameters and on the inputs, as numpy (None where there is none)."""
    convs, bns = _parts(seq)
    n = lambda t: None if t is None else t.detach().cpu().numpy()          # noqa: E731
    g = {'dW': [n(c.weight.grad) for c in convs], 'db': [n(c.bias.grad) for c in convs],
         'dgamma': [n(b.weight.grad) for b in bns], 'dbeta': [n(b.bias.grad) for b in bns]}
    if xs[0].grad is not None:
        g['dx'] = np.concatenate([n(x.grad) for x in xs if x is not None], axis=-1)
    return g


def _run(seq, x, dout, split=0, x_grad=True, launches=None):
    """ops.mlp_f64 and .backward() on rows x (split > 0: the two sources x[:, :split] | x[:, split:]): (out, grads, seq).
    launches (a dict): filled with the fp64 GEMM launches by instantiation of the 'forward' and of the 'backward' (gemm_f64_forms)."""
    ops = _ops()
    xs = [_dev(x)] if split == 0 else [_dev(x[:, :split]), _dev(x[:, split:])]
    for t in xs:
        t.requires_grad_(x_grad)
    g = _dev(dout)
    with F.watch() as fwd:
        out = ops.mlp_f64(seq, *xs)
    with F.watch() as bwd:
        out.backward(g)
    if launches is not None:
        launches.update(forward=fwd.delta, backward=bwd.delta)
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), _grads(seq, xs), seq


def _buffers(seq):
    _, bns = _parts(seq)
    return ([b.running_mean.cpu().numpy() for b in bns], [b.running_var.cpu().numpy() for b in bns], [int(b.num_batches_tracked) for b in bns])


@pytest.mark.parametrize('name', sorted(R.GOLDEN_FILES))
def test_kernel_reproduces_fixture(golden_dir, name):
    case = R.load_case(golden_dir, name)
    ops = _ops()
    seq = _seq(case['p'], case['training'])
    _, _, _, _, tols, ttotal = R.run_case(case)
    worst, loss, xs = 0.0, 0.0, []
    for (x, dout, out, dx), t in zip(case['frames'], tols):
        src = [_dev(x).requires_grad_()] if name != 'layer' else [_dev(x[:, :128]).requires_grad_(), _dev(x[:, 128:]).requires_grad_()]
        got = ops.mlp_f64(seq, *src)
        loss = loss + (got * _dev(dout)).sum()
        xs.append(src)
        worst = max(worst, R.worst_fraction(got.detach().cpu().numpy(), out, t['out']))
    loss.backward()
    torch.cuda.synchronize()
    for (x, dout, out, dx), src, t in zip(case['frames'], xs, tols):
        worst = max(worst, R.worst_fraction(np.concatenate([s.grad.cpu().numpy() for s in src], axis=1), dx, t['dx']))
    worst = max(worst, R.compare_grads(_grads(seq, [torch.zeros(1)]), case['grads'], ttotal))
    rm, rv, nbt = _buffers(seq)
    trm, trv = R.buffer_tolerances(case)
    for l in range(len(rm)):
        if case['training']:
            worst = max(worst, R.worst_fraction(rm[l], case['rm_after'][l], trm[l]), R.worst_fraction(rv[l], case['rv_after'][l], trv[l]))
        else:
            assert np.array_equal(rm[l], case['rm_after'][l]) and np.array_equal(rv[l], case['rv_after'][l])
    assert nbt == case['nbt_after']
    print(f'{name}: worst fraction of the bound {worst:.3f}')
    assert worst <= 1.0


def _against_restatement(stack, rows, training=True, case=None, split=None, launches=None):
    x, p, dout = case if case is not None else R.gpu_case(stack, rows)
    bare = len(p['W']) == 1
    out, cache, (rm, rv) = R.forward(x, p, training)
    want = R.backward(cache, p, dout, training)
    t = R.tolerances(x, p, dout, training)
    seq = _seq(p, training, bare)
    before = _buffers(seq) if not bare else None
    got_out, got, _ = _run(seq, x, dout, split=(128 if stack == 'layer' else 0) if split is None else split, launches=launches)
    worst = max(R.worst_fraction(got_out, out, t['out']), R.compare_grads(got, want, t))
    assert set(got) == set(want) and all(v is not None for k in ('dW', 'db', 'dgamma', 'dbeta') for v in got[k])
    if not bare:
        grm, grv, nbt = _buffers(seq)
        for l in range(len(grm)):
            if training:
                worst = max(worst, R.worst_fraction(grm[l], rm[l], t['rm'][l]), R.worst_fraction(grv[l], rv[l], t['rv'][l]))
                assert nbt[l] == 1
            else:       # bit-unchanged
                assert np.array_equal(grm[l], before[0][l]) and np.array_equal(grv[l], before[1][l]) and nbt[l] == 0
    return worst, got, seq


@pytest.mark.parametrize('stack', R.GPU_STACKS)
def test_kernel_agrees_with_restatement(stack):
    # R: 2 (the smallest), 17 (odd), 64 / 65 (a whole row tile / a ragged one), 1000 (ragged slabs), 1024 = 2 x 512 (two dW slabs)
    for rows in R.GPU_ROWS:
        worst, _, _ = _against_restatement(stack, rows)
        print(f'{stack} R={rows}: worst fraction of the bound {worst:.3f}')
        assert worst <= 1.0


# ---- the instantiations of gemm_f64_kernel (csrc/f64.hip) that only these products reach: two sources, and the operand behind a BN ----
def _gemm_case(channels, rows, seed):
    """(x, params, dout) of a stack ``channels`` at ``rows`` rows, its ReLU condition asserted on the CPU."""
    rs = np.random.RandomState(seed)
    x, p, dout = rs.standard_normal((rows, channels[0])), R.random_params(channels, seed + 1), rs.standard_normal((rows, channels[-1]))
    margin = R.relu_margin(x, p)
    assert margin >= 1e3, f'a BN output lies within {margin:.3g} bounds of zero: pick another seed'
    return x, p, dout


def _planned(cus, *products):
    """Launches by instantiation of the products (M, N, K, K0, bnt) as the plan names them on this device (operands out of torch's
    allocator and the library's workspace carve: 16-byte aligned, natural leading dimensions)."""
    want = np.zeros(10, dtype=np.int64)
    for M, N, K, K0, bnt in products:
        want[F.plan(M, N, K, K0, bnt=bnt, cus=cus)] += 1
    return want


@pytest.mark.parametrize('K0,K1,rows', sorted(F.TWO_SOURCE))
def test_two_source_convolution_reaches_its_form(K0, K1, rows):
    """A bare 64-output convolution of the sources K0 | K1: whole chunks of one source each (32 | 32), chunks of 64 (64 | 64), and the
    general form with a chunk that straddles K0 (40 | 24: the second chunk; 8 | 56: the first), on whole and ragged row tiles.  The same
    run checks dx0 and dx1, the two products on the halves of the transposed weight with ldc = K0 and ldc = K1."""
    cus, form = F.cu_count(), F.TWO_SOURCE[(K0, K1, rows)]
    launches = {}
    worst, _, _ = _against_restatement('two_source', rows, case=_gemm_case((K0 + K1, 64), rows, 7900 + 64 * K0 + rows), split=K0, launches=launches)
    print(f'{K0} | {K1} R={rows}: worst fraction of the bound {worst:.3f}, forward {F.NAMES[int(launches["forward"].argmax())]} on {cus} CUs')
    want = np.zeros(10, dtype=np.int64)
    want[F.index(form)] = 1
    assert np.array_equal(launches['forward'], want), f'wanted {form}, launched {dict(zip(F.NAMES, launches["forward"]))} on a device of {cus} CUs'
    assert np.array_equal(launches['backward'], _planned(cus, (rows, K0, 64, 64, False), (rows, K1, 64, 64, False))), (launches['backward'], cus)
    assert worst <= 1.0


@pytest.mark.parametrize('name', sorted(F.BNT))
def test_product_behind_a_batchnorm_reaches_its_form(name):
    """The second convolution of a two-convolution stack reads max(BN(Y), 0) formed as the operand is loaded: the five BNT
    instantiations, the two wide ones at the row counts at which the launcher takes 64 x 128 tiles on this device."""
    ch, cands, form = F.BNT[name]
    cus, want = F.cu_count(), F.index(form, True)
    rows = F.pick(cands, want, cus, lambda r: dict(M=r, N=ch[2], K=ch[1], bnt=True))
    launches = {}
    worst, _, _ = _against_restatement(name, rows, case=_gemm_case(ch, rows, 8100 + rows), launches=launches)
    print(f'{ch} R={rows}: worst fraction of the bound {worst:.3f}, forward {dict((F.NAMES[i], int(n)) for i, n in enumerate(launches["forward"]) if n)} on {cus} CUs')
    assert np.array_equal(launches['forward'], _planned(cus, (rows, ch[1], ch[0], ch[0], False), (rows, ch[2], ch[1], ch[1], True))), \
        f'wanted {F.NAMES[want]}, launched {dict(zip(F.NAMES, launches["forward"]))} on a device of {cus} CUs'
    assert launches['forward'][want] == 1 and launches['forward'][5:].sum() == 1
    assert np.array_equal(launches['backward'], _planned(cus, (rows, ch[1], ch[2], ch[2], False), (rows, ch[0], ch[1], ch[1], False))), (launches['backward'], cus)
    assert worst <= 1.0


@pytest.mark.parametrize('stack', ['kenc', 'denc', 'layer', 'ragged'])
def test_eval_mode(stack):
    for rows in (17, 1000):
        worst, _, _ = _against_restatement(stack, rows, training=False)
        print(f'{stack} eval R={rows}: worst fraction of the bound {worst:.3f}')
        assert worst <= 1.0


def test_dead_and_constant_channels():
    case = R.dead_constant_case()
    worst, got, _ = _against_restatement('edge', 40, case=case)
    print(f'dead / constant: worst fraction of the bound {worst:.3f}')
    assert worst <= 1.0
    # the dead channel: exact zeros, not small numbers
    assert got['dgamma'][0][3] == 0.0 and got['dbeta'][0][3] == 0.0 and not got['dW'][0][3].any()
    assert all(np.isfinite(v).all() for k in ('dW', 'db', 'dgamma', 'dbeta') for v in got[k]) and np.isfinite(got['dx']).all()


def test_offset_channels_hold_the_bound():
    worst, _, _ = _against_restatement('offset', 64, case=R.offset_case())
    print(f'mean 1e4, spread 1: worst fraction of the bound {worst:.3f}')
    assert worst <= 1.0


def test_empty_and_single_row():
    ops = _ops()
    x, p, dout = R.gpu_case('denc', 2)
    seq = _seq(p, True)
    before = _buffers(seq)
    e = _dev(x[:0]).requires_grad_()
    out = ops.mlp_f64(seq, e)
    assert out.shape == (0, 128)
    out.backward(_dev(dout[:0]))
    torch.cuda.synchronize()
    after = _buffers(seq)
    assert all(np.array_equal(a, b) for a, b in zip(before[0] + before[1], after[0] + after[1])) and after[2] == before[2]
    assert e.grad.shape == (0, 33) and not seq[0].weight.grad.any()
    with pytest.raises(ValueError):
        ops.mlp_f64(seq, _dev(x[:1]))
    assert ops.mlp_f64(seq.eval(), _dev(x[:1])).shape == (1, 128)          # eval mode takes one row, as torch does
    assert ops.mlp_f64(seq[0], _dev(x[:1])).shape == (1, 64)               # ... and so does a bare convolution
    lead = ops.mlp_f64(seq, _dev(np.stack([x, x])))                        # leading dimensions are kept
    assert lead.shape == (2, 2, 128)


def test_optional_outputs_and_determinism():
    ops = _ops()
    x, p, dout = R.gpu_case('layer', 1000)
    first = _run(_seq(p, True), x, dout, split=128)
    second = _run(_seq(p, True), x, dout, split=128)
    assert np.array_equal(first[0], second[0])
    for k in ('dW', 'db', 'dgamma', 'dbeta'):
        assert all(np.array_equal(a, b) for a, b in zip(first[1][k], second[1][k])), k
    assert np.array_equal(first[1]['dx'], second[1]['dx'])
    assert all(np.array_equal(a, b) for a, b in zip(sum(_buffers(first[2])[:2], []), sum(_buffers(second[2])[:2], [])))
    # without x.requires_grad dx is not formed, the rest is the same bits
    quiet = _run(_seq(p, True), x, dout, split=128, x_grad=False)
    assert 'dx' not in quiet[1]
    for k in ('dW', 'db', 'dgamma', 'dbeta'):
        assert all(np.array_equal(a, b) for a, b in zip(first[1][k], quiet[1][k])), k
    # the raw pair, with a subset asked for
    seq = _seq(p, True)
    x0, x1, g = _dev(x[:, :128]), _dev(x[:, 128:]), _dev(dout)
    out, saved = ops.mlp_f64_forward(seq, x0, x1)
    assert np.array_equal(out.cpu().numpy(), first[0])
    dx, dx1, dW, db, dga, dbe = ops.mlp_f64_backward(seq, x0, x1, saved, g, need=(False, True, [False, True], [False, False], [True], [False]))
    assert dx is None and dW[0] is None and db == [None, None] and dbe == [None]
    assert np.array_equal(dx1.cpu().numpy(), first[1]['dx'][:, 128:]) and np.array_equal(dW[1].cpu().numpy(), first[1]['dW'][1])
    assert np.array_equal(dga[0].cpu().numpy(), first[1]['dgamma'][0])
    # a bias gradient alone: the column sums without the weight product, the same bits
    only = ops.mlp_f64_backward(seq, x0, x1, saved, g, need=(False, False, [False, False], [True, True], [False], [False]))
    assert only[2] == [None, None] and all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(only[3], first[1]['db']))
    # nothing recorded without grad
    with torch.no_grad():
        assert ops.mlp_f64(seq, x0, x1).grad_fn is None
    frozen = _seq(p, True).requires_grad_(False)
    assert ops.mlp_f64(frozen, x0, x1).grad_fn is None


def test_refusals():
    ops = _ops()
    x, p, _ = R.gpu_case('denc', 17)
    seq, xd = _seq(p, True), _dev(x)
    with pytest.raises(ValueError):
        ops.mlp_f64(seq, xd.float())
    with pytest.raises(ValueError):
        ops.mlp_f64(seq, xd[:, :32])
    with pytest.raises(ValueError):
        ops.mlp_f64(torch.nn.Sequential(*list(seq)[:3]), xd)                 # ends in BN + ReLU
    bad = _seq(p, True)
    bad[1].momentum = None
    with pytest.raises(ValueError):
        ops.mlp_f64(bad, xd)
    for kw in ({'affine': False}, {'track_running_stats': False}):
        bad = _seq(p, True)
        bad[1] = torch.nn.BatchNorm1d(64, **kw).double().to(DEV)
        with pytest.raises(ValueError):
            ops.mlp_f64(bad, xd)
    with pytest.raises(ValueError):
        ops.mlp_f64(torch.nn.Conv1d(33, 40, 1).double().to(DEV), xd)        # 40 outputs: not a multiple of 16
    with pytest.raises(ValueError):
        ops.mlp_f64(torch.nn.Conv1d(33, 64, 3).double().to(DEV), xd)
    with pytest.raises(RuntimeError):
        ops.mlp_f64(_seq(p, True).cpu(), torch.from_numpy(x))


def _conv(W, b):
    c = torch.nn.Conv1d(W.shape[1], W.shape[0], 1).double()
    with torch.no_grad():
        c.weight.copy_(torch.from_numpy(W)[:, :, None])
        c.bias.copy_(torch.from_numpy(b))
    return c.to(DEV).train()


@pytest.mark.parametrize('mode', sorted(R.PROP_MODES))
def test_composed_training_layer(golden_dir, mode):
    """A training-mode AttentionalPropagation built from ops.mlp_f64 (the projections, merge, the two-source layer MLP) and
    ops.attention_f64, with the channel permutation tests/attention_grad_ref.py pins, reproduces the recorded reference layer - the
    outputs of both frames, the gradients of x, source and every parameter, the buffers - within 32 x the reference's own measured error per quantity (mlp_grad_ref: the
    section on the whole layer; about 1e-13 of a quantity's largest entry)."""
    import attention_grad_ref as A
    ops = _ops()
    c = R.load_prop(golden_dir, mode)
    w, cross, k = c['w'], c['cross'], c['k']
    N, M = c['desc0'].shape[1], c['desc1'].shape[1]
    conv = {ch: _conv(w['W' + ch], w['b' + ch]) for ch in 'qkvm'}
    mlp = _seq(c['p'], True)
    perm = torch.from_numpy(A.PERM).to(DEV)
    d0, d1 = _dev(c['desc0']).requires_grad_(), _dev(c['desc1']).requires_grad_()
    desc = torch.cat([d0, d1], dim=1)
    qkv = torch.stack([ops.mlp_f64(conv[ch], desc)[..., perm] for ch in 'qkv'], dim=2).reshape(desc.shape[0], N + M, 3, 4, 32)
    if k > 0:
        msg, masks = ops.attention_f64(qkv, N, M, cross, topk=k, return_selection=True)
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(masks, c['masks']))
    else:
        msg = ops.attention_f64(qkv, N, M, cross)
    merged = ops.mlp_f64(conv['m'], msg[..., torch.argsort(perm)])
    out0 = ops.mlp_f64(mlp, d0, merged[:, :N].contiguous())                 # frame 0 first: the buffers move in the reference's order
    out1 = ops.mlp_f64(mlp, d1, merged[:, N:].contiguous())
    ((out0 * _dev(c['dout0'])).sum() + (out1 * _dev(c['dout1'])).sum()).backward()
    torch.cuda.synchronize()
    n = lambda v: v.detach().cpu().numpy()                                   # noqa: E731
    g = _grads(mlp, [torch.zeros(1)])
    rm, rv, nbt = _buffers(mlp)
    got = {'out0': n(out0), 'out1': n(out1), 'ddesc0': n(d0.grad), 'ddesc1': n(d1.grad), 'rm0': rm[0], 'rv0': rv[0],
           'dW0': g['dW'][0][:, :, 0], 'db0': g['db'][0], 'dW1': g['dW'][1][:, :, 0], 'db1': g['db'][1], 'dgamma0': g['dgamma'][0], 'dbeta0': g['dbeta'][0]}
    for ch in 'qkvm':
        got['dW' + ch], got['db' + ch] = n(conv[ch].weight.grad)[:, :, 0], n(conv[ch].bias.grad)
    for q in R.PROP_QUANTITIES:
        print(f'composed layer {mode}: {q}: fraction of the bound {R.prop_compare(got, c["want"], c["err"], names=(q,))[0]:.4f}')
    worst, where = R.prop_compare(got, c['want'], c['err'])
    print(f'composed layer {mode}: worst fraction of the bound {worst:.4f} at {where}')
    assert worst <= 1.0 and nbt == c['nbt_after']
