"""The numpy restatement of the training-mode MLP (tests/mlp_grad_ref.py) against the reference's own recorded results
(tests/golden/mlp_grad_*.npz, tools/make_goldens_mlp_grad.py) and torch autograd, the sharpness of its derived bound, and the ReLU
condition of every input the GPU tests (tests/test_gpu_mlp_grad.py) feed the kernels.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_grad_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MARGIN = 1e3


@pytest.mark.parametrize('name', sorted(R.GOLDEN_FILES))
def test_restatement_reproduces_fixture(name):
    case = R.load_case(GOLDEN, name)
    outs, dxs, grads, p, tols, ttotal = R.run_case(case)
    worst = 0.0
    for (x, dout, out, dx), o, d, t in zip(case['frames'], outs, dxs, tols):
        worst = max(worst, R.worst_fraction(o, out, t['out']), R.worst_fraction(d, dx, t['dx']))
    worst = max(worst, R.compare_grads(grads, case['grads'], ttotal))
    trm, trv = R.buffer_tolerances(case)
    for l in range(R.n_bn(p)):
        if case['training']:
            worst = max(worst, R.worst_fraction(p['rm'][l], case['rm_after'][l], trm[l]), R.worst_fraction(p['rv'][l], case['rv_after'][l], trv[l]))
        else:
            assert np.array_equal(p['rm'][l], case['rm_after'][l]) and np.array_equal(case['p']['rv'][l], case['rv_after'][l])
    assert case['nbt_after'] == [len(case['frames']) if case['training'] else 0] * R.n_bn(p)
    print(f'{name}: worst fraction of the bound {worst:.3f}')
    assert worst <= 1.0


def torch_grads(seq, x, dout):
    """(out, grads, (rm, rv)) by autograd; x [R, K] rows."""
    xt = torch.from_numpy(x).requires_grad_()
    out = seq(xt.t()[None])[0].t()
    (out * torch.from_numpy(dout)).sum().backward()
    convs = [m for m in seq if isinstance(m, torch.nn.Conv1d)]
    bns = [m for m in seq if isinstance(m, torch.nn.BatchNorm1d)]
    g = {'dx': xt.grad.numpy(), 'dW': [c.weight.grad.numpy()[:, :, 0] for c in convs], 'db': [c.bias.grad.numpy() for c in convs],
         'dgamma': [b.weight.grad.numpy() for b in bns], 'dbeta': [b.bias.grad.numpy() for b in bns]}
    return out.detach().numpy(), g, ([b.running_mean.numpy() for b in bns], [b.running_var.numpy() for b in bns])


@pytest.mark.parametrize('stack,rows,training', [('kenc', 17, True), ('denc', 65, True), ('layer', 40, True), ('denc', 33, False), ('conv384', 9, True)])
def test_restatement_agrees_with_autograd(stack, rows, training):
    x, p, dout = R.gpu_case(stack, rows, seed=9100 + rows)
    out, cache, (rm, rv) = R.forward(x, p, training)
    g = R.backward(cache, p, dout, training)
    t = R.tolerances(x, p, dout, training)
    want_out, want, (trm, trv) = torch_grads(R.torch_stack(p, training), x, dout)
    worst = max(R.worst_fraction(out, want_out, t['out']), R.compare_grads(g, want, t))
    for l in range(R.n_bn(p)):
        if training:
            worst = max(worst, R.worst_fraction(rm[l], trm[l], t['rm'][l]), R.worst_fraction(rv[l], trv[l], t['rv'][l]))
    print(f'{stack} R={rows} training={training}: worst fraction {worst:.3f}')
    assert worst <= 1.0


def _worst(x, p, dout, fwd_kw=None, bwd_kw=None, p_planted=None):
    """Worst fraction of the bound between the restatement and itself with a mistake planted."""
    out, cache, (rm, rv) = R.forward(x, p)
    g = R.backward(cache, p, dout)
    t = R.tolerances(x, p, dout)
    q = p if p_planted is None else p_planted
    out2, cache2, (rm2, rv2) = R.forward(x, q, **(fwd_kw or {}))
    g2 = R.backward(cache2, q, dout, **(bwd_kw or {}))
    worst = max(R.worst_fraction(out2, out, t['out']), R.compare_grads(g2, g, t))
    for l in range(R.n_bn(p)):
        worst = max(worst, R.worst_fraction(rm2[l], rm[l], t['rm'][l]), R.worst_fraction(rv2[l], rv[l], t['rv'][l]))
    return worst


def test_bound_is_sharp():
    x, p, dout = R.gpu_case('denc', 65)
    assert _worst(x, p, dout) == 0.0
    q = {k: [np.array(v) for v in vs] for k, vs in p.items()}
    q['W'][1][7, 11] *= 1.0 + 1e-6
    assert _worst(x, p, dout, p_planted=q) > 1.0, 'a relative error of 1e-6 in one weight'
    assert _worst(x, p, dout, fwd_kw={'normalise_unbiased': True}) > 1.0, 'unbiased variance in the normalisation'
    assert _worst(x, p, dout, fwd_kw={'running_biased': True}) > 1.0, 'biased variance in running_var'
    assert _worst(x, p, dout, bwd_kw={'drop_dgamma': True}) > 1.0, 'a dropped dgamma term in dY'


def test_bound_catches_mask_on_exact_zero():
    # the one case that plants exact zeros on purpose: a constant channel (zero weight row) with beta = 0 has z == 0 in every row
    x, p, dout = R.dead_constant_case(R=64)
    p['b'][0][5], p['beta'][0][5] = 0.5, 0.0
    _, cache, _ = R.forward(x, p)
    assert (cache[0]['z'][:, 5] == 0.0).all()
    assert _worst(x, p, dout) == 0.0
    assert _worst(x, p, dout, bwd_kw={'mask_ge': True}) > 1.0, 'z >= 0 as the ReLU mask'


def test_bound_catches_one_pass_variance():
    x, p, dout = R.offset_case()
    _, cache, _ = R.forward(x, p)
    assert np.abs(cache[0]['mean']).min() > 9e3 and 0.3 < np.sqrt(cache[0]['var']).mean() < 3.0
    assert _worst(x, p, dout) == 0.0
    assert _worst(x, p, dout, fwd_kw={'variance': 'one_pass'}) > 1.0, 'E[y^2] - E[y]^2 at mean 1e4, spread 1'


def test_relu_condition_of_fixtures():
    for name in sorted(R.GOLDEN_FILES):
        case = R.load_case(GOLDEN, name)
        p = {k: list(v) for k, v in case['p'].items()}
        for x, _, _, _ in case['frames']:
            margin = R.relu_margin(x, p, case['training'])
            print(f'{name}: smallest |z| / bound {margin:.3e}')
            assert margin >= MARGIN
            _, _, (p['rm'], p['rv']) = R.forward(x, p, case['training'])


@pytest.mark.parametrize('stack', [s for s in R.GPU_STACKS if len(R.STACKS[s]) > 2])
def test_relu_condition_of_gpu_inputs(stack):
    for rows in R.GPU_ROWS:
        for training in (True, False):
            x, p, _ = R.gpu_case(stack, rows)
            margin = R.relu_margin(x, p, training)
            print(f'{stack} R={rows} training={training}: smallest |z| / bound {margin:.3e}')
            assert margin >= MARGIN
    x, p, _ = R.offset_case()
    assert R.relu_margin(x, p) >= MARGIN
    # the dead / constant case: the dead channel sits at z = -1, the constant one at z = beta = 0.25
    x, p, _ = R.dead_constant_case()
    assert R.relu_margin(x, p) >= MARGIN


@pytest.mark.parametrize('mode', sorted(R.PROP_MODES))
def test_restated_layer_reproduces_fixture(mode):
    """The whole AttentionalPropagation.forward in training mode, both frames (self full / cross k = 8): the MLP restatement composed with
    the attention's formulas reproduces the reference's outputs, every gradient and the buffers within 32 x the reference's own
    measured error, and the ReLU of the fixture is decided."""
    c = R.load_prop(GOLDEN, mode)
    got = R.prop_run(c)
    worst, where = R.prop_compare(got, c['want'], c['err'])
    margin = R.prop_relu_margin(c, c['err'])
    print(f'layer {mode}: worst fraction of the bound {worst:.3f} at {where}, smallest |z| / bound {margin:.3e}')
    assert worst <= 1.0 and c['nbt_after'] == [2]
    assert margin >= MARGIN
    if np.finfo(np.longdouble).eps < 2.0 ** -60:          # where the 80-bit format exists, the recorded errors are what it gives today
        err = R.prop_reference_error(c, c['want'])
        assert all(abs(err[k] - c['err'][k]) <= 0.5 * c['err'][k] for k in c['err']), (err, c['err'])


@pytest.mark.parametrize('mode', sorted(R.PROP_MODES))
def test_composed_bound_is_sharp(mode):
    c = R.load_prop(GOLDEN, mode)
    good = R.prop_run(c)
    assert R.prop_compare(good, good, c['err'])[0] == 0.0
    for k in ('dWq', 'dWk', 'ddesc0', 'ddesc1'):          # a zeroed gradient
        bad = dict(good, **{k: np.zeros_like(good[k])})
        assert R.prop_compare(bad, c['want'], c['err'], names=(k,))[0] > 1.0, f'a zeroed {k}'
    bad = dict(good, ddesc0=-good['ddesc0'])
    assert R.prop_compare(bad, c['want'], c['err'], names=('ddesc0',))[0] > 1.0, 'a sign-flipped ddesc0'
    for name in ('Wq', 'Wk', 'Wv', 'Wm'):                   # a relative error of 1e-6 in one projection weight
        w = dict(c['w'], **{name: c['w'][name].copy()})
        w[name][5, 9] *= 1.0 + 1e-6
        bad = R.prop_run(dict(c, w=w))
        assert R.prop_compare(bad, c['want'], c['err'], names=('out0', 'out1', 'ddesc0', 'ddesc1'))[0] > 1.0, f'1e-6 in one entry of {name}'
    bad = R.prop_run(c, no_perm_back=True)
    assert R.prop_compare(bad, c['want'], c['err'], names=('dWq', 'dWk', 'dWv', 'ddesc0', 'ddesc1'))[0] > 1.0, 'no channel permutation on the way back'
    bad = R.prop_run(c, drop_dgamma=True)
    assert R.prop_compare(bad, c['want'], c['err'], names=('dW0', 'dWm', 'dWq', 'ddesc0'))[0] > 1.0, 'a dropped dgamma term'
