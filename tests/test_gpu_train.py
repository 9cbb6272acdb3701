"""``MDGAT.training_forward`` on the device - the whole differentiable fp64 step composed from the library's primitives
(mdgat_matcher_amd/train.py) - against the reference's recorded steps (tests/golden/train_*.npz, tools/make_goldens_train.py).

Tolerance: per quantity 32 x the reference's own measured error ``err`` stored in the fixtures (tests/train_ref.py): the loss,
every recorded gradient, every BatchNorm buffer.  Matches are compared exactly (the generator refuses a case whose arg-max is decided by
less than 1e-5).  The matching scores come from ``ops.extract``, which reads Z rounded to float32 and takes exp in float32: they are held
to its own bound, extract_ref.SCORE_TOL = 1e-6 (values <= 1), not to an fp64 one.  Every comparison prints the worst fraction of the
bound it met.

The shape cases (train_ref.SHAPE_CASES) take the step past one tile of every kernel it composes, to B = 1, dynamic self and full cross
layers and two pairs of layers, under the same rule.  Their fixtures hold the reference's value of everything but the layers'
convolution weights; for those the expected value is the float64 restatement run here on the host, which the generator held to the
reference.  A dynamic layer's selection is asserted equal to the restatement's before any gradient is compared."""
import functools

import numpy as np
import pytest
import torch

import extract_ref as E
import train_ref as T
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@functools.lru_cache(maxsize=None)
def _case(case):
    return T.load(GOLDEN, case)


def _net(method, training=True, **over):
    from mdgat_matcher_amd import MDGAT
    net = MDGAT(T.config(method, **over)).double()
    net.load_state_dict(T.initial_state())
    return net.to(DEV).train(training)


def _data(case):
    return {k: torch.from_numpy(v.copy()).to(DEV) for k, v in _case(case)['data'].items()}


def _result(net, out):
    """``train_ref.flatten``'s dict of what a step left on the module."""
    n = lambda t: t.detach().cpu().numpy()          # noqa: E731
    q = {'loss': n(out['loss'])}
    q.update({'grad:' + k: n(p.grad) for k, p in net.named_parameters() if p.grad is not None})
    q.update({'buf:' + k: n(b) for k, b in net.named_buffers() if not k.endswith('num_batches_tracked')})
    return q


def _nbt(net):
    return {k: int(b) for k, b in net.named_buffers() if k.endswith('num_batches_tracked')}


def _step(net, data):
    net.zero_grad(set_to_none=True)
    out = net.training_forward(data)
    out['loss'].mean().backward()
    torch.cuda.synchronize()
    return out


def _report(tag, fr):
    groups = {}
    for k, v in fr.items():
        g = k if k == 'loss' else k.split(':')[0] + ':' + '.'.join(k.split(':')[1].split('.')[:3 if 'gnn' in k else 1])
        groups[g] = max(groups.get(g, 0.0), v)
    for g, v in sorted(groups.items()):
        print(f'{tag}: {g}: worst fraction of the bound {v:.4f}')


@pytest.mark.parametrize('case', sorted(T.CASES))
def test_step_reproduces_fixture(case):
    c = _case(case)
    method = T.CASES[case][0]
    net, data = _net(method), _data(case)
    out = _step(net, data)
    assert out['loss'].grad_fn is not None and tuple(out['loss'].shape) == ((2,) if method == 'gap_loss' else ())
    assert set(out) == {'matches0', 'matches1', 'matching_scores0', 'matching_scores1', 'loss'}
    got = _result(net, out)
    names = [k for k in c['want'] if k != 'Z']
    assert all(('grad:' + k) in got for k, p in net.named_parameters()), 'a parameter was left without a gradient'
    worst, where, fr = T.compare(got, c['want'], c['err'], names=names)
    _report(case, fr)
    print(f'{case}: worst fraction of the bound {worst:.4f} at {where}')
    assert worst <= 1.0
    assert _nbt(net) == c['nbt']
    for f in (0, 1):
        assert out[f'matches{f}'].dtype == torch.int64 and np.array_equal(out[f'matches{f}'].cpu().numpy(), c[f'matches{f}'])
        s = out[f'matching_scores{f}']
        assert s.dtype == torch.float64
        e = float(np.abs(s.cpu().numpy() - c[f'mscores{f}']).max())
        print(f'{case}: matching_scores{f}: {e / E.SCORE_TOL:.4f} of extract\'s bound')
        assert e <= E.SCORE_TOL
    if method != 'superglue':           # the reference's in-place rewrite of the caller's gts
        g0, g1 = c['data']['gt_matches0'], c['data']['gt_matches1']
        assert np.array_equal(data['gt_matches0'].cpu().numpy(), np.where(g0 == -1, g1.shape[1], g0))
        assert np.array_equal(data['gt_matches1'].cpu().numpy(), np.where(g1 == -1, g0.shape[1], g1))
    else:
        assert np.array_equal(data['gt_matches0'].cpu().numpy(), c['data']['gt_matches0'])


def test_second_step_reads_parameters_and_buffers_fresh():
    c = _case('gap')
    net, data = _net('gap_loss'), _data('gap')
    _step(net, data)
    with torch.no_grad():
        for p in net.parameters():
            p -= T.SGD_LR * p.grad
    out = _step(net, _data('gap'))
    worst, where, fr = T.compare(_result(net, out), c['step2']['want'], c['step2']['err'])
    _report('gap, second step', fr)
    print(f'gap, second step: worst fraction of the bound {worst:.4f} at {where}')
    assert worst <= 1.0
    assert set(_nbt(net).values()) == {11}


def test_two_identical_steps_give_the_same_bits():
    res = []
    for _ in range(2):
        net = _net('gap_loss')
        out = _step(net, _data('gap'))
        res.append((_result(net, out), out))
    a, b = res[0][0], res[1][0]
    assert set(a) == set(b) and len(a) > 40
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for k in ('matches0', 'matches1', 'matching_scores0', 'matching_scores1'):
        assert torch.equal(res[0][1][k], res[1][1][k])


def test_eval_mode_leaves_the_buffers_and_agrees_with_forward():
    net, data = _net('gap_loss', training=False), _data('gap')
    before = {k: b.clone() for k, b in net.named_buffers()}
    out = net.training_forward(data)
    assert out['loss'].grad_fn is not None
    out['loss'].mean().backward()
    torch.cuda.synchronize()
    assert all(torch.equal(b, before[k]) for k, b in net.named_buffers())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    with torch.no_grad():
        ref = net(_data('gap'))
        quiet = net.training_forward(_data('gap'))
    assert quiet['loss'].grad_fn is None and torch.equal(quiet['loss'], out['loss'].detach())
    for f in (0, 1):
        assert torch.equal(out[f'matches{f}'], ref[f'matches{f}'])
        d = (out[f'matching_scores{f}'] - ref[f'matching_scores{f}']).abs().max().item()
        print(f'eval mode: matching_scores{f}: training_forward against forward: {d:.3e}')


# ---- the shape cases (train_ref.SHAPE_CASES): the step past one tile of every kernel it composes ----
def _shape_net(case, training=True):
    from mdgat_matcher_amd import MDGAT
    method, _, _, _, L, k, _ = T.case_spec(case)
    net = MDGAT(T.config(method, L=L, k=k)).double()
    net.load_state_dict(T.initial_state(L=L))
    return net.to(DEV).train(training)


@functools.lru_cache(maxsize=None)
def _restated(case):
    """The float64 restatement of the case's step on the host: the expected value of the layers' convolution weights, and the masks."""
    method, _, _, _, L, k, _ = T.case_spec(case)
    return T.step(T.numpy_state(T.initial_state(L=L)), _case(case)['data'], method, L=L, k_list=k)


@pytest.mark.parametrize('case', sorted(T.SHAPE_CASES))
def test_step_reproduces_shape_fixture(case, monkeypatch):
    from mdgat_matcher_amd import ops
    c, res = _case(case), _restated(case)
    method, B, N, M, L, k_list, _ = T.case_spec(case)
    net, data = _shape_net(case), _data(case)
    calls, attention = [], ops.attention_f64

    def recording(qkv, *a, **kw):           # what every layer handed its attention
        calls.append((qkv.detach().clone(), a, kw))
        return attention(qkv, *a, **kw)
    monkeypatch.setattr(ops, 'attention_f64', recording)
    out = _step(net, data)
    monkeypatch.undo()
    assert out['loss'].grad_fn is not None and tuple(out['loss'].shape) == ((B,) if method == 'gap_loss' else ())
    assert set(out) == {'matches0', 'matches1', 'matching_scores0', 'matching_scores1', 'loss'}
    # a dynamic layer kept the keys the restatement kept: a gradient outside the bound below is no selection difference in disguise
    sched = T.topk_schedule(L, k_list)
    assert len(calls) == 2 * L
    for i, (qkv, a, kw) in enumerate(calls):
        assert a == (N, M, bool(i % 2)) and kw == {'topk': sched[i]}
        if sched[i] > 0:
            _, masks = ops.attention_f64(qkv, N, M, bool(i % 2), topk=sched[i], return_selection=True)
            for side, (got_m, want_m) in enumerate(zip(masks, res['masks'][i])):
                differ = int((got_m.cpu().numpy() != want_m).any(-1).sum())
                assert differ == 0, f'layer {i}, frame {side}: {differ} rows selected unlike the top-{sched[i]} of the fp64 logits (gap {res["topk_gap"]:.2e})'
    got = _result(net, out)
    assert all(('grad:' + k) in got for k, p in net.named_parameters()), 'a parameter was left without a gradient'
    want = T.shape_want(c, res)
    names = [k for k in want if k != 'Z']
    assert len(names) == len(c['err']) - 1 and sum(not T.shape_stored(k) for k in names) == 12 * L
    worst, where, fr = T.compare(got, want, c['err'], names=names)
    _report(case, fr)
    print(f'{case}: worst fraction of the bound {worst:.4f} at {where}')
    assert worst <= 1.0
    assert _nbt(net) == c['nbt']
    for f in (0, 1):
        assert out[f'matches{f}'].dtype == torch.int64 and np.array_equal(out[f'matches{f}'].cpu().numpy(), c[f'matches{f}'])
        s = out[f'matching_scores{f}']
        assert s.dtype == torch.float64
        e = float(np.abs(s.cpu().numpy() - c[f'mscores{f}']).max())
        print(f'{case}: matching_scores{f}: {e / E.SCORE_TOL:.4f} of extract\'s bound')
        assert e <= E.SCORE_TOL
    if method != 'superglue':           # the reference's in-place rewrite of the caller's gts
        g0, g1 = c['data']['gt_matches0'], c['data']['gt_matches1']
        assert np.array_equal(data['gt_matches0'].cpu().numpy(), np.where(g0 == -1, g1.shape[1], g0))
        assert np.array_equal(data['gt_matches1'].cpu().numpy(), np.where(g1 == -1, g0.shape[1], g1))
    else:
        assert np.array_equal(data['gt_matches0'].cpu().numpy(), c['data']['gt_matches0'])


@pytest.mark.parametrize('case', ['one_pair', 'tiles'])
def test_two_identical_shape_steps_give_the_same_bits(case):
    res = []
    for _ in range(2):
        net = _shape_net(case)
        out = _step(net, _data(case))
        res.append((_result(net, out), out))
    a, b = res[0][0], res[1][0]
    assert set(a) == set(b) == {k for k in _case(case)['err'] if k != 'Z'}
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for k in ('matches0', 'matches1', 'matching_scores0', 'matching_scores1'):
        assert torch.equal(res[0][1][k], res[1][1][k])


@pytest.mark.parametrize('case', sorted(T.SHAPE_CASES))
def test_eval_mode_agrees_with_forward_at_shape(case):
    """``training_forward`` in eval mode against the exact-mode ``forward`` of the same module.  Each side's scores are ``ops.extract``'s,
    within SCORE_TOL of exp of its Z: 2 x SCORE_TOL between them."""
    net = _shape_net(case, training=False)
    before = {k: b.clone() for k, b in net.named_buffers()}
    out = net.training_forward(_data(case))
    assert out['loss'].grad_fn is not None
    out['loss'].mean().backward()
    torch.cuda.synchronize()
    assert all(torch.equal(b, before[k]) for k, b in net.named_buffers())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    with torch.no_grad():
        ref = net(_data(case))
    assert all(torch.equal(b, before[k]) for k, b in net.named_buffers())
    for f in (0, 1):
        assert torch.equal(out[f'matches{f}'], ref[f'matches{f}'])
        d = (out[f'matching_scores{f}'] - ref[f'matching_scores{f}']).abs().max().item()
        print(f'{case}, eval mode: matching_scores{f}: training_forward against forward: {d / (2 * E.SCORE_TOL):.4f} of the bound')
        assert d <= 2 * E.SCORE_TOL


def _train_loop(net, batches, optimizer):
    """The body of the reference's training loop (train.py:226-248) on ready batches: forward through the (wrapped) module, the mean of
    the returned loss, backward, one optimizer step; batches the forward asks to skip are skipped.  Returns the losses."""
    losses = []
    for batch in batches:
        out = net(batch)
        if 'skip_train' in out:
            continue
        optimizer.zero_grad()
        loss = torch.mean(out['loss'])
        losses.append(loss.item())
        loss.backward()
        optimizer.step()
    return losses


def test_training_loop_through_forward(monkeypatch):
    from mdgat_matcher_amd import MDGAT
    monkeypatch.setenv('MDGAT_TRAIN_FORWARD', '1')
    core = MDGAT(T.config('gap_loss')).double()
    core.load_state_dict(T.initial_state())
    net = torch.nn.DataParallel(core.to(DEV), device_ids=[0])
    before = {k: p.detach().clone() for k, p in core.named_parameters()}
    optimizer = torch.optim.Adam(net.parameters(), lr=core.lr)
    net.double().train()
    empty = _data('gap')
    empty['keypoints0'] = empty['keypoints0'][:, :0]
    losses = _train_loop(net, [_data('gap'), empty, _data('gap')], optimizer)
    torch.cuda.synchronize()
    print(f'two Adam iterations: loss {losses[0]:.6f} -> {losses[1]:.6f}')
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses) and losses[0] != losses[1]
    assert abs(losses[0] - float(_case('gap')['want']['loss'].mean())) < 1e-9
    moved = [k for k, p in core.named_parameters() if not torch.equal(p.detach(), before[k])]
    # (a bias in front of a BatchNorm has a gradient of rounding noise, which may be an exact zero: the weights must all have moved)
    assert {k for k in before if k.endswith('.weight') or k == 'bin_score'} <= set(moved), sorted(set(before) - set(moved))
    assert all(torch.isfinite(p).all() for p in core.parameters())
    # what was trained is what evaluates: the packed weights follow after repack()
    core.eval()
    with torch.no_grad():
        composed = core.training_forward(_data('gap'))
        core.repack()
        packed = core(_data('gap'))
    for f in (0, 1):
        assert torch.equal(composed[f'matches{f}'], packed[f'matches{f}'])
        d = (composed[f'matching_scores{f}'] - packed[f'matching_scores{f}']).abs().max().item()
        print(f'after training: matching_scores{f}: training_forward against forward: {d:.3e}')
    # ... and they are not the initial weights' matches or scores any more
    fresh = _net('gap_loss', training=False)
    with torch.no_grad():
        first = fresh(_data('gap'))
    assert (first['matching_scores0'] - packed['matching_scores0']).abs().max().item() > 1e-5


def test_forward_without_the_key_still_raises(monkeypatch):
    monkeypatch.delenv('MDGAT_TRAIN_FORWARD', raising=False)
    with pytest.raises(NotImplementedError):
        _net('gap_loss')(_data('gap'))


def test_early_out_and_refusals():
    net = _net('gap_loss')
    d = _data('gap')
    d['keypoints1'] = d['keypoints1'][:, :0]
    out = net.training_forward(d)
    assert out['skip_train'] is True and tuple(out['matches0'].shape) == (20,) and out['matches0'].dtype == torch.int32
    assert set(_nbt(net).values()) == {7}                      # nothing ran
    d = _data('gap')
    d['gt_matches0'][1, 3] = 29                                # outside [-1, M = 28]
    with pytest.raises(IndexError):
        net.training_forward(d)
    for method in ('superglue', 'triplet_loss'):               # N != M
        with pytest.raises(ValueError, match='equal size'):
            _net(method).training_forward(_data('gap'))
    with pytest.raises(NotImplementedError):
        _net('gap_loss').float().training_forward(_data('gap'))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net.training_forward({k: v.cpu() for k, v in _data('gap').items()})


def test_residual_operand_of_the_mlp():
    """ops.mlp_f64_tensors(..., residual=r) is ops.mlp_f64 + r in the last product's epilogue: the same bits as the sum formed by torch
    (one rounding either way), dout reaches the residual unchanged, and without a residual the entry gives mlp_f64's bits."""
    import mlp_grad_ref as R
    from mdgat_matcher_amd import ops
    for stack, rows in (('layer', 65), ('denc', 1000), ('conv128', 17)):
        x, p, dout = R.gpu_case(stack, rows)
        seq = R.torch_stack(p, True).to(DEV)
        seq2 = R.torch_stack(p, True).to(DEV)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)          # noqa: E731
        srcs = [t(x[:, :128]), t(x[:, 128:])] if stack == 'layer' else [t(x)]
        res = t(np.random.RandomState(rows).standard_normal(dout.shape))
        a_in = [s.clone().requires_grad_() for s in srcs]
        b_in = [s.clone().requires_grad_() for s in srcs]
        ra, rb = res.clone().requires_grad_(), res.clone().requires_grad_()
        want = ops.mlp_f64(seq, *a_in) + ra
        convs = [m for m in seq2 if isinstance(m, torch.nn.Conv1d)]
        bns = [m for m in seq2 if isinstance(m, torch.nn.BatchNorm1d)]
        got = ops.mlp_f64_tensors(b_in[0], [c.weight for c in convs], [c.bias for c in convs], bns, True,
                                  x1=b_in[1] if len(b_in) > 1 else None, residual=rb)
        assert torch.equal(got, want), stack
        want.backward(t(dout))
        got.backward(t(dout))
        torch.cuda.synchronize()
        assert torch.equal(rb.grad, t(dout)) and torch.equal(ra.grad, rb.grad)
        assert all(torch.equal(u.grad, v.grad) for u, v in zip(a_in, b_in))
        assert all(torch.equal(u.grad, v.grad) for u, v in zip(seq.parameters(), seq2.parameters()))
        assert all(torch.equal(u, v) for u, v in zip(seq.buffers(), seq2.buffers()))
        plain = ops.mlp_f64_tensors(srcs[0], [c.weight for c in convs], [c.bias for c in convs], bns, False, x1=srcs[1] if len(srcs) > 1 else None)
        assert torch.equal(plain, ops.mlp_f64(seq2.eval(), *srcs))
