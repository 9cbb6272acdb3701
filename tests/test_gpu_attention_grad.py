"""The backward of the fp64 attention on the device: csrc/attention_grad.hip through ops.attention_f64_backward and through autograd
of ops.attention_f64.  Expected values: the reference's own gradients (tests/golden/attention_grad_*.npz,
tools/make_goldens_attention_grad.py) and the numpy restatement tests/attention_grad_ref.py (pinned to the reference and to torch
autograd of the oracle by tests/test_attention_grad_ref.py).

Tolerance (attention_grad_ref.tolerances), derived there: K u sum|a_k b_k| per dot product, the formulas rerun on absolute values,
a logit's error carried into the probabilities as a relative error, times 4.  Every entry is compared, none excluded, and every
comparison prints the worst |difference| / tolerance it met.  For dynamic layers the restatement is fed the kernel's own selection,
which is first asserted equal to the top-k of the fp64 logits.

Measured on an MI355X (worst fraction of the bound per case): see DESIGN section 7.5."""
import numpy as np
import pytest
import torch

import attention_grad_ref as R
from test_attention_grad_ref import CASE_NAMES, random_inputs

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _ops():
    from mdgat_matcher_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _forward_selection(x, N, M, cross, k):
    """(message, raw selection words, masks) of the forward launch; the words are None for full attention."""
    ops = _ops()
    msg, sel = ops._attention_f64_values(x, N, M, cross, k, k > 0)
    return msg, sel, (ops.topk_sel_to_masks(sel, x.shape[0], N, M, cross) if k > 0 else None)


def _assert_within(got, want, tol, what):
    assert np.isfinite(got).all(), what
    fr = [R.worst_fraction(got[:, :, i], want[:, :, i], tol[:, :, i]) for i in range(3)]
    print(f'{what}: dq {fr[0]:.2e} dk {fr[1]:.2e} dv {fr[2]:.2e} of the bound')
    assert max(fr) <= 1.0, f'{what}: {max(fr):.3e} of the bound'
    return max(fr)


def _run_against_restatement(B, N, M, cross, k, seed, pairs=None):
    """The kernel on B pairs against the restatement on the pairs ``pairs`` (default: all), with the kernel's own masks."""
    ops = _ops()
    qkv, dmsg = random_inputs(B, N, M, seed)
    x = _dev(qkv)
    _, sel, masks = _forward_selection(x, N, M, cross, k)
    got = ops.attention_f64_backward(x, N, M, cross, _dev(dmsg), k, sel).cpu().numpy()
    idx = list(range(B)) if pairs is None else list(pairs)
    sub = None
    if k > 0:
        sub = tuple(m[idx].cpu().numpy() for m in masks)
        own, gap = R.topk_masks(qkv[idx], N, M, cross, k)
        for a, b in zip(sub, own):
            assert np.array_equal(a, b), f'{int((a ^ b).any(-1).sum())} rows selected unlike the top-k of the fp64 logits (gap {gap:.2e})'
    want = R.backward(qkv[idx], N, M, cross, dmsg[idx], sub)
    tol = R.tolerances(qkv[idx], N, M, cross, dmsg[idx], sub)
    return _assert_within(got[idx], want, tol, f'B={B} {N}x{M} cross={cross} k={k}'), got


# ------------------------------------------------------------------------------------------------ 1: goldens and restatement
@pytest.mark.parametrize('case', CASE_NAMES)
def test_kernel_reproduces_the_references_gradient(golden_dir, case):
    g = R.load_golden(golden_dir, case)
    B, N, M, cross, k = (int(v) for v in g['meta'])
    cross = bool(cross)
    x = _dev(g['qkv'])
    msg, sel, masks = _forward_selection(x, N, M, cross, k)
    if k > 0:
        for a, b in zip(masks, g['masks']):
            assert np.array_equal(a.cpu().numpy(), b)
    assert np.abs(msg.cpu().numpy() - g['msg']).max() < 1e-11
    got = _ops().attention_f64_backward(x, N, M, cross, _dev(g['dmsg']), k, sel).cpu().numpy()
    _assert_within(got, g['dqkv'], R.tolerances(g['qkv'], N, M, cross, g['dmsg'], g['masks']), case)


@pytest.mark.parametrize('B,N,M,cross,k', [(2, 17, 17, False, 16), (2, 40, 56, True, 8), (2, 64, 64, False, 0), (2, 64, 64, False, 1), (2, 64, 64, True, 63),
                                           (2, 100, 70, False, 70), (2, 300, 500, True, 64), (1, 513, 513, False, 512), (1, 1024, 1024, False, 128),
                                           (1, 2048, 2048, False, 0), (1, 2048, 2048, True, 64)])
def test_kernel_against_the_restatement(B, N, M, cross, k):
    _run_against_restatement(B, N, M, cross, k, seed=N + 13 * M + k)


@pytest.mark.parametrize('cross,k', [(False, 0), (True, 0), (False, 128), (True, 128)])
def test_kernel_against_the_restatement_64_pairs_of_512(cross, k):
    """The flagship shape: every pair travels through the kernel; the restatement is run on pairs 0, 31 and 63."""
    _run_against_restatement(64, 512, 512, cross, k, seed=512 + k + cross, pairs=(0, 31, 63))


# ------------------------------------------------------------------------------------------------ 2: the forward's forms
@pytest.mark.parametrize('form', [0, 1])
def test_backward_under_both_full_attention_forward_forms(form):
    """The backward does not depend on the forward's launch form; with either one set the gradient is within the bound and the same bits."""
    from mdgat_matcher_amd import _lib
    lib = _lib.load()
    ops = _ops()
    N, M = 100, 70
    qkv, dmsg = random_inputs(2, N, M, 77)
    x = _dev(qkv).requires_grad_()
    plain = ops.attention_f64_backward(x, N, M, True, _dev(dmsg))
    lib.mdgat_set_f64_attention_form(form)
    try:
        msg = ops.attention_f64(x, N, M, True)
        msg.backward(_dev(dmsg))
    finally:
        lib.mdgat_set_f64_attention_form(-2)
    assert np.abs(msg.detach().cpu().numpy() - R.forward(qkv, N, M, True)).max() < 1e-11
    assert torch.equal(x.grad, plain)
    _assert_within(x.grad.cpu().numpy(), R.backward(qkv, N, M, True, dmsg), R.tolerances(qkv, N, M, True, dmsg), f'form {form}')


# ------------------------------------------------------------------------------------------------ 3: determinism
@pytest.mark.parametrize('cross,k', [(False, 0), (True, 128)])
def test_runs_repeat_and_a_pair_does_not_depend_on_its_batch(cross, k):
    ops = _ops()
    B, N, M = 64, 512, 512
    qkv, dmsg = random_inputs(B, N, M, 9 + k)
    x, g = _dev(qkv), _dev(dmsg)
    _, sel, _ = _forward_selection(x, N, M, cross, k)
    one = ops.attention_f64_backward(x, N, M, cross, g, k, sel)
    two = ops.attention_f64_backward(x, N, M, cross, g, k, sel)
    assert torch.equal(one, two)
    for b in (0, 37):
        _, sel_b, _ = _forward_selection(x[b:b + 1], N, M, cross, k)
        if k > 0:
            W = sel.numel() // B
            assert torch.equal(sel_b, sel[b * W:(b + 1) * W])
        alone = ops.attention_f64_backward(x[b:b + 1], N, M, cross, g[b:b + 1], k, sel_b)
        assert torch.equal(alone[0], one[b])


@pytest.mark.parametrize('N,M,cross', [(64, 64, False), (40, 56, True), (300, 500, True)])
def test_one_kept_key_sends_exact_zeros(N, M, cross):
    """k = 1: keys that no query kept get exactly 0.0 in dk and dv, and dq - the gradient through a one-element softmax - is within
    the bound of 0."""
    B = 2
    worst, got = _run_against_restatement(B, N, M, cross, 1, seed=3 * N + M)
    qkv, dmsg = random_inputs(B, N, M, 3 * N + M)
    masks, _ = R.topk_masks(qkv, N, M, cross, 1)
    tol = R.tolerances(qkv, N, M, cross, dmsg, masks)
    assert (np.abs(got[:, :, 0]) <= tol[:, :, 0]).all()
    seen = 0
    for (qs, ks), mask in zip(R._sides(N, M, cross), masks):
        unkept = ~mask.any(axis=2)
        rows = np.transpose(got[:, ks, 1:], (0, 3, 1, 2, 4))
        assert (rows[unkept] == 0.0).all()
        seen += int(unkept.sum())
    assert seen > 0


# ------------------------------------------------------------------------------------------------ 4: autograd
@pytest.mark.parametrize('N,M,cross,k', [(64, 64, False, 0), (40, 56, True, 8), (512, 512, False, 128)])
def test_autograd_of_attention_f64(N, M, cross, k):
    ops = _ops()
    B = 2
    qkv, dmsg = random_inputs(B, N, M, 21 + k)
    x, g = _dev(qkv), _dev(dmsg)
    plain = ops.attention_f64(x, N, M, cross, topk=k)
    assert plain.grad_fn is None and not plain.requires_grad
    plain_sel, plain_masks = ops.attention_f64(x, N, M, cross, topk=max(k, 1), return_selection=True)
    xg = x.clone().requires_grad_()
    msg = ops.attention_f64(xg, N, M, cross, topk=k)
    assert msg.grad_fn is not None and torch.equal(msg.detach(), plain)
    msg.backward(g)
    _, sel, _ = _forward_selection(x, N, M, cross, k)
    assert torch.equal(xg.grad, ops.attention_f64_backward(x, N, M, cross, g, k, sel))
    # the masks come back the same, and are not differentiable
    xs = x.clone().requires_grad_()
    msg2, masks2 = ops.attention_f64(xs, N, M, cross, topk=max(k, 1), return_selection=True)
    assert msg2.grad_fn is not None and torch.equal(msg2.detach(), plain_sel)
    assert all(torch.equal(a, b) and not a.requires_grad for a, b in zip(masks2, plain_masks))
    # under no_grad nothing is recorded
    with torch.no_grad():
        assert ops.attention_f64(xg, N, M, cross, topk=k).grad_fn is None
    # once differentiable
    xd = x.clone().requires_grad_()
    first, = torch.autograd.grad(ops.attention_f64(xd, N, M, cross, topk=k), xd, g, create_graph=True)
    with pytest.raises(RuntimeError):
        first.sum().backward()


def test_fp32_class_attention_stays_without_a_backward():
    ops = _ops()
    qkv, _ = random_inputs(1, 64, 64, 4)
    out = ops.attention(_dev(qkv).float().requires_grad_(), 64, 64, False)
    assert out.grad_fn is None


# ------------------------------------------------------------------------------------------------ 5: composition
def test_composition_reproduces_the_references_multi_headed_attention(golden_dir):
    """torch fp64 1x1 convolutions on the device around ops.attention_f64, channels permuted from the reference's dim * 4 + head to
    the library's head * 32 + dim (pack.py): the module's output, dx, dsource and the eight weight and bias gradients the reference's
    MultiHeadedAttention.forward recorded (dynamic, one direction of a cross layer), within the composed bound."""
    ops = _ops()
    g = R.load_mha(golden_dir)
    n, m, k = g['x'].shape[1], g['source'].shape[1], g['k']
    leaf = lambda a: _dev(a).requires_grad_()                                                    # noqa: E731
    x, source = leaf(g['x']), leaf(g['source'])
    w = {name: leaf(a) for name, a in g['w'].items()}
    perm = torch.from_numpy(R.PERM).to(DEV)
    conv = lambda t, W, b: torch.nn.functional.conv1d(t.transpose(1, 2), W[:, :, None], b).transpose(1, 2)     # noqa: E731
    desc = torch.cat([x, source], dim=1)
    qkv = torch.stack([conv(desc, w['W' + c], w['b' + c])[..., perm] for c in 'qkv'], dim=2).reshape(1, n + m, 3, 4, 32)
    msg, masks = ops.attention_f64(qkv, n, m, True, topk=k, return_selection=True)
    assert msg.grad_fn is not None
    assert np.array_equal(masks[0].cpu().numpy(), g['masks'][0])
    out = conv(msg[:, :n][..., torch.argsort(perm)], w['Wm'], w['bm'])
    assert np.abs(out.detach().cpu().numpy() - g['out']).max() < 1e-11
    (out * _dev(g['dout'])).sum().backward()
    got = {'dx': x.grad, 'dsource': source.grad, **{'d' + name: t.grad for name, t in w.items()}}
    tol = R.mha_tolerances(g['x'], g['source'], g['w'], g['dout'], g['masks'])
    for name in R.MHA_GRADS:
        frac = R.worst_fraction(got[name].cpu().numpy(), g[name], tol[name])
        print(f'{name}: {frac:.2e} of the bound', end='; ')
        assert frac <= 1.0, (name, frac)
    print()


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_error_paths():
    ops = _ops()
    qkv, dmsg = random_inputs(1, 8, 9, 1)
    x, g = _dev(qkv), _dev(dmsg)
    with pytest.raises(RuntimeError):
        ops.attention_f64_backward(torch.from_numpy(qkv), 8, 9, False, torch.from_numpy(dmsg))
    with pytest.raises(ValueError, match='selection'):
        ops.attention_f64_backward(x, 8, 9, False, g, topk=4)
    with pytest.raises(ValueError):
        ops.attention_f64_backward(x, 8, 9, False, g[:, :, :64])
    with pytest.raises(ValueError):
        ops.attention_f64_backward(x, 9, 9, False, g)
    with pytest.raises(ValueError):
        ops.attention_f64_backward(x, 8, 9, False, g, topk=4, selection=torch.zeros(3, dtype=torch.int32, device=DEV))
    sel = torch.zeros(ops.topk_sel_words(1, 8, 9), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match='number of keys'):
        ops.attention_f64_backward(x, 8, 9, False, g, topk=9, selection=sel)


def test_raw_abi_refuses_bad_arguments_without_a_launch():
    from mdgat_matcher_amd import _lib
    lib = _lib.load()
    ops = _ops()
    B, N, M, k = 2, 24, 20, 8
    qkv, dmsg = random_inputs(B, N, M, 1)
    x, g = _dev(qkv), _dev(dmsg)
    _, sel, _ = _forward_selection(x, N, M, True, k)
    out = torch.full(x.shape, 7.0, dtype=torch.float64, device=DEV)
    need = lib.mdgat_attention_backward_workspace_bytes(B, N, M)
    assert need >= B * 4 * (N + M) * 16 and need % 256 == 0 and need < B * 4 * (N + M) * 16 + 256
    assert lib.mdgat_attention_backward_workspace_bytes(B, 2049, M) == 0 and lib.mdgat_attention_backward_workspace_bytes(B, 2048, 2048) > 0
    assert lib.mdgat_attention_backward_workspace_bytes(0, N, M) == 0
    ws = torch.empty(need + 512, dtype=torch.uint8, device=DEV)
    base = ws.data_ptr() + (-ws.data_ptr()) % 256
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()                                                                                     # noqa: E731

    def call(B=B, N=N, M=M, topk=k, qkv=p(x), sel=p(sel), dmsg=p(g), wsp=base, nbytes=need):
        return lib.mdgat_attention_backward_f64(B, N, M, 1, topk, qkv, sel, dmsg, p(out), wsp, nbytes, st)
    assert call(N=2049) == _lib.ERR_UNSUPPORTED and '2048' in _lib.last_error()
    assert call(M=2049) == _lib.ERR_UNSUPPORTED
    assert call(topk=M + 1) == _lib.ERR_BAD_ARG and 'number of keys' in _lib.last_error()
    assert call(topk=-1) == _lib.ERR_BAD_ARG
    assert call(sel=None) == _lib.ERR_BAD_ARG and 'selection' in _lib.last_error()
    assert call(nbytes=need - 1) == _lib.ERR_BAD_ARG and 'workspace' in _lib.last_error()
    assert call(wsp=base + 8) == _lib.ERR_BAD_ARG
    assert call(wsp=None) == _lib.ERR_BAD_ARG
    assert call(qkv=None) == _lib.ERR_BAD_ARG and 'null' in _lib.last_error()
    assert call(dmsg=None) == _lib.ERR_BAD_ARG
    assert call(B=-1) == _lib.ERR_BAD_ARG
    assert call(N=0) == _lib.ERR_BAD_ARG
    assert call(B=0) == _lib.OK
    torch.cuda.synchronize()
    assert (out == 7.0).all()                        # nothing was launched
    assert call(topk=0, sel=None) == _lib.OK         # full attention ignores sel
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not (out == 7.0).any()
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(out, ops.attention_f64_backward(x, N, M, True, g, k, sel))
    empty = ops.attention_f64_backward(x[:0], N, M, True, g[:0])
    assert tuple(empty.shape) == (0, N + M, 3, 4, 32)


# ------------------------------------------------------------------------------------------------ 7: streams
def test_on_a_stream_of_the_callers_own():
    ops = _ops()
    N, M, k = 100, 70, 16
    qkv, dmsg = random_inputs(2, N, M, 8)
    x, g = _dev(qkv), _dev(dmsg)
    _, sel, _ = _forward_selection(x, N, M, True, k)
    one = ops.attention_f64_backward(x, N, M, True, g, k, sel)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.device(DEV), torch.cuda.stream(side):
        xg = x.clone().requires_grad_()
        ops.attention_f64(xg, N, M, True, topk=k).backward(g)
        two = ops.attention_f64_backward(x, N, M, True, g, k, sel)
    torch.cuda.synchronize()
    assert torch.equal(one, two) and torch.equal(xg.grad, one)
