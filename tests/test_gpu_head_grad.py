"""The matching head on the device: ops.match_head (final_proj and the score matrix by the exact mode's launches) and its backward
csrc/head_grad.hip through ops.match_head_backward and through autograd.  Expected values: the reference's own gradients
(tests/golden/head_grad*.npz, tools/make_goldens_head_grad.py) and the numpy restatement tests/head_grad_ref.py (pinned to the
reference and to torch autograd by tests/test_head_grad_ref.py).

Tolerance (head_grad_ref.tolerances), derived: a dot product of length K in fp64, in any order, with or without FMA, is off by at
most K u sum|a_k b_k| to first order, u = 2^-53; the formulas run on absolute values give sum|a_k b_k| = A per entry, K is the sum of
the contraction lengths on the way to the entry, and the tolerance is 4 K u A (two implementations, first-order truncation), plus
2^-24 |value| for an output rounded to float32.  Every comparison prints the worst |difference| / tolerance it met.

Measured on an MI355X (worst fraction of the bound over the file): see DESIGN section 7.4."""
import numpy as np
import pytest
import torch

import gemm_f64_forms as F
import head_grad_ref as R
from sinkhorn_grad_ref import max_rel
from test_head_grad_ref import CASE_METHODS, GRADS, random_inputs, torch_head

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module')
def g(golden_dir):
    return R.load_golden(golden_dir)


def _ops():
    from mdgat_matcher_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _backward(a):
    return [t.cpu().numpy() for t in _ops().match_head_backward(*[_dev(x) for x in a])]


def _assert_within(got, want, tol, what, out_eps=0.0):
    assert np.isfinite(got).all(), what
    frac = R.worst_fraction(got, want, tol, out_eps)
    print(f'{what}: {frac:.2e} of the bound', end='; ')
    assert frac <= 1.0, f'{what}: {frac:.3e} of the bound'
    return frac


# ------------------------------------------------------------------------------------------------ 1: the reference's own gradients
@pytest.mark.parametrize('case,meth', CASE_METHODS)
def test_kernel_reproduces_the_references_gradient(g, case, meth):
    a = [g[f'{case}_{k}'] for k in ('desc0', 'desc1', 'W', 'b')] + [g[f'{case}_{meth}_dscores']]
    tol = R.tolerances(*a)
    for k, got in zip(GRADS, _backward(a)):
        _assert_within(got, g[f'{case}_{meth}_{k}'], tol[k], f'{case} {meth} {k}')
    print()


# ------------------------------------------------------------------------------------------------ 2 / 3: the shapes it runs at
SHAPES = [(1, 1, 1), (1, 1, 5), (2, 17, 33), (2, 33, 17), (3, 64, 64), (2, 257, 255), (64, 512, 512), (2, 2048, 2048), (1, 2175, 2175)]
F32_SHAPES = [(2, 17, 33), (2, 257, 255)]


def _check_shape(B, N, M, f32):
    ops = _ops()
    a = random_inputs(B, N, M, 4000 + 7 * N + M, np.float32 if f32 else np.float64)
    a64 = [x.astype(np.float64) for x in a]             # (float32 inputs: the yardstick runs on the same rounded values)
    tol = R.tolerances(*a64)
    eps = 2.0 ** -24 if f32 else 0.0
    t = [_dev(x) for x in a]
    what = f'{B}x{N}x{M} {"fp32" if f32 else "fp64"}'
    scores = ops.match_head(*t[:4])
    assert scores.dtype == t[0].dtype and tuple(scores.shape) == (B, N, M)
    _assert_within(scores.cpu().numpy(), R.forward(*a64[:4]), tol['scores'], f'{what} scores', eps)
    got = ops.match_head_backward(*t)
    for k, x, like, want in zip(GRADS, got, t, R.backward(*a64)):
        assert x.dtype == like.dtype and x.shape == like.shape, k
        assert np.abs(want).max() > 0
        _assert_within(x.cpu().numpy(), want, tol[k], f'{what} {k}', eps)
    print()


@pytest.mark.parametrize('B,N,M', SHAPES)
def test_kernel_against_the_restatement(B, N, M):
    _check_shape(B, N, M, False)


@pytest.mark.parametrize('B,N,M', F32_SHAPES)
def test_kernel_against_the_restatement_float32(B, N, M):
    _check_shape(B, N, M, True)


# ------------------------------------------------------------------------------------------------ 3: the forward
# (gemm_f64_forms.BATCHED: batched, scaled score products of more than a round of workgroups, each written for one instantiation of
# gemm_f64_kernel - B is the first candidate for which the launcher's plan names that instantiation on this device)
@pytest.mark.parametrize('B,N,M', [(2, 17, 33), (3, 64, 64), (2, 257, 255)] + sorted(F.BATCHED))
def test_forward_against_torch_and_grad_fn(B, N, M):
    ops = _ops()
    want = None
    if (B, N, M) in F.BATCHED:
        form, cands = F.BATCHED[(B, N, M)]
        cus, want = F.cu_count(), F.index(form)
        B = F.pick(cands, want, cus, lambda b: dict(M=N, N=M, K=128, batch=b))
    a = random_inputs(B, N, M, 4000 + 7 * N + M)
    t = [_dev(x) for x in a[:4]]
    with F.watch() as launches:
        plain = ops.match_head(*t)
    if want is not None:        # final_proj of either frame, then the scores: by the counters, the instantiation this case was written for
        planned = np.zeros(10, dtype=np.int64)
        for idx in (F.plan(B * N, 128, 128, cus=cus), F.plan(B * M, 128, 128, cus=cus), F.plan(N, M, 128, batch=B, cus=cus)):
            planned[idx] += 1
        assert np.array_equal(launches.delta, planned) and launches.delta[want] >= 1, \
            f'{B}x{N}x{M}: wanted {F.NAMES[want]} for the scores, launched {launches.launched()} on a device of {cus} CUs'
    assert plain.grad_fn is None and not plain.requires_grad
    ref = torch_head(*t)
    _assert_within(plain.cpu().numpy(), ref.cpu().numpy(), R.tolerances(*a[:4])['scores'], f'{B}x{N}x{M} scores vs torch fp64')
    with torch.no_grad():
        quiet = ops.match_head(t[0].clone().requires_grad_(), *t[1:])
    assert quiet.grad_fn is None
    for i in range(4):
        r = [x.clone().requires_grad_(j == i) for j, x in enumerate(t)]
        s = ops.match_head(*r)
        assert s.grad_fn is not None and s.requires_grad
        assert torch.equal(s.detach(), plain) and torch.equal(quiet, plain)
    conv = ops.match_head(t[0], t[1], t[2].reshape(128, 128, 1), t[3])
    assert torch.equal(conv, plain)
    print()


def test_autograd_returns_the_raw_backward_in_the_shapes_given():
    ops = _ops()
    a = random_inputs(2, 40, 56, 11)
    t = [_dev(x) for x in a]
    r = [t[0].clone().requires_grad_(), t[1].clone().requires_grad_(), t[2].reshape(128, 128, 1).clone().requires_grad_(), t[3].clone().requires_grad_()]
    (ops.match_head(*r) * t[4]).sum().backward()
    raw = ops.match_head_backward(*t)
    assert r[2].grad.shape == (128, 128, 1)
    for x, y in zip(r, raw):
        assert torch.equal(x.grad.reshape(y.shape), y)
    s = ops.match_head(*r)
    gz, = torch.autograd.grad(s.sum(), r[0], create_graph=True)
    with pytest.raises(RuntimeError):
        gz.sum().backward()


# ------------------------------------------------------------------------------------------------ 4: batch independence and order
def test_a_pairs_gradient_does_not_depend_on_its_batch_and_runs_repeat():
    ops = _ops()
    B, N, M = 64, 200, 168
    a = random_inputs(B, N, M, 37)
    t = [_dev(x) for x in a]
    full = ops.match_head_backward(*t)
    alone = ops.match_head_backward(t[0][37:38], t[1][37:38], t[2], t[3], t[4][37:38])
    assert torch.equal(alone[0][0], full[0][37]) and torch.equal(alone[1][0], full[1][37])
    # the other pairs carry other descriptors and other dscores
    d0, d1, G = t[0].flip(1).clone(), t[1].roll(3, 1).clone(), (t[4] * 3).clone()
    d0[37], d1[37], G[37] = t[0][37], t[1][37], t[4][37]
    other = ops.match_head_backward(d0, d1, t[2], t[3], G)
    assert torch.equal(other[0][37], full[0][37]) and torch.equal(other[1][37], full[1][37])
    again = ops.match_head_backward(*t)
    for x, y in zip(again, full):
        assert torch.equal(x, y)


def test_64_pairs_of_512_repeat_bit_for_bit():
    ops = _ops()
    t = [_dev(x) for x in random_inputs(64, 512, 512, 4000 + 7 * 512 + 512)]
    first = ops.match_head_backward(*t)
    second = ops.match_head_backward(*t)
    for x, y in zip(first, second):
        assert torch.equal(x, y)


@pytest.mark.parametrize('N,M', [(64, 64), (257, 255), (33, 600)])
def test_two_pairs_sum_to_the_batch_bit_for_bit(N, M):
    ops = _ops()
    t = [_dev(x) for x in random_inputs(2, N, M, 91 + N)]
    both = ops.match_head_backward(*t)
    one = [ops.match_head_backward(t[0][b:b + 1], t[1][b:b + 1], t[2], t[3], t[4][b:b + 1]) for b in range(2)]
    assert torch.equal(both[2], one[0][2] + one[1][2])
    assert torch.equal(both[3], one[0][3] + one[1][3])
    for b in range(2):
        assert torch.equal(both[0][b], one[b][0][0]) and torch.equal(both[1][b], one[b][1][0])


# ------------------------------------------------------------------------------------------------ 5: desc -> scores -> Z -> loss -> backward
@pytest.mark.parametrize('case,meth', CASE_METHODS)
def test_the_whole_chain_reproduces_the_references_gradients(g, case, meth):
    """Tolerance: the 1e-8 of max|g| (1e-8 relative for dalpha) that tests/test_gpu_sinkhorn_grad.py and the composition test of
    tests/test_gpu_loss_grad.py assert for this chain."""
    ops = _ops()
    d0, d1, W, b = [_dev(g[f'{case}_{k}']).requires_grad_() for k in ('desc0', 'desc1', 'W', 'b')]
    al = torch.tensor(float(g[f'{case}_alpha']), dtype=torch.float64, device=DEV, requires_grad=True)
    scores = ops.match_head(d0, d1, W, b)
    Z = ops.log_optimal_transport(scores, al, int(g[f'{case}_iters']))
    loss = ops.matching_loss(Z, _dev(g[f'{case}_gt0']), _dev(g[f'{case}_gt1']), meth, float(g[f'{case}_gamma']))
    w = _dev(np.asarray(g[f'{case}_{meth}_w'], dtype=np.float64))
    ((loss * w).sum() if meth == 'gap_loss' else loss.mean() * w).backward()
    errs = {k: max_rel(t.grad.cpu(), torch.from_numpy(g[f'{case}_{meth}_{k}'])) for k, t in zip(GRADS, (d0, d1, W, b))}
    ref_da = float(g[f'{case}_{meth}_dalpha'])
    errs['dalpha'] = abs(float(al.grad) - ref_da) / abs(ref_da)
    print(f'{case} {meth}: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert all(v < 1e-8 for v in errs.values()), errs


# ------------------------------------------------------------------------------------------------ 6: optional outputs and errors
def test_only_the_gradients_asked_for(g):
    ops = _ops()
    a = random_inputs(2, 70, 90, 3)
    t = [_dev(x) for x in a]
    full = ops.match_head_backward(*t)
    d0 = t[0].clone().requires_grad_()
    r = [d0, t[1].clone(), t[2].clone(), t[3].clone()]
    (ops.match_head(*r) * t[4]).sum().backward()
    assert torch.equal(d0.grad, full[0]) and all(x.grad is None for x in r[1:])
    for i in range(4):
        need = tuple(j == i for j in range(4))
        part = ops.match_head_backward(*t, need=need)
        assert all((x is None) != n for x, n in zip(part, need)) and torch.equal(part[i], full[i])
    assert ops.match_head_backward(*t, need=(False,) * 4) == (None,) * 4
    e = ops.match_head_backward(t[0][:0], t[1][:0], t[2], t[3], t[4][:0])
    assert e[0].shape == (0, 70, 128) and e[1].shape == (0, 90, 128) and not e[2].any() and not e[3].any()
    assert ops.match_head(t[0][:0], t[1][:0], t[2], t[3]).shape == (0, 70, 90)


def test_error_paths():
    ops = _ops()
    a = random_inputs(2, 8, 9, 1)
    t = [_dev(x) for x in a]
    cpu = [torch.from_numpy(x) for x in a]
    with pytest.raises(RuntimeError):
        ops.match_head(*cpu[:4])
    with pytest.raises(RuntimeError):
        ops.match_head_backward(*cpu)
    with pytest.raises(ValueError):
        ops.match_head(t[0], t[1], t[2][:64], t[3])
    with pytest.raises(ValueError):
        ops.match_head(t[0], t[1], t[2].reshape(128, 128, 1, 1), t[3])
    with pytest.raises(ValueError):
        ops.match_head_backward(t[0], t[1], t[2].t()[:, :64], t[3], t[4])
    with pytest.raises(ValueError):
        ops.match_head(t[0], t[1][:1], t[2], t[3])
    with pytest.raises(ValueError):
        ops.match_head(t[0][:, :, :64], t[1], t[2], t[3])
    with pytest.raises(ValueError):
        ops.match_head_backward(*t[:4], t[4][:, :, :8])
    with pytest.raises(RuntimeError, match='2175'):
        ops.match_head(torch.zeros(1, 2176, 128, dtype=torch.float64, device=DEV), t[1][:1], t[2], t[3])


def test_raw_abi_refuses_bad_arguments_without_a_launch():
    from mdgat_matcher_amd import _lib
    lib = _lib.load()
    B, N, M = 2, 8, 9
    d0, d1, W, b, G = [_dev(x) for x in random_inputs(B, N, M, 1)]
    out = [torch.full(s, 7.0, dtype=torch.float64, device=DEV) for s in ((B, N, 128), (B, M, 128), (128, 128), (128,))]
    scores = torch.full((B, N, M), 7.0, dtype=torch.float64, device=DEV)
    need = lib.mdgat_match_head_workspace_bytes(B, N, M)
    assert need > 0 and need % 256 == 0
    assert lib.mdgat_match_head_workspace_bytes(B, 2176, M) == 0 and lib.mdgat_match_head_workspace_bytes(B, N, 2175) > 0
    ws = torch.empty(need + 512, dtype=torch.uint8, device=DEV)
    base = ws.data_ptr() + (-ws.data_ptr()) % 256
    st = torch.cuda.current_stream().cuda_stream
    p = lambda x: x.data_ptr()                                                                                     # noqa: E731

    def bwd(B=B, N=N, M=M, d0=p(d0), G=p(G), wsp=base, nbytes=need):
        return lib.mdgat_match_head_backward(B, N, M, d0, p(d1), p(W), p(b), G, p(out[0]), p(out[1]), p(out[2]), p(out[3]), wsp, nbytes, st)

    def fwd(B=B, N=N, M=M, W=p(W), wsp=base, nbytes=need):
        return lib.mdgat_match_head_f64(B, N, M, p(d0), p(d1), W, p(b), p(scores), wsp, nbytes, st)
    for call in (bwd, fwd):
        assert call(nbytes=need - 1) == _lib.ERR_BAD_ARG and 'workspace' in _lib.last_error()
        assert call(wsp=base + 8) == _lib.ERR_BAD_ARG
        assert call(wsp=None) == _lib.ERR_BAD_ARG
        assert call(N=2176) == _lib.ERR_UNSUPPORTED and '2175' in _lib.last_error()
        assert call(M=2176) == _lib.ERR_UNSUPPORTED
        assert call(B=-1) == _lib.ERR_BAD_ARG
        assert call(N=0) == _lib.ERR_BAD_ARG
        assert call(B=0) == _lib.OK
    assert bwd(d0=None) == _lib.ERR_BAD_ARG and 'null' in _lib.last_error()
    assert bwd(G=None) == _lib.ERR_BAD_ARG
    assert fwd(W=None) == _lib.ERR_BAD_ARG
    torch.cuda.synchronize()
    for x in out + [scores]:
        assert (x == 7.0).all()                      # nothing was launched
    assert lib.mdgat_match_head_backward(B, N, M, p(d0), p(d1), p(W), p(b), p(G), None, None, None, None, base, need, st) == _lib.OK
    assert bwd() == _lib.OK and fwd() == _lib.OK
    torch.cuda.synchronize()
    for x in out + [scores]:
        assert torch.isfinite(x).all() and not (x == 7.0).all()
