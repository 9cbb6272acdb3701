"""Every plain instantiation of gemm_f64_kernel (csrc/f64.hip) at the shape that reaches it, through the raw mdgat_pointwise_f64 entry:
C = act(A W^T + b) (+ R) against the same operation in np.longdouble on the CPU.  (The BNT instantiations and the two-source chunks:
tests/test_gpu_mlp_grad.py; batched and scaled products: tests/test_gpu_head_grad.py; the launcher's rule: tests/test_gemm_f64_plan.py.)

Tolerance, derived: a sum of K products in fp64, in any order, with or without FMA, is off by at most K u sum_k |a_mk||w_nk| to first
order (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), u = 2^-53; the scale, the bias and the residual add one
rounding each.  Per element, with S = sum_k |a_mk||w_nk|:

    |got - ref| <= (K + 3) u (|scale| S + |b_n| + |r_mn|)

(scale = 1 through this entry.)  A ReLU is decided the same way by both sides only where the pre-activation is far from zero: every
ReLU case asserts on the CPU that no pre-activation lies within 1e3 bounds of zero.  Every case prints the worst fraction of the bound it
met, and asserts by the launch counters (mdgat_gemm_f64_launches) the instantiation it was written for; shapes that depend on the
device's CU count are picked by mdgat_gemm_f64_plan from the candidates of tests/gemm_f64_forms.py.

Every operand is a view into a larger buffer that is NaN outside the view, and the output buffer holds a sentinel bit pattern: a read
beyond a view poisons the result, a write beyond the M x N view changes a sentinel."""
import numpy as np
import pytest
import torch

import gemm_f64_forms as F

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = 2.0 ** -53
LD = np.longdouble
SENTINEL = np.array([0x7ff8dead0000beef], dtype=np.uint64).view(np.int64)[0]      # a quiet NaN no arithmetic produces
#  (bias, relu, residual)
VARIANTS = [(False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, True, True)]

_products = {}


def _operands(M, N, K, seed):
    """Asymmetric random operands (a transposed or swapped fragment mapping cannot pass: tests/test_gpu_ops.py::
    test_pointwise_is_transpose_safe), their product in long double and S = |A||W|^T.  Computed once per shape, never written again."""
    key = (M, N, K, seed)
    if key not in _products:
        rs = np.random.RandomState(seed)
        a = rs.standard_normal((M, K)) + 0.25 * np.arange(M)[:, None] / M
        w = rs.standard_normal((N, K)) * (1.0 + np.arange(K) / K) / np.sqrt(K)
        b = rs.standard_normal(N)
        r = rs.standard_normal((M, N))
        P = np.einsum('mk,nk->mn', a.astype(LD), w.astype(LD))
        S = np.abs(a) @ np.abs(w).T
        for v in (a, w, b, r, P, S):
            v.setflags(write=False)
        _products[key] = (a, w, b, r, P, S)
    return _products[key]


def _expected(M, N, K, seed, bias, relu, res):
    """(ref in long double, bound) of one case; asserts the ReLU condition."""
    a, w, b, r, P, S = _operands(M, N, K, seed)
    bb = b if bias else np.zeros(N)
    rr = r if res else np.zeros((M, N))
    bound = (K + 3) * U * (S + np.abs(bb) + np.abs(rr))
    pre = P + bb.astype(LD)
    if relu:
        margin = float((np.abs(pre) / bound).min())
        assert margin >= 1e3, f'a pre-activation lies within {margin:.3g} bounds of zero: pick another seed'
        pre = np.maximum(pre, LD(0))
    return pre + rr.astype(LD), bound


def _view(values, off, ld, tail=3):
    """A host buffer, NaN everywhere but for ``values`` [rows][cols] laid out from element ``off`` with leading dimension ``ld``."""
    rows, cols = values.shape
    assert ld >= cols
    buf = np.full(off + rows * ld + tail, np.nan)
    buf[off:off + rows * ld].reshape(rows, ld)[:, :cols] = values
    return buf


def _launch(M, N, K, A, offA, lda, W, offW, ldw, b, relu, R, offR, ldr, Cbuf, offC, ldc):
    """mdgat_pointwise_f64 on device buffers (element offsets into them); R may be Cbuf itself."""
    from mdgat_matcher_amd import _lib
    p = lambda t, off: t.data_ptr() + 8 * off                      # noqa: E731
    rc = _lib.load().mdgat_pointwise_f64(M, N, K, p(A, offA), lda, p(W, offW), ldw, None if b is None else b.data_ptr(), int(relu),
                                         None if R is None else p(R, offR), ldr, p(Cbuf, offC), ldc, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, 'mdgat_pointwise_f64')
    torch.cuda.synchronize()


def _case(what, M, N, K, bias, relu, res, want, seed=None, offA=0, lda=None, offW=0, ldw=None, offC=0, ldc=None, ldr=None, alias=False):
    """One product: the bound, the sentinels around C, the instantiation.  ``want``: a form of gemm_f64_forms.FORMS.
    alias: R is C itself, preloaded with the residual."""
    seed = 100000 + 1000 * M + 10 * N + K if seed is None else seed
    lda, ldw, ldc = lda or K, ldw or K, ldc or N
    ldr = ldc if alias else (ldr or N)
    a, w, b, r, _, _ = _operands(M, N, K, seed)
    ref, bound = _expected(M, N, K, seed, bias, relu, res)
    dev = lambda x: torch.from_numpy(x).to(DEV)                    # noqa: E731
    A, W = dev(_view(a, offA, lda)), dev(_view(w, offW, ldw))
    assert A.data_ptr() % 16 == 0 and W.data_ptr() % 16 == 0
    host = np.full(offC + M * ldc + 5, SENTINEL, dtype=np.int64)
    inside = np.zeros(host.shape, dtype=bool)
    inside[offC:offC + M * ldc].reshape(M, ldc)[:, :N] = True
    if alias:
        assert res
        host[offC:offC + M * ldc].reshape(M, ldc)[:, :N] = r.view(np.int64)
    Cbuf = dev(host)
    Rbuf, offR = (Cbuf, offC) if alias else (dev(_view(r, 1, ldr)), 1) if res else (None, 0)
    cus = F.cu_count()
    with F.watch() as wt:
        _launch(M, N, K, A, offA, lda, W, offW, ldw, dev(b.copy()) if bias else None, relu, Rbuf, offR, ldr, Cbuf, offC, ldc)
    back = Cbuf.cpu().numpy()
    got = back[offC:offC + M * ldc].reshape(M, ldc)[:, :N].view(np.float64)
    frac = float((np.abs(got.astype(LD) - ref) / bound).max())
    print(f'{what} {M}x{N}x{K} bias={int(bias)} relu={int(relu)} res={int(res)}: worst fraction of the bound {frac:.3f}, '
          f'launched {wt.launched()} on {cus} CUs')
    F.assert_launched(wt, F.index(want), cus, what)
    assert wt.delta.sum() == 1, wt.launched()
    assert np.array_equal(back[~inside], host[~inside]), f'{what}: {int((back[~inside] != host[~inside]).sum())} words outside the {M} x {N} view changed'
    assert frac <= 1.0, f'{what}: {frac:.3e} of the bound'          # (a NaN fails this too)
    return frac


# ------------------------------------------------------------------------------------------------ (a) one case per plain instantiation
@pytest.mark.parametrize('bias,relu,res', VARIANTS)
@pytest.mark.parametrize('form', F.FORMS)
def test_every_plain_instantiation(form, bias, relu, res):
    cus = F.cu_count()
    M, N, K = F.pick(F.PLAIN[form], F.index(form), cus, lambda s: dict(M=s[0], N=s[1], K=s[2]))
    _case(form, M, N, K, bias, relu, res, form)


@pytest.mark.parametrize('bias,relu,res', [(False, False, False), (True, True, True)])
def test_wide_general_form_ragged_in_every_dimension(bias, relu, res):
    cus = F.cu_count()
    M, N, K = F.pick(F.WIDE_RAGGED, F.index('<4,slow>'), cus, lambda s: dict(M=s[0], N=s[1], K=s[2]))
    _case('<4,slow> ragged', M, N, K, bias, relu, res, '<4,slow>')


# ------------------------------------------------------------------------------------------------ (b) tile edges of the general form
# M in {1, 63, 65, 129}, N in {1, 15, 17, 63, 65, 129}, K in {1, 3, 5, 31, 33, 63, 65}: every value at least once
EDGES = [(1, 1, 1), (63, 15, 3), (65, 17, 5), (129, 63, 31), (1, 65, 33), (63, 129, 63), (65, 1, 65), (129, 129, 65), (129, 17, 1),
         (65, 65, 33), (63, 63, 63)]


def test_edge_shapes_hold_every_value():
    for i, vals in enumerate(((1, 63, 65, 129), (1, 15, 17, 63, 65, 129), (1, 3, 5, 31, 33, 63, 65))):
        assert {s[i] for s in EDGES} == set(vals)


@pytest.mark.parametrize('bias,relu,res', [(False, False, False), (True, True, True)])
@pytest.mark.parametrize('M,N,K', EDGES)
def test_tile_edges_of_the_general_form(M, N, K, bias, relu, res):
    _case('edge', M, N, K, bias, relu, res, '<2,slow>')


# ------------------------------------------------------------------------------------------------ (c) strides, alignment, aliasing
# name -> (keyword arguments of _case, the form of the 64 x 64 x 64 base); the 65 x 48 x 33 base is <2,slow> whatever its operands
LAYOUTS = {
    'natural': ({}, '<2,fast,64>'),
    'A_odd_offset': ({'offA': 1}, '<2,slow>'),
    'W_odd_offset': ({'offW': 1}, '<2,slow>'),
    'A_and_W_even_offset': ({'offA': 2, 'offW': 6}, '<2,fast,64>'),
    'lda_K+1': ({'lda': 1}, '<2,slow>'),
    'ldw_K+1': ({'ldw': 1}, '<2,slow>'),
    'lda_ldw_K+2': ({'lda': 2, 'ldw': 2}, '<2,fast,64>'),
    'ldc_N+3_ldr_N+5': ({'ldc': 3, 'ldr': 5, 'offC': 3}, '<2,fast,64>'),
    'R_aliases_C': ({'alias': True, 'offC': 1}, '<2,fast,64>'),
    'R_aliases_C_ldc_N+3': ({'alias': True, 'ldc': 3, 'offC': 2}, '<2,fast,64>'),
}


@pytest.mark.parametrize('base', [(64, 64, 64), (65, 48, 33)])
@pytest.mark.parametrize('name', sorted(LAYOUTS))
def test_strides_alignment_and_aliasing(name, base):
    M, N, K = base
    kw, fast_form = LAYOUTS[name]
    kw = dict(kw)
    for k, natural in (('lda', K), ('ldw', K), ('ldc', N), ('ldr', N)):
        if k in kw:
            kw[k] += natural
    want = fast_form if base == (64, 64, 64) else '<2,slow>'
    # the launcher's own statement of the case: the plan, told whether the alignment conditions hold, names the same form
    aligned = kw.get('offA', 0) % 2 == 0 and kw.get('offW', 0) % 2 == 0 and kw.get('lda', K) % 2 == 0 and kw.get('ldw', K) % 2 == 0
    assert F.plan(M, N, K, aligned=aligned, cus=F.cu_count()) == F.index(want)
    _case(name, M, N, K, True, True, True, want, **kw)


# ------------------------------------------------------------------------------------------------ the ten indices
def test_counters_never_run_backwards_and_name_ten_forms():
    before = F.counts()
    _case('counter', 64, 64, 64, False, False, False, '<2,fast,64>')
    after = F.counts()
    assert len(after) == 10 and (after >= before).all() and after.sum() == before.sum() + 1
    assert len(set(F.NAMES)) == 10
