"""tests/attention_grad_ref.py - the numpy restatement of the fp64 attention's gradient and its derived error bound - against the
reference's own gradients (tests/golden/attention_grad_*.npz, tools/make_goldens_attention_grad.py) and against torch autograd
through the oracle's attention / dynamic_attention on further seeded shapes; and the conditions on the inputs of
tests/test_gpu_attention_grad_hard.py (how far the logits reach, that the lazy reference moves, the restatement against
np.longdouble).  CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attention_grad_ref as R
from oracle import mdgat_oracle as O

CASE_NAMES = [c[0] for c in R.CASES]


def random_inputs(B, N, M, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((B, N + M, 3, 4, 32)) * 1.3, rs.standard_normal((B, N + M, 128))


def oracle_backward(qkv, N, M, cross, dmsg, k):
    """(message, dqkv, masks) by torch autograd through the oracle's functions, frame by frame, in the library's layout."""
    B = qkv.shape[0]
    x = torch.from_numpy(qkv).clone().requires_grad_()
    fr = ((0, N), (N, N + M))
    masks, parts = [], []
    for side in range(2):
        lo, hi = fr[side]
        slo, shi = fr[1 - side] if cross else fr[side]
        q, kk, v = (x[:, a:b, i].permute(0, 3, 2, 1) for a, b, i in ((lo, hi, 0), (slo, shi, 1), (slo, shi, 2)))
        if k > 0:
            rep = []
            out, _ = O.dynamic_attention(q, kk, v, k, report=rep)
            masks.append(rep[0]['own'].numpy())
        else:
            out, _ = O.attention(q, kk, v)
        parts.append((lo, hi, out.permute(0, 3, 2, 1).reshape(B, hi - lo, 128)))
    msg = torch.cat([p[2] for p in parts], dim=1)
    (msg * torch.from_numpy(dmsg)).sum().backward()
    return msg.detach().numpy(), x.grad.numpy(), tuple(masks) if k > 0 else None


@pytest.fixture(scope='module')
def goldens(golden_dir):
    return {c: R.load_golden(golden_dir, c) for c in CASE_NAMES}


def _args(g):
    B, N, M, cross, k = (int(v) for v in g['meta'])
    return (g['qkv'], N, M, bool(cross)), k


def test_fixture_holds_every_case(goldens):
    for (case, B, N, M, cross, k) in R.CASES:
        g = goldens[case]
        assert tuple(int(v) for v in g['meta']) == (B, N, M, int(cross), k)
        assert g['qkv'].shape == (B, N + M, 3, 4, 32) and g['dqkv'].shape == g['qkv'].shape
        assert g['dmsg'].shape == (B, N + M, 128) and g['msg'].shape == g['dmsg'].shape
        assert all(np.isfinite(g[n]).all() for n in ('qkv', 'dmsg', 'msg', 'dqkv'))
        if k > 0:
            assert all((m.sum(axis=-1) == k).all() for m in g['masks'])
            own, gap = R.topk_masks(g['qkv'], N, M, cross, k)
            assert gap >= 1e-9 and all(np.array_equal(a, b) for a, b in zip(own, g['masks']))
    assert {c[4] for c in R.CASES} == {False, True} and {c[5] for c in R.CASES} == {0, 1, 16}


@pytest.mark.parametrize('case', CASE_NAMES)
def test_backward_restates_the_references_gradients(goldens, case):
    g = goldens[case]
    a, k = _args(g)
    assert np.abs(R.forward(*a, g['masks']) - g['msg']).max() < 1e-13
    frac = R.worst_fraction(R.backward(*a, g['dmsg'], g['masks']), g['dqkv'], R.tolerances(*a, g['dmsg'], g['masks']))
    print(f'{case}: {frac:.2e} of the bound')
    assert frac <= 1.0


@pytest.mark.parametrize('B,N,M,cross,k', [(1, 1, 1, False, 0), (1, 5, 3, True, 2), (2, 17, 17, False, 16), (2, 33, 31, True, 0), (1, 64, 64, False, 63),
                                           (2, 100, 70, True, 70), (1, 130, 97, True, 8), (1, 257, 130, False, 0)])
def test_backward_is_what_autograd_takes_through_the_oracle(B, N, M, cross, k):
    qkv, dmsg = random_inputs(B, N, M, 1000 * N + 10 * M + k)
    msg, want, masks = oracle_backward(qkv, N, M, cross, dmsg, k)
    assert np.abs(R.forward(qkv, N, M, cross, masks) - msg).max() < 1e-12
    frac = R.worst_fraction(R.backward(qkv, N, M, cross, dmsg, masks), want, R.tolerances(qkv, N, M, cross, dmsg, masks))
    print(f'{frac:.2e} of the bound')
    assert frac <= 1.0


@pytest.mark.parametrize('case', ['dyn_self_n48_k16', 'dyn_cross_n40m56_k16', 'dyn_cross_b2_n20m28_k16'])
def test_the_bound_notices_one_swapped_key(goldens, case):
    """One kept key of one row swapped for the row's best key that was not kept: more than 100 x the tolerance away somewhere."""
    g = goldens[case]
    a, k = _args(g)
    qkv, N, M, cross = a
    masks = [m.copy() for m in g['masks']]
    side, b, h, row = 1, 0, 2, 3
    qs, ks = R._sides(N, M, cross)[side]
    S = R.SCALE * (qkv[b, qs, 0, h][row] @ qkv[b, ks, 1, h].T)
    kept = masks[side][b, h, row]
    worst_kept = np.where(kept, S, np.inf).argmin()
    best_other = np.where(kept, -np.inf, S).argmax()
    masks[side][b, h, row, worst_kept], masks[side][b, h, row, best_other] = False, True
    assert masks[side][b, h, row].sum() == k
    frac = R.worst_fraction(R.backward(*a, g['dmsg'], tuple(masks)), g['dqkv'], R.tolerances(*a, g['dmsg'], g['masks']))
    print(f'{case}: a swapped key is {frac:.2e} of the bound')
    assert frac > 100.0


@pytest.mark.parametrize('case', CASE_NAMES)
def test_the_bound_notices_a_relative_error_of_1e_6(goldens, case):
    g = goldens[case]
    a, k = _args(g)
    frac = R.worst_fraction(g['dqkv'] * (1.0 + 1e-6), g['dqkv'], R.tolerances(*a, g['dmsg'], g['masks']))
    assert frac > 1.0, frac


@pytest.mark.parametrize('case', ['dyn_self_n48_k1', 'dyn_cross_n40m56_k1'])
def test_one_kept_key_has_no_gradient_through_the_softmax(goldens, case):
    """k = 1: a one-element softmax is constant - dq is 0 (within the bound), and dk / dv rows of keys no query kept are exactly 0.0."""
    g = goldens[case]
    a, k = _args(g)
    qkv, N, M, cross = a
    tol = R.tolerances(*a, g['dmsg'], g['masks'])
    for d in (R.backward(*a, g['dmsg'], g['masks']), g['dqkv']):
        assert (np.abs(d[:, :, 0]) <= tol[:, :, 0]).all()
        seen = 0
        for (qs, ks), mask in zip(R._sides(N, M, cross), g['masks']):
            unkept = ~mask.any(axis=2)                       # [B, 4, keys]
            rows = np.transpose(d[:, ks, 1:], (0, 3, 1, 2, 4))   # [B, 4, keys, 2, 32]
            assert (rows[unkept] == 0.0).all()
            seen += int(unkept.sum())
        assert seen > 0
    assert np.abs(g['dqkv'][:, :, 2]).max() > 0


def test_tolerance_arithmetic_and_worst_fraction():
    qkv, dmsg = random_inputs(1, 9, 7, 5)
    tol = R.tolerances(qkv, 9, 7, True, dmsg)
    assert tol.shape == qkv.shape and (tol > 0).all()
    # twice the upstream gradient: twice the gradient, twice the bound
    assert np.allclose(R.tolerances(qkv, 9, 7, True, 2 * dmsg), 2 * tol, rtol=1e-12)
    assert np.allclose(R.backward(qkv, 9, 7, True, 2 * dmsg), 2 * R.backward(qkv, 9, 7, True, dmsg), rtol=1e-12, atol=0)
    # the closing products: dv's bound is (P (rel + nq u))^T |G| - at least 4 nq u |dv| (frame 0's rows: read by frame 1's 7 queries)
    Ps = R.probabilities(qkv, 9, 7, True)
    assert (tol[:, :, 2] >= 4 * 7 * R.U * np.abs(R.backward(qkv, 9, 7, True, dmsg))[:, :, 2] * (1 - 1e-12))[:, :9].all() and len(Ps) == 2
    assert R.worst_fraction(np.ones(3), np.ones(3), np.zeros(3)) == 0.0 and R.worst_fraction(np.ones(3), np.zeros(3), np.zeros(3)) == np.inf


# ---- hard logits and selections as inputs: the restatement's own extensions, and the conditions on the inputs of
# ---- tests/test_gpu_attention_grad_hard.py, asserted from the restatement alone ----
@pytest.mark.parametrize('case', CASE_NAMES)
def test_rows_that_keep_a_key_have_the_bits_they_had(goldens, case):
    """The softmax that lets a row keep no key, against the one it replaces (which answers such a row with NaN): the same bits on
    every fixture, and on a fixture with some rows emptied the same bits in the rows that were not."""
    def plain(S, mask):
        if mask is not None:
            S = np.where(mask, S, -np.inf)
        e = np.exp(S - S.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)
    g = goldens[case]
    (qkv, N, M, cross), k = _args(g)
    for side, S in enumerate(R.logits(qkv, N, M, cross)):
        mask = None if g['masks'] is None else g['masks'][side]
        assert np.array_equal(R._softmax(S, mask), plain(S, mask))
        holed = (np.ones(S.shape, dtype=bool) if mask is None else mask).copy()
        holed[:, :, ::3] = False
        with np.errstate(invalid='ignore'):
            want = plain(S, holed)
        got = R._softmax(S, holed)
        assert np.isnan(want[:, :, ::3]).all() and (got[:, :, ::3] == 0.0).all()
        keep = np.ones(S.shape[2], dtype=bool)
        keep[::3] = False
        assert np.array_equal(got[:, :, keep], want[:, :, keep])
    assert np.array_equal(R.backward(qkv, N, M, cross, g['dmsg'], g['masks']),
                          R._backward(qkv, N, M, cross, g['dmsg'], tuple(plain(S, None if g['masks'] is None else g['masks'][i])
                                                                         for i, S in enumerate(R.logits(qkv, N, M, cross)))))


def test_rows_without_a_key_send_nothing():
    B, N, M, cross = 2, 9, 7, True
    qkv, dmsg = random_inputs(B, N, M, 5)
    masks = R.varied_masks(B, N, M, cross, 1)
    empty = [~m.any(axis=-1) for m in masks]
    assert all(e.any() and not e.all() for e in empty)
    msg, d, tol = R.forward(qkv, N, M, cross, masks), R.backward(qkv, N, M, cross, dmsg, masks), R.tolerances(qkv, N, M, cross, dmsg, masks)
    assert all(np.isfinite(x).all() for x in (msg, d, tol))
    for (qs, ks), e in zip(R._sides(N, M, cross), empty):
        assert (np.transpose(msg[:, qs].reshape(B, -1, 4, 32), (0, 2, 1, 3))[e] == 0.0).all()
        assert (np.transpose(d[:, qs, 0], (0, 2, 1, 3))[e] == 0.0).all() and (np.transpose(tol[:, qs, 0], (0, 2, 1, 3))[e] == 0.0).all()
    # emptied rows contribute nothing to dk and dv: the same as those rows' dmsg set to zero
    none = R.constant_masks(B, N, M, cross, False)
    assert not R.backward(qkv, N, M, cross, dmsg, none).any() and not R.tolerances(qkv, N, M, cross, dmsg, none).any()
    assert not R.forward(qkv, N, M, cross, none).any()


@pytest.mark.parametrize('B,N,M,cross', [(1, 5, 3, True), (2, 49, 65, True), (2, 65, 49, False), (1, 33, 96, True), (1, 64, 64, False)])
@pytest.mark.parametrize('pad', [0, 1])
def test_masks_to_words_inverts_topk_sel_to_masks(B, N, M, cross, pad):
    from mdgat_matcher_amd import ops
    masks = R.varied_masks(B, N, M, cross, seed=N + M)
    words = R.masks_to_words(masks, B, N, M, cross, pad)
    W = (max(N, M) + 31) // 32
    assert words.dtype == np.int32 and words.shape == (B, 4, N + M, W)
    back = ops.topk_sel_to_masks(torch.from_numpy(words).reshape(-1), B, N, M, cross)
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(back, masks))
    # the bits that address no key, all of them: the words hold exactly the kept keys plus, with pad = 1, every other bit
    nk = (M, N) if cross else (N, M)
    ones = sum(int(np.unpackbits(words[:, :, rows].view(np.uint8)).sum()) for rows in (slice(0, N), slice(N, N + M)))
    kept = sum(int(m.sum()) for m in masks)
    assert ones == kept + pad * B * 4 * (N * (W * 32 - nk[0]) + M * (W * 32 - nk[1]))
    assert np.array_equal(R.masks_to_words(back, B, N, M, cross, pad), words)


def _hard_case_list():
    out = []
    for (f, B, N, M, cross, k) in R.LOGIT_CASES:
        out += [(f'{f}-{B}x{N}x{M}-{"cross" if cross else "self"}-k{k}-{d}', f, B, N, M, cross, k, None, d) for d in ('plain', 'rows')]
    for (f, B, N, M, cross) in R.SELECTION_CASES:
        out += [(f'{f}-{B}x{N}x{M}-{"cross" if cross else "self"}-{kind}', f, B, N, M, cross, 0, kind, 'plain') for kind in R.SELECTION_KINDS]
    for (f, B, N, M, cross, k) in R.SINGLE_CASES + R.INVARIANCE_CASES:
        out.append((f'{f}-{B}x{N}x{M}-{"cross" if cross else "self"}-k{k}', f, B, N, M, cross, k, None, 'plain'))
    return out


HARD_CASE_LIST = _hard_case_list()


@pytest.mark.parametrize('name,family,B,N,M,cross,k,kind,rows', HARD_CASE_LIST, ids=[c[0] for c in HARD_CASE_LIST])
def test_inputs_of_the_hard_gpu_cases(name, family, B, N, M, cross, k, kind, rows):
    """Conditions on the INPUTS of every case tests/test_gpu_attention_grad_hard.py runs, from the restatement alone: the logits stay
    where the forward is tested (|S| <= 256); no kept probability lies below exp_fast's clamp at exp(-700), where the kernel's 1e-304
    would meet a 0 whose tolerance is 0; a top-k selection is decided by a gap far above a logit's error; the fp64 restatement is
    within HALF the bound of the same formulas in np.longdouble (of the docstring's x 4, a factor 2 is "for the two implementations
    compared": each gets half); and it is within the bound of torch autograd through the oracle wherever the oracle can express the
    selection (every key, or the top k)."""
    qkv, dmsg = R.family_inputs(family, B, N, M, cross)
    if rows == 'rows':
        dmsg = R.alternate_rows(dmsg)
    masks = None
    if kind is not None:
        masks = R.selection_masks(kind, B, N, M, cross)
    elif k > 0:
        masks, gap = R.topk_masks(qkv, N, M, cross, k)
        a_s = max(float(s.max()) for s in R.logits(np.abs(qkv), N, M, cross))
        print(f'top-{k} gap {gap:.2e}, a logit\'s error {32 * R.U * a_s:.2e}')
        assert gap > 1e3 * 32 * R.U * a_s
    reach = []
    for side, S in enumerate(R.logits(qkv, N, M, cross)):
        kept = np.ones(S.shape, dtype=bool) if masks is None else masks[side]
        assert np.abs(S).max() <= 256.0
        Sk = np.where(kept, S, -np.inf)
        mx = Sk.max(axis=-1, keepdims=True)
        rows_kept = np.isfinite(mx[..., 0])
        with np.errstate(invalid='ignore', divide='ignore'):
            lse = mx + np.log(np.exp(Sk - mx).sum(axis=-1, keepdims=True))
        if rows_kept.any():
            reach.append(float((S - lse)[kept].min()))
    print(f'{name}: max|logit| {max(float(np.abs(s).max()) for s in R.logits(qkv, N, M, cross)):.1f}, min(S - lse) over the kept {min(reach, default=0.0):.1f}')
    assert min(reach, default=0.0) > -700.0
    tol = R.tolerances(qkv, N, M, cross, dmsg, masks)
    got, wide = R.backward(qkv, N, M, cross, dmsg, masks), R.backward_longdouble(qkv, N, M, cross, dmsg, masks)
    assert wide.dtype == np.longdouble and np.isfinite(got).all() and np.isfinite(tol).all() and np.isfinite(wide).all()
    assert not ((tol == 0.0) & (wide != 0.0)).any()
    frac = R.worst_fraction((got - wide).astype(np.float64), np.zeros(got.shape), tol)
    print(f'restatement against longdouble (eps {np.finfo(np.longdouble).eps:.2e}): {frac:.2e} of the bound')
    assert frac <= 0.5
    if kind in (None, 'all'):
        msg, want, own = oracle_backward(qkv, N, M, cross, dmsg, k)
        if k > 0:
            assert all(np.array_equal(a, b) for a, b in zip(own, masks))
        assert np.abs(R.forward(qkv, N, M, cross, masks) - msg).max() <= 1e-12 * max(1.0, np.abs(msg).max())
        frac = R.worst_fraction(got, want, tol)
        print(f'restatement against autograd of the oracle: {frac:.2e} of the bound')
        assert frac <= 1.0


@pytest.mark.parametrize('family', R.HARD)
def test_hard_families_move_the_lazy_reference(family):
    """``lazy_trace`` as the witness that a family reaches the path, the way the launch counters are for the form tests: with every key
    kept, each (side, head) of each shape has a wave-block in which a lane that already holds a sum rescales it by a factor below 1;
    ramp, lastkey and gauss at scale 6 rescale by less than 1e-20 somewhere; quarter ends with a row's quarter references at least 50
    apart.  (Under a top-k selection the counts are printed: eight kept keys of 49 often share a block.)"""
    smallest, apart = 1.0, 0.0
    for (f, B, N, M, cross, k) in R.LOGIT_CASES:
        if f != family:
            continue
        qkv, _ = R.family_inputs(f, B, N, M, cross)
        t = R.lazy_trace(qkv, N, M, cross, R.topk_masks(qkv, N, M, cross, k)[0] if k > 0 else None)
        print(f'{f} {B}x{N}x{M} cross={cross} k={k}: rescaling wave-blocks per (side, head) {t["blocks"].tolist()}, '
              f'smallest factor {t["factor"].min():.1e}, quarters up to {t["apart"].max():.1f} apart')
        if k == 0:
            assert (t['blocks'] >= 1).all()
        smallest, apart = min(smallest, float(t['factor'].min())), max(apart, float(t['apart'].max()))
    if family in R.TINY_FACTOR:
        assert smallest < 1e-20
    if family == 'quarter':
        assert apart >= 50.0


def test_lazy_trace_barely_moves_on_the_old_inputs():
    """What the earlier inputs reach, for the record: on 2 x 64 x 64 no wave-block rescales a sum it holds."""
    qkv, _ = random_inputs(2, 64, 64, 64 + 13 * 64)
    t = R.lazy_trace(qkv, 64, 64, False)
    print(t['blocks'].tolist(), t['factor'].min())
    assert t['blocks'].sum() <= 4 and t['factor'].min() > 1e-5


# ---- the attention inside the reference's MultiHeadedAttention.forward: the channel convention and the convolutions around it ----
def test_composition_restates_the_references_multi_headed_attention(golden_dir):
    """The 1x1 convolutions composed in numpy around the restatement, channels permuted from the reference's dim * 4 + head to the
    library's head * 32 + dim: the module's output and all ten recorded gradients."""
    g = R.load_mha(golden_dir)
    a = (g['x'], g['source'], g['w'])
    assert g['k'] == 8 and g['x'].shape == (1, 40, 128) and g['source'].shape == (1, 56, 128)
    assert np.abs(R.mha_forward(*a, g['masks']) - g['out']).max() < 1e-12
    got, tol = R.mha_backward(*a, g['dout'], g['masks']), R.mha_tolerances(*a, g['dout'], g['masks'])
    for name in R.MHA_GRADS:
        frac = R.worst_fraction(got[name], g[name], tol[name])
        print(f'{name}: {frac:.2e} of the bound', end='; ')
        assert frac <= 1.0, (name, frac)
        assert np.abs(g[name]).max() > 0


def test_composition_notices_the_wrong_channel_convention(golden_dir, monkeypatch):
    """Only the permutation is varied - head * 32 + dim taken for the reference's own order, the recorded selection kept: the gradients
    leave the bound by orders of magnitude (with the right permutation the same call is inside it: the test above)."""
    g = R.load_mha(golden_dir)
    a = (g['x'], g['source'], g['w'])
    tol = R.mha_tolerances(*a, g['dout'], g['masks'])
    monkeypatch.setattr(R, 'PERM', np.arange(128))
    got = R.mha_backward(*a, g['dout'], g['masks'])
    assert min(R.worst_fraction(got[name], g[name], tol[name]) for name in ('dx', 'dsource', 'dWq', 'dWk', 'dWv', 'dWm')) > 100.0


def test_generator_check_reproduces_the_committed_files():
    """tools/make_goldens_attention_grad.py --check: the committed fixtures are what the reference computes.  Runs where the reference
    is (tools/make_goldens.py: REF); elsewhere there is nothing to compare against."""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
    sys.path.insert(0, tools)
    try:
        import make_goldens
    finally:
        sys.path.remove(tools)
    if not os.path.isfile(os.path.join(make_goldens.REF, 'models', 'mdgat.py')):
        pytest.skip('the reference is not on this machine')
    r = subprocess.run([sys.executable, os.path.join(tools, 'make_goldens_attention_grad.py'), '--check'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'OK' in r.stdout.splitlines()[-1]
