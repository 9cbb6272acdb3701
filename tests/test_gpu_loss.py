"""The evaluation loss of MDGAT.forward (models/mdgat.py:486-594) on the device: csrc/loss.hip through ops.matching_loss, the module's
forward with config['eval_loss'] / MDGAT_EVAL_LOSS=1, and train.py's validation loop through the integration shim.  Expected values:
the reference's own losses (tests/golden/loss_cases.npz, tools/make_goldens_loss.py) and the fp64 restatement of tests/loss_ref.py."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from loss_ref import GT_PATTERNS, gt_batch, pair_losses

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
METHODS = ('superglue', 'triplet_loss', 'gap_loss')


@pytest.fixture(scope='module')
def g(golden_dir):
    return np.load(os.path.join(golden_dir, 'loss_cases.npz'))


def _methods(g, case):
    return [m for m in METHODS if f'{case}_{m}_loss' in g.files]


def _case(g, case):
    B, n, m, L, S, seed, first_pair = [int(x) for x in g[f'{case}_meta']]
    k = [None if x < 0 else int(x) for x in g[f'{case}_k']]
    return B, n, m, L, S, seed, first_pair, k


def _net(g, case, method, **over):
    from mdgat_matcher_amd import MDGAT, synth
    B, n, m, L, S, seed, first_pair, k = _case(g, case)
    cfg = synth.default_config(L=L, k=k, sinkhorn_iterations=S, loss_method=method, triplet_loss_gamma=float(g[f'{case}_gamma']), **over)
    net = MDGAT(cfg).double()
    net.load_state_dict(synth.make_state_dict(L=L, seed=seed))
    return net.eval().to(DEV)


def _data(g, case, pairs=None):
    from mdgat_matcher_amd import synth
    B, n, m, L, S, seed, first_pair, k = _case(g, case)
    d = {kk: v.to(DEV) for kk, v in synth.make_batch(B, n, m, first_pair=first_pair).items()}
    d['gt_matches0'] = torch.from_numpy(g[f'{case}_gt0']).to(DEV)
    d['gt_matches1'] = torch.from_numpy(g[f'{case}_gt1']).to(DEV)
    if pairs is not None:
        d = {kk: v[pairs] for kk, v in d.items()}
    return d


def _close(got, want, rtol, atol=0.0):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(np.isinf(got), np.isinf(want))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= atol + rtol * np.abs(want[fin])), (got, want)


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('case', ['n64', 'n48m64', 'planted_sub', 'planted_inf'])
def test_matching_loss_matches_restatement(g, case):
    from mdgat_matcher_amd import ops
    Z = g[f'{case}_Z']
    g0, g1 = g[f'{case}_gt0'], g[f'{case}_gt1']
    gamma = float(g[f'{case}_gamma'])
    planted = case.startswith('planted')
    for meth in _methods(g, case):
        t0, t1 = torch.from_numpy(g0).to(DEV), torch.from_numpy(g1).to(DEV)
        got = ops.matching_loss(torch.from_numpy(Z).to(DEV), t0, t1, meth, gamma).cpu().numpy()
        # (the subnormal band of exp: device and host exp / log may round a subnormal differently)
        _close(got, pair_losses(Z, g0, g1, meth, gamma), 1e-6 if planted else 1e-12)
        Z32 = Z.astype(np.float32)
        got32 = ops.matching_loss(torch.from_numpy(Z32).to(DEV), t0, t1, meth, gamma).cpu().numpy()
        _close(got32, pair_losses(Z32.astype(np.float64), g0, g1, meth, gamma), 1e-6 if planted else 1e-10)
        # the gts are not touched, and a pair's value does not depend on the batch it travels in
        assert np.array_equal(t0.cpu().numpy(), g0) and np.array_equal(t1.cpu().numpy(), g1)
        alone = ops.matching_loss(torch.from_numpy(Z[-1:]).to(DEV), t0[-1:], t1[-1:], meth, gamma).cpu().numpy()
        assert np.array_equal(alone, got[-1:], equal_nan=True)
    if case == 'planted_inf':
        assert np.isinf(got).all()


def test_matching_loss_refuses_bad_input(g):
    from mdgat_matcher_amd import ops
    Z = torch.from_numpy(g['n48m64_Z']).to(DEV)
    g0, g1 = torch.from_numpy(g['n48m64_gt0']).to(DEV), torch.from_numpy(g['n48m64_gt1']).to(DEV)
    with pytest.raises(ValueError):
        ops.matching_loss(Z, g0, g1, 'triplet_loss')
    with pytest.raises(ValueError):
        ops.matching_loss(Z, g0[:, :-1], g1, 'gap_loss')


# ------------------------------------------------------------------------------------------------ the kernel at the shapes it runs
def _rel(got, want):
    """the largest |got - want| / |want| over the finite values (0 where there are none; inf where want is 0 and got is not)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want) & np.isfinite(got)
    err, den = np.abs(got[fin] - want[fin]), np.abs(want[fin])
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.max(np.where(err == 0, 0.0, err / den), initial=0.0))


def _lp_Z(B, n, m, seed):
    """log-probabilities as the module's Z: ops.sinkhorn_f64 of random scores, fp64 on the device (a spread of +-15 and a bin score of
    0: the dustbin does not outweigh every inner entry, and every gt pattern gives every loss a nonzero value up to 2048 keypoints)"""
    from mdgat_matcher_amd import ops
    gen = torch.Generator().manual_seed(seed)
    s = (torch.rand(B, n, m, generator=gen, dtype=torch.float64) * 2 - 1) * 15
    return ops.sinkhorn_f64(s.to(DEV), 0.0, 20)


def _check_methods(Z, g0, g1, methods, rtol64=1e-11, rtol32=1e-10):
    """ops.matching_loss on Z (fp64, on the device) and on its fp32 rounding against pair_losses of the same values."""
    from mdgat_matcher_amd import ops
    t0, t1 = torch.from_numpy(g0).to(DEV), torch.from_numpy(g1).to(DEV)
    Z32 = Z.to(torch.float32)
    for meth in methods:
        for Zd, rtol in ((Z, rtol64), (Z32, rtol32)):
            got = ops.matching_loss(Zd, t0, t1, meth, 0.5).cpu().numpy()
            want = pair_losses(Zd.cpu().double().numpy(), g0, g1, meth, 0.5)
            assert np.all(want != 0), (meth, want)          # (a pattern whose loss is 0 would test little)
            print(f'{meth} {str(Zd.dtype)[6:]} {_rel(got, want):.1e}', end='; ')
            _close(got, want, rtol)
    print()


# one pair per gt pattern of loss_ref.gt_pattern: P's order across the 256-column chunks of loss_gap_order_kernel, a row with hundreds
# of positives for nth_other, every positive in the dustbin row, explicit dustbin indices (superglue counts only a literal -1)
@pytest.mark.parametrize('n', [255, 256, 257, 511, 2048])
def test_matching_loss_square_frames(n):
    g0, g1 = gt_batch(GT_PATTERNS, n, n, seed=n)
    _check_methods(_lp_Z(len(GT_PATTERNS), n, n, seed=n), g0, g1, METHODS)


# gap takes ragged pairs: N > M, N < M, one row, one column, and the tile kernel's 16-row tiles full (15 + the dustbin row) and with a
# second tile of the dustbin row alone
@pytest.mark.parametrize('n,m', [(700, 300), (300, 700), (1, 2048), (2048, 1), (15, 600), (16, 600)])
def test_gap_loss_ragged_frames(n, m):
    g0, g1 = gt_batch(GT_PATTERNS, n, m, seed=n + m)
    _check_methods(_lp_Z(len(GT_PATTERNS), n, m, seed=n + m), g0, g1, ('gap_loss',))


def test_matching_loss_planted_beyond_the_first_256_columns():
    """Entries in exp's subnormal band and below its underflow in columns >= 256 (the second round of the tile kernel's column loop
    and of gap's column pass): positives and negatives of rows and columns, and the dustbin row, as make_goldens_loss.plant does."""
    from mdgat_matcher_amd import ops
    n = m = 511
    g0, g1 = gt_batch(GT_PATTERNS, n, m, seed=3)
    Z = _lp_Z(len(GT_PATTERNS), n, m, seed=3).cpu().numpy()
    rs = np.random.RandomState(3)
    for b in range(len(GT_PATTERNS)):
        p0, p1 = np.where(g0[b] == -1, m, g0[b]), np.where(g1[b] == -1, n, g1[b])
        for i in range(0, n, 5):
            if p0[i] >= 256:
                Z[b, i, p0[i]] = rs.uniform(-740.0, -709.0)
            Z[b, i, 256 + i % (m + 1 - 256)] = rs.uniform(-740.0, -709.0)
        for j in range(257, m, 7):
            Z[b, p1[j], j] = rs.uniform(-740.0, -709.0)
            Z[b, (p1[j] + 3) % (n + 1), j] = rs.uniform(-760.0, -745.2)
        Z[b, n, 257::9] = rs.uniform(-740.0, -709.0, Z[b, n, 257::9].shape[0])
    assert ((Z[:, :, 256:] > -740) & (Z[:, :, 256:] < -709)).any() and (Z[:, :, 256:] < -745.2).any()
    t0, t1 = torch.from_numpy(g0).to(DEV), torch.from_numpy(g1).to(DEV)
    finite = 0
    for z in (Z, Z.astype(np.float32)):
        for meth in METHODS:
            got = ops.matching_loss(torch.from_numpy(z).to(DEV), t0, t1, meth, 0.5).cpu().numpy()
            want = pair_losses(z.astype(np.float64), g0, g1, meth, 0.5)
            print(f'{meth} {z.dtype} {_rel(got, want):.1e}', end='; ')
            # (the subnormal band of exp: device and host exp / log may round a subnormal differently)
            _close(got, want, 1e-6)
            finite += int(np.isfinite(want).sum())
    print()
    assert finite > 0


def test_matching_loss_pairs_are_bitwise_batch_independent():
    """Six pairs of 512, each with another gt pattern: every pair alone gives its row of the batch, every method, fp64 and fp32 Z."""
    from mdgat_matcher_amd import ops
    g0, g1 = gt_batch(GT_PATTERNS + ('partial',), 512, 512, seed=6)
    t0, t1 = torch.from_numpy(g0).to(DEV), torch.from_numpy(g1).to(DEV)
    Z = _lp_Z(6, 512, 512, seed=6)
    worst = 0.0
    for Zd in (Z, Z.to(torch.float32)):
        for meth in METHODS:
            batch = ops.matching_loss(Zd, t0, t1, meth, 0.5)
            for b in range(6):
                alone = ops.matching_loss(Zd[b:b + 1], t0[b:b + 1], t1[b:b + 1], meth, 0.5)
                worst = max(worst, (alone - batch[b:b + 1]).abs().max().item())
                assert torch.equal(alone, batch[b:b + 1]), (meth, Zd.dtype, b)
    print(f'max |alone - batch| = {worst:.1e}')


def test_gap_loss_at_its_row_limit():
    """N = 15000 (loss_gap_order_kernel's N + 2 row counters in LDS: 60 KB) is computed; 15001 is refused; the next call is right."""
    from mdgat_matcher_amd import ops
    n, m = 15000, 3
    rs = np.random.RandomState(15000)
    Z = np.log(rs.uniform(1e-6, 1.0, (1, n + 1, m + 1))) - 6.0
    g0, g1 = gt_batch(['explicit_dustbin'], n, m, seed=15000)
    want = pair_losses(Z, g0, g1, 'gap_loss', 0.5)
    args = (torch.from_numpy(Z).to(DEV), torch.from_numpy(g0).to(DEV), torch.from_numpy(g1).to(DEV), 'gap_loss', 0.5)
    got = ops.matching_loss(*args).cpu().numpy()
    print(f'N=15000: {_rel(got, want):.1e}')
    _close(got, want, 1e-11)
    with pytest.raises(RuntimeError, match='15000'):
        ops.matching_loss(torch.zeros(1, n + 2, m + 1, dtype=torch.float64, device=DEV), torch.zeros(1, n + 1, dtype=torch.int64, device=DEV),
                          torch.zeros(1, m, dtype=torch.int64, device=DEV), 'gap_loss', 0.5)
    again = ops.matching_loss(*args).cpu().numpy()
    assert np.array_equal(again, got)


# ------------------------------------------------------------------------------------------------ the module, exact mode
@pytest.mark.parametrize('case', ['n64', 'n48m64', 'b8n256'])
def test_exact_mode_loss_is_the_references(g, case):
    for meth in _methods(g, case):
        net = _net(g, case, meth, eval_loss=True)
        assert net.exact()
        data = _data(g, case)
        with torch.no_grad():
            out = net(data)
        want = g[f'{case}_{meth}_loss']
        assert out['loss'].dtype == torch.float64 and tuple(out['loss'].shape) == want.shape
        _close(out['loss'].cpu().numpy(), want, 1e-9, 1e-12)
        # the reference's in-place rewrite of the caller's gts (none for superglue)
        np.testing.assert_array_equal(data['gt_matches0'].cpu().numpy(), g[f'{case}_{meth}_gt0_after'])
        np.testing.assert_array_equal(data['gt_matches1'].cpu().numpy(), g[f'{case}_{meth}_gt1_after'])
        assert data['gt_matches0'].dtype == torch.int16
        # everything else is the forward without the loss, bit for bit
        off = _net(g, case, meth)
        with torch.no_grad():
            ref = off(_data(g, case))
        for key in ('matches0', 'matches1', 'matching_scores0', 'matching_scores1'):
            assert torch.equal(out[key], ref[key]), key
        assert float(ref['loss']) == 0.0


def test_exact_mode_Z_unchanged_by_the_loss(g):
    from mdgat_matcher_amd import _lib
    net = _net(g, 'n64', 'gap_loss', eval_loss=True)
    d = _data(g, 'n64')
    args = (d['keypoints0'], d['scores0'], d['descriptors0'], d['keypoints1'], d['scores1'], d['descriptors1'])
    req = net._loss_request(d, d['keypoints0'], d['keypoints1'])
    with torch.no_grad():
        on = net._run(*args, want_Z=True, loss=req)
        off = net._run(*args, want_Z=True)
    torch.cuda.synchronize()
    for a, b in zip(on, off):
        assert torch.equal(a, b)
    np.testing.assert_allclose(req['loss'].cpu().numpy(), g['n64_gap_loss_loss'], rtol=1e-9)
    assert req['method'] == _lib.LOSS_GAP


# ------------------------------------------------------------------------------------------------ the fp32-class path
@pytest.mark.parametrize('case', ['n64', 'b8n256'])
def test_fp32_path_loss(g, case):
    from mdgat_matcher_amd import ops
    for meth in _methods(g, case):
        net = _net(g, case, meth, eval_loss=True, arithmetic='fp32')
        assert not net.exact()
        d = _data(g, case)
        args = (d['keypoints0'], d['scores0'], d['descriptors0'], d['keypoints1'], d['scores1'], d['descriptors1'])
        req = net._loss_request(d, d['keypoints0'], d['keypoints1'])
        with torch.no_grad():
            Z = net._run(*args, want_Z=True, loss=req)[4]
            own = ops.matching_loss(Z, d['gt_matches0'], d['gt_matches1'], meth, float(g[f'{case}_gamma']))
        _close(req['loss'].cpu().numpy(), own.cpu().numpy(), 1e-10)
        with torch.no_grad():
            out = net(_data(g, case))
        want = g[f'{case}_{meth}_loss']
        _close(out['loss'].cpu().numpy(), want, 0.0, 2e-3)


# ------------------------------------------------------------------------------------------------ determinism
_DET_SCRIPT = r'''
import sys, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_gpu_loss as T
import numpy as np
g = np.load({golden!r})
print(repr(T._batch64_losses(g).tolist()))
'''


def _batch64_losses(g):
    """gap losses of 64 pairs of 64 keypoints (the n64 pairs and gts repeated), exact mode, split-key attention (batch-independent)."""
    from mdgat_matcher_amd import _lib
    lib = _lib.load()
    prev = lib.mdgat_set_f64_attention_form(0)
    try:
        net = _net(g, 'n64', 'gap_loss', eval_loss=True)
        d = _data(g, 'n64', pairs=[i % 2 for i in range(64)])
        with torch.no_grad():
            return net(d)['loss'].cpu()
    finally:
        lib.mdgat_set_f64_attention_form(prev)


def test_loss_is_bitwise_independent_of_batch_lanes_and_slices(g, golden_dir):
    from mdgat_matcher_amd import _lib
    lib = _lib.load()
    prev = lib.mdgat_set_f64_attention_form(0)
    try:
        net = _net(g, 'n64', 'gap_loss', eval_loss=True)
        with torch.no_grad():
            alone = net(_data(g, 'n64', pairs=[1]))['loss'].cpu()
        for lanes in (1, 2):
            net.set_lanes(lanes)
            with torch.no_grad():
                batch = net(_data(g, 'n64', pairs=[i % 2 for i in range(64)]))['loss'].cpu()
            assert torch.equal(batch[1::2], alone.expand(32)), lanes
    finally:
        lib.mdgat_set_f64_attention_form(prev)
    # MDGAT_FORWARD_SLICE_POINTS is read once per process: slices of 8 pairs in a fresh child
    env = dict(os.environ, MDGAT_FORWARD_SLICE_POINTS='1024')
    code = _DET_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'), golden=os.path.join(golden_dir, 'loss_cases.npz'))
    res = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    sliced = torch.tensor(eval(res.stdout.strip().splitlines()[-1]), dtype=torch.float64)
    assert torch.equal(sliced[1::2], alone.expand(32))


# ------------------------------------------------------------------------------------------------ the largest Z
def test_exact_mode_two_pairs_of_2048():
    """The streaming fp64 Sinkhorn writes the fp64 Z the loss reads (frames beyond 575 keypoints)."""
    from mdgat_matcher_amd import MDGAT, ops, synth
    L = 9
    cfg = synth.default_config(L=L, sinkhorn_iterations=100, loss_method='gap_loss', eval_loss=True)
    net = MDGAT(cfg).double()
    net.load_state_dict(synth.make_state_dict(L=L, seed=0))
    net = net.eval().to(DEV)
    assert net.exact()
    d = {kk: v.to(DEV) for kk, v in synth.make_batch(2, 2048, 2048, first_pair=60).items()}
    gen = torch.Generator().manual_seed(5)
    d['gt_matches0'] = torch.randint(-1, 2048, (2, 2048), generator=gen, dtype=torch.int16).to(DEV)
    d['gt_matches1'] = torch.randint(-1, 2048, (2, 2048), generator=gen, dtype=torch.int16).to(DEV)
    args = (d['keypoints0'], d['scores0'], d['descriptors0'], d['keypoints1'], d['scores1'], d['descriptors1'])
    req = net._loss_request(d, d['keypoints0'], d['keypoints1'])
    with torch.no_grad():
        m0, m1, s0, s1, Z = net._run(*args, want_Z=True, loss=req)
        off = net._run(*args, want_Z=True)
        z32 = ops.matching_loss(Z, d['gt_matches0'], d['gt_matches1'], 'gap_loss', 0.5)
    torch.cuda.synchronize()
    assert torch.equal(m0, off[0]) and torch.equal(m1, off[1]) and torch.equal(Z, off[4])
    loss = req['loss'].cpu()
    assert torch.isfinite(loss).all() and int(req['bad'].item()) == 0
    # the fp32 rounding of the same Z: within what rounding Z to fp32 moves the loss
    np.testing.assert_allclose(loss.numpy(), z32.cpu().numpy(), rtol=1e-4)
    # and the kernel on that Z against the restatement: the rounded Z's loss exactly, the forward's own within the rounding
    want = pair_losses(Z.cpu().double().numpy(), d['gt_matches0'].cpu().numpy(), d['gt_matches1'].cpu().numpy(), 'gap_loss', 0.5)
    print(f'Z {Z.dtype}: {_rel(z32.cpu().numpy(), want):.1e} against the restatement')
    _close(z32.cpu().numpy(), want, 1e-10)
    np.testing.assert_allclose(loss.numpy(), want, rtol=1e-4)


# ------------------------------------------------------------------------------------------------ contract
def test_contract(g, monkeypatch):
    from mdgat_matcher_amd import MDGAT, synth
    # shapes and dtypes: gap [B], the others 0-d, in the module's dtype (float32 module: the fp32-class path)
    for meth in METHODS:
        B, n, m, L, S, seed, first_pair, k = _case(g, 'n64')
        net = MDGAT(synth.default_config(L=L, k=k, sinkhorn_iterations=S, loss_method=meth, eval_loss=True))
        net.load_state_dict(synth.make_state_dict(L=L, seed=seed))
        net = net.eval().to(DEV)
        d = {kk: (v.float() if v.is_floating_point() else v) for kk, v in _data(g, 'n64').items()}
        with torch.no_grad():
            loss = net(d)['loss']
        assert loss.dtype == torch.float32
        assert tuple(loss.shape) == ((B,) if meth == 'gap_loss' else ())
    # n != m: triplet and superglue refuse before any launch
    for meth in ('triplet_loss', 'superglue'):
        with pytest.raises(ValueError):
            _net(g, 'n48m64', meth, eval_loss=True)(_data(g, 'n48m64'))
    # the gts are required
    d = _data(g, 'n64')
    del d['gt_matches1']
    with pytest.raises(KeyError):
        _net(g, 'n64', 'gap_loss', eval_loss=True)(d)
    # an index out of range: IndexError, and the device goes on working
    net = _net(g, 'n64', 'triplet_loss', eval_loss=True)
    d = _data(g, 'n64')
    d['gt_matches0'][1, 7] = 65
    with torch.no_grad():
        with pytest.raises(IndexError):
            net(d)
        out = net(_data(g, 'n64'))
    np.testing.assert_allclose(float(out['loss']), float(g['n64_triplet_loss_loss']), rtol=1e-9)
    # off unless asked for: no key and no environment variable
    monkeypatch.delenv('MDGAT_EVAL_LOSS', raising=False)
    with torch.no_grad():
        out = _net(g, 'n64', 'triplet_loss')(_data(g, 'n64'))
    assert float(out['loss']) == 0.0 and out['loss'].dim() == 0


# ------------------------------------------------------------------------------------------------ train.py's validation loop
@pytest.fixture()
def models_mdgat():
    shim = os.path.join(ROOT, 'integration')
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == 'models' or k.startswith('models.')}
    sys.path.insert(0, shim)
    try:
        yield importlib.import_module('models.mdgat')
    finally:
        sys.path.remove(shim)
        for k in [k for k in sys.modules if k == 'models' or k.startswith('models.')]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_train_py_validation_loop_unchanged(g, models_mdgat, monkeypatch):
    """train.py:188-196, 222 and 263-285 as they stand, MDGAT_EVAL_LOSS=1 in the environment: four validation batches of two pairs
    (the b8n256 pairs); the mean validation loss is the reference's loss over the eight pairs."""
    from torch.autograd import Variable
    from mdgat_matcher_amd import synth
    monkeypatch.setenv('MDGAT_EVAL_LOSS', '1')
    B, n, m, L, S, seed, first_pair, k = _case(g, 'b8n256')
    config = {'net': synth.default_config(L=L, k=k, sinkhorn_iterations=S, loss_method='triplet_loss')}
    assert 'eval_loss' not in config['net']
    net = models_mdgat.MDGAT(config.get('net', {}))                        # train.py:188
    net = torch.nn.DataParallel(net)                                         # train.py:196
    net.to(torch.device(DEV))
    net.double().train()                                                     # train.py:222
    # the fp64 weights training leaves in the module (loaded before .double() they would be rounded to fp32)
    net.module.load_state_dict(synth.make_state_dict(L=L, seed=seed))
    full = _data(g, 'b8n256')
    val_loader = [{kk: v[i:i + 2].cpu() for kk, v in full.items()} for i in range(0, B, 2)]
    with torch.no_grad():
        mean_val_loss = []
        for i, pred in enumerate(val_loader):                                # train.py:267-285
            net.eval()
            for kk in pred:
                if kk != 'idx0' and kk != 'idx1' and kk != 'sequence':
                    if type(pred[kk]) == torch.Tensor:
                        pred[kk] = Variable(pred[kk].cuda().detach())
                    else:
                        pred[kk] = Variable(torch.stack(pred[kk]).cuda().detach())
            data = net(pred)
            pred = {**pred, **data}
            Loss = pred['loss']
            mean_val_loss.append(Loss)
        mean_val_loss = torch.mean(torch.stack(mean_val_loss)).item()
    assert abs(mean_val_loss - float(g['b8n256_triplet_loss_loss'])) <= 1e-9 * abs(float(g['b8n256_triplet_loss_loss']))
