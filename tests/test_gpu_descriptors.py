"""The FPFH_gloabal and FPFH_only descriptor encoders on the device, against the unmodified reference's recorded outputs
(tests/golden/desc_*.npz, tools/make_goldens_descriptors.py): the exact-mode forward (encoder tap, Z, matches, scores), the float32
module (parity_util's bounds), ragged batches, ``ops.frame_max_f64`` and ``MDGAT.training_forward``; and one digest of what the default
descriptor computed before these encoders existed.

Tolerances.  The encoder tap: 2e-6, what tests/test_gpu_f64.py holds the 'FPFH' encoders' tap to (the tap is rounded to float32).  Z:
the literal 1e-4.  Matching scores: extract_ref.SCORE_TOL.  ``training_forward``: 32 x the error stored with every quantity."""
import functools

import numpy as np
import pytest
import torch

import descriptor_digest
import descriptor_ref as DR
import extract_ref as E
import parity_util as P
import train_ref as T
from conftest import GOLDEN
from mdgat_matcher_amd import MDGAT, _lib, ops, synth

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ENC_TOL = 2e-6
INPUTS = ('keypoints0', 'scores0', 'descriptors0', 'keypoints1', 'scores1', 'descriptors1')


@functools.lru_cache(maxsize=None)
def _eval(descriptor):
    return dict(np.load(T.golden_path(GOLDEN, DR.eval_file(descriptor))))


@functools.lru_cache(maxsize=None)
def _ragged():
    return dict(np.load(T.golden_path(GOLDEN, DR.RAGGED_FILE)))


def _net(descriptor, dtype=torch.float64, training=False, method='gap_loss', **over):
    net = MDGAT(DR.config(method, descriptor, **over)).to(dtype)
    net.load_state_dict(DR.initial_state(descriptor))
    return net.to(dtype).to(DEV).train(training)


def _dev(g, prefix='in:'):
    return {k[len(prefix):]: torch.from_numpy(g[k].copy()).to(DEV) for k in g if k.startswith(prefix)}


def _run_with_taps(net, d, sel=False):
    B, n, m = d['keypoints0'].shape[0], d['keypoints0'].shape[1], d['keypoints1'].shape[1]
    taps = {'x_enc': torch.empty(B, n + m, 128, device=DEV)}
    if sel:
        taps['topk_sel'] = torch.zeros(len(net._topk_schedule()) * ops.topk_sel_words(B, n, m), dtype=torch.int32, device=DEV)
    out = net._run(*[d[k] for k in INPUTS], want_Z=True, taps=taps)
    torch.cuda.synchronize()
    net.check(DEV)
    return out, taps


def _against_fixture(tag, out, g, prefix=''):
    """matches identical, Z within the literal 1e-4, scores at extract's bound"""
    m0, m1, s0, s1, Z = out
    ez = float(np.abs(Z.cpu().double().numpy() - g[prefix + 'Z']).max())
    es = max(float(np.abs(s.cpu().double().numpy() - g[prefix + f'mscores{f}']).max()) for f, s in enumerate((s0, s1)))
    print(f'{tag}: max|Z - reference| {ez:.3e}, scores {es:.3e}')
    assert np.array_equal(m0.cpu().numpy(), g[prefix + 'matches0']) and np.array_equal(m1.cpu().numpy(), g[prefix + 'matches1'])
    assert ez < P.Z_TOL and es <= E.SCORE_TOL, (ez, es)


# ---- the exact-mode forward ----
@pytest.mark.parametrize('descriptor', DR.DESCRIPTORS)
def test_exact_forward_reproduces_the_reference(descriptor):
    g = _eval(descriptor)
    net, d = _net(descriptor), _dev(g)
    assert net.exact()
    out, taps = _run_with_taps(net, d)
    n = d['keypoints0'].shape[1]
    enc = taps['x_enc'].cpu().double().numpy()
    ee = max(float(np.abs(enc[:, :n] - g['enc0']).max()), float(np.abs(enc[:, n:] - g['enc1']).max()))
    print(f'{descriptor}: encoder tap: max|x_enc - reference| {ee:.3e}')
    assert ee < ENC_TOL
    _against_fixture(descriptor, out, g)
    # the dict API, match and match_frames give the same bits
    data = {k: v.clone() for k, v in d.items()}
    with torch.no_grad():
        o = net(data)
        rec = [torch.cat([d[f'keypoints{f}'], d[f'scores{f}'][..., None], d[f'descriptors{f}']], dim=-1) for f in (0, 1)]
        fr = net.match_frames(rec[0], rec[1], normalize=False, return_scores=True)
    assert torch.equal(o['matches0'], out[0]) and torch.equal(o['matches1'], out[1]) and torch.equal(o['matching_scores0'], out[2].double())
    # (match_frames reads float32 records: the reference's loader arithmetic, not the fixture's float64 inputs - matches only)
    assert torch.equal(fr[0], out[0]) and torch.equal(fr[1], out[1])
    # ... and with the one-product-per-launch layers
    lib = _lib.load()
    prev = lib.mdgat_set_f64_layer_fusion(0)
    try:
        plain, ptaps = _run_with_taps(net, d)
    finally:
        lib.mdgat_set_f64_layer_fusion(prev)
    assert torch.equal(ptaps['x_enc'], taps['x_enc']) and all(torch.equal(a, b) for a, b in zip(plain, out))


def test_evaluate_runs_for_both_descriptors():
    for descriptor in DR.DESCRIPTORS:
        g = _eval(descriptor)
        net, d = _net(descriptor), _dev(g)
        with torch.no_grad():
            ev = net.evaluate({k: v.clone() for k, v in d.items()})
        assert np.array_equal(ev['matches0'].cpu().numpy(), g['matches0']) and tuple(ev['metrics'].shape) == (2, len(_lib.EVAL_COLUMNS))


def test_load_packed_carries_the_pooled_encoder():
    """A rank that receives its weights by broadcast (shard.broadcast_weights) installs the blob, the fp64 blob and the pooled encoder."""
    from mdgat_matcher_amd import pack
    g = _eval('FPFH_gloabal')
    src, d = _net('FPFH_gloabal'), _dev(g)
    dst = MDGAT(DR.config('gap_loss', 'FPFH_gloabal')).double().to(DEV).eval()          # its own parameters: random
    blob = torch.from_numpy(src.packed_weights()).to(DEV)
    blob64 = torch.from_numpy(src.packed_weights(np.float64)).to(DEV)
    with pytest.raises(ValueError):
        dst.load_packed(blob, blob64)
    dst.load_packed(blob, blob64, torch.from_numpy(pack.pack_pooled_encoder(src.state_dict())).to(DEV))
    args = (d['keypoints0'], d['descriptors0'], d['keypoints1'], d['descriptors1'], d['scores0'], d['scores1'])
    with torch.no_grad():
        a, b = src.match(*args, return_scores=True), dst.match(*args, return_scores=True)
    src.check(DEV), dst.check(DEV)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- the float32 module: fp64 encoders, the fp32-class path behind them ----
def _selection_rows(net, d):
    """the kept keys of every dynamic layer as boolean masks (parity_util.hip_forward_with_selection)"""
    return P.hip_forward_with_selection(net, d)


@pytest.mark.parametrize('descriptor', DR.DESCRIPTORS)
def test_float32_module_is_within_the_parity_bounds(descriptor):
    g = _eval(descriptor)
    d = _dev(g)
    net32, net64 = _net(descriptor, torch.float32), _net(descriptor)
    assert not net32.exact() and net32._handle_f64() == (descriptor == 'FPFH_gloabal')
    d32 = {k: (v.float() if v.is_floating_point() else v) for k, v in d.items()}
    out, forced = _selection_rows(net32, d32)
    net32.check(DEV)
    _, exact = _selection_rows(net64, d)
    # rows of a pair whose selection differs from the exact mode's (which is the reference's): the literal bar applies to the others
    flips = torch.zeros(out[4].shape[0], dtype=torch.int64)
    for i in forced:
        for a, b in zip(forced[i], exact[i]):
            flips += (a ^ b).any(-1).flatten(1).sum(1)
    res = {'out': out, 'flips_per_pair': flips}
    P.assert_plain(res, g['Z'], g['matches0'], g['matches1'], g['mscores0'], g['mscores1'], tag=f'{descriptor} float32 module')
    with torch.no_grad():
        o = net32({k: v.clone() for k, v in d32.items()})
    assert o['matching_scores0'].dtype == torch.float32 and np.array_equal(o['matches0'].cpu().numpy(), g['matches0'])
    if descriptor == 'FPFH_gloabal':
        # arithmetic='fp32' on a float64 module: the same path, the same bits
        pinned = _net(descriptor, arithmetic='fp32')
        assert not pinned.exact()
        with torch.no_grad():
            m = pinned.match(d['keypoints0'], d['descriptors0'], d['keypoints1'], d['descriptors1'], d['scores0'], d['scores1'], return_scores=True)
        pinned.check(DEV)
        assert torch.equal(m[0], out[0]) and torch.equal(m[1], out[1])
        assert float((m[4] - out[4]).abs().max()) < P.Z_TOL        # (float64 inputs instead of their float32 roundings)


@pytest.mark.parametrize('dtype', (torch.float64, torch.float32))
def test_fpfh_only_ignores_the_keypoint_values(dtype):
    g = _eval('FPFH_only')
    net = _net('FPFH_only', dtype)
    d = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in _dev(g).items()}
    zero = {k: (torch.zeros_like(v) if k.startswith('keypoints') else v) for k, v in d.items() if not k.startswith('scores')}
    sign = torch.where(torch.rand_like(d['keypoints0']) < 0.5, -1.0, 1.0)
    huge = dict(zero, keypoints0=1e6 * sign, keypoints1=torch.full_like(d['keypoints1'], -1e6))
    assert 'scores0' not in zero and 'scores1' not in huge
    with torch.no_grad():
        a, b, c = net(dict(zero)), net(dict(huge)), net({k: v.clone() for k, v in d.items()})
        za = net.match(zero['keypoints0'], zero['descriptors0'], zero['keypoints1'], zero['descriptors1'], return_scores=True)[4]
        zb = net.match(huge['keypoints0'], huge['descriptors0'], huge['keypoints1'], huge['descriptors1'], return_scores=True)[4]
    net.check(DEV)
    for k in ('matches0', 'matches1', 'matching_scores0', 'matching_scores1'):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    assert torch.equal(za, zb) and np.array_equal(a['matches0'].cpu().numpy(), g['matches0'])


# ---- ragged batches of the pooled encoder ----
@pytest.fixture
def pinned_attention_form():
    lib = _lib.load()
    prev = lib.mdgat_set_f64_attention_form(0)        # a pair's bits then do not depend on the batch it travels in (tests/test_gpu_ragged_forward.py)
    yield
    lib.mdgat_set_f64_attention_form(prev)


def _same(a, b, what):
    for k in ('matches0', 'matches1', 'matching_scores0', 'matching_scores1'):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)


def test_forward_ragged_gloabal_equals_every_pair_alone_and_the_reference(pinned_attention_form):
    g = _ragged()
    net = _net('FPFH_gloabal', k=[])
    pairs = [_dev(g, f'p{i}:in:') for i in range(len(DR.RAGGED_COUNTS))]
    assert [(p['keypoints0'].shape[1], p['keypoints1'].shape[1]) for p in pairs] == list(DR.RAGGED_COUNTS)
    assert int(g['visible'][g['visible'] >= 0].min()) >= 8          # a pool over the padded rows would change at least 8 channels per short frame
    with torch.no_grad():
        got = net.forward_ragged(pairs, return_Z=True)
        for i, p in enumerate(pairs):
            _same(got[i], net(p), i)
            Z = net.match(p['keypoints0'], p['descriptors0'], p['keypoints1'], p['descriptors1'], p['scores0'], p['scores1'], return_scores=True)[4]
            assert torch.equal(got[i]['Z'], Z), i
            o = got[i]
            _against_fixture(f'ragged pair {i}', (o['matches0'], o['matches1'], o['matching_scores0'], o['matching_scores1'], o['Z']), g, f'p{i}:')
        ev = net.evaluate_ragged([dict(p) for p in pairs])
        for i, p in enumerate(pairs):
            alone = net.evaluate(dict(p))['metrics'][0]          # (ratios without a denominator are NaN in both)
            assert np.array_equal(ev['metrics'][i].cpu().numpy(), alone.cpu().numpy(), equal_nan=True), i
    net.check(DEV)


def test_forward_ragged_gloabal_over_several_row_tiles(pinned_attention_form):
    """300 keypoints: every thread of the pool walks 38 rows, the last phases one fewer."""
    net = _net('FPFH_gloabal', k=[])
    data = synth.make_batch(2, 300, 300, first_pair=70, device=DEV)
    pairs = [{k: v[b:b + 1] for k, v in data.items()} for b in range(2)]
    with torch.no_grad():
        got = net.forward_ragged(pairs, return_Z=True)
        for b, p in enumerate(pairs):
            _same(got[b], net(p), b)
            Z = net.match(p['keypoints0'], p['descriptors0'], p['keypoints1'], p['descriptors1'], p['scores0'], p['scores1'], return_scores=True)[4]
            assert torch.equal(got[b]['Z'], Z), b
    net.check(DEV)


def test_forward_ragged_fpfh_only_equals_every_pair_alone(pinned_attention_form):
    net = _net('FPFH_only', k=[])
    pairs = [{k: v.to(DEV) for k, v in synth.make_batch(1, n, m, first_pair=80 + i).items()} for i, (n, m) in enumerate(((7, 12), (33, 20), (12, 33)))]
    with torch.no_grad():
        got = net.forward_ragged(pairs, return_Z=True)
        for i, p in enumerate(pairs):
            _same(got[i], net(p), i)
            # the keypoints' values reach nothing
            moved = dict(p, keypoints0=p['keypoints0'] * 3.0 + 1.0, keypoints1=-p['keypoints1'])
            Z = net.match(moved['keypoints0'], p['descriptors0'], moved['keypoints1'], p['descriptors1'], return_scores=True)[4]
            assert torch.equal(got[i]['Z'], Z), i
    net.check(DEV)


# ---- ops.frame_max_f64 ----
@pytest.mark.parametrize('B', (1, 3))
@pytest.mark.parametrize('n', (1, 20, 64, 65, 300))
def test_frame_max_f64(B, n):
    gen = torch.Generator().manual_seed(100 * n + B)
    e = (torch.randn(B, n, 128, generator=gen, dtype=torch.float64) - 1.5).to(DEV)          # (most maxima of short frames are negative)
    dg = torch.randn(B, 128, generator=gen, dtype=torch.float64).to(DEV)
    a = e.clone().requires_grad_(True)
    g, idx = ops.frame_max_f64(a)
    assert g.grad_fn is not None and not idx.requires_grad and idx.dtype == torch.int64
    b = e.clone().requires_grad_(True)
    want, widx = b.max(dim=1)
    assert torch.equal(g, want) and torch.equal(idx, widx)           # (continuous random values: no ties)
    (g * dg).sum().backward()
    (want * dg).sum().backward()
    assert torch.equal(a.grad, b.grad)
    assert torch.equal(ops.frame_max_backward(dg, idx, n), b.grad)
    with torch.no_grad():
        g2, idx2 = ops.frame_max_f64(e)
    assert g2.grad_fn is None and torch.equal(g2, want) and torch.equal(idx2, widx)


def test_frame_max_f64_refusals_and_ties():
    with pytest.raises(ValueError):
        ops.frame_max_f64(torch.zeros(1, 4, 64, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        ops.frame_max_f64(torch.zeros(1, 4, 128, device=DEV))
    with pytest.raises(ValueError):
        ops.frame_max_f64(torch.zeros(1, 0, 128, dtype=torch.float64, device=DEV))
    # of equal values the FIRST row wins, whatever phase of the kernel holds it; one writer per (pair, channel)
    e = torch.zeros(1, 40, 128, dtype=torch.float64, device=DEV) - 1.0
    e[0, 13] = 2.0
    e[0, 29] = 2.0
    e[0, 5, :64] = 2.0
    g, idx = ops.frame_max_f64(e)
    assert bool((g == 2.0).all()) and bool((idx[0, :64] == 5).all()) and bool((idx[0, 64:] == 13).all())
    # a NaN wins and is handed on, as torch.max hands it on (the first NaN's row)
    e[0, 21, 3] = float('nan')
    e[0, 30, 3] = float('nan')
    g2, idx2 = ops.frame_max_f64(e)
    want, widx = e.max(dim=1)
    assert bool(torch.isnan(g2[0, 3])) and int(idx2[0, 3]) == 21 == int(widx[0, 3]) and torch.equal(g2.nan_to_num(7.0), want.nan_to_num(7.0))
    de = ops.frame_max_backward(torch.ones(1, 128, dtype=torch.float64, device=DEV), idx, 40)
    assert float(de.sum()) == 128.0 and float(de[0, 5, :64].sum()) == 64.0 and float(de[0, 13, 64:].sum()) == 64.0


# ---- training_forward ----
@functools.lru_cache(maxsize=None)
def _case(descriptor, case):
    return DR.load_train(GOLDEN, descriptor, case)


def _data(descriptor, case):
    return {k: torch.from_numpy(v.copy()).to(DEV) for k, v in _case(descriptor, case)['data'].items()}


def _step(net, data):
    net.zero_grad(set_to_none=True)
    out = net.training_forward(data)
    out['loss'].mean().backward()
    torch.cuda.synchronize()
    return out


def _result(net, out):
    n = lambda t: t.detach().cpu().numpy()          # noqa: E731
    q = {'loss': n(out['loss'])}
    q.update({'grad:' + k: n(p.grad) for k, p in net.named_parameters() if p.grad is not None})
    q.update({'buf:' + k: n(b) for k, b in net.named_buffers() if not k.endswith('num_batches_tracked')})
    return q


@pytest.mark.parametrize('case', DR.TRAIN_CASES)
@pytest.mark.parametrize('descriptor', DR.DESCRIPTORS)
def test_training_forward_reproduces_the_recorded_step(descriptor, case):
    c = _case(descriptor, case)
    method = T.CASES[case][0]
    net, data = _net(descriptor, training=True, method=method), _data(descriptor, case)
    out = _step(net, data)
    got = _result(net, out)
    assert all(('grad:' + k) in got for k, _ in net.named_parameters()), 'a parameter was left without a gradient'
    names = [k for k in c['want'] if k != 'Z']
    assert len(names) == len(got)
    worst, where, fr = T.compare(got, c['want'], c['err'], names=names)
    enc = max(v for k, v in fr.items() if 'enc.' in k)
    print(f'{descriptor} {case}: worst fraction of the bound {worst:.4f} at {where}; over the encoders\' gradients and buffers {enc:.4f}')
    assert worst <= 1.0
    assert {k: int(b) for k, b in net.named_buffers() if k.endswith('num_batches_tracked')} == c['nbt']
    for f in (0, 1):
        assert np.array_equal(out[f'matches{f}'].cpu().numpy(), c[f'matches{f}'])
        assert float(np.abs(out[f'matching_scores{f}'].cpu().numpy() - c[f'mscores{f}']).max()) <= E.SCORE_TOL


@pytest.mark.parametrize('descriptor', DR.DESCRIPTORS)
def test_two_identical_steps_give_the_same_bits(descriptor):
    res = []
    for _ in range(2):
        net = _net(descriptor, training=True)
        out = _step(net, _data(descriptor, 'gap'))
        res.append((_result(net, out), out))
    a, b = res[0][0], res[1][0]
    assert set(a) == set(b) and len(a) > 40
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for k in ('matches0', 'matches1', 'matching_scores0', 'matching_scores1'):
        assert torch.equal(res[0][1][k], res[1][1][k])


@pytest.mark.parametrize('descriptor', DR.DESCRIPTORS)
def test_eval_mode_training_forward_agrees_with_forward(descriptor):
    net = _net(descriptor)
    before = {k: b.clone() for k, b in net.named_buffers()}
    out = net.training_forward(_data(descriptor, 'gap'))
    out['loss'].mean().backward()
    torch.cuda.synchronize()
    assert all(torch.equal(b, before[k]) for k, b in net.named_buffers())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    with torch.no_grad():
        ref = net(_data(descriptor, 'gap'))
    for f in (0, 1):
        assert torch.equal(out[f'matches{f}'], ref[f'matches{f}'])
        assert float((out[f'matching_scores{f}'] - ref[f'matching_scores{f}']).abs().max()) <= E.SCORE_TOL


# ---- the default descriptor computes what it computed before ----
# sha256 of descriptor_digest.fpfh_digest() recorded from the build of the commit before the FPFH_gloabal / FPFH_only encoders
FPFH_DIGEST = '0b268be1cfea355535177229acb8a44eba50ac7aa8f4df8748437d67794c179a'


def test_default_descriptor_is_bit_identical_to_the_build_before():
    assert descriptor_digest.fpfh_digest(DEV) == FPFH_DIGEST
