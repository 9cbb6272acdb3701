"""The FPFH_gloabal and FPFH_only descriptor encoders on the host: the module's parameters against the reference's recorded state-dict
names (tests/golden/desc_*_eval.npz, tools/make_goldens_descriptors.py), the packer, and the numpy restatement of the two encoders
(tests/descriptor_ref.py) against the reference's recorded encoder outputs and gradients - with the planted mistakes its bound must
catch.  No GPU."""
import hashlib
import os

import numpy as np
import pytest
import torch

import descriptor_ref as DR
import mlp_grad_ref as R
import train_ref as T
from conftest import GOLDEN
from mdgat_matcher_amd import MDGAT, pack, synth

FACTOR = T.FACTOR


def _eval(descriptor):
    return dict(np.load(T.golden_path(GOLDEN, DR.eval_file(descriptor))))


def _net(descriptor, **over):
    return MDGAT(DR.config('gap_loss', descriptor, **over))


@pytest.mark.parametrize('descriptor', DR.DESCRIPTORS)
def test_state_dict_is_the_reference_s(descriptor):
    g = _eval(descriptor)
    want = {str(k): tuple(int(x) for x in str(s).split(',') if x) for k, s in zip(g['names'], g['shapes'])}
    net = _net(descriptor)
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == want, set(got) ^ set(want)
    n_params = {k for k, _ in net.named_parameters()}
    assert sum(int(np.prod(want[k])) for k in n_params) == sum(p.numel() for p in net.parameters())
    assert ('kenc.encoder.0.weight' in got) == (descriptor != 'FPFH_only')
    assert ('denc.encoder2.3.weight' in got) == (descriptor == 'FPFH_gloabal')
    sd = DR.initial_state(descriptor)
    assert set(sd) == set(want) and all(tuple(v.shape) == want[k] for k, v in sd.items())
    net.load_state_dict(sd, strict=True)
    torch.nn.DataParallel(net).load_state_dict({'module.' + k: v for k, v in sd.items()}, strict=True)
    # a state dict of another descriptor does not load
    with pytest.raises(RuntimeError):
        net.load_state_dict(synth.make_state_dict(T.L, DR.SEED), strict=True)


def test_parameter_counts():
    base = sum(p.numel() for p in MDGAT(T.config('gap_loss')).parameters())
    kenc = sum(p.numel() for p in MDGAT(T.config('gap_loss')).kenc.parameters())
    enc2 = 256 * 256 + 256 + 2 * 256 + 128 * 256 + 128                    # Conv1d(256, 256) + BN(256) + Conv1d(256, 128)
    assert sum(p.numel() for p in _net('FPFH_only').parameters()) == base - kenc
    assert sum(p.numel() for p in _net('FPFH_gloabal').parameters()) == base + enc2


def test_init_and_refusals():
    net = _net('FPFH_gloabal')
    assert float(net.denc.encoder2[-1].bias.abs().sum()) == 0.0 and float(net.denc.encoder[-1].bias.abs().sum()) == 0.0      # mdgat.py:159, 161
    assert not hasattr(_net('FPFH_only'), 'kenc')
    for d in ('pointnet', 'pointnetmsg'):
        with pytest.raises(NotImplementedError):
            MDGAT(DR.config('gap_loss', d))
    with pytest.raises(ValueError):
        _net('FPFH_gloabal', attention_dtype='f16')
    # the encoders of a pooled module run in fp64 whatever its dtype; only a float64 one runs the exact mode
    assert _net('FPFH_gloabal')._handle_f64() and not _net('FPFH_gloabal').exact() and _net('FPFH_gloabal').double().exact()
    assert not _net('FPFH_only')._handle_f64()


def test_synth_default_is_unchanged_and_shared():
    a = synth.make_state_dict(T.L, DR.SEED)
    assert list(a) == list(synth.make_state_dict(T.L, DR.SEED, descriptor='FPFH'))
    for d in DR.DESCRIPTORS:
        b = synth.make_state_dict(T.L, DR.SEED, descriptor=d)
        assert all(torch.equal(a[k], b[k]) for k in a if k in b)
    with pytest.raises(ValueError):
        synth.make_state_dict(1, 0, descriptor='pointnet')


# recorded from the commit before the descriptor argument existed: sha256 of pack_state_dict(make_state_dict(L=2, seed), 2, dtype)
PARENT_BLOBS = {(0, 'float32'): '12e00b8cc1304d379efd94f16e87225a5040428963852c995c5fbcd8d0264585',
                (0, 'float64'): 'fe032e089402f52db08b69a55b5049ba20fcb65d1a7cea0b0f82399cf3705469',
                (3, 'float32'): '29b22855f5d3e6328ff65b093549eaed8f646d4cfd0a88a73c5901d57e242ea7',
                (3, 'float64'): '68f67707c8d87993b7ec0c62317c43a92fcfa950b3844cf7295913b00cff74c4'}


@pytest.mark.parametrize('seed', (0, 3))
def test_default_blob_is_byte_identical(seed):
    sd = synth.make_state_dict(L=2, seed=seed)
    for dt in (np.float32, np.float64):
        assert hashlib.sha256(pack.pack_state_dict(sd, 2, dtype=dt).tobytes()).hexdigest() == PARENT_BLOBS[(seed, dt.__name__)]
    assert pack.descriptor_of(sd) == 'FPFH' and pack.descriptor_of({'module.' + k: v for k, v in sd.items()}) == 'FPFH'


KENC_RANGES = (('kenc0_w', 32 * 4), ('kenc0_b', 32), ('kenc1_w', 64 * 32), ('kenc1_b', 64), ('kenc2_w', 128 * 64), ('kenc2_b', 128))


def test_pack_fpfh_only():
    L = T.L
    sd, full = DR.initial_state('FPFH_only'), synth.make_state_dict(L, DR.SEED)
    assert pack.descriptor_of(sd) == 'FPFH_only'
    lay = pack.blob_layout(L)
    for dt in (np.float32, np.float64):
        blob, ref = pack.pack_state_dict(sd, L, dtype=dt), pack.pack_state_dict(full, L, dtype=dt)
        for name, n in KENC_RANGES:
            assert not blob[lay[name]:lay[name] + n].any(), name
        encl = blob[lay['encl_w']:lay['encl_w'] + 128 * 256].reshape(128, 256)
        rencl = ref[lay['encl_w']:lay['encl_w'] + 128 * 256].reshape(128, 256)
        assert not encl[:, 128:].any() and np.array_equal(encl[:, :128], rencl[:, :128]) and rencl[:, 128:].any()
        # encl_b = denc.6.bias alone (the hidden gauge never touches a bias of the last convolution)
        assert np.array_equal(blob[lay['encl_b']:lay['encl_b'] + 128], sd['denc.encoder.6.bias'].numpy().astype(dt))
        # everything but the kenc ranges and encl is the 'FPFH' blob of the same weights
        same = np.ones(blob.size, dtype=bool)
        for name, n in KENC_RANGES:
            same[lay[name]:lay[name] + n] = False
        same[lay['encl_w']:lay['encl_b'] + 128] = False
        assert np.array_equal(blob[same], ref[same])
    with pytest.raises(KeyError):
        pack.pack_pooled_encoder(sd)


def test_pack_fpfh_gloabal():
    L = T.L
    sd = DR.initial_state('FPFH_gloabal')
    assert pack.descriptor_of(sd) == 'FPFH_gloabal'
    lay = pack.blob_layout(L)
    blob = pack.pack_state_dict(sd, L, dtype=np.float64)
    ref = pack.pack_state_dict(synth.make_state_dict(L, DR.SEED), L, dtype=np.float64)
    encl = blob[lay['encl_w']:lay['encl_w'] + 128 * 256].reshape(128, 256)
    assert not encl[:, 128:].any() and np.array_equal(blob[:lay['encl_w']], ref[:lay['encl_w']])       # the kenc and denc stages as for 'FPFH'
    assert np.array_equal(blob[lay['encl_b']:lay['encl_b'] + 128], sd['denc.encoder.6.bias'].numpy())
    p = pack.pack_pooled_encoder(sd)
    assert p.dtype == np.float64 and p.size == pack.POOLED_ENCODER_DOUBLES == 115072
    w1e, w1g = p[:32768].reshape(256, 128), p[32768:65536].reshape(256, 128)
    b1, w2k, b2 = p[65536:65792], p[65792:65792 + 128 * 384].reshape(128, 384), p[-128:]
    # the packed encoder2 computes what the module's eval() BatchNorm computes: on random inputs, against the plain formulas
    rs = np.random.RandomState(5)
    e, g, hk = rs.standard_normal((7, 128)), rs.standard_normal(128), np.abs(rs.standard_normal((7, 128)))
    n = lambda k: sd[k].numpy()          # noqa: E731
    y = np.concatenate([e, np.broadcast_to(g, e.shape)], axis=1) @ n('denc.encoder2.0.weight')[:, :, 0].T + n('denc.encoder2.0.bias')
    z = (y - n('denc.encoder2.1.running_mean')) / np.sqrt(n('denc.encoder2.1.running_var') + 1e-5) * n('denc.encoder2.1.weight') + n('denc.encoder2.1.bias')
    want = np.maximum(z, 0) @ n('denc.encoder2.3.weight')[:, :, 0].T + n('denc.encoder2.3.bias')
    kenc3 = ref[lay['encl_w']:lay['encl_w'] + 128 * 256].reshape(128, 256)[:, 128:]                   # kenc.9 in the hidden gauge of 'FPFH'
    want = want + hk @ kenc3.T + n('kenc.encoder.9.bias')
    hidden = np.maximum(e @ w1e.T + (w1g @ g + b1), 0)
    got = np.concatenate([hidden, hk], axis=1) @ w2k.T + b2
    assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max())
    assert np.array_equal(w2k[:, 256:], kenc3)


# ---- the restatement against the reference's recorded results ----
def _npdata(g, prefix='in:'):
    return {k[len(prefix):]: g[k] for k in g if k.startswith(prefix)}


@pytest.mark.parametrize('descriptor', DR.DESCRIPTORS)
def test_restatement_reproduces_the_encoder_outputs(descriptor):
    g = _eval(descriptor)
    sd = T.numpy_state(DR.initial_state(descriptor))
    data, err = _npdata(g), float(g['enc_err'])
    got = DR.encode(sd, data, descriptor)
    worst = max(float(np.abs(got[f] - g[f'enc{f}']).max()) for f in (0, 1))
    print(f'{descriptor}: encoder outputs: {worst / (FACTOR * err):.4f} of the bound ({FACTOR} x {err:.2e})')
    assert worst <= FACTOR * err
    # the planted mistakes, each far beyond the bound
    plants = ('joint_pool', 'no_kenc') if descriptor == 'FPFH_gloabal' else ()
    for plant in plants:
        bad = DR.encode(sd, data, descriptor, plant=plant)
        d = max(float(np.abs(bad[f] - g[f'enc{f}']).max()) for f in (0, 1))
        print(f'{descriptor}: planted {plant}: {d / (FACTOR * err):.3e} of the bound')
        assert d > 1e6 * FACTOR * err, plant


def test_restatement_reproduces_the_ragged_pairs_and_sees_the_padding():
    g = dict(np.load(T.golden_path(GOLDEN, DR.RAGGED_FILE)))
    sd = T.numpy_state(DR.initial_state('FPFH_gloabal'))
    err = float(_eval('FPFH_gloabal')['enc_err'])
    counts = [tuple(int(x) for x in c) for c in g['counts']]
    assert tuple(counts) == DR.RAGGED_COUNTS
    slots = (max(c[0] for c in counts), max(c[1] for c in counts))
    for i, (n, m) in enumerate(counts):
        data = _npdata(g, f'p{i}:in:')
        assert data['keypoints0'].shape == (1, n, 3) and data['keypoints1'].shape == (1, m, 3)
        got = DR.encode(sd, data, 'FPFH_gloabal')
        assert max(float(np.abs(got[f] - g[f'p{i}:enc{f}']).max()) for f in (0, 1)) <= FACTOR * err
        pad = (slots[0] - n, slots[1] - m)
        bad = DR.encode(sd, data, 'FPFH_gloabal', plant='padded_pool', pad=pad)
        for f in (0, 1):
            d = float(np.abs(bad[f] - g[f'p{i}:enc{f}']).max())
            if pad[f]:
                assert int(g['visible'][i, f]) >= 8
                assert d > 1e6 * FACTOR * err, (i, f)          # a pool over the slot's padded rows is far outside the bound
            else:
                assert int(g['visible'][i, f]) == -1 and d <= FACTOR * err
    # the generator's other conditions, re-checked on the stored inputs: no pool tie, a negative maximum in every frame
    p = T._mlp_p(sd, 'denc.encoder', 3)
    for i in range(len(counts)):
        for f in (0, 1):
            e = R.forward(g[f'p{i}:in:descriptors{f}'].reshape(-1, 33), p, training=False)[0][None]
            assert DR.pool_gap(e) > 1e-9 and int((e.max(axis=1) < 0).sum()) >= 1


@pytest.mark.parametrize('case', DR.TRAIN_CASES)
@pytest.mark.parametrize('descriptor', DR.DESCRIPTORS)
def test_restatement_reproduces_the_recorded_step(descriptor, case):
    c = DR.load_train(GOLDEN, descriptor, case)
    method = T.CASES[case][0]
    sd = T.numpy_state(DR.initial_state(descriptor))
    assert set(k[5:] for k in c['want'] if k.startswith('grad:')) == set(T.param_names(sd))           # every gradient is recorded
    got = DR.step(sd, c['data'], method, descriptor)
    names = [k for k in c['want'] if k in ('loss', 'Z') or k.startswith(('grad:denc.', 'grad:kenc.', 'buf:denc.', 'buf:kenc.'))]
    worst, where, fr = T.compare(T.flatten(got), c['want'], c['err'], names=names)
    print(f'{descriptor} {case}: loss, Z, encoder gradients and buffers: worst fraction of the bound {worst:.4f} at {where}')
    assert worst <= 1.0
    assert {k: int(v) for k, v in got['after'].items() if k.endswith('num_batches_tracked')} == c['nbt']
    if descriptor == 'FPFH_gloabal':
        assert {c['nbt'][f'denc.encoder2.1.num_batches_tracked'], c['nbt']['denc.encoder.1.num_batches_tracked']} == {9}       # 7 + one call per frame
        assert got['pool_gap'] > 1e-9
        if case == 'gap':
            bad = DR.step(sd, c['data'], method, descriptor, plant='no_kenc')
            w, where, _ = T.compare(T.flatten(bad), c['want'], c['err'], names=['loss', 'grad:denc.encoder2.3.weight'])
            print(f'{descriptor} {case}: planted no_kenc: {w:.3e} of the bound at {where}')
            assert w > 1e6


def test_pool_backward_follows_torch_on_ties():
    """Which row of a tie receives the gradient: ONE row, as torch.max's backward sends it - not every row that equals the maximum."""
    rs = np.random.RandomState(3)
    e = rs.standard_normal((2, 6, 128))
    e[:, 4] = e[:, 1]                       # two identical keypoints: every channel one of them wins is tied
    dg = rs.standard_normal((2, 128))
    t = torch.from_numpy(e).requires_grad_(True)
    vals, tidx = t.max(dim=1)
    (vals * torch.from_numpy(dg)).sum().backward()
    g, idx = DR.pool(e)
    assert np.array_equal(g, vals.detach().numpy())
    tied = (e == e.max(axis=1, keepdims=True)).sum(axis=1) > 1
    assert tied.any() and np.array_equal(idx[~tied], tidx.numpy()[~tied])
    # one winner per (pair, channel): the column sums are dg, and off ties it is torch's gradient exactly
    de = DR.pool_backward(dg, idx, e)
    assert np.array_equal(de.sum(axis=1), dg) and int((de != 0).sum()) == dg.size
    want = t.grad.numpy()
    assert np.array_equal(want.sum(axis=1), dg)
    assert np.array_equal(de[:, :, :][np.broadcast_to(~tied[:, None, :], e.shape)], want[np.broadcast_to(~tied[:, None, :], e.shape)])
    # the planted mistake doubles the tied channels' gradient
    bad = DR.pool_backward(dg, idx, e, all_ties=True)
    assert np.array_equal(bad.sum(axis=1)[tied], 2 * dg[tied]) and np.array_equal(bad.sum(axis=1)[~tied], dg[~tied])
