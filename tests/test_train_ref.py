"""tests/train_ref.py - the numpy restatement of a whole training step - against the reference's recorded steps
(tests/golden/train_*.npz, tools/make_goldens_train.py), the sharpness of the measured bound, and the host-side contract of
``MDGAT.training_forward`` / the opt-in dispatch from ``forward``.  CPU only."""
import functools

import numpy as np
import pytest
import torch

import head_grad_ref as H
import loss_grad_ref as LG
import loss_ref as LR
import sinkhorn_grad_ref as S
import train_ref as T
from conftest import GOLDEN


@functools.lru_cache(maxsize=None)
def _case(case):
    return T.load(GOLDEN, case)


@functools.lru_cache(maxsize=None)
def _state():
    return T.numpy_state(T.initial_state())


@functools.lru_cache(maxsize=None)
def _step(case, plant=None):
    return T.step(_state(), _case(case)['data'], T.CASES[case][0], plant=plant)


def test_fixture_files_are_small_and_complete():
    import os
    for name in T.ALL_FILES:
        assert os.path.getsize(T.golden_path(GOLDEN, name)) < (1 << 20), name
    c = _case('gap')
    names = {'grad:' + k for k in T.param_names(_state())}
    assert names <= set(c['want']) and names <= set(c['err']) and {'loss', 'Z'} <= set(c['want'])
    assert sum(k.startswith('buf:') for k in c['want']) == 2 * 7 and len(c['nbt']) == 7
    assert all(e > 0 for e in c['err'].values())
    for case in ('superglue', 'triplet'):
        w = _case(case)['want']
        assert {k for k in w if k.startswith('grad:')} == {'grad:' + k for k in T.param_names(_state()) if k.startswith(T.ENC_PREFIXES)}


@pytest.mark.parametrize('case', sorted(T.CASES))
def test_restatement_meets_fixture(case):
    c, res = _case(case), _step(case)
    worst, where, _ = T.compare(T.flatten(res), c['want'], c['err'])
    print(f'{case}: worst fraction of the bound {worst:.3f} at {where}')
    assert worst <= 1.0
    assert {k: int(v) for k, v in res['after'].items() if k.endswith('num_batches_tracked')} == c['nbt']
    # every BN moved twice: frame 0, then frame 1 (synth's state starts at 7)
    assert set(c['nbt'].values()) == {9}


def test_restatement_meets_second_step():
    c, first = _case('gap'), _step('gap')
    second = T.step(T.sgd(_state(), first['grads'], first['after']), c['data'], 'gap_loss')
    worst, where, _ = T.compare(T.flatten(second), c['step2']['want'], c['step2']['err'])
    print(f'gap, second step: worst fraction of the bound {worst:.3f} at {where}')
    assert worst <= 1.0
    # the step moved: the first step's loss is far outside the second's bound
    assert abs(float(np.mean(first['loss'])) - float(np.mean(c['step2']['want']['loss']))) > 1e-3
    # ... and a second step that reads stale buffers or stale parameters leaves it
    stale_buffers = T.step(T.sgd(_state(), first['grads'], {}), c['data'], 'gap_loss')
    stale_params = T.step(T.sgd(_state(), {}, first['after']), c['data'], 'gap_loss')
    for name, res in (('buffers', stale_buffers), ('parameters', stale_params)):
        worst, where, fr = T.compare(T.flatten(res), c['step2']['want'], c['step2']['err'])
        print(f'gap, second step with stale {name}: {worst:.3g} x the bound at {where}')
        assert worst > 1.0, name
        # in training mode a buffer shows in nothing but its own next value; a stale parameter shows in the loss
        assert (fr['loss'] > 1.0) == (name == 'parameters')
        assert all(v > 1.0 for k, v in fr.items() if k.startswith('buf:'))


# ---- the shape cases: a step past one tile of every kernel it composes ----
@functools.lru_cache(maxsize=None)
def _shape_state(L):
    return T.numpy_state(T.initial_state(L=L))


@functools.lru_cache(maxsize=None)
def _shape_step(case, plant=None):
    method, _, _, _, L, k, _ = T.case_spec(case)
    return T.step(_shape_state(L), _case(case)['data'], method, L=L, k_list=k, plant=plant)


@pytest.mark.parametrize('case', sorted(T.SHAPE_CASES))
def test_shape_fixture_is_complete(case):
    import os
    method, B, n, m, L, k, first = T.case_spec(case)
    g = T.R.load_files(GOLDEN, T.FILES[case])
    assert [int(v) for v in g['meta']] == [B, n, m, L, T.ITERS, T.SEED, first] and [int(v) or None for v in g['k']] == k
    c = _case(case)
    assert c['data']['keypoints0'].shape == (B, n, 3) and c['data']['descriptors1'].shape == (B, m, 33)
    quantities = {'loss', 'Z'} | {'grad:' + q for q in T.param_names(_shape_state(L))} | \
        {'buf:' + q for q in _shape_state(L) if q.endswith(('running_mean', 'running_var'))}
    # every quantity has its measured error; the reference's value of all but the layers' convolution weights
    assert set(c['err']) == quantities and all(e > 0 for e in c['err'].values())
    assert set(c['want']) == {q for q in quantities if T.shape_stored(q)}
    assert len(quantities) - len(c['want']) == 2 * L * 6
    assert len(c['nbt']) == 5 + 2 * L and c['want']['Z'].shape == (B, n + 1, m + 1)
    assert all(os.path.getsize(T.golden_path(GOLDEN, name)) < (1 << 20) for name in T.FILES[case])


@pytest.mark.parametrize('case', sorted(T.SHAPE_CASES))
def test_restatement_meets_shape_fixture(case):
    c, res = _case(case), _shape_step(case)
    worst, where, _ = T.compare(T.flatten(res), c['want'], c['err'])
    print(f'{case}: worst fraction of the bound {worst:.3f} at {where}')
    assert worst <= 1.0
    assert {k: int(v) for k, v in res['after'].items() if k.endswith('num_batches_tracked')} == c['nbt']
    assert set(c['nbt'].values()) == {9}
    # the layers the case is there for are dynamic, and their selection was decided by a margin
    sched = T.topk_schedule(*T.case_spec(case)[4:6])
    assert [mk is not None for mk in res['masks']] == [k > 0 for k in sched] and any(sched) and res['topk_gap'] > 1e-9


@pytest.mark.parametrize('plant', T.TAIL_PLANTS)
def test_tail_plants_leave_the_bound_only_past_one_tile(plant):
    """A mistake confined to a ragged tail tile of the attention backward, or to the second slab of a dW: the bound of 'tiles' sees
    it (against what the device test compares with: the stored values, the restatement for the layers' weights), and on 'gap' - less
    than one tile of everything - it changes no bit, which is why the small fixtures cannot hold it."""
    c = _case('tiles')
    want = T.shape_want(c, _shape_step('tiles'))
    worst, where, fr = T.compare(T.flatten(_shape_step('tiles', plant)), want, c['err'])
    out = sorted(k for k, v in fr.items() if v > 1.0)
    print(f'{plant} on tiles: {worst:.3g} x the bound at {where}; {len(out)} of {len(fr)} quantities leave it')
    assert worst > 1.0
    if plant == 'second_slab':          # frame 1 has 3 x 180 = 540 rows: one dW per layer, and nothing else moves at all
        assert out == [f'grad:gnn.layers.{i}.mlp.3.weight' for i in range(4)]
        assert all(v == 0.0 for k, v in fr.items() if k not in out and not T.shape_stored(k))
    else:                               # 70 = 64 + 6 and 180 = 128 + 52: dk and dv of every layer, and what they reach
        assert {f'grad:gnn.layers.{i}.attn.proj.{j}.weight' for i in range(4) for j in (1, 2)} <= set(out)
        assert fr['grad:final_proj.weight'] <= 1.0 and fr['loss'] <= 1.0
    plain, planted = T.flatten(_step('gap')), T.flatten(_step('gap', plant))
    assert set(plain) == set(planted)
    for k in plain:
        assert np.array_equal(plain[k], planted[k]), k


@pytest.mark.parametrize('plant', [p for p in T.PLANTS if p not in T.TAIL_PLANTS])
def test_bound_is_sharp(plant):
    c = _case('gap')
    got = T.flatten(_step('gap', plant))
    worst, where, fr = T.compare(got, c['want'], c['err'])
    print(f'{plant}: {worst:.3g} x the bound at {where}')
    assert worst > 1.0
    if plant == 'frame_order':          # the values of a step do not depend on the order of the frames: only the buffers tell
        assert all(v <= 1.0 for k, v in fr.items() if not k.startswith('buf:'))
        assert all(v > 1.0 for k, v in fr.items() if k.startswith('buf:'))
    if plant == 'no_bin_grad':
        assert where == 'grad:bin_score' and sum(v > 1.0 for v in fr.values()) == 1


def test_matches_come_from_the_recorded_Z():
    from oracle import mdgat_oracle as O
    c = _case('gap')
    m0, m1, s0, s1 = O.extract_matches(torch.from_numpy(c['want']['Z']), 'gap_loss', False, 0.2)
    assert np.array_equal(m0.numpy(), c['matches0']) and np.array_equal(m1.numpy(), c['matches1'])
    assert np.abs(s0.numpy() - c['mscores0']).max() < 1e-12 and np.abs(s1.numpy() - c['mscores1']).max() < 1e-12
    for case in T.CASES:            # something matched in every case: the scores are the float kind (mdgat.py:464-467)
        m = _case(case)['matches0']
        print(f'{case}: {int((m >= 0).sum())} of {m.size} keypoints of frame 0 matched')
        assert (m >= 0).any(), case


def test_float64_pieces_agree_with_their_pinned_siblings():
    """head, optimal transport and loss are written out in train_ref for the 80-bit evaluation; in float64 each is its pinned sibling."""
    c, res = _case('gap'), _step('gap')
    Z, gt0, gt1 = c['want']['Z'], c['data']['gt_matches0'], c['data']['gt_matches1']
    for method in T.METHODS:
        zz = Z if method == 'gap_loss' else Z[:, :21, :21]
        a0, a1 = (gt0, gt1) if method == 'gap_loss' else (np.clip(gt0, -1, 19), np.clip(gt1[:, :20], -1, 19))
        loss, dZ = T.loss_forward_backward(zz, a0, a1, method, T.GAMMA)
        want = LR.module_loss(zz, a0, a1, method, T.GAMMA)
        assert np.allclose(loss, want, rtol=1e-13, atol=0), method
        wd = LG.pair_grads(zz, a0, a1, method, T.GAMMA, np.full(2, 0.5))
        assert np.abs(dZ - wd).max() <= 1e-13 * np.abs(wd).max(), method
    rs = np.random.RandomState(3)
    d0, d1, W, b = rs.standard_normal((2, 9, 128)), rs.standard_normal((2, 13, 128)), rs.standard_normal((128, 128, 1)) / 11, rs.standard_normal(128)
    scores, st = T.head_forward(d0, d1, W, b)
    G = rs.standard_normal(scores.shape)
    assert np.abs(scores - H.forward(d0, d1, W, b)).max() < 1e-12
    for a, w in zip(T.head_backward(d0, d1, W, st, G), H.backward(d0, d1, W, b, G)):
        assert np.abs(a - w).max() <= 1e-12 * np.abs(w).max()
    from oracle import mdgat_oracle as O
    Zs, sst = T.sinkhorn_forward(scores, 0.7, 20)
    assert np.abs(Zs - O.log_optimal_transport(torch.from_numpy(scores), torch.tensor(0.7, dtype=torch.float64), 20).numpy()).max() < 1e-12
    GZ = rs.standard_normal(Zs.shape)
    ds, da = T.sinkhorn_backward(sst, GZ)
    wds, wda = S.sinkhorn_grad(scores, 0.7, 20, GZ)
    assert np.abs(ds - wds.numpy()).max() <= 1e-10 * np.abs(wds.numpy()).max() and abs(da - float(wda.sum())) <= 1e-10 * abs(float(wda.sum()))
    assert res['Z'].dtype == np.float64


def test_schedule_and_permutation_are_the_package_s():
    from mdgat_matcher_amd import pack, train
    assert list(T.PERM) == train._PERM
    for L, k in ((1, [8]), (2, [16, None, 8, None]), (9, [128, None, 128, None, 64, None, 64, None]), (2, [])):
        assert T.topk_schedule(L, k) == pack.resolve_topk_schedule(L, k)


# ---- the host-side contract ----
def _net(**over):
    from mdgat_matcher_amd import MDGAT
    return MDGAT(T.config('gap_loss', **over)).double()


def _cpu_data():
    return {k: torch.from_numpy(v.copy()) for k, v in _case('gap')['data'].items()}


def test_training_forward_has_no_cpu_fallback():
    for net in (_net().train(), _net().eval()):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            net.training_forward(_cpu_data())


def test_forward_in_training_mode_is_opt_in(monkeypatch):
    monkeypatch.delenv('MDGAT_TRAIN_FORWARD', raising=False)
    with pytest.raises(NotImplementedError):
        _net().train()(_cpu_data())
    with pytest.raises(NotImplementedError):
        _net(train_forward=False).train()(_cpu_data())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _net(train_forward=True).train()(_cpu_data())
    monkeypatch.setenv('MDGAT_TRAIN_FORWARD', '1')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _net().train()(_cpu_data())
    with pytest.raises(NotImplementedError):
        _net(train_forward=False).train()(_cpu_data())           # the config key wins over the environment
    # the empty-keypoint early-out comes first, in every mode (mdgat.py:374-382)
    d = _cpu_data()
    d['keypoints0'] = d['keypoints0'][:, :0]
    out = _net().train()(d)
    assert out['skip_train'] is True and out['matches0'].shape == (0,) and out['matches1'].shape == (28,)
    assert _net().train().training_forward(d)['skip_train'] is True


def test_mlp_tensors_entry_checks_its_arguments():
    from mdgat_matcher_amd import ops
    x = torch.zeros(4, 128, dtype=torch.float64)
    w, b = torch.zeros(128, 128, dtype=torch.float64), torch.zeros(128, dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.mlp_f64_tensors(x, [w, w], [b, b])                                  # two convolutions need a BatchNorm1d between them
    with pytest.raises(ValueError):
        ops.mlp_f64_tensors(x, [w[:40]], [b[:40]])                              # 40 outputs: not a multiple of 16
    with pytest.raises(RuntimeError):
        ops.mlp_f64_tensors(x, [w], [b], residual=x)                            # CPU tensors
