"""Training batches straight from raw frame records: ops.assemble_frames_train (the loader's train-mode assembly: saliency filter, truncate
or pad to max_keypoints, float32 FPFH normalisation) and MDGAT.training_batch_frames / training_forward_frames.  The yardsticks are the
reference loader's own outputs with ensure_kpts_num=True (tests/golden/train_loader.npz) - bit for bit - the host restatement
tests/train_frames_ref.py at the shapes the golden lacks, and MDGAT.training_forward on the batch built from the loader's outputs."""
import functools

import numpy as np
import pytest
import torch

import train_frames_ref as R
from conftest import GOLDEN
from oracle import mdgat_oracle as O

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@functools.lru_cache(maxsize=None)
def _golden():
    return R.load_golden(GOLDEN)


@functools.lru_cache(maxsize=None)
def _bank(name):
    """The set's frames as a bank with a frame of NaN records no pair points at in front of, between and behind them:
    (bank, frame number -> index in the bank)."""
    from mdgat_matcher_amd import ops
    _, sets = _golden()
    s = sets[name]
    poison = np.full((9, 37), np.nan, dtype=np.float32)
    frames, where = [poison], {}
    for i in s['frames']:
        where[i] = len(frames)
        frames += [s['rec'][i], poison]
    return ops.pack_frames(frames, DEV), where


def _chunk(name):
    _, sets = _golden()
    bank, where = _bank(name)
    pairs = sets[name]['pairs']
    return bank, [where[a] for a, _ in pairs], [where[b] for _, b in pairs]


def _transforms(name):
    g, sets = _golden()
    s = sets[name]
    tr = [O.frame_transforms(s['pose'][a], s['pose'][b], g['T_cam0_velo']) for a, b in s['pairs']]
    return tuple(torch.from_numpy(np.stack([t[i] for t in tr])) for i in range(3))


def _net(method='triplet_loss', training=True, dtype=torch.float64, **over):
    from mdgat_matcher_amd import MDGAT, synth
    net = MDGAT(synth.default_config(L=2, k=[8, None, 8, None], sinkhorn_iterations=20, loss_method=method, **over))
    net.load_state_dict(synth.make_state_dict(L=2, seed=1))
    return net.to(dtype).to(DEV).train(training)


def _words_clear(a):
    assert int(a['range_violation']) == 0 and not bool(a['status'].any())


@pytest.mark.parametrize('name', ['t40', 't64'])
def test_assemble_equals_the_loader(name):
    from mdgat_matcher_amd import ops
    g, sets = _golden()
    s = sets[name]
    T, pairs = s['T'], s['pairs']
    bank, idx0, idx1 = _chunk(name)
    a = ops.assemble_frames_train(bank, idx0, idx1, T, min_saliency=float(g['min_saliency']))
    B = len(pairs)
    _words_clear(a)                  # (the NaN frames around every frame of the bank were not read, nor what the dropped records hold)
    for f in (0, 1):
        assert a[f'keypoints{f}'].dtype == torch.float64 and tuple(a[f'keypoints{f}'].shape) == (B, T, 3)
        assert tuple(a[f'scores{f}'].shape) == (B, T) and tuple(a[f'descriptors{f}'].shape) == (B, T, 33)
        assert a[f'keypoints{f}_f32'].dtype == torch.float32 and a[f'source{f}'].dtype == torch.int32 and a[f'salient{f}'].dtype == torch.int32
        for j, pair in enumerate(pairs):
            want = R.loader_inputs(g, name, j, f)
            for k, w in want.items():
                assert torch.equal(a[f'{k}{f}'][j].cpu(), torch.from_numpy(w)), (name, j, f, k)
            ref = R.assemble_frame(s['rec'][pair[f]], T, float(g['min_saliency']))
            assert torch.equal(a[f'keypoints{f}_f32'][j].cpu(), torch.from_numpy(ref['keypoints_f32'])), (j, f)
            assert torch.equal(a[f'source{f}'][j].cpu(), torch.from_numpy(ref['source'])), (j, f)
            assert int(a[f'salient{f}'][j]) == ref['salient'], (j, f)
    # a frame shared by two pairs gives the same rows in both
    seen, shared = {}, 0
    for f in (0, 1):
        for j, pair in enumerate(pairs):
            if pair[f] in seen:
                f2, j2 = seen[pair[f]]
                for k in ('keypoints', 'scores', 'descriptors', 'source'):
                    assert torch.equal(a[f'{k}{f}'][j], a[f'{k}{f2}'][j2])
                shared += 1
            seen[pair[f]] = (f, j)
    assert shared >= (1 if name == 't40' else 0)
    # without the normalisation: the records' own FPFH rows
    raw = ops.assemble_frames_train(bank, idx0[:1], idx1[:1], T, normalize=False)
    src = raw['source0'][0].cpu().numpy()
    assert torch.equal(raw['descriptors0'][0].cpu(), torch.from_numpy(s['rec'][pairs[0][0]][src, 4:].astype(np.float64)))


@functools.lru_cache(maxsize=None)
def _seeded_frames():
    """Frames the golden has no like of: (records, kept): one record; 100 records (no multiple of 64) of which one is kept, the last;
    3000 records with more kept than any T below; 3000 with 300 kept; 777 with 512 kept; 65 all kept."""
    rs = np.random.RandomState(1234)
    spec = [(1, 1), (100, 1), (3000, 1500), (3000, 300), (777, 512), (65, 65)]
    frames = []
    for n, v in spec:
        r = rs.standard_normal((n, 37)).astype(np.float32)
        r[:, 4:] = np.abs(r[:, 4:]) * 50
        keep = np.zeros(n, dtype=bool)
        keep[rs.permutation(n)[:v]] = True
        if (n, v) == (100, 1):
            keep[:] = False
            keep[-1] = True
        r[:, 3] = np.where(keep, rs.uniform(10.5, 30, n), rs.uniform(-5, 10, n)).astype(np.float32)
        frames.append(r)
    return frames, spec


@pytest.mark.parametrize('T', [1, 512, 2048])
def test_assemble_equals_the_restatement_at_other_shapes(T):
    from mdgat_matcher_amd import ops
    frames, spec = _seeded_frames()
    bank = ops.pack_frames(frames, DEV)
    idx0, idx1 = [0, 2, 4, 1], [1, 3, 5, 2]
    a = ops.assemble_frames_train(bank, idx0, idx1, T)
    _words_clear(a)
    for f, idx in enumerate((idx0, idx1)):
        for b, i in enumerate(idx):
            ref = R.assemble_frame(frames[i], T)
            assert ref['salient'] == spec[i][1]
            assert int(a[f'salient{f}'][b]) == ref['salient'], (T, b, f)
            assert torch.equal(a[f'source{f}'][b].cpu(), torch.from_numpy(ref['source'])), (T, b, f)
            for k in ('keypoints', 'scores', 'descriptors'):
                assert torch.equal(a[f'{k}{f}'][b].cpu(), torch.from_numpy(ref[k])), (T, b, f, k)
            assert torch.equal(a[f'keypoints{f}_f32'][b].cpu(), torch.from_numpy(ref['keypoints_f32'])), (T, b, f)


@pytest.mark.parametrize('mutual', [False, True])
@pytest.mark.parametrize('name', ['t40', 't64'])
def test_training_batch_frames_gives_the_loaders_ground_truth(name, mutual):
    """Padded frames are full of exact duplicates: the ground truth there is decided by the first-minimum tie rule."""
    g, sets = _golden()
    s = sets[name]
    bank, idx0, idx1 = _chunk(name)
    T0, T1, T_gt = _transforms(name)
    net = _net(mutual_check=mutual)
    # gt_mutual=None: the module's own option, as the reference hands one option to loader and model
    batch = net.training_batch_frames(bank, idx0, idx1, T0, T1, T_gt=T_gt, max_keypoints=s['T'], gt_threshold=float(g['threshold']))
    prefix = 'mutual_' if mutual else ''
    assert batch['gt_matches0'].dtype == torch.int64 and tuple(batch['gt_matches0'].shape) == (len(idx0), s['T'])
    for j in range(len(idx0)):
        tag = f'{name}_item{j}_{prefix}'
        for f in (0, 1):
            want = torch.from_numpy(g[tag + f'gt_matches{f}'].astype(np.int64))
            assert torch.equal(batch[f'gt_matches{f}'][j].cpu(), want), (name, mutual, j, f)
        assert int(batch['rep'][j]) == int(g[tag + 'rep']), (name, mutual, j)
        assert torch.equal(batch['T_gt'][j].cpu(), T_gt[j])
        np.testing.assert_allclose(T_gt[j].numpy(), g[tag + 'T_gt'], rtol=0, atol=1e-9)      # (the loader's own T_gt: torch.inverse, to rounding)
    assert {'keypoints0', 'scores0', 'descriptors0', 'keypoints1', 'scores1', 'descriptors1', 'source0', 'source1', 'salient0', 'salient1'} <= set(batch)
    # the option given overrides the module's
    other = net.training_batch_frames(bank, idx0, idx1, T0, T1, max_keypoints=s['T'], gt_threshold=float(g['threshold']), gt_mutual=not mutual)
    tag = f'{name}_item1_' + ('' if mutual else 'mutual_')
    assert torch.equal(other['gt_matches0'][1].cpu(), torch.from_numpy(g[tag + 'gt_matches0'].astype(np.int64))) and 'T_gt' not in other


def _loader_batch(name, items, mutual=False):
    """the batch a DataLoader would collate from the reference loader's outputs of these items"""
    g, _ = _golden()
    prefix = 'mutual_' if mutual else ''
    batch = {}
    for f in (0, 1):
        for k in ('keypoints', 'scores', 'descriptors'):
            batch[f'{k}{f}'] = torch.from_numpy(np.stack([R.loader_inputs(g, name, j, f)[k] for j in items])).to(DEV)
        batch[f'gt_matches{f}'] = torch.from_numpy(np.stack([g[f'{name}_item{j}_{prefix}gt_matches{f}'] for j in items]).astype(np.int64)).to(DEV)
    return batch


def _step(net, forward):
    net.zero_grad(set_to_none=True)
    if net.training:
        out = forward()
        out['loss'].mean().backward()
    else:
        with torch.no_grad():
            out = forward()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('method', ['triplet_loss', 'gap_loss'])
def test_training_forward_frames_equals_training_forward_on_the_loaders_batch(method, training):
    g, sets = _golden()
    items = [1, 2]              # 29 x 7 and 1 x 80 kept: padded frames, and a frame of 40 copies of one keypoint
    bank, idx0, idx1 = _chunk('t40')
    T0, T1, _ = _transforms('t40')
    pick = lambda v: [v[j] for j in items]          # noqa: E731
    ref_net, net = _net(method, training), _net(method, training)
    before = {k: b.clone() for k, b in net.named_buffers()}
    ref = _step(ref_net, lambda: ref_net.training_forward(_loader_batch('t40', items)))
    got = _step(net, lambda: net.training_forward_frames(bank, pick(idx0), pick(idx1), T0[items], T1[items], max_keypoints=40,
                                                         gt_threshold=float(g['threshold'])))
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].dtype == ref[k].dtype and torch.equal(got[k], ref[k]), (method, training, k)
    assert bool(torch.isfinite(got['loss']).all()) and bool((got['matches0'] >= -1).all())
    grads = 0
    for (k, p), (_, q) in zip(net.named_parameters(), ref_net.named_parameters()):
        if training:
            assert p.grad is not None and torch.equal(p.grad, q.grad), k
            grads += 1
        else:
            assert p.grad is None and q.grad is None
    assert grads == (len(list(net.parameters())) if training else 0)
    moved = 0
    for (k, b), (_, c) in zip(net.named_buffers(), ref_net.named_buffers()):
        assert torch.equal(b, c), k
        moved += int(not torch.equal(b, before[k]))
        if not training:
            assert torch.equal(b, before[k]), k
    assert moved > 0 if training else moved == 0


def test_fpfh_only_filters_by_saliency_like_the_other_descriptors():
    from mdgat_matcher_amd import MDGAT, synth
    g, _ = _golden()
    items = [1, 2]
    bank, idx0, idx1 = _chunk('t40')
    T0, T1, _ = _transforms('t40')
    nets = []
    for _ in range(2):
        net = MDGAT(synth.default_config(L=2, k=[8, None, 8, None], sinkhorn_iterations=20, loss_method='gap_loss', descriptor='FPFH_only'))
        net.load_state_dict(synth.make_state_dict(L=2, seed=1, descriptor='FPFH_only'))
        nets.append(net.double().to(DEV).train())
    ref = _step(nets[0], lambda: nets[0].training_forward(_loader_batch('t40', items)))
    got = _step(nets[1], lambda: nets[1].training_forward_frames(bank, [idx0[j] for j in items], [idx1[j] for j in items], T0[items], T1[items],
                                                                 max_keypoints=40, gt_threshold=float(g['threshold'])))
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    for (k, p), (_, q) in zip(nets[1].named_parameters(), nets[0].named_parameters()):
        assert torch.equal(p.grad, q.grad), k


def test_refusals():
    from mdgat_matcher_amd import ops
    rs = np.random.RandomState(5)

    def frame(n, saliency):
        r = rs.standard_normal((n, 37)).astype(np.float32)
        r[:, 4:] = np.abs(r[:, 4:])
        r[:, 3] = saliency
        return r
    dull = frame(20, 10.0)                      # exactly the threshold everywhere, and a NaN: nothing is kept
    dull[7, 3] = np.nan
    good = frame(30, 15.0)
    bank = ops.pack_frames([good, frame(12, 11.0), dull, frame(5, 12.0)], DEV)
    net = _net()
    a = ops.assemble_frames_train(bank, [0, 1, 3], [1, 2, 0], 16)
    assert a['status'].cpu().tolist() == [[0, 0], [0, 1], [0, 0]] and a['salient1'].cpu().tolist() == [12, 0, 30]
    with pytest.raises(ValueError, match=r"pair 1: frame 1 \(frame 2 of the bank\) has no keypoint with saliency > 10: the reference's loader does not terminate"):
        net.training_batch_frames(bank, [0, 1, 3], [1, 2, 0], None, None, max_keypoints=16)
    with pytest.raises(ValueError, match=r'pair 0: frame 0 \(frame 2 of the bank\)'):
        net.training_forward_frames(bank, [2], [0], None, None, max_keypoints=16)
    # a lower bar keeps them (NaN is dropped under any bar)
    low = net.training_batch_frames(bank, [2], [0], None, None, max_keypoints=16, min_saliency=9.5)
    assert int(low['salient0'][0]) == 19 and 7 not in low['source0'][0].cpu().tolist()
    with pytest.raises(IndexError, match=r'idx1\[1\] = 4: the bank holds frames 0 .. 3'):
        net.training_batch_frames(bank, [0, 1], [1, 4], None, None, max_keypoints=16)
    with pytest.raises(ValueError, match='max_keypoints=2049'):
        net.training_batch_frames(bank, [0], [1], None, None, max_keypoints=2049)
    with pytest.raises(NotImplementedError, match='float64 module'):
        _net(dtype=torch.float32).training_forward_frames(bank, [0], [1], None, None, max_keypoints=16)
    # a kept all-zero FPFH row raises; the same row below the bar is never decoded
    zero = good.copy()
    zero[4, 4:] = 0.0
    kept = ops.pack_frames([zero, good], DEV)
    assert int(ops.assemble_frames_train(kept, [0], [1], 16)['range_violation']) == 1
    assert int(ops.assemble_frames_train(kept, [0], [1], 16, normalize=False)['range_violation']) == 0
    with pytest.raises(RuntimeError, match='all-zero FPFH row'):
        net.training_batch_frames(kept, [0], [1], None, None, max_keypoints=16)
    zero[4, 3] = 5.0
    zero[5, :3] = np.inf                       # and a non-finite word in a dropped record
    zero[5, 3] = 5.0
    dropped = ops.pack_frames([zero, good], DEV)
    batch = net.training_batch_frames(dropped, [0], [1], None, None, max_keypoints=16)
    assert int(batch['salient0'][0]) == 28 and int(batch['range_violation']) == 0
    # a kept row beyond the first max_keypoints is not decoded either: the truncation drops it
    late = good.copy()
    late[25, 4:] = 0.0
    assert int(ops.assemble_frames_train(ops.pack_frames([late, good], DEV), [0], [1], 16)['range_violation']) == 0
    assert int(ops.assemble_frames_train(ops.pack_frames([late, good], DEV), [0], [1], 26)['range_violation']) == 1
