"""ops.pack_frames / ops.frames_chunk and MDGAT.match_frames_ragged: what needs no device."""
import numpy as np
import pytest
import torch

from mdgat_matcher_amd import MDGAT, _lib, ops, synth


def _frames(counts, seed=0, dtype=np.float32):
    rs = np.random.RandomState(seed)
    return [rs.standard_normal((n, 37)).astype(dtype) for n in counts]


def test_pack_frames_starts_and_counts_with_an_empty_frame():
    frames = _frames([5, 0, 3, 7])
    frames[2] = torch.from_numpy(frames[2])            # numpy and torch frames side by side
    bank = ops.pack_frames(frames, 'cpu')
    assert bank['counts'].dtype == torch.int32 and bank['counts'].tolist() == [5, 0, 3, 7]
    assert bank['starts'].dtype == torch.int64 and bank['starts'].tolist() == [0, 5, 5, 8]
    rec = bank['records']
    assert rec.dtype == torch.float32 and tuple(rec.shape) == (15, 37) and rec.is_contiguous()
    for i, f in enumerate(frames):
        a, n = int(bank['starts'][i]), int(bank['counts'][i])
        assert torch.equal(rec[a:a + n], torch.as_tensor(f))
    # what np.fromfile(...).reshape(-1, 37) gives for an empty file is a frame like any other
    only_empty = ops.pack_frames([np.zeros((0, 37), np.float32)], 'cpu')
    assert only_empty['counts'].tolist() == [0] and tuple(only_empty['records'].shape) == (0, 37)


def test_pack_frames_refuses_another_record_width():
    frames = _frames([4, 6])
    with pytest.raises(ValueError, match='frame 1 has shape \\(6, 36\\)'):
        ops.pack_frames([frames[0], frames[1][:, :36]], 'cpu')
    with pytest.raises(ValueError, match='frame 0 has shape \\(148,\\)'):
        ops.pack_frames([frames[0].reshape(-1)], 'cpu')
    with pytest.raises(ValueError, match='no frames'):
        ops.pack_frames([], 'cpu')


def test_pack_frames_narrows_float64_to_float32():
    frames = _frames([4, 6], dtype=np.float64)
    bank = ops.pack_frames(frames, 'cpu')
    assert bank['records'].dtype == torch.float32
    assert np.array_equal(bank['records'].numpy(), np.concatenate(frames).astype(np.float32))


def test_frames_chunk_gathers_counts_and_starts():
    bank = ops.pack_frames(_frames([5, 0, 3, 7]), 'cpu')
    (h0, h1), (s0, s1) = ops.frames_chunk(bank, [3, 0, 0], np.array([2, 2, 1]))
    assert h0.dtype == torch.int32 and h0.tolist() == [7, 5, 5] and h1.tolist() == [3, 3, 0]
    assert s0.dtype == torch.int64 and s0.tolist() == [8, 0, 0] and s1.tolist() == [5, 5, 5]


def _net(dtype=torch.float64):
    cfg = synth.default_config(L=2, k=[8, None, 8, None], sinkhorn_iterations=20)
    net = MDGAT(cfg)
    net.load_state_dict(synth.make_state_dict(L=2, seed=1))
    return net.to(dtype).eval()


def test_match_frames_ragged_checks_the_indices_before_any_device():
    bank = ops.pack_frames(_frames([16, 20, 12]), 'cpu')
    net = _net()
    with pytest.raises(IndexError, match='idx1\\[1\\] = 3: the bank holds frames 0 .. 2'):
        net.match_frames_ragged(bank, [0, 1], [2, 3])
    with pytest.raises(IndexError, match='idx0\\[0\\] = -1'):
        net.match_frames_ragged(bank, [-1, 1], [2, 0])
    with pytest.raises(ValueError, match='idx0 holds 2 frames, idx1 3'):
        net.match_frames_ragged(bank, [0, 1], [2, 0, 1])
    with pytest.raises(ValueError, match='idx0 holds 2 frames, idx1 3'):
        net.evaluate_frames_ragged(bank, [0, 1], [2, 0, 1], None, None)
    # the indices are good: the next refusals are forward_ragged's own
    with pytest.raises(ValueError, match='pair 1 has 20 x 7 keypoints: fewer than a dynamic layer keeps'):
        net.match_frames_ragged(ops.pack_frames(_frames([16, 20, 7]), 'cpu'), [0, 1], [1, 2])
    with pytest.raises(NotImplementedError, match='exact mode only'):
        _net(torch.float32).match_frames_ragged(bank, [0], [1])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net.match_frames_ragged(bank, [0], [1])


def test_the_new_entries_are_exported_by_the_built_library():
    lib = _lib.load()
    for name in ('mdgat_forward_frames_ragged', 'mdgat_assemble_frames_f64_ragged', 'mdgat_gt_matches_ragged'):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert callable(ops.pack_frames) and callable(ops.assemble_frames_ragged)
