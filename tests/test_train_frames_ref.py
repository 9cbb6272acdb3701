"""tests/train_frames_ref.py - the host restatement of the loader's train-mode assembly - against the reference loader's own outputs
(tests/golden/train_loader.npz, tools/make_goldens_train_loader.py) bit for bit, and its closed-form slot map against a literal run of the
loader's prepend loop.  Also that the golden covers the branches it was drawn for, and that the library exports the new entry."""
import numpy as np
import pytest
import torch

import train_frames_ref as R
from conftest import GOLDEN


def test_slot_map_is_the_prepend_loop():
    for T in range(1, 71):
        for v in range(1, T + 1):
            assert np.array_equal(R.slot_map(v, T), R.prepend_loop(v, T)), (v, T)
        assert np.array_equal(R.slot_map(T + 5, T), np.arange(T))
    assert R.slot_map(3, 8).tolist() == [0, 1, 0, 1, 2, 0, 1, 2]
    # the deepest case the library takes: eleven steps
    assert np.array_equal(R.slot_map(1, 2048), np.zeros(2048, dtype=np.int64)) and np.array_equal(R.slot_map(3, 2048), R.prepend_loop(3, 2048))


def test_restatement_equals_the_loader_bit_for_bit():
    g, sets = R.load_golden(GOLDEN)
    n_items = 0
    for name, s in sets.items():
        for j, pair in enumerate(s['pairs']):
            for f in (0, 1):
                got = R.assemble_frame(s['rec'][pair[f]], s['T'], float(g['min_saliency']))
                want = R.loader_inputs(g, name, j, f)
                for k, w in want.items():
                    assert got[k].dtype == np.float64 and got[k].shape == w.shape and np.array_equal(got[k], w), (name, j, f, k)
                assert np.array_equal(got['keypoints_f32'].astype(np.float64), want['keypoints'])
                # source names the record behind every slot
                assert np.array_equal(s['rec'][pair[f]][got['source'], :4].astype(np.float64), np.column_stack([want['keypoints'], want['scores']]))
            n_items += 1
    assert n_items == 7


def test_golden_covers_every_branch():
    g, sets = R.load_golden(GOLDEN)
    thr = np.float32(g['min_saliency'])
    kept = {name: {i: len(R.kept_rows(r, thr)) for i, r in s['rec'].items()} for name, s in sets.items()}
    T = sets['t40']['T']
    v = sorted(kept['t40'].values())
    assert T == 40 and any(x > T for x in v) and T in v and any(T / 2 <= x < T for x in v) and 7 in v and 1 in v and T // 2 in v
    assert any(len(r) >= 150 and kept['t40'][i] > T for i, r in sets['t40']['rec'].items())         # more than two waves of records
    assert sets['t64']['T'] == 64 and {64, 63, 33} <= set(kept['t64'].values())
    shared = [i for i in sets['t40']['frames'] if sum(i in p for p in sets['t40']['pairs']) > 1]
    assert shared, 'no frame serves two pairs'
    rec = np.concatenate(list(sets['t40']['rec'].values()))
    s = rec[:, 3]
    assert (s == thr).any() and np.isnan(s).any() and (s == np.nextafter(thr, np.float32(np.inf))).any()
    with np.errstate(invalid='ignore'):
        dropped = rec[~(s > thr)]
    assert (dropped[:, 4:] == 0).all(axis=1).any() and np.isnan(dropped[:, :3]).any()      # what dropped records hold is not looked at
    # padded frames are full of duplicates: the ground truth there is decided by the first-minimum rule
    assert any(int(g[f't40_item{j}_rep']) == T for j in range(5))


def test_a_frame_that_keeps_nothing_is_refused():
    rec = np.ones((5, 37), dtype=np.float32)
    rec[:, 3] = [10.0, 3.0, np.nan, -1.0, 9.999]
    with pytest.raises(ValueError, match='no record with saliency above'):
        R.assemble_frame(rec, 8)
    rec[1, 3] = np.inf
    assert R.assemble_frame(rec, 8)['source'].tolist() == [1] * 8


def test_the_train_assembly_entry_is_exported():
    import os
    import re
    from mdgat_matcher_amd import MDGAT, _lib, ops
    lib = _lib.load()
    name = 'mdgat_assemble_frames_train_f64'
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    hdr = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'mdgat_hip.h')).read()
    assert re.search(r'\bint ' + name + r'\s*\(', hdr)
    assert callable(ops.assemble_frames_train) and callable(MDGAT.training_batch_frames) and callable(MDGAT.training_forward_frames)


@pytest.mark.skipif(torch.cuda.is_available(), reason='hands host addresses over as device pointers: machines without a device only')
def test_the_train_assembly_entry_refuses_on_the_host_copies():
    """Every refusal is made before HIP is touched, as in tests/test_ragged_counts_abi.py (and skipped where a device is present for the
    same reason: a regression must never become a launch on host pointers; there the GPU tests cover the refusals)."""
    import ctypes as C
    from mdgat_matcher_amd import _lib
    lib = _lib.load()
    name = 'mdgat_assemble_frames_train_f64'
    keep = (C.c_double * 8)()
    P = C.addressof(keep)             # stands for every pointer that is not looked at before the refusal
    h = torch.tensor([5, 7], dtype=torch.int32)
    s = torch.tensor([0, 5], dtype=torch.int64)

    def call(B, T, h0=h, h1=h, s0=s, s1=s, rows=12, thr=10.0):
        return lib.mdgat_assemble_frames_train_f64(B, T, P, P, h0.data_ptr(), h1.data_ptr(), P, P, s0.data_ptr(), s1.data_ptr(), P, rows, P, rows, thr, 1,
                                                   P, P, P, P, P, P, P, P, P, None, None)
    assert call(2, 2049) == _lib.ERR_BAD_ARG
    assert _lib.last_error() == f'{name}: max_keypoints=2049: at most 2048 keypoints per frame (the attention\'s limit)'
    assert call(2, 0) == _lib.ERR_BAD_ARG
    assert call(2, 40, rows=11) == _lib.ERR_BAD_ARG
    assert _lib.last_error() == f'{name}: pair 1 reads records 5 .. 12 of 11 and 5 .. 12 of 11: outside the bank'
    assert call(2, 40, h0=torch.tensor([5, 0], dtype=torch.int32)) == _lib.ERR_BAD_ARG
    assert _lib.last_error().startswith(f'{name}: pair 1 has 0 x 7 keypoints')
    assert call(2, 40, thr=float('nan')) == _lib.ERR_BAD_ARG
    assert call(0, 40) == _lib.OK            # an empty chunk launches nothing


def test_python_refusals_need_no_device():
    from mdgat_matcher_amd import MDGAT, ops, synth
    rs = np.random.RandomState(0)
    bank = ops.pack_frames([rs.standard_normal((n, 37)).astype(np.float32) for n in (6, 0, 9)], 'cpu')
    with pytest.raises(ValueError, match='max_keypoints=2049'):
        ops.assemble_frames_train(bank, [0], [2], 2049)
    with pytest.raises(ValueError, match='max_keypoints=0'):
        ops.assemble_frames_train(bank, [0], [2], 0)
    with pytest.raises(ValueError, match='empty chunk'):
        ops.assemble_frames_train(bank, [], [], 40)
    with pytest.raises(ValueError, match='pair 1: frame 1 holds no record'):
        ops.assemble_frames_train(bank, [0, 2], [2, 1], 40)
    with pytest.raises(IndexError, match='idx1\\[0\\] = 3'):
        ops.assemble_frames_train(bank, [0], [3], 40)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.assemble_frames_train(bank, [0], [2], 40)
    net = MDGAT(synth.default_config(L=1, k=[4, None]))
    with pytest.raises(NotImplementedError, match='float64 module'):
        net.training_forward_frames(bank, [0], [2], None, None, max_keypoints=8)
