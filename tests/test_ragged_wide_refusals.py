"""Ragged batches beyond 575 keypoints (the streaming fp64 Sinkhorn with per-pair counts): what the new C entries and
config['ragged_sinkhorn'] accept and refuse before anything touches a device.

The "device" pointers handed to the C entries are the address of a small host tensor.  They are never read, because the call is refused
(or, at B = 0, returns) first - and so that a regression can never become a launch on host pointers, those tests are skipped where a device
is present (there tests/test_gpu_ragged_sinkhorn_stream.py covers the same refusals), as tests/test_ragged_counts_abi.py is."""
import pytest
import torch

from mdgat_matcher_amd import MDGAT, _lib, synth

no_device = pytest.mark.skipif(torch.cuda.is_available(), reason='hands host addresses over as device pointers: machines without a device only')

_KEEP = torch.zeros(64, dtype=torch.float64)
P = _KEEP.data_ptr()             # stands for every pointer that is not looked at before the refusal
K = [8, None, 8, None]


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def _counts(h0, h1):
    return (P, P, h0.data_ptr(), h1.data_ptr())


def _sinkhorn(lib, b, n, m, counts):
    return lib.mdgat_sinkhorn_f64_stream_ragged(b, n, m, *counts, P, 1.0, 10, P, None, 0, None)


def _sinkhorn_extract(lib, b, n, m, counts):
    return lib.mdgat_sinkhorn_f64_extract_stream_ragged(b, n, m, *counts, P, 1.0, 10, _lib.EXTRACT_DUSTBIN, 0.2, P, P, P, P, None, None, 0, None)


ENTRIES = {'mdgat_sinkhorn_f64_stream_ragged': _sinkhorn, 'mdgat_sinkhorn_f64_extract_stream_ragged': _sinkhorn_extract}


def test_the_library_exports_the_new_entries():
    lib = _lib.load()
    for name in ('mdgat_sinkhorn_f64_stream_ragged_workspace_bytes', 'mdgat_sinkhorn_f64_stream_ragged', 'mdgat_sinkhorn_f64_extract_stream_ragged',
                 'mdgat_set_ragged_sinkhorn'):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_workspace_bytes_follow_the_slot_and_are_zero_for_an_unsupported_one():
    size = _lib.load().mdgat_sinkhorn_f64_stream_ragged_workspace_bytes
    assert size(1, 2176, 8) == 0 and size(1, 8, 2176) == 0 and size(0, 64, 64) == 0 and size(1, 0, 64) == 0
    # K alone is [B][Np][Mp rounded up to 128] doubles: 35.6 MB per pair in slots of 2048, and small slots are served too
    assert size(1, 2048, 2048) >= 2048 * 2176 * 8 and size(1, 2048, 2048) < 2 * 2048 * 2176 * 8
    assert size(16, 2048, 2048) >= 16 * 2048 * 2176 * 8
    assert size(3, 16, 16) >= 3 * 16 * 128 * 8
    assert size(1, 2175, 2175) > 0


@no_device
@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_slots_beyond_2175_are_refused_before_the_counts_are_read(entry):
    lib = _lib.load()
    h = _i32([8])
    assert ENTRIES[entry](lib, 1, 2176, 8, _counts(h, h)) == _lib.ERR_UNSUPPORTED
    assert _lib.last_error() == f'{entry}: padded sizes 2176 x 8: the streaming form holds at most 2175 keypoints per frame'
    assert ENTRIES[entry](lib, 1, 8, 2176, _counts(h, h)) == _lib.ERR_UNSUPPORTED
    assert _lib.last_error() == f'{entry}: padded sizes 8 x 2176: the streaming form holds at most 2175 keypoints per frame'


@no_device
@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_a_bad_count_names_the_first_offending_pair(entry):
    lib = _lib.load()
    h0, h1 = _i32([16, 701, 9]), _i32([16, 12, 801])           # (kept alive over the call: the entry reads them through raw pointers)
    rc = ENTRIES[entry](lib, 3, 700, 800, _counts(h0, h1))
    assert rc == _lib.ERR_BAD_ARG
    assert _lib.last_error() == f'{entry}: pair 1 has 701 x 12 keypoints, outside 1 .. 700 x 1 .. 800'
    h0, h1 = _i32([16, 700, 9]), _i32([16, 12, 0])
    rc = ENTRIES[entry](lib, 3, 700, 800, _counts(h0, h1))
    assert rc == _lib.ERR_BAD_ARG
    assert _lib.last_error() == f'{entry}: pair 2 has 9 x 0 keypoints, outside 1 .. 700 x 1 .. 800'
    assert ENTRIES[entry](lib, 3, 700, 800, (P, P, None, None)) == _lib.ERR_BAD_ARG
    assert _lib.last_error() == f'{entry}: null counts pointer'


@no_device
@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_an_empty_batch_is_ok_and_good_counts_get_as_far_as_the_workspace(entry):
    lib = _lib.load()
    h0, h1 = _i32([600, 40, 64]), _i32([40, 610, 64])
    assert ENTRIES[entry](lib, 0, 600, 610, _counts(h0, h1)) == _lib.OK
    assert ENTRIES[entry](lib, 3, 600, 610, _counts(h0, h1)) == _lib.ERR_BAD_ARG           # (no workspace was handed over)
    assert _lib.last_error() == f'{entry}: workspace too small or not 256-byte aligned'


def test_set_ragged_sinkhorn_refuses_a_null_handle():
    assert _lib.load().mdgat_set_ragged_sinkhorn(None, 1) == -1
    assert 'mdgat_set_ragged_sinkhorn' in _lib.last_error()


# ---------------------------------------------------------------------------------------------------- config['ragged_sinkhorn']
def _net(dtype=torch.float64, **over):
    cfg = synth.default_config(L=2, k=K, sinkhorn_iterations=20, **over)
    net = MDGAT(cfg)
    net.load_state_dict(synth.make_state_dict(L=2, seed=1))
    return net.to(dtype).eval()


def _h(n, m):
    return _i32([16, n]), _i32([16, m])


def test_the_three_values_are_accepted_and_a_fourth_is_not():
    assert _net().ragged_sinkhorn == 'resident' and not _net()._ragged_wide()
    for value in ('resident', 'auto', 'streaming'):
        net = _net(ragged_sinkhorn=value)
        assert net.ragged_sinkhorn == value and net._ragged_wide() is (value != 'resident')
    for value in ('wide', 'Auto', 'stream', '1'):
        with pytest.raises(ValueError, match='ragged_sinkhorn'):
            _net(ragged_sinkhorn=value)
    assert MDGAT.RAGGED_WIDE_MAX_KEYPOINTS == 2048 and MDGAT.RAGGED_MAX_KEYPOINTS == 575


def test_the_environment_stands_in_for_modules_without_the_key(monkeypatch):
    monkeypatch.setenv('MDGAT_RAGGED_SINKHORN', 'auto')
    assert _net().ragged_sinkhorn == 'auto' and _net()._ragged_wide()
    assert _net(ragged_sinkhorn='resident').ragged_sinkhorn == 'resident'
    assert _net(ragged_sinkhorn='streaming').ragged_sinkhorn == 'streaming'
    monkeypatch.setenv('MDGAT_RAGGED_SINKHORN', 'garbage')
    with pytest.raises(ValueError, match='ragged_sinkhorn'):
        _net()


@pytest.mark.parametrize('value', ['auto', 'streaming'])
def test_an_exact_module_that_opted_in_takes_2048_keypoints_per_frame(value):
    net = _net(ragged_sinkhorn=value)
    net._ragged_counts_checked(*_h(576, 16), 576, 16)
    net._ragged_counts_checked(*_h(2048, 2048), 2048, 2048)
    with pytest.raises(ValueError, match='pair 1 has 2049 x 16 keypoints: ragged batches hold at most 2048 per frame'):
        net._ragged_counts_checked(*_h(2049, 16), 2049, 16)
    with pytest.raises(ValueError, match='pair 1 has 16 x 2049 keypoints: ragged batches hold at most 2048 per frame'):
        net._ragged_counts_checked(*_h(16, 2049), 16, 2049)
    with pytest.raises(ValueError, match='slots of 2049 x 16 keypoints: ragged batches hold at most 2048 per frame'):
        net._ragged_counts_checked(*_h(16, 16), 2049, 16)
    # ... and then wants a device like every other ragged call
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net.forward_ragged([synth.make_batch(1, n, m, first_pair=b) for b, (n, m) in enumerate([(600, 16), (16, 16)])])


def test_without_the_key_576_is_refused_as_before():
    with pytest.raises(ValueError, match='pair 1 has 576 x 16 keypoints: ragged batches hold at most 575 per frame'):
        _net()._ragged_counts_checked(*_h(576, 16), 576, 16)
    with pytest.raises(ValueError, match='pair 1 has 576 x 16 keypoints: ragged batches hold at most 575 per frame'):
        _net(ragged_sinkhorn='resident')._ragged_counts_checked(*_h(576, 16), 576, 16)


def test_an_fp32_class_module_ignores_the_key():
    """its ragged calls run the fp32-class branch (ragged_arithmetic): no fp64 Sinkhorn, the limit of 512"""
    for net in (_net(torch.float32, ragged_arithmetic='auto', ragged_sinkhorn='auto'),
                _net(torch.float64, arithmetic='fp32', ragged_arithmetic='auto', ragged_sinkhorn='streaming')):
        assert net._ragged_fp32() and not net._ragged_wide()
        net._ragged_counts_checked(*_h(512, 16), 512, 16)
        with pytest.raises(ValueError, match='pair 1 has 513 x 16 keypoints: ragged batches hold at most 512 per frame'):
            net._ragged_counts_checked(*_h(513, 16), 513, 16)
    # and one that is not exact and did not opt into the fp32-class branch is refused as before, whatever the key says
    with pytest.raises(NotImplementedError, match='exact mode only'):
        _net(torch.float32, ragged_sinkhorn='auto').forward_ragged([synth.make_batch(1, 16, 16, first_pair=0)])
