"""The fp32-class ragged forward (config['ragged_arithmetic'] = 'auto') and its per-op entries: what they refuse before they need a device.

The module-level refusals run on CPU tensors and are raised before anything looks for a device.  The ABI refusals follow
test_ragged_counts_abi.py: the "device" pointers are the address of a small host tensor that is never read, because the call is refused (or,
at B = 0, returns) first - and so that a regression can never become a launch on host pointers, those tests are skipped where a device is
present (there the GPU tests of the same entries cover the refusals)."""
import pytest
import torch

from mdgat_matcher_amd import MDGAT, _lib, ops, synth

K = [8, None, 8, None]


def _net(dtype=torch.float32, **over):
    cfg = synth.default_config(L=2, k=K, sinkhorn_iterations=20, **over)
    net = MDGAT(cfg)
    net.load_state_dict(synth.make_state_dict(L=2, seed=1, descriptor=cfg['descriptor']))
    return net.to(dtype).eval()


def _pairs(counts):
    return [synth.make_batch(1, n, m, first_pair=b) for b, (n, m) in enumerate(counts)]


PAIRS = [(16, 16), (20, 12)]


def test_without_the_key_a_float32_module_is_still_refused():
    for net in (_net(), _net(torch.float64, arithmetic='fp32')):
        assert not net._ragged_fp32()
        with pytest.raises(NotImplementedError, match='exact mode only'):
            net.forward_ragged(_pairs(PAIRS))


def test_the_environment_stands_in_for_modules_without_the_key(monkeypatch):
    monkeypatch.setenv('MDGAT_RAGGED_ARITHMETIC', 'auto')
    assert _net()._ragged_fp32()
    assert not _net(ragged_arithmetic='exact')._ragged_fp32()
    with pytest.raises(ValueError, match='ragged_arithmetic'):
        _net(ragged_arithmetic='fp32')


def test_with_the_key_the_module_gets_as_far_as_the_device():
    """a float32 module that opted in passes every refusal; on CPU tensors the next thing it wants is a device"""
    for net in (_net(ragged_arithmetic='auto'), _net(torch.float64, arithmetic='fp32', ragged_arithmetic='auto'),
                _net(ragged_arithmetic='auto', descriptor='FPFH_only')):
        assert net._ragged_fp32()
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            net.forward_ragged(_pairs(PAIRS))


def test_an_exact_module_with_the_key_stays_exact():
    net = _net(torch.float64, ragged_arithmetic='auto')
    assert net.exact() and not net._ragged_fp32()
    with pytest.raises(ValueError, match='pair 0 has 576 x 16 keypoints: ragged batches hold at most 575'):
        net.forward_ragged(_pairs([(576, 16), (16, 16)]))


def test_more_than_512_keypoints():
    net = _net(ragged_arithmetic='auto')
    with pytest.raises(ValueError, match='pair 1 has 16 x 513 keypoints: ragged batches hold at most 512 per frame'):
        net.forward_ragged(_pairs([(16, 16), (16, 513)]))
    with pytest.raises(ValueError, match='at most 512 per frame'):
        net.evaluate_ragged(_pairs([(513, 16), (16, 16)]))


def test_a_count_below_a_layers_k():
    net = _net(ragged_arithmetic='auto')
    with pytest.raises(ValueError, match='pair 1 has 20 x 7 keypoints: fewer than a dynamic layer keeps'):
        net.forward_ragged(_pairs([(16, 16), (20, 7), (9, 9)]))


def test_the_pooled_descriptor_is_not_implemented():
    net = _net(ragged_arithmetic='auto', descriptor='FPFH_gloabal')
    with pytest.raises(NotImplementedError, match="'FPFH_gloabal'"):
        net.forward_ragged(_pairs(PAIRS))


def test_single_f16_attention_is_not_implemented():
    net = _net(ragged_arithmetic='auto', attention_dtype='f16')
    with pytest.raises(NotImplementedError, match="attention_dtype='fp32'"):
        net.forward_ragged(_pairs(PAIRS))


def test_train_mode_and_the_evaluation_loss_are_not_implemented():
    for net in (_net(ragged_arithmetic='auto').train(), _net(ragged_arithmetic='auto', eval_loss=True)):
        with pytest.raises(NotImplementedError, match='eval\\(\\) mode, without the evaluation loss'):
            net.forward_ragged(_pairs(PAIRS))


def test_the_bank_entries_keep_refusing_an_fp32_class_module():
    net = _net(ragged_arithmetic='auto')
    bank = ops.pack_frames([torch.zeros(16, 37), torch.zeros(20, 37)], device='cpu')
    with pytest.raises(NotImplementedError, match='exact mode only'):
        net.match_frames_ragged(bank, [0], [1])


# ---------------------------------------------------------------------------------------------- the C ABI
no_device = pytest.mark.skipif(torch.cuda.is_available(), reason='hands host addresses over as device pointers: machines without a device only')

B, NP, MP = 3, 20, 30
_KEEP = torch.zeros(64, dtype=torch.float64)
P = _KEEP.data_ptr()             # stands for every pointer that is not looked at before the refusal


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def _counts(h0, h1):
    """the four leading pointers of every ragged entry: device counts (never read), host counts"""
    return (P, P, None if h0 is None else h0.data_ptr(), None if h1 is None else h1.data_ptr())


def _attention(lib, b, n, m, counts, topk=0):
    return lib.mdgat_attention_ragged(b, n, m, *counts, 0, topk, P, P, None, P, 1 << 40, None)


def _sinkhorn(lib, b, n, m, counts):
    return lib.mdgat_sinkhorn_ragged(b, n, m, *counts, P, 1.0, 10, P, None)


def _sinkhorn_extract(lib, b, n, m, counts):
    return lib.mdgat_sinkhorn_extract_ragged(b, n, m, *counts, P, 1.0, 10, _lib.EXTRACT_DUSTBIN, 0.2, P, P, P, P, P, None, 0, None)


ENTRIES = {
    'mdgat_attention_ragged': _attention,
    'mdgat_sinkhorn_ragged': _sinkhorn,
    'mdgat_sinkhorn_extract_ragged': _sinkhorn_extract,
}


def test_the_library_exports_the_fp32_ragged_entries():
    lib = _lib.load()
    for name in (*ENTRIES, 'mdgat_forward_ragged', 'mdgat_sinkhorn_ragged_workspace_bytes'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.mdgat_sinkhorn_ragged_workspace_bytes(2, 512, 512) >= 2 * 513 * 513 * 4
    assert lib.mdgat_sinkhorn_ragged_workspace_bytes(2, 513, 512) == 0


@no_device
@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_count_outside_its_slot_names_the_first_pair(entry):
    lib = _lib.load()
    h0, h1 = _i32([16, 21, 9]), _i32([16, 12, 30])
    assert ENTRIES[entry](lib, B, NP, MP, _counts(h0, h1)) == _lib.ERR_BAD_ARG
    assert _lib.last_error() == f'{entry}: pair 1 has 21 x 12 keypoints, outside 1 .. 20 x 1 .. 30'


@no_device
def test_k_beyond_a_pairs_keys():
    lib = _lib.load()
    h0, h1 = _i32([16, 20, 7]), _i32([16, 12, 30])
    assert _attention(lib, B, NP, MP, _counts(h0, h1), topk=8) == _lib.ERR_BAD_ARG
    assert _lib.last_error() == 'mdgat_attention_ragged: pair 2: k=8 exceeds the number of keys (7)'
    assert _attention(lib, 0, NP, MP, _counts(h0, h1), topk=7) == _lib.OK


@no_device
@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_slots_beyond_512_are_refused_before_the_counts_are_read(entry):
    lib = _lib.load()
    h0, h1 = _i32([16, 21, 0]), _i32([16, 12, 31])         # (pairs 1 and 2 are outside their slots as well: not what is reported)
    assert ENTRIES[entry](lib, B, 513, MP, _counts(h0, h1)) == _lib.ERR_UNSUPPORTED
    assert _lib.last_error() == f'{entry}: padded sizes 513 x 30: fp32 ragged batches hold at most 512 keypoints per frame'


@no_device
@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_null_host_counts(entry):
    lib = _lib.load()
    assert ENTRIES[entry](lib, B, NP, MP, _counts(None, _i32([16, 12, 30]))) == _lib.ERR_BAD_ARG
    assert _lib.last_error() == f'{entry}: null counts pointer'


@no_device
@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_empty_batch_launches_nothing(entry):
    lib = _lib.load()
    h0, h1 = _i32([16, 20, 9]), _i32([16, 12, 30])
    assert ENTRIES[entry](lib, 0, NP, MP, _counts(h0, h1)) == _lib.OK
