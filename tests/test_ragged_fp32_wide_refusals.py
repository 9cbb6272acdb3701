"""The fp32 per-op ragged entries for WIDE slots (mdgat_attention_ragged_wide, mdgat_sinkhorn_ragged_wide, mdgat_sinkhorn_extract_ragged_wide;
ops.attention, ops.sinkhorn and ops.sinkhorn_extract with wide=True): what exists and what is refused before a device is needed.

The ABI refusals follow test_ragged_fp32_refusals.py: the "device" pointers are the address of a small host tensor that is never read,
because the call is refused (or, at B = 0, returns) first - and so that a regression can never become a launch on host pointers, those
tests are skipped where a device is present (there tests/test_gpu_ragged_sinkhorn_fp32_wide.py and test_gpu_ragged_attention_fp32_wide.py
cover the refusals)."""
import ctypes as C
import os
import re

import pytest
import torch

from mdgat_matcher_amd import MDGAT, _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = ('mdgat_set_ragged_fp32_slots', 'mdgat_attention_ragged_wide', 'mdgat_sinkhorn_ragged_wide', 'mdgat_sinkhorn_extract_ragged_wide', 'mdgat_sinkhorn_ragged_wide_workspace_bytes', 'mdgat_ragged_wide_launches')


def test_the_library_exports_every_symbol_the_wide_header_declares():
    """tests/test_host.py's check for include/mdgat_hip_wide.h and its table; the main header and its table know nothing of them"""
    hdr = open(os.path.join(ROOT, 'include', 'mdgat_hip_wide.h')).read()
    declared = set(re.findall(r'\b(mdgat_[a-z_0-9]+)\s*\(', hdr))
    assert declared == set(_lib.WIDE_SIGNATURES) == set(WIDE), declared ^ set(_lib.WIDE_SIGNATURES)
    assert not declared & set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in WIDE:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == _lib.WIDE_SIGNATURES[name][1], name


def test_every_wide_symbol_is_covered_by_a_prefilled_case_or_exempt():
    """tests/test_prefilled_table.py's rule for the wide table: an entry that takes a workspace or writes an output buffer has a case of
    tests/test_gpu_prefilled_wide.py, the others a reason from that file's list"""
    import test_gpu_prefilled_wide as PW
    import test_prefilled_table as PT
    assert not set(PW.ENTRIES) & set(PW.EXEMPT)
    assert set(PW.ENTRIES) | set(PW.EXEMPT) == set(_lib.WIDE_SIGNATURES)
    for name, (reason, what) in PW.EXEMPT.items():
        assert reason in PT.REASONS and reason != 'a timing probe' and what, name
        _, args = _lib.WIDE_SIGNATURES[name]
        assert name.endswith('_workspace_bytes') or sum(a is C.c_void_p for a in args) < 3, name
    for name, cases in PW.ENTRIES.items():
        _, args = _lib.WIDE_SIGNATURES[name]
        assert cases and args[-3:] == [C.c_void_p, C.c_size_t, C.c_void_p] and name in PW.WS_OF, name
        assert PW.WS_OF[name] in {**_lib.SIGNATURES, **_lib.WIDE_SIGNATURES}


def test_the_limits():
    hdr = open(os.path.join(ROOT, 'include', 'mdgat_hip.h')).read()
    wide = open(os.path.join(ROOT, 'include', 'mdgat_hip_wide.h')).read()
    assert re.search(r'#define MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS 2048\b', wide)
    assert re.search(r'#define MDGAT_RAGGED_FP32_MAX_KEYPOINTS 512\b', hdr) and MDGAT.RAGGED_FP32_MAX_KEYPOINTS == 512
    counters = int(re.search(r'#define MDGAT_RAGGED_WIDE_COUNTERS (\d+)', wide).group(1))
    assert counters == len(ops.RAGGED_WIDE_LAUNCHES)
    assert int(re.search(r'#define MDGAT_SINKHORN_COUNTERS (\d+)', hdr).group(1)) == 15


def test_the_workspace_holds_a_Z_and_the_split_scratch():
    lib = _lib.load()
    size = lib.mdgat_sinkhorn_ragged_wide_workspace_bytes
    assert size(2, 2048, 2048) >= 2 * 2049 * 2049 * 4 + 2 * 4 * (2 * 16 * 2048 * 2 + 2 * 2049)       # Z; 16 slabs of (max, sum), two parities; u
    assert size(2, 2049, 512) == 0 and size(2, 512, 2049) == 0 and size(0, 64, 64) == 0
    assert size(3, 128, 2048) == (3 * 129 * 2049 * 4 + 255) // 256 * 256                                 # one slab: no scratch
    # 4 slabs: 2 pairs x 2 parities x 4 x 512 granules of 8 bytes, and 2 x 2 x 513 floats of u rounded up to 256 bytes
    assert size(2, 512, 512) == lib.mdgat_sinkhorn_ragged_workspace_bytes(2, 512, 512) + 2 * 2 * 4 * 512 * 8 + 8448
    assert lib.mdgat_sinkhorn_ragged_workspace_bytes(2, 513, 512) == 0                                   # (the old query keeps its limit)


def test_the_counters_read_without_a_device():
    counts = ops.ragged_wide_launches()
    assert tuple(counts) == ops.RAGGED_WIDE_LAUNCHES and all(isinstance(v, int) and v >= 0 for v in counts.values())
    _lib.load().mdgat_ragged_wide_launches(None)          # (a null array is ignored)


def test_the_python_arguments():
    s = torch.zeros(1, 600, 16)
    with pytest.raises(ValueError, match='need counts'):
        ops.sinkhorn(s, 1.0, 2, wide=True)
    with pytest.raises(ValueError, match='needs wide=True'):
        ops.sinkhorn_extract(s, 1.0, 2, counts=([600], [16]), split=True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.sinkhorn(s, 1.0, 2, counts=([600], [16]), wide=True, split=True)
    with pytest.raises(ValueError, match='needs counts'):
        ops.attention(torch.zeros(1, 616, 3, 4, 32), 600, 16, False, wide=True)


# ---------------------------------------------------------------------------------------------- the C ABI
no_device = pytest.mark.skipif(torch.cuda.is_available(), reason='hands host addresses over as device pointers: machines without a device only')

B, NP, MP = 3, 600, 30
_KEEP = torch.zeros(64, dtype=torch.float64)
P = _KEEP.data_ptr()             # stands for every pointer that is not looked at before the refusal


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def _counts(h0, h1):
    return (P, P, None if h0 is None else h0.data_ptr(), None if h1 is None else h1.data_ptr())


def _attention(lib, b, n, m, counts, split=0, topk=0):
    return lib.mdgat_attention_ragged_wide(b, n, m, *counts, 0, topk, P, P, None, P, 1 << 40, None)


def _sinkhorn(lib, b, n, m, counts, split=0):
    return lib.mdgat_sinkhorn_ragged_wide(b, n, m, *counts, P, 1.0, 10, P, split, None, 0, None)


def _sinkhorn_extract(lib, b, n, m, counts, split=0):
    return lib.mdgat_sinkhorn_extract_ragged_wide(b, n, m, *counts, P, 1.0, 10, _lib.EXTRACT_DUSTBIN, 0.2, P, P, P, P, P, split, None, 0, None)


ENTRIES = {'mdgat_attention_ragged_wide': _attention, 'mdgat_sinkhorn_ragged_wide': _sinkhorn, 'mdgat_sinkhorn_extract_ragged_wide': _sinkhorn_extract}


@no_device
@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_count_outside_its_slot_names_the_first_pair(entry):
    lib = _lib.load()
    h0, h1 = _i32([16, 601, 9]), _i32([16, 12, 31])
    assert ENTRIES[entry](lib, B, NP, MP, _counts(h0, h1)) == _lib.ERR_BAD_ARG
    assert _lib.last_error() == f'{entry}: pair 1 has 601 x 12 keypoints, outside 1 .. 600 x 1 .. 30'


@no_device
@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_slots_beyond_2048_are_refused_before_the_counts_are_read(entry):
    lib = _lib.load()
    h0, h1 = _i32([16, 601, 0]), _i32([16, 12, 31])         # (pairs 1 and 2 are outside their slots as well: not what is reported)
    assert ENTRIES[entry](lib, B, 2049, MP, _counts(h0, h1)) == _lib.ERR_UNSUPPORTED
    assert _lib.last_error() == f'{entry}: padded sizes 2049 x 30: fp32 ragged batches hold at most 2048 keypoints per frame'
    assert ENTRIES[entry](lib, B, NP, 2049, _counts(h0, h1)) == _lib.ERR_UNSUPPORTED


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


@no_device
def test_k_beyond_a_pairs_keys():
    lib = _lib.load()
    h0, h1 = _i32([16, 600, 7]), _i32([16, 12, 30])
    assert _attention(lib, B, NP, MP, _counts(h0, h1), topk=8) == _lib.ERR_BAD_ARG
    assert _lib.last_error() == 'mdgat_attention_ragged_wide: pair 2: k=8 exceeds the number of keys (7)'


@no_device
@pytest.mark.parametrize('entry', [e for e in sorted(ENTRIES) if 'sinkhorn' in e])
def test_the_split_form_without_its_workspace_is_refused_before_a_launch(entry):
    lib = _lib.load()
    h0, h1 = _i32([16, 600, 9]), _i32([16, 12, 30])
    assert ENTRIES[entry](lib, B, NP, MP, _counts(h0, h1), split=1) == _lib.ERR_BAD_ARG
    assert _lib.last_error() == f"{entry}: the workspace (a Z where none is given, the split form's scratch) is too small or not 256-byte aligned"


# ---------------------------------------------------------------------------------------------- the module
from mdgat_matcher_amd import synth  # noqa: E402

K2 = [8, None, 8, None]


def _net(dtype=torch.float32, **over):
    cfg = synth.default_config(L=2, k=K2, sinkhorn_iterations=20, **over)
    net = MDGAT(cfg)
    net.load_state_dict(synth.make_state_dict(L=2, seed=1, descriptor=cfg['descriptor']))
    return net.to(dtype).eval()


def _pairs(counts):
    return [synth.make_batch(1, n, m, first_pair=b) for b, (n, m) in enumerate(counts)]


def test_the_key_and_the_environment(monkeypatch):
    assert MDGAT.RAGGED_FP32_WIDE_MAX_KEYPOINTS == 2048 and MDGAT.RAGGED_FP32_MAX_KEYPOINTS == 512
    assert _net().ragged_slots_fp32 == 'narrow' and _net(ragged_slots_fp32='wide').ragged_slots_fp32 == 'wide'
    with pytest.raises(ValueError, match='ragged_slots_fp32'):
        _net(ragged_slots_fp32='2048')
    monkeypatch.setenv('MDGAT_RAGGED_SLOTS_FP32', 'wide')
    assert _net().ragged_slots_fp32 == 'wide' and _net(ragged_slots_fp32='narrow').ragged_slots_fp32 == 'narrow'
    monkeypatch.setenv('MDGAT_RAGGED_SLOTS_FP32', 'broad')
    with pytest.raises(ValueError, match='ragged_slots_fp32'):
        _net()


def test_counts_up_to_2048_pass_and_2049_is_refused_before_a_device_is_needed():
    for net in (_net(ragged_arithmetic='auto', ragged_slots_fp32='wide'), _net(torch.float64, arithmetic='fp32', ragged_arithmetic='auto', ragged_slots_fp32='wide')):
        assert net._ragged_fp32()
        with pytest.raises(ValueError, match='pair 1 has 16 x 2049 keypoints: ragged batches hold at most 2048 per frame'):
            net.forward_ragged(_pairs([(16, 16), (16, 2049)]))
        with pytest.raises(ValueError, match='at most 2048 per frame'):
            net.evaluate_ragged(_pairs([(2049, 16), (16, 16)]))
        with pytest.raises(RuntimeError, match='no CPU fallback'):           # a frame of 600 passes every refusal: next it wants a device
            net.forward_ragged(_pairs([(600, 16), (16, 2048)]))
    bank = ops.pack_frames([torch.zeros(16, 37), torch.zeros(2049, 37)], device='cpu')
    with pytest.raises(ValueError, match='at most 2048 per frame'):
        _net(ragged_arithmetic='module', ragged_slots_fp32='wide').match_frames_ragged(bank, [0], [1])
    with pytest.raises(ValueError, match='pair 0 has 600 x 16 keypoints: ragged batches hold at most 512 per frame'):      # without the key: as before
        _net(ragged_arithmetic='auto').forward_ragged(_pairs([(600, 16)]))


def test_an_exact_module_ignores_the_key():
    net = _net(torch.float64, ragged_arithmetic='auto', ragged_slots_fp32='wide')
    assert net.exact() and not net._ragged_fp32()
    with pytest.raises(ValueError, match='pair 0 has 576 x 16 keypoints: ragged batches hold at most 575'):
        net.forward_ragged(_pairs([(576, 16), (16, 16)]))
