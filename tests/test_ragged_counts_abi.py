"""The per-pair checks of a ragged batch at the C ABI (csrc/ragged.hpp: mdgat_check_ragged), on a machine without a device: every
handle-free ragged entry refuses bad counts on their host copies before it touches HIP, with one return code and one text.

The "device" pointers handed over here are the address of a small host tensor.  They are never read, because the call is refused (or,
at B = 0, returns) first - and so that a regression can never become a launch on host pointers, the whole module is skipped where a
device is present (there the GPU tests of the ragged entries cover the same refusals)."""
import pytest
import torch

from mdgat_matcher_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason='hands host addresses over as device pointers: machines without a device only')

B, NP, MP = 3, 20, 30
_KEEP = torch.zeros(64, dtype=torch.float64)
P = _KEEP.data_ptr()             # stands for every pointer that is not looked at before the refusal


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def _i64(v):
    return torch.tensor(v, dtype=torch.int64)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _counts(h0, h1):
    """the four leading pointers of every ragged entry: device counts (never read), host counts"""
    return (P, P, _ptr(h0), _ptr(h1))


# entry -> the arguments behind (B, Np, Mp, *counts) that get the call as far as the counts
def _gt_matches(lib, b, n, m, counts):
    return lib.mdgat_gt_matches_ragged(b, n, m, *counts, P, P, None, None, 0.5, 0, P, P, P, None)


def _eval_metrics(lib, b, n, m, counts):
    return lib.mdgat_eval_metrics_ragged(b, n, m, *counts, P, P, P, P, P, P, None, 1.0, P, P, P, None)


def _attention(lib, b, n, m, counts, topk=0):
    return lib.mdgat_attention_f64_ragged(b, n, m, *counts, 0, topk, P, P, None, None)


def _sinkhorn(lib, b, n, m, counts):
    return lib.mdgat_sinkhorn_f64_ragged(b, n, m, *counts, P, 1.0, 10, P, None, 0, None)


def _sinkhorn_extract(lib, b, n, m, counts):
    return lib.mdgat_sinkhorn_f64_extract_ragged(b, n, m, *counts, P, 1.0, 10, _lib.EXTRACT_DUSTBIN, 0.2, P, P, P, P, None, None, 0, None)


def _assemble(lib, b, n, m, counts, starts=None, rows=(1000, 1000)):
    s0, s1 = starts if starts is not None else (_i64([0] * max(b, 1)), _i64([0] * max(b, 1)))
    return lib.mdgat_assemble_frames_f64_ragged(b, n, m, *counts, P, P, _ptr(s0), _ptr(s1), P, rows[0], P, rows[1], 1, P, P, None, None, None, None)


ENTRIES = {
    'mdgat_gt_matches_ragged': _gt_matches,
    'mdgat_eval_metrics_ragged': _eval_metrics,
    'mdgat_attention_f64_ragged': _attention,
    'mdgat_sinkhorn_f64_ragged': _sinkhorn,
    'mdgat_sinkhorn_f64_extract_ragged': _sinkhorn_extract,
    'mdgat_assemble_frames_f64_ragged': _assemble,
}


@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_count_outside_its_slot_names_the_first_pair(entry):
    lib = _lib.load()
    h0, h1 = _i32([16, 21, 9]), _i32([16, 12, 30])
    rc = ENTRIES[entry](lib, B, NP, MP, _counts(h0, h1))
    assert rc == _lib.ERR_BAD_ARG
    assert _lib.last_error() == f'{entry}: pair 1 has 21 x 12 keypoints, outside 1 .. 20 x 1 .. 30'


def test_k_beyond_a_pairs_keys():
    lib = _lib.load()
    h0, h1 = _i32([16, 20, 7]), _i32([16, 12, 30])
    assert _attention(lib, B, NP, MP, _counts(h0, h1), topk=8) == _lib.ERR_BAD_ARG
    assert _lib.last_error() == 'mdgat_attention_f64_ragged: pair 2: k=8 exceeds the number of keys (7)'
    assert _attention(lib, 0, NP, MP, _counts(h0, h1), topk=7) == _lib.OK


def test_slots_beyond_the_resident_sinkhorn_are_refused_before_the_counts_are_read():
    lib = _lib.load()
    h0, h1 = _i32([16, 21, 0]), _i32([16, 12, 31])         # (pair 2 is outside its slot as well: not what is reported)
    assert _sinkhorn(lib, B, 576, MP, _counts(h0, h1)) == _lib.ERR_UNSUPPORTED
    assert _lib.last_error() == 'mdgat_sinkhorn_f64_ragged: padded sizes 576 x 30: ragged batches hold at most 575 keypoints per frame'
    assert _sinkhorn_extract(lib, B, 576, MP, _counts(h0, h1)) == _lib.ERR_UNSUPPORTED
    assert _lib.last_error() == 'mdgat_sinkhorn_f64_extract_ragged: padded sizes 576 x 30: ragged batches hold at most 575 keypoints per frame'


def test_records_outside_the_bank():
    lib = _lib.load()
    h0, h1 = _i32([16, 20, 7]), _i32([16, 12, 30])
    starts = (_i64([0, 16, 36]), _i64([0, 16, 28]))
    assert _assemble(lib, B, NP, MP, _counts(h0, h1), starts, rows=(42, 100)) == _lib.ERR_BAD_ARG
    assert _lib.last_error() == 'mdgat_assemble_frames_f64_ragged: pair 2 reads records 36 .. 43 of 42 and 28 .. 58 of 100: outside the bank'
    # a count outside its slot comes first, pair by pair
    wide = _i32([16, 21, 7])
    assert _assemble(lib, B, NP, MP, _counts(wide, h1), starts, rows=(42, 100)) == _lib.ERR_BAD_ARG
    assert _lib.last_error() == 'mdgat_assemble_frames_f64_ragged: pair 1 has 21 x 12 keypoints, outside 1 .. 20 x 1 .. 30'


@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_null_host_counts(entry):
    lib = _lib.load()
    h1 = _i32([16, 12, 30])
    assert ENTRIES[entry](lib, B, NP, MP, _counts(None, h1)) == _lib.ERR_BAD_ARG


@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_empty_batch_launches_nothing(entry):
    lib = _lib.load()
    h0, h1 = _i32([16, 20, 9]), _i32([16, 12, 30])
    assert ENTRIES[entry](lib, 0, NP, MP, _counts(h0, h1)) == _lib.OK
