"""CPU tests of tests/prefilled.py, and the table that keeps the prefilled GPU tests complete: every symbol of ``_lib.SIGNATURES`` is
either covered by named cases of tests/test_gpu_prefilled_ops.py / test_gpu_prefilled_forward.py (``ENTRIES``) or exempt for a stated
reason (``EXEMPT``).  An entry added to the library without a case - or without a reason - fails here, without a GPU."""
import ctypes as C

import pytest
import torch

import prefilled as P
from mdgat_matcher_amd import _lib

OPS, FWD = 'test_gpu_prefilled_ops', 'test_gpu_prefilled_forward'

# C symbol -> the cases that cover it: '<module>::<case id>' (the ids of the modules' CASES tables)
ENTRIES = {
    'mdgat_forward': [f'{FWD}::first-fp32-3x61x66', f'{FWD}::first-fp32-9x48x64', f'{FWD}::first-fp32-2x128x256', f'{FWD}::first-fp32-1x512x512',
                      f'{FWD}::first-fp32-wide-3x61x66', f'{FWD}::first-fp32-wide-9x48x64', f'{FWD}::first-fp32-wide-2x128x256',
                      f'{FWD}::first-fp32-wide-1x512x512', f'{FWD}::sequence-fp32', f'{FWD}::sequence-fp32-wide', f'{FWD}::ragged-fp32-module'],
    'mdgat_forward_f64': [f'{FWD}::first-exact-3x61x66', f'{FWD}::first-exact-1x512x512', f'{FWD}::first-exact-20x128x128',
                          f'{FWD}::first-exact-1x600x577', f'{FWD}::sequence-exact', f'{FWD}::ragged-exact', f'{FWD}::ragged-exact-auto',
                          f'{FWD}::ragged-frames'],
    'mdgat_forward_ragged': [f'{FWD}::ragged-fp32-module'],
    'mdgat_forward_f64_ragged': [f'{FWD}::ragged-exact', f'{FWD}::ragged-exact-auto'],
    'mdgat_forward_frames_ragged': [f'{FWD}::ragged-frames'],
    'mdgat_forward_frames': [f'{FWD}::frames-2x61x66'],
    'mdgat_forward_loss': [f'{FWD}::evaluate-loss-fp32'],
    'mdgat_forward_f64_loss': [f'{FWD}::evaluate-loss-exact'],
    'mdgat_sinkhorn': [f'{OPS}::sinkhorn-cluster-64x64', f'{OPS}::sinkhorn-cluster-130x65', f'{OPS}::sinkhorn-cluster-390x24',
                       f'{OPS}::sinkhorn-cluster-513x40', f'{OPS}::sinkhorn-cluster-2048x8', f'{OPS}::sinkhorn-cluster-40x513',
                       f'{OPS}::sinkhorn-cluster-130x1030', f'{OPS}::sinkhorn-cluster-20x1540', f'{OPS}::sinkhorn-streaming-17x65',
                       f'{OPS}::sinkhorn-streaming-3x513', f'{OPS}::sinkhorn-fallback-130x65'],
    'mdgat_sinkhorn_ragged': [f'{OPS}::sinkhorn-ragged-s64'],
    'mdgat_sinkhorn_extract_ragged': [f'{OPS}::sinkhorn-ragged-s64'],
    'mdgat_extract': [f'{OPS}::extract-5x33x47', f'{FWD}::training-step-gap'],
    'mdgat_attention': [f'{OPS}::attention-plain-48x64'],
    'mdgat_attention_sel': [f'{OPS}::attention-48x64-k0', f'{OPS}::attention-48x64-k16', f'{OPS}::attention-61x66-k8-cross',
                            f'{OPS}::attention-128x256-k0', f'{OPS}::attention-300x500-k64', f'{OPS}::attention-512x512-k128',
                            f'{OPS}::attention-700x600-k100', f'{OPS}::attention-512x448-k0-cross'],
    'mdgat_attention_ragged': [f'{OPS}::attention-ragged-s128-k0', f'{OPS}::attention-ragged-s128-k8'],
    'mdgat_pointwise': [f'{OPS}::pointwise-77x256x256'],
    'mdgat_knn': [f'{OPS}::knn-C3-100x4097-k1', f'{OPS}::knn-C7-257x600-k600', f'{OPS}::knn-C128-64x300-k16'],
    'mdgat_pose': [f'{OPS}::pose-3x40x64'],
    'mdgat_gt_matches': [f'{OPS}::gt_matches-2x100x130'],
    'mdgat_gt_matches_ragged': [f'{OPS}::gt_matches-2x100x130'],
    'mdgat_eval_metrics': [f'{OPS}::evaluate_matches-rand17', f'{FWD}::evaluate-loss-fp32', f'{FWD}::evaluate-loss-exact'],
    'mdgat_eval_metrics_ragged': [f'{OPS}::evaluate_matches-rand17', f'{FWD}::ragged-fp32-module', f'{FWD}::ragged-exact', f'{FWD}::ragged-exact-auto'],
    'mdgat_assemble_frames_f64_ragged': [f'{OPS}::assemble_frames_ragged'],
    'mdgat_assemble_frames_train_f64': [f'{OPS}::assemble_frames_train'],
    'mdgat_sinkhorn_f64': [f'{OPS}::sinkhorn_f64-2x48x64', f'{OPS}::sinkhorn_f64-2x65x129', f'{OPS}::sinkhorn_f64-1x575x33',
                           f'{OPS}::sinkhorn_f64-1x577x30', f'{OPS}::sinkhorn_f64-2x30x700', f'{OPS}::sinkhorn_f64-1x30x1200',
                           f'{OPS}::sinkhorn_f64-2x65x129-form1', f'{OPS}::sinkhorn_backward-2x20x28', f'{OPS}::sinkhorn_backward-1x130x65',
                           f'{OPS}::sinkhorn_backward-1x577x30', f'{FWD}::training-step-gap'],
    'mdgat_sinkhorn_f64_ragged': [f'{OPS}::sinkhorn_f64-ragged-A'],
    'mdgat_sinkhorn_f64_extract_ragged': [f'{OPS}::sinkhorn_f64-ragged-A'],
    'mdgat_sinkhorn_f64_stream_ragged': [f'{OPS}::sinkhorn_f64-stream-ragged-S'],
    'mdgat_sinkhorn_f64_extract_stream_ragged': [f'{OPS}::sinkhorn_f64-stream-ragged-S'],
    'mdgat_sinkhorn_backward': [f'{OPS}::sinkhorn_backward-2x20x28', f'{OPS}::sinkhorn_backward-1x130x65', f'{OPS}::sinkhorn_backward-1x577x30',
                                f'{FWD}::training-step-gap'],
    'mdgat_attention_f64': [f'{OPS}::attention_f64-2x40x56-k0', f'{OPS}::attention_f64-2x40x56-k8-cross', f'{OPS}::attention_f64-1x513x513-k64',
                            f'{OPS}::attention_f64_backward-2x40x56-k8', f'{OPS}::attention_f64_backward-2x64x64-k0', f'{FWD}::training-step-gap'],
    'mdgat_attention_f64_ragged': [f'{OPS}::attention_f64-ragged-A-k8'],
    'mdgat_attention_backward_f64': [f'{OPS}::attention_f64_backward-2x40x56-k8', f'{OPS}::attention_f64_backward-2x64x64-k0',
                                     f'{FWD}::training-step-gap'],
    'mdgat_pointwise_f64': [f'{OPS}::pointwise_f64'],
    'mdgat_frame_max_f64': [f'{OPS}::frame_max_f64-2x37x128'],
    'mdgat_frame_max_backward_f64': [f'{OPS}::frame_max_f64-2x37x128'],
    'mdgat_loss': [f'{OPS}::matching_loss-superglue-2x24x24', f'{OPS}::matching_loss-triplet_loss-2x24x24', f'{OPS}::matching_loss-gap_loss-2x24x24',
                   f'{OPS}::matching_loss-gap_loss-2x20x28'],
    'mdgat_loss_backward': [f'{OPS}::matching_loss-superglue-2x24x24', f'{OPS}::matching_loss-triplet_loss-2x24x24',
                            f'{OPS}::matching_loss-gap_loss-2x24x24', f'{OPS}::matching_loss-gap_loss-2x20x28'],
}
ENTRIES['mdgat_sinkhorn_extract'] = list(ENTRIES['mdgat_sinkhorn'])
ENTRIES['mdgat_sinkhorn_f64_extract'] = [c for c in ENTRIES['mdgat_sinkhorn_f64'] if '::sinkhorn_f64-' in c]
ENTRIES['mdgat_loss_f64'] = ENTRIES['mdgat_loss'] + [f'{FWD}::training-step-gap']
ENTRIES['mdgat_loss_backward_f64'] = ENTRIES['mdgat_loss_backward'] + [f'{FWD}::training-step-gap']
_MLP = [f'{OPS}::mlp_f64-layer-65', f'{OPS}::mlp_f64-denc-1000', f'{OPS}::mlp_f64-conv128-17', f'{FWD}::training-step-gap']
ENTRIES.update({'mdgat_mlp_forward_f64': _MLP, 'mdgat_mlp_forward_residual_f64': _MLP, 'mdgat_mlp_backward_f64': _MLP})
_HEAD = [f'{OPS}::match_head-2x20x28', f'{OPS}::match_head-1x130x65', f'{FWD}::training-step-gap']
ENTRIES.update({'mdgat_match_head_f64': _HEAD, 'mdgat_match_head_backward': _HEAD})

# the measurement-only entries (bench.py's roofline): they take a workspace, and what they leave in it and in `msg` is no result
TIMING_PROBES = ('mdgat_mfma_probe', 'mdgat_mfma_f64_probe', 'mdgat_attention_qk_probe', 'mdgat_attention_qk_probe_sets')
REASONS = ('a query', 'a plan', 'a counter', 'a setter', 'create/destroy', 'a timing probe')
# C symbol -> (one of REASONS, what it is)
EXEMPT = {
    'mdgat_create': ('create/destroy', 'makes a handle; its memory is the library\'s own'),
    'mdgat_destroy': ('create/destroy', 'frees a handle'),
    'mdgat_load_weights': ('a setter', 'copies the packed weights into the handle\'s own memory'),
    'mdgat_load_weights_f64': ('a setter', 'copies the fp64 weights into the handle\'s own memory'),
    'mdgat_load_pooled_encoder_f64': ('a setter', 'copies the pooled encoder\'s weights into the handle\'s own memory'),
    'mdgat_weights_device_ptr': ('a query', 'the address of the handle\'s weights'),
    'mdgat_weights_f64_device_ptr': ('a query', 'the address of the handle\'s fp64 weights'),
    'mdgat_pooled_encoder_doubles': ('a query', 'a size'),
    'mdgat_blob_floats': ('a query', 'a size'),
    'mdgat_topk_sel_words': ('a query', 'a size'),
    'mdgat_last_error': ('a query', 'the last error message'),
    'mdgat_last_token': ('a query', 'the token of the handle\'s last call'),
    'mdgat_matched_any': ('a query', 'reads a host-mapped word of the handle'),
    'mdgat_async_status': ('a query', 'reads and clears the handle\'s status words'),
    'mdgat_profile': ('a counter', 'switches and reads the per-class timers of a handle'),
    'mdgat_workspace_bytes': ('a query', 'a size'),
    'mdgat_forward_loss_workspace_bytes': ('a query', 'a size'),
    'mdgat_loss_workspace_bytes': ('a query', 'a size'),
    'mdgat_loss_backward_workspace_bytes': ('a query', 'a size'),
    'mdgat_sinkhorn_workspace_bytes': ('a query', 'a size'),
    'mdgat_sinkhorn_ragged_workspace_bytes': ('a query', 'a size'),
    'mdgat_sinkhorn_f64_workspace_bytes': ('a query', 'a size'),
    'mdgat_sinkhorn_f64_ragged_workspace_bytes': ('a query', 'a size'),
    'mdgat_sinkhorn_f64_stream_ragged_workspace_bytes': ('a query', 'a size'),
    'mdgat_sinkhorn_backward_workspace_bytes': ('a query', 'a size'),
    'mdgat_match_head_workspace_bytes': ('a query', 'a size'),
    'mdgat_mlp_workspace_bytes': ('a query', 'a size'),
    'mdgat_attention_workspace_bytes': ('a query', 'a size'),
    'mdgat_attention_backward_workspace_bytes': ('a query', 'a size'),
    'mdgat_knn_workspace_bytes': ('a query', 'a size'),
    'mdgat_layer_plan': ('a plan', 'the layer launcher\'s choice as a pure function'),
    'mdgat_sinkhorn_plan': ('a plan', 'the Sinkhorn launchers\' choice as a pure function; the workspace address is never dereferenced'),
    'mdgat_attention_plan': ('a plan', 'the attention launcher\'s choice as a pure function'),
    'mdgat_attention_ragged_plan': ('a plan', 'the attention launcher\'s choice for a ragged batch as a pure function'),
    'mdgat_gemm_f64_plan': ('a plan', 'the fp64 GEMM launcher\'s choice as a pure function'),
    'mdgat_attention_f64_plan': ('a plan', 'the fp64 attention launcher\'s choice as a pure function'),
    'mdgat_attention_f64_geometry': ('a plan', 'the fp64 attention launcher\'s launch geometry as a pure function, into host integers'),
    'mdgat_layer_f64_plan': ('a plan', 'the fp64 layer-tail and encoder launchers\' choice as a pure function'),
    'mdgat_sinkhorn_f64_plan': ('a plan', 'the fp64 Sinkhorn launchers\' choice as a pure function'),
    'mdgat_layer_launches': ('a counter', 'launches by instantiation, into a host array'),
    'mdgat_sinkhorn_launches': ('a counter', 'launches by instantiation, into a host array'),
    'mdgat_attention_launches': ('a counter', 'launches by instantiation, into a host array'),
    'mdgat_gemm_f64_launches': ('a counter', 'launches by instantiation, into a host array'),
    'mdgat_attention_f64_launches': ('a counter', 'launches by instantiation, into a host array'),
    'mdgat_layer_f64_launches': ('a counter', 'layer tails and encoders by form, into a host array'),
    'mdgat_sinkhorn_f64_launches': ('a counter', 'calls of the fp64 Sinkhorn by form, into a host array'),
    'mdgat_set_lanes': ('a setter', 'how many streams a handle splits a large batch over'),
    'mdgat_set_layer_split_tiles': ('a setter', 'a launch parameter of the layer kernel'),
    'mdgat_set_f64_layer_fusion': ('a setter', 'which form the fp64 layer tail takes'),
    'mdgat_set_f64_attention_form': ('a setter', 'which form fp64 full attention takes'),
    'mdgat_set_f64_sinkhorn_form': ('a setter', 'which form the fp64 Sinkhorn takes'),
    'mdgat_set_ragged_sinkhorn': ('a setter', 'which fp64 Sinkhorn a handle\'s ragged batches run'),
    'mdgat_mfma_probe': ('a timing probe', 'measures the f16 MFMA rate; computes no result'),
    'mdgat_mfma_f64_probe': ('a timing probe', 'measures the fp64 MFMA rate; computes no result'),
    'mdgat_attention_qk_probe': ('a timing probe', 'the Q K^T phase alone, for the roofline; its output is not a result'),
    'mdgat_attention_qk_probe_sets': ('a timing probe', 'the standalone Q K^T phase kernel, for the roofline'),
}


# ------------------------------------------------------------------------------------------------------------ the table
def _takes_device_buffers(name):
    """Does the entry, by its signature, take a workspace or write an output buffer?  The C ABI hands device memory over as untyped
    pointers (host arrays are typed: POINTER(c_int), POINTER(c_uint64) ...): a workspace is ``void*, size_t`` in front of the stream, and
    an entry that reads inputs and writes outputs on a stream takes at least three untyped pointers."""
    _, args = _lib.SIGNATURES[name]
    workspace = len(args) >= 3 and args[-3:] == [C.c_void_p, C.c_size_t, C.c_void_p]
    return workspace or sum(a is C.c_void_p for a in args) >= 3


FAMILY_SUFFIXES = ('extract', 'ragged', 'stream', 'f64', 'sel', 'forward', 'backward', 'residual')


def _sized_by_a_query(name):
    """Has the entry a ``*_workspace_bytes`` sibling: ``<entry>_workspace_bytes``, or that of the family it belongs to - the entry's name
    without its trailing variant words (mdgat_sinkhorn_extract -> mdgat_sinkhorn_workspace_bytes)?"""
    stem = name
    while True:
        if stem + '_workspace_bytes' in _lib.SIGNATURES:
            return True
        head, _, last = stem.rpartition('_')
        if last not in FAMILY_SUFFIXES:
            return False
        stem = head


def test_every_symbol_is_covered_or_exempt():
    symbols = set(_lib.SIGNATURES)
    both = set(ENTRIES) & set(EXEMPT)
    assert not both, f'covered AND exempt: {sorted(both)}'
    missing = symbols - set(ENTRIES) - set(EXEMPT)
    assert not missing, f'neither covered by a prefilled case nor exempt with a reason: {sorted(missing)}'
    gone = (set(ENTRIES) | set(EXEMPT)) - symbols
    assert not gone, f'in the tables but not in _lib.SIGNATURES: {sorted(gone)}'


def test_exemptions_carry_a_valid_reason_and_no_entry_that_touches_device_memory():
    for name, (reason, what) in EXEMPT.items():
        assert reason in REASONS and what, (name, reason)
        if name.endswith('_workspace_bytes'):
            assert reason == 'a query', name
            continue
        if reason == 'a timing probe':            # out of scope by the contract, one by one: calling a new entry a probe exempts nothing
            assert name in TIMING_PROBES, f'{name}: a new probe is listed in TIMING_PROBES on purpose, or gets a case'
            continue
        assert not _takes_device_buffers(name), f'{name} takes a workspace or writes an output buffer: it needs a case, not an exemption'
        assert not _sized_by_a_query(name), f'{name} has a *_workspace_bytes sibling: it needs a case, not an exemption'


def test_the_rule_recognises_the_entries_it_is_for():
    """the signature rule is not vacuous: it fires on every covered entry, and on a dummy one"""
    for name in ENTRIES:
        assert _takes_device_buffers(name), name
    for name in ('mdgat_sinkhorn', 'mdgat_sinkhorn_extract', 'mdgat_sinkhorn_f64_extract_stream_ragged', 'mdgat_mlp_backward_f64', 'mdgat_knn'):
        assert _sized_by_a_query(name), name
    assert not _sized_by_a_query('mdgat_set_lanes') and not _takes_device_buffers('mdgat_create')


def test_the_tables_name_the_cases_that_run_the_entries():
    """ENTRIES is exactly what the GPU modules' own CASES tables say: every case id exists, and a case that spies an entry is listed under it"""
    import test_gpu_prefilled_forward as F
    import test_gpu_prefilled_ops as O
    from_cases = {}
    for mod, cases in ((OPS, {cid: c.entries for cid, c in O.CASES.items()}), (FWD, F.CASES)):
        for cid, entries in cases.items():
            for e in entries:
                from_cases.setdefault(e, set()).add(f'{mod}::{cid}')
    assert {k: set(v) for k, v in ENTRIES.items()} == from_cases
    for ids in ENTRIES.values():
        assert ids and len(ids) == len(set(ids))
    assert sorted(TIMING_PROBES) == sorted(n for n, (r, _) in EXEMPT.items() if r == 'a timing probe')
    for entry, query in O.WS_OF.items():
        assert entry in _lib.SIGNATURES and query in _lib.SIGNATURES and _lib.SIGNATURES[query][0] is C.c_size_t, (entry, query)


# ------------------------------------------------------------------------------------------------------------ the helper, on CPU tensors
ANY = dict(touch=lambda t: True)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.float16, torch.int32, torch.int64, torch.uint8, torch.bool])
def test_patterns_per_dtype(dtype):
    with P.prefilled('zero', **ANY) as p:
        z = torch.empty((3, 5), dtype=dtype)
    assert p.count == 1 and p.bytes == z.numel() * z.element_size()
    assert not z.view(torch.uint8).any()
    with P.prefilled('ones', **ANY) as p:
        o = [torch.empty((3, 5), dtype=dtype), torch.empty_like(z), z.new_empty((2, 2)), torch.empty_strided((4, 3), (1, 4), dtype=dtype)]
    assert p.count == 4
    for t in o:
        assert t.dtype == dtype
        if dtype == torch.bool:
            assert t.all()                                     # (a copy of a bool tensor normalises its bytes: every element reads True)
            continue
        assert (t.contiguous().view(torch.uint8) == 0xFF).all()
        if dtype.is_floating_point:
            assert torch.isnan(t).all()                        # every byte 0xFF: a NaN in every float format
        elif dtype in (torch.int32, torch.int64):
            assert (t == -1).all()                             # an index read before it is written points one element in front
    assert (torch.empty_strided((4, 3), (1, 4), dtype=dtype).stride() == (1, 4))


def test_only_the_chosen_tensors_are_touched_and_sizes_are_recorded():
    keep = torch.arange(6.0)
    with P.prefilled('ones') as p:                             # the default: device tensors only
        t = torch.empty(4)
        t.copy_(keep[:4])
    assert p.count == 0 and p.bytes == 0 and torch.equal(t, keep[:4])
    with P.prefilled('ones', **ANY) as p:
        torch.empty(0)
        torch.empty(100, dtype=torch.uint8)
        torch.empty(7, dtype=torch.float64)
        torch.empty(300, dtype=torch.uint8)
    assert p.count == 3 and p.bytes == 456 and p.scratch_bytes == 300         # (an empty tensor is not counted)
    assert p.saw_scratch(300) and not p.saw_scratch(301)


def test_functions_are_restored_after_an_exception():
    before = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    with pytest.raises(ZeroDivisionError):
        with P.prefilled('ones', **ANY):
            assert torch.empty is not before[0]
            1 / 0
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == before
    with P.prefilled('zero', **ANY):
        with P.prefilled('ones', **ANY):                       # nested: the inner fill is applied last, both are undone in order
            assert (torch.empty(3) != torch.empty(3)).all()
        assert not torch.empty(3).any()
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == before
    with pytest.raises(ValueError):
        with P.prefilled('random'):
            pass
    with pytest.raises(ValueError):
        with P.prefilled('replay'):
            pass


def test_replay_starts_every_allocation_from_its_recorded_twin():
    def call(scale):
        a = torch.empty(4)
        a.copy_(torch.arange(4.0) * scale)
        b = torch.empty((2, 3), dtype=torch.int64)
        b.fill_(int(7 * scale))
        c = torch.empty(5, dtype=torch.uint8)                  # never written: keeps what it started with
        return a, b, c
    with P.prefilled('ones', record=True, **ANY) as rec:
        call(4.0)
    assert rec.final is not None and [(s, d) for s, d, _ in rec.final] == [((4,), torch.float32), ((2, 3), torch.int64), ((5,), torch.uint8)]
    seen = []
    with P.prefilled('replay', source=rec, **ANY) as p:
        seen.append(torch.empty(4).clone())                    # the k-th allocation starts with the FINAL bytes of the recorded k-th
        seen.append(torch.empty((2, 3), dtype=torch.int64).clone())
        seen.append(torch.empty(5, dtype=torch.uint8).clone())
        seen.append(torch.empty(2).clone())                    # no twin: 0xFF
    assert p.replayed == 3 and p.count == 4
    assert torch.equal(seen[0], torch.arange(4.0) * 4) and (seen[1] == 28).all() and (seen[2] == 0xFF).all() and torch.isnan(seen[3]).all()
    with P.prefilled('replay', source=rec, **ANY) as p:        # another shape or dtype at the same place: 0xFF, never foreign bytes
        x = torch.empty(5)
        y = torch.empty((2, 3), dtype=torch.float64)
        z = torch.empty(5, dtype=torch.uint8)
    assert p.replayed == 1 and torch.isnan(x).all() and torch.isnan(y).all() and (z == 0xFF).all()
    with pytest.raises(ValueError):
        with P.prefilled('replay', source=P.Prefill('zero', None, True)):
            pass


def test_spy_counts_calls_and_puts_the_entries_back():
    class Lib:
        def __init__(self):
            self.f = lambda x: x + 1
            self.g_workspace_bytes = lambda n: 64 * n
    lib = Lib()
    f, g = lib.f, lib.g_workspace_bytes
    with pytest.raises(KeyError):
        with P.spy(lib, ('f', 'g_workspace_bytes')) as s:
            assert lib.f(1) == 2 and lib.f(2) == 3 and lib.g_workspace_bytes(3) == 192 and lib.g_workspace_bytes(1) == 64
            raise KeyError('x')
    assert s.calls == {'f': 2, 'g_workspace_bytes': 2} and s.most_asked() == 192
    assert lib.f is f and lib.g_workspace_bytes is g


def test_same_bits_tells_nan_payloads_and_signed_zeros_apart():
    a = {'x': torch.tensor([float('nan'), 0.0, 1.0]), 'y': [torch.tensor([1, 2]), None]}
    P.same_bits(P.snapshot(a), P.snapshot({'x': a['x'].clone(), 'y': [a['y'][0].clone(), None]}))
    with pytest.raises(AssertionError, match='1 of 3 elements differ'):
        P.same_bits(P.snapshot(a), P.snapshot({'x': torch.tensor([float('nan'), -0.0, 1.0]), 'y': a['y']}))
    with pytest.raises(AssertionError):
        P.same_bits(P.snapshot(a), P.snapshot({'x': a['x'].double(), 'y': a['y']}))
    with pytest.raises(AssertionError):
        P.same_bits(P.snapshot(a), P.snapshot({'x': a['x']}))
