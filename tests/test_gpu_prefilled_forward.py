"""The module's entry points must return the same bits whatever their outputs and the scratch the module caches per stream held before
(include/mdgat_hip.h: "a workspace and every output buffer may hold anything on entry") - on a first call into poisoned memory, and in
serving, where ONE module re-carves ONE cached workspace for whatever (B, N, M) comes next: pads present then absent, large then small,
the clustered fp64 layer tail then the plain one, the register-resident fp64 Sinkhorn then the streaming one, ragged chunks of changing
slots with a uniform call in between.

The reference result of every call is a FRESH module of the same weights, every allocation zero-filled, that runs this one call only;
everything else must equal it bit for bit (tests/prefilled.py).  What that reference computes is held to the oracle by
tests/test_gpu_forward.py, test_gpu_f64.py and the ragged files.  Small networks (two layers, ten Sinkhorn iterations): every call
takes well under a second.  ``CASES`` (id -> entries) is what tests/test_prefilled_table.py holds against ``_lib.SIGNATURES``."""
import functools

import numpy as np
import pytest
import torch

import sinkhorn_forms as SF
import train_ref as T
from conftest import GOLDEN
from mdgat_matcher_amd import MDGAT, _lib, ops, synth
from prefilled import prefilled, refill_cached, same_bits, snapshot, spy

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
L, K, ITERS = 2, [16, None, 8, None], 10
# ragged chunks hold pairs of 4 keypoints (set A halved): no dynamic layer may keep more (torch.topk raises in the reference)
K_RAGGED = [4, None, 4, None]
# the modules: 'fp32' - weights whose scores the fp32 cluster Sinkhorn holds, its own Z is the result; 'fp32-wide' - weights whose scores
# (up to 120) are beyond the scaling form's range for most pairs, which the gated streaming kernel redoes by their pair flags; 'exact' - a
# float64 module
ARITH = ('fp32', 'fp32-wide', 'exact')
SEED = {'fp32': 5, 'fp32-wide': 1, 'exact': 1}
REDONE = {'fp32': 0, 'fp32-wide': 1, 'exact': 0}           # what ``check`` reports behind a uniform call of each (sinkhorn_fallback)

# The exact module's shapes are here for a form of the fp64 kernels: (3, 61, 66) and (1, 512, 512) the clustered layer tail and the
# register-resident Sinkhorn, (20, 128, 128) the tail with one workgroup per block, (1, 600, 577) the streaming Sinkhorn.  The Sinkhorn's
# form is asserted (``_assert_sinkhorn_form``); the layer tail's - clustered for launches of at most a quarter of the compute units in
# 16-keypoint blocks (include/mdgat_hip.h: mdgat_layer_f64_plan) - is asserted by its launch counters where it is the subject, in
# tests/test_gpu_layer_f64_forms.py, and stays a statement of intent here.
STREAMING_F64 = {(3, 61, 66): False, (1, 512, 512): False, (20, 128, 128): False, (1, 600, 577): True}
FIRST = {'fp32': [(3, 61, 66), (9, 48, 64), (2, 128, 256), (1, 512, 512)], 'fp32-wide': [(3, 61, 66), (9, 48, 64), (2, 128, 256), (1, 512, 512)],
         'exact': [(3, 61, 66), (1, 512, 512), (20, 128, 128), (1, 600, 577)]}
SEQUENCE = {'fp32': [(9, 48, 64), (2, 128, 256), (3, 61, 66), (1, 512, 512), (2, 128, 256), (9, 48, 64)],
            'fp32-wide': [(9, 48, 64), (2, 128, 256), (3, 61, 66), (1, 512, 512), (2, 128, 256), (9, 48, 64)],
            'exact': [(1, 512, 512), (3, 61, 66), (1, 600, 577), (20, 128, 128), (3, 61, 66), (1, 512, 512)]}
FORWARD = {'fp32': 'mdgat_forward', 'fp32-wide': 'mdgat_forward', 'exact': 'mdgat_forward_f64'}
SET_A = ((40, 33), (17, 64), (64, 17), (65, 48), (8, 8), (31, 32), (33, 97))          # tests/test_gpu_ragged_attention.py's
SET_H = tuple(((n + 1) // 2, (m + 1) // 2) for n, m in SET_A)                          # every count halved and rounded up: other slots
UNIFORM = (3, 61, 66)
RAGGED_NETS = {'fp32-module': ('fp32', {'ragged_arithmetic': 'module'}, 'mdgat_forward_ragged'),
               'exact': ('exact', {}, 'mdgat_forward_f64_ragged'),
               'exact-auto': ('exact', {'ragged_sinkhorn': 'auto'}, 'mdgat_forward_f64_ragged')}

CASES = {}          # id -> the C entries the case asserts it ran
CASES.update({f'first-{a}-{B}x{N}x{M}': (FORWARD[a],) for a in ARITH for B, N, M in FIRST[a]})
CASES.update({f'sequence-{a}': (FORWARD[a],) for a in ARITH})
CASES.update({f'ragged-{name}': (entry, 'mdgat_eval_metrics_ragged', FORWARD[a]) for name, (a, _, entry) in RAGGED_NETS.items()})
CASES['ragged-frames'] = ('mdgat_forward_frames_ragged', 'mdgat_forward_f64')
CASES['frames-2x61x66'] = ('mdgat_forward_frames',)
CASES['training-step-gap'] = ('mdgat_mlp_forward_f64', 'mdgat_mlp_forward_residual_f64', 'mdgat_mlp_backward_f64', 'mdgat_attention_f64',
                              'mdgat_attention_backward_f64', 'mdgat_match_head_f64', 'mdgat_match_head_backward', 'mdgat_sinkhorn_f64',
                              'mdgat_sinkhorn_backward', 'mdgat_loss_f64', 'mdgat_loss_backward_f64', 'mdgat_extract')
CASES.update({f'evaluate-loss-{a}': (e, 'mdgat_eval_metrics') for a, e in (('fp32', 'mdgat_forward_loss'), ('exact', 'mdgat_forward_f64_loss'))})
SIZES = ('mdgat_workspace_bytes', 'mdgat_forward_loss_workspace_bytes')


def _new_net(arith, k=K, **over):
    """a fresh module: its own library handle, no cached scratch"""
    net = MDGAT({**synth.default_config(L=L, k=k, sinkhorn_iterations=ITERS), **over})
    net.load_state_dict(synth.make_state_dict(L=L, seed=SEED[arith]))
    net = (net.double() if arith == 'exact' else net.float()).eval().to(DEV)
    assert net.exact() == (arith == 'exact')
    return net


@functools.lru_cache(maxsize=None)
def _batch(B, N, M):
    return {k: v.to(DEV) for k, v in synth.make_batch(B, N, M).items()}


def _status(net):
    """``check`` is clean - it raises on a range violation or a non-finite value - and what it reports (a Sinkhorn launch, or a pair whose
    scores are beyond the scaling form's range, redone by the streaming kernel) is part of the call's result: a stale flag would show here"""
    return torch.tensor([int(v) for _, v in sorted(net.check(DEV).items())])


def _match(net, shape):
    """matches, scores and Z of one uniform call, and the handle's status behind it"""
    d = _batch(*shape)
    out = net.match(d['keypoints0'], d['descriptors0'], d['keypoints1'], d['descriptors1'], d['scores0'], d['scores1'], return_scores=True)
    return out, _status(net)


def _fresh(arith, call, **net_options):
    """the reference of one call: a fresh module, every allocation zero-filled, this call only"""
    with prefilled('zero'):
        out = call(_new_net(arith, **net_options))
        torch.cuda.synchronize()
    return snapshot(out)


@functools.lru_cache(maxsize=None)
def _reference(arith, shape):
    ref = _fresh(arith, lambda net: _match(net, shape))
    assert int(dict(ref)['[1]']) == REDONE[arith], f'{arith} {shape}: the weights no longer take the Sinkhorn path the case is here for'
    return ref


def _assert_sinkhorn_form(arith, shape, launched=None):
    """The Sinkhorn the shape is here for: exact - register-resident or streaming, by the workspace the launcher asks for; fp32 - the
    cluster kernel in the plan's instantiation with the gated streaming kernel behind it, by the launch counters."""
    if arith == 'exact':
        from test_gpu_prefilled_ops import _sinkhorn_f64_is_streaming
        assert _sinkhorn_f64_is_streaming(*shape) == STREAMING_F64[shape], shape
        return
    p = SF.plan(*shape)
    assert p.path == SF.CLUSTER and p.stream != 'none', shape
    assert launched is None or {k: v for k, v in launched.items() if k != SF.EXTRACT} == SF.expected(p), (shape, launched)


def _ran(s, cid):
    for e in CASES[cid]:
        assert s.calls[e] >= 1, f'{cid}: {e} was never called'


# ------------------------------------------------------------------------------------------------------------ (a) first call under poison
@pytest.mark.parametrize('arith,shape', [(a, s) for a in ARITH for s in FIRST[a]], ids=lambda v: v if isinstance(v, str) else 'x'.join(map(str, v)))
def test_first_call_into_poisoned_memory(arith, shape):
    cid = f'first-{arith}-' + 'x'.join(map(str, shape))
    ref = _reference(arith, shape)
    with spy(_lib.load(), CASES[cid] + SIZES) as s, SF.watch() as w, prefilled('ones') as p:
        got = _match(_new_net(arith), shape)
        torch.cuda.synchronize()
    _ran(s, cid)
    _assert_sinkhorn_form(arith, shape, w.launched())
    assert s.most_asked() > 0 and p.saw_scratch(s.most_asked()), (s.most_asked(), p.scratch_bytes)
    same_bits(ref, snapshot(got), f'{cid}: a fresh module under 0xFF against one under 0x00')


# ------------------------------------------------------------------------------------------------------------ (b) one module, a sequence of shapes
@pytest.mark.parametrize('arith', ARITH)
def test_one_module_runs_a_sequence_of_shapes(arith):
    cid = f'sequence-{arith}'
    refs = [_reference(arith, shape) for shape in SEQUENCE[arith]]
    for shape in SEQUENCE[arith]:
        _assert_sinkhorn_form(arith, shape)
    net = _new_net(arith)
    with spy(_lib.load(), CASES[cid] + SIZES) as s:
        for i, shape in enumerate(SEQUENCE[arith]):           # whatever the allocator and the call before left behind
            same_bits(refs[i], snapshot(_match(net, shape)), f'{cid}: call {i} {shape} behind {SEQUENCE[arith][:i]}')
        _ran(s, cid)
        assert len(net._state_for(torch.device(DEV)).workspaces) == 1, 'one stream, one cached workspace'
        for i, shape in enumerate(SEQUENCE[arith]):           # the cached scratch all-ones in front of every call, new allocations too
            filled = refill_cached(net, DEV, 0xFF)
            s.forget_sizes()
            with prefilled('ones') as p:
                got = _match(net, shape)
                torch.cuda.synchronize()
            need = s.most_asked()
            assert max(filled, p.scratch_bytes) >= need > 0, (filled, p.scratch_bytes, need)
            same_bits(refs[i], snapshot(got), f'{cid}: call {i} {shape} into 0xFF scratch behind {SEQUENCE[arith][:i]}')


# ------------------------------------------------------------------------------------------------------------ (c) ragged
@functools.lru_cache(maxsize=None)
def _pairs(counts):
    """the per-pair dicts of a count set as a batch_size=1 loader yields them, with gts and a pose for evaluate_ragged"""
    out = []
    for b, (n, m) in enumerate(counts):
        p = {k: v.to(DEV) for k, v in synth.make_batch(1, n, m, first_pair=b).items()}
        p['gt_matches0'], p['gt_matches1'] = (torch.arange(c, device=DEV)[None] % 3 - 1 for c in (n, m))      # -1, 0, 1: within every frame
        p['T_gt'] = torch.eye(4, dtype=torch.float64, device=DEV)[None]
        out.append(p)
    return tuple(out)


def _assert_fixed_beyond_counts(padded, counts, what):
    """matches -1, scores 0 and Z 0 beyond a pair's counts"""
    m0, m1, s0, s1, Z = padded[:5]
    for b, (n, m) in enumerate(counts):
        assert (m0[b, n:] == -1).all() and (m1[b, m:] == -1).all(), (what, b)
        assert not s0[b, n:].any() and not s1[b, m:].any(), (what, b)
        assert not Z[b, n + 1:].any() and not Z[b, :, m + 1:].any(), (what, b)
        assert torch.isfinite(Z[b, :n + 1, :m + 1]).all(), (what, b)


def _ragged(net, counts):
    """forward_ragged's padded outputs (checked beyond the counts), its dicts, and evaluate_ragged's table on one count set"""
    packed = ops.pack_ragged(list(_pairs(counts)), device=DEV)
    padded = net._run_ragged(packed, True)
    _assert_fixed_beyond_counts(padded, counts, counts[0])
    ev = net.evaluate_ragged(packed)
    return padded[:5], net.forward_ragged(packed, return_Z=True), ev['metrics'], ev['T'], ev['pairs']


def _ragged_rounds(cid, arith, options, calls):
    """``calls``: name -> call(net).  Every call alone on a fresh module under 0xFF, then all of them on ONE module - A, uniform, A halved,
    uniform, A - with its cached scratch refilled with 0xFF in front of each: the bits of the call's fresh zero-filled reference."""
    refs = {name: _fresh(arith, call, k=K_RAGGED, **options) for name, call in calls.items()}
    with spy(_lib.load(), CASES[cid] + SIZES) as s:
        for name, call in calls.items():
            s.forget_sizes()
            with prefilled('ones') as p:
                got = call(_new_net(arith, k=K_RAGGED, **options))
                torch.cuda.synchronize()
            assert s.most_asked() > 0 and p.saw_scratch(s.most_asked()), (name, s.most_asked(), p.scratch_bytes)
            same_bits(refs[name], snapshot(got), f'{cid}: {name} first on a fresh module under 0xFF')
        net = _new_net(arith, k=K_RAGGED, **options)
        for i, name in enumerate(('A', 'uniform', 'H', 'uniform', 'A')):
            if i:
                assert refill_cached(net, DEV, 0xFF) > 0
            with prefilled('ones'):
                got = calls[name](net)
                torch.cuda.synchronize()
            same_bits(refs[name], snapshot(got), f'{cid}: call {i} ({name}) on one module, scratch 0xFF')
        _ran(s, cid)


@pytest.mark.parametrize('name', list(RAGGED_NETS))
def test_ragged_chunks_of_changing_slots(name):
    arith, options, _ = RAGGED_NETS[name]
    calls = {'A': lambda net: _ragged(net, SET_A), 'H': lambda net: _ragged(net, SET_H), 'uniform': lambda net: _match(net, UNIFORM)}
    prev = _lib.load().mdgat_set_f64_attention_form(0)          # (the ragged files' setting: a pair's bits do not depend on its batch)
    try:
        _ragged_rounds(f'ragged-{name}', arith, options, calls)
    finally:
        torch.cuda.synchronize()
        _lib.load().mdgat_set_f64_attention_form(prev)


@functools.lru_cache(maxsize=None)
def _bank():
    """the frames of set A and of its halved twin as raw records in one bank: (bank, {counts: (idx0, idx1)})"""
    frames, where = [], {}
    for counts in (SET_A, SET_H):
        idx0, idx1 = [], []
        for b, (n, m) in enumerate(counts):
            k0, s0, f0, k1, s1, f1 = synth.make_pair(n, m, b)
            for idx, (k, s, f) in ((idx0, (k0, s0, f0)), (idx1, (k1, s1, f1))):
                idx.append(len(frames))
                frames.append(np.concatenate([k, s[:, None], f], axis=1).astype(np.float32))
        where[counts] = (idx0, idx1)
    return ops.pack_frames(frames, DEV), where


def _ragged_frames(net, counts):
    bank, where = _bank()
    idx0, idx1 = where[counts]
    chunk = ops.frames_chunk(bank, idx0, idx1)
    padded, kp0, kp1, _ = net._run_frames_ragged(bank, *chunk, True, True, want_kpts=True)
    _assert_fixed_beyond_counts(padded, counts, ('frames', counts[0]))
    return padded[:5], kp0, kp1, net.match_frames_ragged(bank, idx0, idx1, return_Z=True)


def test_ragged_chunks_from_a_bank_of_records():
    calls = {'A': lambda net: _ragged_frames(net, SET_A), 'H': lambda net: _ragged_frames(net, SET_H), 'uniform': lambda net: _match(net, UNIFORM)}
    prev = _lib.load().mdgat_set_f64_attention_form(0)
    try:
        _ragged_rounds('ragged-frames', 'exact', {}, calls)
    finally:
        torch.cuda.synchronize()
        _lib.load().mdgat_set_f64_attention_form(prev)


def test_match_frames_from_raw_records():
    """mdgat_forward_frames (the encoder kernel splits and normalises the records itself): first call under 0xFF, then behind another shape"""
    cid = 'frames-2x61x66'
    rec = {}
    for B, N, M in ((2, 61, 66), (1, 128, 96)):
        d = synth.make_batch(B, N, M)
        rec[N] = tuple(torch.cat([d['keypoints' + f], d['scores' + f][..., None], d['descriptors' + f]], dim=-1).float().to(DEV) for f in '01')

    def call(net, N=61):
        return net.match_frames(*rec[N], return_scores=True), _status(net)
    ref = _fresh('fp32', call)
    with spy(_lib.load(), CASES[cid] + SIZES) as s:
        net = _new_net('fp32')
        with prefilled('ones') as p:
            got = call(net)
            torch.cuda.synchronize()
        _ran(s, cid)
        assert s.most_asked() > 0 and p.saw_scratch(s.most_asked())
        same_bits(ref, snapshot(got), f'{cid}: a fresh module under 0xFF')
        call(net, 128)
        assert refill_cached(net, DEV, 0xFF) > 0
        same_bits(ref, snapshot(call(net)), f'{cid}: behind 128 x 96, scratch 0xFF')


# ------------------------------------------------------------------------------------------------------------ (d) training and loss
@functools.lru_cache(maxsize=None)
def _gap_case():
    return T.load(GOLDEN, 'gap')


def _gap_data(loud=False):
    d = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in _gap_case()['data'].items()}
    if loud:            # the louder twin: descriptors scaled by 4, the pairs in reverse order
        d = {k: v.flip(0) * (4 if k.startswith('descriptors') else 1) for k, v in d.items()}
    return d


def _training_step(loud=False):
    """tests/test_gpu_train.py's step of the 'gap' fixture on a fresh module: loss, every .grad, every buffer"""
    net = MDGAT(T.config('gap_loss')).double()
    net.load_state_dict(T.initial_state())
    net = net.to(DEV).train(True)
    out = net.training_forward(_gap_data(loud))
    out['loss'].mean().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in net.named_parameters()}
    assert all(g is not None for g in grads.values()), 'a parameter was left without a gradient'
    return {k: v.detach() for k, v in out.items()}, grads, dict(net.named_buffers())


def _three_fills(cid, call, sizes=SIZES):
    """``call(loud)`` under 0x00, under 0xFF and on the bytes a louder call left: the same bits"""
    with spy(_lib.load(), CASES[cid] + sizes) as s, prefilled('zero') as p0:
        zero = snapshot(call(False))
    _ran(s, cid)
    with prefilled('ones') as p1:
        ones = snapshot(call(False))
    with prefilled('zero', record=True) as rec:
        call(True)
    with prefilled('replay', source=rec) as p2:
        replay = snapshot(call(False))
    print(f'{cid}: {p1.count} allocations, {p1.bytes} bytes prefilled, scratch {p1.scratch_bytes} for {s.most_asked()} asked; replayed {p2.replayed} of {p2.count}')
    assert p0.count == p1.count == p2.count == p2.replayed > 0
    assert p1.saw_scratch(s.most_asked())
    same_bits(zero, ones, f'{cid}: 0xFF against 0x00')
    same_bits(zero, replay, f'{cid}: a louder call\'s bytes against 0x00')
    return zero


def test_training_step_under_every_fill():
    import test_gpu_train as TG
    from test_gpu_prefilled_ops import WS_OF
    cid = 'training-step-gap'
    zero = dict(_three_fills(cid, _training_step, tuple(sorted({WS_OF[e] for e in CASES[cid] if e in WS_OF}))))
    # the zero-filled step is the fixture's (test_step_reproduces_fixture's bound on the loss)
    c = TG._case('gap')
    got = {'loss': zero["[0]['loss']"].cpu().numpy()}
    worst, where, _ = T.compare(got, c['want'], c['err'], names=['loss'])
    assert worst <= 1.0, (worst, where)


@pytest.mark.parametrize('arith', ['fp32', 'exact'])
def test_evaluate_with_the_loss_request(arith):
    """``evaluate`` with config['eval_loss'] at the fixture's shapes: mdgat_forward_loss / mdgat_forward_f64_loss fill the loss from the
    workspace's Z, then mdgat_eval_metrics"""
    cid = f'evaluate-loss-{arith}'

    def call(loud):
        net = MDGAT({**T.config('gap_loss'), 'eval_loss': True})
        net.load_state_dict(T.initial_state())
        net = (net.double() if arith == 'exact' else net.float()).eval().to(DEV)
        out = net.evaluate(_gap_data(loud))
        torch.cuda.synchronize()
        return out
    zero = dict(_three_fills(cid, call))
    assert torch.isfinite(zero["['loss']"]).all()
