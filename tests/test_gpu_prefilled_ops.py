"""Every op of ``mdgat_matcher_amd.ops``, alone, must return the same bits whatever its workspace and its outputs held before the call
(include/mdgat_hip.h: "a workspace and every output buffer may hold anything on entry").

Each case runs one op three times on the same inputs - every ``torch.empty`` tensor of the call prefilled with 0x00, with 0xFF (floats NaN,
flags and epochs all-ones, indices -1) and with the final bytes of an earlier, LOUDER call of the same entry at the same shape (inputs
scaled by 4, pairs in reverse order: stale indices in range, stale maxima above the true ones - what fmax / atomicMax / ``>`` ignore in a
NaN) - and every returned tensor, the gradients and the BatchNorm buffers included, must be BIT-identical across the three
(tests/prefilled.py).  No tolerance: the ops are deterministic from run to run.  What the zero-filled run computes is held to the oracle
by the op's own test file at the same shape; where a shape is new to the suite the case adds that file's check (``verify``).

Every case also asserts that the C entries it names really ran (``spy``) and that the fill reached a uint8 allocation at least as large
as the workspace the library asked for.  ``CASES`` (id -> entries) is what tests/test_prefilled_table.py holds against ``_lib.SIGNATURES``.

``MlpSaved`` (what ``mlp_f64`` keeps between forward and backward) is one buffer of saved values AND scratch (the partial sums of the
batch statistics), so its bytes are not compared; the backward that reads it runs under the same fill and its gradients are."""
import functools
import os
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

import attention_forms as AF
import eval_ref as E
import extract_ref as E_X
import mlp_grad_ref as MR
import sinkhorn_forms as SF
from conftest import GOLDEN
from mdgat_matcher_amd import _lib, ops
from oracle import mdgat_oracle as O
from prefilled import prefilled, same_bits, snapshot, spy

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
THR = 0.01              # match_threshold of the extraction cases: the siblings' (random scores match little above it)

# entry -> the query that sizes its workspace
WS_OF = {
    'mdgat_sinkhorn': 'mdgat_sinkhorn_workspace_bytes', 'mdgat_sinkhorn_extract': 'mdgat_sinkhorn_workspace_bytes',
    'mdgat_sinkhorn_extract_ragged': 'mdgat_sinkhorn_ragged_workspace_bytes',
    'mdgat_attention': 'mdgat_attention_workspace_bytes', 'mdgat_attention_sel': 'mdgat_attention_workspace_bytes',
    'mdgat_attention_ragged': 'mdgat_attention_workspace_bytes', 'mdgat_knn': 'mdgat_knn_workspace_bytes',
    'mdgat_sinkhorn_f64': 'mdgat_sinkhorn_f64_workspace_bytes', 'mdgat_sinkhorn_f64_extract': 'mdgat_sinkhorn_f64_workspace_bytes',
    'mdgat_sinkhorn_f64_ragged': 'mdgat_sinkhorn_f64_ragged_workspace_bytes',
    'mdgat_sinkhorn_f64_extract_ragged': 'mdgat_sinkhorn_f64_ragged_workspace_bytes',
    'mdgat_sinkhorn_f64_stream_ragged': 'mdgat_sinkhorn_f64_stream_ragged_workspace_bytes',
    'mdgat_sinkhorn_f64_extract_stream_ragged': 'mdgat_sinkhorn_f64_stream_ragged_workspace_bytes',
    'mdgat_attention_backward_f64': 'mdgat_attention_backward_workspace_bytes',
    'mdgat_mlp_forward_f64': 'mdgat_mlp_workspace_bytes', 'mdgat_mlp_forward_residual_f64': 'mdgat_mlp_workspace_bytes',
    'mdgat_mlp_backward_f64': 'mdgat_mlp_workspace_bytes',
    'mdgat_match_head_f64': 'mdgat_match_head_workspace_bytes', 'mdgat_match_head_backward': 'mdgat_match_head_workspace_bytes',
    'mdgat_loss': 'mdgat_loss_workspace_bytes', 'mdgat_loss_f64': 'mdgat_loss_workspace_bytes',
    'mdgat_loss_backward': 'mdgat_loss_backward_workspace_bytes', 'mdgat_loss_backward_f64': 'mdgat_loss_backward_workspace_bytes',
    'mdgat_sinkhorn_backward': 'mdgat_sinkhorn_backward_workspace_bytes',
}

Case = namedtuple('Case', 'entries make env')
CASES = {}          # id -> Case; make(loud) -> run() -> a nest of tensors, built from seeded inputs (loud: the louder call a replay records)


def case(cid, entries, env=None):
    def register(make):
        assert cid not in CASES, cid
        CASES[cid] = Case(tuple(entries), make, dict(env or {}))
        return make
    return register


def _rs(*seed):
    return np.random.RandomState(zlib.crc32(repr(seed).encode()))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(device=DEV, dtype=dtype) if dtype is not None else t.to(DEV)


def _batch(a, loud, amp=4.0):
    """the louder twin of a batch: scaled by ``amp``, the pairs in reverse order"""
    return np.ascontiguousarray(a[::-1] * amp) if loud else a


# ------------------------------------------------------------------------------------------------------------ fp32 Sinkhorn
def _sinkhorn_run(s, alpha, iters, **kw):
    def run():
        out = {'Z': ops.sinkhorn(s, alpha, iters, **kw)}
        for mode in range(4):
            for want_Z in (False, True):
                out[f'extract{mode}{"+Z" if want_Z else ""}'] = ops.sinkhorn_extract(s, alpha, iters, mode=mode, match_threshold=THR, want_Z=want_Z, **kw)
        return out
    return run


def _mk_sinkhorn(N, M, streaming, loud):
    B = SF.FORMS_BATCH
    p = SF.plan(B, N, M, workspace=not streaming)
    if streaming:
        assert p.path == SF.STREAMING and p.stream == SF.STREAM_CASES[N, M]
    else:
        assert p.path == SF.CLUSTER and (p.scaling, p.GR, p.GC) == SF.CLUSTER_CASES[N, M]
    s = _dev(_batch(_rs('sk', N, M).standard_normal((B, N, M)) * 3.0, loud), torch.float32)
    return _sinkhorn_run(s, 0.8, 10, streaming=streaming)


for _N, _M in SF.CLUSTER_CASES:       # slots, flags and the row / column bests of 1 to 16 slabs
    case(f'sinkhorn-cluster-{_N}x{_M}', ('mdgat_sinkhorn', 'mdgat_sinkhorn_extract'))(functools.partial(_mk_sinkhorn, _N, _M, False))
for _N, _M in ((17, 65), (3, 513)):
    case(f'sinkhorn-streaming-{_N}x{_M}', ('mdgat_sinkhorn', 'mdgat_sinkhorn_extract'))(functools.partial(_mk_sinkhorn, _N, _M, True))


@case('sinkhorn-fallback-130x65', ('mdgat_sinkhorn', 'mdgat_sinkhorn_extract'), env={'MDGAT_SK_FORCE_FALLBACK': '1'})
def _mk_sinkhorn_fallback(loud):
    """the gated streaming kernel redoes the launch: Z lands in the caller's buffer or, without one, in the lent one"""
    run = _mk_sinkhorn(130, 65, False, loud)
    s = _dev(_rs('sk', 130, 65).standard_normal((SF.FORMS_BATCH, 130, 65)) * 3.0, torch.float32)

    def verify(out):        # (the hook is off again) test_sinkhorn_fallback_after_a_lost_partner's bar: it IS the streaming kernel
        assert torch.equal(out['Z'], ops.sinkhorn(s, 0.8, 10, streaming=True))
    run.verify = verify
    return run


@case('sinkhorn-ragged-s64', ('mdgat_sinkhorn_ragged', 'mdgat_sinkhorn_extract_ragged'))
def _mk_sinkhorn_ragged(loud):
    import test_gpu_ragged_sinkhorn_fp32 as RS
    counts, iters, alpha, _, _ = RS.SETS['s64']
    order = list(range(len(counts)))[::-1] if loud else list(range(len(counts)))
    s = RS._scores('s64', order=order) * (4.0 if loud else 1.0)            # NaN beyond every pair's counts
    return _sinkhorn_run(s.to(DEV), alpha, iters, counts=RS._cnt([counts[b] for b in order]))


# ------------------------------------------------------------------------------------------------------------ fp32 attention
def _qkv(B, N, M, loud, tag='qkv'):
    return _batch(_rs(tag, B, N, M).standard_normal((B, N + M, 3, 4, 32)) * 1.3, loud)


def _full_attention_oracle(qkv, N, M, cross, out, tol):
    """test_attention_full's check: the message of every frame against the oracle"""
    import test_gpu_ops as TO
    for lo, hi, q, k, v in TO._frames(qkv, N, M, cross):
        err = float((out.cpu().double()[:, lo:hi] - TO._ref_msg_to_lib(O.attention(q, k, v)[0])).abs().max())
        assert err < tol, (lo, err)


def _mk_attention(N, M, k, cross, form, new, loud):
    B = 2
    for tap in (False, True):
        assert AF.name(AF.plan(B, N, M, k, tap)[0]) == form + (',TAP' if tap and k else ''), (N, M, k, tap)
    host = _qkv(B, N, M, loud)
    x = _dev(host, torch.float32)

    def run():
        return {'msg': ops.attention(x, N, M, cross, topk=k), 'msg+sel': ops.attention(x, N, M, cross, topk=k, return_selection=True)}

    def verify(out):
        if not k:
            _full_attention_oracle(torch.from_numpy(host), N, M, cross, out['msg'], 1e-5)
            assert all(bool(m.all()) for m in out['msg+sel'][1]), 'full attention keeps every key'
        else:
            import test_gpu_ops as TO
            TO._check_topk_cross(torch.from_numpy(host), N, M, k, f'{N}x{M} k={k}', form)
    if new and not loud:
        run.verify = verify
    return run


# (N, M, k, cross, the kernel the launcher picks, is the shape new to the suite)
ATTENTION = [(48, 64, 0, False, 'full<4>', True), (48, 64, 16, False, 'dyn<4>', False),      # pads inside a 32-key block
             (61, 66, 8, True, 'dyn<4>', True),
             (128, 256, 0, False, 'stream', True),                                            # no pads
             (300, 500, 64, False, 'dyn<16>', False), (512, 512, 128, False, 'topk16<512>', False), (700, 600, 100, False, 'wide<4>', False),
             (512, 448, 0, True, 'stream', True)]
for _N, _M, _k, _cross, _form, _new in ATTENTION:
    case(f'attention-{_N}x{_M}-k{_k}{"-cross" if _cross else ""}', ('mdgat_attention_sel',))(
        functools.partial(_mk_attention, _N, _M, _k, _cross, _form, _new))


@case('attention-plain-48x64', ('mdgat_attention',))
def _mk_attention_plain(loud):
    """the entry without a selection argument (ops.attention always calls its sibling): straight through ctypes"""
    B, N, M = 2, 48, 64
    x = _dev(_qkv(B, N, M, loud), torch.float32)
    lib = _lib.load()

    def run():
        out = {}
        for k in (0, 16):
            need = lib.mdgat_attention_workspace_bytes(B, N, M)
            ws = torch.empty(need, dtype=torch.uint8, device=DEV)
            msg = torch.empty((B, N + M, 128), dtype=torch.float32, device=DEV)
            _lib.check(lib.mdgat_attention(B, N, M, 0, k, x.data_ptr(), msg.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream))
            out[k] = msg
        return out

    def verify(out):
        for k in (0, 16):
            assert torch.equal(out[k], ops.attention(x, N, M, False, topk=k))
    if not loud:
        run.verify = verify
    return run


def _assert_full_masks(masks, counts, cross):
    """full attention on a ragged batch keeps every key of a pair for every query of the pair, and nothing beyond its counts"""
    for b, (n, m) in enumerate(counts):
        for mask, nq, nk in ((masks[0], n, m if cross else n), (masks[1], m, n if cross else m)):
            want = torch.zeros_like(mask[b])
            want[:, :nq, :nk] = True
            assert torch.equal(mask[b], want), (b, cross)


def _mk_attention_ragged(k, loud):
    import test_gpu_ragged_attention_fp32 as RA
    counts = RA._counts('s128', k)
    if loud:
        counts = counts[::-1]
    Np, Mp = RA._slots('s128')
    x = (RA._qkv(counts, Np, Mp, 11) * (4.0 if loud else 1.0)).to(DEV)      # NaN beyond every pair's counts
    cnt = ([n for n, _ in counts], [m for _, m in counts])

    def run():
        return {(cross, sel): ops.attention(x, Np, Mp, cross, topk=k, return_selection=sel, counts=cnt) for cross in (False, True) for sel in (False, True)}
    if not k and not loud:
        run.verify = lambda out: [_assert_full_masks(out[cross, True][1], counts, cross) for cross in (False, True)]
    return run


for _k in (0, 8):
    case(f'attention-ragged-s128-k{_k}', ('mdgat_attention_ragged',))(functools.partial(_mk_attention_ragged, _k))


# ------------------------------------------------------------------------------------------------------------ fp32 products, knn
@case('pointwise-77x256x256', ('mdgat_pointwise',))
def _mk_pointwise(loud):
    rs = _rs('pw')
    A, W, b, R = (rs.standard_normal(s) for s in ((77, 256), (256, 256), (256,), (77, 256)))
    A, W, b, R = (_dev(t * (4.0 if loud else 1.0), torch.float32) for t in (A, W / 16, b, R))
    return lambda: {'plain': ops.pointwise(A, W), 'relu+res': ops.pointwise(A, W, b, relu=True, residual=R)}


def _mk_knn(Cc, N, M, k, new, loud):
    rs = _rs('knn', Cc, N, M, k)
    scale = 20.0 if Cc == 3 else 1.0
    x, s = (_batch(scale * rs.standard_normal((2, Cc, n)), loud) for n in (N, M))
    xd, sd = _dev(x, torch.float32), _dev(s, torch.float32)

    def run():
        out = {'mfma': ops.knn(xd, sd, k, adjacency=True), 'idx': ops.knn(xd, sd, k)}
        if Cc == 128:
            out['no mfma'] = ops.knn(xd, sd, k, adjacency=True, mfma=False)
        return out

    def verify(out):      # test_knn_large's check
        import test_gpu_ops as TO
        for kw in ({}, {'mfma': False}):
            frac = TO._knn_check(torch.from_numpy(x), torch.from_numpy(s), k, 2e-4, **kw)
            assert frac <= min(1.0, 0.05 + 0.004 * k)
    if new and not loud:
        run.verify = verify
    return run


for _Cc, _N, _M, _k, _new in ((3, 100, 4097, 1, False), (7, 257, 600, 600, False), (128, 64, 300, 16, True)):
    case(f'knn-C{_Cc}-{_N}x{_M}-k{_k}', ('mdgat_knn',))(functools.partial(_mk_knn, _Cc, _N, _M, _k, _new))


# ------------------------------------------------------------------------------------------------------------ extraction, post-processing
@case('extract-5x33x47', ('mdgat_extract',))
def _mk_extract(loud):
    s = torch.from_numpy(_batch(_rs('ex').standard_normal((5, 33, 47)) * 3.0, loud))
    Z = _dev(O.log_optimal_transport(s, torch.tensor(0.8, dtype=torch.float64), 20), torch.float32)

    def run():
        return {mode: ops.extract(Z, mode=mode, match_threshold=THR) for mode in range(4)}

    def verify(out):        # tests/test_gpu_extract.py's check: the rules applied in fp64 to the Z the kernel read
        for mode in range(4):
            E_X.check_extraction(Z, *out[mode], mode, E_X.f32(THR))
    if not loud:
        run.verify = verify
    return run


def _rigid(rs):
    q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
    T = np.eye(4)
    T[:3, :3] = q * np.sign(np.linalg.det(q))
    T[:3, 3] = rs.standard_normal(3)
    return T


def _cloud_pair(B, N, M, rs):
    """frame 1 = frame 0 moved rigidly plus noise on the shared points, random elsewhere: float32 [B, N, 3], [B, M, 3], T [B, 4, 4]"""
    k0 = rs.standard_normal((B, N, 3)) * 10
    k1 = rs.standard_normal((B, M, 3)) * 10
    T = np.stack([_rigid(rs) for _ in range(B)])
    n = min(N, M)
    for b in range(B):
        k1[b, :n] = (k0[b, :n] - T[b, :3, 3]) @ T[b, :3, :3] + 0.05 * rs.standard_normal((n, 3))
    return k0.astype(np.float32), k1.astype(np.float32), T


@case('pose-3x40x64', ('mdgat_pose',))
def _mk_pose(loud):
    rs = _rs('pose', loud)
    k0, k1, T = _cloud_pair(3, 40, 64, rs)
    m0 = np.where(rs.uniform(size=(3, 40)) < 0.7, np.arange(40)[None], -1).astype(np.int64)
    host = (k0, k1, m0, T)
    k0, k1, m0, T = (_dev(t) for t in host)

    def run():
        return {'with T_gt': ops.pose_from_matches(k0, k1, m0, T_gt=T), 'without': ops.pose_from_matches(k0, k1, m0)}

    def verify(out):        # tests/test_gpu_postproc.py::test_pose_from_matches' bounds, pair by pair
        Tg, st = (t.cpu().numpy() for t in out['with T_gt'])
        for b in range(3):
            Tr, n, inl, ratio, te, re = O.pose_from_matches(host[0][b], host[1][b], host[2][b], host[3][b])
            assert np.abs(Tg[b] - Tr).max() < 1e-9
            assert st[b, 0] == n and st[b, 1] == inl and abs(st[b, 2] - ratio) < 1e-12
            assert abs(st[b, 3] - te) < 1e-9 and abs(st[b, 4] - re) < 1e-7
            assert np.abs(out['without'][0][b].cpu().numpy() - Tr).max() < 1e-9
    if not loud:
        run.verify = verify
    return run


@case('gt_matches-2x100x130', ('mdgat_gt_matches', 'mdgat_gt_matches_ragged'))
def _mk_gt(loud):
    rs = _rs('gt', loud)
    h0, h1, hT = _cloud_pair(2, 100, 130, rs)
    k0, k1, T = (_dev(t) for t in (h0, h1, hT))
    cnt = ([100, 57], [77, 130]) if not loud else ([57, 100], [130, 77])

    def run():
        out = {}
        for mutual in (False, True):
            out[mutual] = ops.gt_matches(k0, k1, None, T, threshold=0.5, mutual=mutual)
            out[mutual, 'counts'] = ops.gt_matches(k0, k1, None, T, threshold=0.5, mutual=mutual, counts=cnt)
        return out

    def verify(out):        # tests/test_gpu_postproc.py::test_gt_matches' check: the oracle's matches, exactly; with counts: of the pair cut to them
        for mutual in (False, True):
            for key, sizes in ((mutual, [(100, 130)] * 2), ((mutual, 'counts'), list(zip(*cnt)))):
                g0, g1, rep = (t.cpu().numpy() for t in out[key])
                for b, (n, m) in enumerate(sizes):
                    r0, r1, rr = O.gt_matches(h0[b, :n], h1[b, :m], None, hT[b], 0.5, mutual)
                    np.testing.assert_array_equal(g0[b, :n], r0)
                    np.testing.assert_array_equal(g1[b, :m], r1)
                    assert int(rep[b]) == rr and (r0 >= 0).sum() > 10 and (g0[b, n:] == -1).all() and (g1[b, m:] == -1).all()
    if not loud:
        run.verify = verify
    return run


@functools.lru_cache(maxsize=None)
def _eval_group(name):
    return E.load_group(np.load(os.path.join(GOLDEN, 'eval_cases.npz')), name)[0]


@case('evaluate_matches-rand17', ('mdgat_eval_metrics', 'mdgat_eval_metrics_ragged'))
def _mk_eval(loud):
    g = _eval_group('rand17')                # the smallest case of test_gpu_eval.py: 3 pairs of 17 x 17
    order = [2, 1, 0] if loud else [0, 1, 2]
    t = {k: _dev(np.ascontiguousarray(g[k][order])) for k in ('matches0', 'matches1', 'gt0', 'gt1', 'kpts0', 'kpts1', 'T_gt')}
    # the same pairs cut to counts: what points beyond them becomes "unmatched"
    cnt = ([17, 12, 9], [17, 12, 14])
    cnt = tuple([c[b] for b in order] for c in cnt)
    cut = {}
    for f, other in (('0', 1), ('1', 0)):
        lim = torch.tensor(cnt[other], device=DEV)[:, None]
        for k in ('matches', 'gt'):
            v = t[k + f].clone()
            v[v >= lim] = -1
            cut[k + f] = v

    def run():
        m, T, _ = ops.evaluate_matches(t['matches0'], t['matches1'], t['gt0'], t['gt1'], t['kpts0'], t['kpts1'], T_gt=t['T_gt'])
        m2, T2, _ = ops.evaluate_matches(t['matches0'], t['matches1'], t['gt0'], t['gt1'], t['kpts0'], t['kpts1'])
        m3, T3, _ = ops.evaluate_matches(cut['matches0'], cut['matches1'], cut['gt0'], cut['gt1'], t['kpts0'], t['kpts1'], T_gt=t['T_gt'], counts=cnt)
        return m, T, m2, T2, m3, T3
    return run


# ------------------------------------------------------------------------------------------------------------ the loaders on the device
@case('assemble_frames_ragged', ('mdgat_assemble_frames_f64_ragged',))
def _mk_assemble(loud):
    import test_gpu_frames_ragged as FR
    frames, idx0, idx1, _ = FR._small_frames()          # the synthetic shuffled bank, one chunk
    if loud:
        frames, idx0, idx1 = [f * np.float32(4.0) for f in frames], idx0[::-1], idx1[::-1]
    bank = ops.pack_frames(frames, DEV)
    return lambda: {norm: ops.assemble_frames_ragged(bank, idx0, idx1, normalize=norm) for norm in (True, False)}


@case('assemble_frames_train', ('mdgat_assemble_frames_train_f64',))
def _mk_assemble_train(loud):
    import test_gpu_train_frames as TF
    frames, _ = TF._seeded_frames()
    idx0, idx1 = [0, 2, 4, 1], [1, 3, 5, 2]
    if loud:
        frames = [np.concatenate([f[:, :3] * 4, f[:, 3:4], f[:, 4:] * 4], axis=1).astype(np.float32) for f in frames]       # (the saliency filter stays)
        idx0, idx1 = idx0[::-1], idx1[::-1]
    bank = ops.pack_frames(frames, DEV)
    return lambda: {T: ops.assemble_frames_train(bank, idx0, idx1, T) for T in (1, 512)}


# ------------------------------------------------------------------------------------------------------------ fp64 Sinkhorn
def _sinkhorn_f64_run(s, alpha, iters, **kw):
    def run():
        out = {'Z': ops.sinkhorn_f64(s, alpha, iters, **kw)}
        for mode in range(4):
            for want_Z in (False, True):
                out[f'extract{mode}{"+Z" if want_Z else ""}'] = ops.sinkhorn_f64_extract(s, alpha, iters, mode=mode, match_threshold=THR, want_Z=want_Z, **kw)
        return out
    return run


class _setting:
    """a process-wide setter of the library held at ``value`` for a block, then put back"""

    def __init__(self, setter, value):
        self.setter, self.value = setter, value

    def __enter__(self):
        self.prev = getattr(_lib.load(), self.setter)(self.value)

    def __exit__(self, *exc):
        if torch.cuda.is_initialized():
            torch.cuda.synchronize()
        getattr(_lib.load(), self.setter)(self.prev)


def _sinkhorn_f64_is_streaming(B, N, M):
    """Which form the launcher takes for B pairs of N x M as it stands, by what it asks for: the streaming form keeps K, [B][N][M + 1
    rounded up to 128] doubles, in the workspace, the register-resident one a few slots per row slab; forcing the streaming form
    (mdgat_set_f64_sinkhorn_form(1)) changes the size exactly where the default is the resident one."""
    lib = _lib.load()
    asked = lib.mdgat_sinkhorn_f64_workspace_bytes(B, N, M)
    with _setting('mdgat_set_f64_sinkhorn_form', 1):
        forced = lib.mdgat_sinkhorn_f64_workspace_bytes(B, N, M)
    assert forced >= 8 * B * N * ((M + 1 + 127) // 128 * 128)
    return asked == forced


def _mk_sinkhorn_f64(B, N, M, iters, form, streaming, chunks, loud):
    # the form the case is here for: resident or streaming by the workspace the launcher asks for; the streaming instantiation holds
    # `chunks` column pairs of 128 per lane at most - this M needs more than the next smaller one holds
    with _setting('mdgat_set_f64_sinkhorn_form', -1 if form is None else form):
        assert _sinkhorn_f64_is_streaming(B, N, M) == streaming, (B, N, M)
    if chunks:
        from sinkhorn_grad_ref import REVERSE_VARIANTS
        need = (M + 1 + 127) // 128
        assert chunks == min(c for c in REVERSE_VARIANTS if c >= need), (M, need)
    s = _dev(_batch(_rs('sk64', N, M).standard_normal((B, N, M)) * 3.0, loud))
    inner = _sinkhorn_f64_run(s, 1.0, iters)

    def run():
        if form is None:
            return inner()
        with _setting('mdgat_set_f64_sinkhorn_form', form):
            return inner()

    def verify(out):        # test_sinkhorn_f64's check at this shape (its own seeded scores)
        import test_gpu_f64 as TF
        if form is None:
            TF._sinkhorn_f64_case(B, N, M, iters, 1.0, 3.0)
        else:
            with _setting('mdgat_set_f64_sinkhorn_form', form):
                TF._sinkhorn_f64_case(B, N, M, iters, 1.0, 3.0)
    if not loud:
        run.verify = verify
    return run


# (B, N, M, iterations, form): resident (one, three and eighteen row slabs), streaming (5, 9 and 17 column chunks), the streaming form forced
# (B, N, M, iterations, form, is it the streaming form, the column chunks of its instantiation)
SINKHORN_F64 = [(2, 48, 64, 5, None, False, 0), (2, 65, 129, 6, None, False, 0), (1, 575, 33, 7, None, False, 0), (1, 577, 30, 8, None, True, 5),
                (2, 30, 700, 9, None, True, 9), (1, 30, 1200, 10, None, True, 17), (2, 65, 129, 6, 1, True, 5)]
for _B, _N, _M, _it, _form, _streaming, _chunks in SINKHORN_F64:
    case(f'sinkhorn_f64-{_B}x{_N}x{_M}{"-form1" if _form else ""}', ('mdgat_sinkhorn_f64', 'mdgat_sinkhorn_f64_extract'))(
        functools.partial(_mk_sinkhorn_f64, _B, _N, _M, _it, _form, _streaming, _chunks))


def _ragged_scores(counts, seed):
    """[B, Np, Mp] float64, NaN beyond every pair's counts; a pair's scores follow from its own sizes"""
    Np, Mp = max(n for n, _ in counts), max(m for _, m in counts)
    s = np.full((len(counts), Np, Mp), np.nan)
    for b, (n, m) in enumerate(counts):
        s[b, :n, :m] = _rs(seed, n, m).standard_normal((n, m)) * 3.0
    return s


def _mk_sinkhorn_f64_ragged(which, loud):
    if which == 'resident':
        import test_gpu_ragged_sinkhorn as R
        counts, kw = R.SET_A, {}
    else:
        import test_gpu_ragged_sinkhorn_stream as R
        counts, kw = R.SET_S, dict(form='streaming')
    counts = counts[::-1] if loud else counts
    s = _dev(_ragged_scores(counts, 'rsk64') * (4.0 if loud else 1.0))
    return _sinkhorn_f64_run(s, 0.7, 8, counts=([n for n, _ in counts], [m for _, m in counts]), **kw)


case('sinkhorn_f64-ragged-A', ('mdgat_sinkhorn_f64_ragged', 'mdgat_sinkhorn_f64_extract_ragged'))(functools.partial(_mk_sinkhorn_f64_ragged, 'resident'))
case('sinkhorn_f64-stream-ragged-S', ('mdgat_sinkhorn_f64_stream_ragged', 'mdgat_sinkhorn_f64_extract_stream_ragged'))(
    functools.partial(_mk_sinkhorn_f64_ragged, 'streaming'))


# ------------------------------------------------------------------------------------------------------------ fp64 attention
def _mk_attention_f64(B, N, M, k, cross, forms, new, loud):
    host = _qkv(B, N, M, loud, 'qkv64')
    x = _dev(host)

    def run():
        out = {}
        for form in forms:
            with _setting('mdgat_set_f64_attention_form', form):
                out[form] = ops.attention_f64(x, N, M, cross, topk=k)
                out[form, 'sel'] = ops.attention_f64(x, N, M, cross, topk=k, return_selection=True)
        return out

    def verify(out):        # tests/test_gpu_f64.py::test_attention_f64_topk_selects_like_fp64's check: torch.topk's keys on the fp64 logits, row by row
        import test_gpu_f64 as TF
        msg, masks = out[forms[0], 'sel']
        for side, ((lo, hi), q, kk, v) in enumerate(TF._sides(torch.from_numpy(host), N, M, cross)):
            report = []
            ref, _ = O.dynamic_attention(q, kk, v, k, report=report)
            assert torch.equal(masks[side].cpu(), report[0]['own'])
            assert (msg.cpu()[:, lo:hi] - TF._ref_msg_to_lib(ref)).abs().max() < TF.F64_TOL
    if new and not loud:
        run.verify = verify
    return run


# (the last: new to the suite - test_gpu_f64.py runs (40, 56) full in both forms and (40, 56, 8, cross) at this batch)
for _B, _N, _M, _k, _cross, _forms, _new in ((2, 40, 56, 0, False, (0, 1), False), (2, 40, 56, 8, True, (-1,), False),
                                             (1, 513, 513, 64, False, (-1,), True)):
    case(f'attention_f64-{_B}x{_N}x{_M}-k{_k}{"-cross" if _cross else ""}', ('mdgat_attention_f64',))(
        functools.partial(_mk_attention_f64, _B, _N, _M, _k, _cross, _forms, _new))


@case('attention_f64-ragged-A-k8', ('mdgat_attention_f64_ragged',))
def _mk_attention_f64_ragged(loud):
    import test_gpu_ragged_attention as R
    counts = R.SET_A[::-1] if loud else R.SET_A
    Np, Mp = max(n for n, _ in counts), max(m for _, m in counts)
    x = np.full((len(counts), Np + Mp, 3, 4, 32), np.nan)
    for b, (n, m) in enumerate(counts):
        rs = _rs('rqkv64', n, m)
        x[b, :n], x[b, Np:Np + m] = rs.standard_normal((n, 3, 4, 32)) * 1.3, rs.standard_normal((m, 3, 4, 32)) * 1.3
    x = _dev(x * (4.0 if loud else 1.0))
    cnt = ([n for n, _ in counts], [m for _, m in counts])

    def run():
        return {(k, cross, sel): ops.attention_f64(x, Np, Mp, cross, topk=k, return_selection=sel, counts=cnt)
                for k in (0, 8) for cross in (False, True) for sel in (False, True)}
    if not loud:
        run.verify = lambda out: [_assert_full_masks(out[0, cross, True][1], counts, cross) for cross in (False, True)]
    return run


def _mk_attention_f64_backward(B, N, M, k, cross, loud):
    x = _dev(_qkv(B, N, M, loud, 'qkv64b'))
    g = _dev(_batch(_rs('dmsg', N, M).standard_normal((B, N + M, 128)), loud))

    def run():
        msg, sel = ops._attention_f64_values(x, N, M, cross, k, k > 0)         # (sel: the words the autograd Function saves)
        direct = ops.attention_f64_backward(x, N, M, cross, g, k, sel)
        leaf = x.clone().requires_grad_(True)
        ops.attention_f64(leaf, N, M, cross, topk=k).backward(g)
        return msg, sel, direct, leaf.grad
    return run


for _B, _N, _M, _k, _cross in ((2, 40, 56, 8, True), (2, 64, 64, 0, False)):
    case(f'attention_f64_backward-{_B}x{_N}x{_M}-k{_k}', ('mdgat_attention_f64', 'mdgat_attention_backward_f64'))(
        functools.partial(_mk_attention_f64_backward, _B, _N, _M, _k, _cross))


# ------------------------------------------------------------------------------------------------------------ fp64 products, the MLP
@case('pointwise_f64', ('mdgat_pointwise_f64',))
def _mk_pointwise_f64(loud):
    rs = _rs('pw64')
    amp = 4.0 if loud else 1.0
    a1, w1, b1 = (_dev(rs.standard_normal(s) * amp) for s in ((130, 33), (64, 33), (64,)))
    a2, w2, b2, r2 = (_dev(rs.standard_normal(s) * amp) for s in ((777, 256), (128, 256), (128,), (777, 128)))
    return lambda: {'130x64x33 relu': ops.pointwise_f64(a1, w1, b1, relu=True), '777x128x256 res': ops.pointwise_f64(a2, w2, b2, residual=r2)}


def _mk_mlp(stack, R, loud):
    x, p, dout = MR.gpu_case(stack, R)
    amp = 4.0 if loud else 1.0
    split = 128 if stack == 'layer' else 0

    def run():
        out = {}
        for training in (True, False):
            for with_res in (False, True):
                seq = MR.torch_stack(p, training).to(DEV)               # fresh modules: the BatchNorm buffers start from equal copies
                mods = list(seq)
                convs = [m for m in mods if isinstance(m, torch.nn.Conv1d)]
                bns = [m for m in mods if isinstance(m, torch.nn.BatchNorm1d)]
                xs = [_dev(x * amp)] if not split else [_dev(x[:, :split] * amp), _dev(x[:, split:] * amp)]
                res = _dev(dout[::-1].copy() * amp) if with_res else None
                leaves = [t.requires_grad_(True) for t in xs + ([res] if with_res else [])]
                y = ops.mlp_f64_tensors(xs[0], [c.weight for c in convs], [c.bias for c in convs], bns, training,
                                        x1=xs[1] if split else None, residual=res)
                y.backward(_dev(dout * amp))
                out[training, with_res] = (y.detach(), [t.grad for t in leaves], [q.grad for q in seq.parameters()], [b for b in seq.buffers()])
        return out
    return run


for _stack, _R in (('layer', 65), ('denc', 1000), ('conv128', 17)):
    case(f'mlp_f64-{_stack}-{_R}', ('mdgat_mlp_forward_f64', 'mdgat_mlp_forward_residual_f64', 'mdgat_mlp_backward_f64'))(
        functools.partial(_mk_mlp, _stack, _R))


@case('frame_max_f64-2x37x128', ('mdgat_frame_max_f64', 'mdgat_frame_max_backward_f64'))
def _mk_frame_max(loud):
    e = _dev(_batch(_rs('fm').standard_normal((2, 37, 128)), loud))
    dg = _dev(_batch(_rs('fmg').standard_normal((2, 128)), loud))

    def run():
        leaf = e.clone().requires_grad_(True)
        g, idx = ops.frame_max_f64(leaf)
        g.backward(dg)
        return g.detach(), idx, leaf.grad, ops.frame_max_backward(dg, idx, 37)

    def verify(out):        # tests/test_gpu_descriptors.py's: torch.max itself (the first row that holds the maximum), dg scattered to it
        g, idx, de, de2 = out
        want = e.max(dim=1)
        assert torch.equal(g, want.values) and torch.equal(idx, want.indices)
        scattered = torch.zeros_like(e).scatter_(1, want.indices[:, None, :], dg[:, None, :])
        assert torch.equal(de, scattered) and torch.equal(de2, scattered)
    if not loud:
        run.verify = verify
    return run


# ------------------------------------------------------------------------------------------------------------ the head, the loss, their gradients
def _mk_match_head(B, N, M, loud):
    rs = _rs('head', N, M)
    d0, d1, ds = (_batch(rs.standard_normal(s), loud) for s in ((B, N, 128), (B, M, 128), (B, N, M)))
    W, b = rs.standard_normal((128, 128)) / 11.3, rs.standard_normal(128) * 0.1

    def run():
        leaves = [_dev(t).requires_grad_(True) for t in (d0, d1, W, b)]
        scores = ops.match_head(*leaves)
        scores.backward(_dev(ds))
        return scores.detach(), [t.grad for t in leaves]

    def verify(out):        # tests/test_gpu_head_grad.py::_check_shape's bounds on these inputs
        import head_grad_ref as HR
        a = [d0, d1, W, b, ds]
        tol = HR.tolerances(*a)
        assert HR.worst_fraction(out[0].cpu().numpy(), HR.forward(*a[:4]), tol['scores']) <= 1.0
        for name, got, want in zip(('ddesc0', 'ddesc1', 'dW', 'db'), out[1], HR.backward(*a)):
            assert HR.worst_fraction(got.cpu().numpy(), want, tol[name]) <= 1.0, name
    if not loud:
        run.verify = verify
    return run


for _B, _N, _M in ((2, 20, 28), (1, 130, 65)):
    case(f'match_head-{_B}x{_N}x{_M}', ('mdgat_match_head_f64', 'mdgat_match_head_backward'))(functools.partial(_mk_match_head, _B, _N, _M))


def _gts(B, N, M, rs):
    """consistent ground-truth matches: half of the smaller frame matched one to one, -1 elsewhere"""
    g0, g1 = np.full((B, N), -1, dtype=np.int64), np.full((B, M), -1, dtype=np.int64)
    for b in range(B):
        rows, cols = rs.permutation(N)[:min(N, M) // 2], rs.permutation(M)[:min(N, M) // 2]
        g0[b, rows], g1[b, cols] = cols, rows
    return g0, g1


def _mk_loss(method, B, N, M, loud):
    rs = _rs('loss', method, N, M)
    s = torch.from_numpy(_batch(rs.standard_normal((B, N, M)) * 2.0, loud, amp=2.0))
    Z = O.log_optimal_transport(s, torch.tensor(1.0, dtype=torch.float64), 20)
    g0, g1 = (_dev(t) for t in _gts(B, N, M, rs))
    dl = _dev(rs.standard_normal(B))

    def run():
        out = {}
        for dtype in (torch.float64, torch.float32):
            leaf = _dev(Z, dtype).requires_grad_(True)
            loss = ops.matching_loss(leaf, g0.clone(), g1.clone(), method, 0.5)
            loss.backward(dl)
            out[dtype] = (loss.detach(), leaf.grad, ops.matching_loss(leaf.detach(), g0.clone(), g1.clone(), method, 0.5))
        return out
    return run


for _method, _B, _N, _M in (('superglue', 2, 24, 24), ('triplet_loss', 2, 24, 24), ('gap_loss', 2, 24, 24), ('gap_loss', 2, 20, 28)):
    case(f'matching_loss-{_method}-{_B}x{_N}x{_M}', ('mdgat_loss', 'mdgat_loss_f64', 'mdgat_loss_backward', 'mdgat_loss_backward_f64'))(
        functools.partial(_mk_loss, _method, _B, _N, _M))


def _mk_sinkhorn_backward(B, N, M, iters, loud):
    rs = _rs('skb', N, M)
    s, dZ = _batch(rs.standard_normal((B, N, M)) * 2.0, loud), _batch(rs.standard_normal((B, N + 1, M + 1)), loud)

    def run():
        scores, alpha = _dev(s).requires_grad_(True), torch.tensor(0.8, dtype=torch.float64, device=DEV, requires_grad=True)
        Z = ops.log_optimal_transport(scores, alpha, iters)
        Z.backward(_dev(dZ))
        return Z.detach(), scores.grad, alpha.grad, ops.sinkhorn_backward(scores.detach(), 0.8, iters, _dev(dZ))

    def verify(out):        # tests/test_gpu_sinkhorn_grad.py::test_fp64_against_oracle_autograd's check and bound
        import test_gpu_sinkhorn_grad as SG
        from sinkhorn_grad_ref import oracle_grad
        ref_ds, ref_da = oracle_grad(torch.from_numpy(s), 0.8, iters, torch.from_numpy(dZ))
        SG._check(out[1].cpu(), out[2].cpu(), ref_ds, ref_da, 1e-8)
        SG._check(out[3][0].cpu(), out[3][1].sum().cpu(), ref_ds, ref_da, 1e-8)
        assert (out[0].cpu() - O.log_optimal_transport(torch.from_numpy(s), torch.tensor(0.8, dtype=torch.float64), iters)).abs().max() < 1e-12
    if not loud:
        run.verify = verify
    return run


# the last: the streaming form's history
for _B, _N, _M, _it in ((2, 20, 28, 20), (1, 130, 65, 10), (1, 577, 30, 5)):
    case(f'sinkhorn_backward-{_B}x{_N}x{_M}', ('mdgat_sinkhorn_f64', 'mdgat_sinkhorn_backward'))(functools.partial(_mk_sinkhorn_backward, _B, _N, _M, _it))


# ------------------------------------------------------------------------------------------------------------ the runner
@pytest.mark.parametrize('cid', sorted(CASES))
def test_prefilled(cid, monkeypatch):
    c = CASES[cid]
    lib = _lib.load()
    sizes = sorted({WS_OF[e] for e in c.entries if e in WS_OF})
    runs = {name: c.make(False) for name in ('zero', 'ones', 'replay')}       # inputs (and modules) are built outside the fills
    louder = c.make(True)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    try:
        with spy(lib, c.entries + tuple(sizes)) as s, prefilled('zero') as p0:
            kept = runs['zero']()
            torch.cuda.synchronize()
        zero = snapshot(kept)
        for e in c.entries:
            assert s.calls[e] >= 1, f'{cid}: {e} was never called'
        with prefilled('ones') as p1:
            ones = runs['ones']()
            torch.cuda.synchronize()
        ones = snapshot(ones)
        with prefilled('zero', record=True) as rec:
            louder()
        with prefilled('replay', source=rec) as p2:
            replay = runs['replay']()
            torch.cuda.synchronize()
        replay = snapshot(replay)
    finally:
        torch.cuda.synchronize()
        for k in c.env:
            monkeypatch.delenv(k)
    need = s.most_asked()
    print(f'{cid}: {p1.count} allocations, {p1.bytes} bytes prefilled, scratch {p1.scratch_bytes} for {need} asked; replayed {p2.replayed} of {p2.count}')
    assert zero, f'{cid}: the case returned no tensor'
    assert p0.count == p1.count == p2.count > 0
    assert p1.saw_scratch(need) and p2.saw_scratch(need), f'{cid}: the fill never reached a workspace of {need} bytes (largest: {p1.scratch_bytes})'
    assert p2.replayed == p2.count, f'{cid}: only {p2.replayed} of {p2.count} allocations found their recorded twin'
    same_bits(zero, ones, f'{cid}: 0xFF against 0x00')
    same_bits(zero, replay, f'{cid}: a louder call\'s bytes against 0x00')
    verify = getattr(runs['zero'], 'verify', None)
    if verify is not None:
        verify(kept)
