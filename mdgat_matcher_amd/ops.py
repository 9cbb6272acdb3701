"""Per-op Python bindings over the C ABI (torch tensors in, torch tensors out; all on a gfx950 device).

These call the same kernels ``mdgat_forward`` launches; they exist for unit parity tests and for
callers that want a single stage (e.g. Sinkhorn on their own score matrix)."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

from . import _lib


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _need_cuda(*ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError('mdgat_matcher_amd ops run on MI355X only (no CPU fallback)')


def _workspace(need, device):
    """Scratch memory for one call of the library: (the buffer that owns it, its first 256-byte aligned address, ``need``)."""
    buf = torch.empty(need + 256, dtype=torch.uint8, device=device)
    return buf, buf.data_ptr() + (-buf.data_ptr()) % 256, need


def _match_outputs(B, N, M, device, want_Z=False):
    """What a matching call fills: (matches0 [B, N], matches1 [B, M] int64, mscores0, mscores1 float32, Z [B, N+1, M+1] float32 or None)."""
    return (torch.empty((B, N), dtype=torch.int64, device=device), torch.empty((B, M), dtype=torch.int64, device=device),
            torch.empty((B, N), dtype=torch.float32, device=device), torch.empty((B, M), dtype=torch.float32, device=device),
            torch.empty((B, N + 1, M + 1), dtype=torch.float32, device=device) if want_Z else None)


RAGGED_WIDE_LAUNCHES = ('stream<16,8>,RAGGED', 'stream<32,8>,RAGGED', 'split iteration, wide', 'split finish, wide',
                        'full<8>,windowed,RAGGED', 'wide<4>,RAGGED', 'wide<4>,TAP,RAGGED', 'wide<8>,RAGGED', 'wide<8>,TAP,RAGGED')


def ragged_wide_launches() -> dict:
    """``mdgat_ragged_wide_launches``: the launches only a wide ragged slot reaches, by name, counted by this process so far (never reset:
    read them before and after a call and subtract)."""
    buf = (C.c_uint64 * len(RAGGED_WIDE_LAUNCHES))()
    _lib.load().mdgat_ragged_wide_launches(buf)
    return dict(zip(RAGGED_WIDE_LAUNCHES, (int(n) for n in buf)))


def _wide_args(wide, split, counts):
    if (wide or split) and counts is None:
        raise ValueError('wide / split select the wide ragged entries: they need counts')
    if split and not wide:
        raise ValueError('split=True is the wide ragged entries\': it needs wide=True')
    return bool(wide), bool(split)


def sinkhorn(scores: torch.Tensor, bin_score: float, iters: int, streaming: bool = False, counts=None, wide: bool = False,
             split: bool = False) -> torch.Tensor:
    """log_optimal_transport (mdgat.py:288-308): scores [B, N, M] -> Z [B, N+1, M+1] (fp32).

    N, M <= 2048 run on the register-resident cluster kernel (128 x 512 tiles per workgroup; needs a small workspace,
    allocated here); ``streaming=True`` selects the one-workgroup-per-pair streaming kernel.

    ``counts`` (a ``pack_ragged`` dict or ``(counts0, counts1)``): a ragged batch in slots of N x M <= 512 - pair b is
    ``scores[b, :counts0[b], :counts1[b]]``, the rest of its slot is never read.  It runs on the streaming kernel:
    ``Z[b, :counts0[b]+1, :counts1[b]+1]`` has the bits of the pair run alone with ``streaming=True`` (its dustbins at row
    ``counts0[b]`` / column ``counts1[b]``), the rest of the slot is 0.

    ``wide=True`` (with counts): slots of up to 2048 x 2048 (``mdgat_sinkhorn_ragged_wide``) - the same contract, slots within 512 x 512 the
    same kernels and bits.  ``split=True`` with it: the split form where the slot has more than 128 rows (a pair's rows over several
    workgroups, one launch per iteration); it agrees with the default form to fp32 rounding, not bit for bit."""
    wide, split = _wide_args(wide, split, counts)
    _need_cuda(scores)
    s = scores.to(torch.float32).contiguous()
    B, N, M = s.shape
    Z = torch.empty((B, N + 1, M + 1), dtype=torch.float32, device=s.device)
    lib = _lib.load()
    with torch.cuda.device(s.device):
        name, lead, _keep = _entry('mdgat_sinkhorn', counts, B, s.device)
        need = 0 if streaming or counts is not None else lib.mdgat_sinkhorn_workspace_bytes(B, N, M)
        if wide:
            name, need = name + '_wide', lib.mdgat_sinkhorn_ragged_wide_workspace_bytes(B, N, M) if split else 0
        _buf, ws_ptr, _ = _workspace(need, s.device) if need else (None, None, 0)
        tail = (int(split), ws_ptr, need) if wide else () if counts is not None else (ws_ptr, need)
        _lib.check(getattr(lib, name)(B, N, M, *lead, s.data_ptr(), float(bin_score), int(iters), Z.data_ptr(), *tail, _stream(s)), name)
    return Z


def sinkhorn_extract(scores: torch.Tensor, bin_score: float, iters: int, mode: int = _lib.EXTRACT_DUSTBIN, match_threshold: float = 0.2,
                     want_Z: bool = False, streaming: bool = False, counts=None, wide: bool = False, split: bool = False):
    """fp32 Sinkhorn + match extraction as the forward runs them (launch_sinkhorn with an extraction request): (matches0, matches1,
    mscores0, mscores1[, Z]).  On the cluster kernel (N, M <= 2048) the arg-maxes are decided in its epilogue and Z is written only
    if wanted; ``streaming=True`` passes no workspace: the one-workgroup-per-pair kernel writes Z and the extraction kernel scans it.

    ``counts`` as in ``sinkhorn``: pair b's matches and scores are those of the pair run alone with ``streaming=True`` (no match: -1; the
    rule of mdgat.py:465-467 per pair); beyond its counts matches are -1 and scores 0.  ``wide``, ``split``: as in ``sinkhorn``
    (``mdgat_sinkhorn_extract_ragged_wide``)."""
    wide, split = _wide_args(wide, split, counts)
    _need_cuda(scores)
    s = scores.to(torch.float32).contiguous()
    B, N, M = s.shape
    m0, m1, s0, s1, Zbuf = _match_outputs(B, N, M, s.device, want_Z=True)     # (Z, or the buffer lent for redone pairs)
    lib = _lib.load()
    with torch.cuda.device(s.device):
        name, lead, _keep = _entry('mdgat_sinkhorn_extract', counts, B, s.device)
        if counts is not None:
            # the ragged entry scans the Z it is given, or - when none is wanted - one it produces into a workspace
            need = 0 if want_Z else lib.mdgat_sinkhorn_ragged_workspace_bytes(B, N, M)
            z_out, lent = want_Z, ()
            if wide:        # (one workspace: a Z where none is wanted, the split form's scratch)
                name, lent = name + '_wide', (int(split),)
                need = lib.mdgat_sinkhorn_ragged_wide_workspace_bytes(B, N, M) if split or not want_Z else 0
        else:
            need = 0 if streaming else lib.mdgat_sinkhorn_workspace_bytes(B, N, M)
            z_out = want_Z or not need
            lent = (None if z_out else Zbuf.data_ptr(),)
        _buf, ws_ptr, _ = _workspace(need, s.device) if need else (None, None, 0)
        _lib.check(getattr(lib, name)(B, N, M, *lead, s.data_ptr(), float(bin_score), int(iters), int(mode), float(match_threshold), m0.data_ptr(),
                                      m1.data_ptr(), s0.data_ptr(), s1.data_ptr(), Zbuf.data_ptr() if z_out else None, *lent,
                                      ws_ptr, need, _stream(s)), name)
    return (m0, m1, s0, s1, Zbuf) if want_Z else (m0, m1, s0, s1)


_RAGGED_KEYS = (('keypoints', 2), ('scores', 1), ('descriptors', 2))      # per-frame inputs and their rank without a batch axis


def pack_ragged(pairs, device=None) -> dict:
    """A ragged batch from per-pair dicts, as the reference's ``batch_size=1`` loader yields them (test.py:132): ``keypoints0/1``
    [N_b, 3], ``scores0/1`` [N_b], ``descriptors0/1`` [N_b, C], with or without a leading batch axis of 1, every pair with its own
    keypoint counts.  Returns the float64 tensors padded with zeros to ``Np = max N_b`` / ``Mp = max M_b`` and stacked, ``counts0`` /
    ``counts1`` (int32 [B], on the tensors' device) with their host copies ``counts0_host`` / ``counts1_host`` (CPU tensors: what the
    library checks before it launches anything), and - where every pair carries them - ``gt_matches0/1`` (int64, padded with -1) and
    ``T_gt`` [B, 4, 4].  Pure torch: it runs on CPU tensors too.  ``device``: where the result lives (default: where the first pair's
    keypoints are)."""
    pairs = list(pairs)
    if not pairs:
        raise ValueError('pack_ragged: no pairs')
    if device is None:
        device = pairs[0]['keypoints0'].device

    def one(t, rank, what):
        t = torch.as_tensor(t)
        if t.dim() == rank + 1 and t.shape[0] == 1:
            t = t[0]
        if t.dim() != rank:
            raise ValueError(f'pack_ragged: {what} has shape {tuple(t.shape)}: expected rank {rank}, or a leading axis of 1')
        return t

    B = len(pairs)
    out, counts = {}, {}
    for f in '01':
        cols = {k: [one(p[k + f], r, k + f) for p in pairs] for k, r in _RAGGED_KEYS}
        n = [int(t.shape[0]) for t in cols['keypoints']]
        for k, _ in _RAGGED_KEYS:
            for b, t in enumerate(cols[k]):
                if int(t.shape[0]) != n[b] or t.shape[1:] != cols[k][0].shape[1:]:
                    raise ValueError(f'pack_ragged: pair {b}: {k}{f} has shape {tuple(t.shape)}, keypoints{f} {n[b]} rows')
        counts[f] = n
        P = max(n)
        for k, _ in _RAGGED_KEYS:
            buf = torch.zeros((B, P) + tuple(cols[k][0].shape[1:]), dtype=torch.float64, device=device)
            for b, t in enumerate(cols[k]):
                buf[b, :n[b]] = t.to(device=device, dtype=torch.float64)
            out[k + f] = buf
        if all('gt_matches' + f in p for p in pairs):
            gt = torch.full((B, P), -1, dtype=torch.int64, device=device)
            for b, p in enumerate(pairs):
                t = one(p['gt_matches' + f], 1, 'gt_matches' + f)
                if int(t.shape[0]) != n[b]:
                    raise ValueError(f'pack_ragged: pair {b}: gt_matches{f} has {int(t.shape[0])} entries, keypoints{f} {n[b]} rows')
                gt[b, :n[b]] = t.to(device=device, dtype=torch.int64)
            out['gt_matches' + f] = gt
        host = torch.tensor(n, dtype=torch.int32)
        out['counts' + f + '_host'] = host
        out['counts' + f] = host.to(device)
    if all('T_gt' in p for p in pairs):
        out['T_gt'] = torch.stack([one(p['T_gt'], 2, 'T_gt').to(device=device, dtype=torch.float64) for p in pairs])
    return out


class _Counts(namedtuple('_Counts', 'd0 d1 h0 h1')):
    """The counts of a ragged batch as the library takes them: int32 [B] on the device (d0, d1) and the same values on the host (h0, h1)."""
    __slots__ = ()

    def ptrs(self):
        """the four leading pointers of every ``*_ragged`` entry, in the ABI's order"""
        return self.d0.data_ptr(), self.d1.data_ptr(), self.h0.data_ptr(), self.h1.data_ptr()


def _ragged_counts(counts, B, device) -> _Counts:
    """counts: a pack_ragged dict, or (counts0, counts1) as tensors or sequences -> device and host int32 copies of both
    (a ``_Counts`` is handed back as it is)."""
    if isinstance(counts, _Counts):
        return counts
    if isinstance(counts, dict):
        h0, h1 = counts['counts0_host'], counts['counts1_host']
    else:
        h0, h1 = (torch.as_tensor(c).detach().to('cpu', torch.int32).contiguous() for c in counts)
    h0, h1 = h0.to(torch.int32).contiguous(), h1.to(torch.int32).contiguous()
    if h0.shape != (B,) or h1.shape != (B,):
        raise ValueError(f'counts: expected two vectors of {B} entries, got {tuple(h0.shape)} / {tuple(h1.shape)}')
    if isinstance(counts, dict) and counts['counts0'].device == device:
        d0, d1 = counts['counts0'].contiguous(), counts['counts1'].contiguous()
    else:
        d0, d1 = h0.to(device), h1.to(device)
    return _Counts(d0, d1, h0, h1)


def _entry(name, counts, B, device):
    """The entry that runs a batch: ``name`` for a uniform one (``counts`` None), ``name_ragged`` fed the count vectors for a ragged one.
    Returns (the entry's name, its leading arguments behind B, N, M, the tensors those point into - to be kept until the call is made)."""
    if counts is None:
        return name, (), None
    cnt = _ragged_counts(counts, B, device)
    return name + '_ragged', cnt.ptrs(), cnt


def _sinkhorn_f64_entry(name, counts, form, B, device):
    """``_entry`` for the two fp64 Sinkhorn ops, whose ragged batches have a second entry: ``form='streaming'`` runs the streaming form's
    (``name_stream_ragged``).  Returns ``_entry``'s triple and the function that sizes the entry's workspace."""
    lib = _lib.load()
    if form not in (None, 'streaming'):
        raise ValueError(f"form={form!r}: expected None or 'streaming'")
    if form is not None and counts is None:
        raise ValueError("form='streaming' selects the ragged entry of the streaming form: it needs counts (a uniform batch follows set_f64_sinkhorn_form)")
    entry, lead, keep = _entry(name, counts, B, device)
    if counts is None:
        return entry, lead, keep, lib.mdgat_sinkhorn_f64_workspace_bytes
    if form == 'streaming':
        return name + '_stream_ragged', lead, keep, lib.mdgat_sinkhorn_f64_stream_ragged_workspace_bytes
    return entry, lead, keep, lib.mdgat_sinkhorn_f64_ragged_workspace_bytes


def pack_frames(frames, device) -> dict:
    """A bank of frames from their raw keypoint records: a list of [n_i, 37] float32 arrays (numpy or torch), as
    ``np.fromfile(path, dtype=np.float32).reshape(-1, 37)`` gives the KITTI keypoint files (load_data.py:146-165) - a whole sequence, or
    whatever a test list walks.  Returns ``{'records': [R, 37] float32 on ``device`` (one concatenation, one upload), 'starts': int64
    [F], 'counts': int32 [F]}`` (host tensors): frame i is rows ``starts[i] .. starts[i] + counts[i]`` of ``records``.  A frame may be
    empty; another width than 37 raises ``ValueError`` naming the frame; other dtypes are narrowed to float32.  Pure torch up to the
    upload.  A chunk of pairs is then two index vectors into the bank (``assemble_frames_ragged``, ``MDGAT.match_frames_ragged``)."""
    rows = []
    for i, f in enumerate(frames):
        t = torch.as_tensor(f)
        if t.dim() != 2 or t.shape[1] != 37:
            raise ValueError(f'pack_frames: frame {i} has shape {tuple(t.shape)}: expected [n, 37] records = xyz | saliency | 33-D FPFH')
        rows.append(t.detach().to(device='cpu', dtype=torch.float32))
    if not rows:
        raise ValueError('pack_frames: no frames')
    counts = torch.tensor([int(t.shape[0]) for t in rows], dtype=torch.int32)
    starts = torch.zeros(len(rows), dtype=torch.int64)
    starts[1:] = torch.cumsum(counts[:-1].to(torch.int64), 0)
    return {'records': torch.cat(rows).contiguous().to(device), 'starts': starts, 'counts': counts}


def frames_chunk(bank, idx0, idx1):
    """The chunk of pairs (idx0[b], idx1[b]) of a ``pack_frames`` bank, checked on the host: (counts0, counts1) int32 [B] and
    (starts0, starts1) int64 [B], CPU tensors.  ``ValueError`` for index vectors of different length, ``IndexError`` for an index
    outside the bank.  Needs no device."""
    i0, i1 = (torch.as_tensor(i, dtype=torch.int64).detach().to('cpu').reshape(-1) for i in (idx0, idx1))
    if i0.numel() != i1.numel():
        raise ValueError(f'idx0 holds {i0.numel()} frames, idx1 {i1.numel()}: a chunk is one frame of each per pair')
    F = int(bank['counts'].numel())
    for name, i in (('idx0', i0), ('idx1', i1)):
        out = ((i < 0) | (i >= F)).nonzero()
        if out.numel():
            b = int(out[0])
            raise IndexError(f'{name}[{b}] = {int(i[b])}: the bank holds frames 0 .. {F - 1}')
    counts, starts = bank['counts'].to(torch.int32), bank['starts'].to(torch.int64)
    return (counts[i0].contiguous(), counts[i1].contiguous()), (starts[i0].contiguous(), starts[i1].contiguous())


def _frames_args(bank, counts, starts, records=None):
    """the device copies of a chunk's counts and starts (one upload each) and the argument list the library's two record entries share"""
    rec = bank['records'] if records is None else records
    _need_cuda(rec)
    if rec.dtype != torch.float32 or rec.dim() != 2 or rec.shape[1] != 37 or not rec.is_contiguous():
        raise ValueError(f"bank['records'] {tuple(rec.shape)} {rec.dtype}: expected contiguous float32 [R, 37] (ops.pack_frames)")
    dev = rec.device
    dc = torch.stack(list(counts)).to(dev)
    ds = torch.stack(list(starts)).to(dev)
    s0, s1 = starts
    args = (*_Counts(dc[0], dc[1], *counts).ptrs(), ds[0].data_ptr(), ds[1].data_ptr(), s0.data_ptr(), s1.data_ptr(),
            rec.data_ptr(), int(rec.shape[0]), rec.data_ptr(), int(rec.shape[0]))
    return args, dc, ds


def assemble_frames_ragged(bank, idx0, idx1, normalize: bool = True) -> dict:
    """What the loader makes of the records of a chunk of pairs, on the device (csrc/f64.hip, the ragged assemble kernel alone): frames
    ``idx0[b]`` / ``idx1[b]`` of a ``pack_frames`` bank, decoded, the FPFH rows L2-normalised in float32 exactly as numpy does it
    (load_data.py:290-292; ``normalize``), widened to float64 and padded with zeros to the largest count.  Returns a ``pack_ragged``-shaped
    dict ``forward_ragged`` accepts - ``keypoints0/1`` [B, Np | Mp, 3], ``scores0/1``, ``descriptors0/1`` [.., 33] (views of the
    kernel's two outputs), ``counts0/1`` and their ``_host`` copies - plus ``keypoints0_f32`` / ``keypoints1_f32`` (the float32 keypoints
    ``gt_matches`` and ``evaluate_matches`` take) and ``range_violation`` (int32 [1] on the device: 1 when a record of a pair held a
    non-finite word or an all-zero FPFH row; reading it synchronises).  Records no pair points at are never read."""
    counts, starts = frames_chunk(bank, idx0, idx1)
    h0, h1 = counts
    B = int(h0.numel())
    if B == 0 or int(h0.min()) < 1 or int(h1.min()) < 1:
        raise ValueError('assemble_frames_ragged: an empty chunk or a pair with an empty frame has nothing to assemble')
    Np, Mp = int(h0.max()), int(h1.max())
    args, dc, ds = _frames_args(bank, counts, starts)
    dev = bank['records'].device
    in4 = torch.empty((B, Np + Mp, 4), dtype=torch.float64, device=dev)
    in33 = torch.empty((B, Np + Mp, 33), dtype=torch.float64, device=dev)
    kp0 = torch.empty((B, Np, 3), dtype=torch.float32, device=dev)
    kp1 = torch.empty((B, Mp, 3), dtype=torch.float32, device=dev)
    guard = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mdgat_assemble_frames_f64_ragged(B, Np, Mp, *args, int(bool(normalize)), in4.data_ptr(), in33.data_ptr(), kp0.data_ptr(),
                                                                kp1.data_ptr(), guard.data_ptr(), _stream(in4)), 'mdgat_assemble_frames_f64_ragged')
    return {'keypoints0': in4[:, :Np, :3], 'scores0': in4[:, :Np, 3], 'descriptors0': in33[:, :Np],
            'keypoints1': in4[:, Np:, :3], 'scores1': in4[:, Np:, 3], 'descriptors1': in33[:, Np:],
            'counts0': dc[0], 'counts1': dc[1], 'counts0_host': h0, 'counts1_host': h1,
            'keypoints0_f32': kp0, 'keypoints1_f32': kp1, 'range_violation': guard}


TRAIN_MAX_KEYPOINTS = 2048      # max_keypoints of assemble_frames_train: the attention's limit


def assemble_frames_train(bank, idx0, idx1, max_keypoints: int, min_saliency: float = 10.0, normalize: bool = True) -> dict:
    """What the loader makes of a chunk of pairs in TRAIN mode (``ensure_kpts_num``, train.py's default for the training and the
    validation set; load_data.py:180-211), on the device in one launch: of frames ``idx0[b]`` / ``idx1[b]`` of a ``pack_frames`` bank the
    records with saliency > ``min_saliency`` (float32; exactly ``min_saliency`` and NaN are dropped) in their order, the first
    ``T = max_keypoints`` of them or - when there are fewer - padded to T by the loader's loop ``vstack((a[:T - len(a)], a))``; then
    decoded, the FPFH rows L2-normalised in float32 exactly as numpy does it (``normalize``), widened to float64.  Returns uniform
    ``keypoints0/1`` [B, T, 3], ``scores0/1`` [B, T], ``descriptors0/1`` [B, T, 33] (float64 views of the kernel's two outputs),
    ``keypoints0_f32/1_f32`` (what ``gt_matches`` takes), ``source0/1`` (int32 [B, T]: the record's row within its frame behind each
    slot), ``salient0/1`` (int32 [B]: records kept) and two device words, which to read synchronises: ``status`` (int32 [B, 2]: 1 where
    frame 0 / 1 of a pair kept NO record - the reference's loop never ends there; that frame's rows are unwritten) and
    ``range_violation`` (int32 [1]: a kept record held a non-finite word or an all-zero FPFH row).  Dropped records are never decoded,
    records no pair points at never read.  ``ValueError`` for an empty chunk, ``max_keypoints`` outside 1 .. 2048 and a frame without
    records."""
    counts, starts = frames_chunk(bank, idx0, idx1)
    h0, h1 = counts
    B, T = int(h0.numel()), int(max_keypoints)
    if B == 0:
        raise ValueError('assemble_frames_train: an empty chunk has nothing to assemble')
    if not 1 <= T <= TRAIN_MAX_KEYPOINTS:
        raise ValueError(f'assemble_frames_train: max_keypoints={max_keypoints}: expected 1 .. {TRAIN_MAX_KEYPOINTS} (the attention\'s limit)')
    for f, h in enumerate(counts):
        if int(h.min()) < 1:
            raise ValueError(f'assemble_frames_train: pair {int(h.argmin())}: frame {f} holds no record')
    args, dc, ds = _frames_args(bank, counts, starts)
    dev = bank['records'].device
    in4 = torch.empty((B, 2 * T, 4), dtype=torch.float64, device=dev)
    in33 = torch.empty((B, 2 * T, 33), dtype=torch.float64, device=dev)
    kp0, kp1 = (torch.empty((B, T, 3), dtype=torch.float32, device=dev) for _ in '01')
    src0, src1 = (torch.empty((B, T), dtype=torch.int32, device=dev) for _ in '01')
    sal0, sal1 = (torch.empty((B,), dtype=torch.int32, device=dev) for _ in '01')
    status = torch.empty((B, 2), dtype=torch.int32, device=dev)
    guard = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mdgat_assemble_frames_train_f64(B, T, *args, float(min_saliency), int(bool(normalize)), in4.data_ptr(), in33.data_ptr(),
                                                               kp0.data_ptr(), kp1.data_ptr(), src0.data_ptr(), src1.data_ptr(), sal0.data_ptr(),
                                                               sal1.data_ptr(), status.data_ptr(), guard.data_ptr(), _stream(in4)),
                   'mdgat_assemble_frames_train_f64')
    return {'keypoints0': in4[:, :T, :3], 'scores0': in4[:, :T, 3], 'descriptors0': in33[:, :T],
            'keypoints1': in4[:, T:, :3], 'scores1': in4[:, T:, 3], 'descriptors1': in33[:, T:],
            'keypoints0_f32': kp0, 'keypoints1_f32': kp1, 'source0': src0, 'source1': src1, 'salient0': sal0, 'salient1': sal1,
            'range_violation': guard, 'status': status}


def sinkhorn_f64(scores: torch.Tensor, bin_score: float, iters: int, counts=None, form=None) -> torch.Tensor:
    """log_optimal_transport (mdgat.py:288-308) in fp64 (csrc/sinkhorn_f64.hip): scores [B, N, M] float64 -> Z [B, N+1, M+1] float64.

    ``counts`` (a ``pack_ragged`` dict or ``(counts0, counts1)``): a ragged batch - pair b is ``scores[b, :counts0[b], :counts1[b]]``,
    the rest of its slot is never read.  ``Z[b, :counts0[b]+1, :counts1[b]+1]`` then has the bits of the pair run alone (its dustbins at
    row ``counts0[b]`` / column ``counts1[b]``), the rest of the slot is 0.  N, M <= 575; the forward only.

    ``form='streaming'`` (with counts): the ragged entry of the streaming form (K in memory, one launch per iteration), in slots of
    N, M <= 2175 - small ones included.  Pair b then has the bits of the pair run alone under ``set_f64_sinkhorn_form(1)``; against the
    pair alone on the register-resident form it agrees to fp64 rounding.  The call is asynchronous.  The workspace holds K for the whole
    slot, ``B * N * roundup(M + 1, 128)`` doubles: 35.6 MB per pair at 2048."""
    _need_cuda(scores)
    if counts is not None and scores.requires_grad:
        raise RuntimeError('sinkhorn_f64(counts=): ragged batches run the forward only (no gradient)')
    s = scores.to(torch.float64).contiguous()
    B, N, M = s.shape
    Z = torch.empty((B, N + 1, M + 1), dtype=torch.float64, device=s.device)
    lib = _lib.load()
    with torch.cuda.device(s.device):
        name, lead, _keep, size = _sinkhorn_f64_entry('mdgat_sinkhorn_f64', counts, form, B, s.device)
        ws, base, need = _workspace(size(B, N, M), s.device)
        _lib.check(getattr(lib, name)(B, N, M, *lead, s.data_ptr(), float(bin_score), int(iters), Z.data_ptr(), base, need, _stream(s)), name)
    return Z


def sinkhorn_f64_extract(scores: torch.Tensor, bin_score: float, iters: int, mode: int = _lib.EXTRACT_DUSTBIN, match_threshold: float = 0.2,
                         want_Z: bool = False, counts=None, form=None):
    """fp64 Sinkhorn + match extraction with every arg-max decided on the fp64 Z: (matches0, matches1, mscores0, mscores1[, Z fp32]).

    ``counts`` as in ``sinkhorn_f64``: pair b's matches and scores are those of the pair run alone (no match: -1; the rule of
    mdgat.py:465-467 per pair); beyond its counts matches are -1 and scores 0.  ``form='streaming'`` as in ``sinkhorn_f64``."""
    _need_cuda(scores)
    if counts is not None and scores.requires_grad:
        raise RuntimeError('sinkhorn_f64_extract(counts=): ragged batches run the forward only (no gradient)')
    s = scores.to(torch.float64).contiguous()
    B, N, M = s.shape
    m0, m1, s0, s1, Z = _match_outputs(B, N, M, s.device, want_Z)
    lib = _lib.load()
    with torch.cuda.device(s.device):
        name, lead, _keep, size = _sinkhorn_f64_entry('mdgat_sinkhorn_f64_extract', counts, form, B, s.device)
        ws, base, need = _workspace(size(B, N, M), s.device)
        _lib.check(getattr(lib, name)(B, N, M, *lead, s.data_ptr(), float(bin_score), int(iters), int(mode), float(match_threshold), m0.data_ptr(),
                                      m1.data_ptr(), s0.data_ptr(), s1.data_ptr(), Z.data_ptr() if Z is not None else None, base, need, _stream(s)), name)
    return (m0, m1, s0, s1, Z) if want_Z else (m0, m1, s0, s1)


def sinkhorn_backward(scores: torch.Tensor, bin_score, iters: int, dZ: torch.Tensor):
    """Gradient of log_optimal_transport (mdgat.py:288-308; csrc/sinkhorn_grad.hip): scores [B, N, M] (float32 or float64), the bin
    score, ``iters`` >= 0 and dZ = dL/dZ [B, N+1, M+1] (any dtype and strides) -> (dscores [B, N, M] in the scores' dtype, dbin [B]
    float64: the bin score's gradient per pair).  The arithmetic is fp64 for both input dtypes.  N, M <= 2175."""
    _need_cuda(scores, dZ)
    if scores.dim() != 3:
        raise ValueError(f'scores must be [B, N, M], got {tuple(scores.shape)}')
    B, N, M = scores.shape
    if tuple(dZ.shape) != (B, N + 1, M + 1):
        raise ValueError(f'dZ {tuple(dZ.shape)} does not fit scores {tuple(scores.shape)}: expected [{B}, {N + 1}, {M + 1}]')
    if dZ.device != scores.device:
        raise ValueError(f'dZ is on {dZ.device}, scores on {scores.device}')
    s = scores.to(torch.float64).contiguous()
    g = dZ.to(torch.float64).contiguous()          # (Z.sum().backward() hands over an expanded, stride-0 tensor)
    dscores = torch.empty((B, N, M), dtype=torch.float64, device=s.device)
    dbin = torch.empty((B,), dtype=torch.float64, device=s.device)
    lib = _lib.load()
    with torch.cuda.device(s.device):
        ws, base, need = _workspace(lib.mdgat_sinkhorn_backward_workspace_bytes(B, N, M, int(iters)), s.device)
        _lib.check(lib.mdgat_sinkhorn_backward(B, N, M, s.data_ptr(), float(bin_score), int(iters), g.data_ptr(), dscores.data_ptr(),
                                               dbin.data_ptr(), base, need, _stream(s)), 'mdgat_sinkhorn_backward')
    return dscores.to(scores.dtype), dbin


_ARITHMETIC = ('auto', 'fp32', 'fp64')


class _LogOptimalTransport(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, alpha, iters, arithmetic):
        a = float(alpha)
        f64 = arithmetic == 'fp64' or (arithmetic == 'auto' and scores.dtype == torch.float64)
        Z = (sinkhorn_f64 if f64 else sinkhorn)(scores, a, iters).to(scores.dtype)
        ctx.save_for_backward(scores)
        ctx.alpha, ctx.iters = a, iters
        ctx.alpha_like = alpha if isinstance(alpha, torch.Tensor) else None
        return Z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dZ):
        scores, = ctx.saved_tensors
        dscores, dbin = sinkhorn_backward(scores, ctx.alpha, ctx.iters, dZ)
        dalpha = None
        if ctx.needs_input_grad[1]:
            al = ctx.alpha_like
            dalpha = dbin.sum().to(device=al.device, dtype=al.dtype).reshape(al.shape)
        return (dscores if ctx.needs_input_grad[0] else None), dalpha, None, None


def log_optimal_transport(scores: torch.Tensor, alpha, iters: int, arithmetic: str = 'auto') -> torch.Tensor:
    """Differentiable log_optimal_transport (mdgat.py:288-308): scores [B, N, M] -> Z [B, N+1, M+1] in the scores' dtype.

    The forward is ``sinkhorn_f64`` for float64 scores and ``sinkhorn`` for float32 ones (``arithmetic='fp32'`` / ``'fp64'`` pins one,
    the vocabulary of MDGAT's ``arithmetic`` config key); the backward is the fp64 kernel of ``sinkhorn_backward`` for both.  Gradients
    flow to ``scores`` and to ``alpha`` when it is a tensor that requires grad (summed over the batch, alpha's shape and dtype).
    Not twice differentiable; N, M <= 2175 for the backward."""
    if arithmetic not in _ARITHMETIC:
        raise ValueError(f'arithmetic must be one of {_ARITHMETIC}, got {arithmetic!r}')
    _need_cuda(scores)
    if scores.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'scores must be float32 or float64, got {scores.dtype}')
    return _LogOptimalTransport.apply(scores, alpha, int(iters), arithmetic)


def extract(Z: torch.Tensor, mode: int = _lib.EXTRACT_DUSTBIN, match_threshold: float = 0.2):
    """Match extraction (mdgat.py:441-483) from Z [B, N+1, M+1]."""
    _need_cuda(Z)
    z = Z.to(torch.float32).contiguous()
    B, N, M = z.shape[0], z.shape[1] - 1, z.shape[2] - 1
    m0 = torch.empty((B, N), dtype=torch.int64, device=z.device)
    m1 = torch.empty((B, M), dtype=torch.int64, device=z.device)
    s0 = torch.empty((B, N), dtype=torch.float32, device=z.device)
    s1 = torch.empty((B, M), dtype=torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        _lib.check(_lib.load().mdgat_extract(B, N, M, z.data_ptr(), int(mode), float(match_threshold), m0.data_ptr(),
                                             m1.data_ptr(), s0.data_ptr(), s1.data_ptr(), _stream(z)), 'mdgat_extract')
    return m0, m1, s0, s1


def topk_sel_words(B: int, N: int, M: int) -> int:
    """uint32 words of one layer's slice of the top-k selection tap (``mdgat_taps.topk_sel``)."""
    return int(_lib.load().mdgat_topk_sel_words(B, N, M))


def topk_sel_to_masks(sel: torch.Tensor, B: int, N: int, M: int, cross: bool):
    """Unpack one layer's selection tap (int32 words [B][4][N+M][W]) into boolean masks
    ``(mask0 [B, 4, N, keys of frame 0's source], mask1 [B, 4, M, keys of frame 1's source])``: True where the dynamic
    layer kept the key (the index set of ``logits.topk(k)``, mdgat.py:202)."""
    W = (max(N, M) + 31) // 32
    w = sel.reshape(B, 4, N + M, W).to(torch.int64) & 0xFFFFFFFF
    bits = ((w[..., None] >> torch.arange(32, device=w.device)) & 1).bool().reshape(B, 4, N + M, W * 32)
    nk0, nk1 = (M, N) if cross else (N, M)
    return bits[:, :, :N, :nk0], bits[:, :, N:, :nk1]


def _selection_masks(sel, B, N, M, cross, topk, cnt, device):
    """The masks ``return_selection`` hands out: (mask0 [B, 4, N, keys of frame 0's source], mask1 [B, 4, M, keys of frame 1's source]).
    A dynamic layer (``topk`` > 0): the library's selection words, decoded.  Full attention writes no words (include/mdgat_hip.h: "slices
    of full-attention layers are left untouched") and is asked for none: every key of the query's source frame is kept - of a ragged
    batch (``cnt``: its ``_Counts``), every key within the pair's counts for every query within them."""
    if topk > 0:
        return topk_sel_to_masks(sel, B, N, M, cross)
    keys0, keys1 = (M, N) if cross else (N, M)
    mask0 = torch.ones((B, 4, N, keys0), dtype=torch.bool, device=device)
    mask1 = torch.ones((B, 4, M, keys1), dtype=torch.bool, device=device)
    if cnt is not None:
        n0, n1 = cnt.d0.to(torch.int64)[:, None, None, None], cnt.d1.to(torch.int64)[:, None, None, None]
        k0, k1 = (n1, n0) if cross else (n0, n1)
        rows, cols = (lambda n: torch.arange(n, device=device)[None, None, :, None]), (lambda n: torch.arange(n, device=device)[None, None, None, :])
        mask0 &= (rows(N) < n0) & (cols(keys0) < k0)
        mask1 &= (rows(M) < n1) & (cols(keys1) < k1)
    return mask0, mask1


def attention(qkv: torch.Tensor, N: int, M: int, cross: bool, topk: int = 0, return_selection: bool = False, counts=None, wide: bool = False):
    """attention / dynamic_attention (mdgat.py:190-210).  qkv [B, N+M, 3, 4, 32] -> message [B, N+M, 128]
    (with ``return_selection``: also the boolean masks of the keys a dynamic layer kept, see topk_sel_to_masks; full attention keeps
    every key of a pair: all True within its counts).
    The fp32-class kernels have no backward: the result never carries a grad_fn (``attention_f64`` is the differentiable one).

    ``counts`` (a ``pack_ragged`` dict or ``(counts0, counts1)``): a ragged batch - pair b has ``counts0[b]`` / ``counts1[b]`` keypoints in
    slots of N / M <= 512 rows; its rows are those of its own q/k/v rows alone, bit-identical wherever it stands in a batch of the same slots;
    message rows and masks beyond its counts are zero / False, and what ``qkv`` holds there reaches no result.  ``wide=True`` (with counts):
    slots of up to 2048 rows (``mdgat_attention_ragged_wide``) - the same contract; slots within 512 run the same kernels and give the same bits."""
    if wide and counts is None:
        raise ValueError('wide selects the wide ragged entry: it needs counts')
    _need_cuda(qkv)
    x = qkv.to(torch.float32).contiguous()
    B, P = x.shape[0], x.shape[1]
    assert P == N + M and tuple(x.shape[2:]) == (3, 4, 32)
    msg = torch.empty((B, P, 128), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        need = lib.mdgat_attention_workspace_bytes(B, N, M)
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        sel = torch.empty(topk_sel_words(B, N, M), dtype=torch.int32, device=x.device) if return_selection and topk > 0 else None
        name, lead, cnt = _entry('mdgat_attention', counts, B, x.device)
        if wide:
            name += '_wide'
        _lib.check(getattr(lib, name if counts is not None else 'mdgat_attention_sel')(
            B, N, M, *lead, int(bool(cross)), int(topk), x.data_ptr(), msg.data_ptr(), sel.data_ptr() if sel is not None else None,
            ws.data_ptr(), need, _stream(x)), name)
    if return_selection:
        return msg, _selection_masks(sel, B, N, M, cross, int(topk), cnt, x.device)
    return msg


class QkProbe:
    """Measurement only (bench.py ``roofline_qk``): the Q K^T phase of the streamed full-attention kernel in isolation
    (``mdgat_attention_qk_probe``).  ``QkProbe(qkv, N, M)`` converts fp32 q/k/v [B, N+M, 3, 4, 32] to the library's split
    layout once; ``run(cross)`` launches only the probe kernel on the current stream."""

    def __init__(self, qkv: torch.Tensor, N: int, M: int):
        _need_cuda(qkv)
        x = qkv.to(torch.float32).contiguous()
        self.B, self.N, self.M = x.shape[0], N, M
        assert x.shape[1] == N + M and tuple(x.shape[2:]) == (3, 4, 32)
        self.lib = _lib.load()
        with torch.cuda.device(x.device):
            self.need = self.lib.mdgat_attention_workspace_bytes(self.B, N, M)
            self.ws = torch.empty(self.need, dtype=torch.uint8, device=x.device)
            self.msg = torch.zeros((self.B, N + M, 128), dtype=torch.float32, device=x.device)
            _lib.check(self.lib.mdgat_attention_qk_probe(self.B, N, M, 0, x.data_ptr(), self.msg.data_ptr(), self.ws.data_ptr(),
                                                         self.need, _stream(x)), 'mdgat_attention_qk_probe')

    def run(self, cross: bool = False, nq_sets: int = 0):
        """nq_sets = 0: the Q K^T phase of the shipped kernel (softmax and P.V knocked out); 1 / 2: the standalone phase kernel
        with 32 / 64 queries per wave (``mdgat_attention_qk_probe_sets``)."""
        with torch.cuda.device(self.ws.device):
            if nq_sets:
                _lib.check(self.lib.mdgat_attention_qk_probe_sets(self.B, self.N, self.M, int(bool(cross)), int(nq_sets), self.ws.data_ptr(),
                                                                  self.msg.data_ptr(), self.ws.data_ptr(), self.need, _stream(self.ws)),
                           'mdgat_attention_qk_probe_sets')
            else:
                _lib.check(self.lib.mdgat_attention_qk_probe(self.B, self.N, self.M, int(bool(cross)), self.ws.data_ptr(),
                                                             self.msg.data_ptr(), self.ws.data_ptr(), self.need, _stream(self.ws)),
                           'mdgat_attention_qk_probe')
        return self.msg


def mfma_sustained(device, reps: int = 4000) -> dict:
    """Measurement only (bench.py ``roofline.sustained_*``): the f16 MFMA rate ``device`` sustains on random operands
    (``mdgat_mfma_probe``: nothing but matrix instructions, two waves per SIMD) and the shader clock it runs at meanwhile."""
    import ctypes as C
    device = torch.device(device)
    lib = _lib.load()
    with torch.cuda.device(device):
        ws = torch.empty(1 << 18, dtype=torch.uint8, device=device)
        ms, flops, ticks = C.c_float(), C.c_double(), C.c_longlong()
        _lib.check(lib.mdgat_mfma_probe(reps, ws.data_ptr(), ws.numel(), C.byref(ms), C.byref(flops), C.byref(ticks),
                                        torch.cuda.current_stream(device).cuda_stream), 'mdgat_mfma_probe')
    return {'tflops': flops.value / (ms.value * 1e-3) / 1e12, 'clock_ghz': ticks.value / (ms.value * 1e6),
            'ms': ms.value, 'ticks_per_mfma_per_simd': ticks.value / (24.0 * reps * 2)}


def pointwise(A: torch.Tensor, W: torch.Tensor, bias=None, relu=False, residual=None) -> torch.Tensor:
    """Conv1d(k=1) over points: A [rows, K] x W [Cout, K]^T (+bias, ReLU, +residual) -> [rows, Cout]."""
    _need_cuda(A, W)
    a = A.to(torch.float32).contiguous()
    w = W.to(torch.float32).contiguous()
    rows, K = a.shape
    cout = w.shape[0]
    assert w.shape[1] == K
    b = bias.to(torch.float32).contiguous() if bias is not None else None
    r = residual.to(torch.float32).contiguous() if residual is not None else None
    out = torch.empty((rows, cout), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().mdgat_pointwise(rows, cout, K, a.data_ptr(), K, w.data_ptr(), K,
                                               b.data_ptr() if b is not None else None, int(relu),
                                               r.data_ptr() if r is not None else None, cout, out.data_ptr(), cout,
                                               _stream(a)), 'mdgat_pointwise')
    return out


def knn(x: torch.Tensor, src: torch.Tensor, k: int, adjacency: bool = False, mfma: bool = True):
    """knn / get_graph_feature (mdgat.py:8-32).  Channel-major inputs like the reference: x [B, C, N], src [B, C, M].
    ``mfma=False`` keeps C = 128 off the matrix cores (distances computed inside the selection kernel)."""
    _need_cuda(x, src)
    xp = x.to(torch.float32).transpose(1, 2).contiguous()
    sp = src.to(torch.float32).transpose(1, 2).contiguous()
    B, N, Cc = xp.shape
    M = sp.shape[1]
    idx = torch.empty((B, N, k), dtype=torch.int64, device=x.device)
    adj = torch.empty((B, N, M), dtype=torch.int64, device=x.device) if adjacency else None
    lib = _lib.load()
    with torch.cuda.device(x.device):
        need = lib.mdgat_knn_workspace_bytes(B, Cc, N, M) if mfma else 0      # C == 128: inner products on the matrix cores
        ws = torch.empty(need, dtype=torch.uint8, device=x.device) if need else None
        _lib.check(lib.mdgat_knn(B, Cc, N, M, int(k), xp.data_ptr(), sp.data_ptr(), idx.data_ptr(),
                                 adj.data_ptr() if adj is not None else None,
                                 ws.data_ptr() if ws is not None else None, need, _stream(x)), 'mdgat_knn')
    return (idx, adj) if adjacency else idx


def pose_from_matches(kpts0: torch.Tensor, kpts1: torch.Tensor, matches0: torch.Tensor, T_gt=None, inlier_dist: float = 1.0):
    """solve_icp + calculate_error (utils/utils_test.py:41-110) for a batch: kpts [B, N, 3] / [B, M, 3], matches0
    [B, N] int64 (-1 = unmatched).  Returns (T [B, 4, 4] float64 mapping frame 1 onto frame 0, stats [B, 5] float64 =
    matches, inliers, inlier ratio, translation error, rotation error; the errors are NaN without ``T_gt``)."""
    _need_cuda(kpts0, kpts1, matches0)
    k0 = kpts0.to(torch.float32).contiguous()
    k1 = kpts1.to(torch.float32).contiguous()
    m0 = matches0.to(torch.int64).contiguous()
    B, N, M = k0.shape[0], k0.shape[1], k1.shape[1]
    T = torch.empty((B, 4, 4), dtype=torch.float64, device=k0.device)
    stats = torch.empty((B, 5), dtype=torch.float64, device=k0.device)
    g = T_gt.to(device=k0.device, dtype=torch.float64).contiguous() if T_gt is not None else None
    with torch.cuda.device(k0.device):
        _lib.check(_lib.load().mdgat_pose(B, N, M, k0.data_ptr(), k1.data_ptr(), m0.data_ptr(),
                                          g.data_ptr() if g is not None else None, float(inlier_dist), T.data_ptr(),
                                          stats.data_ptr(), _stream(k0)), 'mdgat_pose')
    return T, stats


def gt_matches(kpts0: torch.Tensor, kpts1: torch.Tensor, T0=None, T1=None, threshold: float = 0.5, mutual: bool = False, counts=None):
    """Ground-truth matches of the loader (load_data.py:238-285): kpts [B, N, 3] / [B, M, 3] in the sensor frame,
    T0 / T1 [B, 4, 4] float64 sensor -> world (None = identity).  Returns (gt_matches0 [B, N], gt_matches1 [B, M],
    rep [B]) as int64, -1 = no match.

    ``counts`` (a ``pack_ragged`` dict or ``(counts0, counts1)``): a ragged batch in padded slots - pair b's matches and rep are those of
    the pair alone, -1 beyond its counts; the keypoints there are not read."""
    _need_cuda(kpts0, kpts1)
    k0 = kpts0.to(torch.float32).contiguous()
    k1 = kpts1.to(torch.float32).contiguous()
    B, N, M = k0.shape[0], k0.shape[1], k1.shape[1]
    g0 = torch.empty((B, N), dtype=torch.int64, device=k0.device)
    g1 = torch.empty((B, M), dtype=torch.int64, device=k0.device)
    rep = torch.empty((B,), dtype=torch.int64, device=k0.device)
    t0 = T0.to(device=k0.device, dtype=torch.float64).contiguous() if T0 is not None else None
    t1 = T1.to(device=k0.device, dtype=torch.float64).contiguous() if T1 is not None else None
    for name, t in (('T0', t0), ('T1', t1)):
        if counts is not None and t is not None and tuple(t.shape) != (B, 4, 4):
            raise ValueError(f'{name} {tuple(t.shape)}: expected [{B}, 4, 4]')
    tail = (t0.data_ptr() if t0 is not None else None, t1.data_ptr() if t1 is not None else None, float(threshold), int(bool(mutual)),
            g0.data_ptr(), g1.data_ptr(), rep.data_ptr(), _stream(k0))
    with torch.cuda.device(k0.device):
        name, lead, _keep = _entry('mdgat_gt_matches', counts, B, k0.device)
        _lib.check(getattr(_lib.load(), name)(B, N, M, *lead, k0.data_ptr(), k1.data_ptr(), *tail), name)
    return g0, g1, rep


# ---- the evaluation scripts' per-pair record (csrc/eval_metrics.hip) ----
class _EvalColumns(dict):
    """Column name -> index of the table ``evaluate_matches`` returns (``mdgat_eval_column`` of include/mdgat_hip.h), also as
    attributes (``EvalColumns.precision``), and the status bits (``mdgat_eval_status``)."""
    BANNED = _lib.EVAL_BANNED
    TOO_FEW_MATCHES = _lib.EVAL_TOO_FEW_MATCHES
    REGISTRATION_FAIL = _lib.EVAL_REGISTRATION_FAIL
    RTE_OK = _lib.EVAL_RTE_OK
    RRE_OK = _lib.EVAL_RRE_OK

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


EvalColumns = _EvalColumns((name, i) for i, name in enumerate(_lib.EVAL_COLUMNS))


def evaluate_matches(matches0: torch.Tensor, matches1: torch.Tensor, gt0: torch.Tensor, gt1: torch.Tensor, kpts0: torch.Tensor,
                     kpts1: torch.Tensor, T_gt=None, inlier_dist: float = 1.0, counts=None):
    """What test.py:212-296 and test_registration_metric.py:213-264 derive per pair from the matcher's output, on the device:
    matches0 / gt0 [B, N], matches1 / gt1 [B, M] (-1, or the dustbin value M / N in the gts, = unmatched), kpts [B, N, 3] / [B, M, 3]
    and T_gt [B, 4, 4] as ``pose_from_matches`` takes them.  Returns (metrics [B, len(EvalColumns)] float64, T [B, 4, 4] float64,
    EvalColumns): counts exact, every ratio bit for bit numpy's value (0/0 = NaN and x/0 = inf where the script does not guard), the
    pose columns ``pose_from_matches``' arithmetic, and a status column with the scripts' skip rules as bits - the row is filled either
    way (``EvalMeter`` applies the rules).  A gt outside [-1, M] / [-1, N] raises ``IndexError`` like the loss; the tensors are not
    rewritten.  Reading the bad-index word synchronises, as in ``matching_loss``.

    ``counts`` (a ``pack_ragged`` dict or ``(counts0, counts1)``): a ragged batch in padded slots - pair b's row and T are those of the pair
    alone, what lies beyond its counts (the -1 padding of matches and gts, the zero keypoints) is not read."""
    _need_cuda(matches0, kpts0, kpts1)
    dev = kpts0.device
    k0 = kpts0.to(torch.float32).contiguous()
    k1 = kpts1.to(device=dev, dtype=torch.float32).contiguous()
    B, N, M = k0.shape[0], k0.shape[1], k1.shape[1]
    m0, m1, g0, g1 = (t.to(device=dev, dtype=torch.int64).contiguous() for t in (matches0, matches1, gt0, gt1))
    for name, t, n in (('matches0', m0, N), ('gt0', g0, N), ('matches1', m1, M), ('gt1', g1, M)):
        if tuple(t.shape) != (B, n):
            raise ValueError(f'{name} {tuple(t.shape)}: expected [{B}, {n}]')
    g = T_gt.to(device=dev, dtype=torch.float64).contiguous() if T_gt is not None else None
    if g is not None and tuple(g.shape) != (B, 4, 4):
        raise ValueError(f'T_gt {tuple(g.shape)}: expected [{B}, 4, 4]')
    metrics = torch.empty((B, len(EvalColumns)), dtype=torch.float64, device=dev)
    T = torch.empty((B, 4, 4), dtype=torch.float64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        name, lead, _keep = _entry('mdgat_eval_metrics', counts, B, dev)
        _lib.check(getattr(_lib.load(), name)(B, N, M, *lead, m0.data_ptr(), m1.data_ptr(), g0.data_ptr(), g1.data_ptr(), k0.data_ptr(), k1.data_ptr(),
                                              g.data_ptr() if g is not None else None, float(inlier_dist), metrics.data_ptr(), T.data_ptr(),
                                              bad.data_ptr(), _stream(k0)), name)
    if int(bad.item()):
        raise IndexError(f'gt_matches hold an index outside [-1, {M}] (gt0) or [-1, {N}] (gt1), or the matches one outside '
                         f'[-1, {M}) / [-1, {N})')
    return metrics, T, EvalColumns


class _Average:
    """utils/utils_test.py:6-25 as far as the scripts read it: a running sum in arrival order and its quotient by the count."""

    def __init__(self):
        self.sum, self.count, self.avg = 0.0, 0, 0

    def update(self, val, n=1):
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


class EvalMeter:
    """Host-side accumulator over the rows of ``evaluate_matches`` (one device-to-host copy of the table per batch), under the two
    scripts' own rules, so that the aggregates equal theirs bit for bit when the rows do:

    test.py:241-311 - repeatability is appended for every pair; a banned pair counts as banned and failed and is skipped; a pair with
    fewer than 4 matches fails; so does one whose pose is off (trans_error > 2, rot_error > 5 or NaN); the others append to every list.
    ``test_py()`` takes ``np.mean`` over those lists (:326-338) and reports ``fail`` and ``baned_data`` both as counts and divided by the
    index of the last batch, which is what :340-342 print (``fail / i``: one less than the number of ``update`` calls).

    test_registration_metric.py:230-269 - a banned pair is skipped; the others feed the running averages (the script's AverageMeter:
    sums in arrival order), RTE / RRE only where they pass, RR with 1 or 0.  ``registration()`` reports what :282-286 print."""

    _TEST_LISTS = ('precision', 'accuracy', 'recall', 'trans_error', 'rot_error', 'inliers', 'inlier_ratio', 'fp_rate', 'tp_rate',
                   'tp_rate2', 'true_positive', 'false_positive')
    _REG_NAMES = ('rep', 'rre', 'rte', 'inlier', 'inlier_ratio', 'recall', 'tp_rate', 'fp_rate', 'RR')

    def __init__(self):
        self.reset()

    def reset(self):
        self.batches = 0
        self.fail = 0
        self.baned_data = 0
        self.reg_baned_data = 0
        self.lists = {name: [] for name in ('repeatability',) + self._TEST_LISTS}
        self.reg = {name: _Average() for name in self._REG_NAMES}

    def update(self, rows):
        """``rows``: the metrics table ([B, COLS], a tensor on any device or an array), or the dict ``MDGAT.evaluate`` returns."""
        if isinstance(rows, dict):
            rows = rows['metrics']
        if isinstance(rows, torch.Tensor):
            rows = rows.detach().cpu().numpy()
        c = EvalColumns
        self.batches += 1
        for r in rows:
            status = int(r[c.status])
            self._update_test_py(r, status)
            self._update_registration(r, status)
        return self

    def _update_test_py(self, r, status):
        c = EvalColumns
        self.lists['repeatability'].append(r[c.repeatability])
        if status & c.BANNED:
            self.baned_data += 1
            self.fail += 1
            return
        if status & (c.TOO_FEW_MATCHES | c.REGISTRATION_FAIL):
            self.fail += 1
            return
        for name in self._TEST_LISTS:
            self.lists[name].append(r[c[name]])

    def _update_registration(self, r, status):
        c, a = EvalColumns, self.reg
        if status & c.BANNED:
            self.reg_baned_data += 1
            return
        a['rep'].update(r[c.repeatability]), a['fp_rate'].update(r[c.fp_rate_reg]), a['tp_rate'].update(r[c.tp_rate_reg])
        a['recall'].update(r[c.recall]), a['inlier_ratio'].update(r[c.precision]), a['inlier'].update(r[c.true_positive])
        if status & c.RTE_OK:
            a['rte'].update(r[c.trans_error])
        if status & c.RRE_OK:
            a['rre'].update(r[c.rot_error])
        a['RR'].update(1 if (status & c.RTE_OK) and (status & c.RRE_OK) else 0)

    def test_py(self):
        """The aggregates test.py:326-342 prints.  An empty list averages to NaN there as well (numpy warns; silenced here)."""
        import numpy as np
        with np.errstate(invalid='ignore', divide='ignore'):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                out = {name + '_mean': np.mean(v) for name, v in self.lists.items()}
            i = np.float64(self.batches - 1)
            out.update(fail=self.fail, baned_data=self.baned_data, fail_rate=np.float64(self.fail) / i,
                       baned_data_rate=np.float64(self.baned_data) / i)
        return out

    def registration(self):
        """The aggregates test_registration_metric.py:282-286 prints."""
        import numpy as np
        out = {name: a.avg for name, a in self.reg.items()}
        p, r = out['inlier_ratio'], out['recall']
        with np.errstate(invalid='ignore', divide='ignore'):
            out['F1'] = np.float64(2 * p * r) / np.float64(p + r)
        out['baned_data'] = self.reg_baned_data
        return out


# ---- fp64 kernels of the reference-exact mode (csrc/f64.hip; MDGAT(arithmetic='fp64') launches the same ones) ----
def pointwise_f64(a: torch.Tensor, w: torch.Tensor, bias=None, relu: bool = False, residual=None) -> torch.Tensor:
    """Conv1d(k=1) over points in fp64 (mdgat.py:34-46 after BN folding): a [M, K] x w [N, K]^T (+ bias)(ReLU)(+ residual)."""
    _need_cuda(a, w)
    a = a.to(torch.float64).contiguous()
    w = w.to(torch.float64).contiguous()
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K
    bias = bias.to(torch.float64).contiguous() if bias is not None else None
    residual = residual.to(torch.float64).contiguous() if residual is not None else None
    out = torch.empty((M, N), dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().mdgat_pointwise_f64(M, N, K, a.data_ptr(), K, w.data_ptr(), K, bias.data_ptr() if bias is not None else None,
                                                   int(bool(relu)), residual.data_ptr() if residual is not None else None, N,
                                                   out.data_ptr(), N, _stream(a)), 'mdgat_pointwise_f64')
    return out


def _attention_f64_values(qkv, N, M, cross, topk, want_sel, counts=None):
    """The forward launch of ``attention_f64``: (message, the raw selection words or None)."""
    _need_cuda(qkv)
    x = qkv.detach().to(torch.float64).contiguous()
    B, P = x.shape[0], x.shape[1]
    assert P == N + M and tuple(x.shape[2:]) == (3, 4, 32)
    msg = torch.empty((B, P, 128), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        sel = torch.empty(topk_sel_words(B, N, M), dtype=torch.int32, device=x.device) if want_sel and int(topk) > 0 else None
        name, lead, _keep = _entry('mdgat_attention_f64', counts, B, x.device)
        _lib.check(getattr(_lib.load(), name)(B, N, M, *lead, int(bool(cross)), int(topk), x.data_ptr(), msg.data_ptr(),
                                              sel.data_ptr() if sel is not None else None, _stream(x)), name)
    return msg, sel


def attention_f64_backward(qkv: torch.Tensor, N: int, M: int, cross: bool, dmsg: torch.Tensor, topk: int = 0, selection=None) -> torch.Tensor:
    """Gradient of ``attention_f64`` (csrc/attention_grad.hip): the forward's qkv [B, N+M, 3, 4, 32], dmsg = dL/dmessage [B, N+M, 128]
    (any dtype and strides) and, for a dynamic layer (``topk`` > 0), ``selection`` - the forward's raw int32 selection words
    (``mdgat_taps.topk_sel`` layout, what ``topk_sel_to_masks`` decodes) -> dqkv [B, N+M, 3, 4, 32] float64.  The top-k selection is not
    differentiated and not decided again: keys the forward did not keep get exactly 0.0 in dk / dv.  No value atomics: the same bits
    from run to run, and a pair's dqkv does not depend on its batch.  N, M <= 2048."""
    _need_cuda(qkv, dmsg)
    x = qkv.detach().to(torch.float64).contiguous()
    B, P = x.shape[0], x.shape[1]
    if P != N + M or tuple(x.shape[2:]) != (3, 4, 32):
        raise ValueError(f'qkv must be [B, {N + M}, 3, 4, 32], got {tuple(qkv.shape)}')
    if tuple(dmsg.shape) != (B, P, 128):
        raise ValueError(f'dmsg {tuple(dmsg.shape)} does not fit qkv: expected [{B}, {P}, 128]')
    if dmsg.device != x.device:
        raise ValueError(f'dmsg is on {dmsg.device}, qkv on {x.device}')
    topk = int(topk)
    sel = None
    if topk > 0:
        if selection is None:
            raise ValueError(f'topk={topk}: the backward of a dynamic layer needs the forward\'s selection words (selection=)')
        _need_cuda(selection)
        sel = selection.to(device=x.device, dtype=torch.int32).contiguous()
        if sel.numel() != topk_sel_words(B, N, M):
            raise ValueError(f'selection holds {sel.numel()} words, the forward writes {topk_sel_words(B, N, M)}')
    g = dmsg.detach().to(torch.float64).contiguous()
    dqkv = torch.empty_like(x)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        ws, base, need = _workspace(lib.mdgat_attention_backward_workspace_bytes(B, N, M), x.device)
        _lib.check(lib.mdgat_attention_backward_f64(B, N, M, int(bool(cross)), topk, x.data_ptr(), sel.data_ptr() if sel is not None else None,
                                                    g.data_ptr(), dqkv.data_ptr(), base, need, _stream(x)),
                   'mdgat_attention_backward_f64')
    return dqkv


class _AttentionF64(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, N, M, cross, topk, want_sel):
        msg, sel = _attention_f64_values(qkv, N, M, cross, topk, want_sel)
        ctx.save_for_backward(qkv, *((sel,) if topk > 0 else ()))
        ctx.shape = (N, M, cross, topk)
        if sel is None:
            return msg
        ctx.mark_non_differentiable(sel)
        return msg, sel

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dmsg, *_):
        qkv, *sel = ctx.saved_tensors
        N, M, cross, topk = ctx.shape
        dqkv = attention_f64_backward(qkv, N, M, cross, dmsg, topk, sel[0] if sel else None)
        return dqkv.to(qkv.dtype), None, None, None, None, None


def attention_f64(qkv: torch.Tensor, N: int, M: int, cross: bool, topk: int = 0, return_selection: bool = False, counts=None):
    """attention / dynamic_attention (mdgat.py:190-210) in fp64.  qkv [B, N+M, 3, 4, 32] float64 -> message [B, N+M, 128] float64
    (with ``return_selection``: also the masks of the keys a dynamic layer kept, see topk_sel_to_masks; full attention keeps every key of
    a pair: all True within its counts).

    Differentiable with respect to qkv (``attention_f64_backward``; not twice): when qkv requires grad and grad is enabled the message
    carries a grad_fn.  The launch and the values are the same either way; a dynamic layer then always asks for the selection words
    and saves them for the backward (16 MB at 64 pairs of 512), which reads them instead of selecting again.  The masks are not
    differentiable.

    ``counts`` (a ``pack_ragged`` dict or ``(counts0, counts1)``): a ragged batch - pair b has ``counts0[b]`` / ``counts1[b]`` keypoints in
    slots padded to N / M (frame 1 from row N on).  Its rows are those of the pair run alone (bit for bit where both launches run the same
    kernel form, the kept keys always); message rows and masks beyond its counts are zero / False.  The forward only."""
    B = qkv.shape[0]
    topk = int(topk)
    if counts is not None:
        if qkv.requires_grad and torch.is_grad_enabled():
            raise RuntimeError('attention_f64(counts=): ragged batches run the forward only (no gradient)')
        cnt = _ragged_counts(counts, B, qkv.device)
        msg, sel = _attention_f64_values(qkv, N, M, cross, topk, return_selection, cnt)
        return (msg, _selection_masks(sel, B, N, M, cross, topk, cnt, msg.device)) if return_selection else msg
    if torch.is_grad_enabled() and qkv.requires_grad:
        want_sel = topk > 0                           # a dynamic layer always keeps its selection words; full attention writes none
        out = _AttentionF64.apply(qkv, N, M, bool(cross), topk, want_sel)
        msg, sel = out if want_sel else (out, None)
    else:
        msg, sel = _attention_f64_values(qkv, N, M, cross, topk, return_selection)
    if return_selection:
        return msg, _selection_masks(sel, B, N, M, cross, topk, None, msg.device)
    return msg


def mfma_f64_probe(device, reps: int = 2000):
    """Measurement only: (ms, flops, shader ticks) of the v_mfma_f64_16x16x4_f64 probe loop on ``device``."""
    dev = torch.device(device)
    ws = torch.empty(1 << 17, dtype=torch.uint8, device=dev)
    ms, fl, tk = C.c_float(0), C.c_double(0), C.c_longlong(0)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mdgat_mfma_f64_probe(int(reps), ws.data_ptr(), ws.numel(), C.byref(ms), C.byref(fl), C.byref(tk),
                                                    torch.cuda.current_stream(dev).cuda_stream), 'mdgat_mfma_f64_probe')
    return ms.value, fl.value, tk.value


def _loss_args(Z, gt0, gt1, method):
    """What both directions of the loss pass to the library: (method code, Z contiguous in its own precision, N, M, gt0, gt1 int64)."""
    _need_cuda(Z)
    m = _lib.LOSS_METHODS[method] if isinstance(method, str) else int(method)
    z = Z.to(torch.float64 if Z.dtype == torch.float64 else torch.float32).contiguous()
    B, N1, M1 = z.shape
    N, M = N1 - 1, M1 - 1
    if tuple(gt0.shape) != (B, N) or tuple(gt1.shape) != (B, M):
        raise ValueError(f'gt0 {tuple(gt0.shape)} / gt1 {tuple(gt1.shape)} do not fit Z {tuple(z.shape)}: expected [{B}, {N}] / [{B}, {M}]')
    if m != _lib.LOSS_GAP and N != M:
        raise ValueError(f'the {method} loss needs N == M (N={N}, M={M}), as the reference\'s does')
    g0 = gt0.to(device=z.device, dtype=torch.int64).contiguous()
    g1 = gt1.to(device=z.device, dtype=torch.int64).contiguous()
    return m, z, N, M, g0, g1


def _matching_loss_values(Z, gt0, gt1, method, gamma):
    m, z, N, M, g0, g1 = _loss_args(Z, gt0, gt1, method)
    B, f64 = z.shape[0], z.dtype == torch.float64
    loss = torch.empty(B, dtype=torch.float64, device=z.device)
    bad = torch.zeros(1, dtype=torch.int32, device=z.device)
    lib = _lib.load()
    with torch.cuda.device(z.device):
        ws, base, need = _workspace(lib.mdgat_loss_workspace_bytes(B, N, M), z.device)
        fn = lib.mdgat_loss_f64 if f64 else lib.mdgat_loss
        _lib.check(fn(B, N, M, z.data_ptr(), g0.data_ptr(), g1.data_ptr(), m, float(gamma), loss.data_ptr(), bad.data_ptr(),
                      base, need, _stream(z)), 'mdgat_loss_f64' if f64 else 'mdgat_loss')
    if int(bad.item()):
        raise IndexError(f'gt_matches hold an index outside [-1, {M}] (gt0) or [-1, {N}] (gt1)')
    return loss


def matching_loss_backward(Z: torch.Tensor, gt0: torch.Tensor, gt1: torch.Tensor, method, gamma: float, dloss: torch.Tensor) -> torch.Tensor:
    """Gradient of ``matching_loss`` with respect to Z (csrc/loss_grad.hip): Z [B, N+1, M+1] (float32 or float64), the gts and method
    of the forward, and dloss [B] (any dtype and strides), one upstream weight per pair -> dZ [B, N+1, M+1] in Z's dtype, computed in
    fp64: what autograd takes through the reference's loss code (mdgat.py:486-594), with its conventions - a clamp argument that is
    exactly 0 passes the gradient, -log(exp(z)) is differentiated literally (non-finite where exp(z) underflows), ties between a
    row's / column's largest non-positive entries (triplet) take the lowest index.  A pair's dZ is bitwise the same in any batch.
    Synchronises: a gt index outside [-1, M] / [-1, N] raises IndexError."""
    m, z, N, M, g0, g1 = _loss_args(Z, gt0, gt1, method)
    B, f64 = z.shape[0], z.dtype == torch.float64
    if dloss.device != z.device:
        raise ValueError(f'dloss is on {dloss.device}, Z on {z.device}')
    if tuple(dloss.shape) != (B,):
        raise ValueError(f'dloss {tuple(dloss.shape)} does not fit Z {tuple(z.shape)}: expected [{B}]')
    g = dloss.to(torch.float64).contiguous()
    dZ = torch.empty(z.shape, dtype=torch.float64, device=z.device)
    bad = torch.zeros(1, dtype=torch.int32, device=z.device)
    lib = _lib.load()
    with torch.cuda.device(z.device):
        ws, base, need = _workspace(lib.mdgat_loss_backward_workspace_bytes(B, N, M), z.device)
        fn = lib.mdgat_loss_backward_f64 if f64 else lib.mdgat_loss_backward
        _lib.check(fn(B, N, M, z.data_ptr(), g0.data_ptr(), g1.data_ptr(), m, float(gamma), g.data_ptr(), dZ.data_ptr(), bad.data_ptr(),
                      base, need, _stream(z)), 'mdgat_loss_backward_f64' if f64 else 'mdgat_loss_backward')
    if int(bad.item()):
        raise IndexError(f'gt_matches hold an index outside [-1, {M}] (gt0) or [-1, {N}] (gt1)')
    return dZ.to(Z.dtype)


class _MatchingLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Z, gt0, gt1, method, gamma):
        loss = _matching_loss_values(Z, gt0, gt1, method, gamma)
        ctx.save_for_backward(Z, gt0, gt1)
        ctx.method, ctx.gamma = method, gamma
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dloss):
        Z, gt0, gt1 = ctx.saved_tensors
        return matching_loss_backward(Z, gt0, gt1, ctx.method, ctx.gamma, dloss), None, None, None, None


def matching_loss(Z: torch.Tensor, gt0: torch.Tensor, gt1: torch.Tensor, method='triplet_loss', gamma: float = 0.5) -> torch.Tensor:
    """The evaluation loss of MDGAT.forward (mdgat.py:486-594; csrc/loss.hip) on Z [B, N+1, M+1] (float32 or float64; the arithmetic is
    fp64 either way) and ground-truth matches gt0 [B, N] / gt1 [B, M] (any integer dtype, -1 = unmatched; not rewritten).  ``method``:
    ``'superglue'``, ``'triplet_loss'`` or ``'gap_loss'`` (config['loss_method']); ``gamma``: config['triplet_loss_gamma'].  Returns
    the per-pair values [B] float64 - superglue / triplet: the pair's ratio / mean (the module's loss is their mean), gap: the pair's
    loss.  Synchronises: a gt index outside [-1, M] / [-1, N] raises IndexError, as indexing does in the reference.

    Differentiable with respect to Z (``matching_loss_backward``; not twice): when Z requires grad and grad is enabled the result
    carries a grad_fn, so ``matching_loss(log_optimal_transport(scores, bin_score, T), gt0, gt1, method).mean().backward()`` fills
    ``scores.grad`` and ``bin_score.grad``.  The values, and without grad the kernels launched, are the same either way."""
    if torch.is_grad_enabled() and isinstance(Z, torch.Tensor) and Z.requires_grad:
        return _MatchingLoss.apply(Z, gt0, gt1, method, float(gamma))
    return _matching_loss_values(Z, gt0, gt1, method, gamma)


# ---- the matching head (mdgat.py:397 final_proj, 430-431 the score matrix; csrc/head_grad.hip) ----
def _head_args(desc0, desc1, weight, bias):
    """What both directions of the matching head pass to the library: (desc0, desc1, W [128, 128], b as contiguous float64, B, N, M)."""
    _need_cuda(desc0, desc1, weight, bias)
    if desc0.dim() != 3 or desc1.dim() != 3 or desc0.shape[2] != 128 or desc1.shape[2] != 128 or desc0.shape[0] != desc1.shape[0]:
        raise ValueError(f'desc0 / desc1 must be [B, N, 128] / [B, M, 128], got {tuple(desc0.shape)} / {tuple(desc1.shape)}')
    if tuple(weight.shape) not in ((128, 128), (128, 128, 1)):
        raise ValueError(f'weight must be [128, 128] or the Conv1d\'s [128, 128, 1], got {tuple(weight.shape)}')
    if tuple(bias.shape) != (128,):
        raise ValueError(f'bias must be [128], got {tuple(bias.shape)}')
    for t in (desc0, desc1, weight, bias):
        if t.dtype not in (torch.float32, torch.float64):
            raise TypeError(f'the matching head takes float32 or float64 tensors, got {t.dtype}')
        if t.device != desc0.device:
            raise ValueError(f'the matching head\'s tensors are on {t.device} and {desc0.device}')
    f = lambda t: t.detach().to(torch.float64).contiguous()       # noqa: E731
    return f(desc0), f(desc1), f(weight).reshape(128, 128), f(bias), desc0.shape[0], desc0.shape[1], desc1.shape[1]


def _head_workspace(lib, B, N, M, device):
    return _workspace(lib.mdgat_match_head_workspace_bytes(B, N, M), device)


def _match_head_values(desc0, desc1, weight, bias):
    d0, d1, w, b, B, N, M = _head_args(desc0, desc1, weight, bias)
    scores = torch.empty((B, N, M), dtype=torch.float64, device=d0.device)
    lib = _lib.load()
    with torch.cuda.device(d0.device):
        ws, base, need = _head_workspace(lib, B, N, M, d0.device)
        _lib.check(lib.mdgat_match_head_f64(B, N, M, d0.data_ptr(), d1.data_ptr(), w.data_ptr(), b.data_ptr(), scores.data_ptr(), base, need,
                                            _stream(d0)), 'mdgat_match_head_f64')
    return scores.to(desc0.dtype)


def match_head_backward(desc0: torch.Tensor, desc1: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, dscores: torch.Tensor,
                        need=(True, True, True, True)):
    """Gradient of ``match_head`` (csrc/head_grad.hip): the forward's inputs and dscores = dL/dscores [B, N, M] (any dtype and strides)
    -> (ddesc0 [B, N, 128], ddesc1 [B, M, 128], dweight, dbias), each in the dtype (and, the weight, the shape) of its input, computed
    in fp64.  dweight / dbias are the sums over every point of every pair and both frames, added in a fixed order: the same bits from
    run to run, and ddesc of a pair does not depend on its batch.  ``need``: which of the four to compute (None for the others)."""
    d0, d1, w, b, B, N, M = _head_args(desc0, desc1, weight, bias)
    if tuple(dscores.shape) != (B, N, M):
        raise ValueError(f'dscores {tuple(dscores.shape)} does not fit the descriptors: expected [{B}, {N}, {M}]')
    if dscores.device != d0.device:
        raise ValueError(f'dscores is on {dscores.device}, the descriptors on {d0.device}')
    g = dscores.detach().to(torch.float64).contiguous()
    shapes = ((B, N, 128), (B, M, 128), (128, 128), (128,))
    # (zeros, not empty: an empty batch launches nothing and its sums are zero)
    out = [(torch.zeros if B == 0 else torch.empty)(s, dtype=torch.float64, device=d0.device) if n else None for s, n in zip(shapes, need)]
    ptr = [o.data_ptr() if o is not None else None for o in out]
    lib = _lib.load()
    with torch.cuda.device(d0.device):
        ws, base, nbytes = _head_workspace(lib, B, N, M, d0.device)
        _lib.check(lib.mdgat_match_head_backward(B, N, M, d0.data_ptr(), d1.data_ptr(), w.data_ptr(), b.data_ptr(), g.data_ptr(), ptr[0], ptr[1],
                                                 ptr[2], ptr[3], base, nbytes, _stream(d0)), 'mdgat_match_head_backward')
    like = (desc0, desc1, weight, bias)
    return tuple(o.to(t.dtype).reshape(t.shape) if o is not None else None for o, t in zip(out, like))


class _MatchHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, desc0, desc1, weight, bias):
        scores = _match_head_values(desc0, desc1, weight, bias)
        ctx.save_for_backward(desc0, desc1, weight, bias)
        return scores

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dscores):
        return match_head_backward(*ctx.saved_tensors, dscores, need=tuple(ctx.needs_input_grad))


def match_head(desc0: torch.Tensor, desc1: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """The matching head of MDGAT.forward (mdgat.py:397, 430-431): desc0 [B, N, 128], desc1 [B, M, 128] - the GNN's output descriptors,
    point-major (the reference's [B, 128, N] transposed) - ``final_proj``'s weight ([128, 128] or the Conv1d's [128, 128, 1]) and bias
    [128] -> scores [B, N, M] = final_proj(desc0)^T final_proj(desc1) / sqrt(128), in desc0's dtype.  The arithmetic is fp64 for
    float32 and float64 tensors alike, by the launches of the exact mode's forward.  N, M <= 2175.

    Differentiable with respect to all four (``match_head_backward``; not twice): when one of them requires grad and grad is enabled
    the result carries a grad_fn, so ``matching_loss(log_optimal_transport(match_head(desc0, desc1, W, b), bin_score, T), gt0, gt1,
    method).mean().backward()`` fills ``desc0.grad``, ``desc1.grad``, ``W.grad``, ``b.grad`` and ``bin_score.grad``.  The values, and
    without grad the kernels launched, are the same either way."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (desc0, desc1, weight, bias)):
        return _MatchHead.apply(desc0, desc1, weight, bias)
    return _match_head_values(desc0, desc1, weight, bias)


# ---- the reference's MLP in training mode (mdgat.py:34-46: Conv1d(k=1), BatchNorm1d on batch statistics, ReLU; csrc/mlp_grad.hip) ----
class MlpSaved:
    """What ``mlp_f64_forward`` keeps for ``mlp_f64_backward`` beside the inputs: the pre-BN output of every BN layer and mean /
    invstd per channel, in one device buffer laid out by the library."""
    __slots__ = ('buffer', 'base', 'nbytes', 'training', 'rows')

    def __init__(self, buffer, base, nbytes, training, rows):
        self.buffer, self.base, self.nbytes, self.training, self.rows = buffer, base, nbytes, training, rows


def _mlp_modules(seq):
    """(convs, bns) of an nn.Sequential laid out as the reference's MLP lays it out, or of a bare nn.Conv1d."""
    nn = torch.nn
    if isinstance(seq, nn.Conv1d):
        mods = [seq]
    elif isinstance(seq, nn.Sequential):
        mods = list(seq.children())
    else:
        raise ValueError(f'mlp_f64 takes an nn.Sequential laid out as the reference\'s MLP or an nn.Conv1d, got {type(seq).__name__}')
    if not mods or (len(mods) - 1) % 3:
        raise ValueError(f'mlp_f64: {len(mods)} modules are not Conv1d (BatchNorm1d ReLU Conv1d)*')
    convs, bns = mods[0::3], mods[1::3]
    if len(convs) > _lib.MLP_MAX_CONVS:
        raise ValueError(f'mlp_f64: {len(convs)} convolutions, at most {_lib.MLP_MAX_CONVS} are supported')
    for i, m in enumerate(mods):
        want = (nn.Conv1d, nn.BatchNorm1d, nn.ReLU)[i % 3]
        if not isinstance(m, want):
            raise ValueError(f'mlp_f64: module {i} is {type(m).__name__}, the reference\'s MLP has {want.__name__} there')
    for c in convs:
        if c.kernel_size != (1,) or c.stride != (1,) or c.padding != (0,) or c.dilation != (1,) or c.groups != 1 or c.bias is None:
            raise ValueError(f'mlp_f64: {c} is not a plain Conv1d(kernel_size=1) with bias')
    for b in bns:
        if not b.affine or b.weight is None:
            raise ValueError('mlp_f64: BatchNorm1d without affine parameters is not supported')
        if not b.track_running_stats or b.running_mean is None or b.running_var is None:
            raise ValueError('mlp_f64: BatchNorm1d without running statistics is not supported')
        if b.momentum is None:
            raise ValueError('mlp_f64: BatchNorm1d(momentum=None) (cumulative average) is not supported')
    for a, b in zip(convs[:-1], bns):
        if b.num_features != a.out_channels:
            raise ValueError(f'mlp_f64: {b} does not fit {a}')
    for a, b in zip(convs[:-1], convs[1:]):
        if b.in_channels != a.out_channels:
            raise ValueError(f'mlp_f64: {b} does not follow {a}')
    for c in convs:
        if c.out_channels % 16 or not 16 <= c.out_channels <= 512:
            raise ValueError(f'mlp_f64: {c.out_channels} output channels: the kernels take multiples of 16 up to 512')
    if not 1 <= convs[0].in_channels <= 512:
        raise ValueError(f'mlp_f64: {convs[0].in_channels} input channels: the kernels take 1 to 512')
    return convs, bns


def _mlp_rows(x, x1, cin):
    """x [..., K0] (and x1 [..., K1]) -> contiguous rows [R, K0], [R, K1] or None, the leading shape."""
    for t in (x,) if x1 is None else (x, x1):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
            raise ValueError('mlp_f64 takes float64 tensors')
    _need_cuda(x, *(() if x1 is None else (x1,)))
    if x.dim() < 1 or (x1 is not None and (x1.shape[:-1] != x.shape[:-1] or x1.device != x.device)):
        raise ValueError(f'mlp_f64: x {tuple(x.shape)} and x1 {None if x1 is None else tuple(x1.shape)} must share their leading shape and device')
    k0, k1 = x.shape[-1], 0 if x1 is None else x1.shape[-1]
    if k0 < 1 or (x1 is not None and k1 < 1) or k0 + k1 != cin:
        raise ValueError(f'mlp_f64: {k0} + {k1} input channels (channel-last), the first convolution takes {cin}')
    r0 = x.detach().reshape(-1, k0).contiguous()
    r1 = None if x1 is None else x1.detach().reshape(-1, k1).contiguous()
    return r0, r1, tuple(x.shape[:-1])


def _mlp_desc(rows, k0, k1, training, ws, bs, gammas, betas, bufs, eps, momentum, device):
    """The library's descriptor and the tensors it points into (to be kept alive as long as it)."""
    d = _lib.MdgatMlpDesc()
    d.n_conv, d.R, d.K0, d.K1, d.training = len(ws), rows, k0, k1, int(training)
    keep = []

    def ptr(t, inplace=False):
        if t.dtype != torch.float64 or t.device != device:
            raise ValueError(f'mlp_f64: parameters and buffers must be float64 on {device}, got {t.dtype} on {t.device}')
        if inplace and not t.is_contiguous():
            raise ValueError('mlp_f64: the running buffers must be contiguous')
        t = t.detach().contiguous()
        keep.append(t)
        return t.data_ptr()
    for l, (w, b) in enumerate(zip(ws, bs)):
        d.C[l], d.W[l], d.bias[l] = w.shape[0], ptr(w), ptr(b)
    for l, (g, be, (rm, rv, nbt)) in enumerate(zip(gammas, betas, bufs)):
        d.gamma[l], d.beta[l], d.running_mean[l], d.running_var[l] = ptr(g), ptr(be), ptr(rm, True), ptr(rv, True)
        if nbt is not None:
            if nbt.dtype != torch.int64 or nbt.device != device:
                raise ValueError('mlp_f64: num_batches_tracked must be int64 on the device')
            d.num_batches_tracked[l] = nbt.data_ptr()
            keep.append(nbt)
        d.eps[l], d.momentum[l] = float(eps[l]), float(momentum[l])
    return d, keep


def _mlp_buffer(lib, desc, part, device):
    return _workspace(lib.mdgat_mlp_workspace_bytes(C.byref(desc), part), device)


def _mlp_split(seq):
    convs, bns = _mlp_modules(seq)
    ws, bs = [c.weight for c in convs], [c.bias for c in convs]
    gammas, betas = [b.weight for b in bns], [b.bias for b in bns]
    bufs = [(b.running_mean, b.running_var, b.num_batches_tracked) for b in bns]
    training = bool(seq.training)
    if training and any(nbt is None for _, _, nbt in bufs):
        raise ValueError('mlp_f64: BatchNorm1d without num_batches_tracked is not supported')
    return ws, bs, gammas, betas, bufs, [b.eps for b in bns], [b.momentum for b in bns], training


def _mlp_forward(x, x1, ws, bs, gammas, betas, bufs, eps, momentum, training, residual=None):
    r0, r1, lead = _mlp_rows(x, x1, ws[0].shape[1])
    rows, cout = r0.shape[0], ws[-1].shape[0]
    if rows == 1 and training and gammas:
        raise ValueError(f'Expected more than 1 value per channel when training, got input size {tuple(x.shape)}')
    res = None
    if residual is not None:
        if not isinstance(residual, torch.Tensor) or residual.dtype != torch.float64 or residual.device != r0.device or \
                tuple(residual.shape) != lead + (cout,):
            raise ValueError(f'mlp_f64: residual must be float64 {lead + (cout,)} on {r0.device}')
        res = residual.detach().reshape(-1, cout).contiguous()
    out = torch.empty((rows, cout), dtype=torch.float64, device=r0.device)
    if rows == 0:
        return out.reshape(*lead, cout), MlpSaved(None, 0, 0, training, 0)
    d, keep = _mlp_desc(rows, r0.shape[1], 0 if r1 is None else r1.shape[1], training, ws, bs, gammas, betas, bufs, eps, momentum, r0.device)
    lib = _lib.load()
    with torch.cuda.device(r0.device):
        buf, base, need = _mlp_buffer(lib, d, 0, r0.device)
        if res is not None:
            _lib.check(lib.mdgat_mlp_forward_residual_f64(C.byref(d), r0.data_ptr(), None if r1 is None else r1.data_ptr(), res.data_ptr(),
                                                          out.data_ptr(), base, need, _stream(r0)), 'mdgat_mlp_forward_residual_f64')
        else:
            _lib.check(lib.mdgat_mlp_forward_f64(C.byref(d), r0.data_ptr(), None if r1 is None else r1.data_ptr(), out.data_ptr(), base, need,
                                                 _stream(r0)), 'mdgat_mlp_forward_f64')
    del keep
    return out.reshape(*lead, cout), MlpSaved(buf, base, need, training, rows)


def _mlp_backward(x, x1, ws, bs, gammas, betas, bufs, eps, momentum, saved, dout, need):
    """need: (dx, dx1, [dW...], [db...], [dgamma...], [dbeta...]) booleans -> the same structure of tensors / None."""
    r0, r1, lead = _mlp_rows(x, x1, ws[0].shape[1])
    rows, cout = r0.shape[0], ws[-1].shape[0]
    if not isinstance(saved, MlpSaved) or saved.rows != rows:
        raise ValueError('mlp_f64_backward: `saved` is not what mlp_f64_forward returned for these inputs')
    if not isinstance(dout, torch.Tensor) or dout.dtype != torch.float64 or dout.device != r0.device or tuple(dout.shape) != lead + (cout,):
        raise ValueError(f'mlp_f64_backward: dout must be float64 {lead + (cout,)} on {r0.device}')
    g = dout.detach().reshape(-1, cout).contiguous()
    new = (torch.zeros if rows == 0 else torch.empty)        # (an empty batch launches nothing and its sums are zero)
    mk = lambda want, like: new(like.shape, dtype=torch.float64, device=r0.device) if want else None      # noqa: E731
    dx = mk(need[0], r0)
    dx1 = mk(need[1] and r1 is not None, r1 if r1 is not None else r0)
    dW, db = [mk(n, w) for n, w in zip(need[2], ws)], [mk(n, b) for n, b in zip(need[3], bs)]
    dga, dbe = [mk(n, t) for n, t in zip(need[4], gammas)], [mk(n, t) for n, t in zip(need[5], betas)]
    if rows > 0 and any(t is not None for t in [dx, dx1, *dW, *db, *dga, *dbe]):
        d, keep = _mlp_desc(rows, r0.shape[1], 0 if r1 is None else r1.shape[1], saved.training, ws, bs, gammas, betas, bufs, eps, momentum,
                            r0.device)
        gr = _lib.MdgatMlpGrads()
        p = lambda t: None if t is None else t.data_ptr()          # noqa: E731
        gr.dx0, gr.dx1 = p(dx), p(dx1)
        for l in range(len(ws)):
            gr.dW[l], gr.dbias[l] = p(dW[l]), p(db[l])
        for l in range(len(gammas)):
            gr.dgamma[l], gr.dbeta[l] = p(dga[l]), p(dbe[l])
        lib = _lib.load()
        with torch.cuda.device(r0.device):
            buf, base, nbytes = _mlp_buffer(lib, d, 1, r0.device)
            _lib.check(lib.mdgat_mlp_backward_f64(C.byref(d), r0.data_ptr(), None if r1 is None else r1.data_ptr(), saved.base, saved.nbytes, g.data_ptr(),
                                                  C.byref(gr), base, nbytes, _stream(r0)), 'mdgat_mlp_backward_f64')
        del keep
    dx = None if dx is None else dx.reshape(x.shape)
    dx1 = None if dx1 is None else dx1.reshape(x1.shape)
    return dx, dx1, dW, db, dga, dbe


def mlp_f64_forward(seq, x: torch.Tensor, x1: torch.Tensor = None):
    """``mlp_f64`` without autograd: (out, saved), ``saved`` (``MlpSaved``) being what ``mlp_f64_backward`` needs beside the inputs.
    In training mode the BatchNorm buffers of ``seq`` move, exactly once per call."""
    return _mlp_forward(x, x1, *_mlp_split(seq))


def mlp_f64_backward(seq, x: torch.Tensor, x1, saved: MlpSaved, dout: torch.Tensor, need=None):
    """Gradient of ``mlp_f64`` (csrc/mlp_grad.hip): the forward's modules, inputs and ``saved``, and dout = dL/dout [..., C_L] ->
    (dx, dx1, [dW per convolution], [dbias ...], [dgamma per BatchNorm], [dbeta ...]), float64, each in the shape of its tensor (the
    weights [C_out, C_in, 1]).  ``need``: the same structure of booleans - which to compute (None for the others; default: all, dx1
    only with an x1); a product that only an unwanted gradient needs is not formed.  The sums over the rows are added in a fixed
    order: the same bits from run to run.  ``seq``'s parameters must be the forward's; its buffers are not touched."""
    ws, bs, gammas, betas, bufs, eps, momentum, _ = _mlp_split(seq)
    if need is None:
        need = (True, x1 is not None, [True] * len(ws), [True] * len(ws), [True] * len(gammas), [True] * len(gammas))
    return _mlp_backward(x, x1, ws, bs, gammas, betas, bufs, eps, momentum, saved, dout, need)


class _MlpF64(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, x, x1, *params):
        n, nb, bufs, eps, momentum, training = meta
        ws, bs, gammas, betas = params[:n], params[n:2 * n], params[2 * n:2 * n + nb], params[2 * n + nb:]
        out, saved = _mlp_forward(x, x1, ws, bs, gammas, betas, bufs, eps, momentum, training)
        ctx.meta, ctx.saved = meta, saved
        ctx.save_for_backward(x, x1, *params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        n, nb, bufs, eps, momentum, _ = ctx.meta
        x, x1, *params = ctx.saved_tensors
        ws, bs, gammas, betas = params[:n], params[n:2 * n], params[2 * n:2 * n + nb], params[2 * n + nb:]
        want = ctx.needs_input_grad[1:]
        need = (want[0], want[1], want[2:2 + n], want[2 + n:2 + 2 * n], want[2 + 2 * n:2 + 2 * n + nb], want[2 + 2 * n + nb:])
        dx, dx1, dW, db, dga, dbe = _mlp_backward(x, x1, ws, bs, gammas, betas, bufs, eps, momentum, ctx.saved, dout, need)
        return (None, dx, dx1, *dW, *db, *dga, *dbe)


def mlp_f64(seq, x: torch.Tensor, x1: torch.Tensor = None) -> torch.Tensor:
    """The reference's ``MLP`` (mdgat.py:34-46) in fp64 with BatchNorm as ``seq.training`` says - in training mode on the statistics of
    this call's own rows, the gradient running through them (csrc/mlp_grad.hip).  ``seq``: an ``nn.Sequential`` laid out as the
    reference lays it out - Conv1d(k=1), then BatchNorm1d and ReLU between convolutions - this package's encoder / layer modules, the
    reference's own, or a bare ``nn.Conv1d``; 1 to 4 convolutions, output widths multiples of 16 up to 512, up to 512 inputs.
    ``x`` [..., K0] channel-last float64 on the device (the reference's [B, K0, P] transposed); ``x1`` [..., K1] an optional second
    source read beside it (the layer's ``cat([x, message])`` without the copy).  Returns [..., C_L].

    Parameters and buffers are read from the modules.  In training mode ``running_mean``, ``running_var`` and ``num_batches_tracked``
    are updated in place as torch updates them; in eval mode they are read and left alone.  More than one row is needed in training
    mode (ValueError, as in torch).

    Differentiable (``mlp_f64_backward``; not twice) when x, x1 or a parameter requires grad and grad is enabled: ``.backward()`` fills
    ``x.grad``, ``x1.grad`` and the ``.grad`` of the modules' own parameters; a gradient nobody asked for is not computed.  Between
    forward and backward only the inputs, the pre-BN output of every BN layer and mean / invstd per channel are kept."""
    ws, bs, gammas, betas, bufs, eps, momentum, training = _mlp_split(seq)
    params = (*ws, *bs, *gammas, *betas)
    tensors = (x, *params) if x1 is None else (x, x1, *params)
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors):
        return _MlpF64.apply((len(ws), len(gammas), bufs, eps, momentum, training), x, x1, *params)
    return _mlp_forward(x, x1, ws, bs, gammas, betas, bufs, eps, momentum, training)[0]


class _MlpTensorsF64(torch.autograd.Function):
    """``_MlpF64`` with a residual operand: out = mlp(x | x1) + residual; dout reaches the residual unchanged."""

    @staticmethod
    def forward(ctx, meta, x, x1, residual, *params):
        n, nb, bufs, eps, momentum, training = meta
        ws, bs, gammas, betas = params[:n], params[n:2 * n], params[2 * n:2 * n + nb], params[2 * n + nb:]
        out, saved = _mlp_forward(x, x1, ws, bs, gammas, betas, bufs, eps, momentum, training, residual)
        ctx.meta, ctx.saved = meta, saved
        ctx.save_for_backward(x, x1, *params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        n, nb, bufs, eps, momentum, _ = ctx.meta
        x, x1, *params = ctx.saved_tensors
        ws, bs, gammas, betas = params[:n], params[n:2 * n], params[2 * n:2 * n + nb], params[2 * n + nb:]
        want = ctx.needs_input_grad
        p = want[4:]
        need = (want[1], want[2], p[:n], p[n:2 * n], p[2 * n:2 * n + nb], p[2 * n + nb:])
        dx, dx1, dW, db, dga, dbe = _mlp_backward(x, x1, ws, bs, gammas, betas, bufs, eps, momentum, ctx.saved, dout, need)
        return (None, dx, dx1, dout if want[3] else None, *dW, *db, *dga, *dbe)


def mlp_f64_tensors(x: torch.Tensor, weights, biases, bns=(), training: bool = True, x1: torch.Tensor = None,
                    residual: torch.Tensor = None) -> torch.Tensor:
    """``mlp_f64`` on weight TENSORS instead of modules, with an optional residual: the entry of a caller whose weights are computed
    (rows or columns of a module's weight gathered into another channel order, several convolutions' weights stacked into one product)
    and must stay in the autograd graph.  ``weights`` [C_l, C_in] or [C_l, C_in, 1] and ``biases`` [C_l], float64 on the device, one per
    convolution; ``bns``: the ``nn.BatchNorm1d`` between them (one fewer; gamma, beta and the buffers are read from the modules, the
    buffers move when ``training``).  ``residual`` [..., C_L] is added to the output in the last product's epilogue - out = mlp(x | x1) +
    residual, the layer's ``desc + delta`` (mdgat.py:274) and the encoders' ``denc(...) + kenc(...)`` (392-393) - and receives dout
    unchanged in the backward.  Everything else is ``mlp_f64``: the same launches, the same bits, the same limits."""
    ws, bs, bns = list(weights), list(biases), list(bns)
    if not ws or len(bs) != len(ws) or len(bns) != len(ws) - 1 or len(ws) > _lib.MLP_MAX_CONVS:
        raise ValueError(f'mlp_f64_tensors: {len(ws)} weights, {len(bs)} biases, {len(bns)} BatchNorm1d: expected 1 to {_lib.MLP_MAX_CONVS} '
                         'convolutions with one BatchNorm1d between each two')
    for w, b in zip(ws, bs):
        if not isinstance(w, torch.Tensor) or w.dim() not in (2, 3) or (w.dim() == 3 and w.shape[2] != 1) or tuple(b.shape) != (w.shape[0],):
            raise ValueError('mlp_f64_tensors: weights are [C_out, C_in] or [C_out, C_in, 1], biases [C_out]')
        if w.shape[0] % 16 or not 16 <= w.shape[0] <= 512:
            raise ValueError(f'mlp_f64: {w.shape[0]} output channels: the kernels take multiples of 16 up to 512')
    for a, b in zip(ws[:-1], ws[1:]):
        if b.shape[1] != a.shape[0]:
            raise ValueError(f'mlp_f64_tensors: a weight {tuple(b.shape)} does not follow {tuple(a.shape)}')
    for w, b in zip(ws[:-1], bns):
        if not isinstance(b, torch.nn.BatchNorm1d) or b.num_features != w.shape[0] or not b.affine or not b.track_running_stats or \
                b.momentum is None or b.running_mean is None or (training and b.num_batches_tracked is None):
            raise ValueError('mlp_f64_tensors: a BatchNorm1d with affine parameters, running statistics and a momentum is expected '
                             'behind every convolution but the last')
    if not 1 <= ws[0].shape[1] <= 512:
        raise ValueError(f'mlp_f64: {ws[0].shape[1]} input channels: the kernels take 1 to 512')
    gammas, betas = [b.weight for b in bns], [b.bias for b in bns]
    bufs = [(b.running_mean, b.running_var, b.num_batches_tracked) for b in bns]
    eps, momentum, training = [b.eps for b in bns], [b.momentum for b in bns], bool(training)
    params = (*ws, *bs, *gammas, *betas)
    tensors = [t for t in (x, x1, residual, *params) if isinstance(t, torch.Tensor)]
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        return _MlpTensorsF64.apply((len(ws), len(gammas), bufs, eps, momentum, training), x, x1, residual, *params)
    return _mlp_forward(x, x1, ws, bs, gammas, betas, bufs, eps, momentum, training, residual)[0]


# ---- the frame maximum of the pooled descriptor encoder ('FPFH_gloabal', mdgat.py:168: torch.max(desc, dim=2); csrc/pool_f64.hip) ----
def _frame_max_values(e):
    if not isinstance(e, torch.Tensor) or e.dtype != torch.float64 or e.dim() != 3 or e.shape[2] != 128:
        raise ValueError('frame_max_f64 takes a float64 tensor [B, n, 128] (channel-last)')
    _need_cuda(e)
    B, n = e.shape[0], e.shape[1]
    if n < 1:
        raise ValueError('frame_max_f64: a frame without keypoints has no maximum')
    x = e.detach().contiguous()
    g = torch.empty((B, 128), dtype=torch.float64, device=e.device)
    idx = torch.empty((B, 128), dtype=torch.int64, device=e.device)
    with torch.cuda.device(e.device):
        _lib.check(_lib.load().mdgat_frame_max_f64(B, n, x.data_ptr(), g.data_ptr(), idx.data_ptr(), _stream(x)), 'mdgat_frame_max_f64')
    return g, idx


def frame_max_backward(dg: torch.Tensor, idx: torch.Tensor, n: int) -> torch.Tensor:
    """Gradient of ``frame_max_f64``: dg [B, 128] float64 and the forward's ``idx`` [B, 128] int64 -> de [B, n, 128], dg at row idx and
    zero elsewhere.  The indices are the forward's, never decided again; one writer per element, no atomics."""
    if dg.dtype != torch.float64 or idx.dtype != torch.int64 or dg.dim() != 2 or dg.shape[1] != 128 or tuple(idx.shape) != tuple(dg.shape) or \
            idx.device != dg.device or n < 1:
        raise ValueError('frame_max_backward: dg float64 [B, 128], idx int64 [B, 128] on one device, n >= 1')
    _need_cuda(dg)
    B = dg.shape[0]
    dg, idx = dg.detach().contiguous(), idx.contiguous()
    de = torch.empty((B, n, 128), dtype=torch.float64, device=dg.device)
    with torch.cuda.device(dg.device):
        _lib.check(_lib.load().mdgat_frame_max_backward_f64(B, n, dg.data_ptr(), idx.data_ptr(), de.data_ptr(), _stream(dg)),
                   'mdgat_frame_max_backward_f64')
    return de


class _FrameMaxF64(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e):
        g, idx = _frame_max_values(e)
        ctx.n = e.shape[1]
        ctx.save_for_backward(idx)
        ctx.mark_non_differentiable(idx)
        return g, idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dg, _):
        (idx,) = ctx.saved_tensors
        return frame_max_backward(dg, idx, ctx.n)


def frame_max_f64(e: torch.Tensor):
    """``torch.max(e, dim=1)`` for e [B, n, 128] float64 on the device, channel-last: (g [B, 128], idx [B, 128] int64), g the maximum of
    every channel over the frame's n keypoints and idx the FIRST row that holds it - the pooling of the reference's
    ``DescriptorGloabalEncoder`` (mdgat.py:168).  Differentiable (not twice) when e requires grad: the backward sends dg to row idx and
    zero to every other row, with the indices the forward saved."""
    if torch.is_grad_enabled() and isinstance(e, torch.Tensor) and e.requires_grad:
        return _FrameMaxF64.apply(e)
    return _frame_max_values(e)
