"""Drop-in ``MDGAT`` module and ``match()`` API over the gfx950 HIP library.

Host-side mirror of ``/root/reference/models/mdgat.py:315-603`` (class ``MDGAT``) for the FPFH descriptors - ``'FPFH'``,
``'FPFH_gloabal'`` (the descriptor encoder pooled over the frame, mdgat.py:156-174: its encoders run on the fp64 products on every path)
and ``'FPFH_only'`` (no keypoint encoder: keypoints give the shapes only, the saliency is not read) - on the inference path:

* same constructor config dict (``test.py:137-151``), same parameter and buffer names and shapes, so
  ``load_state_dict(checkpoint['net'])`` works (also through ``torch.nn.DataParallel``, whose keys carry a
  ``module.`` prefix - ``test.py:158-159``);
* same ``forward(data: dict) -> dict`` contract: keys ``keypoints0/1, descriptors0/1, scores0/1`` in,
  ``matches0/1`` (int64, -1 = unmatched), ``matching_scores0/1`` (module dtype) and ``loss`` out, the
  empty-keypoint early-out of ``mdgat.py:374-382`` included;
* the module's dtype is the arithmetic request, as it is in the reference: ``net.double()`` (what ``test.py:193`` and
  ``test_registration_metric.py:194`` call before every forward) runs the library's reference-exact mode - fp64 inputs,
  fp64 weights and fp64 matrix-core arithmetic, so that every ``logits.topk(k)`` (``mdgat.py:202``) selects what the
  reference's fp64 run selects (``include/mdgat_hip.h``: ``MDGAT_ARITH_FP64``) and an fp64 Sinkhorn whose arg-maxes
  are the reference's (``config['sinkhorn_arithmetic']``) at every frame size the library takes; a float32 module runs the fp32-class throughput path (5x the rate, Z within
  1e-4 except around the ~1.5 keypoints per pair whose top-k near-tie falls the other way).  ``config['arithmetic']`` =
  ``'fp32'`` / ``'fp64'`` (not a reference key) or ``MDGAT_ARITHMETIC`` in the environment pin one path whatever the dtype;
  results are cast to the module's dtype either way.

All arithmetic happens in ``libmdgat_hip.so``; PyTorch only owns device memory and streams.  There is no
CPU path: tensors that are not on a gfx950 device raise.  Training: ``training_forward`` (``train.py``) is the differentiable fp64
forward; ``forward`` in ``train()`` mode returns it with ``config['train_forward']`` (or ``MDGAT_TRAIN_FORWARD=1``) and raises
otherwise.  The loss VALUE is what the reference's validation loop reads (``train.py:263-299``): with ``config['eval_loss']``
(or ``MDGAT_EVAL_LOSS=1``) ``forward`` computes it on the device (``csrc/loss.hip``); otherwise ``loss`` is a zero scalar.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import weakref
from collections import namedtuple
from typing import Dict, Optional

import torch
from torch import nn

from . import _lib, ops, pack

_D = 128
DESCRIPTORS = ('FPFH', 'FPFH_gloabal', 'FPFH_only')


def _mlp_modules(channels):
    """Parameter container with the reference's Sequential indices (conv 3i, BN 3i+1, ReLU 3i+2)."""
    mods = []
    last = len(channels) - 1
    for i in range(1, len(channels)):
        mods.append(nn.Conv1d(channels[i - 1], channels[i], kernel_size=1, bias=True))
        if i < last:
            mods.append(nn.BatchNorm1d(channels[i]))
            mods.append(nn.ReLU())
    return nn.Sequential(*mods)


class _Encoder(nn.Module):
    def __init__(self, cin, hidden, cout):
        super().__init__()
        self.encoder = _mlp_modules([cin, *hidden, cout])
        nn.init.constant_(self.encoder[-1].bias, 0.0)


class _GlobalEncoder(nn.Module):
    """DescriptorGloabalEncoder (mdgat.py:156-174): the FPFH MLP, then a second MLP over [per-keypoint | frame maximum]."""

    def __init__(self, cin, hidden, cout):
        super().__init__()
        self.encoder = _mlp_modules([cin, *hidden, cout])
        nn.init.constant_(self.encoder[-1].bias, 0.0)
        self.encoder2 = _mlp_modules([2 * cout, 2 * cout, cout])
        nn.init.constant_(self.encoder2[-1].bias, 0.0)


class _Attn(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.merge = nn.Conv1d(d, d, kernel_size=1)
        self.proj = nn.ModuleList([nn.Conv1d(d, d, kernel_size=1) for _ in range(3)])


class _Propagation(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.attn = _Attn(d)
        self.mlp = _mlp_modules([2 * d, 2 * d, d])
        nn.init.constant_(self.mlp[-1].bias, 0.0)


class _GNN(nn.Module):
    def __init__(self, d, n_layers):
        super().__init__()
        self.layers = nn.ModuleList([_Propagation(d) for _ in range(n_layers)])


class _DeviceState:
    """Per-device library handle + packed weights + scratch (one per (module, device)).  The scratch is per STREAM: the
    library only enqueues, so forwards issued on two streams run concurrently on the device and must not share it."""

    MAX_WORKSPACES = 8                  # streams remembered per device (least recently used first out)

    def __init__(self, handle, device, f64=False):
        self.handle = handle
        self.device = device
        self.f64 = f64                  # the handle computes in MDGAT_ARITH_FP64 (fixed at mdgat_create)
        self.exact = f64                # ... and runs the exact mode (False with f64: the fp64 encoders of 'FPFH_gloabal' in front of the fp32-class path)
        self.workspaces = {}            # stream handle -> uint8 tensor, in order of last use
        self.lock = threading.Lock()

    def workspace_for(self, stream: int, need: int, dev):
        """Scratch of the forward being enqueued on ``stream``.  Cached per raw stream handle, bounded (PyTorch hands stream
        handles out of a pool: unbounded, the cache would pin ~0.4 GB per handle ever seen).  While a stream is being CAPTURED
        into a graph the scratch is allocated from the graph's private pool and must live exactly as long as the graph: it is
        handed back uncached (the graph keeps its allocation alive), and an eager call on a recycled handle can never be given
        memory a graph still replays into."""
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            return torch.empty(need, dtype=torch.uint8, device=dev)
        ws = self.workspaces.pop(stream, None)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        self.workspaces[stream] = ws    # (most recently used last)
        while len(self.workspaces) > self.MAX_WORKSPACES:
            self.workspaces.pop(next(iter(self.workspaces)))
        return ws

    def close(self):
        self.workspaces.clear()
        if self.handle:
            _lib.load().mdgat_destroy(self.handle)
            self.handle = None


def _sync_raw_stream(handle: int, dev):
    """Synchronise a stream known by its raw handle (the keys of _DeviceState.workspaces)."""
    torch.cuda.ExternalStream(handle, device=dev).synchronize()


def _close_states(states):
    for st in list(states.values()):
        st.close()
    states.clear()


# What a ragged runner prepares for MDGAT._ragged_forward: the device, (B, Np, Mp), the host counts (h0, h1), the library's entry, its
# arguments between the shape and the outputs (lead) and between Z and the workspace (behind_Z), and what the runner wants back - the
# tensors those arguments point into among it.
_RaggedCall = namedtuple('_RaggedCall', 'dev shape counts entry lead behind_Z kept')


class MDGAT(nn.Module):
    default_config = {
        'descriptor_dim': 128,
        'keypoint_encoder': [32, 64, 128],
        'descritor_encoder': [64, 128],
        'GNN_layers': ['self', 'cross'] * 9,
        'sinkhorn_iterations': 100,
        'match_threshold': 0.2,
    }

    def __init__(self, config):
        super().__init__()
        self.config = {**self.default_config, **config}
        # the reference reads these with config[...] and raises KeyError when absent (mdgat.py:329, 353, 362-367)
        self.descriptor = config['descriptor']
        self.lr = config['lr']
        self.loss_method = config['loss_method']
        self.k = config['k']
        self.mutual_check = config['mutual_check']
        self.triplet_loss_gamma = config['triplet_loss_gamma']
        self.train_step = config['train_step']
        L = self.config['L']
        # not a reference key: 'fp32' (default, the parity path) or 'f16' (single-f16 attention products, a throughput
        # mode outside the parity bar - BASELINE.json configs[2]; 'bf16' is accepted as an alias: the operands are f16,
        # same matrix-core rate, three more mantissa bits)
        self.attention_dtype = str(self.config.get('attention_dtype', 'fp32'))
        if self.attention_dtype not in ('fp32', 'f16', 'bf16'):
            raise ValueError(f"attention_dtype={self.attention_dtype!r}: expected 'fp32' or 'f16'")
        # not a reference key either: how the library executes a batch (include/mdgat_hip.h: mdgat_set_lanes).  0 = its default
        # (two lanes: the halves of a batch in flight on two streams); results do not depend on it
        self.lanes = int(self.config.get('lanes', 0))
        if self.lanes not in (0, 1, 2):
            raise ValueError(f'lanes={self.lanes}: expected 1 or 2 (0: library default)')
        # not a reference key: which arithmetic the forward runs in (include/mdgat_hip.h: mdgat_arithmetic).
        #   'auto' (default): the MODULE'S DTYPE decides, as it does in the reference - a float64 module (test.py:193 and
        #            test_registration_metric.py:194 call net.double() before every forward) runs the reference's own
        #            arithmetic for the encoders and the layers up to the last dynamic one, where the top-k selection of
        #            mdgat.py:202 is decided (csrc/f64.hip); a float32 module runs the fp32-class throughput path;
        #   'fp32' / 'fp64': that path whatever the dtype (bench.py pins its headline this way).
        # MDGAT_ARITHMETIC in the environment replaces the default for modules whose config does not carry the key.
        # 'f64_layers' (optional): how many leading layers run in fp64 (None: through the last layer with a k; 0: encoders only).
        self.arithmetic = str(self.config.get('arithmetic') or os.environ.get('MDGAT_ARITHMETIC') or 'auto')
        if self.arithmetic not in ('auto', 'fp32', 'fp64'):
            raise ValueError(f"arithmetic={self.arithmetic!r}: expected 'auto', 'fp32' or 'fp64'")
        # not a reference key: compute the loss of mdgat.py:486-594 in forward (csrc/loss.hip) from data['gt_matches0/1'] - the value
        # the reference's validation loop (train.py:263-299) averages to choose a checkpoint - instead of returning a zero scalar.
        # MDGAT_EVAL_LOSS=1 in the environment replaces the default (off) for modules whose config does not carry the key.
        ev = self.config.get('eval_loss')
        self.eval_loss = bool(ev) if ev is not None else os.environ.get('MDGAT_EVAL_LOSS') == '1'
        # not a reference key: in train() mode forward returns training_forward(data) - the differentiable fp64 step (train.py) - instead of
        # raising.  MDGAT_TRAIN_FORWARD=1 in the environment replaces the default (off) for modules whose config does not carry the key.
        tf = self.config.get('train_forward')
        self.train_forward = bool(tf) if tf is not None else os.environ.get('MDGAT_TRAIN_FORWARD') == '1'
        # not a reference key: which modules forward_ragged / evaluate_ragged take.  'exact' (default): the exact mode only;
        #   'auto': a module whose forward is fp32-class (not exact()) runs the library's fp32-class ragged forward (mdgat_forward_ragged:
        #   slots of at most 512 keypoints), an exact one its own as before;
        #   'module': EVERY ragged entry - forward_ragged / evaluate_ragged and the bank's match_frames_ragged / evaluate_frames_ragged -
        #   runs the arithmetic the module's forward runs, for all three FPFH descriptors: 'auto', plus the bank entries on an fp32-class
        #   module (mdgat_forward_frames_ragged on its handle) and the pooled descriptor ('FPFH_gloabal': its encoders in fp64, the
        #   fp32-class kernels behind them).
        # MDGAT_RAGGED_ARITHMETIC in the environment replaces the default for modules whose config does not carry the key.
        self.ragged_arithmetic = str(self.config.get('ragged_arithmetic') or os.environ.get('MDGAT_RAGGED_ARITHMETIC') or 'exact')
        if self.ragged_arithmetic not in ('exact', 'auto', 'module'):
            raise ValueError(f"ragged_arithmetic={self.ragged_arithmetic!r}: expected 'exact', 'auto' or 'module'")
        # not a reference key: which fp64 Sinkhorn an EXACT module's ragged batches run (include/mdgat_hip.h: mdgat_set_ragged_sinkhorn).
        #   'resident' (default): the register-resident form only - at most 575 keypoints per frame;
        #   'auto': that form, the same bits, in slots within 575; the streaming form with per-pair counts beyond, up to 2048 per frame;
        #   'streaming': always the streaming form, up to 2048.
        # Where the streaming form runs, a pair has the bits of the pair alone under set_f64_sinkhorn_form(1).  A module whose ragged calls
        # run the fp32-class branch (ragged_arithmetic) ignores the key and keeps its limit of 512.
        # MDGAT_RAGGED_SINKHORN in the environment replaces the default for modules whose config does not carry the key.
        self.ragged_sinkhorn = str(self.config.get('ragged_sinkhorn') or os.environ.get('MDGAT_RAGGED_SINKHORN') or 'resident')
        if self.ragged_sinkhorn not in ('resident', 'auto', 'streaming'):
            raise ValueError(f"ragged_sinkhorn={self.ragged_sinkhorn!r}: expected 'resident', 'auto' or 'streaming'")
        # not a reference key: which form of the fp32 Sinkhorn the fp32-class ragged forward runs (ragged_arithmetic 'auto' / 'module' on a
        # module that is not exact(); include/mdgat_hip.h: mdgat_set_ragged_sinkhorn on an MDGAT_ARITH_FP32 handle).
        #   'pair' (default): one workgroup per pair, all iterations in one launch;
        #   'split': a pair's rows over ceil(Np / 128) workgroups, one launch per iteration, in slots of more than 128 rows (smaller slots run
        #   'pair', the same bits).  Z agrees with 'pair' to fp32 rounding, not bit for bit; the limit of 512 and every refusal stay.
        # An exact module ignores the key.  MDGAT_RAGGED_SINKHORN_FP32 in the environment replaces the default for modules whose config does
        # not carry the key.
        self.ragged_sinkhorn_fp32 = str(self.config.get('ragged_sinkhorn_fp32') or os.environ.get('MDGAT_RAGGED_SINKHORN_FP32') or 'pair')
        if self.ragged_sinkhorn_fp32 not in ('pair', 'split'):
            raise ValueError(f"ragged_sinkhorn_fp32={self.ragged_sinkhorn_fp32!r}: expected 'pair' or 'split'")
        # not a reference key: the slots of the fp32-class ragged forward (include/mdgat_hip_wide.h: mdgat_set_ragged_fp32_slots).  'narrow' (the
        # default): frames of at most 512 keypoints, today's kernels and bits.  'wide': up to 2048 - slots within 512 x 512 run what they run
        # under 'narrow', larger ones the ragged forms of the windowed and wide attention kernels and of the streaming Sinkhorn at 16 and 32
        # columns per lane (ragged_sinkhorn_fp32 = 'split': the split form for up to 16 slabs).  An exact module ignores the key.
        # MDGAT_RAGGED_SLOTS_FP32 in the environment replaces the default for modules whose config does not carry the key.
        self.ragged_slots_fp32 = str(self.config.get('ragged_slots_fp32') or os.environ.get('MDGAT_RAGGED_SLOTS_FP32') or 'narrow')
        if self.ragged_slots_fp32 not in ('narrow', 'wide'):
            raise ValueError(f"ragged_slots_fp32={self.ragged_slots_fp32!r}: expected 'narrow' or 'wide'")
        f64_layers =self.config.get('f64_layers')
        self.f64_layers = None if f64_layers is None or int(f64_layers) < 0 else int(f64_layers)
        # 'sinkhorn_arithmetic' (optional; MDGAT_SINKHORN_ARITHMETIC in the environment): the exact mode's TAIL - every layer, final_proj,
        # the score matrix and the optimal transport in fp64, every arg-max of the extraction decided on the fp64 Z (csrc/sinkhorn_f64.hip).
        #   'auto' (default): on for frames of at most 2175 keypoints (beyond 575 the Sinkhorn streams its couplings from memory, one launch
        #   per iteration), else the fp32-class tail behind the last dynamic layer;
        #   'fp64': required (larger frames are refused);  'fp32': the fp32-class tail (Z good to 7e-6: inside the bar of 1e-4, but an
        #   arg-max whose two candidates lie closer than that may fall the other way - one in 40 960 on a reference-held batch).
        self.sinkhorn_arithmetic = str(self.config.get('sinkhorn_arithmetic') or os.environ.get('MDGAT_SINKHORN_ARITHMETIC') or 'auto')
        if self.sinkhorn_arithmetic not in ('auto', 'fp32', 'fp64'):
            raise ValueError(f"sinkhorn_arithmetic={self.sinkhorn_arithmetic!r}: expected 'auto', 'fp32' or 'fp64'")
        if self.arithmetic == 'fp64' and self.attention_dtype != 'fp32':
            raise ValueError("arithmetic='fp64' and attention_dtype='f16' exclude each other")
        if self.descriptor == 'FPFH_gloabal' and self.attention_dtype != 'fp32':
            raise ValueError("descriptor='FPFH_gloabal' (its encoders run in fp64 on every path) and attention_dtype='f16' exclude each other")
        if self.descriptor == 'FPFH_gloabal' and self.ragged_sinkhorn_fp32 == 'split' and self.arithmetic != 'fp64':
            # (a module is float32 as it is made: only arithmetic='fp64' makes it exact here)
            raise NotImplementedError("ragged_sinkhorn_fp32='split' and descriptor='FPFH_gloabal' exclude each other on an fp32-class module: its handle "
                                      "computes the encoders in fp64 (MDGAT_ARITH_FP64), where mdgat_set_ragged_sinkhorn selects the fp64 Sinkhorn")
        if self.descriptor not in DESCRIPTORS:
            raise NotImplementedError(
                f"descriptor={self.descriptor!r}: the FPFH encoders {DESCRIPTORS} are implemented on MI355X "
                "(the pointnet variants are out of scope, see DESIGN.md)")
        d = self.config['descriptor_dim']
        if d != _D or list(self.config['keypoint_encoder']) != [32, 64, 128] or \
                list(self.config['descritor_encoder']) != [64, 128]:
            raise NotImplementedError('the HIP kernels implement the default widths: descriptor_dim=128, '
                                      'keypoint_encoder=[32,64,128], descritor_encoder=[64,128]')
        # mdgat.py:336-350: 'FPFH_only' has no keypoint encoder, 'FPFH_gloabal' pools the descriptor encoder over the frame
        if self.descriptor != 'FPFH_only':
            self.kenc = _Encoder(4, self.config['keypoint_encoder'], d)
        self.denc = (_GlobalEncoder if self.descriptor == 'FPFH_gloabal' else _Encoder)(33, self.config['descritor_encoder'], d)
        self.gnn = _GNN(d, 2 * L)
        self.final_proj = nn.Conv1d(d, d, kernel_size=1, bias=True)
        self.register_parameter('bin_score', nn.Parameter(torch.tensor(1.)))
        # shared (by reference) with DataParallel replicas: device index -> _DeviceState
        self._states: Dict[int, _DeviceState] = {}
        self._states_lock = threading.RLock()
        # Also shared with the replicas (lists, so that a replica's shallow __dict__ copy sees later updates):
        # [0] the packed fp32 host blob of the owner's parameters.  torch.nn.parallel.replicate() strips the parameters
        #     off the replicas (they become plain attributes; state_dict() of a replica holds only buffers), so a
        #     replica cannot pack - the owner packs in _replicate_for_data_parallel(), before the replicas run;
        # [1] True while a blob installed by load_packed() (e.g. received by an RCCL broadcast) stands in for this
        #     module's own parameters: casts / moves of the module must not throw it away.
        self._blob_holder = [None, False]
        self._blob64_holder = [None]        # exact mode: the same blob before its rounding to fp32 (shared like [0] above)
        self._pooled_holder = [None]        # 'FPFH_gloabal': encoder2 as mdgat_load_pooled_encoder_f64 takes it (pack.pack_pooled_encoder)
        self._sig_holder = [self._signature()]
        # replicas never run __init__, so only the original module owns (and finally frees) the handles
        weakref.finalize(self, _close_states, self._states)

    # ------------------------------------------------------------------ copy / pickle
    _RUNTIME_ATTRS = ('_states', '_states_lock', '_blob_holder', '_blob64_holder', '_pooled_holder', '_sig_holder')

    def __getstate__(self):
        """copy.deepcopy(net) / torch.save(net) (the reference's nn.Module supports both): library handles, locks and packed
        blobs are runtime state of THIS object and are rebuilt on first use of the copy."""
        d = self.__dict__.copy()
        for k in self._RUNTIME_ATTRS:
            d.pop(k, None)
        return d

    def __setstate__(self, d):
        super().__setstate__(d)
        self._states = {}
        self._states_lock = threading.RLock()
        self._blob_holder = [None, False]
        self._blob64_holder = [None]
        self._pooled_holder = [None]
        self._sig_holder = [self._signature()]
        weakref.finalize(self, _close_states, self._states)

    # ------------------------------------------------------------------ cache invalidation
    def _invalidate(self):
        with self._states_lock:
            for st in self._states.values():
                st.close()
            self._states.clear()
            self._blob_holder[0] = None
            self._blob_holder[1] = False
            self._blob64_holder[0] = None
            self._pooled_holder[0] = None

    def _handle_f64(self) -> bool:
        """Is this module's library handle an MDGAT_ARITH_FP64 one?  The exact mode, and every 'FPFH_gloabal' module: its encoders run
        on the fp64 products whatever follows (a float32 module hands over to the fp32-class layers right behind them)."""
        return self.exact() or getattr(self, 'descriptor', 'FPFH') == 'FPFH_gloabal'

    def exact(self) -> bool:
        """Does a forward of this module, as it stands, run the reference-exact (fp64) mode?  'auto' follows the module's
        dtype (net.double() -> True) unless attention_dtype='f16' was asked for, which is a throughput mode by definition."""
        arith = getattr(self, 'arithmetic', 'auto')
        if arith == 'auto':
            return self.bin_score.dtype == torch.float64 and getattr(self, 'attention_dtype', 'fp32') == 'fp32'
        return arith == 'fp64'

    def _signature(self):
        ts = list(self.parameters()) + list(self.buffers())
        return tuple((t.data_ptr(), t._version, t.dtype, t.device) for t in ts)

    def _invalidate_if_changed(self):
        # test.py:193 calls net.double().eval() before EVERY forward: a cast that changes nothing must not
        # throw the packed weights away
        sig = self._signature()
        if sig != self._sig_holder[0]:
            self._sig_holder[0] = sig
            if self._blob_holder[1]:
                # the weights in use were installed by load_packed(): this module's own parameters (random init on
                # every rank but the broadcasting one) are not what runs, so moving / casting them changes nothing
                return
            self._invalidate()

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        if hasattr(self, '_sig_holder'):
            self._invalidate_if_changed()
        return out

    def load_state_dict(self, state_dict, *a, **k):
        out = super().load_state_dict(state_dict, *a, **k)
        self._sig_holder[0] = self._signature()
        self._invalidate()          # new parameters: they replace whatever ran before, a load_packed() blob included
        return out

    def repack(self):
        """Call after modifying parameters in place (nothing else tracks in-place edits); also ends the reign of a
        blob installed by load_packed()."""
        self._invalidate()

    def _replicate_for_data_parallel(self):
        # torch.nn.DataParallel (test.py:158) calls this on the owner, in the caller's thread, before every forward
        # with more than one device: pack here, where the parameters still are parameters
        if not self._blob_holder[1]:
            self._host_blob()
        return super()._replicate_for_data_parallel()

    # ------------------------------------------------------------------ library state
    def _extract_mode(self):
        if self.loss_method == 'superglue':
            return _lib.EXTRACT_THRESHOLD_MUTUAL if self.mutual_check else _lib.EXTRACT_THRESHOLD
        return _lib.EXTRACT_DUSTBIN_MUTUAL if self.mutual_check else _lib.EXTRACT_DUSTBIN

    def _topk_schedule(self):
        return pack.resolve_topk_schedule(self.config['L'], list(self.k))

    def packed_weights(self, dtype=None):
        """fp32 blob (numpy) of the current parameters in the library's layout (``dtype=numpy.float64``: before the
        rounding to fp32 - what arithmetic='fp64' loads in addition)."""
        import numpy as np
        return pack.pack_state_dict(self.state_dict(), self.config['L'], dtype=dtype or np.float32)

    def _host_blob(self):
        """The packed blob, made once per set of parameters and shared with DataParallel replicas."""
        with self._states_lock:
            if self._blob_holder[0] is None:
                if 'bin_score' not in self._parameters:
                    raise RuntimeError('this MDGAT is a DataParallel replica without packed weights: the owner module '
                                       'packs them in _replicate_for_data_parallel() - was replicate() bypassed?')
                self._blob_holder[0] = self.packed_weights()
            if self._blob64_holder[0] is None and self._handle_f64() and 'bin_score' in self._parameters and not self._blob_holder[1]:
                import numpy as np
                self._blob64_holder[0] = self.packed_weights(np.float64)
                if self.descriptor == 'FPFH_gloabal':
                    self._pooled_holder[0] = pack.pack_pooled_encoder(self.state_dict())
            return self._blob_holder[0]

    def _state_for(self, device: torch.device, blob_device_tensor: Optional[torch.Tensor] = None) -> _DeviceState:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        with self._states_lock:
            st = self._states.get(idx)
            if st is not None and ((st.f64 == self._handle_f64() and st.exact == self.exact()) or blob_device_tensor is not None):
                return st
            if st is not None:
                # the module's dtype changed under a blob installed by load_packed() (casts keep such a blob): the handle's
                # arithmetic is fixed at creation, so it is rebuilt from the host copies of the blob(s)
                self._states.pop(idx).close()
            lib = _lib.load()
            L = self.config['L']
            cfg = _lib.MdgatConfig()
            cfg.L = L
            cfg.sinkhorn_iters = int(self.config['sinkhorn_iterations'])
            sched = self._topk_schedule()
            for i, kk in enumerate(sched):
                cfg.topk[i] = kk
            cfg.extract_mode = self._extract_mode()
            cfg.match_threshold = float(self.config['match_threshold'])
            cfg.attention_mode = 0 if self.attention_dtype == 'fp32' else 1
            f64, exact = self._handle_f64(), self.exact()
            cfg.arithmetic = _lib.ARITH_FP64 if f64 else _lib.ARITH_FP32
            fl = getattr(self, 'f64_layers', None)
            cfg.f64_layers = 0 if fl is None else (_lib.F64_ENCODERS_ONLY if fl == 0 else int(fl))     # (C ABI: 0 = automatic)
            cfg.f64_sinkhorn = {'auto': 0, 'fp64': 1, 'fp32': -1}[getattr(self, 'sinkhorn_arithmetic', 'auto')]
            if f64 and not exact:
                # 'FPFH_gloabal' on the fp32-class path: the encoders alone in fp64, the hand-over right behind them
                cfg.f64_layers, cfg.f64_sinkhorn = _lib.F64_ENCODERS_ONLY, -1
            handle = C.c_void_p()
            _lib.check(lib.mdgat_create(C.byref(cfg), idx, C.byref(handle)), 'mdgat_create')
            st = _DeviceState(handle, idx, f64)
            st.exact = exact
            try:
                if self.lanes:
                    _lib.check(lib.mdgat_set_lanes(handle, self.lanes), 'mdgat_set_lanes')
                if exact and self._ragged_wide():
                    if lib.mdgat_set_ragged_sinkhorn(handle, {'auto': 1, 'streaming': 2}[self.ragged_sinkhorn]) < 0:
                        raise RuntimeError('mdgat_set_ragged_sinkhorn: ' + _lib.last_error())
                if not f64 and getattr(self, 'ragged_sinkhorn_fp32', 'pair') == 'split':
                    # an MDGAT_ARITH_FP32 handle: its ragged forwards run the split form of the fp32 Sinkhorn (no other call reads the mode)
                    if lib.mdgat_set_ragged_sinkhorn(handle, 1) < 0:
                        raise RuntimeError('mdgat_set_ragged_sinkhorn: ' + _lib.last_error())
                if not exact and getattr(self, 'ragged_slots_fp32', 'narrow') == 'wide':
                    # the fp32-class ragged plan of this handle (an MDGAT_ARITH_FP32 one, or the fp64 one that runs the encoders alone)
                    if lib.mdgat_set_ragged_fp32_slots(handle, 1) < 0:
                        raise RuntimeError('mdgat_set_ragged_fp32_slots: ' + _lib.last_error())
                if blob_device_tensor is not None:
                    n = blob_device_tensor.numel()
                    _lib.check(lib.mdgat_load_weights(handle, C.c_void_p(blob_device_tensor.data_ptr()), n, 1),
                               'mdgat_load_weights')
                else:
                    blob = self._host_blob()
                    assert blob.size == lib.mdgat_blob_floats(L), (blob.size, lib.mdgat_blob_floats(L))
                    _lib.check(lib.mdgat_load_weights(handle, blob.ctypes.data_as(C.c_void_p), blob.size, 0),
                               'mdgat_load_weights')
                if f64:
                    blob64 = self._blob64_holder[0]
                    if blob64 is None:
                        raise RuntimeError('the exact mode (a float64 module, or arithmetic=\'fp64\') needs the fp64 blob: '
                                           'load_packed(blob, blob64) on ranks that received their weights by broadcast')
                    _lib.check(lib.mdgat_load_weights_f64(handle, blob64.ctypes.data_as(C.c_void_p), blob64.size, 0),
                               'mdgat_load_weights_f64')
                    if self.descriptor == 'FPFH_gloabal':
                        pooled = self._pooled_holder[0]
                        if pooled is None:
                            raise RuntimeError("descriptor='FPFH_gloabal' needs the pooled encoder's weights: load_packed(blob, blob64, pooled) "
                                               'on ranks that received their weights by broadcast')
                        assert pooled.size == lib.mdgat_pooled_encoder_doubles(), pooled.size
                        _lib.check(lib.mdgat_load_pooled_encoder_f64(handle, pooled.ctypes.data_as(C.c_void_p), pooled.size, 0),
                                   'mdgat_load_pooled_encoder_f64')
            except Exception:
                st.close()
                raise
            self._states[idx] = st
            return st

    def set_lanes(self, lanes: int):
        """1: every kernel of a batch on the caller's stream; 2 (library default): the halves of a batch in flight on two
        streams (csrc/api.hip: forward_batched).  Applies to this module's handles on every device, now and later."""
        if lanes not in (1, 2):
            raise ValueError(f'lanes={lanes}: expected 1 or 2')
        with self._states_lock:
            self.lanes = lanes
            for st in self._states.values():
                with st.lock:
                    _lib.check(_lib.load().mdgat_set_lanes(st.handle, lanes), 'mdgat_set_lanes')

    def load_packed(self, blob: torch.Tensor, blob64: Optional[torch.Tensor] = None, pooled: Optional[torch.Tensor] = None):
        """Install an already packed fp32 blob that lives on a GPU (e.g. received by an RCCL broadcast,
        see shard.broadcast_weights) instead of packing this module's own parameters.  arithmetic='fp64' needs
        ``blob64`` as well: the same blob in float64 (``packed_weights(numpy.float64)``); descriptor='FPFH_gloabal' needs ``blob64``
        and ``pooled``, the float64 tensor of ``pack.pack_pooled_encoder``."""
        assert blob.is_cuda and blob.dtype == torch.float32 and blob.is_contiguous()
        if self._handle_f64():
            if blob64 is None or blob64.dtype != torch.float64 or blob64.numel() != blob.numel():
                raise ValueError("the exact mode (a float64 module, or arithmetic='fp64') and descriptor='FPFH_gloabal': load_packed needs "
                                 'blob64, the float64 blob of the same layout')
        if self.descriptor == 'FPFH_gloabal' and (pooled is None or pooled.dtype != torch.float64 or pooled.numel() != pack.POOLED_ENCODER_DOUBLES):
            raise ValueError("descriptor='FPFH_gloabal': load_packed needs pooled, the float64 tensor of pack.pack_pooled_encoder")
        idx = blob.device.index
        with self._states_lock:
            old = self._states.pop(idx, None)
            if old is not None:
                old.close()
            # a host copy as well: any other device of this process (DataParallel replicas, a later .to()) loads the SAME
            # weights from it - never this module's own parameters, which are random init on a rank that received a blob
            self._blob_holder[0] = blob.detach().cpu().numpy().copy()
            self._blob64_holder[0] = blob64.detach().cpu().numpy().copy() if blob64 is not None else None
            self._pooled_holder[0] = pooled.detach().cpu().numpy().copy() if pooled is not None else None
            self._blob_holder[1] = True     # stands until load_state_dict() / repack(): see _invalidate_if_changed
            self._sig_holder[0] = self._signature()
            for other in [i for i in self._states if i != idx]:
                self._states.pop(other).close()
            return self._state_for(blob.device, blob)

    # ------------------------------------------------------------------ forward
    def forward(self, data):
        kpts0, kpts1 = data['keypoints0'], data['keypoints1']
        out_dtype = self.bin_score.dtype
        if kpts0.shape[1] == 0 or kpts1.shape[1] == 0:
            return self._early_out(kpts0, kpts1)
        if self.training and getattr(self, 'train_forward', False):
            return self.training_forward(data)
        if self.training:
            raise NotImplementedError('mdgat_matcher_amd implements inference only: call .eval() (training, the '
                                      'losses of mdgat.py:486-594 and backward are out of scope)')
        loss_req = self._loss_request(data, kpts0, kpts1) if getattr(self, 'eval_loss', False) else None
        token = [0]
        # ('FPFH_only', mdgat.py:421-426, never reads the saliency)
        sig0, sig1 = (None, None) if self.descriptor == 'FPFH_only' else (data['scores0'], data['scores1'])
        res = self._run(kpts0, sig0, data['descriptors0'], kpts1, sig1, data['descriptors1'], token_out=token, loss=loss_req)
        m0, m1, s0, s1 = res[:4]
        s0, s1 = s0.to(out_dtype), s1.to(out_dtype)
        if self.loss_method != 'superglue':
            # mdgat.py:464-467: `if valid0.sum() == 0` - a host-side test in the reference too (it synchronises) - returns
            # INTEGER zero scores (torch.zeros_like(indices)) when no frame-0 keypoint of the whole batch is matched.  The
            # kernels have already zeroed the scores; the dtype follows here.
            # (the library answers from a host-mapped word its extraction kernels write - mdgat_matched_any - so the test costs a
            # stream synchronisation, as in the reference, but no reduction kernel and no copy)
            torch.cuda.current_stream(m0.device).synchronize()
            nothing_matched = not self._matched_any(m0.device, token[0])
            self.check(m0.device, synchronize=False)        # (synchronised above: report this call's status now)
            if nothing_matched:
                s0, s1 = torch.zeros_like(m0), torch.zeros_like(m1)
        else:
            self.check(m0.device)                           # the dict API reports on the failing call in every branch
        loss = m0.new_zeros((), dtype=out_dtype) if loss_req is None else self._finish_loss(loss_req, out_dtype)
        return {
            'matches0': m0,
            'matches1': m1,
            'matching_scores0': s0,
            'matching_scores1': s1,
            'loss': loss,
        }

    RAGGED_MAX_KEYPOINTS = 575      # what the register-resident fp64 Sinkhorn holds (csrc/sinkhorn_f64.hip)
    RAGGED_FP32_WIDE_MAX_KEYPOINTS = 2048     # ... under config['ragged_slots_fp32'] = 'wide' (include/mdgat_hip_wide.h: MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS)
    RAGGED_FP32_MAX_KEYPOINTS = 512     # the slots of the fp32-class ragged forward (include/mdgat_hip.h: MDGAT_RAGGED_FP32_MAX_KEYPOINTS)
    RAGGED_WIDE_MAX_KEYPOINTS = 2048    # an exact module with config['ragged_sinkhorn'] = 'auto' or 'streaming' (MDGAT_RAGGED_WIDE_MAX_KEYPOINTS)

    def _ragged_wide(self) -> bool:
        """Do this module's ragged batches, as it stands, reach the streaming fp64 Sinkhorn?  Opt-in (config['ragged_sinkhorn'] = 'auto' or
        'streaming'), and an exact module only: the fp32-class ragged branch has no fp64 Sinkhorn."""
        return getattr(self, 'ragged_sinkhorn', 'resident') in ('auto', 'streaming') and self.exact() and not self._ragged_fp32()

    def _ragged_fp32(self) -> bool:
        """Does a ragged batch of this module, as it stands, run the fp32-class ragged forward?  Opt-in (config['ragged_arithmetic'] =
        'auto' or 'module'), and then what ``forward`` runs decides: a module that is not ``exact()``."""
        return getattr(self, 'ragged_arithmetic', 'exact') in ('auto', 'module') and not self.exact()

    def _ragged_module(self) -> bool:
        """... and with config['ragged_arithmetic'] = 'module': the bank entries and the pooled descriptor run that arithmetic too."""
        return getattr(self, 'ragged_arithmetic', 'exact') == 'module' and not self.exact()

    @staticmethod
    def _early_out(kpts0, kpts1):
        """the dict of mdgat.py:374-382 for a batch (or, without the batch axis, a pair) with an empty frame"""
        k0, k1 = (k if k.dim() == 3 else k[None] for k in (kpts0, kpts1))
        shape0, shape1 = k0.shape[:-1], k1.shape[:-1]
        return {
            'matches0': k0.new_full(shape0, -1, dtype=torch.int)[0],
            'matches1': k1.new_full(shape1, -1, dtype=torch.int)[0],
            'matching_scores0': k0.new_zeros(shape0, dtype=torch.float64)[0],
            'matching_scores1': k1.new_zeros(shape1, dtype=torch.float64)[0],
            'skip_train': True,
        }

    def _ragged_checked(self, packed):
        """Everything the library assumes of a packed ragged batch, checked before the call (as ``_run`` checks a uniform one): six
        tensors [B, Np | Mp(, 3 | 33)] with one B, count vectors of B entries within the slots and the kernels' limits."""
        h0, h1 = packed['counts0_host'], packed['counts1_host']
        B = int(h0.numel())
        if h0.dim() != 1 or tuple(h1.shape) != (B,) or tuple(packed['counts0'].shape) != (B,) or tuple(packed['counts1'].shape) != (B,):
            raise ValueError(f'ragged batch: the four count vectors must hold one entry per pair (counts0_host {tuple(h0.shape)}, counts1_host '
                             f"{tuple(h1.shape)}, counts0 {tuple(packed['counts0'].shape)}, counts1 {tuple(packed['counts1'].shape)})")
        k0, k1 = packed['keypoints0'], packed['keypoints1']
        if k0.dim() != 3 or k1.dim() != 3 or k0.shape[-1] != 3 or k1.shape[-1] != 3 or packed['descriptors0'].shape[-1] != 33 or \
                packed['descriptors1'].shape[-1] != 33:
            raise ValueError('expected keypoints [B, N, 3] and 33-D FPFH descriptors [B, N, 33]')
        Np, Mp = int(k0.shape[1]), int(k1.shape[1])
        for f, P in (('0', Np), ('1', Mp)):
            for key, tail in (('keypoints', (3,)), ('scores', ()), ('descriptors', (33,))):
                if tuple(packed[key + f].shape) != (B, P) + tail:
                    raise ValueError(f'ragged batch: {key}{f} has shape {tuple(packed[key + f].shape)}: expected {(B, P) + tail} '
                                     f'({B} pairs by the count vectors)')
        self._ragged_counts_checked(h0, h1, Np, Mp)
        return B, Np, Mp

    def _ragged_counts_checked(self, h0, h1, Np, Mp):
        """the kernels' limits on the counts of a ragged batch in slots of Np x Mp"""
        kmax = max([int(k) for k in self._topk_schedule()] + [0])
        fp32_limit = self.RAGGED_FP32_WIDE_MAX_KEYPOINTS if getattr(self, 'ragged_slots_fp32', 'narrow') == 'wide' else self.RAGGED_FP32_MAX_KEYPOINTS
        limit = fp32_limit if self._ragged_fp32() else self.RAGGED_WIDE_MAX_KEYPOINTS if self._ragged_wide() else self.RAGGED_MAX_KEYPOINTS
        for b in range(int(h0.numel())):
            n, m = int(h0[b]), int(h1[b])
            if n > limit or m > limit:
                raise ValueError(f'pair {b} has {n} x {m} keypoints: ragged batches hold at most {limit} per frame')
            if min(n, m) < max(kmax, 1):
                raise ValueError(f'pair {b} has {n} x {m} keypoints: fewer than a dynamic layer keeps (k={kmax}; torch.topk raises in the reference)')
            if n > Np or m > Mp:
                raise ValueError(f'pair {b} has {n} x {m} keypoints in slots of {Np} x {Mp}')
        if Np > limit or Mp > limit:
            raise ValueError(f'slots of {Np} x {Mp} keypoints: ragged batches hold at most {limit} per frame')

    def _ragged_forward(self, inputs, return_Z, fp32_entry=False):
        """One ragged forward through the library: the PADDED device outputs (matches -1 and scores 0 beyond a pair's counts), the host
        counts and - in the dustbin modes, with the call's one synchronisation - which pairs matched anything (mdgat.py:465, per pair).
        ``inputs()`` is the runner's own preparation, made behind the mode refusals: a ``_RaggedCall``.  Returns (the outputs' tuple, the
        call's ``kept``).  ``fp32_entry``: the runner has an fp32-class entry for a module that opted in (``_ragged_fp32``)."""
        fp32 = fp32_entry and self._ragged_fp32()
        if not fp32 and (not self.exact() or self.bin_score.dtype != torch.float64):
            raise NotImplementedError("ragged batches run in the exact mode only: a float64 module (net.double()) without config['arithmetic']='fp32'"
                                      " (forward_ragged and evaluate_ragged take an fp32-class module with config['ragged_arithmetic']='auto')")
        if self.training or getattr(self, 'eval_loss', False):
            raise NotImplementedError('ragged batches run in the exact mode only: eval() mode, without the evaluation loss (eval_loss)' if not fp32 else
                                      'ragged batches run in eval() mode, without the evaluation loss (eval_loss)')
        if fp32 and self._ragged_module() and self.attention_dtype != 'fp32':
            raise NotImplementedError("the fp32-class ragged forward takes attention_dtype='fp32': the single-f16 attention kernels take no per-pair counts")
        if fp32 and not self._ragged_module() and (self.descriptor == 'FPFH_gloabal' or self.attention_dtype != 'fp32'):
            raise NotImplementedError("the fp32-class ragged forward takes descriptor 'FPFH' or 'FPFH_only' and attention_dtype='fp32': the pooled "
                                      "encoder of 'FPFH_gloabal' and the single-f16 attention kernels take no per-pair counts "
                                      "(config['ragged_arithmetic']='module' takes the pooled descriptor)")
        call = inputs()
        dev, shape = call.dev, call.shape
        st = self._state_for(dev)
        lib = _lib.load()
        with torch.cuda.device(dev), st.lock:
            stream = torch.cuda.current_stream(dev).cuda_stream
            ws = st.workspace_for(stream, lib.mdgat_workspace_bytes(st.handle, *shape), dev)
            m0, m1, s0, s1, Z = ops._match_outputs(*shape, dev, return_Z)
            _lib.check(getattr(lib, call.entry)(st.handle, *shape, *call.lead, m0.data_ptr(), m1.data_ptr(), s0.data_ptr(), s1.data_ptr(),
                                                Z.data_ptr() if Z is not None else None, *call.behind_Z, ws.data_ptr(), ws.numel(), stream),
                       call.entry)
        dustbin = self.loss_method != 'superglue'
        # the one synchronisation: which pairs matched nothing comes to the host with it
        matched = (m0 >= 0).any(dim=1).cpu() if dustbin else None
        self.check(dev, synchronize=not dustbin)
        return (m0, m1, s0, s1, Z, *call.counts, matched), call.kept

    def _run_ragged(self, packed, return_Z):
        """``_ragged_forward`` on a packed batch (``ops.pack_ragged``): its outputs' tuple."""
        def inputs():
            B, Np, Mp = self._ragged_checked(packed)
            probe = packed['keypoints0']
            if not probe.is_cuda:
                raise RuntimeError('mdgat_matcher_amd runs on MI355X (gfx950) only: inputs must be on a CUDA/HIP device; there is no CPU fallback')
            dev = probe.device
            # (the pooled descriptor's handle computes its encoders in fp64 on every path: float64 inputs into mdgat_forward_f64_ragged)
            fp32 = self._ragged_fp32() and self.descriptor != 'FPFH_gloabal'
            ins = [packed[k].to(device=dev, dtype=torch.float32 if fp32 else torch.float64).contiguous()
                   for k in ('keypoints0', 'scores0', 'descriptors0', 'keypoints1', 'scores1', 'descriptors1')]
            if self.descriptor == 'FPFH_only':          # keypoints and saliency give the shapes only (as in _run)
                for i in (0, 1, 3, 4):
                    ins[i] = torch.zeros_like(ins[i])
            cnt = ops._ragged_counts(packed, B, dev)
            return _RaggedCall(dev, (B, Np, Mp), (cnt.h0, cnt.h1), 'mdgat_forward_ragged' if fp32 else 'mdgat_forward_f64_ragged',
                               (*cnt.ptrs(), *[t.data_ptr() for t in ins]), behind_Z=(None,), kept=(cnt, ins))        # (behind Z: no taps)
        return self._ragged_forward(inputs, return_Z, fp32_entry=True)[0]

    def _run_frames_ragged(self, bank, counts, starts, normalize, return_Z, want_kpts=False):
        """``_ragged_forward`` fed from a bank of records (``ops.pack_frames``): the chunk's host counts and starts (``ops.frames_chunk``, no
        empty frame among them) -> its outputs' tuple and, with ``want_kpts``, the padded float32 keypoints the assemble kernel wrote."""
        def inputs():
            h0, h1 = counts
            B, Np, Mp = int(h0.numel()), int(h0.max()), int(h1.max())
            self._ragged_counts_checked(h0, h1, Np, Mp)
            rec = bank['records']
            if not rec.is_cuda:
                raise RuntimeError('mdgat_matcher_amd runs on MI355X (gfx950) only: the bank must be on a CUDA/HIP device; there is no CPU fallback')
            dev = rec.device
            if self.descriptor == 'FPFH_only':          # keypoints and saliency are not read (as in _run): a copy of the bank without them
                rec = rec.clone()
                rec[:, :4] = 0
            args, dc, ds = ops._frames_args(bank, counts, starts, records=rec)
            kp0, kp1 = (torch.empty((B, P, 3), dtype=torch.float32, device=dev) if want_kpts else None for P in (Np, Mp))
            return _RaggedCall(dev, (B, Np, Mp), counts, 'mdgat_forward_frames_ragged', (*args, int(bool(normalize))),
                               behind_Z=(kp0.data_ptr() if want_kpts else None, kp1.data_ptr() if want_kpts else None), kept=(kp0, kp1, dc, ds, rec))
        padded, (kp0, kp1, dc, _, _) = self._ragged_forward(inputs, return_Z, fp32_entry=self._ragged_module())
        return padded, kp0, kp1, dc

    def _ragged_scatter(self, empty, early_out, run, return_Z):
        """The per-pair dicts of a chunk some of whose pairs have an empty frame (``empty[b]``): those get ``early_out(b)`` and are set aside,
        the others run in their order as one batch (``run(order)`` -> ``_ragged_forward``'s outputs) and every dict lands at its pair's place."""
        results = [early_out(b) if e else None for b, e in enumerate(empty)]
        order = [b for b, e in enumerate(empty) if not e]
        if order:
            for b, d in zip(order, self._ragged_dicts(run(order), return_Z)):
                results[b] = d
        return results

    @torch.no_grad()
    def match_frames_ragged(self, bank, idx0, idx1, normalize=True, return_Z=False):
        """``forward_ragged`` straight from raw frame records: ``bank`` is what ``ops.pack_frames`` made of a sequence's keypoint files
        (uploaded once), the chunk of pairs two index vectors into it - pair b matches frame ``idx0[b]`` against frame ``idx1[b]``; a
        frame may serve any number of pairs.  Decoding, the loader's float32 FPFH normalisation (``normalize``; load_data.py:290-292,
        bit for bit), widening, padding and the forward run in one call of the library with one synchronisation; nothing is packed on
        the host.  Returns the list of per-pair dicts ``forward_ragged`` returns (same keys, dtypes, leading axis of 1, the integer-zero
        scores of a pair that matched nothing, ``'Z'`` with ``return_Z``), each bit for bit ``match_frames`` on that pair alone under
        ``mdgat_set_f64_attention_form(0)``.  A pair with an empty frame gets the early-out dict of mdgat.py:374-382 and is left out of
        the launch.  Records no pair of the chunk points at are never read.

        ``ValueError`` for index vectors of different length, ``IndexError`` for an index outside the bank (both before anything touches
        a device); then ``forward_ragged``'s refusals: the exact mode only, at most 575 keypoints per frame (2048 with
        ``config['ragged_sinkhorn']`` = 'auto' or 'streaming', as there), no fewer than a dynamic layer's k.  A non-finite record word or an all-zero FPFH row among a pair's own records: ``RuntimeError`` from ``check``.

        With ``config['ragged_arithmetic'] = 'module'`` a module whose forward is fp32-class runs the chunk on ITS arithmetic
        (``mdgat_forward_frames_ragged`` on its handle): 'FPFH' and 'FPFH_only' through the encoder kernel's bank form, which reads the
        records itself, 'FPFH_gloabal' through the fp64 assemble kernel and pooled encoder - each bit for bit ``forward_ragged`` of
        ``ops.assemble_frames_ragged(bank, idx0, idx1, normalize)`` on the same module, with that call's limits (512 keypoints per frame,
        ``attention_dtype='fp32'``, eval() mode without ``eval_loss``)."""
        (h0, h1), (a0, a1) = ops.frames_chunk(bank, idx0, idx1)
        rec = bank['records']
        empty = ((h0 == 0) | (h1 == 0)).tolist()
        zeros = lambda n: rec.new_zeros((1, int(n), 3), dtype=torch.float64)      # noqa: E731
        take = lambda t, order: t[order].contiguous()     # noqa: E731
        return self._ragged_scatter(empty, lambda b: self._early_out(zeros(h0[b]), zeros(h1[b])),
                                    lambda order: self._run_frames_ragged(bank, (take(h0, order), take(h1, order)), (take(a0, order), take(a1, order)),
                                                                          normalize, return_Z)[0], return_Z)

    @torch.no_grad()
    def evaluate_frames_ragged(self, bank, idx0, idx1, T0, T1, T_gt=None, gt_threshold=0.5, gt_mutual=False, normalize=True):
        """``match_frames_ragged`` and then everything the loader and the evaluation scripts derive for the chunk, on the device: the
        ground-truth matches of load_data.py:238-285 (``ops.gt_matches`` with the pairs' counts, on the float32 keypoints the assemble
        kernel wrote; ``gt_threshold``, ``gt_mutual``) and the scripts' per-pair record against them (``ops.evaluate_matches``).  ``T0`` /
        ``T1`` [B, 4, 4] float64: sensor -> world of frame ``idx0[b]`` / ``idx1[b]`` (``pose @ T_cam0_velo``; None = identity), ``T_gt``
        [B, 4, 4] (optional) the relative pose - 4x4 products the caller makes on the host from the pose files.  Returns ``{'pairs':
        match_frames_ragged's list, 'metrics': [B, len(ops.EvalColumns)] float64, 'T': [B, 4, 4], 'gt_matches0': [B, Np], 'gt_matches1':
        [B, Mp] (int64, -1 beyond a pair's counts), 'rep': [B]}``, which ``ops.EvalMeter.update`` takes.  The forward's one
        synchronisation, and ``evaluate_matches``' read of its bad-index word, as in ``evaluate_ragged``.  A pair with an empty frame
        has nothing to evaluate: ``ValueError``."""
        counts, starts = ops.frames_chunk(bank, idx0, idx1)
        h0, h1 = counts
        if int(h0.numel()) == 0 or int(h0.min()) < 1 or int(h1.min()) < 1:
            raise ValueError('evaluate_frames_ragged: an empty chunk or a pair with an empty frame has nothing to evaluate (mdgat.py:374-382): leave it out')
        only = self.descriptor == 'FPFH_only'
        padded, kp0, kp1, dc = self._run_frames_ragged(bank, counts, starts, normalize, False, want_kpts=not only)
        cnt = {'counts0': dc[0], 'counts1': dc[1], 'counts0_host': h0, 'counts1_host': h1}
        if only:        # (the forward ran on a copy of the bank without keypoints: the true ones from the assemble kernel alone)
            a = ops.assemble_frames_ragged(bank, idx0, idx1, normalize=False)
            kp0, kp1 = a['keypoints0_f32'], a['keypoints1_f32']
        g0, g1, rep = ops.gt_matches(kp0, kp1, T0, T1, threshold=gt_threshold, mutual=gt_mutual, counts=cnt)
        metrics, T, _ = ops.evaluate_matches(padded[0], padded[1], g0, g1, kp0, kp1, T_gt=T_gt, counts=cnt)
        return {'pairs': self._ragged_dicts(padded, False), 'metrics': metrics, 'T': T, 'gt_matches0': g0, 'gt_matches1': g1, 'rep': rep}

    def _ragged_dicts(self, padded, return_Z):
        """the per-pair dicts of ``forward`` from the padded outputs of ``_run_ragged`` (views, no copies)"""
        m0, m1, s0, s1, Z, h0, h1, matched = padded
        out_dtype = self.bin_score.dtype
        outs = []
        for b in range(m0.shape[0]):
            n, m = int(h0[b]), int(h1[b])
            pm0, pm1 = m0[b:b + 1, :n], m1[b:b + 1, :m]
            if matched is not None and not bool(matched[b]):
                ps0, ps1 = torch.zeros_like(pm0), torch.zeros_like(pm1)       # INTEGER zeros, as the reference's torch.zeros_like(indices)
            else:
                ps0, ps1 = s0[b:b + 1, :n].to(out_dtype), s1[b:b + 1, :m].to(out_dtype)
            d = {'matches0': pm0, 'matches1': pm1, 'matching_scores0': ps0, 'matching_scores1': ps1, 'loss': m0.new_zeros((), dtype=out_dtype)}
            if return_Z:
                d['Z'] = Z[b:b + 1, :n + 1, :m + 1]
            outs.append(d)
        return outs

    @torch.no_grad()
    def forward_ragged(self, pairs_or_packed, return_Z=False):
        """``forward`` on B pairs of DIFFERENT sizes in one call of the library: a list of the reference's per-pair dicts, as its
        ``batch_size=1`` loader yields them (test.py:132), or what ``ops.pack_ragged`` made of them.  Returns a list of B dicts, each
        what ``forward`` returns for that pair alone - keys, dtypes, the leading batch axis of 1 (``matches0`` [1, N_b]), the integer-zero
        scores of a pair that matched nothing (mdgat.py:464-467, per pair), bit for bit under ``mdgat_set_f64_attention_form(0)`` (but
        for a pair with as many keypoints in both frames as a dynamic layer's k: to rounding, include/mdgat_hip.h) - plus ``'Z'``
        [1, N_b + 1, M_b + 1] float32 with ``return_Z``.  A pair with an empty frame (list input only) gets the early-out dict
        of mdgat.py:374-382 and is left out of the launch.  One call into the library and one synchronisation.

        The exact mode only (a float64 module in eval() mode, no ``eval_loss``): ``NotImplementedError`` otherwise.  ``ValueError`` for a
        frame of more than 575 keypoints or of fewer than a dynamic layer's k, and for tensors that are not [B, N, 3] / [B, N] /
        [B, N, 33] with one B and count vectors of B entries.

        With ``config['ragged_sinkhorn'] = 'auto'`` (or ``MDGAT_RAGGED_SINKHORN=auto``) an exact module takes frames of up to 2048
        keypoints: slots within 575 run as before, the same bits; beyond, the streaming fp64 Sinkhorn runs with the pairs' counts, and
        every pair is bit for bit ``forward`` on that pair alone under ``mdgat_set_f64_attention_form(0)`` and
        ``mdgat_set_f64_sinkhorn_form(1)`` - to fp64 rounding of the pair alone in the default forms, where a small pair runs the
        register-resident Sinkhorn.  ``'streaming'`` runs the streaming form at every size.  Its workspace follows the SLOT: 35.6 MB per
        pair at 2048 keypoints.

        With ``config['ragged_arithmetic'] = 'auto'`` (or ``MDGAT_RAGGED_ARITHMETIC=auto``) a module whose forward is fp32-class (not
        ``exact()``) runs the library's fp32-class ragged forward instead (``mdgat_forward_ragged``): frames of at most 512 keypoints,
        descriptors 'FPFH' and 'FPFH_only', ``attention_dtype='fp32'``, eval() mode without ``eval_loss`` (``NotImplementedError`` /
        ``ValueError`` before anything touches a device).  Per pair the same keys, dtypes and shapes as ``forward`` on the pair alone,
        computed by the kernels that take per-pair counts: to fp32-class rounding of ``forward``, and bit-identical whatever the pair's
        position and companions as long as the slots are equal.  ``'module'`` instead of ``'auto'`` takes 'FPFH_gloabal' as well (inputs
        widened to float64 into ``mdgat_forward_f64_ragged`` on the module's handle: the encoders in fp64 with the frame maximum over a
        pair's own keypoints, the same fp32-class kernels behind them) and opens the bank entries (``match_frames_ragged``).
        ``config['ragged_sinkhorn_fp32'] = 'split'`` (or ``MDGAT_RAGGED_SINKHORN_FP32=split``) runs that forward's Sinkhorn with a pair's
        rows over several workgroups, one launch per iteration, in slots of more than 128 rows: Z to fp32 rounding of the default form's."""
        if isinstance(pairs_or_packed, dict):
            return self._ragged_dicts(self._run_ragged(pairs_or_packed, return_Z), return_Z)
        pairs = list(pairs_or_packed)
        empty = [p['keypoints0'].shape[-2] == 0 or p['keypoints1'].shape[-2] == 0 for p in pairs]
        return self._ragged_scatter(empty, lambda b: self._early_out(pairs[b]['keypoints0'], pairs[b]['keypoints1']),
                                    lambda order: self._run_ragged(ops.pack_ragged([pairs[i] for i in order], device=self.bin_score.device), return_Z),
                                    return_Z)

    @torch.no_grad()
    def evaluate_ragged(self, pairs_or_packed):
        """``forward_ragged`` and then the evaluation scripts' per-pair record of every pair in ONE launch (``ops.evaluate_matches`` with
        the pairs' counts, on the forward's own padded outputs) against their ``gt_matches0/1`` and ``T_gt`` (optional): ``{'pairs': the
        forward's list of dicts, 'metrics': [B, len(ops.EvalColumns)] float64, 'T': [B, 4, 4]}``, rows and poses bit for bit
        ``evaluate``'s on each pair alone - so the scripts' loop over a chunk of pairs becomes
        ``meter.update(net.evaluate_ragged(chunk))``.  Pairs with an empty frame have nothing to evaluate (``evaluate`` returns None for
        them): ``ValueError``."""
        packed = pairs_or_packed if isinstance(pairs_or_packed, dict) else None
        if packed is None:
            pairs = list(pairs_or_packed)
            if any(p['keypoints0'].shape[-2] == 0 or p['keypoints1'].shape[-2] == 0 for p in pairs):
                raise ValueError('evaluate_ragged: a pair with an empty frame has nothing to evaluate (mdgat.py:374-382): leave it out')
            packed = ops.pack_ragged(pairs, device=self.bin_score.device)
        if 'gt_matches0' not in packed or 'gt_matches1' not in packed:
            raise KeyError('gt_matches0')                  # as evaluate() on a dict without them
        padded = self._run_ragged(packed, False)
        m0, m1 = padded[0], padded[1]
        dev = m0.device
        metrics, T, _ = ops.evaluate_matches(m0, m1, packed['gt_matches0'], packed['gt_matches1'], packed['keypoints0'].to(dev),
                                             packed['keypoints1'].to(dev), T_gt=packed.get('T_gt'), counts=packed)
        return {'pairs': self._ragged_dicts(padded, False), 'metrics': metrics, 'T': T}

    def training_forward(self, data):
        """The reference's forward (mdgat.py:369-603, any of the three FPFH descriptors) in fp64 with BatchNorm as ``self.training`` says, composed from the
        differentiable device primitives (``mdgat_matcher_amd/train.py``): the reference's dict, whose ``loss`` (0-d for superglue /
        triplet, [B] for gap) carries a grad_fn whenever grad is enabled and a parameter requires grad, so ``loss.mean().backward()``
        fills the ``.grad`` of this module's own parameters.  In train() mode the BatchNorm buffers move as the reference's do (every
        encoder once per frame, every layer's MLP for frame 0 and then frame 1); in eval() mode they are read and left alone.  Matches
        and loss come from the same Z.  Needs a float64 module on one gfx950 device; CPU tensors raise RuntimeError (no CPU fallback), a
        DataParallel replica NotImplementedError.  The parameters are read from the modules on every call, never from the packed
        weights; the packed weights are dropped (train() mode: always, the buffers move; eval() mode: when a parameter changed in place
        since the last look), but an ``optimizer.step()`` AFTER the last call is seen by nobody: call ``repack()`` before an ``eval()``
        ``forward``.  ``forward`` calls this in train() mode when ``config['train_forward']`` (or
        ``MDGAT_TRAIN_FORWARD=1``) is set."""
        from . import train
        if 'bin_score' in self._parameters:
            if self.training:
                self._invalidate()              # the kernels move the BatchNorm buffers behind autograd's version counters
            else:
                self._invalidate_if_changed()   # in-place optimizer updates since the last call: the packed weights are stale
        return train.training_forward(self, data)

    def training_batch_frames(self, bank, idx0, idx1, T0, T1, T_gt=None, max_keypoints=512, gt_threshold=0.5, gt_mutual=None, min_saliency=10.0,
                              normalize=True):
        """The reference loader's TRAINING batch (``SparseDataset.__getitem__`` with ``ensure_kpts_num``, train.py's default for the training
        and the validation set) for the chunk of pairs ``idx0[b]`` / ``idx1[b]`` of an ``ops.pack_frames`` bank, as device tensors: the
        saliency filter, the truncation or padding to ``max_keypoints``, the float32 FPFH normalisation (``ops.assemble_frames_train``)
        and the ground-truth matches of load_data.py:238-285 (``ops.gt_matches`` on the float32 keypoints) - two launches, one
        synchronisation.  ``T0`` / ``T1`` [B, 4, 4] float64: sensor -> world of the frames (``pose @ T_cam0_velo``; None = identity), as
        in ``evaluate_frames_ragged``; ``gt_mutual`` None = ``self.mutual_check`` (the reference hands one option to loader and model).
        Returns what ``training_forward`` takes - ``keypoints0/1`` [B, T, 3], ``scores0/1``, ``descriptors0/1`` (float64), ``gt_matches0/1``
        (int64 [B, T]) - plus ``rep`` [B], ``T_gt`` when given, and the assemble's ``keypoints0_f32/1_f32``, ``source0/1``, ``salient0/1``.
        ``ValueError`` naming the pair and the frame for a frame without a salient keypoint (the reference's loader does not terminate
        on it); ``RuntimeError`` for a kept record with a non-finite word or an all-zero FPFH row; ``ops.assemble_frames_train``'s
        refusals otherwise."""
        from . import train
        return train.training_batch_frames(self, bank, idx0, idx1, T0, T1, T_gt=T_gt, max_keypoints=max_keypoints, gt_threshold=gt_threshold,
                                           gt_mutual=gt_mutual, min_saliency=min_saliency, normalize=normalize)

    def training_forward_frames(self, bank, idx0, idx1, T0, T1, **batch_options):
        """``training_forward(training_batch_frames(bank, idx0, idx1, T0, T1, **batch_options))``: a training step (train() mode) or a
        validation step (eval() mode: train.py's validation loader runs with ``ensure_kpts_num`` too) straight from a resident bank of
        raw records.  ``training_forward``'s requirements: a float64 module on the bank's device, ``NotImplementedError`` otherwise
        (before anything is launched)."""
        if 'bin_score' not in self._parameters:
            raise NotImplementedError('training_forward on a DataParallel replica: multi-GPU training is out of scope (one device only)')
        dev = bank['records'].device
        if self.bin_score.dtype != torch.float64 or self.bin_score.device != dev:
            raise NotImplementedError(f'training_forward_frames needs a float64 module on the bank\'s device ({dev}): call net.double().to(device) '
                                      f'(the module is {self.bin_score.dtype} on {self.bin_score.device}); the fp32-class path has no backward')
        return self.training_forward(self.training_batch_frames(bank, idx0, idx1, T0, T1, **batch_options))

    def evaluate(self, data):
        """``forward(data)`` and then the evaluation scripts' per-pair record (test.py:212-296, test_registration_metric.py:213-264) of
        the forward's own device outputs against ``data['gt_matches0/1']`` and ``data['T_gt']`` (optional): the forward's dict plus
        ``'metrics'`` [B, len(ops.EvalColumns)] float64 and ``'T'`` [B, 4, 4], the pose from the matches.  The scripts' loop body
        becomes ``meter.update(net.evaluate(pred))`` with an ``ops.EvalMeter``.  ``forward`` itself is unchanged."""
        out = self.forward(data)
        if out.get('skip_train'):                 # an empty frame: nothing to evaluate (mdgat.py:374-382)
            return {**out, 'metrics': None, 'T': None}
        dev = out['matches0'].device
        metrics, T, _ = ops.evaluate_matches(out['matches0'], out['matches1'], data['gt_matches0'], data['gt_matches1'],
                                             data['keypoints0'].to(dev), data['keypoints1'].to(dev), T_gt=data.get('T_gt'))
        return {**out, 'metrics': metrics, 'T': T}

    def _loss_request(self, data, kpts0, kpts1):
        """The loss inputs of mdgat.py:486-594, checked before anything is launched."""
        gt0, gt1 = data['gt_matches0'], data['gt_matches1']            # KeyError when absent, as in the reference (mdgat.py:438-439)
        method = _lib.LOSS_METHODS.get(self.loss_method)
        if method is None:
            raise ValueError(f"loss_method={self.loss_method!r}: the loss is defined for 'superglue', 'triplet_loss' and 'gap_loss'")
        B, N, M = kpts0.shape[0], kpts0.shape[1], kpts1.shape[1]
        if tuple(gt0.shape) != (B, N) or tuple(gt1.shape) != (B, M):
            raise ValueError(f'gt_matches0 {tuple(gt0.shape)} / gt_matches1 {tuple(gt1.shape)}: expected [{B}, {N}] / [{B}, {M}]')
        if method != _lib.LOSS_GAP and N != M:
            raise ValueError(f'loss_method={self.loss_method!r} needs frames of equal size (N={N}, M={M}): the reference\'s index '
                             "tensors do not broadcast otherwise; 'gap_loss' takes ragged pairs")
        dev = kpts0.device
        return {'method': method, 'gt': (gt0, gt1), 'N': N, 'M': M,
                'g0': gt0.to(device=dev, dtype=torch.int64).contiguous(), 'g1': gt1.to(device=dev, dtype=torch.int64).contiguous(),
                'loss': torch.empty(B, dtype=torch.float64, device=dev), 'bad': torch.zeros(1, dtype=torch.int32, device=dev)}

    def _finish_loss(self, req, out_dtype):
        """After the forward's synchronisation: the bad-index word, the reference's in-place rewrite of the gts, the loss."""
        if int(req['bad'].item()):
            raise IndexError(f"gt_matches0 holds a value outside [-1, {req['M']}] or gt_matches1 one outside [-1, {req['N']}]")
        if req['method'] != _lib.LOSS_SUPERGLUE:
            # mdgat.py:519-520, 554-555 rewrite the caller's tensors in place (test.py:237-238 undoes it)
            gt0, gt1 = req['gt']
            gt0[gt0 == -1] = req['M']
            gt1[gt1 == -1] = req['N']
        per_pair = req['loss']
        # gap: one loss per pair [B] (mdgat.py:594); superglue / triplet: the mean (511, 546), 0-d
        return per_pair.to(out_dtype) if req['method'] == _lib.LOSS_GAP else per_pair.mean().to(out_dtype)

    def _matched_any(self, device, token=0) -> bool:
        """Did the forward that carried ``token`` on ``device`` (already synchronised by the caller) match any frame-0 keypoint?
        (mdgat.py:465.)  The token is per call - read under the handle's lock right after the enqueue (``_run``) - so forwards
        other threads or streams put on the same handle in the meantime do not change the answer; 0 = the handle's last call."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        with self._states_lock:
            st = self._states.get(idx)
        flag = C.c_uint(0)
        _lib.check(_lib.load().mdgat_matched_any(st.handle, int(token), C.byref(flag)), 'mdgat_matched_any')
        return bool(flag.value)

    def check(self, device=None, synchronize=True):
        """Status of the asynchronous forwards on ``device`` since the last check.  Raises ``RuntimeError`` if an
        activation left the f16 operand range (|v| >= 6e4) or a non-finite value reached a kernel - the outputs of those
        calls are invalid (``mdgat_async_status``); returns ``{'sinkhorn_fallback': bool}`` otherwise (informational: a
        Sinkhorn launch that lost a partner workgroup was redone by the streaming kernel, results valid).  ``forward``
        (the dict API of the reference) calls this itself; after ``match()`` / ``match_frames()`` - which never
        synchronise - call it once the results are needed."""
        dev = torch.device(device) if device is not None else self.bin_score.device
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        with self._states_lock:
            st = self._states.get(idx)
        if st is None:
            return {'sinkhorn_fallback': False}
        if synchronize:
            # Every stream this module's forwards were enqueued on (the per-stream workspaces remember them) - not just the
            # current one: the status words are per handle, and a caller that ran _run / match_frames on stream A and asks from
            # stream B would otherwise read (and clear) them before A's kernels have written.  Other streams of the process
            # are left alone (no device-wide synchronisation).
            torch.cuda.current_stream(dev).synchronize()
            with st.lock:
                handles = list(st.workspaces)
            cur = torch.cuda.current_stream(dev).cuda_stream
            for hnd in handles:
                if hnd == cur:
                    continue
                if hnd == 0:        # the legacy default stream: pool streams are non-blocking and do not wait for it
                    torch.cuda.default_stream(dev).synchronize()
                else:
                    _sync_raw_stream(hnd, dev)
        fb, rg = C.c_uint(0), C.c_uint(0)
        _lib.check(_lib.load().mdgat_async_status(st.handle, 1, C.byref(fb), C.byref(rg)), 'mdgat_matcher_amd')
        return {'sinkhorn_fallback': bool(fb.value)}

    @staticmethod
    def _f32(t, device):
        return t.to(device=device, dtype=torch.float32).contiguous()

    def _run(self, kpts0, sigma0, fpfh0, kpts1, sigma1, fpfh1, want_Z=False, taps=None, frames=None, normalize=True, token_out=None,
             loss=None):
        """One forward through the library on the current stream.  Either six arrays (keypoints / saliency / FPFH per
        frame) or ``frames=(records0, records1)`` raw [B, N, 37] loader records.  Asynchronous; returns device tensors
        ``(matches0, matches1, mscores0, mscores1, Z or None)``.  ``loss`` (six arrays only): a request of ``_loss_request``
        whose ``loss`` / ``bad`` tensors the forward fills."""
        probe = frames[0] if frames is not None else kpts0
        if not probe.is_cuda:
            raise RuntimeError('mdgat_matcher_amd runs on MI355X (gfx950) only: inputs must be on a CUDA/HIP '
                               'device; there is no CPU fallback')
        dev = probe.device
        st = self._state_for(dev)
        f64 = st.f64
        if frames is not None:
            if frames[0].shape[-1] != 37 or frames[1].shape[-1] != 37 or frames[0].dim() != 3:
                raise ValueError('expected frame records [B, N, 37] = xyz | saliency | 33-D FPFH (load_data.py:152-165)')
            ins = [self._f32(frames[0], dev), self._f32(frames[1], dev)]
            if self.descriptor == 'FPFH_only':
                ins = [t.clone() for t in ins]
                for t in ins:
                    t[..., :4] = 0          # keypoints and saliency are not read (below)
            B, N, M = ins[0].shape[0], ins[0].shape[1], ins[1].shape[1]
        else:
            if fpfh0.shape[-1] != 33 or fpfh1.shape[-1] != 33 or kpts0.shape[-1] != 3 or kpts1.shape[-1] != 3:
                raise ValueError('expected keypoints [B, N, 3] and 33-D FPFH descriptors [B, N, 33]')
            in_dtype = torch.float64 if f64 else torch.float32
            if self.descriptor == 'FPFH_only':
                # mdgat.py:421-426 reads the keypoints for their shapes only and the saliency not at all: the library, whose packed
                # keypoint encoder is all zeros, is handed zeros (0 x a huge or non-finite coordinate would not be an exact zero)
                kpts0, kpts1 = (torch.zeros(k.shape, dtype=in_dtype, device=dev) for k in (kpts0, kpts1))
                sigma0, sigma1 = (torch.zeros(k.shape[:-1], dtype=in_dtype, device=dev) for k in (kpts0, kpts1))
            ins = [t.to(device=dev, dtype=in_dtype).contiguous() for t in (kpts0, sigma0, fpfh0, kpts1, sigma1, fpfh1)]
            B, N, M = kpts0.shape[0], kpts0.shape[1], kpts1.shape[1]
        lib = _lib.load()
        with torch.cuda.device(dev), st.lock:
            stream = torch.cuda.current_stream(dev).cuda_stream
            need = lib.mdgat_forward_loss_workspace_bytes(st.handle, B, N, M) if loss is not None else lib.mdgat_workspace_bytes(st.handle, B, N, M)
            ws = st.workspace_for(stream, need, dev)
            m0, m1, s0, s1, Z = ops._match_outputs(B, N, M, dev, want_Z)
            tap_struct = None
            if taps is not None:
                tap_struct = _lib.MdgatTaps()
                for name in _lib.TAP_NAMES:
                    t = taps.get(name)
                    setattr(tap_struct, name, t.data_ptr() if t is not None else None)
            outs = (m0.data_ptr(), m1.data_ptr(), s0.data_ptr(), s1.data_ptr(), Z.data_ptr() if Z is not None else None,
                    C.byref(tap_struct) if tap_struct is not None else None, ws.data_ptr(), ws.numel(), stream)
            if loss is not None:
                req = _lib.MdgatLossRequest(loss['method'], float(self.triplet_loss_gamma), loss['g0'].data_ptr(), loss['g1'].data_ptr(),
                                            loss['loss'].data_ptr(), loss['bad'].data_ptr())
                fn = lib.mdgat_forward_f64_loss if f64 else lib.mdgat_forward_loss
                rc = fn(st.handle, B, N, M, *[t.data_ptr() for t in ins], *outs[:6], C.byref(req), *outs[6:])
            elif frames is not None:
                rc = lib.mdgat_forward_frames(st.handle, B, N, M, ins[0].data_ptr(), ins[1].data_ptr(), int(bool(normalize)), *outs)
            elif f64:
                rc = lib.mdgat_forward_f64(st.handle, B, N, M, *[t.data_ptr() for t in ins], *outs)
            else:
                rc = lib.mdgat_forward(st.handle, B, N, M, *[t.data_ptr() for t in ins], *outs)
            if token_out is not None:
                token_out[0] = int(lib.mdgat_last_token(st.handle))     # (still under st.lock: this call's token)
            _lib.check(rc, 'mdgat_forward_frames' if frames is not None else 'mdgat_forward_f64' if f64 else 'mdgat_forward')
        return m0, m1, s0, s1, Z

    def profile(self, device, enable: bool):
        """Switch the library's per-kernel-class HIP-event timing of the forward on/off for ``device`` and
        return what was accumulated since the previous call: ``{class: (total_ms, launches)}``."""
        st = self._state_for(torch.device(device))
        ms = (C.c_double * len(_lib.PROF_CLASSES))()
        n = (C.c_longlong * len(_lib.PROF_CLASSES))()
        with st.lock:
            _lib.check(_lib.load().mdgat_profile(st.handle, int(bool(enable)), ms, n), 'mdgat_profile')
        return {name: (ms[i], n[i]) for i, name in enumerate(_lib.PROF_CLASSES)}

    @torch.no_grad()
    def match_frames(self, frames0, frames1, normalize=True, return_scores=False):
        """Match straight from the loader's raw keypoint records (``load_data.py:146-165``): ``frames`` are
        ``[B, N, 37]`` (or ``[N, 37]``) float32 rows ``xyz | saliency | FPFH``, exactly the content of the KITTI
        keypoint ``.bin`` files.  The record split and the FPFH L2 normalisation (``load_data.py:290-292``) happen
        inside the encoder kernel.  Returns ``(matches0, matches1, mscores0, mscores1[, Z])``."""
        single = frames0.dim() == 2
        if single:
            frames0, frames1 = frames0[None], frames1[None]
        m0, m1, s0, s1, Z = self._run(None, None, None, None, None, None, want_Z=return_scores, frames=(frames0, frames1),
                                      normalize=normalize)
        outs = [m0, m1, s0, s1] + ([Z] if return_scores else [])
        if single:
            outs = [o[0] for o in outs]
        return tuple(outs)

    # ------------------------------------------------------------------ match() API
    @torch.no_grad()
    def match(self, kpts0, desc0, kpts1, desc1, scores0=None, scores1=None, return_scores=False):
        """``match(kpts0, desc0, kpts1, desc1)`` convenience API named by the north star.

        kpts [B, N, 3] (or [N, 3]), desc = 33-D FPFH rows (L2-normalised as load_data.py:290-292 does),
        scores = per-keypoint saliency, which the keypoint encoder consumes (mdgat.py:184-188) and is
        therefore required.  Returns ``(matches0, matches1, mscores0, mscores1[, Z])``; ``Z`` is the
        (N+1) x (M+1) log assignment matrix of log_optimal_transport."""
        only = self.descriptor == 'FPFH_only'           # (no KeypointEncoder: the saliency is not read)
        if (scores0 is None or scores1 is None) and not only:
            raise ValueError('match() needs the keypoint saliency scores0/scores1 (KeypointEncoder input)')
        single = kpts0.dim() == 2
        if single:
            kpts0, desc0, kpts1, desc1 = kpts0[None], desc0[None], kpts1[None], desc1[None]
            scores0, scores1 = (None, None) if only else (scores0[None], scores1[None])
        m0, m1, s0, s1, Z = self._run(kpts0, scores0, desc0, kpts1, scores1, desc1, want_Z=return_scores)
        outs = [m0, m1, s0, s1] + ([Z] if return_scores else [])
        if single:
            outs = [o[0] for o in outs]
        return tuple(outs)


def match(model: MDGAT, kpts0, desc0, kpts1, desc1, scores0=None, scores1=None, return_scores=False):
    """Functional form of :meth:`MDGAT.match`."""
    return model.match(kpts0, desc0, kpts1, desc1, scores0, scores1, return_scores=return_scores)
