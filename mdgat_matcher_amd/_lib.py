"""ctypes binding of libmdgat_hip.so (C ABI in include/mdgat_hip.h).

The library is hand-written HIP for gfx950; there is no CPU or PyTorch fallback: if the shared
object is missing, importing the product path raises immediately."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('MDGAT_HIP_LIB') or os.path.join(_HERE, 'libmdgat_hip.so')   # override: kernel experiments only

MAX_LAYERS = 64

EXTRACT_DUSTBIN = 0
EXTRACT_DUSTBIN_MUTUAL = 1
EXTRACT_THRESHOLD = 2
EXTRACT_THRESHOLD_MUTUAL = 3

PROF_CLASSES = ('encoder', 'layer', 'attention_full', 'attention_topk', 'scores', 'sinkhorn', 'extract', 'layer_first', 'layer_last',
                'f64_gemm', 'f64_attention_full', 'f64_attention_topk', 'f64_other')

LOSS_SUPERGLUE = 0
LOSS_TRIPLET = 1
LOSS_GAP = 2
LOSS_METHODS = {'superglue': LOSS_SUPERGLUE, 'triplet_loss': LOSS_TRIPLET, 'gap_loss': LOSS_GAP}     # config['loss_method'] -> mdgat_loss_method

ARITH_FP32 = 0
ARITH_FP64 = 1
F64_ENCODERS_ONLY = -1

# mdgat_eval_column (include/mdgat_hip.h), in order, and the mdgat_eval_status bits
EVAL_COLUMNS = ('n_valid', 'n_valid_gt', 'n_gt_negative', 'true_positive', 'true_negative', 'false_positive', 'n_valid_and_gt_positive',
                'false_positive_reg', 'false_negative', 'repeatability', 'precision', 'recall', 'matching_score', 'accuracy', 'fp_rate',
                'tp_rate', 'tp_rate2', 'fp_rate_reg', 'tp_rate_reg', 'inliers', 'inlier_ratio', 'trans_error', 'rot_error', 'status')
EVAL_BANNED = 1
EVAL_TOO_FEW_MATCHES = 2
EVAL_REGISTRATION_FAIL = 4
EVAL_RTE_OK = 8
EVAL_RRE_OK = 16

OK = 0
ERR_BAD_ARG = -1
ERR_HIP = -2
ERR_UNSUPPORTED = -3
ERR_NO_WEIGHTS = -4


class MdgatConfig(C.Structure):
    _fields_ = [
        ('L', C.c_int32),
        ('sinkhorn_iters', C.c_int32),
        ('topk', C.c_int32 * MAX_LAYERS),
        ('extract_mode', C.c_int32),
        ('match_threshold', C.c_float),
        ('attention_mode', C.c_int32),
        ('arithmetic', C.c_int32),
        ('f64_layers', C.c_int32),
        ('f64_sinkhorn', C.c_int32),
    ]


class MdgatTaps(C.Structure):
    _fields_ = [('x_enc', C.c_void_p), ('x_layers', C.c_void_p), ('mdesc', C.c_void_p), ('scores', C.c_void_p),
                ('topk_sel', C.c_void_p)]


TAP_NAMES = ('x_enc', 'x_layers', 'mdesc', 'scores', 'topk_sel')


class MdgatLossRequest(C.Structure):
    _fields_ = [('method', C.c_int32), ('gamma', C.c_double), ('gt0', C.c_void_p), ('gt1', C.c_void_p), ('loss', C.c_void_p),
                ('bad_index', C.c_void_p)]


MLP_MAX_CONVS = 4


class MdgatMlpDesc(C.Structure):
    _fields_ = [('n_conv', C.c_int32), ('R', C.c_int32), ('K0', C.c_int32), ('K1', C.c_int32), ('C', C.c_int32 * MLP_MAX_CONVS),
                ('training', C.c_int32),
                ('eps', C.c_double * (MLP_MAX_CONVS - 1)), ('momentum', C.c_double * (MLP_MAX_CONVS - 1)),
                ('W', C.c_void_p * MLP_MAX_CONVS), ('bias', C.c_void_p * MLP_MAX_CONVS),
                ('gamma', C.c_void_p * (MLP_MAX_CONVS - 1)), ('beta', C.c_void_p * (MLP_MAX_CONVS - 1)),
                ('running_mean', C.c_void_p * (MLP_MAX_CONVS - 1)), ('running_var', C.c_void_p * (MLP_MAX_CONVS - 1)),
                ('num_batches_tracked', C.c_void_p * (MLP_MAX_CONVS - 1))]


class MdgatMlpGrads(C.Structure):
    _fields_ = [('dx0', C.c_void_p), ('dx1', C.c_void_p), ('dW', C.c_void_p * MLP_MAX_CONVS), ('dbias', C.c_void_p * MLP_MAX_CONVS),
                ('dgamma', C.c_void_p * (MLP_MAX_CONVS - 1)), ('dbeta', C.c_void_p * (MLP_MAX_CONVS - 1))]


# name -> (restype, argtypes); every symbol include/mdgat_hip.h declares
SIGNATURES = {
    'mdgat_create': (C.c_int, [C.POINTER(MdgatConfig), C.c_int, C.POINTER(C.c_void_p)]),
    'mdgat_load_weights': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    'mdgat_load_weights_f64': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    'mdgat_weights_f64_device_ptr': (C.c_void_p, [C.c_void_p]),
    'mdgat_load_pooled_encoder_f64': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    'mdgat_pooled_encoder_doubles': (C.c_size_t, []),
    'mdgat_frame_max_f64': (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'mdgat_frame_max_backward_f64': (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'mdgat_blob_floats': (C.c_size_t, [C.c_int]),
    'mdgat_weights_device_ptr': (C.c_void_p, [C.c_void_p]),
    'mdgat_destroy': (None, [C.c_void_p]),
    'mdgat_last_error': (C.c_char_p, []),
    'mdgat_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    'mdgat_forward': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_void_p] * 4 +
                      [C.c_void_p, C.POINTER(MdgatTaps), C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_forward_f64': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_void_p] * 4 +
                          [C.c_void_p, C.POINTER(MdgatTaps), C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_forward_f64_ragged': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_void_p] * 6 + [C.c_void_p] * 4 +
                                 [C.c_void_p, C.POINTER(MdgatTaps), C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_forward_ragged': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_void_p] * 6 + [C.c_void_p] * 4 +
                             [C.c_void_p, C.POINTER(MdgatTaps), C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_forward_frames_ragged': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8 + [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                              C.c_int] + [C.c_void_p] * 7 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_assemble_frames_f64_ragged': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8 + [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                   C.c_int] + [C.c_void_p] * 6),
    'mdgat_assemble_frames_train_f64': (C.c_int, [C.c_int, C.c_int] + [C.c_void_p] * 8 + [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_float,
                                                  C.c_int] + [C.c_void_p] * 11),
    'mdgat_forward_frames': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 +
                             [C.c_void_p, C.POINTER(MdgatTaps), C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_forward_loss': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_void_p] * 4 +
                           [C.c_void_p, C.POINTER(MdgatTaps), C.POINTER(MdgatLossRequest), C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_forward_f64_loss': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_void_p] * 4 +
                               [C.c_void_p, C.POINTER(MdgatTaps), C.POINTER(MdgatLossRequest), C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_forward_loss_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    'mdgat_loss': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_loss_f64': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_loss_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'mdgat_loss_backward': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_loss_backward_f64': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_loss_backward_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'mdgat_async_status': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    'mdgat_last_token': (C.c_uint, [C.c_void_p]),
    'mdgat_matched_any': (C.c_int, [C.c_void_p, C.c_uint, C.POINTER(C.c_uint)]),
    'mdgat_profile': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    'mdgat_set_lanes': (C.c_int, [C.c_void_p, C.c_int]),
    'mdgat_set_layer_split_tiles': (C.c_int, [C.c_int]),
    'mdgat_layer_plan': (C.c_int, [C.c_int] * 5 + [C.POINTER(C.c_int)] * 3),
    'mdgat_layer_launches': (None, [C.POINTER(C.c_uint64)]),
    'mdgat_set_f64_layer_fusion': (C.c_int, [C.c_int]),
    'mdgat_set_f64_attention_form': (C.c_int, [C.c_int]),
    'mdgat_set_f64_sinkhorn_form': (C.c_int, [C.c_int]),
    'mdgat_sinkhorn_f64': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_sinkhorn_f64_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'mdgat_sinkhorn_f64_extract': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_sinkhorn_f64_ragged_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'mdgat_sinkhorn_f64_ragged': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_void_p]),
    'mdgat_sinkhorn_f64_extract_ragged': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_double, C.c_int, C.c_int, C.c_float] +
                                          [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p]),
    'mdgat_sinkhorn_f64_stream_ragged_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'mdgat_sinkhorn_f64_stream_ragged': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                                   C.c_void_p]),
    'mdgat_sinkhorn_f64_extract_stream_ragged': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_double, C.c_int, C.c_int, C.c_float] +
                                                 [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p]),
    'mdgat_set_ragged_sinkhorn': (C.c_int, [C.c_void_p, C.c_int]),
    'mdgat_sinkhorn_ragged_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'mdgat_sinkhorn_ragged': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    'mdgat_sinkhorn_extract_ragged': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_float, C.c_int, C.c_int, C.c_float] +
                                      [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p]),
    'mdgat_sinkhorn_backward': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_sinkhorn_backward_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    'mdgat_match_head_f64': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p]),
    'mdgat_match_head_backward': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 10 + [C.c_size_t, C.c_void_p]),
    'mdgat_match_head_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'mdgat_mlp_forward_f64': (C.c_int, [C.POINTER(MdgatMlpDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_mlp_forward_residual_f64': (C.c_int, [C.POINTER(MdgatMlpDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                C.c_void_p]),
    'mdgat_mlp_backward_f64': (C.c_int, [C.POINTER(MdgatMlpDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(MdgatMlpGrads),
                                         C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_mlp_workspace_bytes': (C.c_size_t, [C.POINTER(MdgatMlpDesc), C.c_int]),
    'mdgat_sinkhorn': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_size_t, C.c_void_p]),
    'mdgat_sinkhorn_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'mdgat_sinkhorn_extract': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_sinkhorn_plan': (C.c_int, [C.c_int] * 4 + [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    'mdgat_sinkhorn_launches': (None, [C.POINTER(C.c_uint64)]),
    'mdgat_extract': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float] + [C.c_void_p] * 4 + [C.c_void_p]),
    'mdgat_attention': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_size_t, C.c_void_p]),
    'mdgat_attention_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'mdgat_attention_plan': (C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_int)] * 2),
    'mdgat_attention_ragged_plan': (C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_int)] * 2),
    'mdgat_attention_launches': (None, [C.POINTER(C.c_uint64)]),
    'mdgat_mfma_probe': (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.c_void_p]),
    'mdgat_mfma_f64_probe': (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.c_void_p]),
    'mdgat_pointwise_f64': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    'mdgat_gemm_f64_plan': (C.c_int, [C.c_int] * 8),
    'mdgat_gemm_f64_launches': (None, [C.POINTER(C.c_uint64)]),
    'mdgat_attention_f64_plan': (C.c_int, [C.c_int] * 9),
    'mdgat_attention_f64_geometry': (C.c_int, [C.c_int] * 9 + [C.POINTER(C.c_int)] * 3 + [C.POINTER(C.c_size_t)]),
    'mdgat_attention_f64_launches': (None, [C.POINTER(C.c_uint64)]),
    'mdgat_layer_f64_plan': (C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_int)] * 2),
    'mdgat_layer_f64_launches': (None, [C.POINTER(C.c_uint64)]),
    'mdgat_sinkhorn_f64_plan': (C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_int)] * 2),
    'mdgat_sinkhorn_f64_launches': (None, [C.POINTER(C.c_uint64)]),
    'mdgat_attention_f64': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'mdgat_attention_f64_ragged': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 4),
    'mdgat_attention_backward_f64': (C.c_int, [C.c_int] * 5 + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]),
    'mdgat_attention_backward_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'mdgat_attention_qk_probe': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_attention_qk_probe_sets': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_attention_sel': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.c_void_p]),
    'mdgat_attention_ragged': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 4 +
                               [C.c_size_t, C.c_void_p]),
    'mdgat_topk_sel_words': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'mdgat_pointwise': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                  C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    'mdgat_pose': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                             C.c_void_p, C.c_void_p]),
    'mdgat_gt_matches': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'mdgat_gt_matches_ragged': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8 + [C.c_double, C.c_int] + [C.c_void_p] * 4),
    'mdgat_eval_metrics': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_double] + [C.c_void_p] * 4),
    'mdgat_eval_metrics_ragged': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_void_p] * 7 + [C.c_double] + [C.c_void_p] * 4),
    'mdgat_knn': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_knn_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
}

_lib = None


# ... and every symbol include/mdgat_hip_wide.h declares (the per-op ragged entries for slots of up to 2048 keypoints); a table of its own, as
# the header is: tests/test_ragged_fp32_wide_refusals.py holds the two against each other and every entry to a case of
# tests/test_gpu_prefilled_wide.py or a stated exemption, as tests/test_host.py and tests/test_prefilled_table.py do for SIGNATURES
WIDE_SIGNATURES = {
    'mdgat_set_ragged_fp32_slots': (C.c_int, [C.c_void_p, C.c_int]),
    'mdgat_sinkhorn_ragged_wide_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'mdgat_sinkhorn_ragged_wide': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_size_t, C.c_void_p]),
    'mdgat_sinkhorn_extract_ragged_wide': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_float, C.c_int, C.c_int, C.c_float] +
                                           [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    'mdgat_ragged_wide_launches': (None, [C.POINTER(C.c_uint64)]),
    'mdgat_attention_ragged_wide': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_size_t, C.c_void_p]),
}


def load():
    """Load the shared library (once).  Raises if it has not been built - there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            f'or `make -C mdgat_matcher_amd/csrc`.  mdgat_matcher_amd has no CPU / PyTorch fallback.')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in {**SIGNATURES, **WIDE_SIGNATURES}.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    return load().mdgat_last_error().decode('utf-8', 'replace')


def check(rc: int, what: str = 'libmdgat_hip'):
    """Raise like the reference would: RuntimeError carrying the library's message."""
    if rc != OK:
        raise RuntimeError(f'{what} failed (status {rc}): {last_error()}')
