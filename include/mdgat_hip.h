/*
 * mdgat_hip.h - C ABI of libmdgat_hip.so: the MI355X (gfx950) implementation of the inference
 * hot path of MDGAT-matcher.
 *
 * The reference (nubot-nudt/MDGAT-matcher) is pure Python/PyTorch: it has NO native boundary.  The
 * seam this library sits behind is the Python class models.mdgat.MDGAT
 * (/root/reference/models/mdgat.py:315-603) as called from test.py:201 and
 * test_registration_metric.py:202.  Each entry point below names the reference code it replaces.
 * The Python host side (mdgat_matcher_amd/mdgat.py) binds these with ctypes; INTEGRATION.md shows
 * the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every data pointer is DEVICE memory unless stated otherwise;
 *   - all tensors are owned by the caller (PyTorch); the library keeps only its packed weights;
 *   - a workspace and every output buffer may hold anything on entry: no result depends on what they held before the call (a
 *     workspace may be re-used for another shape or another entry; the library clears, inside the call, whatever a kernel needs
 *     cleared).  An optional output that an entry documents as "left untouched" is exactly that;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - return 0 on success, a negative mdgat_status otherwise; mdgat_last_error() gives the text;
 *   - a handle is bound to one device: the forward entry points make it current for the length of the call and restore the
 *     caller's device after it, so they may be called with any device current.  The per-op entry points (mdgat_sinkhorn_f64,
 *     mdgat_attention, ...) run on the current device.  Device indices 0 .. 63 are supported (mdgat_create refuses others).
 *   - thread safety: mdgat_forward / mdgat_forward_frames on ONE handle may be called from
 *     several host threads (and streams) - the library serialises the enqueue of a call internally (a mutex in the handle: the
 *     second lane's stream, its fork / join events and the profiling state are per handle); the device work of calls issued on
 *     different streams overlaps as far as those streams allow, but the halves that run on the handle's second lane queue on
 *     that one stream in call order.  Each call needs its own workspace while it is in flight.  mdgat_set_lanes,
 *     mdgat_load_weights, mdgat_profile and mdgat_destroy must not race with a forward on the same handle.  Exact-mode
 *     (MDGAT_ARITH_FP64) forwards and the fp64 Sinkhorn entry points additionally enqueue one call at a time per device, across
 *     handles: their kernels whose workgroups wait for each other run one launch at a time per device, whatever the stream.
 *
 * Layouts (fp32, row-major, innermost last)
 *   keypoints  kpts  [B][N][3]      saliency sigma [B][N]      FPFH fpfh [B][N][33]
 *   descriptors x    [B][P][128]    P = N + M, frame-0 points first, then frame-1 points
 *   q/k/v      qkv   [B][P][3][4][32]  (which, head, dim) - heads de-interleaved, see pack.py
 *   scores           [B][N][M]      couplings / Z  [B][N+1][M+1]
 *   matches    int64 [B][N] / [B][M]    matching scores fp32 [B][N] / [B][M]
 */
#ifndef MDGAT_HIP_H
#define MDGAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDGAT_MAX_LAYERS 64 /* 2L <= 64 */
#define MDGAT_D 128         /* descriptor_dim (mdgat.py:317) */
#define MDGAT_HEADS 4       /* mdgat.py:255 */
#define MDGAT_FPFH 33       /* mdgat.py:148 */

typedef enum {
    MDGAT_OK = 0,
    MDGAT_ERR_BAD_ARG = -1,     /* e.g. top-k larger than the number of keys (torch.topk raises there) */
    MDGAT_ERR_HIP = -2,         /* a HIP runtime call failed */
    MDGAT_ERR_UNSUPPORTED = -3, /* shape / config outside what the kernels implement */
    MDGAT_ERR_NO_WEIGHTS = -4
} mdgat_status;

/* match-extraction variants of mdgat.py:441-483 */
typedef enum {
    MDGAT_EXTRACT_DUSTBIN = 0,        /* loss_method != 'superglue', mutual_check False (461-464, 480-483) */
    MDGAT_EXTRACT_DUSTBIN_MUTUAL = 1, /* loss_method != 'superglue', mutual_check True  (469-478) */
    MDGAT_EXTRACT_THRESHOLD = 2,      /* loss_method == 'superglue', mutual_check False (444, 455-458) */
    MDGAT_EXTRACT_THRESHOLD_MUTUAL = 3 /* loss_method == 'superglue', mutual_check True (447-453) */
} mdgat_extract_mode;

/* Arithmetic of the attention products (q.k and p.v).  The default carries every operand as two f16 halves and is
 * fp32-faithful (the parity bar); MDGAT_ATTENTION_F16 rounds q, k, v and the probabilities to ONE f16 each (fp32
 * accumulation, fp32 softmax statistics): a throughput mode outside the parity bar (max|dZ| ~ 2e-3), applied where a
 * kernel implements it (full attention with key counts that are multiples of 64, dynamic attention at 512 keys)
 * and ignored elsewhere. */
typedef enum { MDGAT_ATTENTION_FP32 = 0, MDGAT_ATTENTION_F16 = 1 } mdgat_attention_mode;

/* Arithmetic of the forward.  MDGAT_ARITH_FP32 (default): fp32-class products everywhere (split-f16 on the matrix cores) -
 * Z within 1e-4 of the fp64 reference wherever the top-k selections of the dynamic layers agree with the reference's, which
 * near-ties below fp32 resolution do not always (about 1.5 rows per pair at 512 keypoints).
 * MDGAT_ARITH_FP64: the reference's own arithmetic (the reference runs net.double(), test.py:193) where it decides anything
 * discontinuous: the encoders (mdgat.py:392-393) and the propagation layers up to and including the LAST dynamic layer
 * (mdgat.py:259-276 with dynamic_attention 196-210) run in fp64 on v_mfma_f64_16x16x4_f64 from fp64 inputs and fp64 weights
 * (mdgat_load_weights_f64, mdgat_forward_f64; csrc/f64.hip), so that logits.topk(k) selects what the reference selects.  By
 * default (mdgat_config.f64_sinkhorn) the tail runs in fp64 as well up to 2175 keypoints: every layer, final_proj, the score
 * matrix and Sinkhorn, the extraction's arg-maxes decided on the fp64 Z (csrc/sinkhorn_f64.hip).  Beyond that, or with
 * f64_layers != 0 or MDGAT_F64_SINKHORN_OFF, the layers behind the fp64 ones, final_proj, the score matrix and Sinkhorn run on
 * the fp32-class kernels. */
typedef enum { MDGAT_ARITH_FP32 = 0, MDGAT_ARITH_FP64 = 1 } mdgat_arithmetic;

/* Replaces the config dict of MDGAT.__init__ (mdgat.py:325-367) for descriptor == 'FPFH'. */
typedef struct {
    int32_t L;                         /* config['L']: 2L alternating self/cross layers (352-353) */
    int32_t sinkhorn_iters;            /* config['sinkhorn_iterations'] (321) */
    int32_t topk[MDGAT_MAX_LAYERS];    /* per layer 0..2L-1: 0 = attention() (190-194), k > 0 =
                                          dynamic_attention(k) (196-210); schedule of 268-272 is
                                          resolved by the host */
    int32_t extract_mode;              /* mdgat_extract_mode */
    float match_threshold;             /* config['match_threshold'] (322) */
    int32_t attention_mode;            /* mdgat_attention_mode; not a reference key (BASELINE configs[2]) */
    int32_t arithmetic;                /* mdgat_arithmetic; not a reference key (the reference IS fp64) */
    int32_t f64_layers;                /* MDGAT_ARITH_FP64: how many leading propagation layers run in fp64.  0 (what a
                                          zero-initialised config holds): automatic - up to and including the last layer with
                                          topk > 0 (the encoders only when no layer has one); n > 0: exactly n (2L: all of them);
                                          MDGAT_F64_ENCODERS_ONLY (-1): none, the encoders only */
    int32_t f64_sinkhorn;              /* MDGAT_ARITH_FP64: the tail as well - EVERY layer, final_proj, the score matrix and the optimal
                                          transport in fp64, the extraction's arg-maxes decided on the fp64 Z (csrc/sinkhorn_f64.hip).
                                          0 (a zero-initialised config): automatic - on for frames of at most 2175 keypoints (and
                                          f64_layers == 0; up to 575 the Sinkhorn holds the couplings in registers, beyond that it
                                          streams them from memory), else the fp32-class tail; 1: required (larger frames are refused);
                                          MDGAT_F64_SINKHORN_OFF (-1): the fp32-class tail behind the last dynamic layer (rounds 5 / 6:
                                          Z good to 7e-6, an arg-max whose candidates lie closer than that may fall the other way) */
} mdgat_config;
#define MDGAT_F64_ENCODERS_ONLY (-1)
#define MDGAT_F64_SINKHORN_OFF (-1)

typedef struct mdgat_handle mdgat_handle;

/* Optional taps for parity tests: any pointer may be NULL. */
typedef struct {
    float* x_enc;    /* [B][P][128]        encoder sum (mdgat.py:392-393) */
    float* x_layers; /* [2L][B][P][128]    descriptors after every layer (mdgat.py:274) */
    float* mdesc;    /* [B][P][128]        final_proj output (mdgat.py:397) */
    float* scores;   /* [B][N][M]          pre-OT scores (mdgat.py:430-431) */
    uint32_t* topk_sel; /* [2L][mdgat_topk_sel_words(B, N, M)]  the keys every dynamic layer kept (the index set of
                           mdgat.py:202 `logits.topk(k)`) as bit masks [B][4 heads][P queries][W words], W = ceil(max(N, M) / 32):
                           bit j of word w = key 32 w + j of the query's source frame; slices of full-attention layers are
                           left untouched.  Parity tests feed this selection to the oracle to separate near-tie flips of
                           the discontinuous top-k from arithmetic error. */
} mdgat_taps;
size_t mdgat_topk_sel_words(int B, int N, int M);

/* ---- lifetime ------------------------------------------------------------------------------ */

/* MDGAT(config).to(device) (test.py:156, 172).  Fails with MDGAT_ERR_BAD_ARG for a device index outside
 * 0 .. 63, with MDGAT_ERR_UNSUPPORTED unless the device is gfx950. */
int mdgat_create(const mdgat_config* cfg, int device, mdgat_handle** out);

/* net.load_state_dict(...) (test.py:159) after host-side packing (BN folded into the convs, heads
 * de-interleaved, merge folded into mlp.0; mdgat_matcher_amd/pack.py).  Every weight is the fp32
 * rounding of the folded fp64 value.  `blob` holds
 * mdgat_blob_floats(L) fp32 values; `on_device` != 0 when it is device memory (e.g. received by
 * an RCCL broadcast), else host memory. */
int mdgat_load_weights(mdgat_handle* h, const float* blob, size_t n_floats, int on_device);
size_t mdgat_blob_floats(int L);

/* MDGAT_ARITH_FP64: the same blob in fp64 - the folded weights BEFORE their rounding to fp32 (pack.py computes them in fp64;
 * same layout, mdgat_blob_floats(L) doubles).  Needed in addition to mdgat_load_weights (the layers behind the last dynamic
 * one run on the fp32 blob).  Fails with MDGAT_ERR_BAD_ARG on a handle created with another arithmetic. */
int mdgat_load_weights_f64(mdgat_handle* h, const double* blob, size_t n_doubles, int on_device);
/* Device pointer to the handle's fp64 blob (NULL before mdgat_load_weights_f64; for an RCCL broadcast). */
double* mdgat_weights_f64_device_ptr(mdgat_handle* h);

/* descriptor = 'FPFH_gloabal' (mdgat.py:156-174, 342-347): the second MLP of the pooled descriptor encoder, which the blob has no room
 * for.  `w` holds mdgat_pooled_encoder_doubles() fp64 values as pack.py's pack_pooled_encoder lays them out: encoder2.0 folded with its
 * BatchNorm and split into W1e [256][128] (the columns that read the keypoint's own encoder output e) and W1g [256][128] (those that read
 * the frame maximum of e), its bias [256], then [encoder2.3 | kenc.9] [128][384] over [hidden ; the keypoint encoder's last hidden layer]
 * and the sum of the two biases [128].  The blob of such a checkpoint carries [denc.6 | 0] and denc.6's bias as its encl.  MDGAT_ARITH_FP64
 * handles only (MDGAT_ERR_BAD_ARG otherwise); call it after mdgat_load_weights_f64.  From then on every forward of the handle runs
 * desc = encoder2([e ; max over the frame's own keypoints of e]) + kenc(...) in fp64, one product per launch (csrc/api.hip:
 * pooled_encoder64, csrc/pool_f64.hip) - with f64_layers = MDGAT_F64_ENCODERS_ONLY and f64_sinkhorn = MDGAT_F64_SINKHORN_OFF the
 * encoders alone, everything behind them on the fp32-class path.  In a ragged batch the maximum runs over a pair's counts.  A handle
 * this entry was never called on behaves exactly as before. */
int mdgat_load_pooled_encoder_f64(mdgat_handle* h, const double* w, size_t n_doubles, int on_device);
size_t mdgat_pooled_encoder_doubles(void);

/* Device pointer to the handle's packed weights (for an RCCL broadcast from rank 0). */
float* mdgat_weights_device_ptr(mdgat_handle* h);

void mdgat_destroy(mdgat_handle* h);
const char* mdgat_last_error(void);

/* ---- whole forward ---------------------------------------------------------------------------- */

/* Scratch the caller must provide to mdgat_forward for a batch of B pairs with N / M keypoints. */
size_t mdgat_workspace_bytes(const mdgat_handle* h, int B, int N, int M);

/* MDGAT.forward (mdgat.py:369-483) for descriptor == 'FPFH' without the loss (mdgat_forward_loss with a NULL request; the
 * evaluation loss of mdgat.py:486-594 is computed by mdgat_forward_loss below).
 * Z (optional, may be NULL) receives log_optimal_transport's output [B][N+1][M+1]. */
int mdgat_forward(mdgat_handle* h, int B, int N, int M,
                  const float* kpts0, const float* sigma0, const float* fpfh0,
                  const float* kpts1, const float* sigma1, const float* fpfh1,
                  int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                  float* Z, const mdgat_taps* taps,
                  void* workspace, size_t workspace_bytes, void* stream);

/* The same forward in the reference's arithmetic (handle created with MDGAT_ARITH_FP64, both blobs loaded): inputs in fp64 as
 * the reference receives them (test.py:194-199 moves the loader's float64 tensors to the device; layouts as above), outputs as
 * mdgat_forward.  With the fp64 tail (mdgat_arithmetic, mdgat_config.f64_sinkhorn) Z and the matching scores are fp32 roundings
 * of the fp64 Sinkhorn's values and the matches are decided on them in fp64; with the fp32-class tail they come from the fp32
 * Sinkhorn (within 1e-4 of the reference's fp64 values).  The taps receive fp32 roundings of the fp64 stages. */
int mdgat_forward_f64(mdgat_handle* h, int B, int N, int M,
                      const double* kpts0, const double* sigma0, const double* fpfh0,
                      const double* kpts1, const double* sigma1, const double* fpfh1,
                      int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                      float* Z, const mdgat_taps* taps,
                      void* workspace, size_t workspace_bytes, void* stream);
#define MDGAT_RAGGED_MAX_KEYPOINTS 575   /* keypoints per frame (and per padded slot) of a ragged batch: what the register-resident fp64 Sinkhorn holds */
#define MDGAT_RAGGED_FP32_MAX_KEYPOINTS 512   /* the same for the fp32-class entries that take counts (mdgat_forward_ragged and its per-op siblings) */
/* THE COUNTS OF A RAGGED BATCH.  Every ..._ragged entry takes pairs of different sizes in slots padded to Np x Mp and, behind B, Np, Mp, their
 * keypoint counts twice: counts0 / counts1, DEVICE int32 [B], read by the kernels; counts0_host / counts1_host, the same values in HOST
 * memory, on which every check is made before anything is enqueued - one function for all entries (csrc/ragged.hpp), pair by pair:
 * 1 <= counts0[b] <= Np and 1 <= counts1[b] <= Mp; where the entry runs dynamic attention, no k exceeds min(counts0[b], counts1[b])
 * (torch.topk raises in the reference); where it reads a bank of records (starts0 / starts1, DEVICE int64 [B], and starts0_host /
 * starts1_host: mdgat_forward_frames_ragged on a handle of either arithmetic, mdgat_assemble_frames_f64_ragged,
 * mdgat_assemble_frames_train_f64), 0 <= starts[b] and starts[b] + counts[b] <= rows.  Else MDGAT_ERR_BAD_ARG naming the first offending
 * pair; so for a null count or start vector. */
#define MDGAT_RAGGED_WIDE_MAX_KEYPOINTS 2048   /* the same on a handle that opted into the streaming fp64 Sinkhorn (mdgat_set_ragged_sinkhorn): the dynamic fp64 attention's limit */
/* WHICH SINKHORN A RAGGED BATCH RUNS, per handle.  Returns the previous mode, -1 for a null handle or a bad mode.
 * ON AN MDGAT_ARITH_FP32 HANDLE (mdgat_forward_ragged, mdgat_forward_frames_ragged): which form of the fp32 log-domain Sinkhorn.
 *   0  default: one workgroup per pair streams the pair's scores once per iteration, all iterations in one launch;
 *   1, 2  (alike) the SPLIT form wherever the slot has G = ceil(Np / 128) >= 2 slabs of rows: workgroup (b, g) owns rows [128 g, 128 g + 128)
 *      of pair b below counts0[b], one launch of B * G workgroups per iteration and a finishing one that writes Z - the stream's launch
 *      order is the only dependency, no workgroup waits for another, no atomics.  A pair's column partials (one (max, sum) per slab and
 *      column) and its row potentials pass from launch to launch through scratch in the workspace, 2 * G * Mp * 2 + 2 * (Np + 1) floats
 *      per pair, which mdgat_workspace_bytes(h, ...) includes from the moment the mode is set: size the workspace after changing it.
 *      The arithmetic per element is the default form's; the column partials merge in another order, so Z agrees with it to fp32
 *      rounding (both within 1e-4 of the fp64 reference), not bit for bit.  A pair's results depend on its own inputs and its slot alone.
 *      A slot of one slab (Np <= 128) runs the default form, the same bits as under mode 0.  Limits and refusals do not move (512).
 *      mdgat_profile shows every iteration as a launch of MDGAT_PROF_SINKHORN; mdgat_sinkhorn_plan and mdgat_sinkhorn_launches know
 *      nothing of the form beyond its extraction.  The per-op entries (mdgat_sinkhorn_ragged ...) take no handle and never run it.
 * ON AN MDGAT_ARITH_FP64 HANDLE: which fp64 Sinkhorn (the exact mode's entries mdgat_forward_f64_ragged and mdgat_forward_frames_ragged;
 * the enc-only branch, which runs the fp32-class kernels behind fp64 encoders, never looks at it).
 *   0  default: the register-resident form only - slots of at most MDGAT_RAGGED_MAX_KEYPOINTS, refused under
 *      mdgat_set_f64_sinkhorn_form(1);
 *   1  automatic: slots within 575 keypoints, the form not forced to 1, run as under mode 0, the same bits; every other slot runs the
 *      STREAMING form with the counts (mdgat_sinkhorn_f64_extract_stream_ragged's kernels), up to MDGAT_RAGGED_WIDE_MAX_KEYPOINTS = 2048
 *      per frame;
 *   2  always the streaming form, up to the same 2048.
 * Where the streaming form runs, pair b's results are those of mdgat_forward_f64 on the pair alone under mdgat_set_f64_attention_form(0)
 * and mdgat_set_f64_sinkhorn_form(1), bit for bit (with the exception stated below: counts0[b] == counts1[b] == a dynamic layer's k).
 * Against the pair alone in the DEFAULT forms they agree to fp64 rounding: a small pair alone runs the register-resident Sinkhorn, which
 * sums in another order.  Beyond 2048 the entries refuse with MDGAT_ERR_UNSUPPORTED, naming 2048.  mdgat_workspace_bytes(h, ...) follows
 * the mode by the predicate the forward itself uses: wherever a ragged batch in slots of Np x Mp would run the streaming form - mode 2 at
 * every size, mode 1 from a slot of 576 rows or columns on and under mdgat_set_f64_sinkhorn_form(1) - it reserves that form's K,
 * [B][Np][Mp rounded up to 128] doubles, carved by the slot (35.6 MB per pair at 2048): size the workspace after changing either. */
int mdgat_set_ragged_sinkhorn(mdgat_handle* h, int mode);
/* mdgat_forward_f64 on a RAGGED batch: B pairs of different sizes in one call (the evaluation scripts run one pair per call because no two
 * frames hold the same number of keypoints - test.py:132; padding is no way out: padded keypoints change every softmax, every top-k and
 * the optimal transport).  Pair b has counts0[b] x counts1[b] keypoints and is stored in a slot padded to Np x Mp: kpts0 [B][Np][3], sigma0
 * [B][Np], fpfh0 [B][Np][33], frame 1 likewise with Mp; matches0 / mscores0 [B][Np], matches1 / mscores1 [B][Mp], Z [B][Np+1][Mp+1].
 *   - Pair b's results are those of mdgat_forward_f64 on pair b alone (B = 1): its matches, its scores, its block Z[b][0 .. counts0[b]]
 *     [0 .. counts1[b]] with the dustbin row at row counts0[b] and the dustbin column at column counts1[b]; the rule of mdgat.py:465-467
 *     (nothing matched: all scores zero) is applied per pair.  Bit for bit under mdgat_set_f64_attention_form(0); to rounding where the
 *     launch size selects another kernel form for the batch than for the pair.  One exception: a pair with counts0[b] == counts1[b] == k
 *     for a dynamic layer's k runs that layer on the dynamic-attention kernel here and, alone, on the full-attention kernel (top-k of
 *     k keys is all of them): the same keys are kept, the messages agree to fp64 rounding (1e-11), not bit for bit.
 *   - Beyond a pair's counts: matches -1, scores 0, the rest of its Z slot 0.
 *   - What the inputs hold beyond a pair's counts is never read: NaN there reaches no result and no guard.
 *   - Uniform counts (all Np / Mp) give the bits of mdgat_forward_f64 (with the same exception: Np == Mp == a dynamic layer's k).
 * The counts are checked as described at THE COUNTS OF A RAGGED BATCH above, against every dynamic layer's k.  The handle must run the fp64 tail on the register-resident Sinkhorn: Np, Mp <= 575,
 * f64_sinkhorn not MDGAT_F64_SINKHORN_OFF, f64_layers automatic, mdgat_set_f64_sinkhorn_form not 1 (else MDGAT_ERR_UNSUPPORTED); an fp32
 * handle is MDGAT_ERR_BAD_ARG.  A handle in mode 1 or 2 of mdgat_set_ragged_sinkhorn (above) takes Np, Mp <= 2048 under either form.  taps must be NULL.  workspace: mdgat_workspace_bytes(h, B, Np, Mp).  The batch runs unsliced on `stream`.
 * The ragged mdgat_forward_frames is mdgat_forward_frames_ragged below; there is no ragged loss.
 * One more handle is taken: the one that runs the ENCODERS ALONE in fp64 - f64_layers = MDGAT_F64_ENCODERS_ONLY, f64_sinkhorn =
 * MDGAT_F64_SINKHORN_OFF, the pooled encoder loaded (mdgat_load_pooled_encoder_f64; what a float32 'FPFH_gloabal' module creates).  Its
 * batch runs the fp64 assemble kernel and the pooled encoder with the counts (the frame maximum over a pair's own keypoints), the hand-over,
 * and behind it mdgat_forward_ragged's kernels: that entry's results (to fp32-class rounding of the pair alone, bit-identical whatever the
 * pair's position and companions in equal slots) and that entry's limits - Np, Mp <= MDGAT_RAGGED_FP32_MAX_KEYPOINTS, attention_mode not 1. */
int mdgat_forward_f64_ragged(mdgat_handle* h, int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                             const int32_t* counts1_host, const double* kpts0, const double* sigma0, const double* fpfh0, const double* kpts1,
                             const double* sigma1, const double* fpfh1, int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                             float* Z, const mdgat_taps* taps, void* workspace, size_t workspace_bytes, void* stream);
/* mdgat_forward on a RAGGED batch: the fp32-class path (an MDGAT_ARITH_FP32 handle, else MDGAT_ERR_BAD_ARG), laid out as above with float
 * inputs.  The kernels that must know a pair's own size take the counts - the encoder (a keypoint beyond its frame's count reads none of its
 * inputs and is encoded from zeros), the general attention kernel (mdgat_attention_ragged) and the one-workgroup-per-pair streaming Sinkhorn
 * with the extraction (mdgat_sinkhorn_extract_ragged); the row-wise launches in between run over the padded rows.  The stream and topk16
 * attention kernels and the cluster Sinkhorn take no counts, so this is not the uniform forward's kernel selection.
 *   - Pair b's results depend on the pair alone: bit-identical whatever its position and companions, as long as the slots are equal, and to
 *     fp32-class rounding those of mdgat_forward on the pair alone; the rule of mdgat.py:465-467 is applied per pair.
 *   - Beyond a pair's counts: matches -1, scores 0, the rest of its Z slot 0; what the inputs hold there reaches no result and no guard.
 * Np, Mp <= MDGAT_RAGGED_FP32_MAX_KEYPOINTS, attention_mode not 1 (single-f16 products), taps NULL (else MDGAT_ERR_UNSUPPORTED); the counts
 * are checked as described at THE COUNTS OF A RAGGED BATCH, against every dynamic layer's k.  workspace: mdgat_workspace_bytes(h, B, Np, Mp);
 * Z is produced there when the caller wants none.  One unsliced lane on `stream`; no loss.  The same plan fed from a bank of raw records:
 * mdgat_forward_frames_ragged on an MDGAT_ARITH_FP32 handle, below. */
int mdgat_forward_ragged(mdgat_handle* h, int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                         const int32_t* counts1_host, const float* kpts0, const float* sigma0, const float* fpfh0, const float* kpts1,
                         const float* sigma1, const float* fpfh1, int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                         float* Z, const mdgat_taps* taps, void* workspace, size_t workspace_bytes, void* stream);

/* The same forward fed with the loader's raw frame records instead of separate arrays: frames [B][N][37] fp32,
 * one record per keypoint = xyz(3) | saliency(1) | FPFH(33), the layout of the KITTI keypoint files that
 * SparseDataset.__getitem__ reads (load_data.py:146-165).  normalize_fpfh != 0 applies the loader's L2
 * normalisation of the FPFH part (load_data.py:290-292) inside the encoder kernel.  On a MDGAT_ARITH_FP64 handle the records are
 * taken through the loader's own sequence - the normalisation in float32 exactly as numpy computes it (its pairwise summation
 * order, correctly rounded square root / reciprocal / products), then widened to double (load_data.py:294-295) - so that the
 * forward sees bit for bit the inputs the reference's forward sees. */
int mdgat_forward_frames(mdgat_handle* h, int B, int N, int M, const float* frames0, const float* frames1,
                         int normalize_fpfh,
                         int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                         float* Z, const mdgat_taps* taps,
                         void* workspace, size_t workspace_bytes, void* stream);

/* mdgat_forward_f64_ragged fed from a BANK of raw records: the records of a whole sequence lie on the device once (rec0 [rows0][37], rec1
 * [rows1][37] fp32, the layout of mdgat_forward_frames; both may be the same buffer) and a chunk of pairs is two vectors of start rows.
 * Frame 0 of pair b is the counts0[b] records from row starts0[b] of rec0, frame 1 the counts1[b] records from row starts1[b] of rec1;
 * the assemble kernel decodes, normalises (normalize_fpfh, the loader's float32 arithmetic bit for bit as in mdgat_forward_frames), widens
 * and pads them into the forward's slots of Np / Mp rows, zeros beyond the counts.  Everything behind it, every result and every limit
 * are mdgat_forward_f64_ragged's; counts and starts are checked as described at THE COUNTS OF A RAGGED BATCH.
 *   - Only a pair's own records are read: what any other record of the bank holds - NaN included - reaches no result and no guard.
 *   - A non-finite word or (normalize_fpfh) an all-zero FPFH row among a pair's own records raises the handle's range-violation word
 *     (mdgat_async_status), as in mdgat_forward_frames.
 *   - kpts0_out [B][Np][3] / kpts1_out [B][Mp][3] fp32 (optional, each on its own): the keypoints as they lie in the
 *     records, zeros beyond the counts - what mdgat_gt_matches_ragged and mdgat_eval_metrics_ragged take.
 * Np, Mp <= 575, no taps.  workspace: mdgat_workspace_bytes(h, B, Np, Mp).
 * The entry follows the handle, as mdgat_forward_frames does.  On an MDGAT_ARITH_FP32 handle it runs mdgat_forward_ragged's plan with that
 * entry's results and limits (Np, Mp <= MDGAT_RAGGED_FP32_MAX_KEYPOINTS, attention_mode not 1): the encoder kernel's bank form reads the
 * records itself - no assemble pass, no staging copy - with the same normalisation, the same guard and the same kpts0_out / kpts1_out, and
 * hands the layers bit for bit what mdgat_forward_ragged gets from the float32 values of mdgat_assemble_frames_f64_ragged.  On the fp64
 * handle that runs the encoders alone (mdgat_forward_f64_ragged, its last paragraph) the assemble kernel runs in front of that plan. */
int mdgat_forward_frames_ragged(mdgat_handle* h, int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1,
                                const int32_t* counts0_host, const int32_t* counts1_host, const int64_t* starts0, const int64_t* starts1,
                                const int64_t* starts0_host, const int64_t* starts1_host, const float* rec0, int64_t rows0, const float* rec1,
                                int64_t rows1, int normalize_fpfh, int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                                float* Z, float* kpts0_out, float* kpts1_out, void* workspace, size_t workspace_bytes, void* stream);
/* Its assemble launch alone, into caller-owned in4 [B][Np+Mp][4] and in33 [B][Np+Mp][33] fp64 (rows of a pair: frame 0's Np, then frame
 * 1's Mp): x y z saliency and the FPFH row as the encoders read them.  guard (device memory, optional; the caller clears it) is set to 1
 * where the forward would raise its range-violation word.  No handle; counts and starts are checked as described at THE COUNTS OF A
 * RAGGED BATCH. */
int mdgat_assemble_frames_f64_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                     const int32_t* counts1_host, const int64_t* starts0, const int64_t* starts1, const int64_t* starts0_host,
                                     const int64_t* starts1_host, const float* rec0, int64_t rows0, const float* rec1, int64_t rows1,
                                     int normalize_fpfh, double* in4, double* in33, float* kpts0_out, float* kpts1_out, unsigned* guard,
                                     void* stream);

/* The loader's TRAIN-mode assembly of a chunk out of the same bank (SparseDataset.__getitem__ with ensure_kpts_num, train.py's default for
 * the training and the validation set; load_data.py:180-211), one launch, no handle.  Frame f of pair b is the counts[b] records from
 * row starts[b], as above, of any size >= 1.  Per frame:
 *   - the records with saliency > min_saliency (a float32 compare; 10 in the reference: a saliency of exactly min_saliency and a NaN
 *     saliency are dropped) are kept in their order, v of them;
 *   - v >= T: the first T kept records; else the loader's loop `a = vstack((a[:T - len(a)], a))` until T rows stand, so with v = 3 and
 *     T = 8 the slots hold kept rows 0 1 0 1 2 0 1 2;
 *   - every slot is decoded like a record of mdgat_assemble_frames_f64_ragged (normalize_fpfh: the loader's float32 arithmetic bit for
 *     bit) into in4 [B][T+T][4] and in33 [B][T+T][33] fp64 (rows of a pair: frame 0's T, then frame 1's T) and kpts0_out / kpts1_out
 *     [B][T][3] fp32 (what mdgat_gt_matches takes); source0 / source1 [B][T]: the record's row within its frame behind each slot;
 *     salient0 / salient1 [B]: v.
 *   - v == 0: the reference's loop never ends.  status [B][2] (pair, frame) is written for every frame: 1 there, else 0; of such a
 *     frame's outputs only salient (0) is written.
 * Only kept records are decoded: a non-finite word or (normalize_fpfh) an all-zero FPFH row among them sets guard (device memory,
 * optional; the caller clears it) to 1; what a dropped record holds beside its saliency, and what any record outside the chunk holds,
 * is never read.  The outputs are a pure function of the inputs (no atomics on values).  T outside 1 .. 2048 (the attention's limit)
 * and a NaN min_saliency are MDGAT_ERR_BAD_ARG; counts (>= 1, no upper limit) and starts are checked as described at THE COUNTS OF A
 * RAGGED BATCH. */
int mdgat_assemble_frames_train_f64(int B, int T, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                    const int32_t* counts1_host, const int64_t* starts0, const int64_t* starts1, const int64_t* starts0_host,
                                    const int64_t* starts1_host, const float* rec0, int64_t rows0, const float* rec1, int64_t rows1,
                                    float min_saliency, int normalize_fpfh, double* in4, double* in33, float* kpts0_out, float* kpts1_out,
                                    int32_t* source0, int32_t* source1, int32_t* salient0, int32_t* salient1, unsigned* status, unsigned* guard,
                                    void* stream);

/* ---- evaluation loss (mdgat.py:486-594) and its gradient with respect to Z (mdgat_loss_backward below) ------------------------- */

/* config['loss_method'] of the loss: superglue (487-511), triplet_loss (512-546), gap_loss (547-594) */
typedef enum { MDGAT_LOSS_SUPERGLUE = 0, MDGAT_LOSS_TRIPLET = 1, MDGAT_LOSS_GAP = 2 } mdgat_loss_method;

/* What the forward's loss needs besides Z: gt0 [B][N] / gt1 [B][M] int64 ground-truth matches (-1 = unmatched: the dustbin column
 * M / row N), gamma = config['triplet_loss_gamma'], loss [B] fp64 receives one value per pair - superglue: the pair's
 * (-tp - tn) / (xx + M), triplet: the mean of the pair's N + M terms (the module's loss is the mean over pairs of either), gap: the
 * pair's loss.  superglue and triplet need N == M (the reference's index tensors do not broadcast otherwise).  A gt0 value outside
 * [-1, M] or (triplet, gap) a gt1 value outside [-1, N] is an indexing error in the reference: that pair's loss is NaN and bit 0 of
 * *bad_index (device memory, optional; the caller clears it) is set.  The gts are not rewritten (the reference's in-place -1 -> M / N
 * rewrite is left to the caller). */
typedef struct {
    int32_t method;            /* mdgat_loss_method */
    double gamma;
    const int64_t* gt0;
    const int64_t* gt1;
    double* loss;
    unsigned* bad_index;
} mdgat_loss_request;

/* The loss on a caller-supplied Z [B][N+1][M+1] (fp32 or fp64; the arithmetic is fp64 either way).  workspace: 256-byte aligned,
 * mdgat_loss_workspace_bytes.  Reads Z once; no allocation, no synchronisation. */
int mdgat_loss(int B, int N, int M, const float* Z, const int64_t* gt0, const int64_t* gt1, int method, double gamma, double* loss,
               unsigned* bad_index, void* workspace, size_t workspace_bytes, void* stream);
int mdgat_loss_f64(int B, int N, int M, const double* Z, const int64_t* gt0, const int64_t* gt1, int method, double gamma, double* loss,
                   unsigned* bad_index, void* workspace, size_t workspace_bytes, void* stream);
size_t mdgat_loss_workspace_bytes(int B, int N, int M);

/* The gradient autograd takes through the reference's loss code: dZ [B][N+1][M+1] fp64 = sum_b dloss[b] d loss[b] / dZ, with loss [B]
 * the per-pair values of mdgat_loss and dloss [B] fp64 one upstream weight per pair (the mean over pairs of superglue / triplet is the
 * caller's: dloss[b] = 1 / B).  Z fp32 or fp64, the arithmetic fp64 either way; every entry of dZ is written, each by one thread and
 * without atomics on values, so a pair's gradient does not depend on the batch it travels in.  Conventions: a clamp argument that is
 * exactly 0 passes the gradient (torch.clamp); t(z) = -log(exp(z)) is differentiated literally, (-g / e) * e with e = exp(z), which is
 * -+inf or NaN where e is deep in its subnormal band or 0 (below about -745.1), as in the reference; ties between a row's or column's
 * largest non-positive entries (triplet) take the lowest index.  A gt0 value outside [-1, M] or (triplet, gap) a gt1 value outside
 * [-1, N]: that pair's dZ is NaN throughout and bit 0 of *bad (device memory, optional; the caller clears it) is set.  workspace:
 * 256-byte aligned, mdgat_loss_backward_workspace_bytes.  Arguments and limits as mdgat_loss, and (N+1) (M+1) < 2^31.  Reads Z twice;
 * no allocation, no synchronisation. */
int mdgat_loss_backward(int B, int N, int M, const float* Z, const int64_t* gt0, const int64_t* gt1, int method, double gamma,
                        const double* dloss, double* dZ, int32_t* bad, void* workspace, size_t workspace_bytes, void* stream);
int mdgat_loss_backward_f64(int B, int N, int M, const double* Z, const int64_t* gt0, const int64_t* gt1, int method, double gamma,
                            const double* dloss, double* dZ, int32_t* bad, void* workspace, size_t workspace_bytes, void* stream);
size_t mdgat_loss_backward_workspace_bytes(int B, int N, int M);

/* mdgat_forward / mdgat_forward_f64 and the loss of `req` on the forward's own Z: the fp64 Z of the exact mode's fp64 tail, else the
 * fp32 Z.  Outputs, workspace alignment and everything else as the forwards without the loss; req == NULL is exactly those.  The
 * workspace is larger (Z is always materialised: in fp64 on a MDGAT_ARITH_FP64 handle): mdgat_forward_loss_workspace_bytes. */
int mdgat_forward_loss(mdgat_handle* h, int B, int N, int M,
                       const float* kpts0, const float* sigma0, const float* fpfh0,
                       const float* kpts1, const float* sigma1, const float* fpfh1,
                       int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                       float* Z, const mdgat_taps* taps, const mdgat_loss_request* req,
                       void* workspace, size_t workspace_bytes, void* stream);
int mdgat_forward_f64_loss(mdgat_handle* h, int B, int N, int M,
                           const double* kpts0, const double* sigma0, const double* fpfh0,
                           const double* kpts1, const double* sigma1, const double* fpfh1,
                           int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                           float* Z, const mdgat_taps* taps, const mdgat_loss_request* req,
                           void* workspace, size_t workspace_bytes, void* stream);
size_t mdgat_forward_loss_workspace_bytes(const mdgat_handle* h, int B, int N, int M);

/* Asynchronous status of the handle's forwards since the last call with clear != 0 (read it after synchronising the
 * stream: the forward itself never synchronises).  *range_violation != 0: an activation left the f16 operand range
 * (|v| >= 6e4) or a non-finite value reached a kernel - every operand is carried as f16 head + f16 residual (DESIGN.md
 * section 3), so the outputs of those calls are invalid.  The fp64 layers of MDGAT_ARITH_FP64 raise it as well: every fp64
 * product tests its outputs by their exponent bits (not finite, or |v| >= 2^500 - beyond which a logit could overflow and the
 * softmax meet inf - inf; csrc/f64.hip: f64_out_of_range), between the layers, not only at the hand-over; the function then returns MDGAT_ERR_UNSUPPORTED (and the next
 * mdgat_forward on the handle does, if nobody asked before).  *sinkhorn_fallback != 0: informational - a Sinkhorn cluster
 * launch lost a partner workgroup (device shared with other work) and was redone by the streaming kernel inside the same
 * call; the results are valid.  The reference has no counterpart (ATen raises nothing either: it returns inf / NaN). */
int mdgat_async_status(mdgat_handle* h, int clear, unsigned* sinkhorn_fallback, unsigned* range_violation);

/* After the caller's synchronisation: *matched = 1 when the forward that carried `token` matched at least one frame-0 keypoint
 * anywhere in its batch (matches0 >= 0), else 0.  This is the reference's host-side test `valid0.sum() == 0`
 * (models/mdgat.py:464-467: integer zero scores when nothing matched) without a reduction kernel and a device-to-host copy: the
 * extraction kernels write the call's token into a host-mapped slot (256 slots, indexed by the token: calls of several threads
 * and streams on one handle do not disturb each other).  mdgat_last_token returns the token of the most recent
 * mdgat_forward / mdgat_forward_f64 / mdgat_forward_frames enqueued on the handle - read it before another thread can enqueue
 * (the Python wrapper does so under its per-handle lock); token 0 stands for that most recent call. */
unsigned mdgat_last_token(mdgat_handle* h);
int mdgat_matched_any(mdgat_handle* h, unsigned token, unsigned* matched);

/* Per-kernel-class timing of mdgat_forward, measured with HIP events on the launch stream (bench.py's
 * roofline leg).  mdgat_profile(h, enable, ms, launches) returns the time (ms) and launch count
 * accumulated per class since the previous call in ms[MDGAT_PROF_CLASSES] / launches[...] (either may
 * be NULL), clears them, and switches the instrumentation on or off.  While it is on, mdgat_forward
 * ends with a stream synchronisation; an interval covers the launch(es) of the class and the gap
 * before them on that lane's stream (with two lanes in flight the launches of the two lanes share the device: an interval is
 * then a launch's duration under that sharing, as a kernel trace reports it). */
enum {
    MDGAT_PROF_ENCODER = 0,        /* both encoders up to the summed descriptor */
    MDGAT_PROF_LAYER = 1,          /* fused mlp + residual + next q/k/v projection (or final_proj) */
    MDGAT_PROF_ATTENTION_FULL = 2,
    MDGAT_PROF_ATTENTION_TOPK = 3,
    MDGAT_PROF_SCORES = 4,         /* score matrix */
    MDGAT_PROF_SINKHORN = 5,
    MDGAT_PROF_EXTRACT = 6,
    MDGAT_PROF_LAYER_FIRST = 7,    /* the launch before layer 0: q/k/v projection only (a third of a layer launch's work) */
    MDGAT_PROF_LAYER_LAST = 8,     /* the launch after the last layer: mlp + residual + final_proj */
    MDGAT_PROF_F64_GEMM = 9,       /* MDGAT_ARITH_FP64: the Conv1d(k=1) products of the fp64 stages (csrc/f64.hip) */
    MDGAT_PROF_F64_ATTENTION_FULL = 10,
    MDGAT_PROF_F64_ATTENTION_TOPK = 11,
    MDGAT_PROF_F64_OTHER = 12,     /* input assembly, hand-over conversion to fp32 */
    MDGAT_PROF_CLASSES = 13
};
int mdgat_profile(mdgat_handle* h, int enable, double* ms, long long* launches);

/* How a batch is executed (no counterpart in the reference, which hands the whole batch to every ATen kernel,
 * models/mdgat.py:369-483).  lanes = 2 (default; MDGAT_FORWARD_LANES=1 in the environment selects 1): a batch of more than
 * 32 768 keypoints is cut into an even number of balanced slices which alternate between the caller's stream and a second
 * stream owned by the handle - forked from and joined to the caller's stream with events, so the call stays asynchronous
 * and ordered on the caller's stream - because two half-size forwards in flight fill each other's idle phases (csrc/api.hip:
 * forward_batched).  lanes = 1: everything on the caller's stream, slices of 65 536 keypoints beyond 1.5 x that.  Results do
 * not depend on the setting (pairs are independent).  mdgat_workspace_bytes() follows the handle's setting: size the workspace
 * after changing it. */
int mdgat_set_lanes(mdgat_handle* h, int lanes);

/* Which kernel runs the layer tail (mlp + residual + next q|k|v; models/mdgat.py:227-232, 246-248, 274, 397) of a launch.
 * Launches of at most `tiles` tiles of 128 keypoints (default 64; MDGAT_LAYER_SPLIT_TILES in the environment) run the
 * channel-split kernel of csrc/layer_split.hip (32-keypoint workgroups, the eight waves share the output channels: the
 * latency shape, test.py:132 runs batch_size = 1), larger ones the keypoint-split kernels of csrc/layer.hip.  Process-wide;
 * results are bit-identical either way.  tiles = 0: never; tiles < 0: back to the default.  Returns the previous value. */
int mdgat_set_layer_split_tiles(int tiles);

/* Which kernel a layer-tail launch of the fp32 class runs (csrc/layer.hip: launch_layer, which every layer of the fp32-class forward goes
 * through), and with what launch geometry.  The 14 instantiations it can reach, <DO_MLP, MODE3> (DO_MLP 0: projection only, the launch
 * in front of the first fp32-class layer; MODE3 1: the next layer's q | k | v, 2: final_proj) and, for layer_kernel, <.., VW, NW>:
 *    0 split<0,1>      1 split<0,2>      2 split<1,1>      3 split<1,2>       layer_split_kernel: 32 keypoints per workgroup; launches of
 *                                                                             at most mdgat_set_layer_split_tiles tiles of 128 keypoints
 *    4 layer<0,1,0,4>  5 layer<0,2,0,4>  6 layer<1,1,0,4>  7 layer<1,2,0,4>   layer_kernel, 64 keypoints per workgroup: at most 128 tiles
 *    8 layer<0,1,0,8>  9 layer<0,1,1,8> 10 layer<0,2,0,8>                     layer_kernel, 128 keypoints per workgroup: larger launches;
 *   11 layer<1,1,0,8> 12 layer<1,1,1,8> 13 layer<1,2,0,8>                     VW = 1: q | k | v with N and M multiples of 128
 * mdgat_layer_plan: the index for a launch of R = B (N + M) keypoint rows, do_mlp != 0: with the MLP and residual, mode3: 1 = q | k | v,
 * anything else = final_proj.  -1: nothing is launched (R <= 0).  *workgroups (optional): the grid, ceil(R / *keypoints_per_workgroup);
 * *keypoints_per_workgroup (optional): 32, 64 or 128; *v_store (optional): the V^T store path, as the keypoints that go out in one
 * piece - 0: none (final_proj), 1: single halves, 4: 8-byte stores ((N | M) % 4 == 0), 16: whole 32-byte row pieces of a wave
 * ((N | M) % 16 == 0; layer_kernel only: the split kernel stores such frames in runs of 4), 128: 256-byte pieces through the gather
 * buffers (VW).  All 0 with -1.  It reads the current mdgat_set_layer_split_tiles value and nothing else but its arguments: no device
 * is needed or touched; launch_layer takes its branch and its grid from the same code.
 * mdgat_layer_launches: counts[i] = launches of instantiation i by this process so far, on any device and stream (relaxed atomic
 * counters, incremented after a launch that succeeded, never reset: read them before and after a call and subtract). */
#define MDGAT_LAYER_FORMS 14
int mdgat_layer_plan(int R, int N, int M, int do_mlp, int mode3, int* workgroups, int* keypoints_per_workgroup, int* v_store);
void mdgat_layer_launches(uint64_t counts[MDGAT_LAYER_FORMS]);

/* MDGAT_ARITH_FP64: how the tail of an fp64 layer (mlp.0 + ReLU, mlp.3 + residual; models/mdgat.py:246-248, 274) and the next
 * layer's q | k | v projection (227-232) are launched.  1 (default; MDGAT_F64_LAYER_FUSION=0 in the environment selects 0): one
 * launch per layer with the hidden activation kept on chip (csrc/layer_f64.hip) - launches of at most a quarter of the compute
 * units in 16-keypoint blocks (one pair per call) with FOUR workgroups per block that split the output channels and exchange the
 * hidden layer and the new x through L2; 2: the same, one workgroup per block at every launch size; 0: three launches of the fp64
 * product kernel (csrc/f64.hip); 16 / 32: one launch with that many keypoints per workgroup (default: by launch size); any other
 * mode > 0: 1; mode < 0: back to the default.  Process-wide; the results are bit-identical either way.  Returns the previous value. */
int mdgat_set_f64_layer_fusion(int mode);

/* Which kernel a layer tail or the encoder launch of the exact mode runs (csrc/layer_f64.hip: launch_layer_tail_f64, launch_encoder_f64),
 * and with what grid.  The seven forms:
 *    0 tail, three launches     gemm_f64_kernel three times: q | k | v, mlp.0, mlp.3 + residual (mode 0, or a handle without fragment images)
 *    1 tail<1>                  layer_tail_f64_kernel<1>: one workgroup per 16 rows
 *    2 tail<2>                  layer_tail_f64_kernel<2>: one workgroup per 32 rows
 *    3 tail, clustered          layer_tail_f64_cluster_kernel: four workgroups per 16-row block, clusters in whole groups of eight
 *    4 encoder<1>               encoder_f64_kernel<1>: 16 rows per workgroup
 *    5 encoder<2>               encoder_f64_kernel<2>: 32 rows
 *    6 encoder, seven launches  gemm_f64_kernel once per Conv1d of the two encoders (six, and layer 0's q | k | v)
 * mdgat_layer_f64_plan: the form for a launch of R = B (N + M) keypoint rows; encoder != 0: the encoder launch, otherwise a layer tail;
 * has_hid != 0: the tail has its [R][256] scratch (every tail of a forward has); chained != 0: the launch group is chained, which it is
 * unless its stream is being captured into a graph; mode: as mdgat_set_f64_layer_fusion takes it, negative: the current setting; cus: the
 * device's compute units, <= 0: those of the current device (the only argument that touches one).  32 rows per workgroup when
 * ceil(R / 32) >= 2 cus or mode 32 forces them, 16 otherwise; a tail is clustered when mode is 1, has_hid, chained, and its nblk =
 * ceil(R / 16) blocks satisfy 4 nblk <= cus and nblk <= 256.  *workgroups (optional): the grid - ceil(R / *rows_per_workgroup), or for the
 * clustered form ceil(nblk / 8) * 32, of which 4 nblk find rows; *rows_per_workgroup (optional): 16 or 32.  Both 0 for forms 0 and 6
 * (their grids are the product kernel's: mdgat_gemm_f64_plan) and with -1: nothing is launched (R <= 0).  The launchers take their
 * branch and their grid from the same code.
 * mdgat_layer_f64_launches: counts[i] = layer tails / encoders run in form i by this process so far, on any device and stream (relaxed
 * atomic counters, incremented after a launch that succeeded - forms 0 and 6 once per tail / encoder, after the last of their products -
 * never reset: read them before and after a call and subtract).  The pooled encoder (mdgat_load_pooled_encoder_f64) is none of them. */
#define MDGAT_LAYER_F64_FORMS 7
enum {
    MDGAT_LAYER_F64_TAIL_GEMMS = 0,
    MDGAT_LAYER_F64_TAIL_16 = 1,
    MDGAT_LAYER_F64_TAIL_32 = 2,
    MDGAT_LAYER_F64_TAIL_CLUSTER = 3,
    MDGAT_LAYER_F64_ENCODER_16 = 4,
    MDGAT_LAYER_F64_ENCODER_32 = 5,
    MDGAT_LAYER_F64_ENCODER_GEMMS = 6
};
int mdgat_layer_f64_plan(int R, int encoder, int has_hid, int chained, int mode, int cus, int* workgroups, int* rows_per_workgroup);
void mdgat_layer_f64_launches(uint64_t counts[MDGAT_LAYER_F64_FORMS]);

/* MDGAT_ARITH_FP64: how full attention (models/mdgat.py:190-194) is launched.  -1 (default; MDGAT_F64_ATTENTION_FORM in the
 * environment selects another): by launch size - launches of at least four 128-query workgroups per compute unit (32 pairs of 512
 * keypoints) give every wave 32 queries and all the keys of the frame, smaller ones split the keys of a 16- / 32-query tile over
 * the four waves of a workgroup and combine them through LDS.  The two forms sum a row's terms in different orders: they agree to
 * rounding (1e-15 relative), not bit for bit, so what a pair returns can differ in the last bits with the size of the batch it
 * travels in.  0: always the split-key form - a pair's result is then bit-identical whatever the batch; 1: always one wave per
 * 32 queries; mode < -1: back to the environment's / default.  Process-wide.  Returns the previous value. */
int mdgat_set_f64_attention_form(int mode);

/* fp64 Sinkhorn: -1 (default; MDGAT_F64_SINKHORN_FORM in the environment selects another): the register-resident kernel wherever it
 * holds the frames (<= 575 keypoints), the streaming form beyond; 1: the streaming form at every size (tests, measurements: the two sum
 * in different orders and agree to rounding); anything else: back to the environment's / default.  Process-wide; sizes of workspaces
 * asked for before a change are not valid after it.  Returns the previous value. */
int mdgat_set_f64_sinkhorn_form(int mode);

/* ---- per-op entry points (unit parity; the forward uses the same kernels) ---------------------- */

/* log_optimal_transport + log_sinkhorn_iterations (mdgat.py:279-308): scores [B][N][M] -> Z. */
int mdgat_sinkhorn(int B, int N, int M, const float* scores, float bin_score, int iters,
                   float* Z, void* workspace, size_t workspace_bytes, void* stream);
size_t mdgat_sinkhorn_workspace_bytes(int B, int N, int M);
/* ... followed by the match extraction (mdgat.py:441-483), as the forward's score / Sinkhorn / extraction stage runs it: with the
 * workspace of mdgat_sinkhorn_workspace_bytes (256-byte aligned) the cluster kernel decides the arg-maxes in its epilogue, on the
 * registers it stores to Z, and the extraction kernel merges them; without one the streaming kernel writes Z and the extraction kernel
 * scans it.  Z_or_null: Z [B][N+1][M+1] if wanted (required without a workspace).  Z_fallback_or_null: a buffer of Z's size lent to
 * the cluster launch for pairs it hands to the streaming kernel (scores beyond the scaling form's range, a lost partner workgroup)
 * when Z itself is not asked for - what the forward's workspace provides; with neither the launch is cooperative. */
int mdgat_sinkhorn_extract(int B, int N, int M, const float* scores, float bin_score, int iters, int mode, float match_threshold,
                           int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1, float* Z_or_null,
                           float* Z_fallback_or_null, void* workspace, size_t workspace_bytes, void* stream);

/* Which kernels an fp32 Sinkhorn launch runs (csrc/sinkhorn.hip: launch_sinkhorn, which mdgat_sinkhorn, mdgat_sinkhorn_extract, their
 * ragged entry points - a call with counts - and the fp32-class forward go through), and with what launch parameters.  The
 * instantiations, as mdgat_sinkhorn_launches counts them:
 *    0 scaling<false,4>    sinkhorn_scaling_kernel<false, 4>:  one column slab, <= 4 row slabs (N <= 512, M <= 512)
 *    1 scaling<false,16>   sinkhorn_scaling_kernel<false, 16>: one column slab, 5 .. 16 row slabs (N <= 2048, M <= 512)
 *    2 scaling<true,16>    sinkhorn_scaling_kernel<true, 16>:  2 .. 4 column slabs (M <= 2048, N <= 2048)
 *    3 .. 8   stream<1,16> stream<2,16> stream<4,16> stream<8,16> stream<16,8> stream<32,8>: sinkhorn_kernel<NC, NW> launched on its own,
 *             M <= 64 | 128 | 256 | 512 | 1024 | 2048 (the last two: N <= 4096)
 *    9 .. 12  their RAGGED twins <1,16> .. <8,16> (the ragged entry points; from the padded M alone)
 *   13 gated  a streaming kernel launched behind a cluster launch, gated on its error word and per-pair range flags (which one: the
 *             plan's streaming index)
 *   14 extract  extract_kernel (every caller: the fp32 and fp64 Sinkhorn paths and mdgat_extract)
 * mdgat_sinkhorn_plan: the path - 0 the cluster kernel, 1 the streaming kernel alone, -1 nothing is launched (an empty batch) or the
 * launcher refuses (M > 2048, or N > 4096 with M > 512; more workgroups per pair than `cus`; a ragged slot over
 * MDGAT_RAGGED_FP32_MAX_KEYPOINTS) - for B pairs of N x M on a device of `cus` compute units.  workspace / workspace_bytes: what the call
 * would pass (the address is compared and never dereferenced: NULL, too few bytes for mdgat_sinkhorn_workspace_bytes or an address that
 * is not 256-byte aligned select the streaming kernel); fallback_buffer != 0: a Z is asked for or a buffer is lent (else the cluster launch
 * is cooperative and nothing is launched behind it); ragged != 0: the ragged entry points (no workspace is used).  out (optional):
 * [0] the scaling index (0 .. 2, -1: none), [1] the streaming index (3 .. 12: launched alone on path 1 - counted under it - or gated behind
 * the cluster launch on path 0 - counted under 13; -1: none), [2] GR and [3] GC (row slabs of 128 rows, column slabs of 512 columns: GR * GC
 * workgroups per pair), [4] ngroups (pairs in flight), [5] xcd_map (the partners of a pair placed on one XCD, the grid padded to a multiple
 * of 8 groups), [6] the grid of the first launch, [7] cooperative != 0.  A pure function of its arguments: no device is needed or touched;
 * the launchers take every one of these values from the same code.
 * mdgat_sinkhorn_launches: counts[i] = launches of index i by this process so far, on any device and stream (relaxed atomic counters,
 * never reset: read them before and after a call and subtract). */
#define MDGAT_SINKHORN_COUNTERS 15
#define MDGAT_SINKHORN_PLAN_WORDS 8
int mdgat_sinkhorn_plan(int B, int N, int M, int cus, const void* workspace, size_t workspace_bytes, int fallback_buffer, int ragged,
                        int32_t out[MDGAT_SINKHORN_PLAN_WORDS]);
void mdgat_sinkhorn_launches(uint64_t counts[MDGAT_SINKHORN_COUNTERS]);

/* The same in fp64 - the reference's own arithmetic (mdgat.py:279-308 run in float64, test.py:193) - on fp64 scores: Z [B][N+1][M+1]
 * fp64; N, M <= 2175.  Frames of at most 575 keypoints run in one launch with the couplings held in registers; larger ones stream them
 * from memory, one launch per iteration (csrc/sinkhorn_f64.hip).  workspace: mdgat_sinkhorn_f64_workspace_bytes, 256-byte aligned. */
int mdgat_sinkhorn_f64(int B, int N, int M, const double* scores, double bin_score, int iters,
                       double* Z, void* workspace, size_t workspace_bytes, void* stream);
size_t mdgat_sinkhorn_f64_workspace_bytes(int B, int N, int M);
/* ... followed by the match extraction (mdgat.py:441-483) with every arg-max decided on the fp64 Z (a near tie of 1e-6 between two
 * candidates is below what an fp32 Z resolves); Z_or_null: optional fp32 rounding of Z [B][N+1][M+1]. */
int mdgat_sinkhorn_f64_extract(int B, int N, int M, const double* scores, double bin_score, int iters, int mode, float match_threshold,
                               int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1, float* Z_or_null,
                               void* workspace, size_t workspace_bytes, void* stream);

/* RAGGED batches: B pairs of different sizes in one call.  Pair b has counts0[b] x counts1[b] keypoints and is stored in a slot padded to
 * Np x Mp (scores [B][Np][Mp], Z [B][Np+1][Mp+1], matches0 / mscores0 [B][Np], matches1 / mscores1 [B][Mp]); what the inputs hold beyond a
 * pair's counts is never read.  Pair b's results are those of the pair run alone through the uniform entry above, bit for bit: its block
 * Z[b][0 .. counts0[b]][0 .. counts1[b]] with the dustbin row at row counts0[b] and the dustbin column at column counts1[b], its matches
 * (dustbin = no match), its scores, and the rule of mdgat.py:465-467 (no frame-0 keypoint matched: all scores zero) applied to the pair
 * alone.  Beyond a pair's counts the outputs are fixed: the rest of its Z slot 0, matches -1, scores 0.
 * Np, Mp <= 575 (the register-resident form; else MDGAT_ERR_UNSUPPORTED, as under mdgat_set_f64_sinkhorn_form(1)); then the counts are
 * checked as described at THE COUNTS OF A RAGGED BATCH.  workspace:
 * mdgat_sinkhorn_f64_ragged_workspace_bytes, 256-byte aligned.  Unlike their uniform siblings these two entries hand the kernel an error
 * word and read it back: they SYNCHRONISE `stream` before they return, and return MDGAT_ERR_HIP instead of numbers when a workgroup gave
 * up waiting for its partners. */
size_t mdgat_sinkhorn_f64_ragged_workspace_bytes(int B, int Np, int Mp);
int mdgat_sinkhorn_f64_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                              const int32_t* counts1_host, const double* scores, double bin_score, int iters, double* Z, void* workspace,
                              size_t workspace_bytes, void* stream);
int mdgat_sinkhorn_f64_extract_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                      const int32_t* counts1_host, const double* scores, double bin_score, int iters, int mode,
                                      float match_threshold, int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                                      float* Z_or_null, void* workspace, size_t workspace_bytes, void* stream);

/* The two entries above on the STREAMING form of the fp64 Sinkhorn (K in memory, one launch per iteration), whose kernels take the counts
 * as well: the same arguments, layout and fixed outputs beyond the counts, in slots of up to 2175 keypoints - Np, Mp <= 2175, else
 * MDGAT_ERR_UNSUPPORTED with "<entry>: padded sizes Np x Mp: the streaming form holds at most 2175 keypoints per frame".  They ALWAYS run
 * the streaming form, small slots included, whatever mdgat_set_f64_sinkhorn_form says.  Pair b's results are those of the pair run alone
 * through the uniform entry under mdgat_set_f64_sinkhorn_form(1), bit for bit; against the pair alone on the register-resident form they
 * agree to fp64 rounding (the two forms sum in different orders).  A pair works on its own extent only - row slabs 0 .. ceil(n / 32) - 1,
 * column chunks 0 .. ceil((m + 1) / 128) - 1 - so small pairs in large slots cost what they cost alone, not what the slot costs.
 * No workgroup of this form waits for another: there is no error word, and the entries are ASYNCHRONOUS like their uniform siblings.  The
 * counts are checked as described at THE COUNTS OF A RAGGED BATCH before anything is enqueued.  workspace:
 * mdgat_sinkhorn_f64_stream_ragged_workspace_bytes (0 for an unsupported slot), 256-byte aligned.  It is carved by the SLOT: K is
 * [B][Np][Mp rounded up to 128] doubles whatever the pairs' own sizes - 35.6 MB per pair in slots of 2048, 570 MB for 16 pairs. */
size_t mdgat_sinkhorn_f64_stream_ragged_workspace_bytes(int B, int Np, int Mp);
int mdgat_sinkhorn_f64_stream_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                     const int32_t* counts1_host, const double* scores, double bin_score, int iters, double* Z, void* workspace,
                                     size_t workspace_bytes, void* stream);
int mdgat_sinkhorn_f64_extract_stream_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                             const int32_t* counts1_host, const double* scores, double bin_score, int iters, int mode,
                                             float match_threshold, int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                                             float* Z_or_null, void* workspace, size_t workspace_bytes, void* stream);

/* Which kernels a call of the fp64 Sinkhorn runs (csrc/sinkhorn_f64.hip: launch_sinkhorn_f64, which the six entries above and the
 * exact mode's forward go through, and sinkhorn_f64_stream_history, the forward pass of mdgat_sinkhorn_backward).  The eleven forms:
 *    0 resident                   sinkhorn_f64_kernel<8, false>: one launch, the couplings in registers (N <= 576, M <= 575)
 *    1 resident, ragged           sinkhorn_f64_kernel<8, true>: the same with per-pair counts (slots <= 575 x 575)
 *    2, 3, 4 streaming            sinkhorn_f64_wide_iter_kernel / _final_kernel<NC2, false>, NC2 = 5, 9, 17: one launch per iteration and
 *                                 a last one; NC2 column pairs per lane hold ceil((M + 1) / 128) = 1 .. 5, 6 .. 9, 10 .. 17 chunks of 128
 *                                 columns (M <= 639, 1151, 2175; N <= 2175)
 *    5, 6, 7 streaming, ragged    the <NC2, true> instantiations, NC2 from the SLOT's chunk count whatever the pairs' own
 *    8, 9, 10 history             the <NC2, false> iteration launches with the potential history written and no last launch (the backward)
 * mdgat_sinkhorn_f64_plan: the form a call in slots of N x M keypoints runs.  ragged != 0: a call with counts, following ragged_mode as
 * mdgat_set_ragged_sinkhorn takes it (the ragged entries above run mode 0, the stream_ragged ones mode 2); form: -1 or 1 as
 * mdgat_set_f64_sinkhorn_form takes them, any other value: the current setting; history != 0: the backward's history run (a uniform
 * call; it streams at every size, whatever `form`).  *slabs (optional): the row slabs of 32 rows, ceil(N / 32); *chunks (optional): the
 * chunks of 128 columns that hold M + 1 columns, (M + 1 + 127) >> 7, for the streaming forms, 0 for the resident ones.  Negative, with
 * both 0: no form holds the call (N or M beyond 2175 or below 1; a ragged call under mode 0 beyond 575 or under form 1), or history
 * with ragged.  A pure function of its arguments and that setting: no device is needed or touched; the launchers take their branch from
 * the same code.
 * mdgat_sinkhorn_f64_launches: counts[i] = calls run in form i by this process so far, on any device and stream (relaxed atomic
 * counters, incremented once per call after its last launch succeeded - the column merge where arg-maxes are asked for, not the match
 * extraction behind it - never reset: read them before and after a call and subtract). */
#define MDGAT_SINKHORN_F64_FORMS 11
enum {
    MDGAT_SINKHORN_F64_RESIDENT = 0,
    MDGAT_SINKHORN_F64_RESIDENT_RAGGED = 1,
    MDGAT_SINKHORN_F64_STREAM_5 = 2,
    MDGAT_SINKHORN_F64_STREAM_9 = 3,
    MDGAT_SINKHORN_F64_STREAM_17 = 4,
    MDGAT_SINKHORN_F64_STREAM_RAGGED_5 = 5,
    MDGAT_SINKHORN_F64_STREAM_RAGGED_9 = 6,
    MDGAT_SINKHORN_F64_STREAM_RAGGED_17 = 7,
    MDGAT_SINKHORN_F64_HISTORY_5 = 8,
    MDGAT_SINKHORN_F64_HISTORY_9 = 9,
    MDGAT_SINKHORN_F64_HISTORY_17 = 10
};
int mdgat_sinkhorn_f64_plan(int N, int M, int ragged, int ragged_mode, int form, int history, int* slabs, int* chunks);
void mdgat_sinkhorn_f64_launches(uint64_t counts[MDGAT_SINKHORN_F64_FORMS]);

/* RAGGED batches in fp32: mdgat_sinkhorn / mdgat_sinkhorn_extract on pairs of different sizes, laid out as above with fp32 scores and Z.
 * They run the one-workgroup-per-pair streaming kernel (the cluster kernel takes no counts), whose ragged instantiation is picked from the
 * padded sizes alone: pair b's block of Z, its matches and its scores are those of the pair run alone through the uniform entry WITHOUT a
 * workspace (the streaming kernel), bit for bit, whatever its position and companions; the rule of mdgat.py:465-467 is applied to the pair
 * alone; beyond its counts the rest of its Z slot is 0, matches -1, scores 0, and what scores holds there is never read.
 * Np, Mp <= MDGAT_RAGGED_FP32_MAX_KEYPOINTS (else MDGAT_ERR_UNSUPPORTED); then the counts are checked as described at THE COUNTS OF A RAGGED
 * BATCH.  No synchronisation.  The extraction scans Z: Z_or_null, or - when the caller wants none - a Z produced into `workspace`
 * (mdgat_sinkhorn_ragged_workspace_bytes, 256-byte aligned; not needed with Z). */
size_t mdgat_sinkhorn_ragged_workspace_bytes(int B, int Np, int Mp);
int mdgat_sinkhorn_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                          const int32_t* counts1_host, const float* scores, float bin_score, int iters, float* Z, void* stream);
int mdgat_sinkhorn_extract_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                  const int32_t* counts1_host, const float* scores, float bin_score, int iters, int mode,
                                  float match_threshold, int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                                  float* Z_or_null, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of log_optimal_transport (mdgat.py:279-308) in fp64: given scores [B][N][M] fp64, the bin score and dZ = dL/dZ
 * [B][N+1][M+1] fp64 (contiguous), writes dscores [B][N][M] and dbin [B] (the bin score's gradient PER PAIR: the sum of dL/dC over
 * the pair's dustbin row and column; a caller with one shared bin score sums them).  N, M <= 2175 (else MDGAT_ERR_UNSUPPORTED),
 * iters >= 0 (0: dscores = dZ[:, :N, :M]), B >= 0.  The forward's potentials are recomputed (the streaming fp64 iterations with their
 * history kept), then T reverse iterations and one fp64 GEMM (csrc/sinkhorn_grad.hip).  A pair's result does not depend on the
 * batch it travels in.  workspace: mdgat_sinkhorn_backward_workspace_bytes, 256-byte aligned (about 8 (B N (M + 128) + 2 T B
 * (N + M + 192)) bytes).  Asynchronous on `stream`. */
int mdgat_sinkhorn_backward(int B, int N, int M, const double* scores, double bin_score, int iters, const double* dZ, double* dscores,
                            double* dbin, void* workspace, size_t workspace_bytes, void* stream);
size_t mdgat_sinkhorn_backward_workspace_bytes(int B, int N, int M, int iters);

/* The matching head (mdgat.py:397 final_proj = Conv1d(128, 128, 1) with one weight for both frames, 430-431 the score matrix) in
 * fp64 as a call of its own: desc0 [B][N][128], desc1 [B][M][128] (point-major: the GNN's output descriptors, the reference's
 * [B][128][N] transposed), W [128 out][128 in], bias [128] -> scores [B][N][M] = (desc0 W^T + b)(desc1 W^T + b)^T / sqrt(128).  The
 * launches are the exact mode's (mdgat_forward_f64): the fp64 GEMM for final_proj - once per frame, the frames being separate arrays
 * here - then the batched product with scale 1 / sqrt(128); the values are the exact mode's scores.  N, M <= 2175 (else
 * MDGAT_ERR_UNSUPPORTED), B >= 0 (0: nothing is done).  workspace: mdgat_match_head_workspace_bytes, 256-byte aligned.  Asynchronous
 * on `stream`. */
int mdgat_match_head_f64(int B, int N, int M, const double* desc0, const double* desc1, const double* W, const double* bias,
                         double* scores, void* workspace, size_t workspace_bytes, void* stream);
/* Backward of the matching head in fp64: given the forward's inputs and dscores = dL/dscores [B][N][M] (contiguous), writes ddesc0
 * [B][N][128], ddesc1 [B][M][128], dW [128][128] and dbias [128] - the sums over every point of every pair and both frames.  Each of
 * the four may be NULL when the caller does not need it; with all four NULL, or B == 0, nothing is launched and nothing written.
 * The projections are recomputed (the forward's launches), then dmd = s dscores md on fp64 matrix instructions with dscores read once
 * per frame, ddesc = dmd W from the tile on chip, per-pair partials of dW / dbias, and their sum in pair order from pair 0's
 * (csrc/head_grad.hip).  No atomics on values: the result is the same bit for bit from run to run, ddesc of a pair does not depend
 * on the batch it travels in, and for B = 2 dW equals dW(pair 0 alone) + dW(pair 1 alone) exactly.  N, M <= 2175 (else
 * MDGAT_ERR_UNSUPPORTED), B >= 0.  workspace: mdgat_match_head_workspace_bytes, 256-byte aligned (about 8 B (256 (N + M) + 16512)
 * bytes).  Asynchronous on `stream`. */
int mdgat_match_head_backward(int B, int N, int M, const double* desc0, const double* desc1, const double* W, const double* bias,
                              const double* dscores, double* ddesc0, double* ddesc1, double* dW, double* dbias,
                              void* workspace, size_t workspace_bytes, void* stream);
size_t mdgat_match_head_workspace_bytes(int B, int N, int M);      /* both calls; 0 for a shape they refuse */

/* The reference's MLP(channels) (mdgat.py:34-46) in fp64 with BatchNorm on the batch's own statistics, and its backward
 * (csrc/mlp_grad.hip): n_conv Conv1d(k=1), each but the last followed by BatchNorm1d and ReLU.  Rows are points: x0 [R][K0] and the
 * optional second source x1 [R][K1] are read side by side (the layer's cat([x, message]) is never materialised), the output is
 * [R][C[n_conv - 1]].  W[l] is [C[l]][C_in] row-major as in the state_dict (C_in = K0 + K1 for l = 0, else C[l - 1]), bias[l] [C[l]];
 * gamma / beta / running_mean / running_var [l] are [C[l]] and num_batches_tracked[l] one int64, all on the device, for
 * l < n_conv - 1.  No alignment beyond 8 bytes is assumed of any of them.  Supported (else MDGAT_ERR_UNSUPPORTED): 1 to 4
 * convolutions, every C[l] a multiple of 16 and at most 512, 1 <= K0 + K1 <= 512.  R >= 0 (0: nothing is launched); R == 1 with
 * training != 0 and a BatchNorm in the stack is MDGAT_ERR_BAD_ARG, as in torch. */
#define MDGAT_MLP_MAX_CONVS 4
typedef struct {
    int32_t n_conv;
    int32_t R, K0, K1;
    int32_t C[MDGAT_MLP_MAX_CONVS];
    int32_t training;                                  /* != 0: batch statistics, the running buffers move; 0: the running buffers are read */
    double eps[MDGAT_MLP_MAX_CONVS - 1], momentum[MDGAT_MLP_MAX_CONVS - 1];
    const double* W[MDGAT_MLP_MAX_CONVS];
    const double* bias[MDGAT_MLP_MAX_CONVS];
    const double* gamma[MDGAT_MLP_MAX_CONVS - 1];
    const double* beta[MDGAT_MLP_MAX_CONVS - 1];
    double* running_mean[MDGAT_MLP_MAX_CONVS - 1];
    double* running_var[MDGAT_MLP_MAX_CONVS - 1];
    int64_t* num_batches_tracked[MDGAT_MLP_MAX_CONVS - 1];
} mdgat_mlp_desc;
/* the gradients the backward writes; NULL: not wanted, and a product only it needs is not formed */
typedef struct {
    double *dx0, *dx1;                                 /* [R][K0], [R][K1] */
    double* dW[MDGAT_MLP_MAX_CONVS];
    double* dbias[MDGAT_MLP_MAX_CONVS];
    double* dgamma[MDGAT_MLP_MAX_CONVS - 1];
    double* dbeta[MDGAT_MLP_MAX_CONVS - 1];
} mdgat_mlp_grads;
/* Forward.  Y_l = A_{l-1} W_l^T + b_l; per channel the mean and the biased variance over the R rows - per-row-block sum and centred
 * M2, combined in block order by Chan's update, never E[y^2] - E[y]^2 - z = gamma (Y - mean) / sqrt(var + eps) + beta, A_l = max(z, 0).
 * With training != 0 the same call moves running_mean = (1 - m) rm + m mean, running_var = (1 - m) rv + m var R / (R - 1) and adds 1
 * to num_batches_tracked; with training == 0 the running statistics stand in for the batch's and are left alone.  `saved`
 * (mdgat_mlp_workspace_bytes(d, 0), 256-byte aligned) receives what the backward needs beside the inputs: the pre-BN Y_l of every BN
 * layer and mean / invstd per channel.  A_l is never stored: the normalisation and the ReLU are applied where the next product
 * loads its A operand.  Asynchronous on `stream`. */
int mdgat_mlp_forward_f64(const mdgat_mlp_desc* d, const double* x0, const double* x1, double* out, void* saved, size_t saved_bytes,
                          void* stream);
/* The same forward with out = Y_L + residual: residual [R][C[n_conv - 1]] (contiguous, not NULL; may alias out) is added in the last
 * product's epilogue - the layer's desc + delta (mdgat.py:274) and the encoders' denc(...) + kenc(...) (392-393) without a launch of
 * their own.  `saved` is what mdgat_mlp_forward_f64 leaves; the backward is mdgat_mlp_backward_f64 unchanged, and dout is the
 * residual's gradient as it stands. */
int mdgat_mlp_forward_residual_f64(const mdgat_mlp_desc* d, const double* x0, const double* x1, const double* residual, double* out,
                                   void* saved, size_t saved_bytes, void* stream);
/* Backward: the forward's descriptor, inputs and `saved` (with its size), and dout = dL/dout [R][C[n_conv - 1]] (contiguous).  From the last
 * convolution to the first: db = colsum(dY), dW = dY^T A, dA = dY W, dz = dA [z > 0] (zero is not positive), dbeta = colsum(dz),
 * dgamma = colsum(dz yhat), dY = gamma invstd (dz - dbeta / R - yhat dgamma / R) (training == 0: gamma invstd dz).  The sums over the
 * rows run as one chain per element inside a slab of rows (512 for dW / db, 256 for dgamma / dbeta); the slabs' partials are added
 * in slab order by a closing launch.  No atomics on values and no workgroup waits for another: two runs give the same bits.  The
 * walk stops below the lowest gradient that is wanted.  workspace: mdgat_mlp_workspace_bytes(d, 1), 256-byte aligned.
 * Asynchronous on `stream`. */
int mdgat_mlp_backward_f64(const mdgat_mlp_desc* d, const double* x0, const double* x1, const void* saved, size_t saved_bytes,
                           const double* dout, const mdgat_mlp_grads* grads, void* workspace, size_t workspace_bytes, void* stream);
/* part 0: the forward's `saved`; part 1: the backward's workspace.  0 for a descriptor the calls refuse (and for R == 0) */
size_t mdgat_mlp_workspace_bytes(const mdgat_mlp_desc* d, int part);

/* The frame maximum of the pooled descriptor encoder as a call of its own (the training path: ops.frame_max_f64).  e [B][n][128] fp64 ->
 * g [B][128] = max over the n rows, idx [B][128] (optional) the FIRST row that holds it.  The backward writes dg [B][128] to row idx of
 * de [B][n][128] and zero elsewhere: the indices are the forward's, never decided again; one writer per element, no atomics. */
int mdgat_frame_max_f64(int B, int n, const double* e, double* g, int64_t* idx, void* stream);
int mdgat_frame_max_backward_f64(int B, int n, const double* dg, const int64_t* idx, double* de, void* stream);

/* match extraction (mdgat.py:441-483) from Z [B][N+1][M+1]. */
int mdgat_extract(int B, int N, int M, const float* Z, int mode, float match_threshold,
                  int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                  void* stream);

/* attention / dynamic_attention (mdgat.py:190-210) on projected q/k/v in the library layout
 * [B][P][3][4][32]; `cross` selects the other frame as source (mdgat.py:263-266); topk 0 = full.
 * msg [B][P][128] with channel = head*32 + dim.  The kernel consumes q/k/v as split-f16 operands
 * (DESIGN.md section 3); this entry point converts the fp32 input into `workspace` first (16-byte
 * aligned, mdgat_attention_workspace_bytes), the forward writes that layout from its projection. */
int mdgat_attention(int B, int N, int M, int cross, int topk, const float* qkv, float* msg,
                    void* workspace, size_t workspace_bytes, void* stream);
size_t mdgat_attention_workspace_bytes(int B, int N, int M);
/* The same, also returning the kept keys of a dynamic layer (topk > 0) in sel [mdgat_topk_sel_words(B, N, M)]
 * (layout as mdgat_taps.topk_sel). */
int mdgat_attention_sel(int B, int N, int M, int cross, int topk, const float* qkv, float* msg, uint32_t* sel,
                        void* workspace, size_t workspace_bytes, void* stream);
/* mdgat_attention_sel on a RAGGED batch: pair b has counts0[b] / counts1[b] keypoints in slots padded to Np / Mp (qkv [B][Np+Mp][384], frame 1
 * from row Np of a pair; msg and sel laid out for Np, Mp; sel may be NULL).  Pair b's rows depend on its own q/k/v rows alone - not on its
 * position, its companions or what the slots hold beyond its counts, which no result sees - and are bit-identical in every batch with the
 * same slots; message rows and masks beyond its counts are zero.  A dynamic layer keeps exactly topk keys per row, all inside the pair's counts
 * (every key where the source frame has just topk of them).  The instantiation follows the slots alone (never a count): indices 1, 2 for full
 * attention (<= 128 / <= 512 keys per slot), 4, 5, 6 (11, 12, 13 with sel) for a dynamic layer, which mdgat_attention_launches counts as for a
 * uniform launch; the stream, topk16, windowed and wide kernels take no counts.  Np, Mp <= MDGAT_RAGGED_FP32_MAX_KEYPOINTS (else
 * MDGAT_ERR_UNSUPPORTED); then the counts are checked as described at THE COUNTS OF A RAGGED BATCH, against topk.  workspace:
 * mdgat_attention_workspace_bytes(B, Np, Mp). */
int mdgat_attention_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                           const int32_t* counts1_host, int cross, int topk, const float* qkv, float* msg, uint32_t* sel,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Which kernel an attention launch of the fp32 class runs (csrc/attention.hip: launch_attention, which mdgat_attention, mdgat_attention_sel
 * and every layer of the fp32-class forward go through), and with what launch geometry.  The instantiations it can reach:
 *    0 stream              full attention, both frames multiples of 64 keys (attention_stream_kernel<false>)
 *    1 full<4>             attention_kernel<false, 4, false>: full, <= 128 keys                     (tiles of 256 queries)
 *    2 full<8>             attention_kernel<false, 8, false>: full, <= 512 keys                     (256)
 *    3 full<8,windowed>    attention_kernel<false, 8, true>:  full, > 512 keys, a 512-key window    (256)
 *    4 dyn<4>              attention_kernel<true, 4, false>:  top-k, <= 128 keys                    (256)
 *    5 dyn<8>              attention_kernel<true, 8, false>:  top-k, <= 256 keys                    (256)
 *    6 dyn<16>             attention_kernel<true, 16, false>: top-k, <= 512 keys                    (128)
 *    7 topk16<256>         attention_topk16_kernel<false, false, 256>: top-k, 256 x 256             (16)
 *    8 topk16<512>         attention_topk16_kernel<false, false, 512>: top-k, 512 x 512             (16)
 *    9 wide<4>             attention_topk_wide_kernel<4>: top-k, <= 1024 keys                       (64 per pass)
 *   10 wide<8>             attention_topk_wide_kernel<8>: top-k, <= 2048 keys                       (32 per pass)
 *   11 .. 17               the TAP twins of 4 .. 10 (a selection buffer is passed: index + 7)
 *   18 stream,FAST         19 topk16<256>,FAST      20 topk16<512>,FAST      21, 22 the TAP twins of 19, 20
 *                          (mode MDGAT_ATTENTION_F16; the other kernels have no FAST form: mode 1 launches the index mode 0 does)
 * mdgat_attention_plan: the index for B pairs of N x M keypoints, `topk` (0: full), tap != 0: a selection buffer is passed, mode: an
 * mdgat_attention_mode.  -1: nothing is launched (an empty batch) or the launcher refuses (topk < 0, topk > min(N, M), top-k over more
 * than 2048 keys).  *split (optional): the workgroups that share the query tiles of one (pair, frame, head) - gridDim.x of
 * attention_kernel, the grid_split of the 16-query and wide kernels, the tile count of the streamed one.  *tiles (optional): the most
 * query tiles (wide kernels: passes) one workgroup walks, ceil(tiles of the larger frame / split).  Both 0 with -1.  A pure function of
 * its arguments: no device is needed or touched; launch_attention takes its branch and its split from the same code.
 * mdgat_attention_ragged_plan: the same for a ragged batch in slots of Np x Mp (mdgat_attention_ragged; wide != 0: mdgat_attention_ragged_wide,
 * include/mdgat_hip_wide.h; a layer of mdgat_forward_ragged).  The index is the uniform sibling's, the kernel its RAGGED instantiation: from
 * the slots alone - never B or a count - one of 1, 2, 4 .. 6 and 11 .. 13, and beyond 512 keypoints (wide only) 3, 9, 10, 16 or 17; never the stream or
 * topk16 kernels, which take no counts.  Any topk > 0 is a dynamic layer; the split and the tiles are the uniform launch's for the slots.
 * -1: an empty batch, or the launcher refuses (topk < 0, a slot beyond 512 keypoints, with wide beyond 2048).
 * mdgat_attention_launches: counts[i] = launches of instantiation i by this process so far, on any device and stream (relaxed atomic
 * counters, never reset: read them before and after a call and subtract). */
#define MDGAT_ATTENTION_FORMS 23
int mdgat_attention_plan(int B, int N, int M, int topk, int tap, int mode, int* split, int* tiles);
int mdgat_attention_ragged_plan(int B, int Np, int Mp, int topk, int tap, int wide, int* split, int* tiles);
void mdgat_attention_launches(uint64_t counts[MDGAT_ATTENTION_FORMS]);

/* Measurement only (bench.py, roofline_qk): the Q K^T contraction of the streamed full-attention kernel in isolation -
 * the same chunk ring, LDS reads and split-f16 MFMA sequence as mdgat_attention, without V^T traffic, softmax and P.V.
 * msg [B][P][128]: element [p][head * 32] receives the row maximum of the base-2 logits, the rest is left alone.
 * N and M must be multiples of 64.  Not part of the matching path (mdgat.py:192 is its subject). */
int mdgat_attention_qk_probe(int B, int N, int M, int cross, const float* qkv, float* msg,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Measurement only (bench.py, roofline_qk.standalone_*): the same Q K^T phase as a standalone kernel with nq_sets = 1 (32
 * queries per wave, the shipped arrangement) or 2 (64 queries per wave: every K fragment read from LDS feeds two sets of
 * products) - the lever VERDICT r2 names; the full kernel cannot hold the registers for it.  Arguments
 * and output as mdgat_attention_qk_probe.  Not part of the matching path. */
int mdgat_attention_qk_probe_sets(int B, int N, int M, int cross, int nq_sets, const float* qkv, float* msg,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* Measurement only (bench.py, roofline.sustained_*): the rate this device SUSTAINS on v_mfma_f32_16x16x32_f16 with random
 * operands resident in registers (two waves per SIMD, nothing but MFMAs, one workgroup pair per CU, `reps` x 24 MFMAs per
 * wave) - the chip clocks to its power budget under such a load, well below the 2.4 GHz the dense peak is quoted at.
 * workspace: >= 136 KB of device memory, 256-byte aligned.  ms_out: duration of the timed launch (HIP events on `stream`, synchronises),
 * flops_out: FLOPs it executed, ticks_out: shader cycles (s_memtime) one wave spent in its loop.  Not part of the
 * matching path; replaces nothing in the reference. */
int mdgat_mfma_probe(int reps, void* workspace, size_t workspace_bytes, float* ms_out, double* flops_out,
                     long long* ticks_out, void* stream);

/* Measurement only (bench.py, exact_mode.roofline): the rate this device sustains on v_mfma_f64_16x16x4_f64 (two waves per
 * SIMD, operands in registers, `reps` x 16 instructions per wave).  workspace: >= 72 KB, 256-byte aligned.  Outputs as
 * mdgat_mfma_probe.  Not part of the matching path. */
int mdgat_mfma_f64_probe(int reps, void* workspace, size_t workspace_bytes, float* ms_out, double* flops_out,
                         long long* ticks_out, void* stream);

/* Unit parity of the fp64 kernels (csrc/f64.hip; the fp64 forward uses the same launches):
 * mdgat_pointwise_f64: as mdgat_pointwise on doubles, no alignment or K granularity required.
 * mdgat_attention_f64: attention / dynamic_attention (mdgat.py:190-210) on fp64 q | k | v rows [B][P][384] ([which][head][dim]),
 * msg [B][P][128]; sel (optional): the kept keys of a dynamic layer, layout of mdgat_taps.topk_sel. */
int mdgat_pointwise_f64(int M, int N, int K, const double* A, int lda, const double* W, int ldw, const double* bias,
                        int relu, const double* R, int ldr, double* C, int ldc, void* stream);
int mdgat_attention_f64(int B, int N, int M, int cross, int topk, const double* qkv, double* msg, uint32_t* sel, void* stream);
/* Which kernel a product of the fp64 path runs (csrc/f64.hip: gemm_f64_kernel carries every Conv1d(k=1) of the exact mode and every
 * product of the training path, mdgat_pointwise_f64 included).  It exists in ten instantiations, numbered 5 * bnt + form:
 *   form 0: 64 x 64 tiles, guarded 8-byte copies, chunks of 32 (any shape, stride and 8-byte alignment)
 *   form 1: 64 x 64 tiles, whole-tile 16-byte copies, chunks of 32      form 2: the same with chunks of 64
 *   form 3: 64 x 128 tiles, guarded copies                              form 4: 64 x 128 tiles, whole-tile copies
 *   bnt: the A operand is max(a (y - mean) + beta, 0) of what is loaded (the training-mode MLP's products behind a BatchNorm).
 * mdgat_gemm_f64_plan: the index the launcher chooses for C [M][N] = A [M][K] W [N][K]^T whose first K0 columns come from the first
 * source (K0 >= K: one source), `batch` independent products, on a device of `cus` compute units.  aligned != 0: every condition the
 * whole-tile copies put on the operands holds - A, W (and the second source) 16-byte aligned, their leading dimensions (and batch
 * strides) even.  A pure function of its arguments: no device is needed or touched.  -1: no launch (an empty product, or bnt with
 * two sources, which the launcher refuses).
 * mdgat_gemm_f64_launches: counts[i] = launches of instantiation i by this process so far, on any device and stream (relaxed atomic
 * counters, never reset: read them before and after a call and subtract). */
int mdgat_gemm_f64_plan(int M, int N, int K, int K0, int batch, int aligned, int bnt, int cus);
void mdgat_gemm_f64_launches(uint64_t counts[10]);
/* Which kernel mdgat_attention_f64 / mdgat_attention_f64_ragged (and every attention of the exact mode) runs.  attention_f64_kernel exists
 * in seven instantiations:
 *   0: full attention, 16 queries per workgroup      1: full attention, 32 queries per workgroup
 *   2: dynamic attention, at most 512 keys (the fp64 logits stay in registers), writing the selection words      3: the same without them
 *   4: dynamic attention beyond 512 keys (the logits are recomputed), writing the selection words               5: the same without them
 *   6: full attention, one wave per 32 queries
 * mdgat_attention_f64_plan: the index the launcher chooses for B pairs in slots of N x M keypoints, top-k `topk` (0: full attention),
 * tap != 0: selection words are asked for, ragged != 0: per-pair counts are given, the smallest of them `cnt_min` (ignored otherwise),
 * `form` as mdgat_set_f64_attention_form takes it (-1 by launch size, 0, 1), on a device of `cus` compute units.  topk == N == M is full
 * attention unless ragged.  A pure function of its arguments: no device is needed or touched.  Negative: no launch - -1 an empty one,
 * -2 / -3 what the launcher refuses (k above the smallest key count or bad counts / more than 2048 keys in a dynamic layer).
 * mdgat_attention_f64_geometry: the same index, and the launch it stands for: the queries of a workgroup (16, 32, or 128 where a wave owns 32),
 * the query tiles of a (pair, frame, head) = ceil(max(N, M) / queries), the grid = 8 * tiles * B workgroups of 256 threads (eight (frame, head) units per pair), and
 * the launch's dynamic LDS bytes.  Each output may be null; all are 0 where nothing is launched.
 * mdgat_attention_f64_launches: counts[i] = launches of instantiation i by this process so far, on any device and stream (relaxed atomic
 * counters, never reset: read them before and after a call and subtract). */
#define MDGAT_ATTENTION_F64_FORMS 7
int mdgat_attention_f64_plan(int B, int N, int M, int topk, int tap, int ragged, int cnt_min, int form, int cus);
int mdgat_attention_f64_geometry(int B, int N, int M, int topk, int tap, int ragged, int cnt_min, int form, int cus, int* queries, int* tiles,
                                 int* workgroups, size_t* lds_bytes);
void mdgat_attention_f64_launches(uint64_t counts[MDGAT_ATTENTION_F64_FORMS]);
/* The same on a RAGGED batch: pair b has counts0[b] / counts1[b] keypoints in slots padded to Np / Mp (qkv [B][Np+Mp][384], frame 1 from row
 * Np on; msg and sel likewise, sel with the words of mdgat_topk_sel_words(B, Np, Mp)).  Queries and keys beyond a pair's counts take no part
 * and are never read; their message rows and selection words are zero.  A pair's rows are those of mdgat_attention_f64 on the pair alone -
 * bit for bit where both launches run the same kernel form (mdgat_set_f64_attention_form(0), and the larger frame of both launches on the
 * same side of 512 keys for a dynamic layer), to rounding otherwise; the kept keys are the same always.  topk > 0 runs the dynamic kernel
 * also where k equals a pair's key count.  The counts are checked as described at THE COUNTS OF A RAGGED BATCH, against topk. */
int mdgat_attention_f64_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                               const int32_t* counts1_host, int cross, int topk, const double* qkv, double* msg, uint32_t* sel, void* stream);

/* Backward of mdgat_attention_f64 (csrc/attention_grad.hip): given the forward's qkv [B][N+M][384], its selection words `sel` (the
 * `sel` output of the forward, layout of mdgat_taps.topk_sel; required when topk > 0, ignored when topk == 0) and dmsg = dL/dmsg
 * [B][N+M][128] (channel = head * 32 + dim), writes dqkv [B][N+M][384].  The top-k selection is not differentiated and not decided
 * again: a key the forward did not keep has a probability of exactly 0.0 and sends exactly 0.0 to dk / dv.  `cross` as in the forward:
 * the queries of frame 0 read the keys and values of frame 1 and vice versa, so the rows of frame 0 receive dq from their own queries
 * and dk / dv from frame 1's.  Two launches on fp64 matrix instructions: a row pass (per 64 queries: the row's log-sum-exp and
 * D = sum_j P dP to the workspace, dq) and a column pass (per 64 keys: dk, dv).  No atomics on values: every element of dqkv is
 * written exactly once and its terms are added in a fixed order, so the result is the same bit for bit from run to run and a pair's
 * dqkv does not depend on the batch it travels in.  N, M <= 2048 and B (N + M) <= 2^24 rows (else MDGAT_ERR_UNSUPPORTED), 0 <= topk <= min(N, M), B >= 0
 * (0: nothing is launched, nothing written).  topk > 0 with sel == NULL, or a workspace smaller than
 * mdgat_attention_backward_workspace_bytes (16 bytes per pair, head and point) or not 256-byte aligned: MDGAT_ERR_BAD_ARG.
 * Asynchronous on `stream`. */
int mdgat_attention_backward_f64(int B, int N, int M, int cross, int topk, const double* qkv, const uint32_t* sel, const double* dmsg,
                                 double* dqkv, void* workspace, size_t workspace_bytes, void* stream);
size_t mdgat_attention_backward_workspace_bytes(int B, int N, int M);      /* 0 for a shape the call refuses */

/* Conv1d(k=1)(+folded BN)(+ReLU) over points: C[m][n] = act(sum_k A[m][k] W[n][k] + bias[n]) (+R).
 * (MLP of mdgat.py:34-46 after folding.)  K must be a multiple of 32; lda/ldw/ldc multiples of 4. */
int mdgat_pointwise(int M, int N, int K, const float* A, int lda, const float* W, int ldw,
                    const float* bias, int relu, const float* R, int ldr, float* C, int ldc,
                    void* stream);

/* knn() / get_graph_feature() (mdgat.py:8-32; dead code there, named by the north star):
 * x [B][N][C], src [B][M][C] (point-major) -> idx int64 [B][N][k] in topk order (nearest first; exact ties in the
 * order of their indices), and, if adj != NULL, the dense 0/1 int64 adjacency [B][N][M].  Any M; k <= 1024.
 * C == 128 (feature space) runs the inner products on the matrix cores when `workspace` holds
 * mdgat_knn_workspace_bytes(B, C, N, M) bytes (16-byte aligned; the N x M matrix of 2 x.s - |s|^2); other channel
 * counts - or workspace == NULL - compute -sum (x - s)^2 inside the selection kernel and need none. */
int mdgat_knn(int B, int C, int N, int M, int k, const float* x, const float* src, int64_t* idx,
              int64_t* adj, void* workspace, size_t workspace_bytes, void* stream);
size_t mdgat_knn_workspace_bytes(int B, int C, int N, int M);

/* ---- the steps either side of the matcher, fp64 like the reference's numpy ---------- */

/* Pose from matches, per pair: solve_icp (utils/utils_test.py:73-110: centroids, cross covariance, SVD,
 * R = U V^T without reflection fix) on {kpts0[i], kpts1[matches0[i]] : matches0[i] >= 0}, as test.py:213-216
 * selects them; T [B][4][4] maps frame-1 points onto frame 0.  stats [B][5] = number of matches, inliers
 * (|T p1 - p0| < inlier_dist, utils_test.py:55-63), inlier ratio, and - when T_gt [B][4][4] is given -
 * translation / rotation error of inv(T) T_gt (utils_test.py:65-70; the arccos is not clamped there either). */
int mdgat_pose(int B, int N, int M, const float* kpts0, const float* kpts1, const int64_t* matches0,
               const double* T_gt, double inlier_dist, double* T, double* stats, void* stream);

/* Ground-truth matches of SparseDataset.__getitem__ (load_data.py:238-285): nearest neighbours of the
 * world-frame keypoints (T0/T1 [B][4][4] = pose . T_cam0_velo per frame, NULL = identity) in both
 * directions under `threshold`, optional mutual check; -1 = no match; rep [B] = number of frame-0
 * keypoints with a frame-1 keypoint within the threshold (load_data.py:264). */
int mdgat_gt_matches(int B, int N, int M, const float* kpts0, const float* kpts1, const double* T0, const double* T1,
                     double threshold, int mutual, int64_t* gt0, int64_t* gt1, int64_t* rep, void* stream);

/* The same on a RAGGED batch: pair b has counts0[b] x counts1[b] keypoints in slots padded to Np x Mp (kpts0 [B][Np][3], kpts1 [B][Mp][3],
 * gt0 [B][Np], gt1 [B][Mp]); its matches and rep[b] are those of mdgat_gt_matches on the pair alone, gt0 / gt1 beyond its counts are -1,
 * the keypoints there are not read.  The counts are checked as described at THE COUNTS OF A RAGGED BATCH.  The LDS follows Np + Mp (MDGAT_ERR_UNSUPPORTED beyond 160 KB). */
int mdgat_gt_matches_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                            const int32_t* counts1_host, const float* kpts0, const float* kpts1, const double* T0, const double* T1,
                            double threshold, int mutual, int64_t* gt0, int64_t* gt1, int64_t* rep, void* stream);

/* ---- the evaluation scripts' per-pair record ------------------------------------------------------------------------------
 * What test.py:212-296 and test_registration_metric.py:213-264 derive for one pair from the matcher's output, the ground-truth
 * matches, the keypoints and T_gt.  In both scripts valid = matches0 > -1 (test.py:215) and, after the dustbin value M of gt0 has
 * been rewritten to -1 (test.py:237-238), valid_gt = gt0 > -1 (:239); the sums run over the N frame-0 keypoints.  Counts are
 * stored exactly; every ratio is one fp64 division of two exact integers, the value numpy's int64 / int64 gives, bit for bit. */
typedef enum {
    MDGAT_EVAL_N_VALID = 0,                 /* np.sum(valid): predicted matches = len(mkpts0) (test.py:215-216, 282) */
    MDGAT_EVAL_N_VALID_GT,                  /* valid_num = np.sum(valid_gt) (test.py:241) */
    MDGAT_EVAL_N_GT_NEGATIVE,               /* np.sum(matches_gt == -1) (test.py:288) */
    MDGAT_EVAL_TRUE_POSITIVE,               /* tm: matches == matches_gt and valid (test.py:277, 284); `inlier` of
                                               test_registration_metric.py:238, 251 */
    MDGAT_EVAL_TRUE_NEGATIVE,               /* matches == matches_gt and not valid (test.py:278; test_registration_metric.py:240) */
    MDGAT_EVAL_FALSE_POSITIVE,              /* fm: valid and matches_gt == -1 (test.py:279, 285) */
    MDGAT_EVAL_N_VALID_AND_GT_POSITIVE,     /* valid and matches_gt > -1 (test.py:289) */
    MDGAT_EVAL_FALSE_POSITIVE_REG,          /* valid and matches != matches_gt (test_registration_metric.py:239) */
    MDGAT_EVAL_FALSE_NEGATIVE,              /* matches == -1 and matches_gt > -1 (test_registration_metric.py:241) */
    MDGAT_EVAL_REPEATABILITY,               /* valid_num / all_num (test.py:241-244; test_registration_metric.py:235) */
    MDGAT_EVAL_PRECISION,                   /* tp / n_valid if n_valid > 0 else 0 (test.py:282; test_registration_metric.py:243) */
    MDGAT_EVAL_RECALL,                      /* tp / n_valid_gt if n_VALID > 0 else 0 (test.py:283; test_registration_metric.py:244) */
    MDGAT_EVAL_MATCHING_SCORE,              /* tp / N (test.py:286) */
    MDGAT_EVAL_ACCURACY,                    /* (tp + tn) / N (test.py:287) */
    MDGAT_EVAL_FP_RATE,                     /* fp / n_gt_negative, unguarded (test.py:288) */
    MDGAT_EVAL_TP_RATE,                     /* n_valid_and_gt_positive / n_valid_gt, unguarded (test.py:289) */
    MDGAT_EVAL_TP_RATE2,                    /* tp / n_valid_gt, unguarded (test.py:290) */
    MDGAT_EVAL_FP_RATE_REG,                 /* fp_reg / (fp_reg + tn), unguarded (test_registration_metric.py:247) */
    MDGAT_EVAL_TP_RATE_REG,                 /* tp / (tp + fn), unguarded (test_registration_metric.py:248) */
    MDGAT_EVAL_INLIERS,                     /* inlier (utils_test.py:61-62, via test.py:294) */
    MDGAT_EVAL_INLIER_RATIO,                /* inlier / len(mkpts0) (utils_test.py:63) */
    MDGAT_EVAL_TRANS_ERROR,                 /* trans_error (utils_test.py:66-67); rte of calculate_error2 (utils_test.py:34-35, via
                                               test_registration_metric.py:256), the same number */
    MDGAT_EVAL_ROT_ERROR,                   /* rot_error, radians, arccos unclamped (utils_test.py:68-70); rre (utils_test.py:36-38) */
    MDGAT_EVAL_STATUS,                      /* mdgat_eval_status bits, as a number */
    MDGAT_EVAL_COLS
} mdgat_eval_column;

/* The scripts `continue` (or skip an append) in these cases; the row is filled all the same and the caller decides. */
typedef enum {
    MDGAT_EVAL_BANNED = 1,                  /* valid_gt.sum() < len(matches_gt) * 0.1 (test.py:247; test_registration_metric.py:230) */
    MDGAT_EVAL_TOO_FEW_MATCHES = 2,         /* len(mkpts0) < 4 (test.py:272) */
    MDGAT_EVAL_REGISTRATION_FAIL = 4,       /* trans_error > 2 or rot_error > 5 or either is NaN (test.py:296) */
    MDGAT_EVAL_RTE_OK = 8,                  /* rte < 2 (test_registration_metric.py:258) */
    MDGAT_EVAL_RRE_OK = 16                  /* not isnan(rre) and rre < pi / 180 * 5 (test_registration_metric.py:261); RR counts
                                               the pairs with both bits (:264) */
} mdgat_eval_status;

/* matches0 / gt0 [B][N], matches1 / gt1 [B][M] int64; kpts0 [B][N][3] / kpts1 [B][M][3] fp32 and T_gt [B][4][4] fp64 (optional:
 * without it the errors are NaN and MDGAT_EVAL_REGISTRATION_FAIL is set) as mdgat_pose takes them, and the pose columns are
 * mdgat_pose's arithmetic on matches0; T [B][4][4] receives the pose.  A pair without any match has no pose in the reference (the
 * mean of an empty set): its T, inlier ratio and errors are NaN.  metrics [B][MDGAT_EVAL_COLS] fp64.  A gt0 value of -1 or M, a gt1
 * value of -1 or N is "unmatched"; a gt0 value outside [-1, M], a gt1 value outside [-1, N], a matches0 value outside [-1, M) or a
 * matches1 value outside [-1, N) is never used to index: that pair's row and T are NaN and bit 0 of *bad_index (device memory,
 * optional; the caller clears it) is set.  matches1 and gt1 enter no column.  1 <= N, M <= 2175; B == 0 launches nothing.  One launch
 * on `stream`; reads the matches once; no allocation, no synchronisation, no atomics on values. */
int mdgat_eval_metrics(int B, int N, int M, const int64_t* matches0, const int64_t* matches1, const int64_t* gt0, const int64_t* gt1,
                       const float* kpts0, const float* kpts1, const double* T_gt, double inlier_dist, double* metrics, double* T,
                       unsigned* bad_index, void* stream);
/* The same on a RAGGED batch (mdgat_forward_f64_ragged's outputs): pair b has counts0[b] x counts1[b] keypoints in slots padded to Np x Mp
 * (matches0 / gt0 [B][Np], matches1 / gt1 [B][Mp], kpts0 [B][Np][3], kpts1 [B][Mp][3]); what lies beyond a pair's counts is not read, and
 * its row and T are those of mdgat_eval_metrics on the pair alone, bit for bit.  The counts are checked as described at THE COUNTS OF A
 * RAGGED BATCH. */
int mdgat_eval_metrics_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                              const int32_t* counts1_host, const int64_t* matches0, const int64_t* matches1, const int64_t* gt0,
                              const int64_t* gt1, const float* kpts0, const float* kpts1, const double* T_gt, double inlier_dist,
                              double* metrics, double* T, unsigned* bad_index, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDGAT_HIP_H */
