// Shared declarations for libmdgat_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <atomic>
#include "../../include/mdgat_hip.h"
#include "../../include/mdgat_hip_wide.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

#define MDGAT_LOG2E 1.4426950408889634f
#define MDGAT_LN2 0.6931471805599453f

// Split-f16 operands: x = hi + lo / 2048 with hi = f16(x), lo = f16((x - hi) * 2048) - 22 mantissa bits, so
// hi.hi + (hi.lo + lo.hi) / 2048 on the f16 matrix cores is an fp32-class product.
#define MDGAT_SPLIT_SCALE 2048.0f
#define MDGAT_SPLIT_INV 0.00048828125f
#ifdef __HIPCC__
__device__ __forceinline__ void mdgat_split(float x, _Float16& h, _Float16& l) {
    h = (_Float16)x;
    l = (_Float16)((x - (float)h) * MDGAT_SPLIT_SCALE);
}
// The q / k / v operands of the attention kernels carry their residual UNSCALED, x = hi + lo with lo = f16(x - hi): for
// |x| < 0.25 that is an f16 denormal, which the matrix cores honour exactly (tools/ubench/mfma_denorm.hip), its rounding
// is at most 2^-25 absolute (the class of an fp32 product for operands of order one: tools/precision_probe.py, UNSCALED=1),
// and hi.hi + hi.lo + lo.hi then accumulate in ONE register set - no second accumulator, no combine per logit.
__device__ __forceinline__ void mdgat_split_unscaled(float x, _Float16& h, _Float16& l) {
    h = (_Float16)x;
    l = (_Float16)(x - (float)h);
}
#endif

// Key index (within the source frame) of logit register (jb, r) of a lane, relative to the lane's offset, in the S^T = K Q^T
// fragments of the attention kernels (attention.hip).
struct KeyLayout32 { static __device__ constexpr int koff(int jb, int r) { return jb * 32 + 16 * (r >> 3) + (r & 7); } };       // 32x32 fragments, + 8 (lane >> 5)
struct KeyLayout16 { static __device__ constexpr int koff(int jb, int r) { return 16 * (4 * jb + (r >> 2)) + (r & 3); } };      // 16x16 fragments, + 4 (lane >> 4)

// row of the 32x32 MFMA C/D fragment held in accumulator register r by a lane of half `hi`
// (cdna_hip_programming.md section 3: row = (r&3) + 8*(r>>2) + 4*(lane>>5), col = lane&31).
__device__ __forceinline__ constexpr int mfma32_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

void mdgat_set_error(const char* fmt, ...);
int mdgat_check_hip(hipError_t e, const char* what);

// Workspaces are laid out in regions of whole 256-byte units.  A carve function runs the same takes with a null base for the byte
// count and with the caller's base for the pointers: take(p, n) points p at the next n elements (nullptr for a null base).
inline size_t mdgat_align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
struct WsCarver {
    char* base;
    size_t bytes = 0;
    template <typename T> void take(T*& p, size_t n) {
        p = base ? reinterpret_cast<T*>(base + bytes) : nullptr;
        bytes += mdgat_align256(n * sizeof(T));
    }
};

// Per-device state (launch chains, CU counts, LDS opt-ins) is kept for device indices 0 .. MDGAT_MAX_DEVICES - 1;
// mdgat_create refuses the others.  The launchers work on the CURRENT device: the forward makes the handle's current.
constexpr int MDGAT_MAX_DEVICES = 64;
inline int mdgat_current_device() {
    int dev = -1;
    return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < MDGAT_MAX_DEVICES ? dev : -1;
}
// compute units of the current device (asked once per device; 256, the MI355X's, if the runtime cannot tell)
inline int mdgat_cu_count() {
    static std::atomic<int> cached[MDGAT_MAX_DEVICES];
    const int dev = mdgat_current_device();
    int n = dev >= 0 ? cached[dev].load(std::memory_order_relaxed) : 0;
    if (n > 0) return n;
    if (dev < 0 || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 256;
    cached[dev].store(n, std::memory_order_relaxed);
    return n;
}
// Opt a kernel in to `lds` bytes of dynamic LDS, once per device (`done` = the caller's static bitmap of devices;
// one process may drive several GPUs from several threads: torch.nn.DataParallel).
static_assert(MDGAT_MAX_DEVICES <= 64, "one bit per device in mdgat_lds_optin's bitmap");
inline int mdgat_lds_optin(const void* kern, size_t lds, std::atomic<unsigned long long>& done, const char* what) {
    const int dev = mdgat_current_device();       // (-1: not cached)
    if (dev >= 0 && ((done.load(std::memory_order_acquire) >> dev) & 1ull)) return MDGAT_OK;
    if (int rc = mdgat_check_hip(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), what)) return rc;
    if (dev >= 0) done.fetch_or(1ull << dev, std::memory_order_release);
    return MDGAT_OK;
}

// ---- packed-weight blob layout (must match mdgat_matcher_amd/pack.py) --------------------------
struct BlobLayout {
    // encoders (BN folded)
    size_t kenc0_w, kenc0_b;   // [32][4], [32]
    size_t denc0_w, denc0_b;   // [64][33], [64]
    size_t kenc1_w, kenc1_b;   // [64][32], [64]
    size_t kenc2_w, kenc2_b;   // [128][64], [128]
    size_t denc1_w, denc1_b;   // [128][64], [128]
    size_t encl_w, encl_b;     // [128][256] = [denc.6 | kenc.9], [128]
    size_t layer0;             // start of layer 0
    size_t layer_stride;
    // per layer (relative to layer start)
    size_t qkv_w, qkv_b;       // [384][128] rows = which*128 + head*32 + dim, [384]
    size_t mlp1_w, mlp1_b;     // [256][256] cols = [x | head-major message (merge folded)], [256]
    size_t mlp2_w, mlp2_b;     // [128][256], [128]
    size_t final_w, final_b;   // [128][128], [128]
    size_t bin_score;          // [1] (+3 pad)
    size_t total;
};
BlobLayout mdgat_blob_layout(int L);

// ---- kernel launchers (all asynchronous on `stream`) --------------------------------------------
struct GemmArgs {
    const float* A0; int lda0; int K0;   // columns [0, K0) of the input come from A0
    const float* A1; int lda1;           // columns [K0, K) from A1 (unused when K0 == K)
    const float* W; int ldw;             // [N][K]
    const float* bias;                   // [N] or nullptr
    const float* R; int ldr;             // residual [M][N] or nullptr
    float* C; int ldc;
    int M, N, K;
    int relu;
    float scale;                         // applied to the accumulator before bias
    int batch;                           // grid.z
    long long sA, sW, sC;                // batch strides (elements) of A0, W, C
};
int launch_gemm(const GemmArgs& a, hipStream_t s);
// score matrix [B][N][M] = mdesc0 . mdesc1^T * scale from mdesc [B][N + M][128] (scores.hip)
// zero / zero_bytes (optional, 16-byte granular): memory the kernel clears on the side - the forward hands it the exchange
// slots of the Sinkhorn kernel that runs next (sinkhorn_slots_clear_bytes) instead of a memset launch
// guard (optional, host-mapped): raised when an operand is outside the f16 operand range or not finite
int launch_scores(int B, int N, int M, const float* mdesc, float* scores, float scale, hipStream_t s, void* zero = nullptr, size_t zero_bytes = 0,
                  unsigned* guard = nullptr);

// fused encoders (encoder.hip); inputs either as separate arrays or as raw 37-float frame records
struct Encoder32 {   // the encoder's weights (weights.hpp): kenc.0 and the biases in the fp32 blob, the other matrices as split row images
    const float* w;
    size_t kenc0_w, kenc0_b, denc0_b, kenc1_b, kenc2_b, denc1_b, encl_b;
    const _Float16 *k1s, *k2s, *d0s, *d1s, *els;   // [rows][2][K]: 64x32, 128x64, 64x48, 128x64, 128x256
};
struct EncoderLaunch {
    const float *kpts0, *sigma0, *fpfh0, *kpts1, *sigma1, *fpfh1;
    const float *rec0, *rec1;
    int normalize;
    Encoder32 enc;
    float* x;
    int B, N, M;
    // a ragged batch (device int32 [B], both or neither; arrays, or records that are not normalised): pair b has cnt0[b] / cnt1[b] keypoints in
    // slots of N / M; a keypoint beyond its frame's count reads none of its inputs and is encoded from zeros
    const int *cnt0 = nullptr, *cnt1 = nullptr;
    // a ragged chunk out of a bank of records (device int64 [B], both or neither, with the counts): rec0 / rec1 are the bank's [rows][37],
    // keypoint n of frame f of pair b is record start_f[b] + n - checked by the caller (mdgat_check_ragged); `normalize` is the loader's
    // float32 arithmetic to the bit (fpfh_norm.hpp).  kp0_out [B][N][3] / kp1_out [B][M][3] (optional): the keypoints as they lie in the
    // records, zeros beyond the counts.  guard (optional, host-mapped): raised for a non-finite word or, under normalize, an all-zero FPFH
    // row among a pair's own records.  Records no pair points at are never read.
    const long long *start0 = nullptr, *start1 = nullptr;
    float *kp0_out = nullptr, *kp1_out = nullptr;
    unsigned* guard = nullptr;
};
int launch_encoder(const EncoderLaunch& p, hipStream_t s);
int launch_split_rows_pad(const float* w, _Float16* out, int rows, int Kin, int Kpad, hipStream_t s);

// q/k/v of every point in the split-f16 operand layouts of the attention kernel (attention.hip)
struct Qkv16 {
    _Float16* q16;    // [B][P][4 heads][2 planes][32 dims], pre-scaled by log2(e) / sqrt(32); planes = (hi, unscaled residual)
    _Float16* k16;    // [B][P][4][2][32]
    _Float16* vt16;   // [B][4][2][32][PP]: V transposed, keys contiguous; frame 1 starts at column Npad
    int Npad, PP;     // Npad = N rounded up to 32, PP = Npad + (M rounded up to 32)
};
size_t mdgat_qkv16_halves(int B, int N, int M);
Qkv16 mdgat_qkv16_carve(_Float16* base, int B, int N, int M);
int launch_qkv_split(int B, int N, int M, const float* qkv, const Qkv16& out, hipStream_t s);
// One fp32-class attention call (attention.hip).  Zero-initialise it and set what applies.
struct AttnCall {
    int B, N, M, cross, topk;
    int mode;                           // mdgat_attention_mode (1 = single-f16 products where implemented); a ragged batch always runs the split-f16 kernels
    Qkv16 qkv; float* msg;              // msg [B][N + M][128]
    uint32_t* sel;                      // parity tap, may be null: the kept keys of a dynamic layer as bit masks [B][4][P][W], W = ceil(max(N, M) / 32)
    const int *cnt0, *cnt1;             // both or neither (device int32 [B], checked by the caller against topk): a ragged batch - pair b has cnt0[b] / cnt1[b] keypoints
                                        // in slots of N / M <= MDGAT_RAGGED_FP32_MAX_KEYPOINTS (`wide`: _WIDE_MAX_); message rows (and tap masks) beyond a pair's counts are zero
    bool wide;                          // a ragged batch only: the caller opted in to slots of up to MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS (slots within 512 x 512 run what they run without)
    hipStream_t stream;
};
int launch_attention(const AttnCall& c);
// What launch_attention chooses (mdgat_attention_plan, mdgat_attention_ragged_plan; include/mdgat_hip.h: the table of indices) - the instantiation
// and all of its launch but the pointers - and how often each has been launched by this process (mdgat_attention_launches).  Host code only; the plan
// touches no HIP call.  A ragged call's form follows the slots alone, never a count or B, and is counted under its uniform sibling's index.
enum AttnForm {
    ATTN_STREAM = 0, ATTN_FULL4, ATTN_FULL8, ATTN_FULL8_WINDOWED, ATTN_DYN4, ATTN_DYN8, ATTN_DYN16, ATTN_TOPK16_256, ATTN_TOPK16_512, ATTN_WIDE4,
    ATTN_WIDE8, ATTN_TAP = 7 /* + ATTN_DYN4 .. ATTN_WIDE8 */, ATTN_STREAM_FAST = 18, ATTN_TOPK16_256_FAST, ATTN_TOPK16_512_FAST,
    ATTN_FAST_TAP = 2 /* + the two above */, ATTN_FORMS = MDGAT_ATTENTION_FORMS
};
struct AttnPlan {
    int form;           // AttnForm, or -1: no launch
    int split, tiles;   // workgroups per (pair, frame, head); the most query tiles one of them walks
    int rc;             // why not, where the launcher refuses (MDGAT_OK otherwise; the message is the launcher's)
    bool dyn = false;           // the layer keeps its k largest logits (uniform: unless k keeps every key of both frames; ragged: whenever topk > 0)
    int threads = 0;            // of a workgroup; the stream forms: launch_attention_stream's own, as their LDS
    size_t lds = 0;             // dynamic LDS bytes
    bool lds_attribute = false; // hipFuncSetAttribute(MaxDynamicSharedMemorySize) goes before the launch: every kernel but the wide ones
    bool xcd_grid = false;      // the XCD-aware 1-D grid of the topk16 and wide kernels (8 * split * ceil(units / 8)); else the 3-D grid (split, heads, 2 B)
    int wide_counter = -1;      // RaggedWideCounter of a launch only a wide ragged slot reaches
};
// tap: a selection buffer is passed; ragged: a call with counts; wide: AttnCall::wide (a ragged call only)
AttnPlan attention_plan(int B, int N, int M, int topk, bool tap, int mode, bool ragged = false, bool wide = false);
void attention_count_launch(int form);
void attention_launch_counts(uint64_t counts[MDGAT_ATTENTION_FORMS]);
// full attention as a stream of 64-key chunks (attention_stream.hip); frames with key counts that are multiples of 64
bool attention_stream_supported(int N, int M);
inline int attention_stream_qtiles(int N, int M) { return ((N > M ? N : M) + 127) / 128; }   // workgroups (128 queries each) per (pair, frame, head)
int launch_attention_stream(int B, int N, int M, int cross, const Qkv16& qkv, float* msg, hipStream_t s, int mode = 0);
// measurement only: the Q K^T phase of the streamed kernel in isolation (msg[row][head * 32] receives the row maximum)
int launch_attention_qk_probe(int B, int N, int M, int cross, const Qkv16& qkv, float* msg, hipStream_t s);
int launch_qk_phase_probe(int B, int N, int M, int cross, int nq_sets, const Qkv16& qkv, float* msg, hipStream_t s);

// fused layer tail (layer.hip): [mlp.0 -> mlp.3 -> residual] of one layer + q|k|v projection of the next
// views (weights.hpp): ...s split row images [rows][hi K | lo K | 8 pad], ...f the same in fragment order (launch_frag_image; layer_split.hip)
struct Layer32 { const _Float16 *w1s, *w2s, *w1f, *w2f; const float *b1, *b2; };
struct Proj32 { const _Float16 *w3s, *w3f; const float* b3; int mode3; };   // mode3 1: q|k|v, 2: final_proj
struct LayerLaunch {
    float* x; const float* msg;
    Layer32 mlp;                       // do_mlp
    Proj32 proj;
    Qkv16 out;                         // proj.mode3 == 1
    float* mdesc;                      // proj.mode3 == 2
    int R, N, M;
    int do_mlp;                        // 0: projection only
    unsigned* guard;                   // optional (host-mapped): set to 1 when an input row holds a value outside the f16
                                       // operand range (|v| >= MDGAT_F16_GUARD) or a non-finite one
};
int launch_layer(const LayerLaunch& p, hipStream_t s);
// Which of the 14 instantiations launch_layer runs and its launch geometry (mdgat_layer_plan, include/mdgat_hip.h: the table of
// indices), and how often each has been launched by this process (mdgat_layer_launches).  Host code only; the plan touches no HIP call.
enum LayerForm {
    LAYER_SPLIT = 0 /* + 2 do_mlp + (mode3 != 1) */, LAYER_NW4 = 4 /* + the same */,
    LAYER_NW8 = 8 /* + 3 do_mlp + {0: q|k|v, 1: q|k|v with the V^T gather (VW), 2: final_proj} */, LAYER_FORMS = MDGAT_LAYER_FORMS
};
struct LayerPlan {
    int form;           // LayerForm index, or -1: no launch
    int workgroups;     // grid size: ceil(R / keypoints)
    int keypoints;      // per workgroup: 32 (split), 64 (NW = 4), 128 (NW = 8)
    int v_store;        // keypoints per V^T store run: 0 (final_proj: no V), 1, 4, 16, 128 (VW: 256-byte pieces through the gather buffers)
};
LayerPlan layer_plan(int R, int N, int M, int do_mlp, int mode3);
void layer_launch_counts(uint64_t counts[MDGAT_LAYER_FORMS]);
// rowh >= 2 K: row pitch (halves); the first nperm rows are written in the P/Q row order of layer.hip
int launch_split_rows(const float* w, _Float16* out, int rows, int K, int rowh, int nperm, hipStream_t s);
// row image [rows][rowh] (launch_split_rows) -> fragment order [rows / 16][K / 32][plane][lane = row l15 + 16 g][8 halves] (layer_split.hip)
int launch_frag_image(const _Float16* img, _Float16* out, int rows, int K, int rowh, hipStream_t s);

struct SkExtract {   // match extraction to run after (or fused into) the Sinkhorn kernel
    int mode; float thr;
    int64_t *m0, *m1;
    float *s0, *s1;
    int defer_alldust;   // the batch-wide "no keypoint of frame 0 matched" rule (mdgat.py:465-467) is applied later by
                         // launch_alldust_fixup() over the whole batch (the forward runs large batches in slices)
    unsigned* matched;   // optional (host-mapped): receives matched_token when some frame-0 keypoint of the launch is matched
    unsigned matched_token;
};
int launch_alldust_fixup(int B, int N, int M, int mode, const int64_t* m0, float* s1, hipStream_t s);
// Asynchronous status words of a handle (host-mapped memory the kernels write; read by the host after a synchronisation).
constexpr int MDGAT_STATUS_SK_FALLBACK = 0;   // the Sinkhorn cluster kernel lost a partner workgroup: the launch was redone by the streaming kernel
constexpr int MDGAT_STATUS_RANGE = 1;         // an activation left the f16 operand range or is not finite: the outputs are invalid
constexpr int MDGAT_STATUS_MATCHED = 4;       // first of MDGAT_MATCH_SLOTS words: slot (token % slots) receives the token of a forward whose extraction matched
                                              // at least one frame-0 keypoint (mdgat.py:465: the reference tests valid0.sum() on the host; mdgat_matched_any
                                              // reads the call's slot instead of a reduction + copy; a slot per call: concurrent callers of one handle)
constexpr int MDGAT_MATCH_SLOTS = 256;
constexpr int MDGAT_STATUS_WORDS = MDGAT_STATUS_MATCHED + MDGAT_MATCH_SLOTS;
constexpr float MDGAT_F16_GUARD = 6.0e4f;     // f16 max is 65504; the split's hi plane must stay finite
// One fp32 Sinkhorn call, with `ex` also its match extraction (sinkhorn.hip).  Zero-initialise it and set what applies.
struct SkCall {
    int B, N, M, iters;
    const float *scores, *alpha_dev; float alpha_host;      // [B][N][M]; the bin score as a device scalar, or null: alpha_host
    float *Z, *Zfb;                     // Z [B][N+1][M+1]: may be null with `ex` on the cluster kernel, which fuses the arg-maxes.  Zfb: lent for the pairs the
                                        // streaming kernel redoes when no Z is wanted (neither: the cluster launch is cooperative instead)
    const int *cnt0, *cnt1;             // both or neither (device int32 [B], checked by the caller): a ragged batch on the streaming kernel - pair b has cnt0[b] x
                                        // cnt1[b] keypoints in slots of N x M <= MDGAT_RAGGED_FP32_MAX_KEYPOINTS (`wide`: _WIDE_MAX_).  Z is required: 0 outside a pair's own block
    void* ws; size_t ws_bytes;          // the cluster kernel's workspace; missing, short or not 256-byte aligned: the streaming kernel
    bool slots_cleared;                 // the first sinkhorn_slots_clear_bytes(B, N, M) bytes of ws are already zero on the stream (no memset launch)
    unsigned* status; const SkExtract* ex; hipStream_t stream;      // status: optional, a device pointer to MDGAT_STATUS_WORDS host-mapped words
    bool wide;                          // a ragged batch only: the caller opted in to slots of up to MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS (slots within 512 x 512 run what they run without)
    bool split;                         // a ragged batch only: the split form (one launch per iteration, a pair's rows over several workgroups) where the slot has
    void* split_ws; size_t split_ws_bytes;      // two slabs of 128 rows or more; then its scratch: 256-byte aligned, sinkhorn_split_workspace_bytes(B, N, M)
    void (*launched)(void*); void* launched_ctx;      // optional: called behind every launch of the split form's iterations (the forward's profile marks)
};
int launch_sinkhorn(const SkCall& c);
// What launch_sinkhorn chooses (mdgat_sinkhorn_plan, include/mdgat_hip.h: the table of indices), and how often each
// instantiation has been launched by this process (mdgat_sinkhorn_launches).  Host code only; the plan touches no HIP call.
enum SkForm {
    SK_SCALING_4 = 0, SK_SCALING_16, SK_SCALING_2D,                                               // sinkhorn_scaling_kernel<false, 4>, <false, 16>, <true, 16>
    SK_STREAM_1, SK_STREAM_2, SK_STREAM_4, SK_STREAM_8, SK_STREAM_16, SK_STREAM_32,               // sinkhorn_kernel<NC, NW>, launched on its own
    SK_RAGGED_1, SK_RAGGED_2, SK_RAGGED_4, SK_RAGGED_8,                                           // ... its RAGGED twins
    SK_GATED,                                                                                     // a streaming kernel gated behind a cluster launch
    SK_EXTRACT,                                                                                   // extract_kernel
    SK_COUNTERS = MDGAT_SINKHORN_COUNTERS,
    SK_RAGGED_16 = SK_COUNTERS, SK_RAGGED_32                                                      // sinkhorn_kernel<16, 8, true>, <32, 8, true>: a wide ragged slot of more than 512 /
};                                                                                                // 1024 columns; no index of mdgat_sinkhorn_launches: counted as RAGGED_WIDE_SK_16 / _32
// the launches only a wide ragged slot reaches (mdgat_ragged_wide_launches, include/mdgat_hip_wide.h: the table of indices)
enum RaggedWideCounter {
    RAGGED_WIDE_SK_16 = 0, RAGGED_WIDE_SK_32, RAGGED_WIDE_SPLIT_ITERATION, RAGGED_WIDE_SPLIT_FINISH,      // sinkhorn.hip
    RAGGED_WIDE_ATTN_WINDOWED, RAGGED_WIDE_ATTN_WIDE4 /* + 1 with the tap */, RAGGED_WIDE_ATTN_WIDE8 = RAGGED_WIDE_ATTN_WIDE4 + 2 /* likewise */,      // attention.hip
    RAGGED_WIDE_COUNTERS = MDGAT_RAGGED_WIDE_COUNTERS
};
void ragged_wide_count_launch(int index);
void ragged_wide_launch_counts(uint64_t counts[MDGAT_RAGGED_WIDE_COUNTERS]);
enum SkPath { SK_PATH_NONE = -1, SK_PATH_CLUSTER = 0, SK_PATH_STREAMING = 1 };
struct SkPlan {
    int path;           // SkPath; SK_PATH_NONE: nothing is launched (an empty batch), or rc says why not
    int scaling;        // SK_SCALING_* of a cluster launch, else -1
    int stream;         // SK_STREAM_* / SK_RAGGED_* (SK_RAGGED_16 / _32: a wide ragged slot): launched on its own (streaming path) or gated behind the cluster launch; -1: none
    int GR, GC;         // cluster: row slabs of 128 rows x column slabs of 512 columns, one workgroup each
    int ngroups;        // cluster: pairs in flight
    int xcd_map;        // cluster: the partners of a pair share blockIdx % 8, the grid padded to 8 groups per slot
    int grid;           // workgroups of the (first) launch
    int cooperative;    // cluster: hipLaunchCooperativeKernel
    int rc;             // MDGAT_ERR_UNSUPPORTED where the launcher refuses (the message is the launcher's)
    int split;          // a ragged batch on the split form: row slabs per pair (grid = B * split per launch, `stream` names the NC); 0: not that form
};
// workspace: sinkhorn_workspace_usable; fallback_buffer: a Z, or one lent for redone pairs; ragged: a call with counts
// split: the caller opted in to the split form (a ragged batch only); wide: ... to slots of up to MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS (likewise)
SkPlan sinkhorn_plan(int B, int N, int M, int num_cu, bool workspace, bool fallback_buffer, bool ragged, bool split = false, bool wide = false);
void sinkhorn_launch_counts(uint64_t counts[MDGAT_SINKHORN_COUNTERS]);
size_t sinkhorn_cluster_workspace_bytes(int B, int N, int M);      // the cluster kernel's workspace (its one layout: sinkhorn.hip); 0: the shape is beyond that kernel
size_t sinkhorn_split_workspace_bytes(int B, int N, int M, bool wide = false);      // the split form's scratch; 0: the slot has one slab of rows (or is beyond the ragged kernels; wide: SkCall::wide)
size_t sinkhorn_slots_clear_bytes(int B, int N, int M);            // ... the prefix of it that is zero when a launch starts
bool sinkhorn_workspace_usable(int B, int N, int M, const void* ws, size_t ws_bytes);      // ... whether a buffer is large enough for it and 256-byte aligned

int extract_check_mode(const char* who, int mode);      // the one mode check: "<who>: bad mode <mode>"
// cnt0 / cnt1 (optional, device int32 [B]): a ragged batch in slots of N x M - dustbins at a pair's own counts, the all-dustbin rule per pair,
// matches -1 and scores 0 beyond the counts
int launch_extract(int B, int N, int M, const float* Z, const SkExtract& ex, hipStream_t s, const int* cnt0 = nullptr, const int* cnt1 = nullptr);
int launch_extract_from_bests(int B, int N, int M, const SkExtract* ex, const int* rbest_idx, const float* rbest_val, const int* cbest_idx,
                              const float* cbest_val, hipStream_t s, const int* cnt0 = nullptr, const int* cnt1 = nullptr);

int launch_pose(int B, int N, int M, const float* kpts0, const float* kpts1, const int64_t* matches0, const double* T_gt,
                double inlier_dist, double* T, double* stats, hipStream_t s);
int launch_gt_match(int B, int N, int M, const float* kpts0, const float* kpts1, const double* T0, const double* T1,
                    double threshold, int mutual, int64_t* gt0, int64_t* gt1, int64_t* rep, hipStream_t s, const int* cnt0 = nullptr,
                    const int* cnt1 = nullptr);      // cnt: a ragged batch in slots of N / M - gt -1 beyond a pair's counts
// the evaluation scripts' per-pair record (eval_metrics.hip)
int launch_eval_metrics(int B, int N, int M, const int64_t* matches0, const int64_t* matches1, const int64_t* gt0, const int64_t* gt1,
                        const float* kpts0, const float* kpts1, const double* T_gt, double inlier_dist, double* metrics, double* T,
                        unsigned* bad_index, hipStream_t s, const int* cnt0 = nullptr, const int* cnt1 = nullptr);      // cnt: a ragged batch in slots of N / M

// out[b][i][j] = scale <A[b][i], Bm[b][j]> - col_bias[b][j] over 128 channels, split-f16 products (scores.hip)
int launch_dots(int B, int N, int M, const float* A, size_t strideA, const float* Bm, size_t strideB, float* out, float scale,
                const float* col_bias, hipStream_t s, void* zero = nullptr, size_t zero_bytes = 0, unsigned* guard = nullptr);
int launch_knn(int B, int C, int N, int M, int k, const float* x, const float* src, int64_t* idx, int64_t* adj,
               void* ws, size_t ws_bytes, hipStream_t s);
size_t mdgat_knn_ws_bytes_impl(int B, int C, int N, int M);
