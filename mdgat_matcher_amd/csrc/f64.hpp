// fp64 kernels of the reference-exact mode (f64.hip): declarations shared with api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/mdgat_hip.h"

class CoopGroup;      // coop_chain.hpp

// C[M][N] = act(A W^T + bias) (+ R); the K input columns come from A0 (columns [0, K0)) and A1 (columns [K0, K)).  No alignment
// beyond 8 bytes is assumed of any operand (the FPFH rows are 33 doubles).
struct GemmF64Args {
    const double* A0; int lda0; int K0;
    const double* A1; int lda1;
    const double* W; int ldw;          // [N][K]
    const double* bias;                // [N] or nullptr
    const double* R; int ldr;          // residual [M][N] or nullptr (may alias C)
    double* C; int ldc;
    int M, N, K;
    int relu;
    unsigned* guard;                   // host-mapped status word (MDGAT_STATUS_RANGE) or nullptr: raised when an output is not finite or
                                       // beyond 2^500 in magnitude (f64_out_of_range in f64.hip)
    double scale = 1.0;                // C = act(scale A W^T + bias) (+ R)   (the score matrix: 1 / sqrt(128), mdgat.py:431)
    int batch = 1;                     // independent products; A0, W, C of product z at + z sA, + z sW, + z sC (no second source, bias, residual shared)
    long long sA = 0, sW = 0, sC = 0;
    const double *bn_mean = nullptr, *bn_a = nullptr, *bn_beta = nullptr;      // [K] each, single source (K0 >= K) only: the A operand is
                                       // bn_relu(A0[row][k], mean[k], a[k], beta[k]) (f64_dev.hpp) - the training-mode MLP's BatchNorm + ReLU,
                                       // formed as the operand is loaded
};
int launch_gemm_f64(const GemmF64Args& a, hipStream_t s);
// Which of gemm_f64_kernel's ten instantiations launch_gemm_f64 runs (mdgat_gemm_f64_plan, include/mdgat_hip.h), and how often each
// has been launched by this process (mdgat_gemm_f64_launches).  Host code only; the first touches no HIP call.
int gemm_f64_plan_index(int M, int N, int K, int K0, int batch, int aligned, int bnt, int cus);
void gemm_f64_launch_counts(uint64_t counts[10]);

struct AttnF64Args {
    const double* qkv;     // [B][P][384]: q | k | v, each [4 heads][32 dims] (the rows of pack.py's qkv_w)
    double* msg;           // [B][P][128]: channel = head * 32 + dim
    int N, M, cross, topk;
    float zq;              // standard-normal quantile of the top-k fraction (first probe of the threshold search)
    uint32_t* sel;         // parity tap (mdgat_taps.topk_sel layout) or nullptr
    int selW;
    int units, tiles;      // B * 2 * 4 (pair, frame, head) units; query tiles per unit
    int hist_ints;         // dynamic attention: ints of LDS for the radix-select histograms (attn_hist_ints in f64.hip)
    unsigned* guard;       // as GemmF64Args::guard, for the message rows
    const int* cnt0;       // optional (device int32 [B], both or neither): a ragged batch - pair b has cnt0[b] / cnt1[b] keypoints; N, M are then
    const int* cnt1;       // the padded sizes: strides, grid and LDS follow them, queries and keys the pair's own counts
};
// One fp64 attention call: attention (topk == 0) / dynamic_attention (mdgat.py:190-210) on fp64 q / k / v.  Zero-initialise it and set what applies.
struct AttnF64Call {
    int B, N, M, cross, topk;
    const double* qkv; double* msg;     // AttnF64Args::qkv, ::msg
    uint32_t* sel;                      // optional tap of the kept keys
    // cnt0 / cnt1: a ragged batch in slots padded to N / M (cnt_min: the smallest count of either frame, known to the caller on the host, who
    // has checked 1 <= cnt0[b] <= N, 1 <= cnt1[b] <= M).  A pair's message rows and selection words are those of the pair run alone wherever
    // the same instantiation runs it; message rows and selection words beyond its counts are zero.
    const int *cnt0, *cnt1; int cnt_min;
    unsigned* guard;                    // as GemmF64Args::guard, for the message rows
    hipStream_t stream;
};
int launch_attention_f64(const AttnF64Call& c);
// mdgat_set_f64_attention_form / MDGAT_F64_ATTENTION_FORM: -1 full attention by launch size; 0 always the split-key form (results do not
// depend on the batch a pair travels in); 1 the big-launch form at every size
int f64_attention_form();
// What launch_attention_f64 chooses (mdgat_attention_f64_plan, mdgat_attention_f64_geometry; include/mdgat_hip.h numbers the forms) - the
// instantiation and all of its launch but the pointers - and how often each has been launched by this process (mdgat_attention_f64_launches).
// Host code only; the plan touches no HIP call.
enum AttnF64Form { ATTN_F64_FULL16 = 0, ATTN_F64_FULL32, ATTN_F64_KEEP_TAP, ATTN_F64_KEEP, ATTN_F64_RECOMPUTE_TAP, ATTN_F64_RECOMPUTE, ATTN_F64_SOLO, ATTN_F64_FORMS = MDGAT_ATTENTION_F64_FORMS };
struct AttnF64Plan {
    int form, rc;           // AttnF64Form and MDGAT_OK, or no launch: -1 nothing to do, -2 / -3 what the launcher refuses as rc (the message is its own)
    bool bad_counts;        // of the two -2 refusals: cnt_min lies outside the slots (else: k above nk_min)
    int nk_max, nk_min;     // the larger slot; the fewest keys a frame has (ragged: cnt_min)
    bool dyn;               // the layer keeps its k largest logits (uniform: unless k == N == M keeps every key; ragged: whenever topk > 0)
    int queries;            // of a workgroup: 16, 32, or 128 (solo: 32 per wave)
    int tiles, workgroups;  // query tiles per (pair, frame, head); the XCD-aware 1-D grid, 8 * tiles * ceil(units / 8)
    int hist_ints;          // AttnF64Args::hist_ints
    size_t lds, lds_optin;  // dynamic LDS bytes of this launch; of the instantiation's largest launch, which it is opted in to once per device
};
// tap: a selection buffer is passed; ragged: a call with counts, the smallest cnt_min; form: f64_attention_form(); cus: the device's compute units
AttnF64Plan attention_f64_plan(int B, int N, int M, int topk, int tap, int ragged, int cnt_min, int form, int cus);
void attention_f64_launch_counts(uint64_t counts[MDGAT_ATTENTION_F64_FORMS]);
// One inference assemble launch: in4 [R][4] = x y z saliency, in33 [R][33] = FPFH; rows pair-major, frame 0 then frame 1.  Zero-initialise
// it and set what applies; the launcher picks the kernel by the inputs that are set.
struct AssembleF64 {
    const double *kpts0, *sigma0, *fpfh0, *kpts1, *sigma1, *fpfh1;      // the six arrays, or
    const float *rec0, *rec1; int normalize;    // raw float32 records [B][N][37] / [B][M][37] (load_data.py:146-165; FPFH normalised as numpy does it in float32, 290-292)
    const int *cnt0, *cnt1;             // optional (the arrays, or a bank): a ragged batch - rows beyond a pair's counts are written as zeros, unread
    // a ragged chunk out of a bank of records: frame f of pair b = the cnt[b] records from row start[b] of rec0 / rec1 [rows][37], in slots of
    // N + M rows per pair; their records beyond the counts unread; kp0 [B][N][3] / kp1 [B][M][3] float32 keypoints (optional)
    const long long *start0, *start1; float *kp0, *kp1;
    double *in4, *in33; int B, N, M; unsigned* guard;
};
int launch_assemble_f64(const AssembleF64& a, hipStream_t s);
// the loader's train-mode assembly (ensure_kpts_num, load_data.py:180-211) of the same chunk: the records with saliency > min_saliency, the
// first T of them or padded to T by the loader's prepend loop; in4 / in33 in slots of T + T rows per pair, kp0 / kp1 [B][T][3], source0 / 1
// [B][T] (the record row within its frame behind each slot), salient0 / 1 [B] (records kept), status [B][2] (1: a frame kept none and was
// left unwritten).  1 <= T <= 2048
int launch_assemble_frames_train_f64(int B, int T, const float* rec0, const float* rec1, const long long* start0, const long long* start1,
                                     const int* cnt0, const int* cnt1, float min_saliency, int normalize, double* in4, double* in33, float* kp0,
                                     float* kp1, int* source0, int* source1, int* salient0, int* salient1, unsigned* status, unsigned* guard,
                                     hipStream_t s);
// guard (all three): host-mapped status word raised when a value is not finite (tested by its bits), or nullptr
int launch_f64_to_f32(const double* in, float* out, size_t n, unsigned* guard, hipStream_t s);

// ---- layer_f64.hip: the tail of a propagation layer (mlp.0 + ReLU, mlp.3 + residual, the next layer's q | k | v) as ONE launch ----
struct LayerF64Args {
    double* x;                 // [R][128] residual stream, updated in place
    const double* msg;         // [R][128] the layer's message (attention output; merge is folded into w1)
    const double *w1f, *b1;    // mlp.0 [256][256] in fragment order (launch_frag64), bias [256]
    const double *w2f, *b2;    // mlp.3 [128][256]
    const double *w3f, *b3;    // the NEXT layer's q | k | v projection [384][128], or nullptr (last fp64 layer)
    double* qkv;               // [R][384] (w3f != nullptr)
    float* x32;                // optional: the new x rounded to fp32 as well (the hand-over to the fp32-class layers)
    int R;
    unsigned* guard;           // as GemmF64Args::guard
    double* hid = nullptr;     // optional scratch [R][256]: with it, launches of few 16-row blocks may run the clustered kernel (layer_f64.hip)
};
int launch_layer_tail_f64(const LayerF64Args& a, CoopGroup& group);      // on the group's stream (coop_chain.hpp)
// both encoders, their sum and layer 0's q | k | v as one launch (mdgat.py:184-188, 152-155, 392-393, 227-232); weights in fragment order
struct EncoderF64Args {
    const double *in4, *in33;                  // [R][4] x y z saliency, [R][33] FPFH (launch_assemble_f64)
    const double *wk0, *bk0, *wd0, *bd0;       // kenc.0 [32][4], denc.0 [64][33] (BN folded)
    const double *wk1, *bk1, *wk2, *bk2;       // kenc.3 [64][32], kenc.6 [128][64]
    const double *wd1, *bd1;                   // denc.3 [128][64]
    const double *wl, *bl;                     // the encoders' last layers as one product over [hd2 ; hk3]: [128][256]
    const double *wq, *bq;                     // layer 0's q | k | v [384][128], or nullptr (no fp64 layer follows)
    double* x; double* qkv;                    // [R][128], [R][384]
    float* x32;                                // optional fp32 rounding of x (the hand-over when no fp64 layer follows)
    int R;
    unsigned* guard;
};
int launch_encoder_f64(const EncoderF64Args& a, hipStream_t s);
// W [N][K] row-major -> the fragment order the kernels of layer_f64.hip load ([N / 16][ceil(K / 8)][64 lanes][2], zero beyond K); N % 16 == 0
int launch_frag64(const double* W, double* out, int N, int K, hipStream_t s);
inline size_t frag64_doubles(int N, int K) { return (size_t)N * ((K + 7) / 8) * 8; }      // ... and its size (where the images are: weights.hpp)
bool layer_f64_fused();               // mdgat_set_f64_layer_fusion / MDGAT_F64_LAYER_FUSION
// Which form a layer tail or the encoder launch takes and its grid (mdgat_layer_f64_plan, include/mdgat_hip.h: the table of forms and the
// arguments), and how often each form has run in this process (mdgat_layer_f64_launches).  Host code only; the plan touches no HIP call
// unless cus <= 0 asks for the current device's count.  The two launchers above decide by it.
struct LayerF64Plan {
    int form;           // MDGAT_LAYER_F64_*, or -1: no launch
    int workgroups;     // the grid (0: the form is not a launch of layer_f64.hip)
    int rows;           // per workgroup: 16 or 32 (0 likewise)
};
LayerF64Plan layer_f64_plan(int R, int encoder, int has_hid, int chained, int mode, int cus);
void layer_f64_launch_counts(uint64_t counts[MDGAT_LAYER_F64_FORMS]);
void layer_f64_count_unfused(int encoder);      // api.hip: a tail / the encoders done as one product per launch (forms 0 / 6)

// ---- dw_f64.hip: dW = dY^T X [Cout][K0 + K1] and db = colsum(dY) [Cout] of a Conv1d(k=1) Y = X W^T + b, the rows cut into slabs ----
struct DwF64Args {
    const double* dY; int Cout;                  // [R][Cout], Cout a multiple of 16
    const double* x0; int K0;                    // the convolution's input: [R][K0] | [R][K1] (x1: nullptr when K1 == 0)
    const double* x1; int K1;
    const double *bn_mean, *bn_a, *bn_beta;      // [K0]: X = bn_relu(x0) as it is loaded (K1 == 0), or nullptr
    int R, slab;                                 // slab b owns the rows [b slab, min((b + 1) slab, R)): ONE chain per output element, rows ascending
    double* P;                                   // the slabs' partials [ceil(R / slab)][Cout (K0 + K1) + Cout]: dW then db
    double *dW, *db;                             // = P[0] + P[1] + ... in slab order; nullptr: not wanted (without dW no product is formed)
};
int launch_dw_f64(const DwF64Args& a, hipStream_t s);
// the reduction alone, over partials [slabs][nW + nb] that the caller formed (head_grad.hip)
int launch_dw_reduce_f64(const double* P, int slabs, int nW, int nb, double* dW, double* db, hipStream_t s);

// ---- head_grad.hip: the matching head (final_proj and the score matrix, mdgat.py:397, 430-431) as a call of its own, and its backward ----
// desc0 [B][N][128], desc1 [B][M][128], W [128][128], bias [128] -> scores [B][N][M] by tail64's launches; the arguments are the
// caller's to check (api.hip); workspace: match_head_f64_workspace_bytes (both calls), 256-byte aligned
size_t match_head_f64_workspace_bytes(int B, int N, int M);
int launch_match_head_f64(int B, int N, int M, const double* desc0, const double* desc1, const double* W, const double* bias, double* scores,
                          void* workspace, hipStream_t s);
// dscores [B][N][M] -> ddesc0, ddesc1, dW [128][128], dbias [128], each optional (nullptr: not wanted)
int launch_match_head_backward_f64(int B, int N, int M, const double* desc0, const double* desc1, const double* W, const double* bias,
                                   const double* dscores, double* ddesc0, double* ddesc1, double* dW, double* dbias, void* workspace, hipStream_t s);

// ---- attention_grad.hip: the backward of launch_attention_f64 (sel: the forward's selection words, read when topk > 0) ----
// the arguments are the caller's to check (api.hip); workspace: attention_backward_f64_workspace_bytes, 256-byte aligned
size_t attention_backward_f64_workspace_bytes(int B, int N, int M);
int launch_attention_backward_f64(int B, int N, int M, int cross, int topk, const double* qkv, const uint32_t* sel, const double* dmsg, double* dqkv,
                                  void* workspace, hipStream_t s);

// ---- mlp_grad.hip: the reference's MLP (Conv1d(k=1) + batch-statistics BatchNorm + ReLU, mdgat.py:34-46) in training mode, and its backward ----
// the descriptor is the caller's to check (api.hip); saved: what the forward keeps for the backward (mlp_f64_saved_bytes), workspace:
// the backward's own (mlp_f64_backward_workspace_bytes), both 256-byte aligned
size_t mlp_f64_saved_bytes(const mdgat_mlp_desc& d);
size_t mlp_f64_backward_workspace_bytes(const mdgat_mlp_desc& d);
int launch_mlp_forward_f64(const mdgat_mlp_desc& d, const double* x0, const double* x1, double* out, void* saved, hipStream_t s,
                           const double* residual = nullptr);      // residual [R][C_L] contiguous or nullptr (may alias out)
int launch_mlp_backward_f64(const mdgat_mlp_desc& d, const double* x0, const double* x1, const void* saved, const double* dout,
                            const mdgat_mlp_grads& g, void* workspace, hipStream_t s);
