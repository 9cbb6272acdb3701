// C ABI of libmdgat_hip.so (see include/mdgat_hip.h) and the launch sequence of one forward.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "common.hpp"
#include "f64.hpp"
#include "sinkhorn_f64.hpp"
#include "coop_chain.hpp"
#include "loss.hpp"
#include "weights.hpp"
#include "pool_f64.hpp"
#include "ragged.hpp"

// ---------------------------------------------------------------------------------- errors
static thread_local char g_err[512] = "";

void mdgat_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int mdgat_check_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return MDGAT_OK;
    mdgat_set_error("%s: %s", what, hipGetErrorString(e));
    return MDGAT_ERR_HIP;
}

extern "C" const char* mdgat_last_error(void) { return g_err; }

// ---------------------------------------------------------------------------------- blob layout
BlobLayout mdgat_blob_layout(int L) {
    BlobLayout b{};
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o += (n + 3) & ~size_t(3); return r; };
    b.kenc0_w = take(32 * 4);    b.kenc0_b = take(32);
    b.denc0_w = take(64 * 33);   b.denc0_b = take(64);
    b.kenc1_w = take(64 * 32);   b.kenc1_b = take(64);
    b.kenc2_w = take(128 * 64);  b.kenc2_b = take(128);
    b.denc1_w = take(128 * 64);  b.denc1_b = take(128);
    b.encl_w = take(128 * 256);  b.encl_b = take(128);
    b.layer0 = o;
    size_t lo = 0;
    auto ltake = [&](size_t n) { size_t r = lo; lo += (n + 3) & ~size_t(3); return r; };
    b.qkv_w = ltake(384 * 128);  b.qkv_b = ltake(384);
    b.mlp1_w = ltake(256 * 256); b.mlp1_b = ltake(256);
    b.mlp2_w = ltake(128 * 256); b.mlp2_b = ltake(128);
    b.layer_stride = lo;
    o += lo * (size_t)(2 * L);
    b.final_w = take(128 * 128); b.final_b = take(128);
    b.bin_score = take(1);
    b.total = o;
    return b;
}

extern "C" size_t mdgat_blob_floats(int L) { return mdgat_blob_layout(L).total; }

// ---------------------------------------------------------------------------------- handle
struct mdgat_handle {
    mdgat_config cfg{};
    int device = 0;
    DeviceWeights w;     // the device copies of the checkpoint and their layout (weights.hpp)
    bool loaded = false, loaded64 = false;
    double* pool64 = nullptr;       // mdgat_load_pooled_encoder_f64: encoder2 of the pooled descriptor encoder (PoolLayout), else nullptr
    unsigned* host_error = nullptr; // MDGAT_STATUS_WORDS host-mapped words the kernels set (common.hpp): Sinkhorn fallback taken, f16 range guard,
                                    // token of the last forward that matched a frame-0 keypoint
    unsigned match_token = 0;       // the running forward's token (a new one per mdgat_forward / mdgat_forward_frames call, never 0)
    // Two lanes (forward_batched): the second lane's stream and the events that fork it off the caller's stream and join it again
    int lanes = 2;                  // 1 or 2 (mdgat_set_lanes; default 2, MDGAT_FORWARD_LANES)
    int ragged_fp32_slots = 0;      // mdgat_set_ragged_fp32_slots: 1: the fp32-class ragged plan takes slots of up to MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS
    int ragged_sinkhorn = 0;        // mdgat_set_ragged_sinkhorn.  MDGAT_ARITH_FP64: which fp64 Sinkhorn an exact ragged batch runs: 0 resident only, 1 automatic,
                                    // 2 streaming.  MDGAT_ARITH_FP32: non-zero: the ragged forwards run the split form of the fp32 Sinkhorn (split32)
    hipStream_t lane_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // optional per-kernel-class timing of mdgat_forward (mdgat_profile): HIP events on the launch stream of each lane
    bool prof_on = false;
    struct ProfLane { std::vector<hipEvent_t> ev; std::vector<int> cls; size_t n = 0; } prof[2];
    double prof_ms[MDGAT_PROF_CLASSES] = {};
    long long prof_launches[MDGAT_PROF_CLASSES] = {};
    // One forward at a time per handle: the fork / join events, the second lane's stream and the profiling event lists are
    // per-handle state.  Two host threads calling mdgat_forward on one handle from two streams are serialised HERE (the enqueue
    // only - microseconds; the device work of the two calls still overlaps as far as their streams allow), so that one call's
    // lane can never fork off the other call's event record.  (The Python wrapper holds its own lock as well.)
    std::mutex enqueue;
};

extern "C" int mdgat_create(const mdgat_config* cfg, int device, mdgat_handle** out) {
    if (!cfg || !out) { mdgat_set_error("mdgat_create: null argument"); return MDGAT_ERR_BAD_ARG; }
    if (cfg->L < 0 || 2 * cfg->L > MDGAT_MAX_LAYERS) { mdgat_set_error("mdgat_create: L=%d out of range", cfg->L); return MDGAT_ERR_BAD_ARG; }
    if (cfg->attention_mode != MDGAT_ATTENTION_FP32 && cfg->attention_mode != MDGAT_ATTENTION_F16) { mdgat_set_error("mdgat_create: bad attention_mode %d", cfg->attention_mode); return MDGAT_ERR_BAD_ARG; }
    if (cfg->arithmetic != MDGAT_ARITH_FP32 && cfg->arithmetic != MDGAT_ARITH_FP64) { mdgat_set_error("mdgat_create: bad arithmetic %d", cfg->arithmetic); return MDGAT_ERR_BAD_ARG; }
    if (cfg->arithmetic == MDGAT_ARITH_FP64 && cfg->attention_mode != MDGAT_ATTENTION_FP32) { mdgat_set_error("mdgat_create: MDGAT_ARITH_FP64 and MDGAT_ATTENTION_F16 exclude each other"); return MDGAT_ERR_BAD_ARG; }
    if (cfg->arithmetic == MDGAT_ARITH_FP64 && cfg->f64_layers > 2 * cfg->L) { mdgat_set_error("mdgat_create: f64_layers=%d > 2L", cfg->f64_layers); return MDGAT_ERR_BAD_ARG; }
    if (cfg->extract_mode < 0 || cfg->extract_mode > 3) { mdgat_set_error("mdgat_create: bad extract_mode %d", cfg->extract_mode); return MDGAT_ERR_BAD_ARG; }
    for (int i = 0; i < 2 * cfg->L; ++i)
        if (cfg->topk[i] < 0) { mdgat_set_error("mdgat_create: topk[%d] < 0", i); return MDGAT_ERR_BAD_ARG; }
    if (device < 0 || device >= MDGAT_MAX_DEVICES) { mdgat_set_error("mdgat_create: device %d outside 0 .. %d", device, MDGAT_MAX_DEVICES - 1); return MDGAT_ERR_BAD_ARG; }
    hipDeviceProp_t prop;
    if (int rc = mdgat_check_hip(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties")) return rc;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        mdgat_set_error("mdgat_create: device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
        return MDGAT_ERR_UNSUPPORTED;
    }
    mdgat_handle* h = new (std::nothrow) mdgat_handle();
    if (!h) { mdgat_set_error("mdgat_create: out of host memory"); return MDGAT_ERR_HIP; }
    h->cfg = *cfg;
    h->device = device;
    DeviceWeights& w = h->w;
    w.bl = mdgat_blob_layout(cfg->L);
    w.im = mdgat_weight_images(w.bl, cfg->L);
    if (const char* e = getenv("MDGAT_FORWARD_LANES")) h->lanes = atoi(e) == 1 ? 1 : 2;
    int prev = 0;
    (void)hipGetDevice(&prev);
    int rc = mdgat_check_hip(hipSetDevice(device), "hipSetDevice");
    if (!rc) rc = mdgat_check_hip(hipMalloc(&w.blob, w.bl.total * sizeof(float)), "hipMalloc(weights)");
    if (!rc && cfg->arithmetic == MDGAT_ARITH_FP64) rc = mdgat_check_hip(hipMalloc(&w.blob64, w.bl.total * sizeof(double)), "hipMalloc(fp64 weights)");
    if (!rc && cfg->arithmetic == MDGAT_ARITH_FP64) rc = mdgat_check_hip(hipMalloc(&w.frag64, w.im.doubles * sizeof(double)), "hipMalloc(fp64 weight fragments)");
    if (!rc) rc = mdgat_check_hip(hipMalloc(&w.split, w.im.halves * sizeof(_Float16)), "hipMalloc(split weights)");
    if (!rc) rc = mdgat_check_hip(hipMemset(w.split, 0, w.im.halves * sizeof(_Float16)), "hipMemset(split weights)");
    if (!rc) rc = mdgat_check_hip(hipHostMalloc(reinterpret_cast<void**>(&h->host_error), MDGAT_STATUS_WORDS * sizeof(unsigned), hipHostMallocMapped), "hipHostMalloc(status words)");
    if (!rc) for (int i = 0; i < MDGAT_STATUS_WORDS; ++i) h->host_error[i] = 0;
    if (!rc) rc = mdgat_check_hip(hipStreamCreateWithFlags(&h->lane_stream, hipStreamNonBlocking), "hipStreamCreate(lane)");
    if (!rc) rc = mdgat_check_hip(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming), "hipEventCreate");
    if (!rc) rc = mdgat_check_hip(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming), "hipEventCreate");
    (void)hipSetDevice(prev);
    if (rc) {
        mdgat_destroy(h);
        return rc;
    }
    *out = h;
    return MDGAT_OK;
}

// largest integer image of |w| over the blob (NaN / inf on top): the weights become f16 head + f16 residual like every operand
__global__ __launch_bounds__(256) void blob_absmax_kernel(const float* w, size_t n, unsigned* out) {
    unsigned m = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = max(m, __builtin_bit_cast(unsigned, w[i]) & 0x7fffffffu);
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

extern "C" int mdgat_load_weights(mdgat_handle* h, const float* blob, size_t n_floats, int on_device) {
    if (!h || !blob) { mdgat_set_error("mdgat_load_weights: null argument"); return MDGAT_ERR_BAD_ARG; }
    const DeviceWeights& w = h->w;
    if (n_floats != w.bl.total) {
        mdgat_set_error("mdgat_load_weights: blob has %zu floats, expected %zu for L=%d", n_floats, w.bl.total, h->cfg.L);
        return MDGAT_ERR_BAD_ARG;
    }
    if (blob != w.blob) {
        if (int rc = mdgat_check_hip(hipMemcpy(w.blob, blob, n_floats * sizeof(float),
                                               on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice),
                                     "hipMemcpy(weights)"))
            return rc;
    }
    // split-f16 copies of the matrices the MFMA kernels consume (synchronous, like the copy above)
    int prev = 0;
    (void)hipGetDevice(&prev);
    int rc = mdgat_check_hip(hipSetDevice(h->device), "hipSetDevice");
    h->loaded = false;
    if (!rc) {
        // f16 operand range of the WEIGHTS (the kernels guard activations): a weight beyond 6e4 would become an infinite f16 head,
        // and what that makes of the activations a ReLU can turn back into finite garbage (max(NaN, 0) = 0).  The packer brings
        // every rescalable channel to unit scale (pack.py: gauge fixing), so this only fires for checkpoints that are broken or
        // hold non-finite values.
        unsigned* dmax = reinterpret_cast<unsigned*>(w.split);       // (scratch: the split images are written below)
        rc = mdgat_check_hip(hipMemset(dmax, 0, sizeof(unsigned)), "hipMemset(weight range)");
        unsigned hmax = 0;
        if (!rc) {
            hipLaunchKernelGGL(blob_absmax_kernel, dim3(256), dim3(256), 0, nullptr, w.blob, n_floats, dmax);
            rc = mdgat_check_hip(hipMemcpy(&hmax, dmax, sizeof(unsigned), hipMemcpyDeviceToHost), "hipMemcpy(weight range)");
        }
        if (!rc && hmax >= __builtin_bit_cast(unsigned, MDGAT_F16_GUARD)) {
            (void)hipSetDevice(prev);
            mdgat_set_error("mdgat_load_weights: a packed weight is not finite or beyond the f16 operand range (|w| >= 6e4; largest image 0x%08x): "
                            "this checkpoint does not fit the split-f16 arithmetic", hmax);
            return MDGAT_ERR_UNSUPPORTED;
        }
        if (!rc) rc = mdgat_check_hip(hipMemset(dmax, 0, sizeof(unsigned)), "hipMemset(weight range)");
    }
    // every matrix that has a row image (WeightImages), and its fragment image from that
    for (const WeightMat& m : w.im.mats) {
        if (rc || m.row == NO_IMAGE) continue;
        rc = m.kpad ? launch_split_rows_pad(w.blob + m.w, w.split + m.row, m.rows, m.K, m.kpad, nullptr)
                    : launch_split_rows(w.blob + m.w, w.split + m.row, m.rows, m.K, m.pitch, m.nperm, nullptr);
        if (!rc && m.frag != NO_IMAGE) rc = launch_frag_image(w.split + m.row, w.split + m.frag, m.rows, m.K, m.pitch, nullptr);
    }
    if (!rc) rc = mdgat_check_hip(hipDeviceSynchronize(), "split weights");
    (void)hipSetDevice(prev);
    if (rc) return rc;
    h->loaded = true;
    return MDGAT_OK;
}

extern "C" float* mdgat_weights_device_ptr(mdgat_handle* h) { return h ? h->w.blob : nullptr; }
extern "C" double* mdgat_weights_f64_device_ptr(mdgat_handle* h) { return h ? h->w.blob64 : nullptr; }

extern "C" int mdgat_load_weights_f64(mdgat_handle* h, const double* blob, size_t n_doubles, int on_device) {
    if (!h || !blob) { mdgat_set_error("mdgat_load_weights_f64: null argument"); return MDGAT_ERR_BAD_ARG; }
    const DeviceWeights& w = h->w;
    if (!w.blob64) { mdgat_set_error("mdgat_load_weights_f64: the handle was not created with MDGAT_ARITH_FP64"); return MDGAT_ERR_BAD_ARG; }
    if (n_doubles != w.bl.total) {
        mdgat_set_error("mdgat_load_weights_f64: blob has %zu doubles, expected %zu for L=%d", n_doubles, w.bl.total, h->cfg.L);
        return MDGAT_ERR_BAD_ARG;
    }
    h->loaded64 = false;
    if (blob != w.blob64)
        if (int rc = mdgat_check_hip(hipMemcpy(w.blob64, blob, n_doubles * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice),
                                     "hipMemcpy(fp64 weights)"))
            return rc;
    // the layer-tail kernel's copies in fragment order (synchronous, like the copy above)
    int prev = 0;
    (void)hipGetDevice(&prev);
    int rc = mdgat_check_hip(hipSetDevice(h->device), "hipSetDevice");
    for (const WeightMat& m : w.im.mats)
        if (!rc && m.frag64 != NO_IMAGE) rc = launch_frag64(w.blob64 + m.w, w.frag64 + m.frag64, m.rows, m.K, nullptr);
    if (!rc) rc = mdgat_check_hip(hipDeviceSynchronize(), "fp64 weight fragments");
    (void)hipSetDevice(prev);
    if (rc) return rc;
    h->loaded64 = true;
    return MDGAT_OK;
}

// ---- descriptor = 'FPFH_gloabal' (mdgat.py:156-174): encoder2 of the pooled descriptor encoder, beside the blob (pack.py: pack_pooled_encoder) ----
namespace PoolLayout {
constexpr size_t W1E = 0;                      // encoder2.0 (BN folded), the columns that read the keypoint's own e   [256][128]
constexpr size_t W1G = W1E + 256 * 128;        // ... the columns that read the frame maximum g                         [256][128]
constexpr size_t B1 = W1G + 256 * 128;         // its bias                                                              [256]
constexpr size_t W2K = B1 + 256;               // [encoder2.3 | kenc.9] over [hidden (256) ; hk3 (128)]                 [128][384]
constexpr size_t B2 = W2K + 128 * 384;         // encoder2.3.bias + kenc.9.bias                                         [128]
constexpr size_t TOTAL = B2 + 128;
}

extern "C" size_t mdgat_pooled_encoder_doubles(void) { return PoolLayout::TOTAL; }

extern "C" int mdgat_load_pooled_encoder_f64(mdgat_handle* h, const double* w, size_t n_doubles, int on_device) {
    const char* who = "mdgat_load_pooled_encoder_f64";
    if (!h || !w) { mdgat_set_error("%s: null argument", who); return MDGAT_ERR_BAD_ARG; }
    if (h->cfg.arithmetic != MDGAT_ARITH_FP64) { mdgat_set_error("%s: the handle was not created with MDGAT_ARITH_FP64 (the pooled encoder runs on the fp64 products)", who); return MDGAT_ERR_BAD_ARG; }
    if (n_doubles != PoolLayout::TOTAL) { mdgat_set_error("%s: %zu doubles, expected %zu", who, n_doubles, PoolLayout::TOTAL); return MDGAT_ERR_BAD_ARG; }
    int prev = 0;
    (void)hipGetDevice(&prev);
    int rc = mdgat_check_hip(hipSetDevice(h->device), "hipSetDevice");
    if (!rc && !h->pool64) rc = mdgat_check_hip(hipMalloc(&h->pool64, PoolLayout::TOTAL * sizeof(double)), "hipMalloc(pooled encoder)");
    if (!rc) rc = mdgat_check_hip(hipMemcpy(h->pool64, w, n_doubles * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice), "hipMemcpy(pooled encoder)");
    (void)hipSetDevice(prev);
    return rc;
}

extern "C" void mdgat_destroy(mdgat_handle* h) {
    if (!h) return;
    for (void* p : {(void*)h->w.blob, (void*)h->w.split, (void*)h->w.blob64, (void*)h->w.frag64, (void*)h->pool64})
        if (p) (void)hipFree(p);
    if (h->host_error) (void)hipHostFree(h->host_error);
    if (h->lane_stream) { (void)hipStreamSynchronize(h->lane_stream); (void)hipStreamDestroy(h->lane_stream); }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    for (auto& pl : h->prof)
        for (hipEvent_t e : pl.ev) (void)hipEventDestroy(e);
    delete h;
}

// ---------------------------------------------------------------------------------- workspace
namespace {
struct Workspace {
    float *x, *qkv, *hid, *msg, *scores, *Z; _Float16* qkv16;
    char* sk; size_t sk_bytes;             // the fp32 Sinkhorn's workspace (0: the shape is beyond its cluster kernel)
    double *x64, *qkv64, *hid64, *msg64;   // MDGAT_ARITH_FP64 only: the residual stream, q|k|v, hidden layer and message of the fp64 layers
    double* scores64;                      // ... the fp64 score matrix [B][N][M]: q | k | v's room where it fits, its own beyond (frames past ~770 keypoints)
    char* sk64; size_t sk64_bytes;         // ... and the workspace of the fp64 Sinkhorn (0: the shape is beyond that kernel), its arg-max arrays behind it
    char* loss; size_t loss_bytes;         // a forward with a loss request (mdgat_forward_loss): the loss kernels' workspace ...
    double* Z64;                           // ... and on an exact-mode handle, whose fp64 tail hands the loss the fp64 Z, room for that Z
    char* sksplit; size_t sksplit_bytes;   // the scratch of the fp32 Sinkhorn's split form (an MDGAT_ARITH_FP32 handle that opted in: split32; 0: the slot has one slab)
    size_t total;   // bytes
};
// sk64: a form of the fp64 Sinkhorn to hold beside the one a uniform call runs at this shape (sinkhorn_f64_form) - a ragged call's, which
// mdgat_set_ragged_sinkhorn can put on the streaming form at sizes where the uniform forward runs the resident one
// split32: room for the split form of the fp32 Sinkhorn, behind everything else
// wide32: ... sized for wide slots (mdgat_set_ragged_fp32_slots)
Workspace carve(void* base, int B, int N, int M, bool f64, bool loss, Sk64Form sk64 = Sk64Form::unsupported, bool split32 = false, bool wide32 = false) {
    const size_t R = (size_t)B * (N + M);
    Workspace w{};
    WsCarver c{static_cast<char*>(base)};
    c.take(w.x, R * 128);
    c.take(w.qkv, R * 384);   // qkv and hid are contiguous: the encoder uses them as one scratch area
    c.take(w.hid, R * 256);
    c.take(w.msg, R * 128);
    c.take(w.scores, (size_t)B * N * M);
    c.take(w.Z, (size_t)B * (N + 1) * (M + 1));
    w.sk_bytes = sinkhorn_cluster_workspace_bytes(B, N, M);
    c.take(w.sk, w.sk_bytes);
    c.take(w.qkv16, mdgat_qkv16_halves(B, N, M));
    if (f64) {
        c.take(w.x64, R * 128);
        c.take(w.qkv64, R * 384);     // qkv64 and hid64 are contiguous: the encoder stages live there
        c.take(w.hid64, R * 256);
        c.take(w.msg64, R * 128);
        const size_t uniform = sinkhorn_f64_workspace_bytes(B, N, M, sinkhorn_f64_form(N, M, false, 0)), beside = sinkhorn_f64_workspace_bytes(B, N, M, sk64);
        w.sk64_bytes = beside > uniform ? beside : uniform;      // (0: the shape is beyond both forms)
        c.take(w.sk64, w.sk64_bytes ? w.sk64_bytes + sinkhorn_f64_bests(nullptr, B, N, M).bytes : 0);
        if ((size_t)N * M <= (size_t)384 * (N + M) || !w.sk64_bytes) w.scores64 = w.qkv64;
        else c.take(w.scores64, (size_t)B * N * M);
    }
    if (loss) {
        w.loss_bytes = loss_workspace_bytes(B, N, M);
        c.take(w.loss, w.loss_bytes);
        if (f64) c.take(w.Z64, (size_t)B * (N + 1) * (M + 1));
    }
    if (split32) {
        w.sksplit_bytes = sinkhorn_split_workspace_bytes(B, N, M, wide32);
        c.take(w.sksplit, w.sksplit_bytes);
    }
    w.total = c.bytes;
    return w;
}
}  // namespace


// ---------------------------------------------------------------------------------- ragged batches
// every per-pair check of a ragged batch (ragged.hpp), for every entry that takes one
int mdgat_check_ragged(const char* who, int B, int Np, int Mp, const RaggedCounts& c, const RaggedStarts* bank, const int* topk, int ntopk, int* cnt_min) {
    if (!c.cnt0 || !c.cnt1 || !c.host0 || !c.host1) { mdgat_set_error("%s: null counts pointer", who); return MDGAT_ERR_BAD_ARG; }
    if (bank && (!bank->start0 || !bank->start1 || !bank->host0 || !bank->host1)) { mdgat_set_error("%s: null starts pointer", who); return MDGAT_ERR_BAD_ARG; }
    int cmin = Np < Mp ? Np : Mp;
    for (int b = 0; b < B; ++b) {
        const int n = c.host0[b], m = c.host1[b], keys = n < m ? n : m;
        if (n < 1 || n > Np || m < 1 || m > Mp) {
            mdgat_set_error("%s: pair %d has %d x %d keypoints, outside 1 .. %d x 1 .. %d", who, b, n, m, Np, Mp);
            return MDGAT_ERR_BAD_ARG;
        }
        for (int i = 0; i < ntopk; ++i)
            if (topk[i] > keys) {      // torch.topk raises (mdgat.py:202)
                if (ntopk > 1) mdgat_set_error("%s: pair %d: k=%d exceeds the number of keys (%d), layer %d", who, b, topk[i], keys, i);
                else mdgat_set_error("%s: pair %d: k=%d exceeds the number of keys (%d)", who, b, topk[i], keys);
                return MDGAT_ERR_BAD_ARG;
            }
        if (bank) {
            // (the pair's records lie inside the bank: the kernel reads rows start .. start + count - 1 and no others)
            const long long s0 = bank->host0[b], s1 = bank->host1[b];
            if (s0 < 0 || s0 + n > bank->rows0 || s1 < 0 || s1 + m > bank->rows1) {
                mdgat_set_error("%s: pair %d reads records %lld .. %lld of %lld and %lld .. %lld of %lld: outside the bank", who, b, s0, s0 + n,
                                bank->rows0, s1, s1 + m, bank->rows1);
                return MDGAT_ERR_BAD_ARG;
            }
        }
        cmin = keys < cmin ? keys : cmin;
    }
    if (cnt_min) *cnt_min = cmin;
    return MDGAT_OK;
}

// ---------------------------------------------------------------------------------- forward
// inputs of a forward: six fp32 arrays, or raw 37-float frame records, or (MDGAT_ARITH_FP64) six fp64 arrays
struct FwdIn {
    const float *kpts0 = nullptr, *sigma0 = nullptr, *fpfh0 = nullptr, *kpts1 = nullptr, *sigma1 = nullptr, *fpfh1 = nullptr;
    const float *rec0 = nullptr, *rec1 = nullptr;
    int normalize_fpfh = 0;
    const double *dk0 = nullptr, *ds0 = nullptr, *df0 = nullptr, *dk1 = nullptr, *ds1 = nullptr, *df1 = nullptr;
    // a ragged batch (mdgat_forward_f64_ragged): the pairs' own keypoint counts in slots of N / M; out of a bank of records
    // (mdgat_forward_frames_ragged): rec0 / rec1 are the bank's, indexed by the starts (ragged.hpp); kp0_out / kp1_out (optional): the
    // padded float32 keypoints [B][N][3] / [B][M][3] the assemble kernel writes for the steps behind the matcher
    RaggedCounts counts;
    RaggedStarts bank;
    float *kp0_out = nullptr, *kp1_out = nullptr;
    static FwdIn arrays(const float* k0, const float* s0, const float* f0, const float* k1, const float* s1, const float* f1) {
        FwdIn in; in.kpts0 = k0; in.sigma0 = s0; in.fpfh0 = f0; in.kpts1 = k1; in.sigma1 = s1; in.fpfh1 = f1; return in;
    }
    static FwdIn arrays(const double* k0, const double* s0, const double* f0, const double* k1, const double* s1, const double* f1) {
        FwdIn in; in.dk0 = k0; in.ds0 = s0; in.df0 = f0; in.dk1 = k1; in.ds1 = s1; in.df1 = f1; return in;
    }
    // the same inputs from pair c on (slices of a batch)
    FwdIn from(size_t c, int N, int M) const {
        auto o = [](auto* q, size_t n) { return q ? q + n : q; };
        return FwdIn{o(kpts0, c * N * 3), o(sigma0, c * N), o(fpfh0, c * N * 33), o(kpts1, c * M * 3), o(sigma1, c * M), o(fpfh1, c * M * 33),
                     o(rec0, bank ? 0 : c * N * 37), o(rec1, bank ? 0 : c * M * 37), normalize_fpfh,      // (a bank is indexed by the starts)
                     o(dk0, c * N * 3), o(ds0, c * N), o(df0, c * N * 33), o(dk1, c * M * 3), o(ds1, c * M), o(df1, c * M * 33),
                     counts.from(c), bank.from(c), o(kp0_out, c * N * 3), o(kp1_out, c * M * 3)};
    }
};

// outputs of a forward: matches, matching scores, Z (optional) and the loss (mdgat_forward_loss)
struct FwdOut {
    int64_t *matches0, *matches1;
    float *mscores0, *mscores1, *Z;
    bool loss;
    mdgat_loss_request lr;
    // the same outputs from pair c on
    FwdOut from(size_t c, int N, int M) const {
        FwdOut o = *this;
        o.matches0 += c * N; o.matches1 += c * M; o.mscores0 += c * N; o.mscores1 += c * M;
        if (Z) o.Z += c * (N + 1) * (M + 1);
        if (loss) { o.lr.gt0 += c * N; o.lr.gt1 += c * M; o.lr.loss += c; }
        return o;
    }
};

// MDGAT_ARITH_FP64: the number of leading propagation layers that run in fp64 (mdgat_config.f64_layers)
static int f64_layer_count(const mdgat_config& cfg) {
    if (cfg.f64_layers > 0) return cfg.f64_layers;
    if (cfg.f64_layers < 0) return 0;       // MDGAT_F64_ENCODERS_ONLY
    int n = 0;
    for (int i = 0; i < 2 * cfg.L; ++i)
        if (cfg.topk[i] > 0) n = i + 1;
    return n;
}

// Batches run in slices on two lanes.  Pairs are independent.  (i) A slice of ~64 pairs fills the part (512 tiles of the
// layer kernel, 2048 workgroups of the attention kernel, one Sinkhorn workgroup per CU at N = M = 512) while its working set
// (q / k / v: 1.6 MB per pair and layer) still fits the 256 MB Infinity Cache between the kernel that writes it and the one
// that reads it, which a batch of 128 no longer does (20 400 pairs/s at B = 64 against 19 100-19 500 at B = 128 ... 512).
// (ii) Round 3: the kernels of ONE forward run back to back with synchronised phases (every layer workgroup loads its tile
// at the same moment, every launch has a tail, the Sinkhorn kernel mostly waits for its partners); two half-size forwards
// on two streams fill each other's gaps: 2 x 32 pairs in flight 21 300 pairs/s against 20 500 for 1 x 64 on the same box
// (tools/overlap_streams.py; 2 x 20 against 1 x 40: 20 300 / 16 350 - a single launch of 1.25 tile rounds has a long tail).
// So: a batch of more than MDGAT_FORWARD_SLICE_POINTS (32 768) keypoints is cut into an EVEN number of balanced slices of at
// most that many, which alternate between the caller's stream and the handle's second stream (forked from and joined to the
// caller's stream by events: the call stays asynchronous and ordered on the caller's stream); each lane has its own half of
// the workspace.  The one batch-wide rule of the reference, mdgat.py:465-467, is applied over the whole batch afterwards.
// Taps (whole-batch layouts) run unsliced; mdgat_set_lanes(h, 1) / MDGAT_FORWARD_LANES=1 keeps everything on the caller's stream
// (slices of 65 536 keypoints beyond 1.5 x that).
struct LanePlan { int nslices, per, lanes; size_t lane_bytes; };
static LanePlan lane_plan(int lanes, int B, int N, int M, bool f64, bool loss) {
    static const long env_points = [] { const char* e = getenv("MDGAT_FORWARD_SLICE_POINTS"); return e ? atol(e) : -1L; }();   // unset: defaults; 0: never slice
    LanePlan p{1, B, 1, 0};
    const long per_pair = (long)N + M;
    if (B <= 1 || per_pair <= 0 || env_points == 0) return p;
    const long total = (long)B * per_pair;
    if (lanes >= 2) {
        const long pts = env_points > 0 ? env_points : 32768L;
        if (total <= pts) return p;
        long n = 2 * ((total + 2 * pts - 1) / (2 * pts));
        if (n > B) n = B;
        p.nslices = (int)n;
        p.per = (int)((B + n - 1) / n);
        p.nslices = (B + p.per - 1) / p.per;
        p.lanes = p.nslices >= 2 ? 2 : 1;
    } else {
        const long pts = env_points > 0 ? env_points : 65536L;
        long slice = pts / per_pair;
        if (slice < 1) slice = 1;
        if ((long)B <= slice + slice / 2) return p;
        const long n = (B + slice - 1) / slice;
        p.per = (int)((B + n - 1) / n);
        p.nslices = (B + p.per - 1) / p.per;
    }
    p.lane_bytes = carve(nullptr, p.per, N, M, f64, loss).total;
    return p;
}

static size_t workspace_bytes(const mdgat_handle* h, int B, int N, int M, bool loss) {
    if (B <= 0 || N <= 0 || M <= 0) return 0;
    // (taps run unsliced: the whole batch's workspace is the lower bound in every case)
    const bool f64 = h && h->cfg.arithmetic == MDGAT_ARITH_FP64;
    // (this knows nothing of the call to come: it holds the form an exact ragged batch in slots of N x M would run on this handle -
    // mdgat_set_ragged_sinkhorn - beside the uniform call's, so the streaming form's K is there whenever a ragged call could need it)
    // (on an MDGAT_ARITH_FP32 handle that opted in, likewise: the scratch of the split form a ragged batch in these slots would run)
    const bool split32 = h && h->cfg.arithmetic == MDGAT_ARITH_FP32 && h->ragged_sinkhorn != 0;
    const size_t whole = carve(nullptr, B, N, M, f64, loss, sinkhorn_f64_form(N, M, true, h ? h->ragged_sinkhorn : 0), split32, h && h->ragged_fp32_slots != 0).total;
    const LanePlan p = lane_plan(h ? h->lanes : 2, B, N, M, f64, loss);
    const size_t laned = p.lane_bytes * (size_t)p.lanes;
    return whole > laned ? whole : laned;
}

extern "C" size_t mdgat_workspace_bytes(const mdgat_handle* h, int B, int N, int M) { return workspace_bytes(h, B, N, M, false); }
extern "C" size_t mdgat_forward_loss_workspace_bytes(const mdgat_handle* h, int B, int N, int M) { return workspace_bytes(h, B, N, M, true); }

// (an MDGAT_ARITH_FP32 handle: non-zero selects the split form of the fp32 Sinkhorn for its ragged forwards - Path::split32)
extern "C" int mdgat_set_ragged_sinkhorn(mdgat_handle* h, int mode) {
    if (!h || mode < 0 || mode > 2) { mdgat_set_error("mdgat_set_ragged_sinkhorn: mode must be 0 (resident), 1 (automatic) or 2 (streaming)"); return -1; }
    const int prev = h->ragged_sinkhorn;
    h->ragged_sinkhorn = mode;
    return prev;
}

// the slots of the fp32-class ragged plan (mdgat_forward_ragged and every entry that runs its plan): 0 up to MDGAT_RAGGED_FP32_MAX_KEYPOINTS, today's
// kernels and bits; 1 up to MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS - slots within 512 x 512 run what they run under 0.  Size the workspace afterwards.
extern "C" int mdgat_set_ragged_fp32_slots(mdgat_handle* h, int mode) {
    if (!h || mode < 0 || mode > 1) { mdgat_set_error("mdgat_set_ragged_fp32_slots: mode must be 0 (512 keypoints per frame) or 1 (wide: 2048)"); return -1; }
    const int prev = h->ragged_fp32_slots;
    h->ragged_fp32_slots = mode;
    return prev;
}

extern "C" int mdgat_set_lanes(mdgat_handle* h, int lanes) {
    if (!h || lanes < 1 || lanes > 2) { mdgat_set_error("mdgat_set_lanes: lanes must be 1 or 2"); return MDGAT_ERR_BAD_ARG; }
    h->lanes = lanes;
    return MDGAT_OK;
}

// How a call runs, decided once for all its slices.
struct Path {
    bool f64;         // MDGAT_ARITH_FP64 (f64.hip): the inputs, encoders and leading layers in the reference's arithmetic
    int first;        // the first propagation layer the fp32-class kernels run (2L: none)
    bool tail64;      // MDGAT_ARITH_FP64: final_proj, scores, Sinkhorn and the extraction's arg-maxes in fp64 too
    bool fused64;     // the fp64 encoders and layer tails as fused launches, the last one writing the hand-over to fp32
    bool cluster32;   // the fp32 Sinkhorn's cluster kernel (N, M <= 2048): arg-maxes fused, Z only materialised when something reads it
    int cnt_min;      // a ragged batch (FwdIn::counts): the smallest keypoint count of any frame; 0 otherwise
    Sk64Form sk64;    // the form of the fp64 Sinkhorn this call runs if it has the fp64 tail (sinkhorn_f64_form; a ragged batch: by mdgat_set_ragged_sinkhorn)
    bool wide32;      // a ragged batch on the fp32-class plan of a handle in mode 1 of mdgat_set_ragged_fp32_slots: the wide launchers, the wide split scratch
    bool split32;     // a ragged batch on an MDGAT_ARITH_FP32 handle that opted in (mdgat_set_ragged_sinkhorn non-zero): the fp32 Sinkhorn's split form
                      // wherever the slot has two slabs of rows or more (sinkhorn_plan decides), its scratch in the workspace
    LanePlan lanes;
};

// Every check of a forward call, before anything is enqueued, and its Path.
static int plan_forward(mdgat_handle* h, int B, int N, int M, const FwdIn& in, const FwdOut& out, const mdgat_taps* taps,
                        const void* workspace, size_t workspace_bytes, Path& p) {
    if (!h) { mdgat_set_error("mdgat_forward: null handle"); return MDGAT_ERR_BAD_ARG; }
    if (out.loss) {
        const int lm = out.lr.method;
        if (lm != MDGAT_LOSS_SUPERGLUE && lm != MDGAT_LOSS_TRIPLET && lm != MDGAT_LOSS_GAP) { mdgat_set_error("mdgat_forward_loss: bad method %d", lm); return MDGAT_ERR_BAD_ARG; }
        if (!out.lr.gt0 || !out.lr.gt1 || !out.lr.loss) { mdgat_set_error("mdgat_forward_loss: null pointer in the loss request"); return MDGAT_ERR_BAD_ARG; }
        if (lm != MDGAT_LOSS_GAP && N != M) {
            mdgat_set_error("mdgat_forward_loss: the superglue and triplet losses need N == M (N=%d M=%d), as the reference's do", N, M);
            return MDGAT_ERR_BAD_ARG;
        }
    }
    // fp64 inputs, or raw float32 records on a handle that computes in fp64 (the loader's own sequence: float32 records, FPFH
    // normalised in float32, widened to double - load_data.py:146-165, 290-295); past these checks, exactly on an exact-mode handle
    const bool f64 = in.dk0 != nullptr || (in.rec0 != nullptr && h->cfg.arithmetic == MDGAT_ARITH_FP64);
    if (!h->loaded) { mdgat_set_error("mdgat_forward: weights not loaded"); return MDGAT_ERR_NO_WEIGHTS; }
    if (f64 && (h->cfg.arithmetic != MDGAT_ARITH_FP64 || !h->loaded64)) {
        mdgat_set_error("mdgat_forward_f64: the handle needs MDGAT_ARITH_FP64 and mdgat_load_weights_f64");
        return h->cfg.arithmetic != MDGAT_ARITH_FP64 ? MDGAT_ERR_BAD_ARG : MDGAT_ERR_NO_WEIGHTS;
    }
    if (!f64 && h->cfg.arithmetic == MDGAT_ARITH_FP64) {
        mdgat_set_error("mdgat_forward: this handle computes in fp64 (MDGAT_ARITH_FP64): call mdgat_forward_f64 with fp64 inputs");
        return MDGAT_ERR_BAD_ARG;
    }
    if (static_cast<volatile unsigned*>(h->host_error)[MDGAT_STATUS_RANGE]) {
        // the forward is asynchronous: what an earlier launch found surfaces here unless the caller asked first
        // (mdgat_async_status after its own synchronisation - MDGAT.forward does)
        h->host_error[MDGAT_STATUS_RANGE] = 0;
        mdgat_set_error("mdgat_forward: a previous call on this handle met activations outside the f16 operand range (|v| >= 6e4; fp64 "
                        "layers of the exact mode: |v| >= 2^500) or non-finite values; its outputs are invalid");
        return MDGAT_ERR_UNSUPPORTED;
    }
    if (B <= 0 || N <= 0 || M <= 0) { mdgat_set_error("mdgat_forward: empty batch/keypoints (B=%d N=%d M=%d) must be handled by the caller", B, N, M); return MDGAT_ERR_BAD_ARG; }
    const bool arrays = in.kpts0 && in.sigma0 && in.fpfh0 && in.kpts1 && in.sigma1 && in.fpfh1;
    const bool arrays64 = in.dk0 && in.ds0 && in.df0 && in.dk1 && in.ds1 && in.df1;
    if ((!arrays && !(in.rec0 && in.rec1) && !arrays64) || !out.matches0 || !out.matches1 || !out.mscores0 || !out.mscores1 || !workspace) {
        mdgat_set_error("mdgat_forward: null pointer argument");
        return MDGAT_ERR_BAD_ARG;
    }
    p.lanes = (taps || in.counts) ? LanePlan{1, B, 1, 0} : lane_plan(h->lanes, B, N, M, f64, out.loss);
    p.sk64 = f64 ? sinkhorn_f64_form(N, M, (bool)in.counts, h->ragged_sinkhorn) : Sk64Form::unsupported;
    p.split32 = in.counts && !f64 && h->cfg.arithmetic == MDGAT_ARITH_FP32 && h->ragged_sinkhorn != 0;
    p.wide32 = in.counts && h->ragged_fp32_slots != 0;
    const size_t need = p.lanes.nslices > 1 ? p.lanes.lane_bytes * (size_t)p.lanes.lanes : carve(nullptr, B, N, M, f64, out.loss, p.sk64, p.split32, p.wide32).total;
    if (workspace_bytes < need) { mdgat_set_error("mdgat_forward: workspace %zu < %zu bytes", workspace_bytes, need); return MDGAT_ERR_BAD_ARG; }
    if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0) { mdgat_set_error("mdgat_forward: workspace must be 256-byte aligned"); return MDGAT_ERR_BAD_ARG; }
    const int L2 = 2 * h->cfg.L;
    for (int i = 0; i < L2; ++i) {
        const int k = h->cfg.topk[i];
        if (k > 0 && (k > N || k > M)) {   // torch.topk raises (mdgat.py:202)
            mdgat_set_error("layer %d: dynamic attention k=%d exceeds the number of keys (N=%d, M=%d)", i, k, N, M);
            return MDGAT_ERR_BAD_ARG;
        }
    }
    // The TAIL in fp64 as well (mdgat_config.f64_sinkhorn; round 6): every layer, final_proj, the score matrix and the optimal
    // transport in the reference's own arithmetic, every arg-max of the extraction decided on the fp64 Z (sinkhorn_f64.hip).  With
    // the fp32-class tail Z is good to 7e-6 - inside the bar of 1e-4, but among 40 960 arg-maxes of a reference-held batch one had
    // its two candidates 1.3e-6 apart and fell the other way (profiles/NOTES_r6.md section 11).
    if (f64 && h->cfg.f64_sinkhorn > 0 && !sinkhorn_f64_supported(N, M)) {
        mdgat_set_error("mdgat_forward_f64: f64_sinkhorn = 1 and %d x %d keypoints are beyond the fp64 Sinkhorn kernels (2175)", N, M);
        return MDGAT_ERR_UNSUPPORTED;
    }
    p.f64 = f64;
    p.tail64 = f64 && h->cfg.f64_sinkhorn >= 0 && sinkhorn_f64_supported(N, M) && h->cfg.f64_layers == 0;
    p.first = p.tail64 ? L2 : f64 ? f64_layer_count(h->cfg) : 0;
    // The tail of a layer - mlp.0 + ReLU, mlp.3 + residual (mdgat.py:246-248, 274) - and the NEXT layer's q | k | v projection
    // (227-232) run as one launch (layer_f64.hip), the hidden activation never leaving the chip, and so do the two encoders with
    // layer 0's projection; the last fp64 launch also writes the fp32 rounding of x, the hand-over.  mdgat_set_f64_layer_fusion(0)
    // keeps the one-product-per-launch form (bit-identical).
    p.fused64 = f64 && layer_f64_fused() && h->w.frag64;
    p.cluster32 = sinkhorn_cluster_workspace_bytes(B, N, M) != 0;
    p.cnt_min = 0;
    // An fp64 handle that runs the encoders ALONE in fp64 - f64_layers = MDGAT_F64_ENCODERS_ONLY, f64_sinkhorn off, the pooled encoder
    // loaded: what a float32 'FPFH_gloabal' module creates - hands over to the fp32-class kernels right behind them (p.first == 0): its
    // ragged batches run the fp32-class branch below behind head64's ragged assemble kernels and the pooled encoder, whose frame maximum
    // is taken over a pair's own counts.  (An exact handle with an fp32-class tail keeps the refusal of the branch behind.)
    const bool enc_only64 = f64 && !p.tail64 && p.first == 0 && h->pool64 && h->cfg.f64_layers < 0 && h->cfg.f64_sinkhorn < 0;
    if (in.counts && (!f64 || enc_only64)) {
        // The ragged plan's fp32-class branch (mdgat_forward_ragged; mdgat_forward_frames_ragged on an MDGAT_ARITH_FP32 handle): the encoder,
        // the general attention kernel and the streaming Sinkhorn take the counts (their RAGGED instantiations; out of a bank the encoder's
        // BANK one, which reads the records itself) in slots of at most MDGAT_RAGGED_FP32_MAX_KEYPOINTS, the row-wise launches in between run
        // over the padded rows, which the encoder makes from zeros.  One unsliced lane, no taps, no loss; the single-f16 attention mode has
        // no kernel that takes counts.  The counts - and the starts into a bank - are checked on their host copies before anything is enqueued.
        const char* who = in.bank ? "mdgat_forward_frames_ragged" : f64 ? "mdgat_forward_f64_ragged" : "mdgat_forward_ragged";
        p.sk64 = Sk64Form::unsupported;      // (mdgat_set_ragged_sinkhorn is the exact tail's: this branch has no fp64 Sinkhorn)
        if (taps || out.loss) { mdgat_set_error("%s: taps and the loss are not supported on a ragged batch", who); return MDGAT_ERR_UNSUPPORTED; }
        if (in.rec0 && !in.bank) { mdgat_set_error("%s: fp32 arrays only (no frame records)", who); return MDGAT_ERR_UNSUPPORTED; }
        if (h->cfg.attention_mode == 1) { mdgat_set_error("%s: attention_mode = 1 (single-f16 products) takes no per-pair counts", who); return MDGAT_ERR_UNSUPPORTED; }
        const int limit = p.wide32 ? MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS : MDGAT_RAGGED_FP32_MAX_KEYPOINTS;      // (mdgat_set_ragged_fp32_slots)
        if (N > limit || M > limit) {
            mdgat_set_error("%s: padded sizes %d x %d: fp32 ragged batches hold at most %d keypoints per frame", who, N, M, limit);
            return MDGAT_ERR_UNSUPPORTED;
        }
        if (int rc = mdgat_check_ragged(who, B, N, M, in.counts, in.bank ? &in.bank : nullptr, h->cfg.topk, L2, &p.cnt_min)) return rc;
    } else if (in.counts) {
        // The ragged plan: the kernels that take per-pair counts are the exact mode's with its fp64 tail on the register-resident Sinkhorn;
        // the batch runs unsliced on the caller's stream (p.lanes above, like a call with taps); the counts (and the starts into a bank)
        // are checked on their host copies, against the whole k schedule (mdgat_check_ragged).
        const char* who = in.bank ? "mdgat_forward_frames_ragged" : "mdgat_forward_f64_ragged";
        if (taps || out.loss) { mdgat_set_error("%s: taps and the loss are not supported on a ragged batch", who); return MDGAT_ERR_UNSUPPORTED; }
        if (h->ragged_sinkhorn != 0 && p.sk64 != Sk64Form::resident) {
            // the handle opted in (mdgat_set_ragged_sinkhorn: mode 2, or mode 1 where the resident form takes no counts): the streaming
            // Sinkhorn's RAGGED instantiations behind the same kernels, in slots up to the dynamic fp64 attention's limit
            if (!p.tail64 || N > MDGAT_RAGGED_WIDE_MAX_KEYPOINTS || M > MDGAT_RAGGED_WIDE_MAX_KEYPOINTS || p.sk64 != Sk64Form::streaming) {
                mdgat_set_error("%s: ragged batches on the streaming Sinkhorn need the fp64 tail: f64_sinkhorn not off, f64_layers automatic, and at most "
                                "%d keypoints per frame (Np=%d, Mp=%d)", who, MDGAT_RAGGED_WIDE_MAX_KEYPOINTS, N, M);
                return MDGAT_ERR_UNSUPPORTED;
            }
        } else
        if (!p.tail64 || N > MDGAT_RAGGED_MAX_KEYPOINTS || M > MDGAT_RAGGED_MAX_KEYPOINTS || p.sk64 != Sk64Form::resident) {
            mdgat_set_error("%s: ragged batches need the fp64 tail on the register-resident Sinkhorn: f64_sinkhorn not off, f64_layers automatic, "
                            "mdgat_set_f64_sinkhorn_form not 1, and at most %d keypoints per frame (Np=%d, Mp=%d)", who, MDGAT_RAGGED_MAX_KEYPOINTS, N, M);
            return MDGAT_ERR_UNSUPPORTED;
        }
        if (int rc = mdgat_check_ragged(who, B, N, M, in.counts, in.bank ? &in.bank : nullptr, h->cfg.topk, L2, &p.cnt_min)) return rc;
    }
    return MDGAT_OK;
}

// What the stages of one forward share: a slice of the call on one lane.
struct Fwd {
    const mdgat_handle* h;
    const Path& p;
    int B, N, M, R;
    Workspace ws;
    Qkv16 q16;               // ws.qkv16 in the attention kernel's layout
    hipStream_t s;
    unsigned* status;        // the handle's status words (device view)
    mdgat_taps taps;         // all null when the call has none
    mdgat_handle::ProfLane& pl;
    int defer_alldust;       // a slice: the batch-wide rule is applied after the last one
    const int *cnt0, *cnt1;  // a ragged batch (FwdIn::counts): null otherwise
    int cnt_min;             // Path::cnt_min
    unsigned* guard() const { return status + MDGAT_STATUS_RANGE; }
    // profiling (off by default): an event after every launch on this lane's stream; the intervals are attributed to the
    // kernel classes after the whole batch has been enqueued (prof_collect), which then ends with a synchronisation
    void mark(int cls) {
        if (!h->prof_on) return;
        if (pl.n == pl.ev.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return;
            pl.ev.push_back(e);
        }
        (void)hipEventRecord(pl.ev[pl.n++], s);
        pl.cls.push_back(cls);
    }
    // a tap (to == nullptr: not asked for): fp32 stages copied, fp64 ones rounded to fp32
    int tap(float* to, const float* from, size_t n, const char* what) const { return to ? mdgat_check_hip(hipMemcpyAsync(to, from, n * sizeof(float), hipMemcpyDeviceToDevice, s), what) : MDGAT_OK; }
    int tap(float* to, const double* from, size_t n) const { return to ? launch_f64_to_f32(from, to, n, nullptr, s) : MDGAT_OK; }
    float* x_tap(int layer) const { return taps.x_layers ? taps.x_layers + (size_t)layer * R * 128 : nullptr; }
    uint32_t* sel_tap(int layer) const { return taps.topk_sel ? taps.topk_sel + (size_t)layer * mdgat_topk_sel_words(B, N, M) : nullptr; }
    SkExtract extract(const FwdOut& o) const {
        return SkExtract{h->cfg.extract_mode, h->cfg.match_threshold, o.matches0, o.matches1, o.mscores0, o.mscores1, defer_alldust,
                         status + MDGAT_STATUS_MATCHED + (h->match_token % MDGAT_MATCH_SLOTS), h->match_token};
    }
    // the loss (mdgat.py:486-594) on the tail's Z, fp64 or fp32 widened to fp64, if the call asked for it; its time is attributed to no class
    template <typename T> int loss(const FwdOut& o, const T* Z) {
        if (!o.loss) return MDGAT_OK;
        if (int rc = launch_loss(B, N, M, Z, o.lr.gt0, o.lr.gt1, o.lr.method, o.lr.gamma, o.lr.loss, o.lr.bad_index, ws.loss, ws.loss_bytes, s)) return rc;
        mark(-1);
        return MDGAT_OK;
    }
    // an fp64 product over all R rows with matrix m of the fp64 blob: C [R][m.rows] = act([A0 (K0 columns) | A1] W^T + b) (+ Rs)
    int gemm64(const WeightMat& m, const double* A0, int K0, const double* A1, int lda1, int relu, const double* Rs, double* C) const {
        const double* w64 = h->w.blob64;
        const GemmF64Args g{A0, K0, K0, A1, lda1, w64 + m.w, m.K, w64 + m.b, Rs, m.rows, C, m.rows, R, m.rows, m.K, relu, guard()};
        return launch_gemm_f64(g, s);
    }
    // the same with a matrix outside the blob: W [n][K] (row pitch ldw), the K input columns from A0 (K0) and A1, over `rows` rows
    int gemm64(const double* W, int ldw, const double* bias, int n, int K, const double* A0, int K0, const double* A1, int lda1, int relu, double* C, int rows) const {
        const GemmF64Args g{A0, K0, K0, A1, lda1, W, ldw, bias, nullptr, n, C, n, rows, n, K, relu, guard()};
        return launch_gemm_f64(g, s);
    }
};

// ---- encoders (mdgat.py:392-393), one fused launch ----
static int encoders32(Fwd& f, const FwdIn& in) {
    EncoderLaunch e{in.kpts0, in.sigma0, in.fpfh0, in.kpts1, in.sigma1, in.fpfh1, in.rec0, in.rec1, in.normalize_fpfh,
                    f.h->w.encoder32(), f.ws.x, f.B, f.N, f.M, f.cnt0, f.cnt1};
    if (in.bank) {      // a ragged chunk out of a bank (mdgat_forward_frames_ragged): the encoder's bank form reads the records itself
        e.start0 = in.bank.start0; e.start1 = in.bank.start1;
        e.kp0_out = in.kp0_out; e.kp1_out = in.kp1_out;
        e.guard = f.guard();
    }
    if (int rc = launch_encoder(e, f.s)) return rc;
    f.mark(MDGAT_PROF_ENCODER);
    return f.tap(f.taps.x_enc, f.ws.x, (size_t)f.R * 128, "tap x_enc");
}

// ---- descriptor = 'FPFH_gloabal' (mdgat_load_pooled_encoder_f64): desc = encoder2([e ; max over the frame of e]) + kenc, e = denc.encoder ----
// One product per launch.  The frame maximum g is taken over a pair's OWN keypoints (the counts of a ragged batch), its half of encoder2.0
// is formed once per (pair, frame) - 2B rows, not R - and joins the keypoint half in an epilogue of its own; encoder2.3 and kenc.9 are one
// product over [hidden ; hk3], as the blob's encl is for 'FPFH'.  Then layer 0's q | k | v by the plain product when the layer tails are fused
// (the fused encoder launch, which would have written it, does not run).
// The q | k | v + hidden area (640 doubles per point) in units of R doubles: hk3 0..128 | hk1 128..160, hk2 ..224, hd1 ..288, hd2 ..416, later
// hidden 128..384 | c (2B x 256 <= 256 R) from 384 | the assembled inputs in the last 37.  e lives in the message area, g (2B x 128) in x's.
static int pooled_encoder64(Fwd& f, const double* in4, const double* in33) {
    const Workspace& ws = f.ws;
    const DeviceWeights& w = f.h->w;
    const double* pw = f.h->pool64;
    const size_t Rz = (size_t)f.R;
    double *hk3 = ws.qkv64, *hk1 = hk3 + Rz * 128, *hk2 = hk1 + Rz * 32, *hd1 = hk2 + Rz * 64, *hd2 = hd1 + Rz * 64;
    double *hidden = ws.qkv64 + Rz * 128, *c = ws.qkv64 + Rz * 384, *e = ws.msg64, *g = ws.x64;
    if (int rc = f.gemm64(w.im.enc(ENC_K0), in4, 4, nullptr, 0, 1, nullptr, hk1)) return rc;
    if (int rc = f.gemm64(w.im.enc(ENC_K1), hk1, 32, nullptr, 0, 1, nullptr, hk2)) return rc;
    if (int rc = f.gemm64(w.im.enc(ENC_K2), hk2, 64, nullptr, 0, 1, nullptr, hk3)) return rc;
    if (int rc = f.gemm64(w.im.enc(ENC_D0), in33, 33, nullptr, 0, 1, nullptr, hd1)) return rc;
    if (int rc = f.gemm64(w.im.enc(ENC_D1), hd1, 64, nullptr, 0, 1, nullptr, hd2)) return rc;
    // e = denc.encoder.6 alone: the first 128 columns of the blob's encl ([denc.6 | 0] for this descriptor, its bias denc.6's)
    const WeightMat& l = w.im.enc(ENC_L);
    if (int rc = f.gemm64(w.blob64 + l.w, l.K, w.blob64 + l.b, 128, 128, hd2, 128, nullptr, 0, 0, e, f.R)) return rc;
    if (int rc = launch_frame_max_f64(FrameMaxArgs{e, f.B, f.N, f.M, f.cnt0, f.cnt1, g, nullptr}, f.s)) return rc;
    if (int rc = f.gemm64(pw + PoolLayout::W1G, 128, pw + PoolLayout::B1, 256, 128, g, 128, nullptr, 0, 0, c, 2 * f.B)) return rc;
    if (int rc = f.gemm64(pw + PoolLayout::W1E, 128, nullptr, 256, 128, e, 128, nullptr, 0, 0, hidden, f.R)) return rc;
    if (int rc = launch_add_rows_relu_f64(hidden, c, 256, f.B, f.N, f.M, f.guard(), f.s)) return rc;
    if (int rc = f.gemm64(pw + PoolLayout::W2K, 384, pw + PoolLayout::B2, 128, 384, hidden, 256, hk3, 128, 0, ws.x64, f.R)) return rc;
    if (f.p.fused64 && f.p.first > 0)
        if (int rc = f.gemm64(w.im.proj(0), ws.x64, 128, nullptr, 0, 0, nullptr, ws.qkv64)) return rc;
    return MDGAT_OK;
}

// ---- MDGAT_ARITH_FP64 (f64.hip): the inputs, the encoders and the layers before p.first in the reference's arithmetic ----
static int head64(Fwd& f, const FwdIn& in, CoopGroup& coop) {
    const Workspace& ws = f.ws;
    const DeviceWeights& w = f.h->w;
    const size_t Rz = (size_t)f.R;
    const int first = f.p.first;
    // the assembled inputs at the END of the hidden area (the fused encoder writes layer 0's q | k | v while other workgroups still
    // read their inputs); the stages of the one-product-per-launch form in the (contiguous) q|k|v + hidden area in front of them:
    // 32 + 64 + 128 + 64 + 128 = 416 of the 603 doubles per point there
    double* in4 = ws.hid64 + Rz * (256 - 37);
    double* in33 = in4 + Rz * 4;
    AssembleF64 as{in.dk0, in.ds0, in.df0, in.dk1, in.ds1, in.df1, in.rec0, in.rec1, in.normalize_fpfh, f.cnt0, f.cnt1};
    as.start0 = in.bank.start0; as.start1 = in.bank.start1; as.kp0 = in.kp0_out; as.kp1 = in.kp1_out;
    as.in4 = in4; as.in33 = in33; as.B = f.B; as.N = f.N; as.M = f.M; as.guard = f.guard();
    if (int rc = launch_assemble_f64(as, f.s)) return rc;
    f.mark(MDGAT_PROF_F64_OTHER);
    // KeypointEncoder (mdgat.py:184-188), DescriptorEncoder (152-155), their sum (392-393) as one product over [hd ; hk]
    if (f.h->pool64) {
        if (int rc = pooled_encoder64(f, in4, in33)) return rc;
    } else if (f.p.fused64) {
        const Mat64 k0 = w.mat64(&w.im.enc(ENC_K0)), d0 = w.mat64(&w.im.enc(ENC_D0)), k1 = w.mat64(&w.im.enc(ENC_K1)), k2 = w.mat64(&w.im.enc(ENC_K2)),
                    d1 = w.mat64(&w.im.enc(ENC_D1)), l = w.mat64(&w.im.enc(ENC_L)), q = w.mat64(first > 0 ? &w.im.proj(0) : nullptr);
        const EncoderF64Args e{in4, in33, k0.wf, k0.b, d0.wf, d0.b, k1.wf, k1.b, k2.wf, k2.b, d1.wf, d1.b, l.wf, l.b, q.wf, q.b,
                               ws.x64, ws.qkv64, first == 0 ? ws.x : nullptr, f.R, f.guard()};
        if (int rc = launch_encoder_f64(e, f.s)) return rc;
    } else {
        double *hk1 = ws.qkv64, *hk2 = hk1 + Rz * 32, *hk3 = hk2 + Rz * 64;      // the keypoint encoder's stages
        double *hd1 = hk3 + Rz * 128, *hd2 = hd1 + Rz * 64;                       // the descriptor encoder's
        if (int rc = f.gemm64(w.im.enc(ENC_K0), in4, 4, nullptr, 0, 1, nullptr, hk1)) return rc;
        if (int rc = f.gemm64(w.im.enc(ENC_K1), hk1, 32, nullptr, 0, 1, nullptr, hk2)) return rc;
        if (int rc = f.gemm64(w.im.enc(ENC_K2), hk2, 64, nullptr, 0, 1, nullptr, hk3)) return rc;
        if (int rc = f.gemm64(w.im.enc(ENC_D0), in33, 33, nullptr, 0, 1, nullptr, hd1)) return rc;
        if (int rc = f.gemm64(w.im.enc(ENC_D1), hd1, 64, nullptr, 0, 1, nullptr, hd2)) return rc;
        if (int rc = f.gemm64(w.im.enc(ENC_L), hd2, 128, hk3, 128, 0, nullptr, ws.x64)) return rc;
        layer_f64_count_unfused(1);
    }
    f.mark(MDGAT_PROF_F64_GEMM);
    if (int rc = f.tap(f.taps.x_enc, ws.x64, Rz * 128)) return rc;
    for (int i = 0; i < first; ++i) {
        // MultiHeadedAttention (mdgat.py:223-237; merge is folded into mlp.0 by pack.py), attention / dynamic_attention (190-210)
        if (!f.p.fused64) {
            if (int rc = f.gemm64(w.im.proj(i), ws.x64, 128, nullptr, 0, 0, nullptr, ws.qkv64)) return rc;
            f.mark(MDGAT_PROF_F64_GEMM);
        }
        const int kk = f.h->cfg.topk[i];
        if (int rc = launch_attention_f64(AttnF64Call{f.B, f.N, f.M, i & 1, kk, ws.qkv64, ws.msg64, f.sel_tap(i), f.cnt0, f.cnt1, f.cnt_min, f.guard(), f.s})) return rc;
        f.mark(kk > 0 ? MDGAT_PROF_F64_ATTENTION_TOPK : MDGAT_PROF_F64_ATTENTION_FULL);
        // AttentionalPropagation + residual (mdgat.py:246-248, 274)
        if (f.p.fused64) {
            const bool last = i + 1 == first;
            const Mat64 w1 = w.mat64(&w.im.layer(i, MAT_W1)), w2 = w.mat64(&w.im.layer(i, MAT_W2)), q = w.mat64(last ? nullptr : &w.im.proj(i + 1));
            const LayerF64Args t{ws.x64, ws.msg64, w1.wf, w1.b, w2.wf, w2.b, q.wf, q.b, ws.qkv64, last ? ws.x : nullptr, f.R, f.guard(), ws.hid64};
            if (int rc = launch_layer_tail_f64(t, coop)) return rc;
        } else {
            if (int rc = f.gemm64(w.im.layer(i, MAT_W1), ws.x64, 128, ws.msg64, 128, 1, nullptr, ws.hid64)) return rc;
            if (int rc = f.gemm64(w.im.layer(i, MAT_W2), ws.hid64, 256, nullptr, 0, 0, ws.x64, ws.x64)) return rc;
            layer_f64_count_unfused(0);
        }
        f.mark(MDGAT_PROF_F64_GEMM);
        if (int rc = f.tap(f.x_tap(i), ws.x64, Rz * 128)) return rc;
    }
    return MDGAT_OK;
}

// ---- p.tail64: final_proj (mdgat.py:397), the score matrix (430-431), the optimal transport (434-436), the extraction (441-483)
// and the loss in fp64 ----
static int tail64(Fwd& f, const FwdOut& o, CoopGroup& coop) {
    const Workspace& ws = f.ws;
    const int B = f.B, N = f.N, M = f.M;
    double* mdesc64 = ws.msg64;          // (the message and q | k | v of the last layer are dead)
    double* scores64 = ws.scores64;      // [B][N][M]: in q | k | v's room while N M <= 384 (N + M)
    if (int rc = f.gemm64(f.h->w.im.proj(2 * f.h->cfg.L), ws.x64, 128, nullptr, 0, 0, nullptr, mdesc64)) return rc;
    if (int rc = f.tap(f.taps.mdesc, mdesc64, (size_t)f.R * 128)) return rc;
    const GemmF64Args sg{mdesc64, 128, 128, nullptr, 0, mdesc64 + (size_t)N * 128, 128, nullptr, nullptr, 0, scores64, M, N, M, 128, 0, f.guard(),
                         0.08838834764831845 /* 1 / sqrt(128) */, B, (long long)(N + M) * 128, (long long)(N + M) * 128, (long long)N * M};
    if (int rc = launch_gemm_f64(sg, f.s)) return rc;
    f.mark(MDGAT_PROF_F64_GEMM);
    if (int rc = f.tap(f.taps.scores, scores64, (size_t)B * N * M)) return rc;
    Sk64Call c{};
    c.B = B; c.N = N; c.M = M; c.scores = scores64; c.alpha_dev = f.h->w.blob64 + f.h->w.bl.bin_score; c.iters = f.h->cfg.sinkhorn_iters;
    c.Z64 = ws.Z64; c.Z32 = o.Z; c.inner = f.h->cfg.extract_mode >= MDGAT_EXTRACT_THRESHOLD;
    c.bests = sinkhorn_f64_bests(ws.sk64 + ws.sk64_bytes, B, N, M);
    c.cnt0 = f.cnt0; c.cnt1 = f.cnt1;
    const SkExtract ex = f.extract(o);
    if (int rc = launch_sinkhorn_f64(c, f.p.sk64, ws.sk64, ws.sk64_bytes, f.s, &coop, f.guard())) return rc;
    if (int rc = launch_extract_from_bests(B, N, M, &ex, c.bests.ri, c.bests.rv, c.bests.ci, c.bests.cv, f.s, f.cnt0, f.cnt1)) return rc;
    f.mark(MDGAT_PROF_SINKHORN);
    return f.loss(o, static_cast<const double*>(ws.Z64));
}

// ---- the hand-over to the fp32-class kernels (nothing behind p.first is discontinuous); the fused fp64 launches write it on the side ----
static int hand_over(Fwd& f) {
    if (f.p.fused64 && !(f.h->pool64 && f.p.first == 0)) return MDGAT_OK;      // (the pooled encoder is never a fused launch)
    const int rc = launch_f64_to_f32(f.ws.x64, f.ws.x, (size_t)f.R * 128, f.guard(), f.s);
    if (!rc) f.mark(MDGAT_PROF_F64_OTHER);
    return rc;
}

// ---- the attentional propagation layers from p.first on (mdgat.py:259-276) ----
// launch i: [attention of layer i] -> [mlp + residual of layer i | q/k/v of layer i + 1 (or final_proj into ws.hid)]
static int layers32(Fwd& f) {
    const mdgat_handle* h = f.h;
    const int L2 = 2 * h->cfg.L;
    // a layer launch whose projection is layer j's q | k | v, or final_proj behind the last layer (j == 2L)
    auto launch = [&](LayerLaunch p, int j, int cls) {
        p.x = f.ws.x; p.R = f.R; p.N = f.N; p.M = f.M; p.out = f.q16; p.mdesc = f.ws.hid; p.guard = f.guard();
        p.proj = h->w.proj32(j);
        const int rc = launch_layer(p, f.s);
        if (!rc) f.mark(cls);
        return rc;
    };
    if (int rc = launch(LayerLaunch{}, f.p.first, MDGAT_PROF_LAYER_FIRST)) return rc;
    for (int i = f.p.first; i < L2; ++i) {
        const int cross = i & 1;   // names = ['self', 'cross'] * L (mdgat.py:352-353)
        const int kk = h->cfg.topk[i];
        AttnCall c{f.B, f.N, f.M, cross, kk, h->cfg.attention_mode, f.q16, f.ws.msg};
        c.sel = f.cnt0 ? nullptr : f.sel_tap(i);      // (a ragged forward taps no selection)
        c.cnt0 = f.cnt0; c.cnt1 = f.cnt1; c.wide = f.p.wide32; c.stream = f.s;
        if (int rc = launch_attention(c)) return rc;
        f.mark(kk > 0 ? MDGAT_PROF_ATTENTION_TOPK : MDGAT_PROF_ATTENTION_FULL);
        LayerLaunch p{};
        p.msg = f.ws.msg; p.do_mlp = 1; p.mlp = h->w.layer32(i);
        if (int rc = launch(p, i + 1, i + 1 < L2 ? MDGAT_PROF_LAYER : MDGAT_PROF_LAYER_LAST)) return rc;
        if (int rc = f.tap(f.x_tap(i), f.ws.x, (size_t)f.R * 128, "tap x_layers")) return rc;
    }
    return MDGAT_OK;
}

// ---- score matrix (mdgat.py:430-431) of the final projection (397, in ws.hid), optimal transport (434-436), match extraction
// (441-483) and the loss ----
static int tail32(Fwd& f, const FwdOut& o) {
    const Workspace& ws = f.ws;
    const int B = f.B, N = f.N, M = f.M;
    const float* mdesc = ws.hid;
    if (int rc = f.tap(f.taps.mdesc, mdesc, (size_t)f.R * 128, "tap mdesc")) return rc;
    // (the score kernel also clears the exchange slots of the Sinkhorn kernel that follows: no memset launch in between)
    const size_t sk_clear = f.p.cluster32 ? sinkhorn_slots_clear_bytes(B, N, M) : 0;
    if (int rc = launch_scores(B, N, M, mdesc, ws.scores, 0.08838834764831845f /* 1 / sqrt(128) */, f.s, sk_clear ? ws.sk : nullptr, sk_clear,
                            f.guard())) return rc;
    f.mark(MDGAT_PROF_SCORES);
    if (int rc = f.tap(f.taps.scores, ws.scores, (size_t)B * N * M, "tap scores")) return rc;
    // (Z is only materialised when the caller asks for it, the streaming Sinkhorn needs it for the extraction or the loss reads it)
    // (a ragged batch: the streaming kernel with the counts - the cluster kernel takes none - into the caller's Z or the workspace's)
    float* const Zroom = o.Z ? o.Z : ws.Z;
    float* Zout = o.Z || f.cnt0 || !f.p.cluster32 || o.loss ? Zroom : nullptr;
    const SkExtract ex = f.extract(o);
    SkCall c{B, N, M, f.h->cfg.sinkhorn_iters, ws.scores, f.h->w.blob + f.h->w.bl.bin_score};
    c.Z = Zout; c.Zfb = Zroom; c.cnt0 = f.cnt0; c.cnt1 = f.cnt1;      // (Zfb: where redone pairs go when the cluster kernel writes no Z)
    c.ws = ws.sk; c.ws_bytes = ws.sk_bytes; c.slots_cleared = sk_clear != 0; c.status = f.status; c.ex = &ex; c.stream = f.s;
    // (a ragged batch of a handle that opted in: the split form, each of its iterations a launch of the profile's Sinkhorn class)
    c.wide = f.p.wide32; c.split = f.p.split32; c.split_ws = ws.sksplit; c.split_ws_bytes = ws.sksplit_bytes;
    c.launched = [](void* fwd) { static_cast<Fwd*>(fwd)->mark(MDGAT_PROF_SINKHORN); }; c.launched_ctx = &f;
    if (int rc = launch_sinkhorn(c)) return rc;
    f.mark(MDGAT_PROF_SINKHORN);
    return f.loss(o, static_cast<const float*>(Zout));
}

// one slice of a call (checked by plan_forward) on one lane
static int forward_impl(mdgat_handle* h, const Path& p, int B, int N, int M, const FwdIn& in, const FwdOut& o, const mdgat_taps* taps,
                        void* workspace, hipStream_t s, unsigned* status, int lane, int defer_alldust) {
    const Workspace ws = carve(workspace, B, N, M, p.f64, o.loss, p.sk64, p.split32, p.wide32);
    Fwd f{h, p, B, N, M, B * (N + M), ws, mdgat_qkv16_carve(ws.qkv16, B, N, M), s, status, taps ? *taps : mdgat_taps{}, h->prof[lane], defer_alldust,
          in.counts.cnt0, in.counts.cnt1, p.cnt_min};
    f.mark(-1);
    int rc;
    if ((N & 31) || (M & 31))   // the attention kernel reads V^T in whole 32-key blocks: pad columns must be zero
        if ((rc = mdgat_check_hip(hipMemsetAsync(f.q16.vt16, 0, (size_t)B * 256 * f.q16.PP * sizeof(_Float16), s), "memset(V^T pads)"))) return rc;
    if (!p.f64) {
        if ((rc = encoders32(f, in))) return rc;
    } else {
        // (the forward's launches of kernels whose workgroups wait for each other - clustered layer tails, the resident fp64 Sinkhorn - as
        // one group of the device's chain: coop_chain.hpp)
        CoopGroup coop;
        if ((rc = coop.open(h->device, s)) || (rc = head64(f, in, coop))) return rc;
        if (p.tail64) return tail64(f, o, coop);
        if ((rc = hand_over(f))) return rc;
    }
    if ((rc = layers32(f))) return rc;
    return tail32(f, o);
}

// profiling: wait for the events of both lanes and add the intervals between consecutive ones to their kernel classes
// (an interval that starts at a -1 mark - the beginning of a forward_impl call - is counted, one that ends there is not)
static int prof_collect(mdgat_handle* h) {
    if (!h->prof_on) return MDGAT_OK;
    for (auto& pl : h->prof) {
        if (pl.n > 1) {
            if (int rc = mdgat_check_hip(hipEventSynchronize(pl.ev[pl.n - 1]), "profile sync")) return rc;
            for (size_t i = 1; i < pl.n; ++i) {
                float ms = 0.f;
                if (pl.cls[i] >= 0 && hipEventElapsedTime(&ms, pl.ev[i - 1], pl.ev[i]) == hipSuccess) {
                    h->prof_ms[pl.cls[i]] += ms;
                    h->prof_launches[pl.cls[i]] += 1;
                }
            }
        }
        pl.n = 0;
        pl.cls.clear();
    }
    return MDGAT_OK;
}

static int forward_batched(mdgat_handle* h, int B, int N, int M, const FwdIn& in,
                           int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1, float* Z,
                           const mdgat_taps* taps, void* workspace, size_t workspace_bytes, void* stream,
                           const mdgat_loss_request* loss_req = nullptr) {
    const FwdOut out{matches0, matches1, mscores0, mscores1, Z, loss_req != nullptr, loss_req ? *loss_req : mdgat_loss_request{}};
    Path p{};
    if (int rc = plan_forward(h, B, N, M, in, out, taps, workspace, workspace_bytes, p)) return rc;
    // the handle's device is current for the whole call, the caller's restored after it: everything below works on the current device
    struct DeviceScope {
        int prev = -1, dev;
        hipError_t set = hipSuccess;
        explicit DeviceScope(int d) : dev(d) { (void)hipGetDevice(&prev); if (prev != dev) set = hipSetDevice(dev); }
        ~DeviceScope() { if (prev != dev) (void)hipSetDevice(prev); }
    } scope(h->device);
    if (int rc = mdgat_check_hip(scope.set, "hipSetDevice")) return rc;
    std::lock_guard<std::mutex> serialise(h->enqueue);
    if (++h->match_token == 0) h->match_token = 1;      // this call's token (mdgat_matched_any): every slice / lane of the call writes the same one
    unsigned* status = nullptr;
    if (int rc = mdgat_check_hip(hipHostGetDevicePointer(reinterpret_cast<void**>(&status), h->host_error, 0), "hipHostGetDevicePointer")) return rc;
    hipStream_t s0 = static_cast<hipStream_t>(stream);
    const LanePlan& lp = p.lanes;
    const bool sliced = lp.nslices > 1;
    int rc = MDGAT_OK;
    if (lp.lanes == 2) {
        // (both lanes start together: a second lane started one to five launches behind the first - complementary kernels
        // side by side - pays the delay as a tail: 20 900 -> 20 300 ... 19 700 pairs/s at B = 64)
        if ((rc = mdgat_check_hip(hipEventRecord(h->ev_fork, s0), "fork record"))) return rc;
        if ((rc = mdgat_check_hip(hipStreamWaitEvent(h->lane_stream, h->ev_fork, 0), "fork wait"))) return rc;
    }
    for (int c = 0, slice = 0; c < B && !rc; c += lp.per, ++slice) {
        const int lane = lp.lanes == 2 ? (slice & 1) : 0;
        rc = forward_impl(h, p, B - c < lp.per ? B - c : lp.per, N, M, in.from(c, N, M), out.from(c, N, M), taps,
                          static_cast<char*>(workspace) + (size_t)lane * lp.lane_bytes, lane ? h->lane_stream : s0, status, lane, sliced);
    }
    if (lp.lanes == 2) {
        // (joined even after a failed launch: the caller's stream must not run ahead of what the second lane was given)
        const int rj = mdgat_check_hip(hipEventRecord(h->ev_join, h->lane_stream), "join record");
        const int rw = mdgat_check_hip(hipStreamWaitEvent(s0, h->ev_join, 0), "join wait");
        if (!rc) rc = rj ? rj : rw;
    }
    if (rc) return rc;
    if (sliced && (rc = launch_alldust_fixup(B, N, M, h->cfg.extract_mode, out.matches0, out.mscores1, s0))) return rc;
    return prof_collect(h);
}

// the array entry points: `who` with its six input arrays, fp32 or fp64
template <typename T> static int forward_arrays(const char* who, mdgat_handle* h, int B, int N, int M, const T* k0, const T* s0, const T* f0, const T* k1,
                                                const T* s1, const T* f1, int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1, float* Z,
                                                const mdgat_taps* taps, void* workspace, size_t workspace_bytes, void* stream, const mdgat_loss_request* req = nullptr) {
    if (!k0 || !s0 || !f0 || !k1 || !s1 || !f1) { mdgat_set_error("%s: null input pointer", who); return MDGAT_ERR_BAD_ARG; }
    return forward_batched(h, B, N, M, FwdIn::arrays(k0, s0, f0, k1, s1, f1), matches0, matches1, mscores0, mscores1, Z, taps, workspace, workspace_bytes, stream, req);
}

extern "C" int mdgat_forward(mdgat_handle* h, int B, int N, int M, const float* kpts0, const float* sigma0,
                             const float* fpfh0, const float* kpts1, const float* sigma1, const float* fpfh1,
                             int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1, float* Z,
                             const mdgat_taps* taps, void* workspace, size_t workspace_bytes, void* stream) {
    return forward_arrays("mdgat_forward", h, B, N, M, kpts0, sigma0, fpfh0, kpts1, sigma1, fpfh1, matches0, matches1, mscores0, mscores1, Z, taps, workspace, workspace_bytes, stream);
}

extern "C" int mdgat_forward_f64(mdgat_handle* h, int B, int N, int M, const double* kpts0, const double* sigma0,
                                 const double* fpfh0, const double* kpts1, const double* sigma1, const double* fpfh1,
                                 int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1, float* Z,
                                 const mdgat_taps* taps, void* workspace, size_t workspace_bytes, void* stream) {
    return forward_arrays("mdgat_forward_f64", h, B, N, M, kpts0, sigma0, fpfh0, kpts1, sigma1, fpfh1, matches0, matches1, mscores0, mscores1, Z, taps, workspace, workspace_bytes, stream);
}

// A ragged batch in the exact mode: pairs of different sizes in slots padded to Np x Mp, one call.  The counts ride in FwdIn: plan_forward
// makes every check - the uniform call's, and the counts' on their host copies - before anything is enqueued and plans the batch unsliced;
// the kernels that take the counts (assemble, attention, Sinkhorn, extraction) get them, the row-wise launches in between run over the
// padded rows, which the assemble kernel has zeroed.
extern "C" int mdgat_forward_f64_ragged(mdgat_handle* h, int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1,
                                        const int32_t* counts0_host, const int32_t* counts1_host, const double* kpts0, const double* sigma0,
                                        const double* fpfh0, const double* kpts1, const double* sigma1, const double* fpfh1, int64_t* matches0,
                                        int64_t* matches1, float* mscores0, float* mscores1, float* Z, const mdgat_taps* taps, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    if (!kpts0 || !sigma0 || !fpfh0 || !kpts1 || !sigma1 || !fpfh1 || !counts0 || !counts1 || !counts0_host || !counts1_host) {
        mdgat_set_error("mdgat_forward_f64_ragged: null input pointer");
        return MDGAT_ERR_BAD_ARG;
    }
    FwdIn in = FwdIn::arrays(kpts0, sigma0, fpfh0, kpts1, sigma1, fpfh1);
    in.counts = RaggedCounts{counts0, counts1, counts0_host, counts1_host};
    return forward_batched(h, B, Np, Mp, in, matches0, matches1, mscores0, mscores1, Z, taps, workspace, workspace_bytes, stream);
}

// The same on the fp32-class path (an MDGAT_ARITH_FP32 handle, float inputs): the ragged plan's second branch in plan_forward.  The encoder,
// the attention kernel and the streaming Sinkhorn take the counts; what the inputs hold beyond them is never read.
extern "C" int mdgat_forward_ragged(mdgat_handle* h, int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1,
                                    const int32_t* counts0_host, const int32_t* counts1_host, const float* kpts0, const float* sigma0,
                                    const float* fpfh0, const float* kpts1, const float* sigma1, const float* fpfh1, int64_t* matches0,
                                    int64_t* matches1, float* mscores0, float* mscores1, float* Z, const mdgat_taps* taps, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    if (!kpts0 || !sigma0 || !fpfh0 || !kpts1 || !sigma1 || !fpfh1 || !counts0 || !counts1 || !counts0_host || !counts1_host) {
        mdgat_set_error("mdgat_forward_ragged: null input pointer");
        return MDGAT_ERR_BAD_ARG;
    }
    if (h && h->cfg.arithmetic != MDGAT_ARITH_FP32) {
        mdgat_set_error("mdgat_forward_ragged: the handle needs MDGAT_ARITH_FP32 (an exact-mode handle runs mdgat_forward_f64_ragged)");
        return MDGAT_ERR_BAD_ARG;
    }
    FwdIn in = FwdIn::arrays(kpts0, sigma0, fpfh0, kpts1, sigma1, fpfh1);
    in.counts = RaggedCounts{counts0, counts1, counts0_host, counts1_host};
    return forward_batched(h, B, Np, Mp, in, matches0, matches1, mscores0, mscores1, Z, taps, workspace, workspace_bytes, stream);
}

// the ABI's int64 starts as the launchers take them
static RaggedStarts ragged_starts(const int64_t* s0, const int64_t* s1, const int64_t* h0, const int64_t* h1, int64_t rows0, int64_t rows1) {
    static_assert(sizeof(long long) == sizeof(int64_t), "the starts are passed on as long long");
    auto ll = [](const int64_t* q) { return reinterpret_cast<const long long*>(q); };
    return RaggedStarts{ll(s0), ll(s1), ll(h0), ll(h1), rows0, rows1};
}

// The same fed from a bank of raw records; the entry follows the handle, as mdgat_forward_frames does.  An exact-mode handle (and the fp64
// handle that runs the encoders alone): the ragged assemble kernel in front, everything behind it as above.  An MDGAT_ARITH_FP32 handle:
// mdgat_forward_ragged's plan, the encoder's bank form reading the records itself.
extern "C" int mdgat_forward_frames_ragged(mdgat_handle* h, int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1,
                                           const int32_t* counts0_host, const int32_t* counts1_host, const int64_t* starts0, const int64_t* starts1,
                                           const int64_t* starts0_host, const int64_t* starts1_host, const float* rec0, int64_t rows0,
                                           const float* rec1, int64_t rows1, int normalize_fpfh, int64_t* matches0, int64_t* matches1,
                                           float* mscores0, float* mscores1, float* Z, float* kpts0_out, float* kpts1_out, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    const char* who = "mdgat_forward_frames_ragged";
    if (!rec0 || !rec1 || !counts0 || !counts1 || !counts0_host || !counts1_host || !starts0 || !starts1 || !starts0_host || !starts1_host) {
        mdgat_set_error("%s: null input pointer", who);
        return MDGAT_ERR_BAD_ARG;
    }
    if (rows0 < 0 || rows1 < 0) { mdgat_set_error("%s: negative record count", who); return MDGAT_ERR_BAD_ARG; }
    FwdIn in;
    in.rec0 = rec0; in.rec1 = rec1; in.normalize_fpfh = normalize_fpfh;
    in.counts = RaggedCounts{counts0, counts1, counts0_host, counts1_host};
    in.bank = ragged_starts(starts0, starts1, starts0_host, starts1_host, rows0, rows1);
    in.kp0_out = kpts0_out; in.kp1_out = kpts1_out;
    return forward_batched(h, B, Np, Mp, in, matches0, matches1, mscores0, mscores1, Z, nullptr, workspace, workspace_bytes, stream);
}

// The assemble launch alone, into caller-owned buffers: every check of the counts and the starts on their host copies, as the forward makes them.
extern "C" int mdgat_assemble_frames_f64_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                                const int32_t* counts1_host, const int64_t* starts0, const int64_t* starts1,
                                                const int64_t* starts0_host, const int64_t* starts1_host, const float* rec0, int64_t rows0,
                                                const float* rec1, int64_t rows1, int normalize_fpfh, double* in4, double* in33, float* kpts0_out,
                                                float* kpts1_out, unsigned* guard, void* stream) {
    const char* who = "mdgat_assemble_frames_f64_ragged";
    if (!rec0 || !rec1 || !in4 || !in33) { mdgat_set_error("%s: null pointer", who); return MDGAT_ERR_BAD_ARG; }
    if (B < 0 || Np <= 0 || Mp <= 0 || rows0 < 0 || rows1 < 0) { mdgat_set_error("%s: bad shape B=%d Np=%d Mp=%d", who, B, Np, Mp); return MDGAT_ERR_BAD_ARG; }
    const RaggedStarts bank = ragged_starts(starts0, starts1, starts0_host, starts1_host, rows0, rows1);
    if (int rc = mdgat_check_ragged(who, B, Np, Mp, RaggedCounts{counts0, counts1, counts0_host, counts1_host}, &bank, nullptr, 0, nullptr)) return rc;
    AssembleF64 as{};      // (the starts are not null - mdgat_check_ragged refuses that with a bank - so this is the launch of the bank kernel)
    as.rec0 = rec0; as.rec1 = rec1; as.normalize = normalize_fpfh; as.cnt0 = counts0; as.cnt1 = counts1;
    as.start0 = bank.start0; as.start1 = bank.start1; as.kp0 = kpts0_out; as.kp1 = kpts1_out;
    as.in4 = in4; as.in33 = in33; as.B = B; as.N = Np; as.M = Mp; as.guard = guard;
    return launch_assemble_f64(as, static_cast<hipStream_t>(stream));
}

// The loader's train-mode assembly of a chunk (ensure_kpts_num): the saliency filter and the pad / truncate to T in front of the same decode.
// A frame may hold any number of records (>= 1), so the counts are checked against no slot size.
extern "C" int mdgat_assemble_frames_train_f64(int B, int T, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                               const int32_t* counts1_host, const int64_t* starts0, const int64_t* starts1,
                                               const int64_t* starts0_host, const int64_t* starts1_host, const float* rec0, int64_t rows0,
                                               const float* rec1, int64_t rows1, float min_saliency, int normalize_fpfh, double* in4, double* in33,
                                               float* kpts0_out, float* kpts1_out, int32_t* source0, int32_t* source1, int32_t* salient0,
                                               int32_t* salient1, unsigned* status, unsigned* guard, void* stream) {
    const char* who = "mdgat_assemble_frames_train_f64";
    if (!rec0 || !rec1 || !in4 || !in33 || !kpts0_out || !kpts1_out || !source0 || !source1 || !salient0 || !salient1 || !status) {
        mdgat_set_error("%s: null pointer", who);
        return MDGAT_ERR_BAD_ARG;
    }
    if (B < 0 || T <= 0 || rows0 < 0 || rows1 < 0) { mdgat_set_error("%s: bad shape B=%d T=%d", who, B, T); return MDGAT_ERR_BAD_ARG; }
    if (T > 2048) { mdgat_set_error("%s: max_keypoints=%d: at most 2048 keypoints per frame (the attention's limit)", who, T); return MDGAT_ERR_BAD_ARG; }
    if (min_saliency != min_saliency) { mdgat_set_error("%s: min_saliency is NaN", who); return MDGAT_ERR_BAD_ARG; }
    const RaggedStarts bank = ragged_starts(starts0, starts1, starts0_host, starts1_host, rows0, rows1);
    if (int rc = mdgat_check_ragged(who, B, INT32_MAX, INT32_MAX, RaggedCounts{counts0, counts1, counts0_host, counts1_host}, &bank, nullptr, 0, nullptr)) return rc;
    return launch_assemble_frames_train_f64(B, T, rec0, rec1, bank.start0, bank.start1, counts0, counts1, min_saliency, normalize_fpfh, in4, in33, kpts0_out,
                                            kpts1_out, source0, source1, salient0, salient1, status, guard, static_cast<hipStream_t>(stream));
}

extern "C" int mdgat_forward_loss(mdgat_handle* h, int B, int N, int M, const float* kpts0, const float* sigma0,
                                  const float* fpfh0, const float* kpts1, const float* sigma1, const float* fpfh1,
                                  int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1, float* Z,
                                  const mdgat_taps* taps, const mdgat_loss_request* req, void* workspace, size_t workspace_bytes, void* stream) {
    return forward_arrays("mdgat_forward_loss", h, B, N, M, kpts0, sigma0, fpfh0, kpts1, sigma1, fpfh1, matches0, matches1, mscores0, mscores1, Z, taps, workspace, workspace_bytes, stream, req);
}

extern "C" int mdgat_forward_f64_loss(mdgat_handle* h, int B, int N, int M, const double* kpts0, const double* sigma0,
                                      const double* fpfh0, const double* kpts1, const double* sigma1, const double* fpfh1,
                                      int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1, float* Z,
                                      const mdgat_taps* taps, const mdgat_loss_request* req, void* workspace, size_t workspace_bytes, void* stream) {
    return forward_arrays("mdgat_forward_f64_loss", h, B, N, M, kpts0, sigma0, fpfh0, kpts1, sigma1, fpfh1, matches0, matches1, mscores0, mscores1, Z, taps, workspace, workspace_bytes, stream, req);
}

extern "C" int mdgat_forward_frames(mdgat_handle* h, int B, int N, int M, const float* frames0, const float* frames1,
                                    int normalize_fpfh, int64_t* matches0, int64_t* matches1, float* mscores0,
                                    float* mscores1, float* Z, const mdgat_taps* taps, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    if (!frames0 || !frames1) { mdgat_set_error("mdgat_forward_frames: null frame pointer"); return MDGAT_ERR_BAD_ARG; }
    FwdIn in;
    in.rec0 = frames0; in.rec1 = frames1; in.normalize_fpfh = normalize_fpfh;
    return forward_batched(h, B, N, M, in, matches0, matches1, mscores0, mscores1, Z, taps, workspace, workspace_bytes, stream);
}

extern "C" int mdgat_async_status(mdgat_handle* h, int clear, unsigned* sinkhorn_fallback, unsigned* range_violation) {
    if (!h) { mdgat_set_error("mdgat_async_status: null handle"); return MDGAT_ERR_BAD_ARG; }
    volatile unsigned* st = h->host_error;
    const unsigned fb = st[MDGAT_STATUS_SK_FALLBACK], rg = st[MDGAT_STATUS_RANGE];
    if (sinkhorn_fallback) *sinkhorn_fallback = fb;
    if (range_violation) *range_violation = rg;
    if (clear) { st[MDGAT_STATUS_SK_FALLBACK] = 0; st[MDGAT_STATUS_RANGE] = 0; }
    if (rg) {
        mdgat_set_error("activations outside the f16 operand range (|v| >= 6e4; fp64 layers of the exact mode: |v| >= 2^500) or non-finite "
                        "values reached a kernel: the outputs of the calls since the last check are invalid (this checkpoint / input does "
                        "not fit the arithmetic)");
        return MDGAT_ERR_UNSUPPORTED;
    }
    return MDGAT_OK;
}

extern "C" unsigned mdgat_last_token(mdgat_handle* h) { return h ? h->match_token : 0u; }

extern "C" int mdgat_matched_any(mdgat_handle* h, unsigned token, unsigned* matched) {
    if (!h || !matched) { mdgat_set_error("mdgat_matched_any: null argument"); return MDGAT_ERR_BAD_ARG; }
    // the extraction kernels of the forward that carried `token` write it into the token's slot when a frame-0 keypoint is matched
    // (host-mapped words; a slot per call, so calls of other threads / streams on this handle in between do not disturb the answer)
    if (!token) token = h->match_token;
    *matched = static_cast<volatile unsigned*>(h->host_error)[MDGAT_STATUS_MATCHED + (token % MDGAT_MATCH_SLOTS)] == token ? 1u : 0u;
    return MDGAT_OK;
}

extern "C" int mdgat_profile(mdgat_handle* h, int enable, double* ms_out, long long* launches_out) {
    if (!h) { mdgat_set_error("mdgat_profile: null handle"); return MDGAT_ERR_BAD_ARG; }
    for (int c = 0; c < MDGAT_PROF_CLASSES; ++c) {
        if (ms_out) ms_out[c] = h->prof_ms[c];
        if (launches_out) launches_out[c] = h->prof_launches[c];
        h->prof_ms[c] = 0.0;
        h->prof_launches[c] = 0;
    }
    h->prof_on = enable != 0;
    return MDGAT_OK;
}

// ---------------------------------------------------------------------------------- per-op entry points
extern "C" size_t mdgat_sinkhorn_workspace_bytes(int B, int N, int M) { return sinkhorn_cluster_workspace_bytes(B, N, M); }

static size_t sk_ragged_z_bytes(int B, int Np, int Mp) { return ((size_t)B * (Np + 1) * (Mp + 1) * sizeof(float) + 255) & ~(size_t)255; }
extern "C" size_t mdgat_sinkhorn_ragged_workspace_bytes(int B, int Np, int Mp) {
    if (B <= 0 || Np <= 0 || Mp <= 0 || Np > MDGAT_RAGGED_FP32_MAX_KEYPOINTS || Mp > MDGAT_RAGGED_FP32_MAX_KEYPOINTS) return 0;
    return sk_ragged_z_bytes(B, Np, Mp);
}
// the wide entries' workspace: a Z of the slot's size, the split form's scratch (0 bytes for a slot of one slab) behind it
extern "C" size_t mdgat_sinkhorn_ragged_wide_workspace_bytes(int B, int Np, int Mp) {
    if (B <= 0 || Np <= 0 || Mp <= 0 || Np > MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS || Mp > MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS) return 0;
    return sk_ragged_z_bytes(B, Np, Mp) + sinkhorn_split_workspace_bytes(B, Np, Mp, true);
}

// the slot limit of the fp32 ragged entries, then the per-pair checks every ragged entry makes (ragged.hpp)
static int sk_ragged_check(const char* who, int B, int Np, int Mp, int iters, const RaggedCounts& c, bool wide) {
    if (B < 0 || Np <= 0 || Mp <= 0 || iters < 0) { mdgat_set_error("%s: bad shape B=%d Np=%d Mp=%d iters=%d", who, B, Np, Mp, iters); return MDGAT_ERR_BAD_ARG; }
    if (B == 0) return MDGAT_OK;
    const int limit = wide ? MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS : MDGAT_RAGGED_FP32_MAX_KEYPOINTS;
    if (Np > limit || Mp > limit) {
        mdgat_set_error("%s: padded sizes %d x %d: fp32 ragged batches hold at most %d keypoints per frame", who, Np, Mp, limit);
        return MDGAT_ERR_UNSUPPORTED;
    }
    return mdgat_check_ragged(who, B, Np, Mp, c, nullptr, nullptr, 0, nullptr);
}
static bool sk_outputs_null(const SkExtract& ex) { return !ex.m0 || !ex.m1 || !ex.s0 || !ex.s1; }
static SkCall sk_op_call(int B, int N, int M, const float* scores, float bin_score, int iters, float* Z, void* workspace, size_t workspace_bytes, void* stream,
                         float* Z_lent = nullptr) {
    SkCall c{B, N, M, iters, scores};
    c.alpha_host = bin_score; c.Z = Z; c.Zfb = Z_lent; c.ws = workspace; c.ws_bytes = workspace_bytes; c.stream = static_cast<hipStream_t>(stream);
    return c;
}

// ONE body for the four Sinkhorn entries.  counts: null for the uniform entries, which run the streaming kernel instead of the cluster kernel without (enough,
// 256-byte aligned) workspace; a ragged batch always does, and its extraction scans Z: the caller's, or one produced into the workspace.  ex: as in the
// forward's call (tail32) - the same launcher, the same SkExtract, the batch-wide rule applied inside the launch.
// c.wide (the wide ragged entries): c.ws is then a workspace of mdgat_sinkhorn_ragged_wide_workspace_bytes - a Z, the split form's scratch behind it.
static int sk_op(const char* who, SkCall c, const RaggedCounts* counts, const SkExtract* ex) {
    if (!c.scores || (ex ? sk_outputs_null(*ex) : !c.Z)) { mdgat_set_error("%s: null pointer", who); return MDGAT_ERR_BAD_ARG; }
    if (ex) if (int rc = extract_check_mode(who, ex->mode)) return rc;
    c.ex = ex;
    if (counts) {
        if (int rc = sk_ragged_check(who, c.B, c.N, c.M, c.iters, *counts, c.wide)) return rc;
        if (c.B == 0) return MDGAT_OK;
        if (c.wide) {
            const size_t zbytes = sk_ragged_z_bytes(c.B, c.N, c.M), split_bytes = c.split ? sinkhorn_split_workspace_bytes(c.B, c.N, c.M, true) : 0;
            if ((!c.Z || split_bytes) && (!c.ws || c.ws_bytes < mdgat_sinkhorn_ragged_wide_workspace_bytes(c.B, c.N, c.M) || (reinterpret_cast<uintptr_t>(c.ws) & 255))) {
                mdgat_set_error("%s: the workspace (a Z where none is given, the split form's scratch) is too small or not 256-byte aligned", who);
                return MDGAT_ERR_BAD_ARG;
            }
            if (split_bytes) { c.split_ws = static_cast<char*>(c.ws) + zbytes; c.split_ws_bytes = split_bytes; }
        } else if (!c.Z && (!c.ws || c.ws_bytes < mdgat_sinkhorn_ragged_workspace_bytes(c.B, c.N, c.M) || (reinterpret_cast<uintptr_t>(c.ws) & 255))) {
            mdgat_set_error("%s: without Z the workspace holds it: too small or not 256-byte aligned", who);
            return MDGAT_ERR_BAD_ARG;
        }
        if (!c.Z) c.Z = static_cast<float*>(c.ws);
        c.cnt0 = counts->cnt0; c.cnt1 = counts->cnt1;
    }
    return launch_sinkhorn(c);
}

extern "C" int mdgat_sinkhorn(int B, int N, int M, const float* scores, float bin_score, int iters, float* Z, void* workspace,
                              size_t workspace_bytes, void* stream) {
    return sk_op("mdgat_sinkhorn", sk_op_call(B, N, M, scores, bin_score, iters, Z, workspace, workspace_bytes, stream), nullptr, nullptr);
}

extern "C" int mdgat_sinkhorn_extract(int B, int N, int M, const float* scores, float bin_score, int iters, int mode, float match_threshold,
                                      int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1, float* Z_or_null,
                                      float* Z_fallback_or_null, void* workspace, size_t workspace_bytes, void* stream) {
    const SkExtract ex{mode, match_threshold, matches0, matches1, mscores0, mscores1};
    return sk_op("mdgat_sinkhorn_extract", sk_op_call(B, N, M, scores, bin_score, iters, Z_or_null, workspace, workspace_bytes, stream, Z_fallback_or_null), nullptr, &ex);
}

// ---- the two above on a ragged batch: the streaming kernel's ragged instantiations (sinkhorn.hip) ----
extern "C" int mdgat_sinkhorn_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                     const int32_t* counts1_host, const float* scores, float bin_score, int iters, float* Z, void* stream) {
    const RaggedCounts counts{counts0, counts1, counts0_host, counts1_host};
    return sk_op("mdgat_sinkhorn_ragged", sk_op_call(B, Np, Mp, scores, bin_score, iters, Z, nullptr, 0, stream), &counts, nullptr);
}

extern "C" int mdgat_sinkhorn_extract_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                             const int32_t* counts1_host, const float* scores, float bin_score, int iters, int mode,
                                             float match_threshold, int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                                             float* Z_or_null, void* workspace, size_t workspace_bytes, void* stream) {
    const RaggedCounts counts{counts0, counts1, counts0_host, counts1_host};
    const SkExtract ex{mode, match_threshold, matches0, matches1, mscores0, mscores1};
    return sk_op("mdgat_sinkhorn_extract_ragged", sk_op_call(B, Np, Mp, scores, bin_score, iters, Z_or_null, workspace, workspace_bytes, stream), &counts, &ex);
}

// ---- the two above in wide slots (up to MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS), on the one-workgroup kernel or - split - the split form ----
extern "C" int mdgat_sinkhorn_ragged_wide(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                          const int32_t* counts1_host, const float* scores, float bin_score, int iters, float* Z, int split,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    const RaggedCounts counts{counts0, counts1, counts0_host, counts1_host};
    SkCall c = sk_op_call(B, Np, Mp, scores, bin_score, iters, Z, workspace, workspace_bytes, stream);
    c.wide = true; c.split = split != 0;
    return sk_op("mdgat_sinkhorn_ragged_wide", c, &counts, nullptr);
}

extern "C" int mdgat_sinkhorn_extract_ragged_wide(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                                  const int32_t* counts1_host, const float* scores, float bin_score, int iters, int mode,
                                                  float match_threshold, int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                                                  float* Z_or_null, int split, void* workspace, size_t workspace_bytes, void* stream) {
    const RaggedCounts counts{counts0, counts1, counts0_host, counts1_host};
    const SkExtract ex{mode, match_threshold, matches0, matches1, mscores0, mscores1};
    SkCall c = sk_op_call(B, Np, Mp, scores, bin_score, iters, Z_or_null, workspace, workspace_bytes, stream);
    c.wide = true; c.split = split != 0;
    return sk_op("mdgat_sinkhorn_extract_ragged_wide", c, &counts, &ex);
}

extern "C" void mdgat_ragged_wide_launches(uint64_t counts[MDGAT_RAGGED_WIDE_COUNTERS]) {
    if (counts) ragged_wide_launch_counts(counts);
}

extern "C" int mdgat_extract(int B, int N, int M, const float* Z, int mode, float match_threshold, int64_t* matches0,
                             int64_t* matches1, float* mscores0, float* mscores1, void* stream) {
    const SkExtract ex{mode, match_threshold, matches0, matches1, mscores0, mscores1};
    if (!Z || sk_outputs_null(ex)) { mdgat_set_error("mdgat_extract: null pointer"); return MDGAT_ERR_BAD_ARG; }
    return launch_extract(B, N, M, Z, ex, static_cast<hipStream_t>(stream));      // (its mode check: extract_check_mode, behind the empty-batch return)
}

extern "C" size_t mdgat_attention_workspace_bytes(int B, int N, int M) {
    if (B <= 0 || N <= 0 || M <= 0) return 0;
    return mdgat_qkv16_halves(B, N, M) * sizeof(_Float16);
}

// ONE body for the four attention entries: the q | k | v split into the workspace, then the forward's launcher.  counts: null for the uniform entries;
// a ragged batch has them on the device for the kernel, on the host for the checks made before the launch (wide: slots of up to
// MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS per frame).
static int attention_op(const char* who, int B, int N, int M, int cross, int topk, const float* qkv, float* msg, uint32_t* sel, void* workspace,
                        size_t workspace_bytes, void* stream, const RaggedCounts* counts = nullptr, bool wide = false) {
    if (!qkv || !msg || !workspace) { mdgat_set_error("%s: null pointer", who); return MDGAT_ERR_BAD_ARG; }
    AttnCall c{B, N, M, cross, topk};
    c.msg = msg; c.sel = sel; c.wide = wide; c.stream = static_cast<hipStream_t>(stream);
    if (counts) {
        if (topk < 0 || B < 0 || N <= 0 || M <= 0) { mdgat_set_error("%s: bad shape B=%d Np=%d Mp=%d topk=%d", who, B, N, M, topk); return MDGAT_ERR_BAD_ARG; }
        if (B == 0) return MDGAT_OK;
        const int limit = wide ? MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS : MDGAT_RAGGED_FP32_MAX_KEYPOINTS;
        if (N > limit || M > limit) {
            mdgat_set_error("%s: padded sizes %d x %d: fp32 ragged batches hold at most %d keypoints per frame", who, N, M, limit);
            return MDGAT_ERR_UNSUPPORTED;
        }
        if (int rc = mdgat_check_ragged(who, B, N, M, *counts, nullptr, &topk, 1, nullptr)) return rc;
        c.cnt0 = counts->cnt0; c.cnt1 = counts->cnt1;
    } else if (topk < 0) { mdgat_set_error("%s: topk < 0", who); return MDGAT_ERR_BAD_ARG; }
    if (workspace_bytes < mdgat_attention_workspace_bytes(B, N, M) || (reinterpret_cast<uintptr_t>(workspace) & 15)) {
        mdgat_set_error("%s: workspace too small or not 16-byte aligned", who);
        return MDGAT_ERR_BAD_ARG;
    }
    c.qkv = mdgat_qkv16_carve(static_cast<_Float16*>(workspace), B, N, M);
    if (int rc = launch_qkv_split(B, N, M, qkv, c.qkv, c.stream)) return rc;      // (a ragged batch: over the padded rows - the kernels read none beyond a pair's counts)
    return launch_attention(c);
}

extern "C" int mdgat_attention(int B, int N, int M, int cross, int topk, const float* qkv, float* msg, void* workspace,
                               size_t workspace_bytes, void* stream) {
    return attention_op("mdgat_attention", B, N, M, cross, topk, qkv, msg, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int mdgat_attention_sel(int B, int N, int M, int cross, int topk, const float* qkv, float* msg, uint32_t* sel,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    return attention_op("mdgat_attention", B, N, M, cross, topk, qkv, msg, sel, workspace, workspace_bytes, stream);
}

extern "C" int mdgat_attention_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                      const int32_t* counts1_host, int cross, int topk, const float* qkv, float* msg, uint32_t* sel, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    const RaggedCounts counts{counts0, counts1, counts0_host, counts1_host};
    return attention_op("mdgat_attention_ragged", B, Np, Mp, cross, topk, qkv, msg, sel, workspace, workspace_bytes, stream, &counts);
}

extern "C" int mdgat_attention_ragged_wide(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                           const int32_t* counts1_host, int cross, int topk, const float* qkv, float* msg, uint32_t* sel, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    const RaggedCounts counts{counts0, counts1, counts0_host, counts1_host};
    return attention_op("mdgat_attention_ragged_wide", B, Np, Mp, cross, topk, qkv, msg, sel, workspace, workspace_bytes, stream, &counts, true);
}

extern "C" int mdgat_attention_plan(int B, int N, int M, int topk, int tap, int mode, int* split, int* tiles) {
    const AttnPlan p = topk < 0 ? AttnPlan{-1, 0, 0, MDGAT_ERR_BAD_ARG} : attention_plan(B, N, M, topk, tap != 0, mode);   // (topk < 0: mdgat_attention refuses)
    if (split) *split = p.split;
    if (tiles) *tiles = p.tiles;
    return p.form;
}

extern "C" int mdgat_attention_ragged_plan(int B, int Np, int Mp, int topk, int tap, int wide, int* split, int* tiles) {
    const AttnPlan p = attention_plan(B, Np, Mp, topk, tap != 0, 0, true, wide != 0);
    if (split) *split = p.split;
    if (tiles) *tiles = p.tiles;
    return p.form;
}

extern "C" void mdgat_attention_launches(uint64_t counts[MDGAT_ATTENTION_FORMS]) {
    if (counts) attention_launch_counts(counts);
}

extern "C" int mdgat_sinkhorn_plan(int B, int N, int M, int cus, const void* workspace, size_t workspace_bytes, int fallback_buffer, int ragged,
                                   int32_t out[MDGAT_SINKHORN_PLAN_WORDS]) {
    const bool usable = !ragged && B > 0 && N > 0 && M > 0 && sinkhorn_workspace_usable(B, N, M, workspace, workspace_bytes);
    const SkPlan p = sinkhorn_plan(B, N, M, cus, usable, fallback_buffer != 0, ragged != 0);
    if (out) {
        const int32_t w[MDGAT_SINKHORN_PLAN_WORDS] = {p.scaling, p.stream, p.GR, p.GC, p.ngroups, p.xcd_map, p.grid, p.cooperative};
        for (int i = 0; i < MDGAT_SINKHORN_PLAN_WORDS; ++i) out[i] = w[i];
    }
    return p.path;
}

extern "C" void mdgat_sinkhorn_launches(uint64_t counts[MDGAT_SINKHORN_COUNTERS]) {
    if (counts) sinkhorn_launch_counts(counts);
}

extern "C" int mdgat_layer_plan(int R, int N, int M, int do_mlp, int mode3, int* workgroups, int* keypoints_per_workgroup, int* v_store) {
    const LayerPlan p = layer_plan(R, N, M, do_mlp, mode3);
    if (workgroups) *workgroups = p.workgroups;
    if (keypoints_per_workgroup) *keypoints_per_workgroup = p.keypoints;
    if (v_store) *v_store = p.v_store;
    return p.form;
}

extern "C" void mdgat_layer_launches(uint64_t counts[MDGAT_LAYER_FORMS]) {
    if (counts) layer_launch_counts(counts);
}

extern "C" int mdgat_attention_qk_probe(int B, int N, int M, int cross, const float* qkv, float* msg, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    if (!qkv || !msg || !workspace) { mdgat_set_error("mdgat_attention_qk_probe: null pointer"); return MDGAT_ERR_BAD_ARG; }
    if (workspace_bytes < mdgat_attention_workspace_bytes(B, N, M) || (reinterpret_cast<uintptr_t>(workspace) & 15)) {
        mdgat_set_error("mdgat_attention_qk_probe: workspace too small or not 16-byte aligned");
        return MDGAT_ERR_BAD_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Qkv16 q16 = mdgat_qkv16_carve(static_cast<_Float16*>(workspace), B, N, M);
    // (qkv == workspace: the operands are already there in the library's split layout - bench.py times only the probe)
    if (static_cast<const void*>(qkv) != workspace)
        if (int rc = launch_qkv_split(B, N, M, qkv, q16, s)) return rc;
    return launch_attention_qk_probe(B, N, M, cross, q16, msg, s);
}

extern "C" int mdgat_attention_qk_probe_sets(int B, int N, int M, int cross, int nq_sets, const float* qkv, float* msg, void* workspace,
                                             size_t workspace_bytes, void* stream) {
    if (!qkv || !msg || !workspace) { mdgat_set_error("mdgat_attention_qk_probe_sets: null pointer"); return MDGAT_ERR_BAD_ARG; }
    if (workspace_bytes < mdgat_attention_workspace_bytes(B, N, M) || (reinterpret_cast<uintptr_t>(workspace) & 15)) {
        mdgat_set_error("mdgat_attention_qk_probe_sets: workspace too small or not 16-byte aligned");
        return MDGAT_ERR_BAD_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Qkv16 q16 = mdgat_qkv16_carve(static_cast<_Float16*>(workspace), B, N, M);
    if (static_cast<const void*>(qkv) != workspace)
        if (int rc = launch_qkv_split(B, N, M, qkv, q16, s)) return rc;
    return launch_qk_phase_probe(B, N, M, cross, nq_sets, q16, msg, s);
}

extern "C" int mdgat_pointwise(int M, int N, int K, const float* A, int lda, const float* W, int ldw, const float* bias,
                               int relu, const float* R, int ldr, float* C, int ldc, void* stream) {
    if (!A || !W || !C) { mdgat_set_error("mdgat_pointwise: null pointer"); return MDGAT_ERR_BAD_ARG; }
    const GemmArgs g{A, lda, K, nullptr, 0, W, ldw, bias, R, ldr, C, ldc, M, N, K, relu, 1.f, 1, 0, 0, 0};
    return launch_gemm(g, static_cast<hipStream_t>(stream));
}

extern "C" size_t mdgat_knn_workspace_bytes(int B, int C, int N, int M) { return mdgat_knn_ws_bytes_impl(B, C, N, M); }

extern "C" int mdgat_knn(int B, int C, int N, int M, int k, const float* x, const float* src, int64_t* idx, int64_t* adj,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !src || !idx) { mdgat_set_error("mdgat_knn: null pointer"); return MDGAT_ERR_BAD_ARG; }
    return launch_knn(B, C, N, M, k, x, src, idx, adj, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int mdgat_pose(int B, int N, int M, const float* kpts0, const float* kpts1, const int64_t* matches0,
                          const double* T_gt, double inlier_dist, double* T, double* stats, void* stream) {
    if (!kpts0 || !kpts1 || !matches0 || !T || !stats) { mdgat_set_error("mdgat_pose: null pointer"); return MDGAT_ERR_BAD_ARG; }
    if (N <= 0 || M <= 0) { mdgat_set_error("mdgat_pose: empty frame"); return MDGAT_ERR_BAD_ARG; }
    return launch_pose(B, N, M, kpts0, kpts1, matches0, T_gt, inlier_dist, T, stats, static_cast<hipStream_t>(stream));
}

extern "C" int mdgat_gt_matches(int B, int N, int M, const float* kpts0, const float* kpts1, const double* T0, const double* T1,
                                double threshold, int mutual, int64_t* gt0, int64_t* gt1, int64_t* rep, void* stream) {
    if (!kpts0 || !kpts1 || !gt0 || !gt1 || !rep) { mdgat_set_error("mdgat_gt_matches: null pointer"); return MDGAT_ERR_BAD_ARG; }
    if (N <= 0 || M <= 0) { mdgat_set_error("mdgat_gt_matches: empty frame"); return MDGAT_ERR_BAD_ARG; }
    return launch_gt_match(B, N, M, kpts0, kpts1, T0, T1, threshold, mutual, gt0, gt1, rep, static_cast<hipStream_t>(stream));
}

extern "C" int mdgat_gt_matches_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                       const int32_t* counts1_host, const float* kpts0, const float* kpts1, const double* T0, const double* T1,
                                       double threshold, int mutual, int64_t* gt0, int64_t* gt1, int64_t* rep, void* stream) {
    if (B < 0) { mdgat_set_error("mdgat_gt_matches_ragged: negative batch"); return MDGAT_ERR_BAD_ARG; }
    if (Np <= 0 || Mp <= 0) { mdgat_set_error("mdgat_gt_matches_ragged: empty frame"); return MDGAT_ERR_BAD_ARG; }
    if (!kpts0 || !kpts1 || !gt0 || !gt1 || !rep) { mdgat_set_error("mdgat_gt_matches_ragged: null pointer"); return MDGAT_ERR_BAD_ARG; }
    if (int rc = mdgat_check_ragged("mdgat_gt_matches_ragged", B, Np, Mp, RaggedCounts{counts0, counts1, counts0_host, counts1_host}, nullptr, nullptr, 0, nullptr)) return rc;
    return launch_gt_match(B, Np, Mp, kpts0, kpts1, T0, T1, threshold, mutual, gt0, gt1, rep, static_cast<hipStream_t>(stream), counts0, counts1);
}

extern "C" int mdgat_eval_metrics(int B, int N, int M, const int64_t* matches0, const int64_t* matches1, const int64_t* gt0, const int64_t* gt1,
                                  const float* kpts0, const float* kpts1, const double* T_gt, double inlier_dist, double* metrics, double* T,
                                  unsigned* bad_index, void* stream) {
    if (B < 0) { mdgat_set_error("mdgat_eval_metrics: negative batch"); return MDGAT_ERR_BAD_ARG; }
    if (N <= 0 || M <= 0) { mdgat_set_error("mdgat_eval_metrics: empty frame"); return MDGAT_ERR_BAD_ARG; }
    if (B > 0 && (!matches0 || !matches1 || !gt0 || !gt1 || !kpts0 || !kpts1 || !metrics || !T)) {
        mdgat_set_error("mdgat_eval_metrics: null pointer");
        return MDGAT_ERR_BAD_ARG;
    }
    return launch_eval_metrics(B, N, M, matches0, matches1, gt0, gt1, kpts0, kpts1, T_gt, inlier_dist, metrics, T, bad_index,
                               static_cast<hipStream_t>(stream));
}

extern "C" int mdgat_eval_metrics_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                         const int32_t* counts1_host, const int64_t* matches0, const int64_t* matches1, const int64_t* gt0,
                                         const int64_t* gt1, const float* kpts0, const float* kpts1, const double* T_gt, double inlier_dist,
                                         double* metrics, double* T, unsigned* bad_index, void* stream) {
    if (B < 0) { mdgat_set_error("mdgat_eval_metrics_ragged: negative batch"); return MDGAT_ERR_BAD_ARG; }
    if (Np <= 0 || Mp <= 0) { mdgat_set_error("mdgat_eval_metrics_ragged: empty frame"); return MDGAT_ERR_BAD_ARG; }
    if (B > 0) {      // (an empty batch may come without pointers)
        if (!matches0 || !matches1 || !gt0 || !gt1 || !kpts0 || !kpts1 || !metrics || !T) { mdgat_set_error("mdgat_eval_metrics_ragged: null pointer"); return MDGAT_ERR_BAD_ARG; }
        if (int rc = mdgat_check_ragged("mdgat_eval_metrics_ragged", B, Np, Mp, RaggedCounts{counts0, counts1, counts0_host, counts1_host}, nullptr, nullptr, 0, nullptr)) return rc;
    }
    return launch_eval_metrics(B, Np, Mp, matches0, matches1, gt0, gt1, kpts0, kpts1, T_gt, inlier_dist, metrics, T, bad_index,
                               static_cast<hipStream_t>(stream), counts0, counts1);
}

extern "C" int mdgat_pointwise_f64(int M, int N, int K, const double* A, int lda, const double* W, int ldw, const double* bias,
                                   int relu, const double* R, int ldr, double* C, int ldc, void* stream) {
    if (!A || !W || !C) { mdgat_set_error("mdgat_pointwise_f64: null pointer"); return MDGAT_ERR_BAD_ARG; }
    const GemmF64Args g{A, lda, K, nullptr, 0, W, ldw, bias, R, ldr, C, ldc, M, N, K, relu, nullptr};
    return launch_gemm_f64(g, static_cast<hipStream_t>(stream));
}

extern "C" int mdgat_gemm_f64_plan(int M, int N, int K, int K0, int batch, int aligned, int bnt, int cus) {
    return gemm_f64_plan_index(M, N, K, K0, batch, aligned, bnt, cus);
}

extern "C" void mdgat_gemm_f64_launches(uint64_t counts[10]) {
    if (counts) gemm_f64_launch_counts(counts);
}

extern "C" int mdgat_attention_f64_plan(int B, int N, int M, int topk, int tap, int ragged, int cnt_min, int form, int cus) {
    return attention_f64_plan(B, N, M, topk, tap, ragged, cnt_min, form, cus).form;
}

extern "C" int mdgat_attention_f64_geometry(int B, int N, int M, int topk, int tap, int ragged, int cnt_min, int form, int cus, int* queries, int* tiles,
                                            int* workgroups, size_t* lds_bytes) {
    const AttnF64Plan p = attention_f64_plan(B, N, M, topk, tap, ragged, cnt_min, form, cus);
    if (queries) *queries = p.queries;
    if (tiles) *tiles = p.tiles;
    if (workgroups) *workgroups = p.workgroups;
    if (lds_bytes) *lds_bytes = p.lds;
    return p.form;
}

extern "C" void mdgat_attention_f64_launches(uint64_t counts[MDGAT_ATTENTION_F64_FORMS]) {
    if (counts) attention_f64_launch_counts(counts);
}

extern "C" int mdgat_layer_f64_plan(int R, int encoder, int has_hid, int chained, int mode, int cus, int* workgroups, int* rows_per_workgroup) {
    const LayerF64Plan p = layer_f64_plan(R, encoder, has_hid, chained, mode, cus);
    if (workgroups) *workgroups = p.workgroups;
    if (rows_per_workgroup) *rows_per_workgroup = p.rows;
    return p.form;
}

extern "C" void mdgat_layer_f64_launches(uint64_t counts[MDGAT_LAYER_F64_FORMS]) {
    if (counts) layer_f64_launch_counts(counts);
}

extern "C" int mdgat_sinkhorn_f64_plan(int N, int M, int ragged, int ragged_mode, int form, int history, int* slabs, int* chunks) {
    return sinkhorn_f64_plan(N, M, ragged, ragged_mode, form, history, slabs, chunks);
}

extern "C" void mdgat_sinkhorn_f64_launches(uint64_t counts[MDGAT_SINKHORN_F64_FORMS]) {
    if (counts) sinkhorn_f64_launches(counts);
}

// ---- the matching head (final_proj, the score matrix) and its backward: csrc/head_grad.hip ----
// the shape and buffer checks of the gradient entries (this section and the two below)
// nmax: keypoints per frame; rows: the rows the largest array of a pair holds
static int grad_shape(const char* who, int B, int N, int M, int nmax, int rows) {
    if (B < 0 || N <= 0 || M <= 0) { mdgat_set_error("%s: bad shape B=%d N=%d M=%d", who, B, N, M); return MDGAT_ERR_BAD_ARG; }
    if (N > nmax || M > nmax) { mdgat_set_error("%s: %d x %d keypoints > %d supported", who, N, M, nmax); return MDGAT_ERR_UNSUPPORTED; }
    if ((long long)B * rows > (1 << 24)) { mdgat_set_error("%s: B=%d N=%d M=%d: more than 2^24 rows (%d per pair)", who, B, N, M, rows); return MDGAT_ERR_UNSUPPORTED; }
    return MDGAT_OK;
}
static int grad_buffer(const char* who, const char* what, const void* p, size_t have, size_t need) {
    if (!p || have < need || (reinterpret_cast<uintptr_t>(p) & 255)) { mdgat_set_error("%s: %s too small or not 256-byte aligned", who, what); return MDGAT_ERR_BAD_ARG; }
    return MDGAT_OK;
}

constexpr int MATCH_HEAD_NMAX = 2175;             // the Sinkhorn backward's limit (sinkhorn_grad.hip), which the chain composes with
static int match_head_shape(const char* who, int B, int N, int M) { return grad_shape(who, B, N, M, MATCH_HEAD_NMAX, N > M ? N : M); }

extern "C" size_t mdgat_match_head_workspace_bytes(int B, int N, int M) {
    if (B <= 0 || match_head_shape("mdgat_match_head_workspace_bytes", B, N, M)) return 0;
    return match_head_f64_workspace_bytes(B, N, M);
}

extern "C" int mdgat_match_head_f64(int B, int N, int M, const double* desc0, const double* desc1, const double* W, const double* bias,
                                    double* scores, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = match_head_shape("mdgat_match_head_f64", B, N, M)) return rc;
    if (B == 0) return MDGAT_OK;
    if (!desc0 || !desc1 || !W || !bias || !scores) { mdgat_set_error("mdgat_match_head_f64: null pointer"); return MDGAT_ERR_BAD_ARG; }
    if (int rc = grad_buffer("mdgat_match_head_f64", "workspace", workspace, workspace_bytes, match_head_f64_workspace_bytes(B, N, M))) return rc;
    return launch_match_head_f64(B, N, M, desc0, desc1, W, bias, scores, workspace, static_cast<hipStream_t>(stream));
}

extern "C" int mdgat_match_head_backward(int B, int N, int M, const double* desc0, const double* desc1, const double* W, const double* bias,
                                         const double* dscores, double* ddesc0, double* ddesc1, double* dW, double* dbias,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = match_head_shape("mdgat_match_head_backward", B, N, M)) return rc;
    if (B == 0) return MDGAT_OK;
    if (!desc0 || !desc1 || !W || !bias || !dscores) { mdgat_set_error("mdgat_match_head_backward: null pointer"); return MDGAT_ERR_BAD_ARG; }
    if (int rc = grad_buffer("mdgat_match_head_backward", "workspace", workspace, workspace_bytes, match_head_f64_workspace_bytes(B, N, M))) return rc;
    return launch_match_head_backward_f64(B, N, M, desc0, desc1, W, bias, dscores, ddesc0, ddesc1, dW, dbias, workspace, static_cast<hipStream_t>(stream));
}

// ---- the reference's MLP in training mode (Conv1d(k=1) + batch-statistics BatchNorm + ReLU) and its backward: csrc/mlp_grad.hip ----
constexpr int MLP_CMAX = 512;
static int mlp_shape(const char* who, const mdgat_mlp_desc* d) {
    if (!d) { mdgat_set_error("%s: null descriptor", who); return MDGAT_ERR_BAD_ARG; }
    if (d->R < 0 || d->K0 < 0 || d->K1 < 0) { mdgat_set_error("%s: bad shape R=%d K0=%d K1=%d", who, d->R, d->K0, d->K1); return MDGAT_ERR_BAD_ARG; }
    if (d->n_conv < 1 || d->n_conv > MDGAT_MLP_MAX_CONVS) { mdgat_set_error("%s: %d convolutions, 1 to %d supported", who, d->n_conv, MDGAT_MLP_MAX_CONVS); return MDGAT_ERR_UNSUPPORTED; }
    if (d->K0 < 1 || d->K0 + d->K1 > MLP_CMAX) { mdgat_set_error("%s: %d + %d input channels, 1 to %d supported", who, d->K0, d->K1, MLP_CMAX); return MDGAT_ERR_UNSUPPORTED; }
    for (int l = 0; l < d->n_conv; ++l)
        if (d->C[l] < 16 || d->C[l] > MLP_CMAX || d->C[l] % 16) {
            mdgat_set_error("%s: convolution %d has %d output channels: a multiple of 16 up to %d is supported", who, l, d->C[l], MLP_CMAX);
            return MDGAT_ERR_UNSUPPORTED;
        }
    if (d->R > (1 << 24)) { mdgat_set_error("%s: %d rows: more than 2^24", who, d->R); return MDGAT_ERR_UNSUPPORTED; }
    if (d->R == 1 && d->training && d->n_conv > 1) {
        mdgat_set_error("%s: batch statistics need more than one row (R = 1 in training mode)", who);
        return MDGAT_ERR_BAD_ARG;
    }
    return MDGAT_OK;
}
static int mlp_pointers(const char* who, const mdgat_mlp_desc* d, const double* x0, const double* x1) {
    bool ok = x0 && (d->K1 == 0 || x1);
    for (int l = 0; l < d->n_conv; ++l) ok = ok && d->W[l] && d->bias[l];
    for (int l = 0; l + 1 < d->n_conv; ++l)
        ok = ok && d->gamma[l] && d->beta[l] && d->running_mean[l] && d->running_var[l] && (!d->training || d->num_batches_tracked[l]);
    if (!ok) { mdgat_set_error("%s: null pointer", who); return MDGAT_ERR_BAD_ARG; }
    for (int l = 0; l + 1 < d->n_conv; ++l)
        if (!(d->eps[l] >= 0.0) || (d->training && !(d->momentum[l] >= 0.0 && d->momentum[l] <= 1.0))) {
            mdgat_set_error("%s: BatchNorm %d: eps=%g momentum=%g", who, l, d->eps[l], d->momentum[l]);
            return MDGAT_ERR_BAD_ARG;
        }
    return MDGAT_OK;
}
extern "C" size_t mdgat_mlp_workspace_bytes(const mdgat_mlp_desc* d, int part) {
    if (mlp_shape("mdgat_mlp_workspace_bytes", d) || d->R == 0 || part < 0 || part > 1) return 0;
    return part == 0 ? mlp_f64_saved_bytes(*d) : mlp_f64_backward_workspace_bytes(*d);
}

extern "C" int mdgat_mlp_forward_f64(const mdgat_mlp_desc* d, const double* x0, const double* x1, double* out, void* saved, size_t saved_bytes,
                                     void* stream) {
    const char* who = "mdgat_mlp_forward_f64";
    if (int rc = mlp_shape(who, d)) return rc;
    if (d->R == 0) return MDGAT_OK;
    if (int rc = mlp_pointers(who, d, x0, x1)) return rc;
    if (!out) { mdgat_set_error("%s: null pointer", who); return MDGAT_ERR_BAD_ARG; }
    if (int rc = grad_buffer(who, "saved", saved, saved_bytes, mlp_f64_saved_bytes(*d))) return rc;
    return launch_mlp_forward_f64(*d, x0, x1, out, saved, static_cast<hipStream_t>(stream));
}

extern "C" int mdgat_mlp_forward_residual_f64(const mdgat_mlp_desc* d, const double* x0, const double* x1, const double* residual, double* out,
                                              void* saved, size_t saved_bytes, void* stream) {
    const char* who = "mdgat_mlp_forward_residual_f64";
    if (int rc = mlp_shape(who, d)) return rc;
    if (d->R == 0) return MDGAT_OK;
    if (int rc = mlp_pointers(who, d, x0, x1)) return rc;
    if (!out || !residual) { mdgat_set_error("%s: null pointer", who); return MDGAT_ERR_BAD_ARG; }
    if (int rc = grad_buffer(who, "saved", saved, saved_bytes, mlp_f64_saved_bytes(*d))) return rc;
    return launch_mlp_forward_f64(*d, x0, x1, out, saved, static_cast<hipStream_t>(stream), residual);
}

extern "C" int mdgat_mlp_backward_f64(const mdgat_mlp_desc* d, const double* x0, const double* x1, const void* saved, size_t saved_bytes,
                                      const double* dout, const mdgat_mlp_grads* grads, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mdgat_mlp_backward_f64";
    if (int rc = mlp_shape(who, d)) return rc;
    if (d->R == 0) return MDGAT_OK;
    if (int rc = mlp_pointers(who, d, x0, x1)) return rc;
    if (!dout || !grads) { mdgat_set_error("%s: null pointer", who); return MDGAT_ERR_BAD_ARG; }
    if (int rc = grad_buffer(who, "saved", saved, saved_bytes, mlp_f64_saved_bytes(*d))) return rc;
    if (int rc = grad_buffer(who, "workspace", workspace, workspace_bytes, mlp_f64_backward_workspace_bytes(*d))) return rc;
    return launch_mlp_backward_f64(*d, x0, x1, saved, dout, *grads, workspace, static_cast<hipStream_t>(stream));
}

// ONE body for the two fp64 attention entries, as attention_op is for the fp32-class ones.  counts: null for the uniform entry; a ragged batch
// has them on the device for the kernel, on the host for the checks made before the launch.
static int attention_f64_op(const char* who, AttnF64Call c, const RaggedCounts* counts) {
    if (!c.qkv || !c.msg) { mdgat_set_error("%s: null pointer", who); return MDGAT_ERR_BAD_ARG; }
    if (counts) {
        if (c.topk < 0 || c.B < 0 || c.N <= 0 || c.M <= 0) { mdgat_set_error("%s: bad shape B=%d Np=%d Mp=%d topk=%d", who, c.B, c.N, c.M, c.topk); return MDGAT_ERR_BAD_ARG; }
        if (int rc = mdgat_check_ragged(who, c.B, c.N, c.M, *counts, nullptr, &c.topk, 1, &c.cnt_min)) return rc;
        c.cnt0 = counts->cnt0; c.cnt1 = counts->cnt1;
    } else if (c.topk < 0) { mdgat_set_error("%s: topk < 0", who); return MDGAT_ERR_BAD_ARG; }
    return launch_attention_f64(c);
}

extern "C" int mdgat_attention_f64(int B, int N, int M, int cross, int topk, const double* qkv, double* msg, uint32_t* sel, void* stream) {
    AttnF64Call c{B, N, M, cross, topk, qkv, msg, sel};
    c.stream = static_cast<hipStream_t>(stream);
    return attention_f64_op("mdgat_attention_f64", c, nullptr);
}

extern "C" int mdgat_attention_f64_ragged(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                          const int32_t* counts1_host, int cross, int topk, const double* qkv, double* msg, uint32_t* sel, void* stream) {
    const RaggedCounts counts{counts0, counts1, counts0_host, counts1_host};
    AttnF64Call c{B, Np, Mp, cross, topk, qkv, msg, sel};
    c.stream = static_cast<hipStream_t>(stream);
    return attention_f64_op("mdgat_attention_f64_ragged", c, &counts);
}

// ---- the backward of mdgat_attention_f64: csrc/attention_grad.hip ----
constexpr int ATTENTION_GRAD_NMAX = 2048;         // the forward's limit for dynamic layers
static int attention_grad_shape(const char* who, int B, int N, int M) { return grad_shape(who, B, N, M, ATTENTION_GRAD_NMAX, N + M); }

extern "C" size_t mdgat_attention_backward_workspace_bytes(int B, int N, int M) {
    if (B <= 0 || attention_grad_shape("mdgat_attention_backward_workspace_bytes", B, N, M)) return 0;
    return attention_backward_f64_workspace_bytes(B, N, M);
}

extern "C" int mdgat_attention_backward_f64(int B, int N, int M, int cross, int topk, const double* qkv, const uint32_t* sel, const double* dmsg,
                                            double* dqkv, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mdgat_attention_backward_f64";
    if (int rc = attention_grad_shape(who, B, N, M)) return rc;
    if (topk < 0 || topk > (N < M ? N : M)) { mdgat_set_error("%s: k=%d outside [0, %d], the number of keys", who, topk, N < M ? N : M); return MDGAT_ERR_BAD_ARG; }
    if (B == 0) return MDGAT_OK;
    if (!qkv || !dmsg || !dqkv) { mdgat_set_error("%s: null pointer", who); return MDGAT_ERR_BAD_ARG; }
    if (topk > 0 && !sel) { mdgat_set_error("%s: topk=%d needs the forward's selection words (sel)", who, topk); return MDGAT_ERR_BAD_ARG; }
    if (int rc = grad_buffer(who, "workspace", workspace, workspace_bytes, attention_backward_f64_workspace_bytes(B, N, M))) return rc;
    return launch_attention_backward_f64(B, N, M, cross, topk, qkv, sel, dmsg, dqkv, workspace, static_cast<hipStream_t>(stream));
}

// ---- the frame maximum of the pooled descriptor encoder as a call of its own, and its backward: csrc/pool_f64.hip ----
extern "C" int mdgat_frame_max_f64(int B, int n, const double* e, double* g, int64_t* idx, void* stream) {
    const char* who = "mdgat_frame_max_f64";
    if (B < 0 || n < 1 || (long long)B * n > (1LL << 24)) { mdgat_set_error("%s: bad shape B=%d n=%d (n >= 1, at most 2^24 rows)", who, B, n); return MDGAT_ERR_BAD_ARG; }
    if (B == 0) return MDGAT_OK;
    if (!e || !g) { mdgat_set_error("%s: null pointer", who); return MDGAT_ERR_BAD_ARG; }
    return launch_frame_max_f64(FrameMaxArgs{e, B, n, 0, nullptr, nullptr, g, idx}, static_cast<hipStream_t>(stream));
}

extern "C" int mdgat_frame_max_backward_f64(int B, int n, const double* dg, const int64_t* idx, double* de, void* stream) {
    const char* who = "mdgat_frame_max_backward_f64";
    if (B < 0 || n < 1 || (long long)B * n > (1LL << 24)) { mdgat_set_error("%s: bad shape B=%d n=%d (n >= 1, at most 2^24 rows)", who, B, n); return MDGAT_ERR_BAD_ARG; }
    if (B == 0) return MDGAT_OK;
    if (!dg || !idx || !de) { mdgat_set_error("%s: null pointer", who); return MDGAT_ERR_BAD_ARG; }
    return launch_frame_max_backward_f64(B, n, dg, idx, de, static_cast<hipStream_t>(stream));
}
