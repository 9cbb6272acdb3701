// Log-domain Sinkhorn optimal transport with dustbins and match extraction.
//
// Replaces: log_optimal_transport (mdgat.py:288-308), log_sinkhorn_iterations (279-285) and the match
// extraction of mdgat.py:441-483.
//
// The (N+1) x (M+1) coupling matrix of mdgat.py:298-299 is the N x M score block bordered by the constant
// bin score, so the kernel never materialises it: only the scores are read, the border terms are
// closed-form (alpha + v_M for every row, alpha + u_N for every column, and the dustbin row/column
// potentials are log-sum-exps of the potential vectors themselves).
//
// gfx950 mapping (round 1): one workgroup per pair, NW waves.  Per iteration the score block is streamed
// ONCE (it is L2/MALL resident: 1 MB per pair at N=M=512): a wave takes rows i = wave, wave+NW, ...;
// lane l holds columns l, l+64, ... of the row in registers, adds the column potentials (registers),
// reduces max / sum-of-exp2 across the wave -> u_i, and immediately folds the same registers, now with
// the fresh u_i, into per-lane running (max, sum) accumulators of the COLUMN log-sum-exps.  The NW
// per-wave column partials are merged through LDS -> v_j.  Everything is kept in the base-2 log domain
// (potentials carry a factor log2(e)) so each element costs v_exp_f32 without a pre-multiply.
#include "common.hpp"
#include <atomic>
#include <cstdlib>

namespace {

constexpr float NEG_BIG = -1.0e30f;   // finite stand-in for -inf (keeps a - b well defined)

struct SkArgs {
    const float* scores;      // [B][N][M]
    const float* alpha_dev;   // device scalar or nullptr
    float alpha_host;
    float* Z;                 // [B][N+1][M+1]
    int N, M, iters;
    // fallback use: a pair is only redone if bit 0 of *only_if is set (the cluster kernel's error word: the launch lost a partner
    // workgroup - every pair is redone) or its own word of pair_flags is (the pair's scores are beyond the range of the scaling
    // form - the other pairs of the launch keep the cluster kernel's result: what a pair gets does not depend on its batch);
    // a workgroup that runs raises status_fallback (host-mapped, optional)
    const unsigned* only_if;
    unsigned* status_fallback;
    const unsigned* pair_flags;
    // RAGGED instantiations only (device int32 [B]): pair b has cnt0[b] x cnt1[b] keypoints; N, M above are then the padded sizes - the strides of
    // scores and Z and what the LDS is sized for
    const int* cnt0;
    const int* cnt1;
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float lg2(float x) { return __builtin_amdgcn_logf(x); }   // v_log_f32 = log2

// log2-sum-exp2 over `n` LDS values plus one extra term, by one wave
__device__ __forceinline__ float wave_lse2(const float* x, int n, float extra, int lane) {
    float m = extra;
    for (int i = lane; i < n; i += 64) m = fmaxf(m, x[i]);
    m = wave_max(m);
    float s = 0.f;
    for (int i = lane; i < n; i += 64) s += ex2(x[i] - m);
    s = wave_sum(s) + ex2(extra - m);
    return m + lg2(s);
}

// sinkhorn_kernel's row pass of one iteration (its loop, as a function for the virtual waves below) as wave `vw` of `nw`: the rows vw, vw + nw, ...
// of the pair - u_i from the row's log-sum-exp over the lane's NC columns (v in registers), then the same registers, with the fresh u_i, folded
// into the lane's running (max, sum) of the COLUMN log-sum-exps - and the wave's column partials into pm / ps [vw][M].  A wave without rows
// stores (NEG_BIG, 0).
template <int NC>
__device__ __forceinline__ void sk_row_pass(const float* S, int Ms, int N, int M, int vw, int nw, int lane, float bM, float lmu, float* u,
                                            const float* v, float* pm, float* ps) {
    // column potentials of this lane's columns
    float vr[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int j = c * 64 + lane;
        vr[c] = j < M ? v[j] : 0.f;
    }
    float cm[NC], cs[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { cm[c] = NEG_BIG; cs[c] = 0.f; }

    for (int i = vw; i < N; i += nw) {
        const float* row = S + (size_t)i * Ms;
        float s[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int j = c * 64 + lane;
            s[c] = j < M ? row[j] * MDGAT_LOG2E : NEG_BIG;
        }
        float m = bM;
#pragma unroll
        for (int c = 0; c < NC; ++c) m = fmaxf(m, s[c] + vr[c]);
        m = wave_max(m);
        float e = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) e += ex2(s[c] + vr[c] - m);
        e = wave_sum(e) + ex2(bM - m);
        const float ui = lmu - (m + lg2(e));          // mdgat.py:283
        if (lane == 0) u[i] = ui;
#pragma unroll
        for (int c = 0; c < NC; ++c) {                // fold into the column LSEs (mdgat.py:284)
            const float w = s[c] + ui;
            const float nm = fmaxf(cm[c], w);
            cs[c] = cs[c] * ex2(cm[c] - nm) + ex2(w - nm);
            cm[c] = nm;
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int j = c * 64 + lane;
        if (j < M) { pm[vw * M + j] = cm[c]; ps[vw * M + j] = cs[c]; }
    }
}

// RAGGED: per-pair keypoint counts in padded slots (SkArgs::cnt0 / cnt1).  A pair then computes exactly what it computes alone through the
// instantiation its own M selects: rows, columns, norm, mu, nu and the dustbins are its own, only the strides are the slots'; a lane's column
// registers beyond the pair's M hold NEG_BIG as they do beyond M in a uniform launch - exp2 gives an exact 0, added last - so a wider NC
// changes no bit.  The rest of the pair's Z slot is written 0.
// The 8-wave RAGGED instantiations (NC = 16, 32: wide slots of more than 512 columns) also hold pairs of at most 512 columns, which alone run on 16
// waves: wave w there folds rows w, w + 16, ... into its column partials, and the 16 partials merge in ascending w.  Such a pair gets the same
// bits here from 16 VIRTUAL waves: physical wave w plays virtual wave w and then virtual wave w + 8, each over its own rows in ascending order
// with 8 column registers, which hold a pair of this width (sk_row_pass).
template <int NC, int NW, bool RAGGED = false>
__global__ __launch_bounds__(NW * 64) void sinkhorn_kernel(SkArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Ns = a.N, Ms = a.M;                // the strides (RAGGED: the padded sizes)
    int N = Ns, M = Ms;
    if constexpr (RAGGED) { N = __builtin_amdgcn_readfirstlane(a.cnt0[blockIdx.x]); M = __builtin_amdgcn_readfirstlane(a.cnt1[blockIdx.x]); }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (a.only_if) {
        const bool mine = (__hip_atomic_load(a.only_if, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1u) != 0 ||
                          (a.pair_flags && __hip_atomic_load(a.pair_flags + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0);
        if (!mine) return;
        if (tid == 0 && a.status_fallback) __hip_atomic_store(a.status_fallback, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const float* S = a.scores + (size_t)blockIdx.x * Ns * Ms;
    float* Z = a.Z + (size_t)blockIdx.x * (Ns + 1) * (Ms + 1);

    constexpr bool VWAVES = RAGGED && NW == 8;
    const bool two = VWAVES && M <= 512;                      // (workgroup-uniform) 16 virtual waves
    const int nwv = two ? 16 : NW;
    float* u = smem;                 // [N+1]
    float* v = u + (N + 1);          // [M+1]
    float* pm = v + (M + 1);         // [nwv][M]
    float* ps = pm + nwv * M;        // [nwv][M]

    const float alpha = (a.alpha_dev ? *a.alpha_dev : a.alpha_host) * MDGAT_LOG2E;
    const float norm = -logf((float)(N + M));                 // mdgat.py:301
    const float lmu = norm * MDGAT_LOG2E;                     // rows 0..N-1 (302)
    const float lmuN = (logf((float)M) + norm) * MDGAT_LOG2E; // dustbin row
    const float lnu = lmu;                                    // cols 0..M-1 (303)
    const float lnuM = (logf((float)N) + norm) * MDGAT_LOG2E; // dustbin column

    for (int i = tid; i <= N; i += NW * 64) u[i] = 0.f;
    for (int j = tid; j <= M; j += NW * 64) v[j] = 0.f;
    __syncthreads();

    for (int it = 0; it < a.iters; ++it) {
        if (two) {
            // a pair of at most 512 columns in a wide slot: the row pass as virtual wave `wave`, then as virtual wave `wave + 8`, of 16
            const float bM = alpha + v[M];
            if (wave == NW - 1) {
                const float lse = alpha + wave_lse2(v, M, v[M], lane);
                if (lane == 0) u[N] = lmuN - lse;
            }
            sk_row_pass<8>(S, Ms, N, M, wave, 16, lane, bM, lmu, u, v, pm, ps);
            sk_row_pass<8>(S, Ms, N, M, wave + 8, 16, lane, bM, lmu, u, v, pm, ps);
        } else {
            // column potentials of this lane's columns
            float vr[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int j = c * 64 + lane;
                vr[c] = j < M ? v[j] : 0.f;
            }
            const float bM = alpha + v[M];   // dustbin-column term of every row
            if (wave == NW - 1) {
                // dustbin row: u_N = log_mu_N - LSE_j(alpha + v_j), j = 0..M
                const float lse = alpha + wave_lse2(v, M, v[M], lane);
                if (lane == 0) u[N] = lmuN - lse;
            }
            float cm[NC], cs[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) { cm[c] = NEG_BIG; cs[c] = 0.f; }

            for (int i = wave; i < N; i += NW) {
                const float* row = S + (size_t)i * Ms;
                float s[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const int j = c * 64 + lane;
                    s[c] = j < M ? row[j] * MDGAT_LOG2E : NEG_BIG;
                }
                float m = bM;
#pragma unroll
                for (int c = 0; c < NC; ++c) m = fmaxf(m, s[c] + vr[c]);
                m = wave_max(m);
                float e = 0.f;
#pragma unroll
                for (int c = 0; c < NC; ++c) e += ex2(s[c] + vr[c] - m);
                e = wave_sum(e) + ex2(bM - m);
                const float ui = lmu - (m + lg2(e));          // mdgat.py:283
                if (lane == 0) u[i] = ui;
#pragma unroll
                for (int c = 0; c < NC; ++c) {                // fold into the column LSEs (mdgat.py:284)
                    const float w = s[c] + ui;
                    const float nm = fmaxf(cm[c], w);
                    cs[c] = cs[c] * ex2(cm[c] - nm) + ex2(w - nm);
                    cm[c] = nm;
                }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int j = c * 64 + lane;
                if (j < M) { pm[wave * M + j] = cm[c]; ps[wave * M + j] = cs[c]; }
            }
        }
        __syncthreads();
        const float bN = alpha + u[N];   // dustbin-row term of every column
        if (two) {      // the partials of the 16 virtual waves, in the same order and the same expressions
            for (int j = tid; j < M; j += NW * 64) {
                float m = bN;
#pragma unroll
                for (int w = 0; w < 16; ++w) m = fmaxf(m, pm[w * M + j]);
                float e = ex2(bN - m);
#pragma unroll
                for (int w = 0; w < 16; ++w) e += ps[w * M + j] * ex2(pm[w * M + j] - m);
                v[j] = lnu - (m + lg2(e));
            }
        } else
        for (int j = tid; j < M; j += NW * 64) {
            float m = bN;
#pragma unroll
            for (int w = 0; w < NW; ++w) m = fmaxf(m, pm[w * M + j]);
            float e = ex2(bN - m);
#pragma unroll
            for (int w = 0; w < NW; ++w) e += ps[w * M + j] * ex2(pm[w * M + j] - m);
            v[j] = lnu - (m + lg2(e));
        }
        if (wave == 0) {
            // dustbin column: v_M = log_nu_M - LSE_i(alpha + u_i), i = 0..N
            const float lse = alpha + wave_lse2(u, N, u[N], lane);
            if (lane == 0) v[M] = lnuM - lse;
        }
        __syncthreads();
    }

    // Z = couplings + u + v - norm (mdgat.py:285, 307), back in natural-log units
    const float uN = u[N], vM = v[M];
    for (int i = wave; i < N; i += NW) {
        const float ui = u[i];
        const float* row = S + (size_t)i * Ms;
        float* zr = Z + (size_t)i * (Ms + 1);
        for (int j = lane; j < M; j += 64) zr[j] = (row[j] * MDGAT_LOG2E + ui + v[j]) * MDGAT_LN2 - norm;
        if (lane == 0) zr[M] = (alpha + ui + vM) * MDGAT_LN2 - norm;
        if constexpr (RAGGED)
            for (int j = M + 1 + lane; j <= Ms; j += 64) zr[j] = 0.f;
    }
    float* zl = Z + (size_t)N * (Ms + 1);
    for (int j = tid; j <= M; j += NW * 64) zl[j] = (alpha + uN + v[j]) * MDGAT_LN2 - norm;
    if constexpr (RAGGED) {
        // the rest of the slot: the dustbin row's tail and the rows below it, which are contiguous
        float* rest = zl + M + 1;
        const int nrest = (Ms - M) + (Ns - N) * (Ms + 1);
        for (int j = tid; j < nrest; j += NW * 64) rest[j] = 0.f;
    }
}


// ------------------------------------------------------------------------------------------------
// helpers of the cluster kernel
constexpr int SLOT_STRIDE = 520;

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move(float identity, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, identity), __builtin_bit_cast(int, v),
                                                                 CTRL, ROW_MASK, 0xf, false));
}
// wave-wide reductions on the VALU (DPP row shifts + row broadcasts); result broadcast from lane 63
__device__ __forceinline__ float wave_max_dpp(float v) {
    v = fmaxf(v, dpp_move<0x111, 0xf>(NEG_BIG, v));   // row_shr:1
    v = fmaxf(v, dpp_move<0x112, 0xf>(NEG_BIG, v));   // row_shr:2
    v = fmaxf(v, dpp_move<0x114, 0xf>(NEG_BIG, v));   // row_shr:4
    v = fmaxf(v, dpp_move<0x118, 0xf>(NEG_BIG, v));   // row_shr:8
    v = fmaxf(v, dpp_move<0x142, 0xa>(NEG_BIG, v));   // row_bcast:15 -> rows 1, 3
    v = fmaxf(v, dpp_move<0x143, 0xc>(NEG_BIG, v));   // row_bcast:31 -> rows 2, 3
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v += dpp_move<0x111, 0xf>(0.f, v);
    v += dpp_move<0x112, 0xf>(0.f, v);
    v += dpp_move<0x114, 0xf>(0.f, v);
    v += dpp_move<0x118, 0xf>(0.f, v);
    v += dpp_move<0x142, 0xa>(0.f, v);
    v += dpp_move<0x143, 0xc>(0.f, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// Sixteen wave-wide sums at once: acc[r] = this lane's partial of row r; returns, in lane r (< 16), the wave total of
// row r.  Each stage halves the number of registers while doubling the lanes already summed: lane-half swap
// (v_permlane32_swap), 16-lane-row swap (v_permlane16_swap), row rotation by 8, bank shifts by 4, two quad steps -
// about 40 instructions and short dependency chains instead of sixteen 7-deep DPP chains.  (The permlane swaps go
// through inline asm: the clang builtins of this ROCm return the first result twice.)
// The compiler does not see through an asm, so it inserts none of the wait states these instructions need after a
// vector write of their operands / before a vector read of their results (observed: wrong values without them).
__device__ __forceinline__ void swap_halves32(float& a, float& b) { asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ void swap_rows16(float& a, float& b) { asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b)); }
template <int CTRL, int BANK>
__device__ __forceinline__ float dpp_bank_move(float old, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, 0xf, BANK, false));
}
__device__ __forceinline__ float wave_sum16(float (&acc)[16], int lane) {
    float s[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) { float x = acc[r], y = acc[r + 8]; swap_halves32(x, y); s[r] = x + y; }   // lanes < 32: row r, others row r + 8
    float t[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { float x = s[r], y = s[r + 4]; swap_rows16(x, y); t[r] = x + y; }      // 16-lane row q: row r + 4 q
    const bool b3 = (lane & 8) != 0, b2 = (lane & 4) != 0;
    float v[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const float keep = b3 ? t[r + 2] : t[r], give = b3 ? t[r] : t[r + 2];
        v[r] = keep + dpp_bank_move<0x128, 0xf>(0.f, give);            // row_ror:8
    }
    const float keep = b2 ? v[1] : v[0], give = b2 ? v[0] : v[1];
    float o = dpp_bank_move<0x104, 0x5>(0.f, give);                    // row_shl:4 into lanes 0-3, 8-11 of each row
    o = dpp_bank_move<0x114, 0xa>(o, give);                            // row_shr:4 into lanes 4-7, 12-15
    float w = keep + o;
    w += dpp_bank_move<0xb1, 0xf>(0.f, w);                             // quad_perm [1, 0, 3, 2]
    w += dpp_bank_move<0x4e, 0xf>(0.f, w);                             // quad_perm [2, 3, 0, 1]
    // lanes 4 q .. 4 q + 3 hold the total of row q: bring it to lane q
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(16 * lane, __builtin_bit_cast(int, w)));
}

typedef __attribute__((address_space(1))) unsigned long long gu64;
// cache policy of the polling loads: agent scope (served by the L2, never by a CU's L1).  "nt" measures the same and had
// been used until round 3; "sc0" alone hits stale L1 lines (partners time out).
#define SK_LD "sc1"

// ------------------------------------------------------------------------------------------------
// Scaling-form cluster kernel (N, M <= 512), the production path.
//
// The log-domain iteration of mdgat.py:283-284 is the classical Sinkhorn matrix scaling written for
// numerical range.  Here the range is handled once: with K_ij = exp2(s_ij + u0_i + v0_j) for absorbed
// potentials (u0_i = - max(row max, dustbin) at start, v0 = 0) the SAME iteration is
//      a_i = mu_i / (sum_j K_ij b_j),   b_j = nu_j / (sum_i K_ij a_i),      u = u0 + log2 a,  v = v0 + log2 b
// i.e. two FMAs per matrix element and iteration instead of two exp2 and eight adds / maxes, and no
// transcendental in the loop.  Every row of K has its largest entry equal to 1 and the dustbin row /
// column entries are positive, so no sum can vanish; entries that underflow are < 2^-126 of their
// row's largest and cannot matter.  When a scaling factor leaves [2^-40, 2^40] it is folded back into
// K and the absorbed potentials (b: decided on b alone, which is bit-identical in all workgroups of a
// pair; a: per row, purely local), so any dynamic range the log-domain form handles is handled here.
//
// G workgroups (8 waves each, one per CU) share one pair: workgroup j owns rows [128 j, 128 j + 128), wave w of it
// 16 of those rows, lane l the columns 8 l .. 8 l + 7: a lane keeps a 16 x 8 block of K (128 VGPRs) for all
// iterations.  Row sums: 8 in-lane FMAs per row + one transposed wave reduction for the 16 rows (wave_sum16).  Column
// sums: in-lane over the wave's 16 rows, the 8 waves merged through LDS, the G workgroups through L2 as 8-byte
// {epoch, value} granules (the data is the flag, two slot sets alternate by epoch parity; relaxed agent-scope atomics,
// or non-temporal accesses once the partners have agreed that they share an XCD; partners are placed on one XCD for
// speed only; spins are bounded: a timeout raises the launch's error word, and the one-workgroup-per-pair streaming kernel
// that follows every cluster launch - it leaves at once otherwise - then redoes the whole launch: the result is correct
// whatever else occupies the device, only late).  The launch is a plain one when every workgroup has a CU of its own
// (launch_scaling), cooperative otherwise.
struct SksArgs {
    const float* scores;
    const float* alpha_dev;
    float alpha_host;
    float* Z;
    unsigned long long* slots;   // per group: column slots [2][GC][GR][SLOT_STRIDE], then row slots [2][GR][GC][ROW_STRIDE]; zeroed per launch
    unsigned* error_word;        // bit 0: a workgroup gave up waiting for a partner (the whole launch is redone); bit 1: some pair is out of range
    unsigned* pair_flags;        // [B], zeroed per launch: this pair's scores are beyond the range of the scaling form (it alone is redone)
    unsigned* range_guard;       // optional, host-mapped: set when a score is not finite (an activation upstream left the f16 range)
    int B, N, M, iters, ngroups, GR, GC;
    int xcd_map;         // workgroup blockIdx = (slot * P + partner) * 8 + xcd: the partners of a pair share blockIdx % 8 (launch_scaling)
    // fused arg-max of the match extraction (mdgat.py:441-483): per row over this workgroup's columns, per column over
    // its rows (merged later); ext_mode < 0: off.  Z may be NULL when only the matches are wanted.
    int ext_mode;
    int* rbest_idx;      // [B][GC][N]
    float* rbest_val;    // [B][GC][N]
    int* cbest_idx;      // [B][GR][M]
    float* cbest_val;    // [B][GR][M]
};

constexpr int SKS_THREADS = 512;
constexpr int SKS_LDS_FLOATS = 520 + 8 * 512 + 8 + 8 + 8 * 512;
constexpr int ROW_STRIDE = 136;

// Granule traffic between the workgroups of a pair.  Agent scope (sc1) works wherever the partners run.  When all of
// them report the same XCC_ID (checked per pair with an agent-scope exchange first), they share one L2: plain 8-byte
// stores and agent-scope loads issued by hand (several in flight, one wait) carry the hand-off at lower latency.
__device__ __forceinline__ unsigned long long xload(gu64* p, bool same_xcd) {
    if (same_xcd) {
        unsigned long long v;
        asm volatile("global_load_dwordx2 %0, %1, off " SK_LD "\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
        return v;
    }
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void xstore(gu64* p, unsigned long long v, bool same_xcd) {
    // A PLAIN store: the CU's L1 writes through to the XCD's L2, where the partners' (L1-bypassing) loads find it, and it stays
    // there.  With `nt` - as until round 3 - the L2 streamed every granule on to HBM: 115 MB written per launch at B = 64
    // (PMC WRITE_SIZE) against 11 MB now, and the hand-off waited for it: 3.2 -> 2.85 us per iteration, 391 -> 355 us per launch.
    if (same_xcd) asm volatile("global_store_dwordx2 %0, %1, off" :: "v"(p), "v"(v) : "memory");
    else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Poll the granules `base[p * stride]`, p in [0, n) except `self`, until they carry `tag`; all outstanding partners are
// polled concurrently.  vals[p] receives the payloads.  Bounded: a timeout sets the error word.
// `extra` (optional): one more granule polled in the same round trips (the dustbin column's partial of a partner, by the
// lanes of the last wave that own it): extra_val receives its payload.
template <int NMAX>
__device__ __forceinline__ void poll_partners(gu64* base, size_t stride, int n, int self, unsigned tag, float (&vals)[NMAX],
                                              bool& failed, unsigned* error_word, bool same_xcd = false,
                                              gu64* extra = nullptr, float* extra_val = nullptr) {
    unsigned pending = ((1u << n) - 1u) & ~(1u << self);
    bool extra_pending = extra != nullptr;
    unsigned spins = 0;
    while (pending || extra_pending) {
        unsigned long long x[NMAX], xe = 0;
        if (NMAX <= 4 && same_xcd) {
            // all outstanding partners in ONE round trip: the loads are issued back to back and awaited together (a wait per
            // load cost 346 against 337 us per launch at B = 64 once the stores had become plain; with up to 16 partners
            // the sixteen granules in flight cost 86 more spilled registers: those kernels keep the serial poll)
#pragma unroll
            for (int p = 0; p < NMAX; ++p)
                if (pending & (1u << p)) asm volatile("global_load_dwordx2 %0, %1, off " SK_LD : "=v"(x[p]) : "v"(base + (size_t)p * stride) : "memory");
            if (extra_pending) asm volatile("global_load_dwordx2 %0, %1, off " SK_LD : "=v"(xe) : "v"(extra) : "memory");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int p = 0; p < NMAX; ++p)
                if (pending & (1u << p)) asm volatile("" : "+v"(x[p]));       // (uses stay behind the wait)
            asm volatile("" : "+v"(xe));
        } else if (same_xcd) {
            // more than four partners on one XCD (up to 16 row slabs, N <= 2048 with M <= 512): four granules in flight per round
            // trip, consumed before the next four are requested (all sixteen at once cost 86 spilled registers; one at a time - a
            // wait per load, as until round 4 - a round trip each: 8 x 2048 x 512 0.747 -> 0.592 ms per 100 iterations)
#pragma unroll
            for (int p = 0; p < NMAX; ++p) x[p] = 0;
#pragma unroll
            for (int p0 = 0; p0 < NMAX; p0 += 4) {
                if (!((pending >> p0) & 0xfu) && !(extra_pending && p0 == 0)) continue;
                unsigned long long y[4] = {0, 0, 0, 0};
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (pending & (1u << (p0 + u))) asm volatile("global_load_dwordx2 %0, %1, off " SK_LD : "=v"(y[u]) : "v"(base + (size_t)(p0 + u) * stride) : "memory");
                if (extra_pending && p0 == 0) asm volatile("global_load_dwordx2 %0, %1, off " SK_LD : "=v"(xe) : "v"(extra) : "memory");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    asm volatile("" : "+v"(y[u]));
                    if ((pending & (1u << (p0 + u))) && (unsigned)(y[u] >> 32) == tag) {
                        vals[p0 + u] = __builtin_bit_cast(float, (unsigned)y[u]);
                        pending &= ~(1u << (p0 + u));
                    }
                }
                asm volatile("" : "+v"(xe));
            }
        } else {
            // partners on different XCDs: agent-scope atomic loads, which the compiler pipelines (all outstanding ones in flight) -
            // as long as this loop holds nothing else: until round 4 it went through xload() with its run-time same_xcd branch per
            // load, which serialised the sixteen loads of the two-dimensional kernels (8 x 2048 x 2048 1.81 -> 1.55 ms per 100
            // iterations, 8 x 1024 x 1024 0.805 -> 0.687)
#pragma unroll
            for (int p = 0; p < NMAX; ++p)
                if (pending & (1u << p)) x[p] = __hip_atomic_load(base + (size_t)p * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (extra_pending) xe = __hip_atomic_load(extra, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int p = 0; p < NMAX; ++p)
            if ((pending & (1u << p)) && (unsigned)(x[p] >> 32) == tag) {
                vals[p] = __builtin_bit_cast(float, (unsigned)x[p]);
                pending &= ~(1u << p);
            }
        if (extra_pending && (unsigned)(xe >> 32) == tag) {
            *extra_val = __builtin_bit_cast(float, (unsigned)xe);
            extra_pending = false;
        }
        if (pending || extra_pending) {
            if (failed || ++spins > (1u << 22)) { failed = true; atomicOr(error_word, 1u); break; }
            __builtin_amdgcn_s_sleep(1);
        }
    }
}

// The pair's matrix is tiled GR x GC: workgroup (jr, jc) keeps rows [128 jr, 128 jr + 128) x columns [512 jc, 512 jc + 512)
// in registers: wave w 16 of those rows, lane l the 8 columns 8 l .. 8 l + 7 (RPW x 8 block, 128 VGPRs).  Per-row
// quantities (absorbed potential, dustbin-column entry, scaling a) live in lane r of the wave for row r; the scaling is
// broadcast for the column pass with v_readlane.  Per-column quantities of the lane's 8 columns live in registers; the
// thread that finalises column t keeps its own copies.  Row sums cross the GC column slabs, column sums the GR row slabs
// (TWO_D = more than one column slab: N, M up to 2048).
// GMAX = compile-time bound on the row slabs (4: N <= 512, 16: N <= 2048)
template <bool TWO_D, int GMAX>
__global__ __launch_bounds__(SKS_THREADS, 2) void sinkhorn_scaling_kernel(SksArgs a) {
    constexpr int RPW = 16;               // rows per wave
    __shared__ __attribute__((aligned(16))) float lds[SKS_LDS_FLOATS];
    float* bvec = lds;                    // [512] column scalings of the slab, [512] = dustbin column
    float* colp = lds + 520;              // [8 waves][512] per-wave column sums
    float* pdust = colp + 8 * 512;        // [8] per-wave sums of the dustbin column
    int* flags = reinterpret_cast<int*>(pdust + 8);   // [0]: a column scaling of the slab left the safe range
    int* colpi = flags + 8;               // [8 waves][512] row indices of the per-wave column maxima (fused extraction)

    const int N = a.N, M = a.M, GR = a.GR, GC = TWO_D ? a.GC : 1;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int P = GR * GC;
    int group, w;
    if (a.xcd_map) {                      // partners share blockIdx % 8 (observed: the XCD); the grid is padded to 8 groups per slot
        const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
        w = q % P;
        group = (q / P) * 8 + xcd;
        if (group >= a.ngroups) return;   // (padding: the whole workgroup leaves)
    } else {
        group = blockIdx.x / P;
        w = blockIdx.x % P;
    }
    const int jr = w / GC, jc = w % GC;
    const float alpha = (a.alpha_dev ? *a.alpha_dev : a.alpha_host) * MDGAT_LOG2E;
    const float norm = -logf((float)(N + M));
    const float mu = 1.0f / (float)(N + M);                    // exp(log_mu) of mdgat.py:302 (rows 0..N-1)
    const float muN = (float)M / (float)(N + M);               // dustbin row
    const float nu = mu;                                       // columns 0..M-1 (mdgat.py:303)
    const float nuM = (float)N / (float)(N + M);               // dustbin column
    const int row0 = (jr * 8 + wave) * RPW;   // first row of this wave
    const int col0 = lane * 8;                // first local column of this lane
    const int gcol0 = jc * 512 + col0;        // ... global
    const bool my_row_valid = lane < RPW && row0 + lane < N;   // lane r carries the per-row state of row r
    const size_t col_slots = (size_t)2 * GC * GR * SLOT_STRIDE, row_slots = (size_t)2 * GR * GC * ROW_STRIDE;
    gu64* cslots = (gu64*)(a.slots) + (size_t)group * (col_slots + row_slots);
    gu64* rslots = cslots + col_slots;
    unsigned cep = 0, rep_ = 0, xep = 0;  // column / row / XCC-id exchange counters (granule tags)
    bool failed = false;
    const float RANGE_HI = 1.099511627776e12f, RANGE_LO = 9.094947017729282e-13f;   // 2^40, 2^-40

    // sum (or max) of one per-row value (lanes < RPW, plus lane RPW of wave 0 for the dustbin row) over the GC column slabs
    auto row_exchange = [&](float v, bool take_max) -> float {
        if (!TWO_D) return v;
        ++rep_;
        const bool active = lane <= RPW;          // lane RPW: the dustbin row (every wave publishes / polls the same value)
        const int idx = lane < RPW ? wave * RPW + lane : 128;
        float out = v;
        if (active) {
            gu64* base = rslots + ((size_t)(rep_ & 1) * GR + jr) * GC * ROW_STRIDE + idx;
            __hip_atomic_store(base + (size_t)jc * ROW_STRIDE, ((unsigned long long)rep_ << 32) | __builtin_bit_cast(unsigned, v),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            float vals[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) vals[p] = take_max ? NEG_BIG : 0.f;
            poll_partners<4>(base, ROW_STRIDE, GC, jc, rep_, vals, failed, a.error_word);
            out = take_max ? NEG_BIG : 0.f;
#pragma unroll
            for (int p = 0; p < 4; ++p) {             // fixed order: bit-identical in every partner (GC <= 4)
                const float x = (p == jc) ? v : vals[p];
                out = take_max ? fmaxf(out, x) : out + x;
            }
        }
        return out;
    };

    for (int pair = group; pair < a.B; pair += a.ngroups) {
        const float* S = a.scores + (size_t)pair * N * M;
        // ---- this lane's RPW x 8 block of scores (base-2 log units); invalid entries -> exp2 gives 0 ----
        float K[RPW][8];
        const bool vec_ok = (M & 3) == 0 && gcol0 + 8 <= M;
        unsigned gmax = 0;                // largest |score| of this lane as an integer image: NaN / inf on top
        // (the path is chosen per LANE, outside the row loop: chosen per row, the three-way branch kept the loads of different rows
        // in different basic blocks - the ragged path then ran its 128 loads one round trip at a time)
        if (vec_ok) {
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const int i = row0 + r;
                const float* row = S + (size_t)min(i, N - 1) * M;
                const f32x4 x0 = *reinterpret_cast<const f32x4*>(row + gcol0);
                const f32x4 x1 = *reinterpret_cast<const f32x4*>(row + gcol0 + 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    gmax = max(gmax, max(__builtin_bit_cast(unsigned, x0[c]) & 0x7fffffffu, __builtin_bit_cast(unsigned, x1[c]) & 0x7fffffffu));
                    K[r][c] = i < N ? x0[c] * MDGAT_LOG2E : NEG_BIG;
                    K[r][4 + c] = i < N ? x1[c] * MDGAT_LOG2E : NEG_BIG;
                }
            }
        } else if (gcol0 >= M) {
            // a lane whose eight columns all lie beyond M loads nothing (M = 256: half of every wave - as clamped scalar
            // loads, 128 per lane, they cost the launch of one pair 10 us in a phase trace)
#pragma unroll
            for (int r = 0; r < RPW; ++r)
#pragma unroll
                for (int c = 0; c < 8; ++c) K[r][c] = NEG_BIG;
        } else {
            // ragged columns (M not a multiple of 4, or the lane that holds the last valid columns): every load first ...
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const float* row = S + (size_t)min(row0 + r, N - 1) * M;
#pragma unroll
                for (int c = 0; c < 8; ++c) K[r][c] = row[min(gcol0 + c, M - 1)];
            }
            // ... then the guard, the scale and the mask
#pragma unroll
            for (int r = 0; r < RPW; ++r)
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float x = K[r][c];
                    gmax = max(gmax, __builtin_bit_cast(unsigned, x) & 0x7fffffffu);
                    K[r][c] = (row0 + r < N && gcol0 + c < M) ? x * MDGAT_LOG2E : NEG_BIG;
                }
        }
        if (a.range_guard && gmax >= 0x7f800000u) __hip_atomic_store(a.range_guard, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        // ---- absorb the row maximum (all column slabs, dustbin column included): every row of K has largest entry <= 1 ----
        float u0r = 0.f, kbr = 0.f, ar = 0.f;     // lane r: absorbed potential, dustbin-column entry, scaling of row r
        {
            float mrow = NEG_BIG;
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                float m = K[r][0];
#pragma unroll
                for (int c = 1; c < 8; ++c) m = fmaxf(m, K[r][c]);
                m = wave_max_dpp(m);                   // wave-uniform
                mrow = (lane == r) ? m : mrow;
            }
            mrow = fmaxf(row_exchange(mrow, true), alpha);
            u0r = -mrow;
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const float m = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mrow), r));
#pragma unroll
                for (int c = 0; c < 8; ++c) K[r][c] = ex2(K[r][c] - m);
            }
        }
        if (my_row_valid) { kbr = ex2(alpha + u0r); ar = 1.f; } else { u0r = 0.f; }
        // Range of the scaling form: an entry more than ~100 octaves below its row's largest - a score 69 below the row
        // maximum, or a bin score that far from it - is on its way out of fp32 (2^-126, sooner after a fold), and a column
        // (or the dustbin column) made of such entries only has no sum left, where the log-domain reference still resolves
        // it.  No trained network is near that; when the inputs are (tools/fuzz_sinkhorn.py: scores spread over 100+ units),
        // the launch is handed to the log-domain streaming kernel: raise the error word.
        {
            float kmin = my_row_valid ? kbr : 1.f;
#pragma unroll
            for (int r = 0; r < RPW; ++r)
#pragma unroll
                for (int c = 0; c < 8; c += 2) {
                    const bool v0_ = row0 + r < N && gcol0 + c < M, v1_ = row0 + r < N && gcol0 + c + 1 < M;
                    kmin = fminf(kmin, fminf(v0_ ? K[r][c] : 1.f, v1_ ? K[r][c + 1] : 1.f));
                }
            if (kmin < 0x1p-100f) {
                atomicOr(a.error_word, 2u);
                __hip_atomic_store(a.pair_flags + pair, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        // absorbed dustbin row: u0_N = -alpha, so its entries are exp2(v0_j) = 1
        float u0N = -alpha, aN = 1.f;
        float v0[8], kr[8], b[8];         // per lane column: absorbed potential, dustbin-row entry, column scaling
#pragma unroll
        for (int c = 0; c < 8; ++c) { v0[c] = 0.f; kr[c] = (gcol0 + c < M) ? 1.f : 0.f; b[c] = (gcol0 + c < M) ? 1.f : 0.f; }
        float v0M = 0.f, kc = 1.f, bM = 1.f;
        // state of the columns this thread finalises: local column tid (global 512 jc + tid); thread 0 also the dustbin column
        const bool tcol_valid = jc * 512 + tid < M;
        float krt = 1.f, v0t = 0.f, bt = 1.f;
        __syncthreads();                  // previous pair's readers of the LDS vectors are done
        if (tid == 0) flags[0] = 0;
        // do all row-slab partners of this pair sit on one XCD?  (slot 513 of the parity-0 buffer, agent scope)
        bool same_xcd = false;
        if (!TWO_D && GR > 1) {
            ++xep;
            if (tid == 0) {
                const unsigned my_xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xf;     // HW_REG_XCC_ID[3:0]
                gu64* xb = cslots + (size_t)jc * GR * SLOT_STRIDE + 513;
                const unsigned xtag = 0x80000000u | xep;
                __hip_atomic_store(xb + (size_t)jr * SLOT_STRIDE, ((unsigned long long)xtag << 32) | my_xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                float ids[GMAX];
#pragma unroll
                for (int pp = 0; pp < GMAX; ++pp) ids[pp] = 0.f;
                poll_partners<GMAX>(xb, SLOT_STRIDE, GR, jr, xtag, ids, failed, a.error_word);
                bool same = !failed;
#pragma unroll
                for (int pp = 0; pp < GMAX; ++pp)
                    if (pp < GR && pp != jr && __builtin_bit_cast(unsigned, ids[pp]) != my_xcc) same = false;
                flags[1] = same ? 1 : 0;
            }
            __syncthreads();
            same_xcd = flags[1] != 0;
        }

        for (int it = 0; it < a.iters; ++it) {
            // ---- row update (mdgat.py:283): a_i = mu_i / sum_j K_ij b_j ----
            float psum = 0.f;
            {
                float racc[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float acc = K[r][0] * b[0];
#pragma unroll
                    for (int c = 1; c < 8; ++c) acc = fmaf(K[r][c], b[c], acc);
                    racc[r] = acc;
                }
                psum = wave_sum16(racc, lane);                 // lane r: row r (lanes >= 16 are not used)
                psum = lane < 16 ? psum : 0.f;
            }
            {
                float pd = kr[0] * b[0];
#pragma unroll
                for (int c = 1; c < 8; ++c) pd = fmaf(kr[c], b[c], pd);
                pd = wave_sum_dpp(pd);                         // dustbin row over this slab's columns
                if (TWO_D) {
                    psum = (lane == RPW) ? pd : psum;
                    psum = row_exchange(psum, false);          // rows of this wave and the dustbin row, over all column slabs
                    pd = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, psum), RPW));
                }
                aN = muN * __builtin_amdgcn_rcpf(fmaf(kc, bM, pd));
            }
            ar = my_row_valid ? mu * __builtin_amdgcn_rcpf(fmaf(kbr, bM, psum)) : 0.f;
            const float dsum = wave_sum_dpp(kbr * ar);
            // ---- column update, wave-local part (mdgat.py:284): sum_i K_ij a_i over this wave's rows ----
            float q[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) q[c] = 0.f;
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const float arr = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ar), r));
#pragma unroll
                for (int c = 0; c < 8; ++c) q[c] = fmaf(K[r][c], arr, q[c]);
            }
            {
                f32x4* qw = reinterpret_cast<f32x4*>(colp + wave * 512 + col0);
                qw[0] = f32x4{q[0], q[1], q[2], q[3]};
                qw[1] = f32x4{q[4], q[5], q[6], q[7]};
                if (lane == 0) pdust[wave] = dsum;
            }
            __syncthreads();
            // ---- merge the 8 waves, exchange with the row-slab partners, new column scalings ----
            ++cep;
            {
                gu64* base = cslots + ((size_t)(cep & 1) * GC + jc) * GR * SLOT_STRIDE;
                const unsigned long long tagbits = (unsigned long long)cep << 32;
                // (b0) wave 7 publishes the dustbin column's partial sum (slot 512) BEFORE the column exchange, so that its
                //      own poll of the partners' dustbin slots after (a) finds them already there
                float dloc = 0.f;
                if (wave == 7) {
                    dloc = pdust[0];
#pragma unroll
                    for (int ww = 1; ww < 8; ++ww) dloc += pdust[ww];
                    if (GR > 1 && lane == 0) xstore(base + (size_t)jr * SLOT_STRIDE + 512, tagbits | __builtin_bit_cast(unsigned, dloc), same_xcd);
                }
                // (a) every thread: its own column of the slab, all row-slab partners polled concurrently; lane p of the last
                //     wave polls row slab p's dustbin partial in the same round trips (a second poll after this one kept
                //     the whole workgroup waiting at the barrier for one more L2 round trip per iteration)
                bool have_dust = false;
                float dust_in = 0.f;
                if (tcol_valid) {
                    float loc = colp[tid];
#pragma unroll
                    for (int ww = 1; ww < 8; ++ww) loc += colp[ww * 512 + tid];
                    float vals[GMAX];
#pragma unroll
                    for (int pp = 0; pp < GMAX; ++pp) vals[pp] = 0.f;
                    if (GR > 1) {
                        xstore(base + (size_t)jr * SLOT_STRIDE + tid, tagbits | __builtin_bit_cast(unsigned, loc), same_xcd);
                        const bool my_dust = wave == 7 && lane < GR && lane != jr;
                        poll_partners<GMAX>(base + tid, SLOT_STRIDE, GR, jr, cep, vals, failed, a.error_word, same_xcd,
                                            my_dust ? base + (size_t)lane * SLOT_STRIDE + 512 : nullptr, &dust_in);
                        have_dust = my_dust && !failed;
                    }
                    float total = 0.f;
#pragma unroll
                    for (int pp = 0; pp < GMAX; ++pp) total += (pp == jr) ? loc : vals[pp];   // fixed order: bit-identical in every partner
                    bt = nu * __builtin_amdgcn_rcpf(fmaf(krt, aN, total));
                    bvec[tid] = bt;
                    if (!(bt > RANGE_LO && bt < RANGE_HI)) flags[0] = 1;
                }
                // (b) wave 7: the dustbin column (slot 512), lane p polls row slab p
                if (wave == 7) {
                    float mine = have_dust ? dust_in : dloc;
                    if (GR > 1) {
                        if (lane < GR && lane != jr && !have_dust) {
                            unsigned spins = 0;
                            while (true) {
                                const unsigned long long x = xload(base + (size_t)lane * SLOT_STRIDE + 512, same_xcd);
                                if ((unsigned)(x >> 32) == cep) { mine = __builtin_bit_cast(float, (unsigned)x); break; }
                                if (failed || ++spins > (1u << 22)) { failed = true; atomicOr(a.error_word, 1u); break; }
                                __builtin_amdgcn_s_sleep(1);
                            }
                        }
                    }
                    float total = 0.f;
#pragma unroll
                    for (int pp = 0; pp < GMAX; ++pp)
                        if (pp < GR) total += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine), pp));
                    if (lane == 0) bvec[512] = nuM * __builtin_amdgcn_rcpf(fmaf(kc, aN, total));
                }
            }
            __syncthreads();
            {
                const f32x4 x0 = *reinterpret_cast<const f32x4*>(bvec + col0);
                const f32x4 x1 = *reinterpret_cast<const f32x4*>(bvec + col0 + 4);
                b[0] = x0[0]; b[1] = x0[1]; b[2] = x0[2]; b[3] = x0[3]; b[4] = x1[0]; b[5] = x1[1]; b[6] = x1[2]; b[7] = x1[3];
#pragma unroll
                for (int c = 0; c < 8; ++c) if (gcol0 + c >= M) b[c] = 0.f;
                bM = bvec[512];
            }
            // ---- fold scalings that left [2^-40, 2^40] back into K and the absorbed potentials (rare) ----
            // (Measured: with the folds hoisted out of the iteration loop - an inner loop that only reads the block - the
            // 128 register copies per iteration disappear from the N <= 512 kernel, for -1 %; the two larger kernels spill
            // 75 / 195 registers instead of 59 / 49: N = 2048 +12 %.)
            if (flags[0] != 0) {                   // identical in all row-slab partners (same b for this column slab)
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    if (gcol0 + c < M) {
#pragma unroll
                        for (int r = 0; r < RPW; ++r) K[r][c] *= b[c];
                        v0[c] += lg2(b[c]);
                        kr[c] *= b[c];
                        b[c] = 1.f;
                    }
                }
                if (tcol_valid) { krt *= bt; v0t += lg2(bt); bt = 1.f; }
                __syncthreads();                   // everyone has read the flag and bvec
                if (tid == 0) flags[0] = 0;
            }
            if (!(bM > RANGE_LO && bM < RANGE_HI)) {      // uniform everywhere: bM is replicated bit-identically
                kbr *= bM;
                kc *= bM;
                v0M += lg2(bM);
                bM = 1.f;
            }
            if (!(aN > RANGE_LO && aN < RANGE_HI)) {      // uniform everywhere
#pragma unroll
                for (int c = 0; c < 8; ++c) kr[c] *= aN;
                krt *= aN;
                kc *= aN;
                u0N += lg2(aN);
                aN = 1.f;
            }
            {
                const bool fold = my_row_valid && !(ar > RANGE_LO && ar < RANGE_HI);   // identical in all column-slab partners
                const unsigned long long fm = __ballot(fold);
                if (fm) {
#pragma unroll
                    for (int r = 0; r < RPW; ++r) {
                        if (fm & (1ull << r)) {
                            const float arr = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ar), r));
#pragma unroll
                            for (int c = 0; c < 8; ++c) K[r][c] *= arr;
                        }
                    }
                    if (fold) { kbr *= ar; u0r += lg2(ar); ar = 1.f; }
                }
            }
        }

        // ---- Z = couplings + u + v - norm (mdgat.py:285, 307), natural-log units; fused arg-max ----
        float* Zp = a.Z ? a.Z + (size_t)pair * (N + 1) * (M + 1) : nullptr;
        const bool partner_lost = (__hip_atomic_load(a.error_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1u) != 0 ||
                                  __hip_atomic_load(a.pair_flags + pair, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;   // (or: this pair out of range)
        const float poison = partner_lost ? __builtin_nanf("") : 0.f;   // a partner never arrived: whatever this launch writes is
                                                                       // overwritten by the gated streaming kernel that follows
        const bool ran = a.iters > 0;    // with zero iterations u = v = 0 (the absorbed potentials are not potentials)
        const float VM = ran ? v0M + lg2(bM) + poison : 0.f;
        const float Ur = (ran && my_row_valid) ? u0r + lg2(ar) : 0.f;    // lane r: potential of row r
        float V[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) V[c] = (ran && gcol0 + c < M) ? v0[c] + lg2(b[c]) : 0.f;
        // Z (base-2) = s + U + V with s = lg2(K) - u0 - v0 from the register block: the scores are not read a second time
        // (67 MB per launch at B = 64).  K = exp2(s + u0 + v0) <= 1 carries s to ~1e-7; an entry that underflowed to 0 OR INTO THE
        // DENORMALS (v_log_f32 returns -inf for a denormal: found by tools/fuzz_forward.py on scores spanning 100 units)
        // (more than 126 octaves below its row maximum) is re-read.  Only where the block's registers have room for it:
        // in the kernels for more than 512 keypoints the longer live range of K costs 12 more spilled registers inside
        // the iteration loop (N = 2048: 7.5 -> 9.1 us per iteration), so they read the scores again instead.
        constexpr bool FROM_K = !TWO_D && GMAX == 4;
        const float dUr = Ur - u0r;                   // lane r
        float dV[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) dV[c] = V[c] - v0[c];
        const bool ext = a.ext_mode >= 0;
        const bool inner = a.ext_mode >= MDGAT_EXTRACT_THRESHOLD;   // arg-max over the inner N x M block only
        const bool last_c = jc == GC - 1, last_r = jr == GR - 1;
        float cbv[8];
        int cbi[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) { cbv[c] = -__builtin_inff(); cbi[c] = 0; }
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int i = row0 + r;
            if (i < N) {
                const float U = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, Ur), r));
                const float dU = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dUr), r));
                const float* row = S + (size_t)i * M;
                float z[8];
                if (FROM_K) {
                    bool under = false;
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        under |= (gcol0 + c < M) && !(K[r][c] >= 1.17549435e-38f);
                        z[c] = (gcol0 + c < M) ? (lg2(K[r][c]) + dU + dV[c]) * MDGAT_LN2 - norm : -__builtin_inff();
                    }
                    if (__any(under)) {
#pragma unroll
                        for (int c = 0; c < 8; ++c)
                            if ((gcol0 + c < M) && !(K[r][c] >= 1.17549435e-38f)) z[c] = (row[gcol0 + c] * MDGAT_LOG2E + U + V[c]) * MDGAT_LN2 - norm;
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < 8; ++c)
                        z[c] = (gcol0 + c < M) ? (row[min(gcol0 + c, M - 1)] * MDGAT_LOG2E + U + V[c]) * MDGAT_LN2 - norm : -__builtin_inff();
                }
                const float zM = (alpha + U + VM) * MDGAT_LN2 - norm;
                if (Zp) {
                    float* zr = Zp + (size_t)i * (M + 1);
#pragma unroll
                    for (int c = 0; c < 8; ++c)
                        if (gcol0 + c < M) zr[gcol0 + c] = z[c];
                    if (last_c && lane == 0) zr[M] = zM;
                }
                if (ext) {
                    // row: first maximal column of this slab (torch.max); the last slab adds the dustbin column unless `inner`
                    float bv = z[0];
                    int bi = gcol0;
#pragma unroll
                    for (int c = 1; c < 8; ++c)
                        if (z[c] > bv) { bv = z[c]; bi = gcol0 + c; }
                    {
                        // wave maximum on the vector ALU (DPP), then the LOWEST lane that holds it (lanes are in column order
                        // and bi is the lane's own first maximum: torch.max's first maximal index) - one ballot and two
                        // readlanes instead of twelve dependent ds_bpermute per row
                        const float mx = wave_max_dpp(bv);
                        const unsigned long long hit = __ballot(bv == mx);
                        const int first = hit ? __builtin_ctzll(hit) : 0;        // (no lane: NaN-poisoned row)
                        bi = __builtin_amdgcn_readlane(bi, first);
                        bv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bv), first));
                    }
                    if (!inner && last_c && zM > bv) { bv = zM; bi = M; }
                    if (lane == 0) {
                        a.rbest_idx[((size_t)pair * GC + jc) * N + i] = bi;
                        a.rbest_val[((size_t)pair * GC + jc) * N + i] = bv;
                    }
                    // columns: first maximal row among this wave's rows (ascending, strict compare)
#pragma unroll
                    for (int c = 0; c < 8; ++c)
                        if (z[c] > cbv[c]) { cbv[c] = z[c]; cbi[c] = i; }
                }
            }
        }
        const float UN = ran ? u0N + lg2(aN) : 0.f;
        const float zNt = (alpha + UN + (ran ? v0t + lg2(bt) + poison : 0.f)) * MDGAT_LN2 - norm;   // Z[N][512 jc + tid]
        if (last_r && Zp) {
            float* zl = Zp + (size_t)N * (M + 1);
            if (tcol_valid) zl[jc * 512 + tid] = zNt;
            if (last_c && tid == 0) zl[M] = (alpha + UN + VM) * MDGAT_LN2 - norm;
        }
        if (ext) {
            // merge the 8 waves (ascending rows), add the dustbin row (last row slab only, not `inner`)
            __syncthreads();             // colp's readers of the last iteration are done
            {
                f32x4* qw = reinterpret_cast<f32x4*>(colp + wave * 512 + col0);
                qw[0] = f32x4{cbv[0], cbv[1], cbv[2], cbv[3]};
                qw[1] = f32x4{cbv[4], cbv[5], cbv[6], cbv[7]};
                int* qi = colpi + wave * 512 + col0;
#pragma unroll
                for (int c = 0; c < 8; ++c) qi[c] = cbi[c];
            }
            __syncthreads();
            if (tcol_valid) {
                float bv = colp[tid];
                int bi = colpi[tid];
#pragma unroll
                for (int ww = 1; ww < 8; ++ww) {
                    const float v = colp[ww * 512 + tid];
                    if (v > bv) { bv = v; bi = colpi[ww * 512 + tid]; }
                }
                if (!inner && last_r && zNt > bv) { bv = zNt; bi = N; }
                a.cbest_val[((size_t)pair * GR + jr) * M + jc * 512 + tid] = bv;
                a.cbest_idx[((size_t)pair * GR + jr) * M + jc * 512 + tid] = bi;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// match extraction: one workgroup per pair
struct ExArgs {
    const float* Z;
    int N, M, mode;
    float thr;
    int64_t* m0; int64_t* m1;
    float* s0; float* s1;
    const unsigned* sk_error;   // optional: error word of the cluster kernel that produced the arg-maxes (bit 0: a lost partner) ...
    const float* Zfb;           // ... in which case the streaming fallback has written Z here: scan it instead
    const unsigned* pair_flags; // ... or, with sk_error, this pair alone was redone by the streaming kernel ([B])
    // optional, zeroed before the launch (B < 65536): one ticket word, (workgroups whose pair matched anything) << 16 |
    // workgroups done.  The last workgroup to finish applies the batch-wide rule of mdgat.py:465-467 (nothing matched
    // anywhere: all scores zero) - no separate fix-up launch
    unsigned* alldust_counters;
    int B;
    // Z == NULL: the arg-maxes were computed by the Sinkhorn kernel (row bests per column slab [B][GC][N], column bests
    // per row slab [B][GR][M])
    const int* rbest_idx; const float* rbest_val; const int* cbest_idx; const float* cbest_val; int GR, GC;
    // optional (host-mapped word): set to matched_token when a frame-0 keypoint of this pair is matched - what the host-side test
    // of mdgat.py:465 (`valid0.sum() == 0`) needs to know, without a reduction kernel and a copy (mdgat_matched_any)
    unsigned* matched; unsigned matched_token;
    // optional (device int32 [B], both or neither; with the arg-maxes of sinkhorn_f64.hip's ragged launch): pair b has cnt0[b] x cnt1[b]
    // keypoints in slots of N x M.  Its dustbins are the indices cnt1[b] / cnt0[b], the rule of mdgat.py:465-467 is applied to it alone (as
    // when it is the only pair of the call), and beyond its counts matches are -1 and scores 0.
    const int* cnt0; const int* cnt1;
};

__global__ __launch_bounds__(1024) void extract_kernel(ExArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Ns = a.N, Ms = a.M;                // the strides
    int N = Ns, M = Ms;
    if (a.cnt0) { N = a.cnt0[blockIdx.x]; M = a.cnt1[blockIdx.x]; }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the cluster kernel lost a partner workgroup (bounded spin ran out): its fused arg-maxes are garbage; the gated streaming
    // kernel has recomputed Z since
    const bool redone = a.sk_error && ((__hip_atomic_load(a.sk_error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1u) != 0 ||
                                       (a.pair_flags && __hip_atomic_load(a.pair_flags + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0));
    const float* Zsrc = redone ? a.Zfb : a.Z;
    const float* Z = Zsrc + (size_t)blockIdx.x * (Ns + 1) * (Ms + 1);
    int* idx0 = reinterpret_cast<int*>(smem);   // [N]
    int* idx1 = idx0 + Ns;                      // [M]
    float* val0 = reinterpret_cast<float*>(idx1 + Ms);  // [N]
    float* val1 = val0 + Ns;                    // [M]
    const bool inner = a.mode >= MDGAT_EXTRACT_THRESHOLD;   // arg-max over the inner N x M block only
    const int ncol = inner ? M : M + 1;   // columns scanned per row
    const int nrow = inner ? N : N + 1;   // rows scanned per column
    if (!Zsrc) {
        for (int i = tid; i < N; i += 1024) {
            const size_t base = (size_t)blockIdx.x * a.GC * Ns + i;
            float bv = a.rbest_val[base];
            int bi = a.rbest_idx[base];
            for (int g = 1; g < a.GC; ++g) {         // ascending column slabs, strict compare: first maximal column
                const float v = a.rbest_val[base + (size_t)g * Ns];
                if (v > bv) { bv = v; bi = a.rbest_idx[base + (size_t)g * Ns]; }
            }
            idx0[i] = bi; val0[i] = bv;
        }
        for (int j = tid; j < M; j += 1024) {
            const size_t base = (size_t)blockIdx.x * a.GR * Ms + j;
            float bv = a.cbest_val[base];
            int bi = a.cbest_idx[base];
            for (int g = 1; g < a.GR; ++g) {         // ascending row slabs, strict compare: first maximal row
                const float v = a.cbest_val[base + (size_t)g * Ms];
                if (v > bv) { bv = v; bi = a.cbest_idx[base + (size_t)g * Ms]; }
            }
            idx1[j] = bi; val1[j] = bv;
        }
    } else {
    // rows: first maximal index (torch.max semantics)
    for (int i = wave; i < N; i += 16) {
        const float* zr = Z + (size_t)i * (Ms + 1);
        float bv = -__builtin_inff();
        int bi = 0x7fffffff;
        for (int j = lane; j < ncol; j += 64) {
            const float z = zr[j];
            if (z > bv) { bv = z; bi = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { idx0[i] = bi; val0[i] = bv; }
    }
    // columns
    for (int j = tid; j < M; j += 1024) {
        float bv = -__builtin_inff();
        int bi = 0;
        for (int i = 0; i < nrow; ++i) {
            const float z = Z[(size_t)i * (Ms + 1) + j];
            if (z > bv) { bv = z; bi = i; }
        }
        idx1[j] = bi; val1[j] = bv;
    }
    }
    __syncthreads();

    int64_t* m0 = a.m0 + (size_t)blockIdx.x * Ns;
    int64_t* m1 = a.m1 + (size_t)blockIdx.x * Ms;
    float* s0 = a.s0 + (size_t)blockIdx.x * Ns;
    float* s1 = a.s1 + (size_t)blockIdx.x * Ms;

    int nmatch = 0;          // frame-0 keypoints of this thread with a match (matches0 >= 0)
    if (a.mode == MDGAT_EXTRACT_DUSTBIN || a.mode == MDGAT_EXTRACT_DUSTBIN_MUTUAL) {
        const bool mutual = a.mode == MDGAT_EXTRACT_DUSTBIN_MUTUAL;
        int nvalid = 0;
        for (int i = tid; i < N; i += 1024) {
            const int j = idx0[i];
            const bool valid = j < M;
            const bool keep = valid && (!mutual || idx1[j] == i);
            m0[i] = valid ? j : -1;
            s0[i] = keep ? expf(val0[i]) : 0.f;
            nvalid += valid;
        }
        for (int j = tid; j < M; j += 1024) {
            const int i = idx1[j];
            const bool valid = i < N;
            const bool keep = valid && (!mutual || idx0[i] == j);
            m1[j] = valid ? i : -1;
            s1[j] = keep ? expf(val1[j]) : 0.f;
        }
        nmatch = nvalid;
        if (a.alldust_counters) {
            // mdgat.py:465-467 over the whole batch: one ticket word = (workgroups that matched anything) << 16 | workgroups done;
            // the last workgroup to arrive decides
            const int any_valid = __syncthreads_or(nvalid > 0);         // (also: this workgroup's stores are issued)
            __shared__ int last;
            if (tid == 0) {
                __threadfence();                                         // scores of this pair before the ticket
                const unsigned old = atomicAdd(a.alldust_counters, (any_valid ? 0x10000u : 0u) + 1u);
                last = (old & 0xffffu) == (unsigned)a.B - 1 && (old >> 16) == 0 && !any_valid;
                __threadfence();
            }
            __syncthreads();
            if (last) {                                                  // (s0 is zero already: no row was valid)
                float* s1all = a.s1;
                for (size_t i = tid; i < (size_t)a.B * Ms; i += 1024) s1all[i] = 0.f;
            }
        } else if (a.cnt0) {
            // a ragged batch: mdgat.py:465-467 for this pair alone (s0 is zero already; every thread rewrites the scores it stored)
            if (!__syncthreads_or(nvalid > 0))
                for (int j = tid; j < M; j += 1024) s1[j] = 0.f;
        }
    } else if (a.mode == MDGAT_EXTRACT_THRESHOLD) {
        for (int i = tid; i < N; i += 1024) {
            const float e = expf(val0[i]);
            const bool valid = e > a.thr;
            m0[i] = valid ? idx0[i] : -1;
            s0[i] = valid ? e : 0.f;
            nmatch += valid;
        }
        for (int j = tid; j < M; j += 1024) {
            const float e = expf(val1[j]);
            const bool valid = e > a.thr;
            m1[j] = valid ? idx1[j] : -1;
            s1[j] = valid ? e : 0.f;
        }
    } else {   // MDGAT_EXTRACT_THRESHOLD_MUTUAL (mdgat.py:447-453)
        for (int i = tid; i < N; i += 1024) {
            const bool mutual0 = idx1[idx0[i]] == i;
            const float ms0 = mutual0 ? expf(val0[i]) : 0.f;
            const bool valid0 = mutual0 && ms0 > a.thr;
            m0[i] = valid0 ? idx0[i] : -1;
            s0[i] = ms0;
            nmatch += valid0;
        }
        for (int j = tid; j < M; j += 1024) {
            const int i = idx1[j];
            const bool mutual1 = idx0[i] == j;
            const bool mutual0_i = idx1[idx0[i]] == i;
            const float ms0_i = mutual0_i ? expf(val0[i]) : 0.f;
            const float ms1 = mutual1 ? ms0_i : 0.f;
            const bool valid1 = mutual1 && (mutual0_i && ms0_i > a.thr);
            m1[j] = valid1 ? i : -1;
            s1[j] = ms1;
        }
    }
    if (a.cnt0) {
        for (int i = N + tid; i < Ns; i += 1024) { m0[i] = -1; s0[i] = 0.f; }
        for (int j = M + tid; j < Ms; j += 1024) { m1[j] = -1; s1[j] = 0.f; }
    }
    if (a.matched) {
        const int any = __syncthreads_or(nmatch > 0);
        if (any && tid == 0) __hip_atomic_store(a.matched, a.matched_token, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// mdgat.py:465-467: when NO frame-0 keypoint of the whole batch is matched (valid0.sum() == 0), both score vectors are
// zeros.  matches0 >= 0 <=> valid0 in both dustbin modes, so the written matches are scanned (no counter shared between
// launches): every workgroup stops at the first chunk that holds a match - the first one on real data.
__global__ __launch_bounds__(256) void extract_alldust_fixup(const int64_t* m0, size_t n0, float* s1, size_t n1) {
    for (size_t base = 0; base < n0; base += 256) {
        const size_t i = base + threadIdx.x;
        if (__syncthreads_or(i < n0 && m0[i] >= 0)) return;
    }
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n1; i += (size_t)gridDim.x * 256) s1[i] = 0.f;
}

// ------------------------------------------------------------------------------------------------
// Split form of the log-domain kernel: a call with counts in slots of N x M <= 512 keypoints, a pair's rows cut into G = ceil(N / 128)
// slabs (by the slot alone).  Workgroup (b, g) owns rows [128 g, 128 g + 128) of pair b below the pair's own count; iteration `it` is
// ONE LAUNCH of B * G workgroups, so the stream's launch order is the only dependency between the workgroups of a pair: nobody waits,
// polls or adds atomically.  The arithmetic per element is sinkhorn_kernel's.  Between launches a pair's state lives in scratch, indexed
// by the parity of `it`: one (max, sum) column partial per slab, and the row potentials u with u_N behind the pair's last row.
// A launch reads only what the launch before it wrote: v = 0 at it = 0 comes from no memory.
//
// WIDE slots (SkCall::wide, a frame beyond 512 keypoints, up to MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS): the same kernels, instantiated for up to
// SK_SPLIT_WIDE_GMAX = 16 slabs and, where the slot has more than 512 columns (NC = 16, 32), with 8 waves instead of 16 - sinkhorn_kernel's own
// choice at those widths, for its reasons: a thread of 8 waves has 256 VGPRs for its four arrays of NC floats, and the workgroup's
// (N + 1) + (M + 1) + 2 * NW * M floats of LDS are 144 KB at 2048 x 2048 where 16 waves would want 272 KB.  A wave then takes 16 rows of a slab
// instead of 8; the order of every merge - waves ascending, then slabs ascending - is the narrow form's.  Slots within 512 x 512 keep the
// GMAX = 4 instantiations: their code and bits do not move.
constexpr int SK_SPLIT_ROWS = 128, SK_SPLIT_GMAX = 4, SK_SPLIT_NW = 16, SK_SPLIT_WIDE_GMAX = 16, SK_SPLIT_WIDE_NW = 8;
struct SkSplitArgs {
    const float* scores;      // [B][N][M]
    const float* alpha_dev;
    float alpha_host;
    float* Z;                 // [B][N+1][M+1]
    int N, M, iters;          // the slot (strides), the iterations of the call
    const int* cnt0;
    const int* cnt1;
    float2* part;             // [B][2][G][M]: (max, sum) of a slab's column log-sum-exps, by parity of the iteration that wrote them
    float* u;                 // [B][2][N+1]: the row potentials of an iteration, u_N at the pair's own count
    int G, it;                // slabs per pair; the iteration this launch runs (the finishing launch: iters)
};

// The pair's potentials as iteration `it` starts, formed by a whole workgroup in LDS (every workgroup of a pair forms the same bits):
// u[0 .. N] of iteration it - 1 from scratch, v[0 .. M - 1] as the merge, in ascending g, of the G column partials of iteration it - 1 with
// the dustbin-row term - sinkhorn_kernel's merge of its per-wave partials; a slab without rows wrote (NEG_BIG, 0), which adds an exact 0
// below the maximum - and v_M from that u.  it = 0: all zero.  Ends on a barrier.
template <int NW, int GMAX>
__device__ __forceinline__ void sk_split_potentials(const SkSplitArgs& a, int b, int it, int N, int M, float alpha, float lnu, float lnuM,
                                                    float* u, float* v) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (it == 0) {
        for (int i = tid; i <= N; i += NW * 64) u[i] = 0.f;
        for (int j = tid; j <= M; j += NW * 64) v[j] = 0.f;
        __syncthreads();
        return;
    }
    const int prev = (it - 1) & 1;
    const float* up = a.u + ((size_t)b * 2 + prev) * (a.N + 1);
    const float2* pp = a.part + ((size_t)b * 2 + prev) * a.G * a.M;
    for (int i = tid; i <= N; i += NW * 64) u[i] = up[i];
    const float bN = alpha + up[N];      // dustbin-row term of every column
    for (int j = tid; j < M; j += NW * 64) {
        float2 p[GMAX];
#pragma unroll
        for (int g = 0; g < GMAX; ++g) p[g] = g < a.G ? pp[(size_t)g * a.M + j] : float2{NEG_BIG, 0.f};
        float m = bN;
#pragma unroll
        for (int g = 0; g < GMAX; ++g) m = fmaxf(m, p[g].x);
        float e = ex2(bN - m);
#pragma unroll
        for (int g = 0; g < GMAX; ++g) e += p[g].y * ex2(p[g].x - m);
        v[j] = lnu - (m + lg2(e));
    }
    __syncthreads();
    if (wave == 0) {
        // dustbin column: v_M = log_nu_M - LSE_i(alpha + u_i), i = 0..N
        const float lse = alpha + wave_lse2(u, N, u[N], lane);
        if (lane == 0) v[M] = lnuM - lse;
    }
    __syncthreads();
}

template <int NC, int NW, int GMAX = SK_SPLIT_GMAX>
__global__ __launch_bounds__(NW * 64) void sinkhorn_split_kernel(SkSplitArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Ns = a.N, Ms = a.M;
    const int b = blockIdx.x / a.G, g = blockIdx.x % a.G;
    const int N = __builtin_amdgcn_readfirstlane(a.cnt0[b]), M = __builtin_amdgcn_readfirstlane(a.cnt1[b]);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cur = a.it & 1;
    float2* pout = a.part + (((size_t)b * 2 + cur) * a.G + g) * Ms;
    const int r0 = g * SK_SPLIT_ROWS, r1 = min(r0 + SK_SPLIT_ROWS, N);
    if (r0 >= N) {
        // a slab beyond the pair's rows: the neutral partial.  The whole workgroup leaves here, in front of every barrier
        for (int j = tid; j < M; j += NW * 64) pout[j] = float2{NEG_BIG, 0.f};
        return;
    }
    const float* S = a.scores + (size_t)b * Ns * Ms;
    float* ucur = a.u + ((size_t)b * 2 + cur) * (Ns + 1);

    float* u = smem;                 // [N+1]: the previous iteration's
    float* v = u + (N + 1);          // [M+1]
    float* pm = v + (M + 1);         // [NW][M]
    float* ps = pm + NW * M;         // [NW][M]

    const float alpha = (a.alpha_dev ? *a.alpha_dev : a.alpha_host) * MDGAT_LOG2E;
    const float norm = -logf((float)(N + M));                 // mdgat.py:301
    const float lmu = norm * MDGAT_LOG2E;                     // rows 0..N-1 (302)
    const float lmuN = (logf((float)M) + norm) * MDGAT_LOG2E; // dustbin row
    const float lnu = lmu;                                    // cols 0..M-1 (303)
    const float lnuM = (logf((float)N) + norm) * MDGAT_LOG2E; // dustbin column

    sk_split_potentials<NW, GMAX>(a, b, a.it, N, M, alpha, lnu, lnuM, u, v);

    // column potentials of this lane's columns
    float vr[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int j = c * 64 + lane;
        vr[c] = j < M ? v[j] : 0.f;
    }
    const float bM = alpha + v[M];   // dustbin-column term of every row
    if (g == 0 && wave == NW - 1) {
        // dustbin row: u_N = log_mu_N - LSE_j(alpha + v_j), j = 0..M (every workgroup of the pair would form the same bits: slab 0 stores them)
        const float lse = alpha + wave_lse2(v, M, v[M], lane);
        if (lane == 0) ucur[N] = lmuN - lse;
    }
    float cm[NC], cs[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { cm[c] = NEG_BIG; cs[c] = 0.f; }

    for (int i = r0 + wave; i < r1; i += NW) {
        const float* row = S + (size_t)i * Ms;
        float s[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int j = c * 64 + lane;
            s[c] = j < M ? row[j] * MDGAT_LOG2E : NEG_BIG;
        }
        float m = bM;
#pragma unroll
        for (int c = 0; c < NC; ++c) m = fmaxf(m, s[c] + vr[c]);
        m = wave_max(m);
        float e = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) e += ex2(s[c] + vr[c] - m);
        e = wave_sum(e) + ex2(bM - m);
        const float ui = lmu - (m + lg2(e));          // mdgat.py:283
        if (lane == 0) ucur[i] = ui;
#pragma unroll
        for (int c = 0; c < NC; ++c) {                // fold into the column LSEs (mdgat.py:284)
            const float w = s[c] + ui;
            const float nm = fmaxf(cm[c], w);
            cs[c] = cs[c] * ex2(cm[c] - nm) + ex2(w - nm);
            cm[c] = nm;
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int j = c * 64 + lane;
        if (j < M) { pm[wave * M + j] = cm[c]; ps[wave * M + j] = cs[c]; }
    }
    __syncthreads();
    // the slab's partial: the waves in ascending order (a wave without rows holds (NEG_BIG, 0); wave 0 always has a row)
    for (int j = tid; j < M; j += NW * 64) {
        float m = pm[j];
#pragma unroll
        for (int w = 1; w < NW; ++w) m = fmaxf(m, pm[w * M + j]);
        float e = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) e += ps[w * M + j] * ex2(pm[w * M + j] - m);
        pout[j] = float2{m, e};
    }
}

// The finishing launch: the last u (scratch) and v (formed as above), then Z = couplings + u + v - norm (mdgat.py:285, 307) in natural-log
// units over the pair's own block, the dustbins at its own counts, 0 over the rest of the slot.  Workgroup (b, g) writes the rows
// [128 g, 128 g + 128) of the slot's N + 1, the last one to the slot's end.
template <int NW, int GMAX = SK_SPLIT_GMAX>
__global__ __launch_bounds__(NW * 64) void sinkhorn_split_finish_kernel(SkSplitArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Ns = a.N, Ms = a.M;
    const int b = blockIdx.x / a.G, g = blockIdx.x % a.G;
    const int N = __builtin_amdgcn_readfirstlane(a.cnt0[b]), M = __builtin_amdgcn_readfirstlane(a.cnt1[b]);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float* S = a.scores + (size_t)b * Ns * Ms;
    float* Z = a.Z + (size_t)b * (Ns + 1) * (Ms + 1);
    float* u = smem;                 // [N+1]
    float* v = u + (N + 1);          // [M+1]
    const float alpha = (a.alpha_dev ? *a.alpha_dev : a.alpha_host) * MDGAT_LOG2E;
    const float norm = -logf((float)(N + M));
    const float lnu = norm * MDGAT_LOG2E;
    const float lnuM = (logf((float)N) + norm) * MDGAT_LOG2E;
    sk_split_potentials<NW, GMAX>(a, b, a.iters, N, M, alpha, lnu, lnuM, u, v);
    const float uN = u[N], vM = v[M];
    const int r0 = g * SK_SPLIT_ROWS, r1 = g == a.G - 1 ? Ns + 1 : r0 + SK_SPLIT_ROWS;
    for (int i = r0 + wave; i < r1; i += NW) {
        float* zr = Z + (size_t)i * (Ms + 1);
        if (i < N) {
            const float ui = u[i];
            const float* row = S + (size_t)i * Ms;
            for (int j = lane; j < M; j += 64) zr[j] = (row[j] * MDGAT_LOG2E + ui + v[j]) * MDGAT_LN2 - norm;
            if (lane == 0) zr[M] = (alpha + ui + vM) * MDGAT_LN2 - norm;
            for (int j = M + 1 + lane; j <= Ms; j += 64) zr[j] = 0.f;
        } else if (i == N) {
            for (int j = lane; j <= M; j += 64) zr[j] = (alpha + uN + v[j]) * MDGAT_LN2 - norm;
            for (int j = M + 1 + lane; j <= Ms; j += 64) zr[j] = 0.f;
        } else {
            for (int j = lane; j <= Ms; j += 64) zr[j] = 0.f;
        }
    }
}

template <int NC, int NW, bool RAGGED = false>
int launch_sk(const SkArgs& a, int B, hipStream_t s) {
    // (the 8-wave RAGGED instantiations: a pair of at most 512 columns keeps the partials of 16 virtual waves, [16][512] at the most)
    const size_t partials = RAGGED && NW == 8 && a.M < 1024 ? (size_t)16 * 512 : (size_t)NW * a.M;
    const size_t lds = ((size_t)(a.N + 1) + (a.M + 1) + 2 * partials) * sizeof(float);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sinkhorn_kernel<NC, NW, RAGGED>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return mdgat_check_hip(e, "sinkhorn LDS attribute");
    hipLaunchKernelGGL((sinkhorn_kernel<NC, NW, RAGGED>), dim3(B), dim3(NW * 64), lds, s, a);
    return mdgat_check_hip(hipGetLastError(), "sinkhorn launch");
}

}  // namespace

// tiling of a pair: GR row slabs of 128 rows (16 rows per wave) x GC column slabs of 512 columns, one workgroup each
static void sk_tiling(int N, int M, int& GR, int& GC) { GR = (N + 127) / 128; GC = (M + 511) / 512; }
static int sk_max_groups(int P) { return 256 / P > 64 ? 64 : (256 / P < 1 ? 1 : 256 / P); }      // pairs of P workgroups in flight on a 256-CU part (upper bound used for sizing)

// ---- the cluster kernel's workspace, stated once: byte offsets from its 256-byte aligned base ----
//   header  256 bytes: word 0 the launch's error word, words 2 and 3 the all-dustbin ticket of the extraction
//   slots   the exchange slots of a pair in flight (SksArgs::slots), for sk_max_groups pairs; rounded up to 256 together with the header
//   flags   the per-pair range flags: B words, rounded up to 256
//   bests   the fused arg-maxes: row bests [B][GC][N] (int, then float), column bests [B][GR][M] (int, then float)
// Header, slots and flags are zero when a launch starts: a partner that reads a stale slot or flag spins to its bound.
constexpr int SK_CLUSTER_MAX = 2048, SK_WORD_ERROR = 0, SK_WORD_TICKET = 2;    // keypoints per frame the cluster kernel takes (its limit is stated here only); header words
struct SkLayout {
    int GR, GC;
    size_t per_group, flags_bytes;                                             // bytes of one pair's slots, of the flags
    size_t header, slots, flags, rbest_idx, rbest_val, cbest_idx, cbest_val;   // offsets
    size_t clear_bytes, total;                                                 // header + slots + flags; all of it (0: the shape is beyond the cluster kernel)
    template <typename T> T* at(void* ws, size_t offset) const { return reinterpret_cast<T*>(static_cast<char*>(ws) + offset); }
    bool usable(const void* ws, size_t ws_bytes) const { return total && ws && ws_bytes >= total && (reinterpret_cast<uintptr_t>(ws) & 255) == 0; }
};
static SkLayout sk_layout(int B, int N, int M) {
    SkLayout l{};
    if (N <= 0 || M <= 0 || N > SK_CLUSTER_MAX || M > SK_CLUSTER_MAX) return l;
    sk_tiling(N, M, l.GR, l.GC);
    l.per_group = ((size_t)2 * l.GC * l.GR * SLOT_STRIDE + (size_t)2 * l.GR * l.GC * ROW_STRIDE) * sizeof(unsigned long long);
    l.flags_bytes = ((size_t)B * sizeof(unsigned) + 255) & ~(size_t)255;
    l.slots = l.header + 256;
    l.flags = (l.slots + l.per_group * sk_max_groups(l.GR * l.GC) + 255) & ~(size_t)255;
    l.rbest_idx = l.clear_bytes = l.flags + l.flags_bytes;
    l.rbest_val = l.rbest_idx + (size_t)B * l.GC * N * sizeof(int);
    l.cbest_idx = l.rbest_val + (size_t)B * l.GC * N * sizeof(float);
    l.cbest_val = l.cbest_idx + (size_t)B * l.GR * M * sizeof(int);
    l.total = l.cbest_val + (size_t)B * l.GR * M * sizeof(float);
    return l;
}
size_t sinkhorn_cluster_workspace_bytes(int B, int N, int M) { return sk_layout(B, N, M).total; }

// ---- the split form's scratch, stated once: byte offsets from its 256-byte aligned base; nothing in it is read before the call wrote it ----
//   part    SkSplitArgs::part: per pair 2 * G * M (max, sum) granules
//   u       SkSplitArgs::u: per pair 2 * (N + 1) floats
struct SkSplitLayout {
    int G;                       // slabs of 128 rows in a slot (0: the slot is beyond the ragged kernels)
    size_t part, u, total;       // total 0: the split form does not apply (G < 2)
    bool usable(const void* ws, size_t ws_bytes) const { return total && ws && ws_bytes >= total && (reinterpret_cast<uintptr_t>(ws) & 255) == 0; }
};
static int sk_ragged_limit(bool wide) { return wide ? MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS : MDGAT_RAGGED_FP32_MAX_KEYPOINTS; }
static bool sk_wide_slot(int N, int M) { return N > MDGAT_RAGGED_FP32_MAX_KEYPOINTS || M > MDGAT_RAGGED_FP32_MAX_KEYPOINTS; }
static SkSplitLayout sk_split_layout(int B, int N, int M, bool wide) {
    SkSplitLayout l{};
    if (B <= 0 || N <= 0 || M <= 0 || N > sk_ragged_limit(wide) || M > sk_ragged_limit(wide)) return l;
    l.G = (N + SK_SPLIT_ROWS - 1) / SK_SPLIT_ROWS;
    if (l.G < 2) return l;
    l.u = ((size_t)B * 2 * l.G * M * sizeof(float2) + 255) & ~(size_t)255;
    l.total = l.u + (((size_t)B * 2 * (N + 1) * sizeof(float) + 255) & ~(size_t)255);
    return l;
}
size_t sinkhorn_split_workspace_bytes(int B, int N, int M, bool wide) { return sk_split_layout(B, N, M, wide).total; }
size_t sinkhorn_slots_clear_bytes(int B, int N, int M) { return sk_layout(B, N, M).clear_bytes; }
bool sinkhorn_workspace_usable(int B, int N, int M, const void* ws, size_t ws_bytes) { return sk_layout(B, N, M).usable(ws, ws_bytes); }

// ---- the launchers' choices as a pure function (mdgat_sinkhorn_plan; no HIP call), and the launches counted by it ----
static std::atomic<unsigned long long> sinkhorn_launch_count[SK_COUNTERS];
static void sinkhorn_count_launch(int index) { sinkhorn_launch_count[index].fetch_add(1, std::memory_order_relaxed); }
void sinkhorn_launch_counts(uint64_t counts[MDGAT_SINKHORN_COUNTERS]) {
    for (int i = 0; i < SK_COUNTERS; ++i) counts[i] = sinkhorn_launch_count[i].load(std::memory_order_relaxed);
}
// ... and the launches that only a wide ragged slot reaches, attention.hip's among them (mdgat_ragged_wide_launches)
static std::atomic<unsigned long long> ragged_wide_launch_count[RAGGED_WIDE_COUNTERS];
void ragged_wide_count_launch(int index) { ragged_wide_launch_count[index].fetch_add(1, std::memory_order_relaxed); }
void ragged_wide_launch_counts(uint64_t counts[MDGAT_RAGGED_WIDE_COUNTERS]) {
    for (int i = 0; i < RAGGED_WIDE_COUNTERS; ++i) counts[i] = ragged_wide_launch_count[i].load(std::memory_order_relaxed);
}

SkPlan sinkhorn_plan(int B, int N, int M, int num_cu, bool workspace, bool fallback_buffer, bool ragged, bool split, bool wide) {
    SkPlan p{SK_PATH_NONE, -1, -1, 0, 0, 0, 0, 0, 0, MDGAT_OK, 0};
    if (B <= 0 || N <= 0 || M <= 0) return p;
    // the one-workgroup-per-pair streaming kernel: any shape up to M = 2048, no workspace
    const int nc = M <= 64 ? 0 : M <= 128 ? 1 : M <= 256 ? 2 : M <= 512 ? 3 : (M <= 1024 && N <= 4096) ? 4 : (M <= 2048 && N <= 4096) ? 5 : -1;
    if (ragged) {
        // the RAGGED instantiation for the slot, picked from the padded sizes alone (launch_sinkhorn: a call with counts)
        // (wide: the caller opted in to slots of up to MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS; more than 512 columns select the NC = 16 and 32 twins)
        if (N > sk_ragged_limit(wide) || M > sk_ragged_limit(wide)) { p.rc = MDGAT_ERR_UNSUPPORTED; return p; }
        p.path = SK_PATH_STREAMING;
        p.stream = nc <= 3 ? SK_RAGGED_1 + nc : SK_RAGGED_16 + (nc - 4);
        p.grid = B;
        // the split form where the caller opted in and the slot has more than one slab of rows: iters launches of B * G workgroups and a
        // finishing one, in the slot's NC; a slot of one slab keeps the one-workgroup kernel
        if (const int G = sk_split_layout(B, N, M, wide).G; split && G >= 2) { p.split = G; p.grid = B * G; }
        return p;
    }
    if (!workspace || N > SK_CLUSTER_MAX || M > SK_CLUSTER_MAX) {
        if (nc < 0) { p.rc = MDGAT_ERR_UNSUPPORTED; return p; }
        p.path = SK_PATH_STREAMING;
        p.stream = SK_STREAM_1 + nc;
        p.grid = B;
        return p;
    }
    sk_tiling(N, M, p.GR, p.GC);
    const int P = p.GR * p.GC;                     // workgroups per pair, one per CU
    int ngroups = num_cu / P;
    if (ngroups > sk_max_groups(P)) ngroups = sk_max_groups(P);
    if (ngroups > B) ngroups = B;
    p.ngroups = ngroups;
    if (ngroups < 1) { p.rc = MDGAT_ERR_UNSUPPORTED; return p; }
    // Placement: the workgroups of a pair exchange through L2 every iteration, which is fast and steady only inside one XCD
    // (workgroup i runs on XCD i % 8): group g takes the workgroups with blockIdx % 8 == g % 8, and the grid is padded to a
    // multiple of 8 groups - the surplus workgroups leave at once.  (Before: only batches that are multiples of 8 were placed,
    // others ran their partners on four different XCDs - 1.0 ms against an erratic 1.0 ... 3.5 ms per forward at B = 2 ... 4 -
    // and a batch of 12 ran as 8 + 4.)  A pair's workgroups must fit the 32 CUs of an XCD next to the other groups placed there.
    const int ng8 = (ngroups + 7) & ~7;
    p.xcd_map = P * (ng8 / 8) <= num_cu / 8;
    p.grid = p.xcd_map ? ng8 * P : ngroups * P;
    p.path = SK_PATH_CLUSTER;
    p.scaling = p.GC > 1 ? SK_SCALING_2D : p.GR > 4 ? SK_SCALING_16 : SK_SCALING_4;
    // The workgroups of a pair wait for each other, so all of them must become resident.  A workgroup takes a whole CU
    // (512 threads x 256 registers), and ngroups * P <= num_cu by construction: every workgroup gets a CU as soon as the
    // stragglers of earlier launches leave.  A plain launch therefore suffices when this launch has the device to itself, and
    // it starts 20-30 us sooner than hipLaunchCooperativeKernel (measured at B = 64: 430 -> 397 us for launch + 100
    // iterations).  It is NOT assumed: workgroups are dispatched in order (per XCD), so of every concurrent cluster launch at
    // most one pair per XCD is incomplete and the complete ones finish and make room - but enough concurrent launches (other
    // streams, other processes) could leave every CU with a workgroup whose partners cannot be dispatched.  The spins are
    // therefore bounded, a workgroup that gives up raises the launch's error word, and the streaming kernel launched right
    // behind (gated on that word: it leaves at once otherwise, ~3 us) redoes the launch one workgroup per pair - slow, never
    // wrong.  Without a fallback buffer (no Z and none lent) the launch is cooperative: the runtime then checks co-residency.
    const bool can_fall_back = fallback_buffer && nc >= 0;
    p.cooperative = !can_fall_back || ngroups * P > num_cu;
    if (can_fall_back) p.stream = SK_STREAM_1 + nc;
    return p;
}

// (the kernels' argument structs are filled by name behind their leading fields, the call and its Z)  An extraction request for B pairs in slots of
// N x M; its source - a Z to scan, or arg-maxes (GR = GC = 1 unless said otherwise) - is the caller's to add
static ExArgs ex_args(const SkExtract& ex, int B, int N, int M) {
    ExArgs a{};
    a.N = N; a.M = M; a.B = B; a.mode = ex.mode; a.thr = ex.thr; a.m0 = ex.m0; a.m1 = ex.m1; a.s0 = ex.s0; a.s1 = ex.s1;
    a.GR = a.GC = 1; a.matched = ex.matched; a.matched_token = ex.matched_token;
    return a;
}

int extract_check_mode(const char* who, int mode) {
    if (mode < 0 || mode > 3) { mdgat_set_error("%s: bad mode %d", who, mode); return MDGAT_ERR_BAD_ARG; }
    return MDGAT_OK;
}

int launch_alldust_fixup(int B, int N, int M, int mode, const int64_t* m0, float* s1, hipStream_t s) {
    if (mode != MDGAT_EXTRACT_DUSTBIN && mode != MDGAT_EXTRACT_DUSTBIN_MUTUAL) return MDGAT_OK;
    const size_t n = (size_t)B * M;
    hipLaunchKernelGGL(extract_alldust_fixup, dim3((unsigned)((n + 255) / 256 < 16 ? (n + 255) / 256 : 16)), dim3(256), 0, s,
                       m0, (size_t)B * N, s1, n);
    return mdgat_check_hip(hipGetLastError(), "extract fixup launch");
}

static int launch_extract_impl(const ExArgs& a, const SkExtract& ex, hipStream_t s) {
    if (int rc = extract_check_mode("extract", a.mode)) return rc;
    const size_t lds = (size_t)(2 * (a.N + a.M) + 4) * sizeof(float);
    hipLaunchKernelGGL(extract_kernel, dim3(a.B), dim3(1024), lds, s, a);
    if (int rc = mdgat_check_hip(hipGetLastError(), "extract launch")) return rc;
    sinkhorn_count_launch(SK_EXTRACT);
    if (ex.defer_alldust || a.alldust_counters || a.cnt0) return MDGAT_OK;      // (counters, or a ragged batch: the kernel applied the rule itself)
    return launch_alldust_fixup(a.B, a.N, a.M, a.mode, a.m0, a.s1, s);
}

int launch_extract(int B, int N, int M, const float* Z, const SkExtract& ex, hipStream_t s, const int* cnt0, const int* cnt1) {
    if (B <= 0) return MDGAT_OK;
    ExArgs a = ex_args(ex, B, N, M);
    a.Z = Z; a.cnt0 = cnt0; a.cnt1 = cnt1;
    return launch_extract_impl(a, ex, s);
}

// the extraction from arg-maxes another kernel has decided (sinkhorn_f64.hip: on the fp64 Z): rbest [B][N], cbest [B][M]
int launch_extract_from_bests(int B, int N, int M, const SkExtract* ex, const int* rbest_idx, const float* rbest_val, const int* cbest_idx,
                              const float* cbest_val, hipStream_t s, const int* cnt0, const int* cnt1) {
    if (B <= 0) return MDGAT_OK;
    if ((cnt0 != nullptr) != (cnt1 != nullptr)) { mdgat_set_error("extract: per-pair counts for one frame only"); return MDGAT_ERR_BAD_ARG; }
    ExArgs a = ex_args(*ex, B, N, M);
    a.rbest_idx = rbest_idx; a.rbest_val = rbest_val; a.cbest_idx = cbest_idx; a.cbest_val = cbest_val; a.cnt0 = cnt0; a.cnt1 = cnt1;
    return launch_extract_impl(a, *ex, s);
}

// the streaming kernel in the plan's instantiation; gated: behind a cluster launch (a.only_if), counted apart
static int launch_streaming(const SkArgs& a, int B, int form, bool gated, hipStream_t s) {
    static int (*const launch[])(const SkArgs&, int, hipStream_t) = {      // SK_STREAM_1 .. SK_STREAM_32, SK_RAGGED_1 .. SK_RAGGED_8
        launch_sk<1, 16>, launch_sk<2, 16>, launch_sk<4, 16>, launch_sk<8, 16>, launch_sk<16, 8>, launch_sk<32, 8>,
        launch_sk<1, 16, true>, launch_sk<2, 16, true>, launch_sk<4, 16, true>, launch_sk<8, 16, true>};
    if (form == SK_RAGGED_16 || form == SK_RAGGED_32) {      // a wide ragged slot of more than 512 columns: counted apart (ragged_wide_launch_counts)
        const int rc = form == SK_RAGGED_16 ? launch_sk<16, 8, true>(a, B, s) : launch_sk<32, 8, true>(a, B, s);
        if (!rc) ragged_wide_count_launch(form == SK_RAGGED_16 ? RAGGED_WIDE_SK_16 : RAGGED_WIDE_SK_32);
        return rc;
    }
    if (form < SK_STREAM_1 || form > SK_RAGGED_8) { mdgat_set_error("sinkhorn: M=%d > 2048 unsupported", a.M); return MDGAT_ERR_UNSUPPORTED; }
    const int rc = launch[form - SK_STREAM_1](a, B, s);
    if (!rc) sinkhorn_count_launch(gated ? SK_GATED : form);
    return rc;
}

// the cluster kernel, the gated streaming kernel behind it where the plan has one, then the extraction from the cluster kernel's arg-maxes
static int launch_scaling(const SkCall& c, const SkPlan& pl, const SkLayout& l) {
    hipStream_t s = c.stream;
    if (pl.rc) { mdgat_set_error("sinkhorn: %d workgroups per pair do not fit the device", pl.GR * pl.GC); return pl.rc; }
    if (!c.slots_cleared) {    // (the forward has the score kernel clear l.clear_bytes; here: the slots of the pairs in flight, and the flags)
        if (int rc = mdgat_check_hip(hipMemsetAsync(c.ws, 0, l.slots + l.per_group * pl.ngroups, s), "memset(sinkhorn slots)")) return rc;
        if (int rc = mdgat_check_hip(hipMemsetAsync(l.at<char>(c.ws, l.flags), 0, l.flags_bytes, s), "memset(sinkhorn pair flags)")) return rc;
    }
    unsigned* const header = l.at<unsigned>(c.ws, l.header);
    // test hook (tests/test_gpu_ops.py): pretend a partner was lost - the launch's error word starts out set, so the gated
    // streaming kernel and the extraction from its Z run for real
    if (const char* f = getenv("MDGAT_SK_FORCE_FALLBACK"); f && *f == '1')
        if (int rc = mdgat_check_hip(hipMemsetAsync(header + SK_WORD_ERROR, 1, sizeof(unsigned), s), "memset(sinkhorn error word)")) return rc;
    SksArgs a{c.scores, c.alpha_dev, c.alpha_host, c.Z};
    a.slots = l.at<unsigned long long>(c.ws, l.slots); a.error_word = header + SK_WORD_ERROR; a.pair_flags = l.at<unsigned>(c.ws, l.flags);
    a.range_guard = c.status ? c.status + MDGAT_STATUS_RANGE : nullptr;
    a.B = c.B; a.N = c.N; a.M = c.M; a.iters = c.iters; a.ngroups = pl.ngroups; a.GR = pl.GR; a.GC = pl.GC; a.xcd_map = pl.xcd_map;
    a.ext_mode = c.ex ? c.ex->mode : -1;
    if (c.ex) {
        a.rbest_idx = l.at<int>(c.ws, l.rbest_idx); a.rbest_val = l.at<float>(c.ws, l.rbest_val);
        a.cbest_idx = l.at<int>(c.ws, l.cbest_idx); a.cbest_val = l.at<float>(c.ws, l.cbest_val);
    }
    void* args[] = {&a};
    const void* kern = pl.scaling == SK_SCALING_2D ? reinterpret_cast<const void*>(sinkhorn_scaling_kernel<true, 16>)
                     : pl.scaling == SK_SCALING_16 ? reinterpret_cast<const void*>(sinkhorn_scaling_kernel<false, 16>)
                                                  : reinterpret_cast<const void*>(sinkhorn_scaling_kernel<false, 4>);
    // plain or cooperative, and whether the gated streaming kernel follows: sinkhorn_plan
    float* zfb = c.Z ? c.Z : c.Zfb;
    const bool can_fall_back = pl.stream >= 0;
    const hipError_t e = pl.cooperative ? hipLaunchCooperativeKernel(kern, dim3(pl.grid), dim3(SKS_THREADS), args, 0, s)
                                        : hipLaunchKernel(kern, dim3(pl.grid), dim3(SKS_THREADS), args, 0, s);
    if (int rc = mdgat_check_hip(e, "sinkhorn scaling launch")) return rc;
    sinkhorn_count_launch(pl.scaling);
    if (can_fall_back) {
        SkArgs f{c.scores, c.alpha_dev, c.alpha_host, zfb, c.N, c.M, c.iters};
        f.only_if = a.error_word; f.status_fallback = c.status ? c.status + MDGAT_STATUS_SK_FALLBACK : nullptr; f.pair_flags = a.pair_flags;
        if (int rc = launch_streaming(f, c.B, pl.stream, true, s)) return rc;
    }
    if (!c.ex) return MDGAT_OK;
    ExArgs x = ex_args(*c.ex, c.B, c.N, c.M);
    x.sk_error = can_fall_back ? a.error_word : nullptr; x.Zfb = zfb; x.pair_flags = a.pair_flags;
    x.alldust_counters = (c.ex->defer_alldust || c.B >= 65536) ? nullptr : header + SK_WORD_TICKET;      // (cleared with the slots)
    x.rbest_idx = a.rbest_idx; x.rbest_val = a.rbest_val; x.cbest_idx = a.cbest_idx; x.cbest_val = a.cbest_val; x.GR = pl.GR; x.GC = pl.GC;
    return launch_extract_impl(x, *c.ex, s);
}

// the split form (SkPlan::split slabs per pair): one launch per iteration and the finishing one into Z, then extract_kernel on that Z
template <int NC, int NW = SK_SPLIT_NW, int GMAX = SK_SPLIT_GMAX>
static hipError_t launch_sk_split(const SkSplitArgs& a, int B, hipStream_t s, bool prepare) {
    const size_t lds = ((size_t)(a.N + 1) + (a.M + 1) + 2 * (size_t)NW * a.M) * sizeof(float);
    if (prepare) return hipFuncSetAttribute(reinterpret_cast<const void*>(sinkhorn_split_kernel<NC, NW, GMAX>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((sinkhorn_split_kernel<NC, NW, GMAX>), dim3(B * a.G), dim3(NW * 64), lds, s, a);
    return hipGetLastError();
}
static int launch_split(const SkCall& c, const SkPlan& pl) {
    // by the slot's NC: SK_RAGGED_1 .. SK_RAGGED_8, SK_RAGGED_16, SK_RAGGED_32; a wide slot (more than 512 rows or columns) on the instantiations for
    // up to 16 slabs, 8 waves where NC >= 16
    typedef hipError_t (*Launch)(const SkSplitArgs&, int, hipStream_t, bool);
    static const Launch narrow[] = {launch_sk_split<1>, launch_sk_split<2>, launch_sk_split<4>, launch_sk_split<8>};
    static const Launch wide[] = {launch_sk_split<1, SK_SPLIT_NW, SK_SPLIT_WIDE_GMAX>, launch_sk_split<2, SK_SPLIT_NW, SK_SPLIT_WIDE_GMAX>,
                                  launch_sk_split<4, SK_SPLIT_NW, SK_SPLIT_WIDE_GMAX>, launch_sk_split<8, SK_SPLIT_NW, SK_SPLIT_WIDE_GMAX>,
                                  launch_sk_split<16, SK_SPLIT_WIDE_NW, SK_SPLIT_WIDE_GMAX>, launch_sk_split<32, SK_SPLIT_WIDE_NW, SK_SPLIT_WIDE_GMAX>};
    const bool wide_slot = c.wide && sk_wide_slot(c.N, c.M);
    const SkSplitLayout l = sk_split_layout(c.B, c.N, c.M, c.wide);
    const int nc = pl.stream >= SK_RAGGED_16 ? 4 + (pl.stream - SK_RAGGED_16) : pl.stream - SK_RAGGED_1;
    if (pl.stream < SK_RAGGED_1 || nc > (wide_slot ? 5 : 3) || pl.split != l.G || pl.split > (wide_slot ? SK_SPLIT_WIDE_GMAX : SK_SPLIT_GMAX)) {
        mdgat_set_error("sinkhorn: no split form for slots of %d x %d", c.N, c.M);
        return MDGAT_ERR_UNSUPPORTED;
    }
    if (!l.usable(c.split_ws, c.split_ws_bytes)) { mdgat_set_error("sinkhorn: the split form needs %zu bytes of 256-byte aligned scratch", l.total); return MDGAT_ERR_BAD_ARG; }
    SkSplitArgs a{c.scores, c.alpha_dev, c.alpha_host, c.Z, c.N, c.M, c.iters, c.cnt0, c.cnt1};
    a.part = reinterpret_cast<float2*>(static_cast<char*>(c.split_ws) + l.part); a.u = reinterpret_cast<float*>(static_cast<char*>(c.split_ws) + l.u); a.G = l.G;
    const Launch run = wide_slot ? wide[nc] : narrow[nc];
    if (int rc = mdgat_check_hip(run(a, c.B, c.stream, true), "sinkhorn LDS attribute")) return rc;
    for (a.it = 0; a.it < c.iters; ++a.it) {
        if (int rc = mdgat_check_hip(run(a, c.B, c.stream, false), "sinkhorn split launch")) return rc;
        if (wide_slot) ragged_wide_count_launch(RAGGED_WIDE_SPLIT_ITERATION);
        if (c.launched) c.launched(c.launched_ctx);
    }
    const size_t lds = ((size_t)(c.N + 1) + (c.M + 1)) * sizeof(float);
    if (wide_slot) hipLaunchKernelGGL((sinkhorn_split_finish_kernel<SK_SPLIT_NW, SK_SPLIT_WIDE_GMAX>), dim3(c.B * a.G), dim3(SK_SPLIT_NW * 64), lds, c.stream, a);
    else hipLaunchKernelGGL((sinkhorn_split_finish_kernel<SK_SPLIT_NW>), dim3(c.B * a.G), dim3(SK_SPLIT_NW * 64), lds, c.stream, a);
    if (int rc = mdgat_check_hip(hipGetLastError(), "sinkhorn split finishing launch")) return rc;
    if (wide_slot) ragged_wide_count_launch(RAGGED_WIDE_SPLIT_FINISH);
    return c.ex ? launch_extract(c.B, c.N, c.M, c.Z, *c.ex, c.stream, c.cnt0, c.cnt1) : MDGAT_OK;
}

// On a usable workspace the cluster kernel; otherwise, and for every call with counts, the streaming kernel into Z - a ragged batch on the RAGGED instantiation
// for its slot, picked from the padded sizes alone: a wider NC than a pair's own M would select gives the pair the same bits - or, where the caller opted in
// (SkCall::split) and the slot has two slabs of rows or more, the split form - then extract_kernel on that Z.
int launch_sinkhorn(const SkCall& c) {
    const int B = c.B, N = c.N, M = c.M;
    if (B <= 0) return MDGAT_OK;
    const bool ragged = c.cnt0 || c.cnt1;
    if (!c.scores || (ragged && (!c.cnt0 || !c.cnt1))) { mdgat_set_error("sinkhorn: null pointer"); return MDGAT_ERR_BAD_ARG; }
    if (!c.Z && !c.ex) { mdgat_set_error("sinkhorn: nothing to compute (no Z, no extraction)"); return MDGAT_ERR_BAD_ARG; }
    if (N <= 0 || M <= 0 || c.iters < 0) { mdgat_set_error("sinkhorn: bad shape N=%d M=%d iters=%d", N, M, c.iters); return MDGAT_ERR_BAD_ARG; }
    const SkLayout l = sk_layout(B, N, M);
    const bool usable = !ragged && l.usable(c.ws, c.ws_bytes);      // (the cluster kernel takes no counts)
    const SkPlan p = sinkhorn_plan(B, N, M, usable ? mdgat_cu_count() : 0, usable, c.Z || c.Zfb, ragged, ragged && c.split, ragged && c.wide);
    if (usable) return launch_scaling(c, p, l);
    if (!c.Z) { mdgat_set_error("sinkhorn: the streaming kernel needs a Z buffer"); return MDGAT_ERR_BAD_ARG; }
    if (ragged && p.rc) { mdgat_set_error("sinkhorn: ragged slots of %d x %d: at most %d keypoints per frame", N, M, sk_ragged_limit(c.wide)); return p.rc; }
    if (p.split) return launch_split(c, p);
    SkArgs a{c.scores, c.alpha_dev, c.alpha_host, c.Z, N, M, c.iters};
    a.cnt0 = c.cnt0; a.cnt1 = c.cnt1;
    if (int rc = launch_streaming(a, B, p.stream, false, c.stream)) return rc;
    return c.ex ? launch_extract(B, N, M, c.Z, *c.ex, c.stream, c.cnt0, c.cnt1) : MDGAT_OK;
}
