// The backward of the fp64 attention (attention / dynamic_attention, mdgat.py:190-210; forward: attention_f64_kernel in f64.hip).
//
// Per (pair, frame, head), s = 1 / sqrt(32), Q [nq][32] the frame's queries, K, V [nk][32] the keys and values of its source (the
// frame itself, or the other one in a cross layer), G = dL/dO [nq][32]:
//      S = s Q K^T,   P = softmax of S over the KEPT keys of each row (all keys, or the forward's top-k set), exactly 0 elsewhere,   O = P V
//      D_i = sum_d G_id O_id = sum_j P_ij dP_ij,   dP = G V^T,   dS_ij = P_ij (dP_ij - D_i)
//      dQ = s dS K,   dK = s dS^T Q,   dV = P^T G
// (tests/attention_grad_ref.py restates it in numpy).  The selection is an INPUT: the forward's selection words (mdgat_taps.topk_sel
// layout, [B][4][N + M][W] with bit j of word w = key 32 w + j of the row's source frame).  Nothing is decided again here, so no
// near tie can fall differently between forward and backward, and a key that was not kept contributes a P of exactly 0.0 - the
// forward's "exp(-700) instead of 0" shortcut is not used.
//
// Two passes on v_mfma_f64_16x16x4_f64 (operand / accumulator layout: f64_dev.hpp), no workgroup waits for another, no value atomics:
//   ag_row_kernel  a workgroup owns 64 queries of a (pair, frame, head), a wave 16 of them, and walks the source's keys in blocks of
//                  16 whose K and V tiles pass through LDS (two buffers, one barrier per block; the next block travels in registers
//                  under the products).  Walk 1: S^T = K Q^T and dP^T = V G^T put a query's four keys (g, g + 4, g + 8, g + 12) into
//                  one lane; every LANE keeps an online softmax of its own quarter of the keys (maximum, sum of exp, sum of exp x dP)
//                  against a lazy reference (f64.hip: it moves only when a logit exceeds it by 8), and the four quarters are
//                  combined once at the end: lse_i and D_i, which go to the workspace.  Walk 2: the logits and dP again,
//                  P = exp(S - lse), dS = P (dP - D) is the B operand of dQ^T = K^T dS as it stands.
//   ag_col_kernel  a workgroup owns 64 keys of a (pair, key frame, head), a wave 16 of them (their K and V fragments stay in
//                  registers), and walks the queries that read them in blocks of 16: s Q and G tiles, the rows' lse and D and the
//                  selection words of the workgroup's keys pass through LDS.  S = (s Q) K^T and dP = G V^T put a key's four
//                  queries into one lane; P and dS are the B operands of dV^T = G^T P and dK^T = (s Q)^T dS.
// Every element of dqkv is written exactly once - dq by the row pass, dk and dv by the column pass - and its terms are added in key
// (query) order by one chain: the bits repeat from run to run and a pair's gradient does not depend on the batch it travels in.
// Matrix work per 16 x 16 tile pair: 16 + 24 instructions in the row pass, 32 in the column pass, against 16 in the forward.
// Why the row pass walks twice: dS needs the row's D, which is complete only after the last key, and a row's S and dP cannot wait for
// it on chip - 2 x 2048 doubles per query, 2 MB for a workgroup's 64 queries - so they are formed again; the alternative that folds
// D out of the sum (dQ = s (sum_j P dP K - D sum_j P K)) saves eight instructions per tile pair and subtracts two nearly equal sums.
// Workspace: lse and D, 16 bytes per (pair, head, point).
#include "common.hpp"
#include "f64.hpp"
#include "f64_dev.hpp"

#include "exp2_tab256.hpp"

namespace {

constexpr int AG_LD = 34;                        // pitch of a staged [16][32] tile: rows stay 16-byte aligned
constexpr int AG_TILE = 16 * AG_LD;
constexpr double AG_SCALE = 0.17677669529663687; // 1 / sqrt(32) (mdgat.py:192, 201)
constexpr double AG_NEG = -1e300;                // "no key yet": finite, so that differences of references stay numbers
constexpr double AG_TAU = 8.0;                   // the lazy reference of walk 1 (TAU_LAZY of the forward)
constexpr size_t AG_ROW_LDS = (256 + 4 * AG_TILE) * sizeof(double);
constexpr size_t AG_COL_LDS = AG_ROW_LDS + 2 * 32 * sizeof(double) + 2 * 32 * sizeof(uint32_t);

struct AgArgs {
    int N, M, cross;
    const double* qkv;       // [B][P][384]
    const uint32_t* sel;     // [B][4][P][selW] (MASK kernels)
    int selW;
    const double* dmsg;      // [B][P][128]
    double* dqkv;            // [B][P][384]
    double* stats;           // [B][4][P][2]: lse, D
    int units, tiles;        // B * 2 * 4 units (pair, frame, head); 64-row tiles per unit
};

// this thread's 32 bytes of the two [16][32] tiles of a block: tile tid >> 7, row (tid & 127) >> 3, columns 4 (tid & 7) ...
struct AgPiece { f64x2 v[2]; };
__device__ __forceinline__ AgPiece ag_fetch(const double* base0, int stride0, const double* base1, int stride1, int row0, int rows, int tid) {
    const int e = tid & 127, row = row0 + (e >> 3), col = (e & 7) * 4;
    AgPiece p;
    p.v[0] = p.v[1] = f64x2{0.0, 0.0};
    if (row < rows) {
        const double* src = (tid >> 7) ? base1 + (size_t)row * stride1 + col : base0 + (size_t)row * stride0 + col;
        p.v[0] = *reinterpret_cast<const f64x2*>(src);
        p.v[1] = *reinterpret_cast<const f64x2*>(src + 2);
    }
    return p;
}
__device__ __forceinline__ void ag_stash(double* tiles, const AgPiece& p, int tid) {
    const int e = tid & 127;
    double* dst = tiles + (tid >> 7) * AG_TILE + (e >> 3) * AG_LD + (e & 7) * 4;
    *reinterpret_cast<f64x2*>(dst) = p.v[0];
    *reinterpret_cast<f64x2*>(dst + 2) = p.v[1];
}

// the two [16 x 16] products of a block that share the staged operand's row: X = T0 B0^T, Y = T1 B1^T (A: tile row l15, dims 8 g + j)
__device__ __forceinline__ void ag_products(const double* T, int l15, int g, const double (&b0)[8], const double (&b1)[8], f64x4& X, f64x4& Y) {
    const double* p0 = T + l15 * AG_LD + 8 * g;
    const double* p1 = p0 + AG_TILE;
    X = f64x4{0.0, 0.0, 0.0, 0.0};
    Y = X;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f64x2 x = *reinterpret_cast<const f64x2*>(p0 + 2 * j), y = *reinterpret_cast<const f64x2*>(p1 + 2 * j);
        X = mfma64(x[0], b0[2 * j], X);
        X = mfma64(x[1], b0[2 * j + 1], X);
        Y = mfma64(y[0], b1[2 * j], Y);
        Y = mfma64(y[1], b1[2 * j + 1], Y);
    }
}
// acc^T += T^T w: A = tile rows 4 s + g (k), dims 2 l15 and 2 l15 + 1 (two output blocks), B = w[s]
__device__ __forceinline__ void ag_accumulate(const double* T, int l15, int g, const f64x4& w, f64x4& acc0, f64x4& acc1) {
    const double* p = T + g * AG_LD + 2 * l15;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const f64x2 x = *reinterpret_cast<const f64x2*>(p + 4 * s * AG_LD);
        acc0 = mfma64(x[0], w[s], acc0);
        acc1 = mfma64(x[1], w[s], acc1);
    }
}

template <bool MASK>
__global__ __launch_bounds__(256) void ag_row_kernel(AgArgs a) {
    extern __shared__ __attribute__((aligned(16))) double ag_lds[];
    double* tab = ag_lds;
    double* tiles = ag_lds + 256;            // [2 buffers][K tile, V tile]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    // (the forward's grid: workgroups i, i + 8, ... - one XCD - walk the tiles of one unit)
    const int slot = blockIdx.x >> 3;
    const int unit = (slot / a.tiles) * 8 + (blockIdx.x & 7), tile = slot % a.tiles;
    if (unit >= a.units) return;
    const int head = unit & 3, side = (unit >> 2) & 1, b = unit >> 3;
    const int P = a.N + a.M;
    const int nq = side ? a.M : a.N, q_off = side ? a.N : 0;
    const int src = a.cross ? 1 - side : side;
    const int nk = src ? a.M : a.N, k_off = src ? a.N : 0;
    const int q0 = tile * 64;
    if (q0 >= nq) return;
    tab[tid] = MDGAT_EXP2_TAB256[tid];       // (256 threads; the first barrier of the walk is in front of the first exponential)
    const ExpConst ec = exp_const();
    const bool active = q0 + wave * 16 < nq;           // (a wave without queries still stages and meets the barriers)
    const int query = q0 + wave * 16 + l15;
    const bool valid = query < nq;
    const size_t qrow = (size_t)b * P + q_off + (valid ? query : nq - 1);

    // B operands of both products: dims 8 g + j of query l15 - s Q and G
    double qf[8], gf[8];
    {
        const f64x2* qp = reinterpret_cast<const f64x2*>(a.qkv + qrow * 384 + head * 32 + 8 * g);
        const f64x2* gp = reinterpret_cast<const f64x2*>(a.dmsg + qrow * 128 + head * 32 + 8 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f64x2 q = qp[j], gv = gp[j];
            qf[2 * j] = valid ? q[0] * AG_SCALE : 0.0;
            qf[2 * j + 1] = valid ? q[1] * AG_SCALE : 0.0;
            gf[2 * j] = valid ? gv[0] : 0.0;
            gf[2 * j + 1] = valid ? gv[1] : 0.0;
        }
    }
    const uint32_t* selrow = MASK ? a.sel + (((size_t)b * 4 + head) * P + q_off + (valid ? query : nq - 1)) * a.selW : nullptr;
    const double* kbase = a.qkv + ((size_t)b * P + k_off) * 384 + 128 + head * 32;
    const int nblk = (nk + 15) >> 4;

    auto walk = [&](auto body) {
        AgPiece r = ag_fetch(kbase, 384, kbase + 128, 384, 0, nk, tid);
        ag_stash(tiles, r, tid);
        __syncthreads();
        for (int jb = 0; jb < nblk; ++jb) {
            const bool more = jb + 1 < nblk;
            if (more) r = ag_fetch(kbase, 384, kbase + 128, 384, (jb + 1) * 16, nk, tid);
            if (active) body(jb, tiles + (jb & 1) * 2 * AG_TILE);
            if (more) ag_stash(tiles + ((jb + 1) & 1) * 2 * AG_TILE, r, tid);
            __syncthreads();
        }
    };
    // which of this lane's four keys (16 jb + g + 4 r) the row kept: bit r
    auto kept = [&](int jb) -> unsigned {
        unsigned bits = 0xfu;
        if (MASK) {
            const uint32_t w = selrow[jb >> 1] >> (16 * (jb & 1) + g);
            bits = (w & 1u) | ((w >> 3) & 2u) | ((w >> 6) & 4u) | ((w >> 9) & 8u);
        }
        const int over = jb * 16 + 16 - nk;            // the last block of a ragged frame
        if (over > 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (jb * 16 + g + 4 * r >= nk) bits &= ~(1u << r);
        }
        return bits;
    };

    // ---- walk 1: the row's lse and D ----
    double m = AG_NEG, mthr = AG_NEG, l = 0.0, d = 0.0;
    walk([&](int jb, const double* T) {
        f64x4 S, dP;
        ag_products(T, l15, g, qf, gf, S, dP);
        const unsigned bits = kept(jb);
        double lm = AG_NEG;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if ((bits >> r) & 1u) lm = fmax(lm, S[r]);
        if (__any(lm > mthr)) {
            const double mnew = fmax(m, lm);
            const double sc = exp_fast(m - mnew, tab, ec);       // (lanes that stay: exp(0) = 1 exactly; first key of a lane: 1e-304 x 0)
            l *= sc;
            d *= sc;
            m = mnew;
            mthr = mnew + AG_TAU;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double p = ((bits >> r) & 1u) ? exp_fast(S[r] - m, tab, ec) : 0.0;
            l += p;
            d = __builtin_fma(p, dP[r], d);
        }
    });
    double lse = 0.0, Dv = 0.0;
    if (active) {
        const double mx = quad_max(m);
        const double f = exp_fast(m - mx, tab, ec);              // (a lane without a kept key: l = d = 0)
        const double L = quad_sum(l * f), Dn = quad_sum(d * f);
        // (a row whose selection words keep no key - the forward never writes one - has L = 0: it keeps lse = D = 0, every P of it
        // is the select's 0.0 in both passes, and it sends exact zeros instead of NaN)
        if (L > 0.0) {
            lse = mx + log(L);
            Dv = Dn / L;
        }
        if (g == 0 && valid) *reinterpret_cast<f64x2*>(a.stats + (((size_t)b * 4 + head) * P + q_off + query) * 2) = f64x2{lse, Dv};
    }

    // ---- walk 2: dS, dQ^T = K^T dS ----
    f64x4 dq0 = {0.0, 0.0, 0.0, 0.0}, dq1 = dq0;
    walk([&](int jb, const double* T) {
        f64x4 S, dP, dS;
        ag_products(T, l15, g, qf, gf, S, dP);
        const unsigned bits = kept(jb);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double p = ((bits >> r) & 1u) ? exp_fast(S[r] - lse, tab, ec) : 0.0;
            dS[r] = p * (dP[r] - Dv);
        }
        ag_accumulate(T, l15, g, dS, dq0, dq1);
    });
    // D: lane (query l15, g), register r of block t -> dim 2 (g + 4 r) + t
    if (valid) {
        double* dst = a.dqkv + qrow * 384 + head * 32 + 2 * g;
#pragma unroll
        for (int r = 0; r < 4; ++r) *reinterpret_cast<f64x2*>(dst + 8 * r) = f64x2{dq0[r] * AG_SCALE, dq1[r] * AG_SCALE};
    }
}

template <bool MASK>
__global__ __launch_bounds__(256) void ag_col_kernel(AgArgs a) {
    extern __shared__ __attribute__((aligned(16))) double ag_lds[];
    double* tab = ag_lds;
    double* tiles = ag_lds + 256;                                      // [2 buffers][s Q tile, G tile]
    double* stat = tiles + 4 * AG_TILE;                                // [2][16 queries][lse, D]
    uint32_t* words = reinterpret_cast<uint32_t*>(stat + 2 * 32);      // [2][16 queries][2 words: the workgroup's 64 keys]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int slot = blockIdx.x >> 3;
    const int unit = (slot / a.tiles) * 8 + (blockIdx.x & 7), tile = slot % a.tiles;
    if (unit >= a.units) return;
    const int head = unit & 3, kfr = (unit >> 2) & 1, b = unit >> 3;
    const int P = a.N + a.M;
    const int nk = kfr ? a.M : a.N, k_off = kfr ? a.N : 0;
    const int side = a.cross ? 1 - kfr : kfr;                          // the frame whose queries read these keys
    const int nq = side ? a.M : a.N, q_off = side ? a.N : 0;
    const int k0 = tile * 64;
    if (k0 >= nk) return;
    tab[tid] = MDGAT_EXP2_TAB256[tid];
    const ExpConst ec = exp_const();
    const bool active = k0 + wave * 16 < nk;
    const int key = k0 + wave * 16 + l15;
    const bool valid = key < nk;
    const size_t krow = (size_t)b * P + k_off + (valid ? key : nk - 1);

    // B operands of both products: dims 8 g + j of key l15 - K and V
    double kf[8], vf[8];
    {
        const f64x2* kp = reinterpret_cast<const f64x2*>(a.qkv + krow * 384 + 128 + head * 32 + 8 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f64x2 k = kp[j], v = kp[64 + j];
            kf[2 * j] = valid ? k[0] : 0.0;
            kf[2 * j + 1] = valid ? k[1] : 0.0;
            vf[2 * j] = valid ? v[0] : 0.0;
            vf[2 * j + 1] = valid ? v[1] : 0.0;
        }
    }
    const double* qbase = a.qkv + ((size_t)b * P + q_off) * 384 + head * 32;
    const double* gbase = a.dmsg + ((size_t)b * P + q_off) * 128 + head * 32;
    const size_t srow = ((size_t)b * 4 + head) * P + q_off;
    const int nblk = (nq + 15) >> 4;

    struct Extra { f64x2 st; uint32_t w; };
    auto fetch = [&](int qb, AgPiece& r, Extra& x) {
        r = ag_fetch(qbase, 384, gbase, 128, qb * 16, nq, tid);
        if (tid < 128) {                                               // the Q tile is staged times s: S = (s Q) K^T, dK = dS^T (s Q)
            r.v[0] *= AG_SCALE;
            r.v[1] *= AG_SCALE;
        }
        x.st = f64x2{0.0, 0.0};
        x.w = 0u;
        if (tid < 16) {
            if (qb * 16 + tid < nq) x.st = *reinterpret_cast<const f64x2*>(a.stats + (srow + qb * 16 + tid) * 2);
        } else if (MASK && tid < 48) {
            const int i = tid - 16, q = qb * 16 + (i >> 1), w = (k0 >> 5) + (i & 1);
            if (q < nq && w < a.selW) x.w = a.sel[(srow + q) * a.selW + w];
        }
    };
    auto stash = [&](int buf, const AgPiece& r, const Extra& x) {
        ag_stash(tiles + buf * 2 * AG_TILE, r, tid);
        if (tid < 16) *reinterpret_cast<f64x2*>(stat + buf * 32 + 2 * tid) = x.st;
        else if (MASK && tid < 48) words[buf * 32 + tid - 16] = x.w;
    };

    f64x4 dk0 = {0.0, 0.0, 0.0, 0.0}, dk1 = dk0, dv0 = dk0, dv1 = dk0;
    AgPiece r;
    Extra x;
    fetch(0, r, x);
    stash(0, r, x);
    __syncthreads();
    for (int qb = 0; qb < nblk; ++qb) {
        const bool more = qb + 1 < nblk;
        if (more) fetch(qb + 1, r, x);
        if (active) {
            const int buf = qb & 1;
            const double* T = tiles + buf * 2 * AG_TILE;
            f64x4 S, dP, p, dS;
            ag_products(T, l15, g, kf, vf, S, dP);                     // lane: key l15, queries g + 4 r
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int qi = g + 4 * rr;
                const f64x2 st = *reinterpret_cast<const f64x2*>(stat + buf * 32 + 2 * qi);
                bool keep = valid;
                if (MASK) keep = keep && ((words[buf * 32 + 2 * qi + (wave >> 1)] >> ((wave & 1) * 16 + l15)) & 1u);
                p[rr] = keep ? exp_fast(S[rr] - st[0], tab, ec) : 0.0;
                dS[rr] = p[rr] * (dP[rr] - st[1]);
            }
            ag_accumulate(T + AG_TILE, l15, g, p, dv0, dv1);           // dV^T += G^T P
            ag_accumulate(T, l15, g, dS, dk0, dk1);                    // dK^T += (s Q)^T dS
        }
        if (more) stash((qb + 1) & 1, r, x);
        __syncthreads();
    }
    if (valid) {
        double* dst = a.dqkv + krow * 384 + 128 + head * 32 + 2 * g;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            *reinterpret_cast<f64x2*>(dst + 8 * rr) = f64x2{dk0[rr], dk1[rr]};
            *reinterpret_cast<f64x2*>(dst + 128 + 8 * rr) = f64x2{dv0[rr], dv1[rr]};
        }
    }
}

}  // namespace

size_t attention_backward_f64_workspace_bytes(int B, int N, int M) { return mdgat_align256((size_t)B * 4 * (N + M) * 2 * sizeof(double)); }

int launch_attention_backward_f64(int B, int N, int M, int cross, int topk, const double* qkv, const uint32_t* sel, const double* dmsg, double* dqkv,
                                  void* workspace, hipStream_t s) {
    if (B <= 0 || N <= 0 || M <= 0) return MDGAT_OK;
    AgArgs a{};
    a.N = N; a.M = M; a.cross = cross; a.qkv = qkv; a.sel = sel; a.dmsg = dmsg; a.dqkv = dqkv;
    a.stats = static_cast<double*>(workspace);
    const int nmax = N > M ? N : M;
    a.selW = (nmax + 31) / 32;
    a.units = B * 2 * MDGAT_HEADS;
    a.tiles = (nmax + 63) / 64;
    const unsigned grid = 8u * a.tiles * ((a.units + 7) / 8);
    if (topk > 0) {
        hipLaunchKernelGGL(ag_row_kernel<true>, dim3(grid), dim3(256), AG_ROW_LDS, s, a);
        hipLaunchKernelGGL(ag_col_kernel<true>, dim3(grid), dim3(256), AG_COL_LDS, s, a);
    } else {
        hipLaunchKernelGGL(ag_row_kernel<false>, dim3(grid), dim3(256), AG_ROW_LDS, s, a);
        hipLaunchKernelGGL(ag_col_kernel<false>, dim3(grid), dim3(256), AG_COL_LDS, s, a);
    }
    return mdgat_check_hip(hipGetLastError(), "attention backward launch");
}
