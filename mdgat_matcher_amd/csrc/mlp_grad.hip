// The reference's MLP(channels) (mdgat.py:34-46) in TRAINING mode and its backward, in fp64: Conv1d(k=1), and after every convolution
// but the last BatchNorm1d on the batch's own statistics and ReLU.  The inference forward folds BN into the weights (pack.py); a
// training step cannot: the statistics are taken over all R = B P rows of the call, the gradient runs through them, and the running
// buffers move.  tests/mlp_grad_ref.py restates all of it in numpy.
//
// Rows are points: x0 [R][K0] | x1 [R][K1] side by side (GemmF64Args::A0 / A1: the layer's cat([x, message]) is never built), W_l
// [C_l][C_in] as in the state_dict, out [R][C_L].  Per convolution l:
//      Y_l = A_{l-1} W_l^T + b_l;   mean_c, var_c (biased) over the rows;   z = gamma (Y - mean) invstd + beta;   A_l = max(z, 0)
// What is kept for the backward is Y_l of every BN layer and mean / invstd / a = gamma invstd per channel.  A_l is NEVER stored:
// z = fma(Y - mean, a, beta) is recomputed where the next product loads its A operand (mg_gemm_bn_kernel), where dW loads its B
// operand (mg_dw_kernel) and where the backward masks (mg_bnbwd_*) - the same instruction everywhere, so the sign of z is the same
// everywhere.  torch keeps the convolution output, the BN output and the ReLU output of every layer.
//
// Forward launches.  Layer 0 is the exact mode's launch_gemm_f64 (two sources, no transform); the layers behind a BN run
// mg_gemm_bn_kernel, that kernel's tile loop (64 x 64 / 64 x 128 tiles, chunks of 32 through LDS, the next chunk in flight in
// registers) with the normalisation and the ReLU between the global load and the LDS store.  Batch statistics: mg_stats_kernel gives
// every slab of 256 rows its column sums and, around the SLAB's mean, the centred sums of squares M2 (two passes over rows that are
// in cache after the first); mg_stats_final_kernel combines the slabs in slab order by Chan's update
//      delta = mean_b - mean;  mean += delta n_b / n;  M2 += M2_b + delta^2 n_a n_b / n
// - never E[y^2] - E[y]^2 - and moves the running buffers (running_var takes the unbiased M2 / (R - 1)).  With training == 0 the
// running statistics stand in and nothing is written to them.
//
// Backward, from the last convolution to the first (dY_L = dout):
//   mg_dw_kernel      dW_l = dY_l^T A_{l-1} and db_l = colsum(dY_l) over a slab of 512 rows: both operands are contracted over their
//                     ROWS, so both fragments are coalesced loads and there is no LDS (hg_dw_kernel's shape); a wave owns 32 x 32 of
//                     dW, ONE chain per element inside the slab; the B operand is A_{l-1} recomputed from Y_{l-1} as it is loaded.
//   mg_reduce_kernel  the slabs' partials added in slab order.
//   dA_{l-1} = dY_l W_l: launch_gemm_f64 on W_l transposed into the workspace (mg_transpose_kernel; a weight is at most 2 MB); at
//                     the first layer one launch per source writes dx0 / dx1 from the two row ranges of the transposed weight.
//   mg_bnbwd_partial_kernel / _final_kernel   dz = dA [z > 0]; dbeta = colsum(dz), dgamma = colsum(dz yhat): slabs of 256 rows, their
//                     partials added in slab order.
//   mg_bnbwd_apply_kernel   dY_{l-1} = a (dz - dbeta / R - yhat dgamma / R) in place of dA (training == 0: a dz).
// No value atomics, no workgroup waits for another: the bits are the same from run to run.  The walk stops below the lowest
// gradient that is wanted.  A channel that is dead for the whole batch has dz = 0 exactly, hence exact zeros in dgamma, dbeta, dY and
// its row of dW.
#include "common.hpp"
#include "f64.hpp"
#include "f64_dev.hpp"

namespace {

constexpr int MG_SLAB = 256;        // rows per partial of a column statistic (mean / M2, dbeta / dgamma)
constexpr int MG_DW_SLAB = 512;     // rows per partial of dW / db
constexpr int MG_BM = 64, MG_KC = 32, MG_LD = MG_KC + 2;      // gemm_f64_kernel's tile: row pitch 34 doubles

// the one place z is formed: every kernel that needs z or its sign calls this
__device__ __forceinline__ double bn_z(double y, double mean, double a, double beta) { return __builtin_fma(y - mean, a, beta); }
__device__ __forceinline__ double bn_relu(double y, double mean, double a, double beta) {
    const double z = bn_z(y, mean, a, beta);
    return z > 0.0 ? z : 0.0;
}

// ================================================================================================ forward product behind a BN
struct MgGemmArgs {
    const double* Y; int K;            // [M][K]: the previous convolution's output
    const double *mean, *a, *beta;     // [K] each: its BN
    const double* W;                   // [N][K]
    const double* bias;                // [N]
    double* C;                         // [M][N]
    int M, N;
};

// FAST: whole tiles, K a multiple of 32, W 16-byte aligned: 16-byte loads without predicates (as gemm_f64_kernel's)
template <int WN, bool FAST>
__global__ __launch_bounds__(256) void mg_gemm_bn_kernel(MgGemmArgs p) {
    constexpr int BN = 32 * WN;
    extern __shared__ __attribute__((aligned(16))) double mg_lds[];
    double* As = mg_lds;                      // [64][MG_LD]
    double* Ws = mg_lds + MG_BM * MG_LD;      // [BN][MG_LD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int wm = wave & 1, wn = wave >> 1;
    const int row0 = blockIdx.x * MG_BM, col0 = blockIdx.y * BN;
    constexpr int NA = MG_BM * MG_KC / 256, NW = BN * MG_KC / 256;
    double ra[NA], rw[NW];
    auto fetch = [&](int k0) {
        if (FAST) {
            const int kk = k0 + (tid & 15) * 2;          // this thread's two channels of the chunk: the same for every row it loads
            const double m0 = p.mean[kk], m1 = p.mean[kk + 1], a0 = p.a[kk], a1 = p.a[kk + 1], b0 = p.beta[kk], b1 = p.beta[kk + 1];
#pragma unroll
            for (int u = 0; u < NA / 2; ++u) {
                const int r = (tid + 256 * u) >> 4;
                const f64x2 v = *reinterpret_cast<const f64x2*>(p.Y + (size_t)(row0 + r) * p.K + kk);
                ra[2 * u] = bn_relu(v[0], m0, a0, b0); ra[2 * u + 1] = bn_relu(v[1], m1, a1, b1);
            }
#pragma unroll
            for (int u = 0; u < NW / 2; ++u) {
                const int r = (tid + 256 * u) >> 4;
                const f64x2 v = *reinterpret_cast<const f64x2*>(p.W + (size_t)(col0 + r) * p.K + kk);
                rw[2 * u] = v[0]; rw[2 * u + 1] = v[1];
            }
            return;
        }
        const int kk = k0 + (tid & 31);
        const bool ink = kk < p.K;
        const double m = ink ? p.mean[kk] : 0.0, aa = ink ? p.a[kk] : 0.0, bb = ink ? p.beta[kk] : 0.0;
#pragma unroll
        for (int u = 0; u < NA; ++u) {
            const int row = row0 + ((tid + 256 * u) >> 5);
            ra[u] = (ink && row < p.M) ? bn_relu(p.Y[(size_t)row * p.K + kk], m, aa, bb) : 0.0;       // (beyond the tile: 0, not max(beta, 0))
        }
#pragma unroll
        for (int u = 0; u < NW; ++u) {
            const int n = col0 + ((tid + 256 * u) >> 5);
            rw[u] = (ink && n < p.N) ? p.W[(size_t)n * p.K + kk] : 0.0;
        }
    };
    auto stash = [&]() {
        if (FAST) {
#pragma unroll
            for (int u = 0; u < NA / 2; ++u) { const int idx = tid + 256 * u; *reinterpret_cast<f64x2*>(As + (idx >> 4) * MG_LD + (idx & 15) * 2) = f64x2{ra[2 * u], ra[2 * u + 1]}; }
#pragma unroll
            for (int u = 0; u < NW / 2; ++u) { const int idx = tid + 256 * u; *reinterpret_cast<f64x2*>(Ws + (idx >> 4) * MG_LD + (idx & 15) * 2) = f64x2{rw[2 * u], rw[2 * u + 1]}; }
            return;
        }
#pragma unroll
        for (int u = 0; u < NA; ++u) { const int idx = tid + 256 * u; As[(idx >> 5) * MG_LD + (idx & 31)] = ra[u]; }
#pragma unroll
        for (int u = 0; u < NW; ++u) { const int idx = tid + 256 * u; Ws[(idx >> 5) * MG_LD + (idx & 31)] = rw[u]; }
    };
    f64x4 acc[2][WN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    fetch(0);
    stash();
    __syncthreads();
    const double* ap = As + (wm * 32 + l15) * MG_LD + g;
    const double* wp = Ws + (wn * 16 * WN + l15) * MG_LD + g;
    for (int k0 = 0; k0 < p.K; k0 += MG_KC) {
        const bool more = k0 + MG_KC < p.K;
        if (more) fetch(k0 + MG_KC);
        const int rem = p.K - k0;
        const int steps = rem >= MG_KC ? MG_KC / 4 : (rem + 3) >> 2;
        for (int j = 0; j < steps; ++j) {
            double fa[2], fw[WN];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = ap[i * 16 * MG_LD + 4 * j];
#pragma unroll
            for (int i = 0; i < WN; ++i) fw[i] = wp[i * 16 * MG_LD + 4 * j];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int n = 0; n < WN; ++n) acc[i][n] = mfma64(fa[i], fw[n], acc[i][n]);
        }
        if (more) {
            __syncthreads();
            stash();
            __syncthreads();
        }
    }
    // D: lane (column l15, g), register i -> row g + 4 i of the 16 x 16 block
#pragma unroll
    for (int nb = 0; nb < WN; ++nb) {
        const int n = col0 + wn * 16 * WN + nb * 16 + l15;
        if (n >= p.N) continue;
        const double bias = p.bias[n];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = row0 + wm * 32 + mb * 16 + g + 4 * i;
                if (row < p.M) p.C[(size_t)row * p.N + n] = acc[mb][nb][i] + bias;
            }
    }
}

// ================================================================================================ batch statistics
// a workgroup: 64 columns x one slab of rows; wave q walks rows q, q + 4, ...; the four waves are combined as (0 + 1) + (2 + 3)
__device__ __forceinline__ double mg_quarters(double (*red)[64], double v, int q, int l) {
    __syncthreads();          // (the previous combine's reads are done)
    red[q][l] = v;
    __syncthreads();
    return (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
}

struct MgStatArgs { const double* Y; int R, C; double* P; };      // P [slabs][2][C]: column sum, M2 around the slab's own mean
__global__ __launch_bounds__(256) void mg_stats_kernel(MgStatArgs p) {
    __shared__ double red[4][64];
    const int l = threadIdx.x & 63, q = threadIdx.x >> 6, c = blockIdx.y * 64 + l;
    const int r0 = blockIdx.x * MG_SLAB, n = min(MG_SLAB, p.R - r0);
    const bool in = c < p.C;
    const double* y = p.Y + (size_t)r0 * p.C + c;
    double s = 0.0;
    if (in) for (int r = q; r < n; r += 4) s += y[(size_t)r * p.C];
    const double tot = mg_quarters(red, s, q, l);
    const double bm = tot / (double)n;
    double m2 = 0.0;
    if (in) for (int r = q; r < n; r += 4) { const double d = y[(size_t)r * p.C] - bm; m2 = __builtin_fma(d, d, m2); }
    m2 = mg_quarters(red, m2, q, l);
    if (in && q == 0) {
        p.P[((size_t)blockIdx.x * 2) * p.C + c] = tot;
        p.P[((size_t)blockIdx.x * 2 + 1) * p.C + c] = m2;
    }
}

struct MgStatFinalArgs {
    const double* P; int R, C, training;
    double eps, momentum;
    const double* gamma;
    double *rm, *rv; long long* nbt;
    double* S;                          // [3][C]: mean, invstd, a = gamma invstd
};
__global__ __launch_bounds__(256) void mg_stats_final_kernel(MgStatFinalArgs p) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= p.C) return;
    double mean, var;
    if (p.training) {
        const int slabs = (p.R + MG_SLAB - 1) / MG_SLAB;
        double n = 0.0, M2 = 0.0;
        mean = 0.0;
        for (int b = 0; b < slabs; ++b) {         // Chan's update, in slab order
            const double nb = (double)min(MG_SLAB, p.R - b * MG_SLAB);
            const double mb = p.P[((size_t)b * 2) * p.C + c] / nb, delta = mb - mean, nt = n + nb;
            mean += delta * nb / nt;
            M2 += p.P[((size_t)b * 2 + 1) * p.C + c] + delta * delta * n * nb / nt;
            n = nt;
        }
        var = M2 / (double)p.R;
        p.rm[c] = (1.0 - p.momentum) * p.rm[c] + p.momentum * mean;
        p.rv[c] = (1.0 - p.momentum) * p.rv[c] + p.momentum * (M2 / (double)(p.R - 1));
        if (c == 0 && p.nbt) *p.nbt += 1;
    } else {
        mean = p.rm[c];
        var = p.rv[c];
    }
    const double invstd = 1.0 / sqrt(var + p.eps);
    p.S[c] = mean;
    p.S[p.C + c] = invstd;
    p.S[2 * p.C + c] = p.gamma[c] * invstd;
}

// ================================================================================================ BN + ReLU backward
struct MgBnBwdArgs {
    double* dA;                         // [R][C]: dL/dA in, dL/dY out (apply)
    const double* Y; const double* S; const double* beta;
    int R, C, training;
    double* P;                          // [slabs][2][C]: partial dbeta, dgamma
    double* Q;                          // [4][C]: dbeta, dgamma, dbeta / R, dgamma / R (zeros when training == 0)
    double *dgamma, *dbeta;             // the caller's, or nullptr
};
__global__ __launch_bounds__(256) void mg_bnbwd_partial_kernel(MgBnBwdArgs p) {
    __shared__ double red[4][64];
    const int l = threadIdx.x & 63, q = threadIdx.x >> 6, c = blockIdx.y * 64 + l;
    const int r0 = blockIdx.x * MG_SLAB, n = min(MG_SLAB, p.R - r0);
    const bool in = c < p.C;
    double s1 = 0.0, s2 = 0.0;
    if (in) {
        const double mean = p.S[c], invstd = p.S[p.C + c], a = p.S[2 * p.C + c], beta = p.beta[c];
        const size_t o = (size_t)r0 * p.C + c;
        for (int r = q; r < n; r += 4) {
            const double y = p.Y[o + (size_t)r * p.C];
            const double dz = bn_z(y, mean, a, beta) > 0.0 ? p.dA[o + (size_t)r * p.C] : 0.0;
            s1 += dz;
            s2 = __builtin_fma(dz, (y - mean) * invstd, s2);
        }
    }
    s1 = mg_quarters(red, s1, q, l);
    s2 = mg_quarters(red, s2, q, l);
    if (in && q == 0) {
        p.P[((size_t)blockIdx.x * 2) * p.C + c] = s1;
        p.P[((size_t)blockIdx.x * 2 + 1) * p.C + c] = s2;
    }
}
__global__ __launch_bounds__(256) void mg_bnbwd_final_kernel(MgBnBwdArgs p) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= p.C) return;
    const int slabs = (p.R + MG_SLAB - 1) / MG_SLAB;
    double s1 = p.P[c], s2 = p.P[p.C + c];
    for (int b = 1; b < slabs; ++b) { s1 += p.P[((size_t)b * 2) * p.C + c]; s2 += p.P[((size_t)b * 2 + 1) * p.C + c]; }
    p.Q[c] = s1;
    p.Q[p.C + c] = s2;
    p.Q[2 * p.C + c] = p.training ? s1 / (double)p.R : 0.0;
    p.Q[3 * p.C + c] = p.training ? s2 / (double)p.R : 0.0;
    if (p.dbeta) p.dbeta[c] = s1;
    if (p.dgamma) p.dgamma[c] = s2;
}
// grid (ceil(R / 64), ceil(C / 64)): 64 rows x 64 columns per workgroup
__global__ __launch_bounds__(256) void mg_bnbwd_apply_kernel(MgBnBwdArgs p) {
    const int l = threadIdx.x & 63, q = threadIdx.x >> 6, c = blockIdx.y * 64 + l;
    if (c >= p.C) return;
    const double mean = p.S[c], invstd = p.S[p.C + c], a = p.S[2 * p.C + c], beta = p.beta[c];
    const double mb = p.training ? p.Q[2 * p.C + c] : 0.0, mg = p.training ? p.Q[3 * p.C + c] : 0.0;     // (eval mode: Q may not have been formed)
    const int r0 = blockIdx.x * 64, n = min(64, p.R - r0);
    for (int r = q; r < n; r += 4) {
        const size_t o = (size_t)(r0 + r) * p.C + c;
        const double y = p.Y[o];
        const double dz = bn_z(y, mean, a, beta) > 0.0 ? p.dA[o] : 0.0;
        p.dA[o] = a * (dz - mb - (y - mean) * invstd * mg);
    }
}

// ================================================================================================ dW, db
struct MgDwArgs {
    const double* dY; int Cout;                     // [R][Cout]
    const double* x0; int K0;                       // the convolution's input: [R][K0] | [R][K1]; behind a BN: x0 = Y_{l-1}
    const double* x1; int K1;
    const double *mean, *a, *beta;                  // the BN between (A = max(z, 0) is formed as it is loaded), or nullptr
    int R;
    double* P;                                      // [slabs][Cout (K0 + K1) + Cout]
    int want_w;                                     // 0: only db is wanted - the waves of the first column tile add up their A fragments, no product is formed
};
__global__ __launch_bounds__(256) void mg_dw_kernel(MgDwArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int Cin = p.K0 + p.K1, Cout = p.Cout;
    const int tn = (Cin + 31) >> 5, tm = (Cout + 31) >> 5;
    const int id = blockIdx.y * 4 + wave;
    if (id >= tm * tn) return;
    const int rt = id / tn, ct = id % tn;
    const bool prod = p.want_w != 0;
    if (!prod && ct != 0) return;
    const int r0 = blockIdx.x * MG_DW_SLAB, cnt = min(MG_DW_SLAB, p.R - r0);
    // A: row = output channel (l15), k = point (g); Cout is a multiple of 16: the first half of the 32 always exists
    const bool oka1 = rt * 32 + 16 < Cout;
    const double* ap = p.dY + (size_t)(r0 + g) * Cout + rt * 32 + l15;
    // B: k = point, column = input channel
    const double* bp[2] = {nullptr, nullptr};
    int ldb[2] = {0, 0};
    bool okb[2];
    double mu[2] = {0.0, 0.0}, aa[2] = {0.0, 0.0}, be[2] = {0.0, 0.0};
    const bool bn = p.mean != nullptr;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ci = ct * 32 + h * 16 + l15;
        okb[h] = prod && ci < Cin;
        if (!okb[h]) continue;
        const bool first = ci < p.K0;
        ldb[h] = first ? p.K0 : p.K1;
        bp[h] = (first ? p.x0 + ci : p.x1 + (ci - p.K0)) + (size_t)(r0 + g) * ldb[h];
        if (bn) { mu[h] = p.mean[ci]; aa[h] = p.a[ci]; be[h] = p.beta[ci]; }
    }
    auto ldA = [&](int r, int h, bool in) -> double { return (in && (h == 0 || oka1)) ? ap[(size_t)r * Cout + h * 16] : 0.0; };
    auto ldB = [&](int r, int h, bool in) -> double {
        if (!(in && okb[h])) return 0.0;
        const double v = bp[h][(size_t)r * ldb[h]];
        return bn ? bn_relu(v, mu[h], aa[h], be[h]) : v;
    };
    f64x4 acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[r][c] = f64x4{0.0, 0.0, 0.0, 0.0};
    double s0 = 0.0, s1 = 0.0;
    auto step = [&](double a0, double a1, double b0, double b1) {
        if (prod) {
            acc[0][0] = mfma64(a0, b0, acc[0][0]);
            acc[0][1] = mfma64(a0, b1, acc[0][1]);
            acc[1][0] = mfma64(a1, b0, acc[1][0]);
            acc[1][1] = mfma64(a1, b1, acc[1][1]);
        }
        s0 += a0;
        s1 += a1;
    };
    int r = 0;
    for (; r + 16 <= cnt; r += 16) {          // sixteen loads in flight in front of sixteen products
        double fa[4][2], fb[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            fa[u][0] = ldA(r + 4 * u, 0, true); fa[u][1] = ldA(r + 4 * u, 1, true);
            fb[u][0] = ldB(r + 4 * u, 0, true); fb[u][1] = ldB(r + 4 * u, 1, true);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) step(fa[u][0], fa[u][1], fb[u][0], fb[u][1]);
    }
    for (; r < cnt; r += 4) {
        const bool in = r + g < cnt;
        step(ldA(r, 0, in), ldA(r, 1, in), ldB(r, 0, in), ldB(r, 1, in));
    }
    double* Pp = p.P + (size_t)blockIdx.x * ((size_t)Cout * Cin + Cout);
    if (prod)
#pragma unroll
    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int co = rt * 32 + rr * 16 + g + 4 * i, ci = ct * 32 + c * 16 + l15;
                if (co < Cout && ci < Cin) Pp[(size_t)co * Cin + ci] = acc[rr][c][i];
            }
    // db: the four quarters of the rows (k = g) as (0 + 1) + (2 + 3)
    s0 = quad_sum(s0);
    s1 = quad_sum(s1);
    if (ct == 0 && g == 0) {
        Pp[(size_t)Cout * Cin + rt * 32 + l15] = s0;
        if (oka1) Pp[(size_t)Cout * Cin + rt * 32 + 16 + l15] = s1;
    }
}

struct MgReduceArgs { const double* P; int slabs; int nW, nb; double *dW, *db; };      // dW == nullptr: the grid covers db alone
__global__ __launch_bounds__(256) void mg_reduce_kernel(MgReduceArgs p) {
    const int idx = blockIdx.x * 256 + threadIdx.x + (p.dW ? 0 : p.nW), part = p.nW + p.nb;
    if (idx >= part) return;
    double s = p.P[idx];
    for (int b = 1; b < p.slabs; ++b) s += p.P[(size_t)b * part + idx];
    if (idx < p.nW) { if (p.dW) p.dW[idx] = s; }
    else if (p.db) p.db[idx - p.nW] = s;
}

// Wt [K][N] = W [N][K]^T
__global__ __launch_bounds__(256) void mg_transpose_kernel(const double* W, double* Wt, int N, int K) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < N * K) Wt[idx] = W[(size_t)(idx % N) * K + idx / N];
}

// ================================================================================================ host
inline int mg_cin(const mdgat_mlp_desc& d, int l) { return l == 0 ? d.K0 + d.K1 : d.C[l - 1]; }
inline int mg_slabs(int R, int slab) { return (R + slab - 1) / slab; }

struct MgSaved { double* Y[MDGAT_MLP_MAX_CONVS - 1]; double* S[MDGAT_MLP_MAX_CONVS - 1]; double* P; size_t bytes; };
MgSaved mg_carve_saved(void* base, const mdgat_mlp_desc& d) {
    MgSaved w{};
    WsCarver c{static_cast<char*>(base)};
    int maxc = 0;
    for (int l = 0; l + 1 < d.n_conv; ++l) {
        c.take(w.Y[l], (size_t)d.R * d.C[l]);
        c.take(w.S[l], (size_t)3 * d.C[l]);
        maxc = d.C[l] > maxc ? d.C[l] : maxc;
    }
    c.take(w.P, (size_t)mg_slabs(d.R, MG_SLAB) * 2 * maxc);
    w.bytes = c.bytes;
    return w;
}

struct MgWs { double* Wt; double* G[2]; double* Pw; double* Pb; double* Q; size_t bytes; };
MgWs mg_carve_ws(void* base, const mdgat_mlp_desc& d) {
    MgWs w{};
    WsCarver c{static_cast<char*>(base)};
    size_t maxw = 0, maxpart = 0;
    int maxc = 0;
    for (int l = 0; l < d.n_conv; ++l) {
        const size_t nw = (size_t)d.C[l] * mg_cin(d, l);
        maxw = nw > maxw ? nw : maxw;
        maxpart = nw + d.C[l] > maxpart ? nw + d.C[l] : maxpart;
        if (l + 1 < d.n_conv) maxc = d.C[l] > maxc ? d.C[l] : maxc;
    }
    c.take(w.Wt, maxw);
    c.take(w.G[0], (size_t)d.R * maxc);
    c.take(w.G[1], d.n_conv > 2 ? (size_t)d.R * maxc : 0);
    c.take(w.Pw, (size_t)mg_slabs(d.R, MG_DW_SLAB) * maxpart);
    c.take(w.Pb, (size_t)mg_slabs(d.R, MG_SLAB) * 2 * maxc);
    c.take(w.Q, (size_t)4 * maxc);
    w.bytes = c.bytes;
    return w;
}

int mg_launch_gemm_bn(const MgGemmArgs& a, hipStream_t s) {
    static std::atomic<unsigned long long> d2{0}, d4{0}, d2f{0}, d4f{0};
    const int wn = a.N % 128 == 0 ? 4 : 2, bn = 32 * wn;
    const bool fast = a.M % MG_BM == 0 && a.N % bn == 0 && a.K % MG_KC == 0 && (reinterpret_cast<uintptr_t>(a.W) & 15) == 0;
    const size_t lds = (size_t)(MG_BM + bn) * MG_LD * sizeof(double);
    const dim3 grid((a.M + MG_BM - 1) / MG_BM, (a.N + bn - 1) / bn);
    auto go = [&](auto kern, std::atomic<unsigned long long>& done) -> int {
        if (int rc = mdgat_lds_optin(reinterpret_cast<const void*>(kern), lds, done, "mlp forward LDS")) return rc;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a);
        return MDGAT_OK;
    };
    if (wn == 4) return fast ? go(mg_gemm_bn_kernel<4, true>, d4f) : go(mg_gemm_bn_kernel<4, false>, d4);
    return fast ? go(mg_gemm_bn_kernel<2, true>, d2f) : go(mg_gemm_bn_kernel<2, false>, d2);
}

}  // namespace

size_t mlp_f64_saved_bytes(const mdgat_mlp_desc& d) { return mg_carve_saved(nullptr, d).bytes; }
size_t mlp_f64_backward_workspace_bytes(const mdgat_mlp_desc& d) { return mg_carve_ws(nullptr, d).bytes; }

int launch_mlp_forward_f64(const mdgat_mlp_desc& d, const double* x0, const double* x1, double* out, void* saved, hipStream_t s) {
    if (d.R <= 0) return MDGAT_OK;
    const MgSaved sv = mg_carve_saved(saved, d);
    const int R = d.R;
    for (int l = 0; l < d.n_conv; ++l) {
        const int N = d.C[l], K = mg_cin(d, l);
        double* dst = l + 1 == d.n_conv ? out : sv.Y[l];
        if (l == 0) {
            const GemmF64Args g{x0, d.K0, d.K0, d.K1 > 0 ? x1 : nullptr, d.K1, d.W[0], K, d.bias[0], nullptr, 0, dst, N, R, N, K, 0, nullptr};
            if (int rc = launch_gemm_f64(g, s)) return rc;
        } else {
            const double* S = sv.S[l - 1];
            const MgGemmArgs g{sv.Y[l - 1], K, S, S + 2 * K, d.beta[l - 1], d.W[l], d.bias[l], dst, R, N};
            if (int rc = mg_launch_gemm_bn(g, s)) return rc;
        }
        if (l + 1 == d.n_conv) break;
        if (d.training) {
            const MgStatArgs st{dst, R, N, sv.P};
            hipLaunchKernelGGL(mg_stats_kernel, dim3((unsigned)mg_slabs(R, MG_SLAB), (unsigned)((N + 63) / 64)), dim3(256), 0, s, st);
        }
        const MgStatFinalArgs fin{sv.P, R, N, d.training, d.eps[l], d.momentum[l], d.gamma[l], d.running_mean[l], d.running_var[l],
                                  reinterpret_cast<long long*>(d.num_batches_tracked[l]), sv.S[l]};
        hipLaunchKernelGGL(mg_stats_final_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, fin);
    }
    return mdgat_check_hip(hipGetLastError(), "mlp forward launch");
}

int launch_mlp_backward_f64(const mdgat_mlp_desc& d, const double* x0, const double* x1, const void* saved, const double* dout,
                            const mdgat_mlp_grads& g, void* workspace, hipStream_t s) {
    if (d.R <= 0) return MDGAT_OK;
    const MgSaved sv = mg_carve_saved(const_cast<void*>(saved), d);
    const MgWs ws = mg_carve_ws(workspace, d);
    const int R = d.R, L = d.n_conv;
    // below[l]: a gradient is wanted that needs dA_{l-1} = dY_l W_l (the inputs', a lower convolution's, a lower BN's)
    bool below[MDGAT_MLP_MAX_CONVS];
    bool any = g.dx0 || (d.K1 > 0 && g.dx1);
    for (int l = 0; l < L; ++l) {
        below[l] = any;
        any = any || g.dW[l] || g.dbias[l] || (l + 1 < L && (g.dgamma[l] || g.dbeta[l]));
    }
    const double* dY = dout;
    for (int l = L - 1; l >= 0; --l) {
        const int N = d.C[l], K = mg_cin(d, l);
        if (g.dW[l] || g.dbias[l]) {
            const double* S = l > 0 ? sv.S[l - 1] : nullptr;
            const MgDwArgs a{dY, N, l > 0 ? sv.Y[l - 1] : x0, l > 0 ? K : d.K0, l > 0 ? nullptr : x1, l > 0 ? 0 : d.K1,
                             S, S ? S + 2 * K : nullptr, l > 0 ? d.beta[l - 1] : nullptr, R, ws.Pw, g.dW[l] != nullptr};
            const int slabs = mg_slabs(R, MG_DW_SLAB), waves = ((N + 31) / 32) * ((K + 31) / 32);
            hipLaunchKernelGGL(mg_dw_kernel, dim3((unsigned)slabs, (unsigned)((waves + 3) / 4)), dim3(256), 0, s, a);
            const MgReduceArgs r{ws.Pw, slabs, N * K, N, g.dW[l], g.dbias[l]};
            hipLaunchKernelGGL(mg_reduce_kernel, dim3((unsigned)(((g.dW[l] ? N * K : 0) + N + 255) / 256)), dim3(256), 0, s, r);
        }
        if (!below[l]) break;
        hipLaunchKernelGGL(mg_transpose_kernel, dim3((unsigned)((N * K + 255) / 256)), dim3(256), 0, s, d.W[l], ws.Wt, N, K);
        if (l == 0) {              // dA_0 split back into the two sources: the row ranges [0, K0) and [K0, K) of the transposed weight
            if (g.dx0) {
                const GemmF64Args p{dY, N, N, nullptr, 0, ws.Wt, N, nullptr, nullptr, 0, g.dx0, d.K0, R, d.K0, N, 0, nullptr};
                if (int rc = launch_gemm_f64(p, s)) return rc;
            }
            if (d.K1 > 0 && g.dx1) {
                const GemmF64Args p{dY, N, N, nullptr, 0, ws.Wt + (size_t)d.K0 * N, N, nullptr, nullptr, 0, g.dx1, d.K1, R, d.K1, N, 0, nullptr};
                if (int rc = launch_gemm_f64(p, s)) return rc;
            }
            break;
        }
        double* buf = ws.G[(L - 1 - l) & 1];
        const GemmF64Args p{dY, N, N, nullptr, 0, ws.Wt, N, nullptr, nullptr, 0, buf, K, R, K, N, 0, nullptr};
        if (int rc = launch_gemm_f64(p, s)) return rc;
        const MgBnBwdArgs b{buf, sv.Y[l - 1], sv.S[l - 1], d.beta[l - 1], R, K, d.training, ws.Pb, ws.Q, g.dgamma[l - 1], g.dbeta[l - 1]};
        const unsigned ct = (unsigned)((K + 63) / 64);
        if (d.training || b.dgamma || b.dbeta) {          // (eval mode: dY = a dz needs neither sum)
            hipLaunchKernelGGL(mg_bnbwd_partial_kernel, dim3((unsigned)mg_slabs(R, MG_SLAB), ct), dim3(256), 0, s, b);
            hipLaunchKernelGGL(mg_bnbwd_final_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, b);
        }
        if (!(g.dW[l - 1] || g.dbias[l - 1] || below[l - 1])) break;       // only this BN's own gradients were wanted
        hipLaunchKernelGGL(mg_bnbwd_apply_kernel, dim3((unsigned)((R + 63) / 64), ct), dim3(256), 0, s, b);
        dY = buf;
    }
    return mdgat_check_hip(hipGetLastError(), "mlp backward launch");
}
