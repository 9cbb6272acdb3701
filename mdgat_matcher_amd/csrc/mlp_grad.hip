// The reference's MLP(channels) (mdgat.py:34-46) in TRAINING mode and its backward, in fp64: Conv1d(k=1), and after every convolution
// but the last BatchNorm1d on the batch's own statistics and ReLU.  The inference forward folds BN into the weights (pack.py); a
// training step cannot: the statistics are taken over all R = B P rows of the call, the gradient runs through them, and the running
// buffers move.  tests/mlp_grad_ref.py restates all of it in numpy.
//
// Rows are points: x0 [R][K0] | x1 [R][K1] side by side (GemmF64Args::A0 / A1: the layer's cat([x, message]) is never built), W_l
// [C_l][C_in] as in the state_dict, out [R][C_L].  Per convolution l:
//      Y_l = A_{l-1} W_l^T + b_l;   mean_c, var_c (biased) over the rows;   z = gamma (Y - mean) invstd + beta;   A_l = max(z, 0)
// What is kept for the backward is Y_l of every BN layer and mean / invstd / a = gamma invstd per channel.  A_l is NEVER stored:
// z = fma(Y - mean, a, beta) is recomputed where the next product loads its A operand (gemm_f64_kernel, f64.hip), where dW loads its B
// operand (dw_f64_kernel, dw_f64.hip) and where the backward masks (mg_bnbwd_*) - the same function everywhere (bn_z / bn_relu,
// f64_dev.hpp), so the sign of z is the same everywhere.  torch keeps the convolution output, the BN output and the ReLU output of
// every layer.
//
// Forward launches.  Every product is the exact mode's launch_gemm_f64: layer 0 with its two sources, the layers behind a BN with
// the operand transform (GemmF64Args::bn_*: the normalisation and the ReLU between the global load and the LDS store); tile width
// and chunk depth are that launcher's.  A NaN in Y: this file honours NaNs, so it stays a NaN through the statistics and reaches
// every value of the layer through mean and a; in the operand of the next product a NaN z counts as 0, under f64.hip's flags as
// under this file's (bn_relu).  Batch statistics: mg_stats_kernel gives
// every slab of 256 rows its column sums and, around the SLAB's mean, the centred sums of squares M2 (two passes over rows that are
// in cache after the first); mg_stats_final_kernel combines the slabs in slab order by Chan's update
//      delta = mean_b - mean;  mean += delta n_b / n;  M2 += M2_b + delta^2 n_a n_b / n
// - never E[y^2] - E[y]^2 - and moves the running buffers (running_var takes the unbiased M2 / (R - 1)).  With training == 0 the
// running statistics stand in and nothing is written to them.
//
// Backward, from the last convolution to the first (dY_L = dout):
//   launch_dw_f64     dW_l = dY_l^T A_{l-1} and db_l = colsum(dY_l) (dw_f64.hip): slabs of 512 rows, ONE chain per element inside a
//                     slab, the B operand A_{l-1} recomputed from Y_{l-1} as it is loaded; the slabs' partials added in slab order.
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

}  // namespace

size_t mlp_f64_saved_bytes(const mdgat_mlp_desc& d) { return mg_carve_saved(nullptr, d).bytes; }
size_t mlp_f64_backward_workspace_bytes(const mdgat_mlp_desc& d) { return mg_carve_ws(nullptr, d).bytes; }

int launch_mlp_forward_f64(const mdgat_mlp_desc& d, const double* x0, const double* x1, double* out, void* saved, hipStream_t s,
                           const double* residual) {
    if (d.R <= 0) return MDGAT_OK;
    const MgSaved sv = mg_carve_saved(saved, d);
    const int R = d.R;
    for (int l = 0; l < d.n_conv; ++l) {
        const int N = d.C[l], K = mg_cin(d, l);
        double* dst = l + 1 == d.n_conv ? out : sv.Y[l];
        GemmF64Args g{x0, d.K0, d.K0, d.K1 > 0 ? x1 : nullptr, d.K1, d.W[l], K, d.bias[l], nullptr, 0, dst, N, R, N, K, 0, nullptr};
        if (l > 0) {               // behind a BN: A = max(z, 0) of the previous convolution's output, formed as the operand is loaded
            g.A0 = sv.Y[l - 1]; g.lda0 = g.K0 = K; g.A1 = nullptr; g.lda1 = 0;
            g.bn_mean = sv.S[l - 1]; g.bn_a = sv.S[l - 1] + 2 * K; g.bn_beta = d.beta[l - 1];
        }
        if (l + 1 == d.n_conv && residual) { g.R = residual; g.ldr = N; }       // out = Y_L + residual, added in the last product's epilogue
        if (int rc = launch_gemm_f64(g, s)) return rc;
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
            // the convolution's input: x0 | x1, or behind a BN A_{l-1} recomputed from Y_{l-1} as it is loaded
            const double* S = l > 0 ? sv.S[l - 1] : nullptr;
            const DwF64Args a{dY, N, l > 0 ? sv.Y[l - 1] : x0, l > 0 ? K : d.K0, l > 0 ? nullptr : x1, l > 0 ? 0 : d.K1,
                              S, S ? S + 2 * K : nullptr, l > 0 ? d.beta[l - 1] : nullptr, R, MG_DW_SLAB, ws.Pw, g.dW[l], g.dbias[l]};
            if (int rc = launch_dw_f64(a, s)) return rc;
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
