// The weight and bias gradients of a Conv1d(k=1) Y = X W^T + b in fp64: dW = dY^T X [Cout][Cin] and db = colsum(dY), on
// v_mfma_f64_16x16x4_f64, and the ordered reduction of per-slab partials that the training-mode MLP (mlp_grad.hip) and the matching
// head (head_grad.hip) share.
//
//   dw_f64_kernel         Both operands are contracted over their ROWS, so both fragments are coalesced loads from L2 and there is no
//                         LDS.  A workgroup: one slab of rows x four 32 x 32 tiles of dW, one per wave, four accumulators each: ONE
//                         chain per output element inside a slab, rows ascending, the ragged tail masked to zeros.  The column
//                         source may be two arrays side by side (x0 | x1) and may stand behind a BatchNorm + ReLU, formed as it is
//                         loaded (bn_relu, f64_dev.hpp).  db rides along: every lane adds up the A fragment values it loads (a
//                         quarter of the rows each), the four quarters are combined as (0 + 1) + (2 + 3) (quad_sum).  When dW is not
//                         wanted only the waves of the first column tile run, and no product is formed.  (hg_dw_kernel of
//                         head_grad.hip is the whole-tile case Cout = Cin = 128 over a pair's two frames, kept for its speed.)
//   dw_reduce_f64_kernel  dW / db = slab 0's partial + slab 1's + ... in slab order.
// No value atomics and no workgroup waits for another: the bits are the same from run to run, and a batch's dW is the sum of its
// slabs' dW in slab order.
#include "common.hpp"
#include "f64.hpp"
#include "f64_dev.hpp"

namespace {

__global__ __launch_bounds__(256) void dw_f64_kernel(DwF64Args p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int Cin = p.K0 + p.K1, Cout = p.Cout;
    const int tn = (Cin + 31) >> 5, tm = (Cout + 31) >> 5;
    const int id = blockIdx.y * 4 + wave;
    if (id >= tm * tn) return;
    const int rt = id / tn, ct = id % tn;
    const bool prod = p.dW != nullptr;
    if (!prod && ct != 0) return;
    const int r0 = blockIdx.x * p.slab, cnt = min(p.slab, p.R - r0);
    // A: row = output channel (l15), k = point (g); Cout is a multiple of 16: the first half of the 32 always exists
    const bool oka1 = rt * 32 + 16 < Cout;
    const double* ap = p.dY + (size_t)(r0 + g) * Cout + rt * 32 + l15;
    // B: k = point, column = input channel
    const double* bp[2] = {nullptr, nullptr};
    int ldb[2] = {0, 0};
    bool okb[2];
    double mu[2] = {0.0, 0.0}, aa[2] = {0.0, 0.0}, be[2] = {0.0, 0.0};
    const bool bn = p.bn_mean != nullptr;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ci = ct * 32 + h * 16 + l15;
        okb[h] = prod && ci < Cin;
        if (!okb[h]) continue;
        const bool first = ci < p.K0;
        ldb[h] = first ? p.K0 : p.K1;
        bp[h] = (first ? p.x0 + ci : p.x1 + (ci - p.K0)) + (size_t)(r0 + g) * ldb[h];
        if (bn) { mu[h] = p.bn_mean[ci]; aa[h] = p.bn_a[ci]; be[h] = p.bn_beta[ci]; }
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

// dW == nullptr: the grid covers db alone
__global__ __launch_bounds__(256) void dw_reduce_f64_kernel(const double* P, int slabs, int nW, int nb, double* dW, double* db) {
    const int idx = blockIdx.x * 256 + threadIdx.x + (dW ? 0 : nW), part = nW + nb;
    if (idx >= part) return;
    double s = P[idx];
    for (int b = 1; b < slabs; ++b) s += P[(size_t)b * part + idx];
    if (idx < nW) dW[idx] = s;
    else if (db) db[idx - nW] = s;
}

}  // namespace

int launch_dw_reduce_f64(const double* P, int slabs, int nW, int nb, double* dW, double* db, hipStream_t s) {
    hipLaunchKernelGGL(dw_reduce_f64_kernel, dim3((unsigned)(((dW ? nW : 0) + nb + 255) / 256)), dim3(256), 0, s, P, slabs, nW, nb, dW, db);
    return mdgat_check_hip(hipGetLastError(), "dw_f64 launch");
}

int launch_dw_f64(const DwF64Args& a, hipStream_t s) {
    if (a.R <= 0 || !(a.dW || a.db)) return MDGAT_OK;
    const int Cin = a.K0 + a.K1, slabs = (a.R + a.slab - 1) / a.slab, waves = ((a.Cout + 31) / 32) * ((Cin + 31) / 32);
    hipLaunchKernelGGL(dw_f64_kernel, dim3((unsigned)slabs, (unsigned)((waves + 3) / 4)), dim3(256), 0, s, a);
    return launch_dw_reduce_f64(a.P, slabs, a.Cout * Cin, a.Cout, a.dW, a.db, s);
}
