// Backward of log_optimal_transport (mdgat.py:279-308) in fp64: dZ -> d scores, d bin score, for fp64 scores of N, M <= 2175.
//
// The math (tests/sinkhorn_grad_ref.py restates it in torch).  C is the (N+1) x (M+1) coupling matrix, K = exp(C - row maximum),
// and the forward's scaling vectors are a_t = mu / (K b_{t-1}), b_t = nu / (K^T a_t) from b_0 = 1 - the av / bvec of the streaming
// form (sinkhorn_f64.hip).  With G = dZ, d = rowsum(G) and gv_T = colsum(G), the reverse iterations t = T .. 1 run
//      y_t = b_t gv_t / nu;   gu_t = [t == T] d - a_t (K y_t);   x_t = a_t gu_t / mu;   gv_{t-1} = - b_{t-1} (K^T x_t)   (t > 1)
// and the gradient of the couplings is the rank-2T correction   dC = G - K o (X^T Y),   X = [x_t; a_t]_t  [2T][N+1],
// Y = [b_{t-1}; y_t]_t  [2T][M+1].  d scores = dC[:N, :M]; d bin score = the sum of dC over the dustbin row and column.
//
// gfx950 mapping, per call:
//   1. the streaming forward's init / iteration launches with the history written through (sinkhorn_f64_stream_history): a_t into the
//      odd rows of X, b_{t-1} into the even rows of Y - the history IS half of the GEMM's operands; K and b_T stay in the workspace;
//   2. skg_rows_kernel / skg_cols0_kernel: d, and y_T into Y's last row;
//   3. per reverse step one streaming pass over K shaped as sinkhorn_f64_wide_iter_kernel (skg_reverse_kernel: workgroup = pair x
//      slab of 32 rows, a wave a row at a time: the row dot with y, gu and x of the row, then K_ij x_i into the wave's column partials,
//      the eight waves' partials through LDS out as the slab's), and skg_cols_kernel: the slabs' partials summed in slab order into
//      gv_{t-1} and y_{t-1}.  No workgroup waits for another and no value atomics, so the bits do not depend on the batch;
//   4. skg_coupling_kernel: dC = G - K o (X^T Y) on v_mfma_f64_16x16x4_f64, fragments straight from L2 (the operands of a pair are
//      2T x (N+1+M+1) doubles), 64 x 64 tiles of four waves; the epilogue writes d scores and keeps the dustbin row / column of dC;
//   5. skg_dalpha_kernel: per pair their sum, one wave in a fixed order.
#include "common.hpp"
#include "f64_dev.hpp"
#include "sinkhorn_f64.hpp"

namespace {

constexpr int SKG_ROWS = 32;                                           // rows per slab (as the streaming forward)
constexpr int SKG_NMAX = 2175;                                         // the streaming forward's limit

struct SkgArgs {
    int B, N, M, Mp, Np, G, T, t;
    const double* K;          // [B][N][Mp]
    const double* bT;         // [B][Mp]: b_T
    const double* dZ;         // [B][N + 1][M + 1]
    double* X;                // [B][2T][Np]: rows 2(t-1): x_t, 2(t-1)+1: a_t
    double* Y;                // [B][2T][Mp]: rows 2(t-1): b_{t-1}, 2(t-1)+1: y_t
    double* P;                // [B][G][Mp]: column partials of a reverse step, per slab
    double* d;                // [B][N + 1]: rowsum(dZ)
    double* drow;             // [B][M + 1]: the dustbin row of dC
    double* dcol;             // [B][N]: the dustbin column of dC (rows < N)
    double* dscores;          // [B][N][M]
    double* dbin;             // [B]
};

__device__ __forceinline__ double skg_wave_sum(double v) {      // butterfly: the same bits in every lane
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// d_i = sum_j dZ_ij, one wave per row (N + 1 rows)
__global__ __launch_bounds__(512) void skg_rows_kernel(SkgArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per = (a.N + 1 + 7) / 8;
    const int pair = blockIdx.x / per, i = (blockIdx.x % per) * 8 + wave;
    if (i > a.N) return;
    const double* g = a.dZ + ((size_t)pair * (a.N + 1) + i) * (a.M + 1);
    double s = 0.0;
    for (int j = lane; j <= a.M; j += 64) s += g[j];
    s = skg_wave_sum(s);
    if (lane == 0) a.d[(size_t)pair * (a.N + 1) + i] = s;
}

// y_T = b_T gv_T / nu with gv_T = colsum(dZ), one thread per column (rows in order); zero in the padding
__global__ __launch_bounds__(128) void skg_cols0_kernel(SkgArgs a) {
    const int per = a.Mp >> 7;
    const int pair = blockIdx.x / per, j = (blockIdx.x % per) * 128 + threadIdx.x;
    const double nm = (double)(a.N + a.M);
    double y = 0.0;
    if (j <= a.M) {
        const double* g = a.dZ + (size_t)pair * (a.N + 1) * (a.M + 1) + j;
        double s = 0.0;
        for (int i = 0; i <= a.N; ++i) s += g[(size_t)i * (a.M + 1)];
        y = a.bT[(size_t)pair * a.Mp + j] * s * (j < a.M ? nm : nm / a.N);
    }
    a.Y[((size_t)pair * 2 * a.T + 2 * (a.T - 1) + 1) * a.Mp + j] = y;
}

typedef double skg_x2 __attribute__((ext_vector_type(2)));

// reverse step t: gu_t and x_t of every row from the row dot K y_t, and the slab's partials of K^T x_t (sinkhorn_f64_wide_iter_kernel's
// shape: y -> LDS, a wave a row at a time with the next row's K in flight, 16-byte loads, the waves' partials summed through LDS)
template <int NC2>
__global__ __launch_bounds__(512) void skg_reverse_kernel(SkgArgs a) {
    extern __shared__ __attribute__((aligned(16))) double skg_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.N, M = a.M, Mp = a.Mp, G = a.G;
    const int nc2 = Mp >> 7;
    double* yl = skg_lds;                          // [Mp]
    double* colbuf = skg_lds + Mp;                 // [8][Mp]
    const int pair = blockIdx.x / G, g = blockIdx.x % G;
    const double nm = (double)(N + M);
    const bool first = a.t == a.T;
    const double* at = a.X + ((size_t)pair * 2 * a.T + 2 * (a.t - 1) + 1) * a.Np;
    double* xt = a.X + ((size_t)pair * 2 * a.T + 2 * (a.t - 1)) * a.Np;
    const double* yt = a.Y + ((size_t)pair * 2 * a.T + 2 * (a.t - 1) + 1) * Mp;
    const double* dv = a.d + (size_t)pair * (N + 1);
    for (int j = 2 * tid; j < Mp; j += 1024) *reinterpret_cast<skg_x2*>(yl + j) = *reinterpret_cast<const skg_x2*>(yt + j);
    double acc[2 * NC2];
#pragma unroll
    for (int c = 0; c < 2 * NC2; ++c) acc[c] = 0.0;
    const int rbeg = g * SKG_ROWS, rend = rbeg + SKG_ROWS < N ? rbeg + SKG_ROWS : N;
    const double* kbase = a.K + (size_t)pair * N * Mp + 2 * lane;
    auto fetch = [&](skg_x2 (&kv)[NC2], int row) {
        const double* k = kbase + (size_t)row * Mp;
#pragma unroll
        for (int c = 0; c < NC2; ++c) kv[c] = (c < nc2 && row < rend) ? *reinterpret_cast<const skg_x2*>(k + 128 * c) : skg_x2{0.0, 0.0};
    };
    auto work = [&](const skg_x2 (&kv)[NC2], int row) {
        double p = 0.0;
#pragma unroll
        for (int c = 0; c < NC2; ++c)
            if (c < nc2) {
                const skg_x2 yy = *reinterpret_cast<const skg_x2*>(yl + 128 * c + 2 * lane);
                p = __builtin_fma(kv[c].x, yy.x, p);
                p = __builtin_fma(kv[c].y, yy.y, p);
            }
        const double ai = at[row];
        const double gu = (first ? dv[row] : 0.0) - ai * skg_wave_sum(p);
        const double xi = ai * gu * nm;                                  // / mu_i
        if (lane == 0) xt[row] = xi;
#pragma unroll
        for (int c = 0; c < NC2; ++c) {
            acc[2 * c] = __builtin_fma(kv[c].x, xi, acc[2 * c]);
            acc[2 * c + 1] = __builtin_fma(kv[c].y, xi, acc[2 * c + 1]);
        }
    };
    skg_x2 ka[NC2], kb[NC2];
    fetch(ka, rbeg + wave);
    __syncthreads();
    // the dustbin row (K = 1): every wave forms its x the same way, the last slab adds it to the columns it covers (j <= M)
    double sy = 0.0;
    for (int j = lane; j <= M; j += 64) sy += yl[j];
    const double aN = at[N];
    const double xN = aN * ((first ? dv[N] : 0.0) - aN * skg_wave_sum(sy)) * (nm / M);
    for (int row = rbeg + wave; row < rend; row += 16) {
        fetch(kb, row + 8);
        work(ka, row);
        if (row + 8 < rend) {
            fetch(ka, row + 16);
            work(kb, row + 8);
        }
    }
#pragma unroll
    for (int c = 0; c < NC2; ++c)
        if (c < nc2) *reinterpret_cast<skg_x2*>(colbuf + (size_t)wave * Mp + 128 * c + 2 * lane) = skg_x2{acc[2 * c], acc[2 * c + 1]};
    __syncthreads();
    const bool last = g == G - 1;
    double* mine = a.P + ((size_t)pair * G + g) * Mp;
    for (int j = tid; j < Mp; j += 512) {
        double p = colbuf[j];
#pragma unroll
        for (int w = 1; w < 8; ++w) p += colbuf[(size_t)w * Mp + j];
        if (last && j <= M) p += xN;
        mine[j] = p;
    }
    if (last && tid == 0) xt[N] = xN;
}

// gv_{t-1} = - b_{t-1} (sum of the slabs' partials, in slab order) and y_{t-1} = b_{t-1} gv_{t-1} / nu; zero in the padding
__global__ __launch_bounds__(128) void skg_cols_kernel(SkgArgs a) {
    const int per = a.Mp >> 7;
    const int pair = blockIdx.x / per, j = (blockIdx.x % per) * 128 + threadIdx.x;
    const double nm = (double)(a.N + a.M);
    double y = 0.0;
    if (j <= a.M) {
        const double* Pp = a.P + (size_t)pair * a.G * a.Mp + j;
        double s = Pp[0];
        for (int q = 1; q < a.G; ++q) s += Pp[(size_t)q * a.Mp];
        const double b = a.Y[((size_t)pair * 2 * a.T + 2 * (a.t - 1)) * a.Mp + j];        // b_{t-1}
        y = -b * s * b * (j < a.M ? nm : nm / a.N);
    }
    a.Y[((size_t)pair * 2 * a.T + 2 * (a.t - 2) + 1) * a.Mp + j] = y;
}

// dC = G - K o (X^T Y) for a 64 x 64 tile of a pair's (N + 1) x (M + 1) couplings: four waves of 32 x 32, each four 16 x 16 MFMA
// accumulators over k = 0 .. 2T - 1 (fragments loaded from L2; rows beyond N of X and columns beyond M of Y are read - both lie
// inside the padded arrays - and not stored).  Epilogue: d scores, and the dustbin row / column of dC for skg_dalpha_kernel.
__global__ __launch_bounds__(256) void skg_coupling_kernel(SkgArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = a.N, M = a.M, KT = 2 * a.T;
    const int tc = (M + 1 + 63) / 64, tr = (N + 1 + 63) / 64;
    const int pair = blockIdx.x / (tr * tc), rem = blockIdx.x % (tr * tc);
    const int i0 = (rem / tc) * 64 + 32 * (wave >> 1), j0 = (rem % tc) * 64 + 32 * (wave & 1);
    const double* Xp = a.X + (size_t)pair * KT * a.Np + i0 + (lane & 15);
    const double* Yp = a.Y + (size_t)pair * KT * a.Mp + j0 + (lane & 15);
    f64x4 acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[r][c] = f64x4{0.0, 0.0, 0.0, 0.0};
    auto step = [&](int k0, bool in) {
        const int k = k0 + (lane >> 4);
        const double x0 = in ? Xp[(size_t)k * a.Np] : 0.0, x1 = in ? Xp[(size_t)k * a.Np + 16] : 0.0;
        const double y0 = in ? Yp[(size_t)k * a.Mp] : 0.0, y1 = in ? Yp[(size_t)k * a.Mp + 16] : 0.0;
        acc[0][0] = mfma64(x0, y0, acc[0][0]);
        acc[0][1] = mfma64(x0, y1, acc[0][1]);
        acc[1][0] = mfma64(x1, y0, acc[1][0]);
        acc[1][1] = mfma64(x1, y1, acc[1][1]);
    };
    int k0 = 0;
    for (; k0 + 4 <= KT; k0 += 4) step(k0, true);
    if (k0 < KT) step(k0, k0 + (lane >> 4) < KT);                     // 2T = 2 mod 4: the last two k
    const double* Gp = a.dZ + (size_t)pair * (N + 1) * (M + 1);
    const double* Kp = a.K + (size_t)pair * N * a.Mp;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = i0 + 16 * r + (lane >> 4) + 4 * q, j = j0 + 16 * c + (lane & 15);
                if (i > N || j > M) continue;
                const double kij = i < N ? Kp[(size_t)i * a.Mp + j] : 1.0;
                const double dc = Gp[(size_t)i * (M + 1) + j] - kij * acc[r][c][q];
                if (i < N && j < M) a.dscores[((size_t)pair * N + i) * M + j] = dc;
                else if (i == N) a.drow[(size_t)pair * (M + 1) + j] = dc;
                else a.dcol[(size_t)pair * N + i] = dc;
            }
}

// d bin score of a pair: its dustbin row and column of dC summed by one wave in a fixed order
__global__ __launch_bounds__(64) void skg_dalpha_kernel(SkgArgs a) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    double s = 0.0;
    for (int j = lane; j <= a.M; j += 64) s += a.drow[(size_t)pair * (a.M + 1) + j];
    for (int i = lane; i < a.N; i += 64) s += a.dcol[(size_t)pair * a.N + i];
    s = skg_wave_sum(s);
    if (lane == 0) a.dbin[pair] = s;
}

// the workspace: the streaming forward's, then X, Y, d, the dustbin row / column (a null base: its size only)
struct SkgWs { Sk64Stream fw; double *X, *Y, *d, *drow, *dcol; int Np; size_t bytes; };
SkgWs skg_carve(void* base, int B, int N, int M, int T) {
    SkgWs w{};
    w.fw = sinkhorn_f64_stream_carve(base, B, N, M);
    w.Np = (N + 1 + 63) & ~63;
    WsCarver c{base ? static_cast<char*>(base) + w.fw.bytes : nullptr};
    c.take(w.X, (size_t)B * 2 * T * w.Np); c.take(w.Y, (size_t)B * 2 * T * w.fw.Mp);
    c.take(w.d, (size_t)B * (N + 1)); c.take(w.drow, (size_t)B * (M + 1)); c.take(w.dcol, (size_t)B * N);
    w.bytes = w.fw.bytes + c.bytes;
    return w;
}

template <int NC2>
int skg_reverse_launches(SkgArgs a, hipStream_t s) {
    const size_t lds = (size_t)9 * a.Mp * sizeof(double);
    static std::atomic<unsigned long long> optin{0};
    if (int rc = mdgat_lds_optin(reinterpret_cast<const void*>(skg_reverse_kernel<NC2>), lds, optin, "sinkhorn backward LDS")) return rc;
    for (int t = a.T; t >= 1; --t) {
        a.t = t;
        hipLaunchKernelGGL(skg_reverse_kernel<NC2>, dim3((unsigned)(a.B * a.G)), dim3(512), lds, s, a);
        if (t > 1) hipLaunchKernelGGL(skg_cols_kernel, dim3((unsigned)(a.B * (a.Mp >> 7))), dim3(128), 0, s, a);
    }
    return mdgat_check_hip(hipGetLastError(), "sinkhorn backward (reverse) launch");
}

}  // namespace

extern "C" size_t mdgat_sinkhorn_backward_workspace_bytes(int B, int N, int M, int iters) {
    if (B <= 0 || N <= 0 || M <= 0 || N > SKG_NMAX || M > SKG_NMAX || iters < 0) return 0;
    return skg_carve(nullptr, B, N, M, iters).bytes;
}

extern "C" int mdgat_sinkhorn_backward(int B, int N, int M, const double* scores, double bin_score, int iters, const double* dZ, double* dscores,
                                       double* dbin, void* workspace, size_t workspace_bytes, void* stream) {
    if (B < 0 || N <= 0 || M <= 0 || iters < 0) { mdgat_set_error("mdgat_sinkhorn_backward: bad shape B=%d N=%d M=%d iters=%d", B, N, M, iters); return MDGAT_ERR_BAD_ARG; }
    if (N > SKG_NMAX || M > SKG_NMAX) { mdgat_set_error("mdgat_sinkhorn_backward: %d x %d keypoints > %d supported", N, M, SKG_NMAX); return MDGAT_ERR_UNSUPPORTED; }
    if (B == 0) return MDGAT_OK;
    if (!scores || !dZ || !dscores || !dbin) { mdgat_set_error("mdgat_sinkhorn_backward: null pointer"); return MDGAT_ERR_BAD_ARG; }
    const SkgWs w = skg_carve(workspace, B, N, M, iters);
    if (!workspace || workspace_bytes < w.bytes || (reinterpret_cast<uintptr_t>(workspace) & 255)) {
        mdgat_set_error("mdgat_sinkhorn_backward: workspace too small or not 256-byte aligned");
        return MDGAT_ERR_BAD_ARG;
    }
    const hipStream_t s = static_cast<hipStream_t>(stream);
    Sk64Call fw{};
    fw.B = B; fw.N = N; fw.M = M; fw.scores = scores; fw.alpha = bin_score; fw.iters = iters;
    if (int rc = sinkhorn_f64_stream_history(fw, w.X, w.Np, w.Y, workspace, s)) return rc;
    SkgArgs a{};
    a.B = B; a.N = N; a.M = M; a.Mp = w.fw.Mp; a.Np = w.Np; a.G = w.fw.G; a.T = iters;
    a.K = w.fw.K; a.bT = w.fw.bvec; a.dZ = dZ; a.X = w.X; a.Y = w.Y; a.P = w.fw.P; a.d = w.d; a.drow = w.drow; a.dcol = w.dcol;
    a.dscores = dscores; a.dbin = dbin;
    if (iters > 0) {
        hipLaunchKernelGGL(skg_rows_kernel, dim3((unsigned)(B * ((N + 1 + 7) / 8))), dim3(512), 0, s, a);
        hipLaunchKernelGGL(skg_cols0_kernel, dim3((unsigned)(B * (a.Mp >> 7))), dim3(128), 0, s, a);
        const int nc2 = a.Mp >> 7;
        if (int rc = nc2 <= 5 ? skg_reverse_launches<5>(a, s) : nc2 <= 9 ? skg_reverse_launches<9>(a, s) : skg_reverse_launches<17>(a, s)) return rc;
    }
    const int tiles = ((N + 1 + 63) / 64) * ((M + 1 + 63) / 64);
    hipLaunchKernelGGL(skg_coupling_kernel, dim3((unsigned)(B * tiles)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(skg_dalpha_kernel, dim3((unsigned)B), dim3(64), 0, s, a);
    return mdgat_check_hip(hipGetLastError(), "sinkhorn backward launch");
}
