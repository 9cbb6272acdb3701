// Evaluation losses of MDGAT.forward (models/mdgat.py:486-594) on a materialised Z [B][N+1][M+1]: superglue, triplet_loss and
// gap_loss, every value in fp64 whatever the precision of Z.
//
// triplet / gap: one pass over Z.  A workgroup takes LOSS_TR rows of one pair and every column: its threads walk the columns (a
// row of a pair is m+1 elements, so rows are not 16-byte aligned: scalar loads, coalesced across the workgroup) and keep the
// tile's LOSS_TR row accumulators in registers and one column accumulator per column visited.  The row accumulators are reduced
// across the workgroup at the end and turned into the row's term; the column partials go to a slab [B][tiles][M].  A second
// kernel, one workgroup per pair, combines the slab in tile order, adds the column terms to the row terms in a fixed order and
// writes the pair's loss.  No atomics on values: a pair's loss does not depend on the batch it travels in.
// superglue reads 2n+m values per pair: the second kernel alone.
//
// gap's column half is not a reduction over the columns of Z.  The reference (mdgat.py:576-587) boolean-masks Z[:, :m]: the m
// positives Z[gt1(j), j] in ROW-MAJOR order form a vector P, the n m other entries in row-major order an n x m matrix V, and term
// c pairs P[c] with column c of V.  Row i of Z contributes its m - a_i non-positives (a_i: the columns whose positive lies in row
// i) to V's row-major sequence from position i m - A_i on (A_i = a_0 + ... + a_{i-1}), so the entry of rank k among them lands in
// column (k - A_i) mod m of V.  A per-pair prologue (loss_gap_order_kernel) sorts the columns by (positive's row, column) - P in
// order and, per row, its positive columns - and the tile kernel's column pass takes for each column c of V and each row of its
// tile the one entry of that row that lands there.
//
// t(z) = -log(exp(z)) is what the reference applies (mdgat.py:541-542, 569-570, 585-586): -z up to rounding where exp(z) is a
// normal number, but exp(z) is subnormal below -708.4 and 0 below -745.1 (t = +inf), so it is computed literally there.
#include <math.h>

#include "common.hpp"
#include "loss.hpp"

namespace {

// (the tile shape, t(z), clamp and the gt index rule: loss.hpp, shared with the gradient's dense pass)
__device__ inline double clamp0(double x) { return loss_clamp0(x); }
__device__ inline int gt_index(int64_t g, int dust) { return loss_gt_index(g, dust); }
size_t tiles_of(int N) { return loss_tiles_of(N); }

// the workspace: rowterm [B][N] | slab [B][tiles][M] | gap: tpos [B][M] (t of P) | cols [B][M] (the columns in P's order) | A [B][N+2]
// | the gradient's statistics pass (grad): rowaux [B][N] | slabaux [B][tiles][M]
using LossWs = LossStats;
LossWs carve_loss(void* base, int B, int N, int M, bool grad = false) {
    LossWs w{};
    WsCarver c{static_cast<char*>(base)};
    c.take(w.rowterm, (size_t)B * N);
    c.take(w.slab, (size_t)B * tiles_of(N) * M);
    c.take(w.tpos, (size_t)B * M);
    c.take(w.cols, (size_t)B * M);
    c.take(w.A, (size_t)B * (N + 2));
    if (grad) {
        c.take(w.rowaux, (size_t)B * N);
        c.take(w.slabaux, (size_t)B * tiles_of(N) * M);
    }
    w.tiles = (int)tiles_of(N);
    w.total = c.bytes;
    return w;
}

// the rank-th (0-based) column of a row that is not one of its a positive columns pos[0] < ... < pos[a-1]: rank + #{t : pos[t] - t <= rank}
__device__ inline int nth_other(const int* pos, int a, int rank) {
    int lo = 0, hi = a;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pos[mid] - mid <= rank) lo = mid + 1;
        else hi = mid;
    }
    return rank + lo;
}

// gap, one workgroup per pair: A[i] = number of positives in rows < i (i = 0 .. N + 1), cols = the M columns stably sorted by their
// positive's row, tpos[k] = t(Z[row][cols[k]]) (P).  Deterministic: counts through LDS integer atomics, ranks by comparison.
template <typename T>
__global__ __launch_bounds__(LOSS_THREADS) void loss_gap_order_kernel(const T* __restrict__ Z, const int64_t* __restrict__ gt1, int N, int M,
                                                                     int* __restrict__ A_out, int* __restrict__ cols, double* __restrict__ tpos) {
    extern __shared__ int h[];                  // [N + 2]
    __shared__ int keys[LOSS_THREADS];
    __shared__ int part[LOSS_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t ld = (size_t)M + 1;
    const T* Zb = Z + (size_t)b * (N + 1) * ld;
    const int64_t* g = gt1 + (size_t)b * M;
    auto row_of = [&](int j) { const int p = gt_index(g[j], N); return p < 0 ? N : p; };    // (a bad index: the pair's loss is NaN anyway)
    for (int i = tid; i < N + 2; i += LOSS_THREADS) h[i] = 0;
    __syncthreads();
    for (int j = tid; j < M; j += LOSS_THREADS) atomicAdd(&h[row_of(j) + 1], 1);
    __syncthreads();
    // inclusive scan of h[0 .. N+1] (h[0] = 0): thread chunks, then the chunk sums
    const int per = (N + 2 + LOSS_THREADS - 1) / LOSS_THREADS;
    const int lo = tid * per, hi = min(lo + per, N + 2);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += h[i];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0)
        for (int k = 1; k < LOSS_THREADS; ++k) part[k] += part[k - 1];
    __syncthreads();
    int run = tid ? part[tid - 1] : 0;
    for (int i = lo; i < hi; ++i) { run += h[i]; h[i] = run; }
    __syncthreads();
    for (int i = tid; i < N + 2; i += LOSS_THREADS) A_out[(size_t)b * (N + 2) + i] = h[i];
    __syncthreads();
    // stable ranks, 256 columns at a time; h[r] is the next free slot of row r
    for (int base = 0; base < M; base += LOSS_THREADS) {
        const int j = base + tid;
        const int key = j < M ? row_of(j) : -1;
        keys[tid] = key;
        __syncthreads();
        int before = 0, same = 0;
        for (int t = 0; t < LOSS_THREADS; ++t) {
            const bool eq = keys[t] == key;
            before += eq && t < tid;
            same += eq;
        }
        int slot = 0;
        if (key >= 0) slot = h[key] + before;
        __syncthreads();
        if (key >= 0) {
            if (before + 1 == same) h[key] += same;         // the key's last column in this chunk advances it
            cols[(size_t)b * M + slot] = j;
            const int p = gt_index(g[j], N);
            tpos[(size_t)b * M + slot] = p >= 0 ? loss_t((double)Zb[p * ld + j]) : __builtin_nan("");
        }
        __syncthreads();
    }
}

// sum (or max) over the workgroup in a fixed order: lanes by a butterfly, then the four waves in order
template <bool MAX>
__device__ inline double block_reduce(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o, 64);
        v = MAX ? fmax(v, w) : v + w;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
    for (int k = 1; k < LOSS_THREADS / 64; ++k) r = MAX ? fmax(r, red[k]) : r + red[k];
    return r;
}

// GAP: row i accumulates sum_{j != pos} clamp(t(pos) - t(Z[i][j]) + gamma, 0) over the m+1 columns, column j the same over the
// n+1 rows.  Else (triplet): row i the max of Z[i][j] over j != pos, column j the max over i != pos (the hard negative of topk(2)).
// GRAD (the gradient's statistics pass, launch_loss_stats): the same walk, leaving the raw records of LossStats in place of the terms -
// the sums with their active counts (a clamp argument >= 0 is active, as torch.clamp's backward has it), the maxima with their
// index.  Ties take the LOWEST index, the rule of every arg-max of this library (torch.topk leaves the choice open).  GRAD = false is
// the forward as it always was.
template <typename T, bool GAP, bool GRAD>
__global__ __launch_bounds__(LOSS_THREADS) void loss_tile_kernel(const T* __restrict__ Z, const int64_t* __restrict__ gt0,
                                                                const int64_t* __restrict__ gt1, int N, int M, int tiles, double gamma,
                                                                double* __restrict__ rowterm, double* __restrict__ slab,
                                                                const double* __restrict__ tpos, const int* __restrict__ cols,
                                                                const int* __restrict__ Arows, int* __restrict__ rowaux,
                                                                int* __restrict__ slabaux) {
    __shared__ int s_pc[LOSS_TR];
    __shared__ int s_A[LOSS_TR + 1];
    __shared__ double s_tp[LOSS_TR];
    __shared__ double red[LOSS_THREADS / 64][LOSS_TR];
    __shared__ int redaux[GRAD ? LOSS_THREADS / 64 : 1][LOSS_TR];
    const int b = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int i0 = tile * LOSS_TR;
    const size_t ld = (size_t)M + 1;
    const T* Zb = Z + (size_t)b * (N + 1) * ld;
    if (threadIdx.x < LOSS_TR) {
        const int i = i0 + threadIdx.x;
        int p = -1;
        double tp = 0.0;
        if (i < N) {
            p = gt_index(gt0[(size_t)b * N + i], M);
            tp = p >= 0 ? loss_t((double)Zb[i * ld + p]) : __builtin_nan("");
        }
        s_pc[threadIdx.x] = p;
        s_tp[threadIdx.x] = tp;
    }
    if (GAP && threadIdx.x <= LOSS_TR) s_A[threadIdx.x] = Arows[(size_t)b * (N + 2) + min(i0 + (int)threadIdx.x, N + 1)];
    __syncthreads();
    int pc[LOSS_TR];
    double tp[LOSS_TR], acc[LOSS_TR];
    int aux[GRAD ? LOSS_TR : 1];            // GRAD: the row's active count (gap) / the column of its maximum, -1 = none yet (triplet)
#pragma unroll
    for (int r = 0; r < LOSS_TR; ++r) {
        pc[r] = s_pc[r];
        tp[r] = s_tp[r];
        acc[r] = GAP ? 0.0 : -INFINITY;
        if (GRAD) aux[r] = GAP ? 0 : -1;
    }
    const int rows = N + 1 - i0 < LOSS_TR ? N + 1 - i0 : LOSS_TR;     // rows of Z in this tile (row N: the dustbin row)
    for (int j = threadIdx.x; j <= M; j += LOSS_THREADS) {
        const int prow = !GAP && j < M ? gt_index(gt1[(size_t)b * M + j], N) : -1;
        double z[LOSS_TR];
#pragma unroll
        for (int r = 0; r < LOSS_TR; ++r) z[r] = r < rows ? (double)Zb[(i0 + r) * ld + j] : 0.0;
        double c = -INFINITY;
        int ci = -1;
#pragma unroll
        for (int r = 0; r < LOSS_TR; ++r) {
            const int i = i0 + r;
            const bool row_term = i < N && j != pc[r];                  // (i < N: also false past the tile's last row)
            if (GAP) {
                if (row_term) {
                    const double x = tp[r] - loss_t(z[r]) + gamma;
                    acc[r] += clamp0(x);
                    if (GRAD) aux[r] += x >= 0.0;
                }
            } else if (GRAD) {
                // strict >: a thread's columns (and a tile's rows) come in increasing order, so the first of equals stays
                if (row_term && (aux[r] < 0 || z[r] > acc[r])) { acc[r] = z[r]; aux[r] = j; }
                if (r < rows && j < M && i != prow && (ci < 0 || z[r] > c)) { c = z[r]; ci = i; }
            } else {
                if (row_term) acc[r] = fmax(acc[r], z[r]);
                if (r < rows && j < M && i != prow) c = fmax(c, z[r]);
            }
        }
        if (!GAP && j < M) {
            slab[((size_t)b * tiles + tile) * M + j] = c;
            if (GRAD) slabaux[((size_t)b * tiles + tile) * M + j] = ci;
        }
    }
    if (GAP) {
        // column c of V: from each row i of the tile the entry of rank (c + A_i) mod m among the row's non-positives, if it has one
        const int* pcols = cols + (size_t)b * M;
        for (int c = threadIdx.x; c < M; c += LOSS_THREADS) {
            const double tq = tpos[(size_t)b * M + c];
            double z[LOSS_TR];
            bool has[LOSS_TR];
#pragma unroll
            for (int r = 0; r < LOSS_TR; ++r) {         // (all loads first, then the sum in row order)
                const int Ai = s_A[r], a = s_A[r + 1] - Ai;
                const int rank = c + Ai >= M ? c + Ai - M : c + Ai;
                has[r] = r < rows && rank < M - a;
                const int j = a ? nth_other(pcols + Ai, a, rank) : rank;
                z[r] = has[r] ? (double)Zb[(i0 + r) * ld + j] : 0.0;
            }
            double v = 0.0;
            int active = 0;
#pragma unroll
            for (int r = 0; r < LOSS_TR; ++r)
                if (has[r]) {
                    const double x = tq - loss_t(z[r]) + gamma;
                    v += clamp0(x);
                    if (GRAD) active += x >= 0.0;
                }
            slab[((size_t)b * tiles + tile) * M + c] = v;
            if (GRAD) slabaux[((size_t)b * tiles + tile) * M + c] = active;
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < LOSS_TR; ++r) {
        double v = acc[r];
        int a = GRAD ? aux[r] : 0;
        for (int o = 32; o > 0; o >>= 1) {
            const double w = __shfl_xor(v, o, 64);
            if (GRAD) {
                const int wa = __shfl_xor(a, o, 64);
                if (GAP) { v += w; a += wa; }
                else if (wa >= 0 && (a < 0 || w > v || (w == v && wa < a))) { v = w; a = wa; }
            } else {
                v = GAP ? v + w : fmax(v, w);
            }
        }
        if (lane == 0) {
            red[wv][r] = v;
            if (GRAD) redaux[wv][r] = a;
        }
    }
    __syncthreads();
    if (threadIdx.x < LOSS_TR && i0 + (int)threadIdx.x < N) {
        const int r = threadIdx.x;
        double v = red[0][r];
        if (GRAD) {
            int a = redaux[0][r];
            for (int k = 1; k < LOSS_THREADS / 64; ++k) {
                const double w = red[k][r];
                const int wa = redaux[k][r];
                if (GAP) { v += w; a += wa; }
                else if (wa >= 0 && (a < 0 || w > v || (w == v && wa < a))) { v = w; a = wa; }
            }
            // gap: S_i and its active count; triplet: the clamp argument and the negative's column
            rowterm[(size_t)b * N + i0 + r] = GAP ? v : s_tp[r] - loss_t(v) + gamma;
            rowaux[(size_t)b * N + i0 + r] = a;
            return;
        }
        for (int k = 1; k < LOSS_THREADS / 64; ++k) v = GAP ? v + red[k][r] : fmax(v, red[k][r]);
        // gap: 2 log(sum + 1) (mdgat.py:572); triplet: clamp(t(pos) - t(neg) + gamma, 0) (543-545)
        rowterm[(size_t)b * N + i0 + r] = GAP ? 2.0 * log(v + 1.0) : clamp0(s_tp[r] - loss_t(v) + gamma);
    }
}

// One workgroup per pair: the column terms from the slab, the row terms, the pair's loss.  superglue (mdgat.py:487-511) from Z alone.
template <typename T>
__global__ __launch_bounds__(LOSS_THREADS) void loss_pair_kernel(const T* __restrict__ Z, const int64_t* __restrict__ gt0,
                                                                const int64_t* __restrict__ gt1, int N, int M, int tiles, int method,
                                                                double gamma, const double* __restrict__ rowterm,
                                                                const double* __restrict__ slab, double* __restrict__ loss,
                                                                unsigned* bad_index) {
    __shared__ double red[LOSS_THREADS / 64];
    const int b = blockIdx.x;
    const size_t ld = (size_t)M + 1;
    const T* Zb = Z + (size_t)b * (N + 1) * ld;
    double rs = 0.0, cs = 0.0, unmatched = 0.0, bad = 0.0;
    for (int i = threadIdx.x; i < N; i += LOSS_THREADS) {
        const int p = gt_index(gt0[(size_t)b * N + i], M);
        if (p < 0) bad = 1.0;
        if (method == MDGAT_LOSS_SUPERGLUE) rs += p >= 0 ? (double)Zb[i * ld + p] : 0.0;
        else rs += rowterm[(size_t)b * N + i];
    }
    for (int j = threadIdx.x; j < M; j += LOSS_THREADS) {
        const int64_t g = gt1[(size_t)b * M + j];
        if (method == MDGAT_LOSS_SUPERGLUE) {
            // only a literal -1 counts as unmatched; the reference reads gt1 through `== -1` alone
            if (g == -1) { cs += (double)Zb[N * ld + j]; unmatched += 1.0; }
            continue;
        }
        const int prow = gt_index(g, N);
        if (prow < 0) bad = 1.0;
        const double* col = slab + (size_t)b * tiles * M + j;
        if (method == MDGAT_LOSS_GAP) {
            double s = 0.0;
#pragma unroll 8
            for (int t = 0; t < tiles; ++t) s += col[(size_t)t * M];
            cs += 2.0 * log(s + 1.0);
        } else {
            double mx = -INFINITY;
#pragma unroll 8
            for (int t = 0; t < tiles; ++t) mx = fmax(mx, col[(size_t)t * M]);
            const double tq = prow >= 0 ? loss_t((double)Zb[prow * ld + j]) : 0.0;
            cs += clamp0(tq - loss_t(mx) + gamma);
        }
    }
    rs = block_reduce<false>(rs, red);
    cs = block_reduce<false>(cs, red);
    unmatched = block_reduce<false>(unmatched, red);
    bad = block_reduce<true>(bad, red);
    if (threadIdx.x == 0) {
        double v;
        if (method == MDGAT_LOSS_SUPERGLUE) v = (-rs - cs) / (unmatched + M);
        else if (method == MDGAT_LOSS_GAP) v = (rs / N + cs / M) / 2.0;
        else v = (rs + cs) / (double)(N + M);
        if (bad != 0.0) {
            v = __builtin_nan("");
            if (bad_index) atomicOr(bad_index, 1u);
        }
        loss[b] = v;
    }
}

}  // namespace

size_t loss_workspace_bytes(int B, int N, int M) {
    if (B <= 0 || N <= 0 || M <= 0) return 0;
    return carve_loss(nullptr, B, N, M).total;
}

template <typename T>
int launch_loss(int B, int N, int M, const T* Z, const int64_t* gt0, const int64_t* gt1, int method, double gamma, double* loss,
                unsigned* bad_index, void* workspace, size_t workspace_bytes, hipStream_t s) {
    if (!Z || !gt0 || !gt1 || !loss) { mdgat_set_error("mdgat_loss: null pointer"); return MDGAT_ERR_BAD_ARG; }
    if (B <= 0 || N <= 0 || M <= 0) { mdgat_set_error("mdgat_loss: empty batch / frame (B=%d N=%d M=%d)", B, N, M); return MDGAT_ERR_BAD_ARG; }
    if (method != MDGAT_LOSS_SUPERGLUE && method != MDGAT_LOSS_TRIPLET && method != MDGAT_LOSS_GAP) {
        mdgat_set_error("mdgat_loss: bad method %d", method);
        return MDGAT_ERR_BAD_ARG;
    }
    if (method != MDGAT_LOSS_GAP && N != M) {
        mdgat_set_error("mdgat_loss: the superglue and triplet losses need N == M (N=%d M=%d), as the reference's do", N, M);
        return MDGAT_ERR_BAD_ARG;
    }
    const size_t need = loss_workspace_bytes(B, N, M);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 255)) {
        mdgat_set_error("mdgat_loss: workspace %zu < %zu bytes or not 256-byte aligned", workspace_bytes, need);
        return MDGAT_ERR_BAD_ARG;
    }
    if (method == MDGAT_LOSS_GAP && N > LOSS_GAP_MAX_ROWS) {
        mdgat_set_error("mdgat_loss: gap_loss is implemented for N <= %d (N=%d)", LOSS_GAP_MAX_ROWS, N);
        return MDGAT_ERR_UNSUPPORTED;
    }
    const int tiles = (int)tiles_of(N);
    const LossWs w = carve_loss(workspace, B, N, M);
    double *rowterm = w.rowterm, *slab = w.slab;
    if (method == MDGAT_LOSS_GAP) {
        hipLaunchKernelGGL((loss_gap_order_kernel<T>), dim3(B), dim3(LOSS_THREADS), (N + 2) * sizeof(int), s, Z, gt1, N, M, w.A, w.cols, w.tpos);
        if (int rc = mdgat_check_hip(hipGetLastError(), "loss_gap_order_kernel")) return rc;
        hipLaunchKernelGGL((loss_tile_kernel<T, true, false>), dim3((unsigned)B * tiles), dim3(LOSS_THREADS), 0, s, Z, gt0, gt1, N, M, tiles, gamma,
                           rowterm, slab, w.tpos, w.cols, w.A, (int*)nullptr, (int*)nullptr);
    } else if (method == MDGAT_LOSS_TRIPLET) {
        hipLaunchKernelGGL((loss_tile_kernel<T, false, false>), dim3((unsigned)B * tiles), dim3(LOSS_THREADS), 0, s, Z, gt0, gt1, N, M, tiles, gamma,
                           rowterm, slab, w.tpos, w.cols, w.A, (int*)nullptr, (int*)nullptr);
    }
    if (method != MDGAT_LOSS_SUPERGLUE)
        if (int rc = mdgat_check_hip(hipGetLastError(), "loss_tile_kernel")) return rc;
    hipLaunchKernelGGL((loss_pair_kernel<T>), dim3(B), dim3(LOSS_THREADS), 0, s, Z, gt0, gt1, N, M, tiles, method, gamma, rowterm, slab, loss,
                       bad_index);
    return mdgat_check_hip(hipGetLastError(), "loss_pair_kernel");
}

template int launch_loss<float>(int, int, int, const float*, const int64_t*, const int64_t*, int, double, double*, unsigned*, void*, size_t,
                                hipStream_t);
template int launch_loss<double>(int, int, int, const double*, const int64_t*, const int64_t*, int, double, double*, unsigned*, void*, size_t,
                                 hipStream_t);

LossStats loss_stats_carve(void* base, int B, int N, int M) { return carve_loss(base, B, N, M, true); }

// the caller (launch_loss_backward) has checked the arguments
template <typename T>
int launch_loss_stats(int B, int N, int M, const T* Z, const int64_t* gt0, const int64_t* gt1, int method, double gamma, const LossStats& w,
                      hipStream_t s) {
    const int tiles = w.tiles;
    if (method == MDGAT_LOSS_GAP) {
        hipLaunchKernelGGL((loss_gap_order_kernel<T>), dim3(B), dim3(LOSS_THREADS), (N + 2) * sizeof(int), s, Z, gt1, N, M, w.A, w.cols, w.tpos);
        if (int rc = mdgat_check_hip(hipGetLastError(), "loss_gap_order_kernel")) return rc;
        hipLaunchKernelGGL((loss_tile_kernel<T, true, true>), dim3((unsigned)B * tiles), dim3(LOSS_THREADS), 0, s, Z, gt0, gt1, N, M, tiles, gamma,
                           w.rowterm, w.slab, w.tpos, w.cols, w.A, w.rowaux, w.slabaux);
    } else {
        hipLaunchKernelGGL((loss_tile_kernel<T, false, true>), dim3((unsigned)B * tiles), dim3(LOSS_THREADS), 0, s, Z, gt0, gt1, N, M, tiles, gamma,
                           w.rowterm, w.slab, w.tpos, w.cols, w.A, w.rowaux, w.slabaux);
    }
    return mdgat_check_hip(hipGetLastError(), "loss_tile_kernel (statistics)");
}

template int launch_loss_stats<float>(int, int, int, const float*, const int64_t*, const int64_t*, int, double, const LossStats&, hipStream_t);
template int launch_loss_stats<double>(int, int, int, const double*, const int64_t*, const int64_t*, int, double, const LossStats&, hipStream_t);

extern "C" size_t mdgat_loss_workspace_bytes(int B, int N, int M) { return loss_workspace_bytes(B, N, M); }

extern "C" int mdgat_loss(int B, int N, int M, const float* Z, const int64_t* gt0, const int64_t* gt1, int method, double gamma, double* loss,
                          unsigned* bad_index, void* workspace, size_t workspace_bytes, void* stream) {
    return launch_loss(B, N, M, Z, gt0, gt1, method, gamma, loss, bad_index, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int mdgat_loss_f64(int B, int N, int M, const double* Z, const int64_t* gt0, const int64_t* gt1, int method, double gamma,
                              double* loss, unsigned* bad_index, void* workspace, size_t workspace_bytes, void* stream) {
    return launch_loss(B, N, M, Z, gt0, gt1, method, gamma, loss, bad_index, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}
