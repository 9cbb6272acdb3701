// Gradient of MDGAT's losses (models/mdgat.py:486-594; values: loss.hip) with respect to Z [B][N+1][M+1]: what autograd takes
// through the reference's loss code, given one upstream weight dloss[b] per pair.  fp64 whatever the precision of Z.
//
// Three passes, no atomics on values and one writer per entry of dZ, so a pair's gradient is bitwise the same alone, in any batch
// and whatever the other pairs carry:
//   1. statistics (loss.hip, launch_loss_stats): the forward's tile kernel - and gap's ordering prologue - leaving raw records:
//      triplet the hard negative's index per row / per tile and column, gap the sums S with their active counts;
//   2. loss_grad_pair_kernel, one workgroup per pair: the tiles' column records combined in tile order, the weights of the row and
//      column terms (roww / colw), the inverse of gap's column order (cpos), superglue's count of unmatched columns, the bad flag;
//   3. loss_grad_dense_kernel, one thread per entry of dZ in memory order (rows are m+1 elements and not 16-byte aligned: the flat
//      index keeps loads and stores coalesced across row ends): the entry's contribution in its row's terms plus the one in its
//      column's terms, written once.
//
// Conventions (those of torch autograd on the reference's code):
//   * torch.clamp(x, min=0) passes the gradient where x >= 0: a term that is exactly 0 is active; NaN is not.
//   * t(z) = -log(exp(z)) is differentiated literally: with e = exp(z) a gradient g on t becomes (-g / e) * e on z.  That is -g to an
//     ulp where e is normal, -+inf where 1 / e overflows, NaN where e == 0 (below about -745.1) even for g == 0.  Not repaired: the
//     loss itself is +inf or garbage at such entries.  In gap every entry of Z[:n] / Z[:, :m] goes through t, in triplet only the
//     positives and the hard negatives do (the others are exactly 0).
//   * gap applies t to the positive AFTER repeating it against its m (n) partners: its gradient is the sum of the partners'
//     (-g / e) * e, i.e. count x (-w / e) * e for count > 0 active partners and (-0 / e) * e for none.
//   * Arg-max ties in triplet: torch.topk leaves the choice open; the LOWEST index is taken, as everywhere in this library.
//   * gap's column half follows the reference's row-major P / V pairing (loss.hip): entry (i, j) of Z[:, :m] that is not a positive
//     has rank k among its row's non-positives and lands in column (k - A_i) mod m of V - the forward's arithmetic, inverted.
#include <math.h>

#include "common.hpp"
#include "loss.hpp"

namespace {

// the workspace: the statistics pass's records, then roww [B][N] | colw [B][M] | colaux [B][M] | cpos [B][M] | pairw [B] | pairbad [B]
struct LossGradWs {
    LossStats st;
    double *roww, *colw, *pairw;
    int *colaux, *cpos, *pairbad;
    size_t total;
};
LossGradWs carve_loss_grad(void* base, int B, int N, int M) {
    LossGradWs w{};
    w.st = loss_stats_carve(base, B, N, M);
    WsCarver c{static_cast<char*>(base)};
    c.bytes = w.st.total;
    c.take(w.roww, (size_t)B * N);
    c.take(w.colw, (size_t)B * M);
    c.take(w.pairw, (size_t)B);
    c.take(w.colaux, (size_t)B * M);
    c.take(w.cpos, (size_t)B * M);
    c.take(w.pairbad, (size_t)B);
    w.total = c.bytes;
    return w;
}

// d t(z) / d z applied to a gradient g on t, literally as autograd does (e = exp(z))
__device__ inline double dt_dz(double g, double e) { return (-g / e) * e; }

// One workgroup per pair.  Row records -> roww; the tiles' column records combined in tile order -> colw / colaux:
//   triplet  roww[i] / colw[j] = the term's weight g / (n + m) if it is active, else 0; colaux[j] = the column's negative row;
//   gap      roww[i] = g / (n (S_i + 1)), colw[c] = g / (m (S_c + 1)), colaux[c] = column c of V's active count, cpos[j] = the place of
//            column j in P's order;
//   superglue pairw = -g / (xx + m).
template <typename T>
__global__ __launch_bounds__(LOSS_THREADS) void loss_grad_pair_kernel(const T* __restrict__ Z, const int64_t* __restrict__ gt0,
                                                                     const int64_t* __restrict__ gt1, int N, int M, int tiles, int method,
                                                                     double gamma, const double* __restrict__ dloss,
                                                                     const double* __restrict__ rowterm, const double* __restrict__ slab,
                                                                     const int* __restrict__ slabaux, const double* __restrict__ tpos,
                                                                     const int* __restrict__ cols, double* __restrict__ roww,
                                                                     double* __restrict__ colw, int* __restrict__ colaux,
                                                                     int* __restrict__ cpos, double* __restrict__ pairw,
                                                                     int* __restrict__ pairbad, unsigned* bad_word) {
    __shared__ int s_bad, s_xx;
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t ld = (size_t)M + 1;
    const T* Zb = Z + (size_t)b * (N + 1) * ld;
    const double g = dloss[b];
    if (tid == 0) { s_bad = 0; s_xx = 0; }
    __syncthreads();
    int bad = 0, xx = 0;
    for (int i = tid; i < N; i += LOSS_THREADS) {
        if (loss_gt_index(gt0[(size_t)b * N + i], M) < 0) bad = 1;
        if (method == MDGAT_LOSS_TRIPLET) roww[(size_t)b * N + i] = rowterm[(size_t)b * N + i] >= 0.0 ? g / (double)(N + M) : 0.0;
        if (method == MDGAT_LOSS_GAP) roww[(size_t)b * N + i] = g / ((double)N * (rowterm[(size_t)b * N + i] + 1.0));
    }
    for (int j = tid; j < M; j += LOSS_THREADS) {
        const int64_t gj = gt1[(size_t)b * M + j];
        if (method == MDGAT_LOSS_SUPERGLUE) {
            xx += gj == -1;                 // only a literal -1 counts; the reference reads gt1 through `== -1` alone
            continue;
        }
        const int prow = loss_gt_index(gj, N);
        if (prow < 0) bad = 1;
        const double* col = slab + (size_t)b * tiles * M + j;
        const int* colx = slabaux + (size_t)b * tiles * M + j;
        if (method == MDGAT_LOSS_GAP) {     // (j is a column c of V here)
            double s = 0.0;
            int active = 0;
#pragma unroll 8
            for (int t = 0; t < tiles; ++t) { s += col[(size_t)t * M]; active += colx[(size_t)t * M]; }
            colw[(size_t)b * M + j] = g / ((double)M * (s + 1.0));
            colaux[(size_t)b * M + j] = active;
            cpos[(size_t)b * M + cols[(size_t)b * M + j]] = j;          // cols is a permutation of the columns: one writer each
        } else {
            double mx = -INFINITY;
            int arg = -1;
            for (int t = 0; t < tiles; ++t) {                           // tiles in row order, strict >: the lowest row of equals
                const double v = col[(size_t)t * M];
                const int a = colx[(size_t)t * M];
                if (a >= 0 && (arg < 0 || v > mx)) { mx = v; arg = a; }
            }
            const double tq = prow >= 0 ? loss_t((double)Zb[prow * ld + j]) : 0.0;
            colw[(size_t)b * M + j] = tq - loss_t(mx) + gamma >= 0.0 ? g / (double)(N + M) : 0.0;
            colaux[(size_t)b * M + j] = arg;
        }
    }
    if (bad) atomicOr(&s_bad, 1);
    if (xx) atomicAdd(&s_xx, xx);
    __syncthreads();
    if (tid == 0) {
        pairw[b] = -g / ((double)s_xx + (double)M);
        pairbad[b] = s_bad;
        if (s_bad && bad_word) atomicOr(bad_word, 1u);
    }
}

template <typename T, int METHOD>
__global__ __launch_bounds__(LOSS_THREADS) void loss_grad_dense_kernel(const T* __restrict__ Z, const int64_t* __restrict__ gt0,
                                                                      const int64_t* __restrict__ gt1, int N, int M, unsigned per_pair,
                                                                      double gamma, const double* __restrict__ roww,
                                                                      const int* __restrict__ rowaux, const double* __restrict__ colw,
                                                                      const int* __restrict__ colaux, const int* __restrict__ cpos,
                                                                      const double* __restrict__ tpos, const int* __restrict__ cols,
                                                                      const int* __restrict__ Arows, const double* __restrict__ pairw,
                                                                      const int* __restrict__ pairbad, double* __restrict__ dZ) {
    const unsigned b = blockIdx.x / per_pair;
    const unsigned ld = (unsigned)M + 1, entries = (unsigned)(N + 1) * ld;
    const unsigned idx = (blockIdx.x - b * per_pair) * LOSS_THREADS + threadIdx.x;
    if (idx >= entries) return;
    const T* Zb = Z + (size_t)b * entries;
    double* out = dZ + (size_t)b * entries + idx;
    if (pairbad[b]) { *out = __builtin_nan(""); return; }      // (before anything is indexed by a gt value)
    const int i = (int)(idx / ld), j = (int)(idx - (unsigned)i * ld);
    double v = 0.0;
    if (METHOD == MDGAT_LOSS_SUPERGLUE) {
        if (i < N ? loss_gt_index(gt0[(size_t)b * N + i], M) == j : (j < M && gt1[(size_t)b * M + j] == -1)) v = pairw[b];
        *out = v;
        return;
    }
    const double z = (double)Zb[idx];
    if (METHOD == MDGAT_LOSS_TRIPLET) {
        // only the positives and the hard negatives pass through t
        const int p0 = i < N ? loss_gt_index(gt0[(size_t)b * N + i], M) : -1;
        const int n0 = i < N ? rowaux[(size_t)b * N + i] : -1;
        const int p1 = j < M ? loss_gt_index(gt1[(size_t)b * M + j], N) : -1;
        const int n1 = j < M ? colaux[(size_t)b * M + j] : -1;
        if (j == p0 || j == n0 || i == p1 || i == n1) {
            const double e = exp(z);
            if (j == p0) v += dt_dz(roww[(size_t)b * N + i], e);
            if (j == n0) v += dt_dz(-roww[(size_t)b * N + i], e);
            if (i == p1) v += dt_dz(colw[(size_t)b * M + j], e);
            if (i == n1) v += dt_dz(-colw[(size_t)b * M + j], e);
        }
        *out = v;
        return;
    }
    // gap
    const double e = exp(z), tz = loss_t(z);
    if (i < N) {
        const int p0 = loss_gt_index(gt0[(size_t)b * N + i], M);
        const double w = roww[(size_t)b * N + i];
        if (j == p0) {
            const int active = rowaux[(size_t)b * N + i];
            v += active > 0 ? (double)active * dt_dz(w, e) : dt_dz(0.0, e);
        } else {
            const double x = loss_t((double)Zb[(unsigned)i * ld + p0]) - tz + gamma;
            v += dt_dz(x >= 0.0 ? -w : 0.0, e);
        }
    }
    if (j < M) {
        const int p1 = loss_gt_index(gt1[(size_t)b * M + j], N);
        if (i == p1) {
            const int c = cpos[(size_t)b * M + j];
            const int active = colaux[(size_t)b * M + c];
            v += active > 0 ? (double)active * dt_dz(colw[(size_t)b * M + c], e) : dt_dz(0.0, e);
        } else {
            // rank of column j among row i's non-positives: j minus the row's positive columns below j (cols: ascending within a row)
            const int Ai = Arows[(size_t)b * (N + 2) + i], a = Arows[(size_t)b * (N + 2) + i + 1] - Ai;
            const int* pos = cols + (size_t)b * M + Ai;
            int lo = 0, hi = a;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (pos[mid] < j) lo = mid + 1;
                else hi = mid;
            }
            int c = j - lo - Ai;
            if (c < 0) c += M;
            const double x = tpos[(size_t)b * M + c] - tz + gamma;
            v += dt_dz(x >= 0.0 ? -colw[(size_t)b * M + c] : 0.0, e);
        }
    }
    *out = v;
}

template <typename T>
int launch_loss_backward(int B, int N, int M, const T* Z, const int64_t* gt0, const int64_t* gt1, int method, double gamma, const double* dloss,
                         double* dZ, int32_t* bad, void* workspace, size_t workspace_bytes, hipStream_t s) {
    if (!Z || !gt0 || !gt1 || !dloss || !dZ) { mdgat_set_error("mdgat_loss_backward: null pointer"); return MDGAT_ERR_BAD_ARG; }
    if (B <= 0 || N <= 0 || M <= 0) { mdgat_set_error("mdgat_loss_backward: empty batch / frame (B=%d N=%d M=%d)", B, N, M); return MDGAT_ERR_BAD_ARG; }
    if (method != MDGAT_LOSS_SUPERGLUE && method != MDGAT_LOSS_TRIPLET && method != MDGAT_LOSS_GAP) {
        mdgat_set_error("mdgat_loss_backward: bad method %d", method);
        return MDGAT_ERR_BAD_ARG;
    }
    if (method != MDGAT_LOSS_GAP && N != M) {
        mdgat_set_error("mdgat_loss_backward: the superglue and triplet losses need N == M (N=%d M=%d), as the reference's do", N, M);
        return MDGAT_ERR_BAD_ARG;
    }
    const LossGradWs w = carve_loss_grad(workspace, B, N, M);
    if (!workspace || workspace_bytes < w.total || (reinterpret_cast<uintptr_t>(workspace) & 255)) {
        mdgat_set_error("mdgat_loss_backward: workspace %zu < %zu bytes or not 256-byte aligned", workspace_bytes, w.total);
        return MDGAT_ERR_BAD_ARG;
    }
    if (method == MDGAT_LOSS_GAP && N > LOSS_GAP_MAX_ROWS) {
        mdgat_set_error("mdgat_loss_backward: gap_loss is implemented for N <= %d (N=%d)", LOSS_GAP_MAX_ROWS, N);
        return MDGAT_ERR_UNSUPPORTED;
    }
    // the dense pass indexes a pair's entries and the grid's workgroups with 32 bits
    const unsigned long long entries = (unsigned long long)(N + 1) * (unsigned long long)(M + 1);
    const unsigned long long per_pair = (entries + LOSS_THREADS - 1) / LOSS_THREADS;
    if (entries >= (1ull << 31) || per_pair * (unsigned long long)B >= (1ull << 31)) {
        mdgat_set_error("mdgat_loss_backward: B (N+1) (M+1) = %d x %llu entries of dZ exceed the dense pass's 32-bit grid", B, entries);
        return MDGAT_ERR_UNSUPPORTED;
    }
    if (method != MDGAT_LOSS_SUPERGLUE)
        if (int rc = launch_loss_stats(B, N, M, Z, gt0, gt1, method, gamma, w.st, s)) return rc;
    hipLaunchKernelGGL((loss_grad_pair_kernel<T>), dim3(B), dim3(LOSS_THREADS), 0, s, Z, gt0, gt1, N, M, w.st.tiles, method, gamma, dloss,
                       w.st.rowterm, w.st.slab, w.st.slabaux, w.st.tpos, w.st.cols, w.roww, w.colw, w.colaux, w.cpos, w.pairw, w.pairbad,
                       reinterpret_cast<unsigned*>(bad));
    if (int rc = mdgat_check_hip(hipGetLastError(), "loss_grad_pair_kernel")) return rc;
    const dim3 grid((unsigned)(per_pair * B)), block(LOSS_THREADS);
#define LOSS_GRAD_DENSE(METHOD)                                                                                                            \
    hipLaunchKernelGGL((loss_grad_dense_kernel<T, METHOD>), grid, block, 0, s, Z, gt0, gt1, N, M, (unsigned)per_pair, gamma, w.roww,       \
                       w.st.rowaux, w.colw, w.colaux, w.cpos, w.st.tpos, w.st.cols, w.st.A, w.pairw, w.pairbad, dZ)
    if (method == MDGAT_LOSS_SUPERGLUE) LOSS_GRAD_DENSE(MDGAT_LOSS_SUPERGLUE);
    else if (method == MDGAT_LOSS_TRIPLET) LOSS_GRAD_DENSE(MDGAT_LOSS_TRIPLET);
    else LOSS_GRAD_DENSE(MDGAT_LOSS_GAP);
#undef LOSS_GRAD_DENSE
    return mdgat_check_hip(hipGetLastError(), "loss_grad_dense_kernel");
}

}  // namespace

extern "C" size_t mdgat_loss_backward_workspace_bytes(int B, int N, int M) {
    if (B <= 0 || N <= 0 || M <= 0) return 0;
    return carve_loss_grad(nullptr, B, N, M).total;
}

extern "C" int mdgat_loss_backward(int B, int N, int M, const float* Z, const int64_t* gt0, const int64_t* gt1, int method, double gamma,
                                   const double* dloss, double* dZ, int32_t* bad, void* workspace, size_t workspace_bytes, void* stream) {
    return launch_loss_backward(B, N, M, Z, gt0, gt1, method, gamma, dloss, dZ, bad, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int mdgat_loss_backward_f64(int B, int N, int M, const double* Z, const int64_t* gt0, const int64_t* gt1, int method, double gamma,
                                       const double* dloss, double* dZ, int32_t* bad, void* workspace, size_t workspace_bytes, void* stream) {
    return launch_loss_backward(B, N, M, Z, gt0, gt1, method, gamma, dloss, dZ, bad, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}
