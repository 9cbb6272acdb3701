// The pooled descriptor encoder (descriptor = 'FPFH_gloabal', mdgat.py:156-174) in fp64: what it needs beside the products of f64.hip.
//
//   frame_max_f64_kernel        g[unit][c] = max over the unit's rows of e[row][c], and (optionally) the row that holds it.  A unit is one
//                               frame of one pair; its rows are the frame's OWN keypoints - with the count vectors of a ragged batch the
//                               rows at or beyond a pair's count are not read (they hold denc(0), a finite non-zero vector).  One
//                               workgroup per (unit, 32 channels): 8 row phases x 32 channels, every thread walks the rows phase, phase + 8,
//                               ... keeping (value, row); the 8 phases are combined through LDS in phase order.  A value replaces the
//                               running one only when it is LARGER, and of two equal values the lower row stays: the result is the
//                               maximum whatever the order (no value atomics, nothing depends on the batch a pair travels in), the row
//                               is the first that holds it.  A NaN wins against every number, as in torch.max (the first NaN's row): the
//                               training op hands it on like the MLP kernels around it; in the forward the product in front of this
//                               kernel has raised the range guard by then.
//   add_rows_relu_f64_kernel    hid[row][c] = max(hid[row][c] + add[unit(row)][c], 0): the pooled half of encoder2.0, formed ONCE per (pair,
//                               frame) as a 2B-row product, reaches the R rows of the keypoint half here; the range guard is tested on
//                               the sum before the ReLU, as the product epilogues test theirs.
//   frame_max_backward_kernel   de[b][row][c] = row == idx[b][c] ? dg[b][c] : 0 - the indices are the forward's, never decided again; one
//                               writer per element, no atomics.
#include "common.hpp"
#include "f64.hpp"
#include "f64_dev.hpp"
#include "pool_f64.hpp"

namespace {

constexpr int P_CH = 32, P_PH = 8;       // channels and row phases of a workgroup (256 threads)

// does (v, row r) replace (best, row at)?  Larger wins, NaN wins against numbers, of equals the lower row.
__device__ __forceinline__ bool pool_better(double v, int r, double best, int at) {
    const bool vn = v != v, bn = best != best;
    if (vn || bn) return vn && (!bn || r < at);
    return v > best || (v == best && r < at);
}

__global__ __launch_bounds__(256) void frame_max_f64_kernel(FrameMaxArgs a) {
    __shared__ double sv[P_PH][P_CH];
    __shared__ int si[P_PH][P_CH];
    const int unit = blockIdx.x, c = blockIdx.y * P_CH + (threadIdx.x & (P_CH - 1)), ph = threadIdx.x / P_CH;
    int b = unit, f = 0;
    if (a.M > 0) { b = unit >> 1; f = unit & 1; }
    int n = f ? a.M : a.N;
    if (a.cnt0) n = f ? a.cnt1[b] : a.cnt0[b];
    n = n < 0 ? 0 : (n > (f ? a.M : a.N) ? (f ? a.M : a.N) : n);      // (checked on the host; never beyond the slot)
    const double* e = a.e + ((size_t)b * (a.N + a.M) + (f ? a.N : 0)) * 128 + c;
    double best = -__builtin_inf();
    int at = 0;
    for (int r = ph; r < n; r += P_PH) {
        const double v = e[(size_t)r * 128];
        if (pool_better(v, r, best, at)) { best = v; at = r; }
    }
    sv[ph][threadIdx.x & (P_CH - 1)] = best;
    si[ph][threadIdx.x & (P_CH - 1)] = at;
    __syncthreads();
    if (ph == 0) {
        const int l = threadIdx.x;
        for (int p = 1; p < P_PH; ++p) {
            const double v = sv[p][l];
            const int r = si[p][l];
            if (pool_better(v, r, best, at)) { best = v; at = r; }
        }
        a.g[(size_t)unit * 128 + c] = best;
        if (a.idx) a.idx[(size_t)unit * 128 + c] = at;
    }
}

__global__ __launch_bounds__(256) void add_rows_relu_f64_kernel(double* hid, const double* add, int C, size_t total, int N, int M, unsigned* guard) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / C;
    const int c = (int)(i - row * C);
    const size_t b = row / (size_t)(N + M);
    const int f = (int)(row - b * (N + M)) >= N;
    const double v = hid[i] + add[(2 * b + f) * C + c];
    if (f64_out_of_range(v)) f64_raise(guard);
    hid[i] = v > 0.0 ? v : 0.0;
}

__global__ __launch_bounds__(256) void frame_max_backward_kernel(const double* dg, const int64_t* idx, double* de, int n, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i & 127);
    const size_t row = i >> 7, b = row / n;
    const int r = (int)(row - b * n);
    de[i] = idx[b * 128 + c] == r ? dg[b * 128 + c] : 0.0;
}

}  // namespace

int launch_frame_max_f64(const FrameMaxArgs& a, hipStream_t s) {
    const int units = a.M > 0 ? 2 * a.B : a.B;
    if (units <= 0) return MDGAT_OK;
    hipLaunchKernelGGL(frame_max_f64_kernel, dim3(units, 128 / P_CH), dim3(256), 0, s, a);
    return mdgat_check_hip(hipGetLastError(), "frame_max_f64_kernel");
}

int launch_add_rows_relu_f64(double* hid, const double* add, int C, int B, int N, int M, unsigned* guard, hipStream_t s) {
    const size_t total = (size_t)B * (N + M) * C;
    if (!total) return MDGAT_OK;
    hipLaunchKernelGGL(add_rows_relu_f64_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, hid, add, C, total, N, M, guard);
    return mdgat_check_hip(hipGetLastError(), "add_rows_relu_f64_kernel");
}

int launch_frame_max_backward_f64(int B, int n, const double* dg, const int64_t* idx, double* de, hipStream_t s) {
    const size_t total = (size_t)B * n * 128;
    if (!total) return MDGAT_OK;
    hipLaunchKernelGGL(frame_max_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, dg, idx, de, n, total);
    return mdgat_check_hip(hipGetLastError(), "frame_max_backward_kernel");
}
