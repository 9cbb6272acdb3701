// Device functions of the rigid pose from matches (solve_icp + calculate_error, utils/utils_test.py:41-110), shared by the pose
// kernel (postproc.hip) and the per-pair evaluation record (eval_metrics.hip): one workgroup of 256 threads per pair, fp64.
#pragma once
#include "common.hpp"

namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// workgroup-wide sum of NV doubles per thread -> every thread gets the totals (scratch: [16][NV])
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* scratch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum_d(v[i]);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) scratch[wave * NV + i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double s = 0.0;
        for (int w = 0; w < nw; ++w) s += scratch[w * NV + i];
        v[i] = s;
    }
}

// One-sided Jacobi SVD of a 3x3 matrix (fp64): A = U diag(s) V^T.  Returns R = U V^T, the orthogonal factor
// np.dot(U, Vh) of solve_icp (unique for a non-singular A, reflections included).
__device__ void polar_uvt(const double (&A)[3][3], double (&R)[3][3]) {
    double G[3][3], V[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { G[i][j] = A[i][j]; V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int i = 0; i < 3; ++i) { alpha += G[i][p] * G[i][p]; beta += G[i][q] * G[i][q]; gamma += G[i][p] * G[i][q]; }
                off = fmax(off, fabs(gamma) / (sqrt(alpha * beta) + 1e-300));
                if (fabs(gamma) < 1e-300) continue;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int i = 0; i < 3; ++i) {
                    const double gp = G[i][p], gq = G[i][q];
                    G[i][p] = c * gp - s * gq; G[i][q] = s * gp + c * gq;
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq;
                }
            }
        if (off < 1e-15) break;
    }
    // columns of G are s_j u_j; R = sum_j u_j v_j^T
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = 0.0;
    for (int k = 0; k < 3; ++k) {
        double nrm = 0.0;
        for (int i = 0; i < 3; ++i) nrm += G[i][k] * G[i][k];
        nrm = sqrt(nrm);
        const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;   // singular direction: contributes nothing (degenerate input)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[i][j] += G[i][k] * inv * V[j][k];
    }
}

// One pair's pose, by the whole workgroup (256 threads, every one of them calls this).  k0 [N][3] / k1 [M][3] are the pair's
// keypoints, match(i) the frame-1 partner of frame-0 keypoint i (anything outside [0, M) = unmatched; never used to index then),
// G the pair's T_gt [4][4] or NULL, T [4][4] receives the pose.  scratch [4 * 16] and Rt [12] are LDS.  Thread 0 gets
// st[5] = matches, inliers, inlier ratio, translation error, rotation error (rad; both NaN without G); the others leave st alone.
template <typename MatchFn>
__device__ __forceinline__ void pose_of_pair(const float* k0, const float* k1, MatchFn match, int N, int M, const double* G, double inlier_dist,
                                             double* T, double* scratch, double* Rt, double (&st)[5]) {
    const int tid = threadIdx.x;
    // ---- centroids of the matched points (utils_test.py:89-95): Q = frame-0 points, P = their frame-1 partners ----
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < N; i += 256) {
        const int64_t j = match(i);
        if (j >= 0 && j < M) {
            acc[0] += 1.0;
            for (int c = 0; c < 3; ++c) { acc[1 + c] += (double)k0[i * 3 + c]; acc[4 + c] += (double)k1[j * 3 + c]; }
        }
    }
    {
        double v4[4] = {acc[0], acc[1], acc[2], acc[3]};
        block_sum<4>(v4, scratch);
        acc[0] = v4[0]; acc[1] = v4[1]; acc[2] = v4[2]; acc[3] = v4[3];
        double v3[4] = {acc[4], acc[5], acc[6], 0.0};
        block_sum<4>(v3, scratch);
        acc[4] = v3[0]; acc[5] = v3[1]; acc[6] = v3[2];
    }
    const double n = acc[0];
    const double inv_n = n > 0.0 ? 1.0 / n : 0.0;
    const double uq[3] = {acc[1] * inv_n, acc[2] * inv_n, acc[3] * inv_n};
    const double up[3] = {acc[4] * inv_n, acc[5] * inv_n, acc[6] * inv_n};

    // ---- H = Qc^T Pc (utils_test.py:97) ----
    double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < N; i += 256) {
        const int64_t j = match(i);
        if (j >= 0 && j < M) {
            double q[3], p[3];
            for (int c = 0; c < 3; ++c) { q[c] = (double)k0[i * 3 + c] - uq[c]; p[c] = (double)k1[j * 3 + c] - up[c]; }
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) h[r * 3 + c] += q[r] * p[c];
        }
    }
    {
        double v[4] = {h[0], h[1], h[2], h[3]};
        block_sum<4>(v, scratch); h[0] = v[0]; h[1] = v[1]; h[2] = v[2]; h[3] = v[3];
        double w[4] = {h[4], h[5], h[6], h[7]};
        block_sum<4>(w, scratch); h[4] = w[0]; h[5] = w[1]; h[6] = w[2]; h[7] = w[3];
        double z[4] = {h[8], 0, 0, 0};
        block_sum<4>(z, scratch); h[8] = z[0];
    }
    if (tid == 0) {
        double A[3][3], R[3][3];
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) A[r][c] = h[r * 3 + c];
        polar_uvt(A, R);                                           // R = U V^T (utils_test.py:97-98)
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) Rt[r * 4 + c] = R[r][c];
            Rt[r * 4 + 3] = uq[r] - (R[r][0] * up[0] + R[r][1] * up[1] + R[r][2] * up[2]);   // t = uq - R up (99)
        }
        for (int i = 0; i < 12; ++i) T[i] = Rt[i];
        T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
    }
    __syncthreads();
    // ---- inliers: |T p1 - p0| < 1 m (utils_test.py:55-63) ----
    double cnt[4] = {0, 0, 0, 0};
    for (int i = tid; i < N; i += 256) {
        const int64_t j = match(i);
        if (j >= 0 && j < M) {
            double d2 = 0.0;
            for (int r = 0; r < 3; ++r) {
                const double w = Rt[r * 4 + 0] * (double)k1[j * 3 + 0] + Rt[r * 4 + 1] * (double)k1[j * 3 + 1] +
                                 Rt[r * 4 + 2] * (double)k1[j * 3 + 2] + Rt[r * 4 + 3] - (double)k0[i * 3 + r];
                d2 += w * w;
            }
            if (sqrt(d2) < inlier_dist) cnt[0] += 1.0;
        }
    }
    block_sum<4>(cnt, scratch);
    if (tid == 0) {
        st[0] = n; st[1] = cnt[0]; st[2] = n > 0.0 ? cnt[0] / n : 0.0;
        double rte = __builtin_nan(""), rre = __builtin_nan("");
        if (G) {
            // T_error = inv(T) T_gt with inv(T) = [R^T | -R^T t] (utils_test.py:65-70; R is orthogonal)
            double E[3][4];
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 4; ++c) {
                    double s = 0.0;
                    for (int k = 0; k < 3; ++k) s += Rt[k * 4 + r] * (G[k * 4 + c] - (c == 3 ? Rt[k * 4 + 3] : 0.0));
                    E[r][c] = s;
                }
            rte = sqrt(E[0][3] * E[0][3] + E[1][3] * E[1][3] + E[2][3] * E[2][3]);
            rre = acos((E[0][0] + E[1][1] + E[2][2] - 1.0) * 0.5);   // unclamped, like the reference: may be NaN
        }
        st[3] = rte; st[4] = rre;
    }
}

}  // namespace
