// The steps on either side of the matcher that the reference does per pair on the host with numpy
// (SURVEY.md section 8f):
//
//   pose_kernel      rigid pose from the matches: solve_icp (utils/utils_test.py:73-110: centroids, 3x3 cross
//                    covariance, SVD, R = U V^T - no reflection fix, like the reference), inlier count and
//                    RTE / RRE against a ground-truth pose (calculate_error, utils_test.py:41-71)
//   gt_match_kernel  ground-truth matches of a frame pair: brute-force nearest neighbours of the world-frame
//                    keypoints in both directions under a distance threshold, optional mutual check
//                    (load_data.py:238-285)
//
// Both are tiny (3-D points, <= 2048 per frame) and latency bound: one workgroup per pair, fp64 arithmetic like the
// reference (MI355X runs fp64 at half the fp32 vector rate), so the results agree to round-off, not to 1e-4.
#include "common.hpp"
#include "pose_dev.hpp"   // the pose arithmetic itself, shared with eval_metrics.hip

namespace {

struct PoseArgs {
    const float* kpts0;      // [B][N][3]
    const float* kpts1;      // [B][M][3]
    const int64_t* matches0; // [B][N], -1 = unmatched
    const double* T_gt;      // [B][4][4] or NULL
    double* T;               // [B][4][4]
    double* stats;           // [B][5]: matches, inliers, inlier ratio, translation error, rotation error (rad)
    int N, M;
    double inlier_dist;
};

__global__ __launch_bounds__(256) void pose_kernel(PoseArgs a) {
    __shared__ double scratch[4 * 16];
    __shared__ double Rt[12];
    const int b = blockIdx.x;
    const int64_t* m0 = a.matches0 + (size_t)b * a.N;
    double st[5];
    pose_of_pair(a.kpts0 + (size_t)b * a.N * 3, a.kpts1 + (size_t)b * a.M * 3, [m0](int i) { return m0[i]; }, a.N, a.M,
                 a.T_gt ? a.T_gt + (size_t)b * 16 : nullptr, a.inlier_dist, a.T + (size_t)b * 16, scratch, Rt, st);
    if (threadIdx.x == 0) {
        double* out = a.stats + (size_t)b * 5;
        for (int i = 0; i < 5; ++i) out[i] = st[i];
    }
}

struct GtArgs {
    const float* kpts0;   // [B][N][3] sensor-frame keypoints
    const float* kpts1;   // [B][M][3]
    const double* T0;     // [B][4][4] sensor -> world of frame 0 (pose . T_cam0_velo, load_data.py:238-242) or NULL
    const double* T1;     // [B][4][4]
    int64_t* gt0;         // [B][N]
    int64_t* gt1;         // [B][M]
    int64_t* rep;         // [B] repeatability count (load_data.py:264)
    int N, M, mutual;
    double threshold;
    const int *cnt0, *cnt1;   // a ragged batch: the pairs' own keypoint counts in slots of N / M (device int32 [B]); NULL otherwise
};

__device__ __forceinline__ void to_world(const double* T, const float* p, double (&w)[3]) {
    if (!T) { w[0] = p[0]; w[1] = p[1]; w[2] = p[2]; return; }
#pragma unroll
    for (int r = 0; r < 3; ++r) w[r] = T[r * 4 + 0] * (double)p[0] + T[r * 4 + 1] * (double)p[1] + T[r * 4 + 2] * (double)p[2] + T[r * 4 + 3];
}

// RAGGED: pair b works on its own cnt0[b] x cnt1[b] keypoints in slots of N x M (the strides of every array and of the LDS layout);
// gt0 / gt1 beyond the counts are written as -1, rep counts the pair's own rows.  The uniform instantiation is the kernel as it was.
template <bool RAGGED>
__global__ __launch_bounds__(256) void gt_match_kernel(GtArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int N = a.N, M = a.M, b = blockIdx.x, tid = threadIdx.x;
    const int n0 = RAGGED ? a.cnt0[b] : N, n1 = RAGGED ? a.cnt1[b] : M;
    double* w0 = sm;                 // [N][3] world-frame keypoints of frame 0
    double* w1 = w0 + 3 * N;         // [M][3]
    int* nn0 = reinterpret_cast<int*>(w1 + 3 * M);   // [N] argmin over frame 1 (min2 of load_data.py:259)
    int* nn1 = nn0 + N;                                 // [M] argmin over frame 0 (min1, 258)
    double* d0 = reinterpret_cast<double*>(nn1 + M + ((N + M) & 1));   // [N] min distance of a frame-0 point (min1v, 260)
    double* d1 = d0 + N;                                // [M] (min2v, 281)
    __shared__ int repc;
    if (tid == 0) repc = 0;
    const double* T0 = a.T0 ? a.T0 + (size_t)b * 16 : nullptr;
    const double* T1 = a.T1 ? a.T1 + (size_t)b * 16 : nullptr;
    for (int i = tid; i < n0; i += 256) { double w[3]; to_world(T0, a.kpts0 + ((size_t)b * N + i) * 3, w); w0[3 * i] = w[0]; w0[3 * i + 1] = w[1]; w0[3 * i + 2] = w[2]; }
    for (int j = tid; j < n1; j += 256) { double w[3]; to_world(T1, a.kpts1 + ((size_t)b * M + j) * 3, w); w1[3 * j] = w[0]; w1[3 * j + 1] = w[1]; w1[3 * j + 2] = w[2]; }
    __syncthreads();
    // cdist + argmin (first minimum, like numpy) in both directions
    for (int i = tid; i < n0; i += 256) {
        double best = __builtin_inf(); int bj = 0;
        const double x = w0[3 * i], y = w0[3 * i + 1], z = w0[3 * i + 2];
        for (int j = 0; j < n1; ++j) {
            const double dx = x - w1[3 * j], dy = y - w1[3 * j + 1], dz = z - w1[3 * j + 2];
            const double d = sqrt(dx * dx + dy * dy + dz * dz);
            if (d < best) { best = d; bj = j; }
        }
        nn0[i] = bj; d0[i] = best;
    }
    for (int j = tid; j < n1; j += 256) {
        double best = __builtin_inf(); int bi = 0;
        const double x = w1[3 * j], y = w1[3 * j + 1], z = w1[3 * j + 2];
        for (int i = 0; i < n0; ++i) {
            const double dx = w0[3 * i] - x, dy = w0[3 * i + 1] - y, dz = w0[3 * i + 2] - z;
            const double d = sqrt(dx * dx + dy * dy + dz * dz);
            if (d < best) { best = d; bi = i; }
        }
        nn1[j] = bi; d1[j] = best;
    }
    __syncthreads();
    int64_t* g0 = a.gt0 + (size_t)b * N;
    int64_t* g1 = a.gt1 + (size_t)b * M;
    if (RAGGED) {
        for (int i = n0 + tid; i < N; i += 256) g0[i] = -1;
        for (int j = n1 + tid; j < M; j += 256) g1[j] = -1;
    }
    int local = 0;
    if (!a.mutual) {
        // match1[min1v < thr] = min2[min1v < thr]; match2[min2v < thr] = min1[min2v < thr] (load_data.py:278-283)
        for (int i = tid; i < n0; i += 256) { const bool ok = d0[i] < a.threshold; g0[i] = ok ? nn0[i] : -1; local += ok; }
        for (int j = tid; j < n1; j += 256) g1[j] = d1[j] < a.threshold ? nn1[j] : -1;
    } else {
        // load_data.py:272-276: matches = {j : j = min2[i] for some i with min1v[i] < thr}  intersected with
        // {j : min2[min1[j]] == j}; match1[min1[j]] = j, match2[j] = min1[j] for those j
        for (int i = tid; i < n0; i += 256) { g0[i] = -1; local += d0[i] < a.threshold; }
        for (int j = tid; j < n1; j += 256) g1[j] = -1;
        __syncthreads();
        for (int j = tid; j < n1; j += 256) {
            const int i = nn1[j];
            if (nn0[i] == j && d0[i] < a.threshold) { g1[j] = i; g0[i] = j; }
        }
    }
    if (local) atomicAdd(&repc, local);
    __syncthreads();
    if (tid == 0) a.rep[b] = repc;
}

}  // namespace

int launch_pose(int B, int N, int M, const float* kpts0, const float* kpts1, const int64_t* matches0, const double* T_gt,
                double inlier_dist, double* T, double* stats, hipStream_t s) {
    if (B <= 0) return MDGAT_OK;
    PoseArgs a{kpts0, kpts1, matches0, T_gt, T, stats, N, M, inlier_dist};
    hipLaunchKernelGGL(pose_kernel, dim3(B), dim3(256), 0, s, a);
    return mdgat_check_hip(hipGetLastError(), "pose launch");
}

int launch_gt_match(int B, int N, int M, const float* kpts0, const float* kpts1, const double* T0, const double* T1,
                    double threshold, int mutual, int64_t* gt0, int64_t* gt1, int64_t* rep, hipStream_t s, const int* cnt0, const int* cnt1) {
    if (B <= 0) return MDGAT_OK;
    const size_t lds = (size_t)(3 * (N + M) + (N + M)) * sizeof(double) + (size_t)(N + M + 2) * sizeof(int);
    if (lds > 160 * 1024) { mdgat_set_error("gt_match: %d + %d keypoints exceed the LDS budget", N, M); return MDGAT_ERR_UNSUPPORTED; }
    GtArgs a{kpts0, kpts1, T0, T1, gt0, gt1, rep, N, M, mutual, threshold, cnt0, cnt1};
    auto kern = cnt0 ? gt_match_kernel<true> : gt_match_kernel<false>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(B), dim3(256), lds, s, a);
    return mdgat_check_hip(hipGetLastError(), "gt_match launch");
}
