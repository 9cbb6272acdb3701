// The per-pair record of the reference's two evaluation scripts, computed where the forward left its outputs: what test.py:212-296
// and test_registration_metric.py:213-264 derive for one pair from matches0, the ground-truth matches, the keypoints and T_gt -
// with list comprehensions over every keypoint and a numpy SVD on the host - as one row of MDGAT_EVAL_COLS doubles
// (include/mdgat_hip.h names the columns and cites the line each restates).
//
// One workgroup of 256 threads per pair.  Pass 1 reads matches0 and gt0 once, classifies every frame-0 keypoint into the scripts'
// sets (integer counters per thread, summed over the workgroup in a fixed order: lanes by a butterfly, then the waves in order)
// and leaves the checked match of each keypoint in LDS; the pose (pose_dev.hpp: solve_icp + calculate_error, the arithmetic of
// mdgat_pose) then runs from LDS.  Every ratio is ONE fp64 division of two exact integers, which is what numpy's true_divide of
// two int64 does, so the values equal the scripts' bit for bit; the unguarded ones (fp_rate, tp_rate, tp_rate2 and the
// registration script's two) give NaN for 0/0 and inf for x/0 as numpy does.  The scripts' `continue` rules are status bits: the
// row is filled anyway and the host meter decides what to append.  No allocation, no synchronisation, no atomics on values (the
// bad-index word is a flag, set as mdgat_loss sets it): a pair's row does not depend on the batch it travels in.
#include "common.hpp"
#include "pose_dev.hpp"

namespace {

constexpr int EVAL_NMAX = 2175;        // the limit of the fp64 tail (Sinkhorn, its backward, the matching head)
constexpr int EVAL_NCOUNT = 10;

enum { C_VALID, C_VALID_GT, C_GT_NEG, C_TP, C_TN, C_FP, C_VALID_GTPOS, C_FP_REG, C_FN, C_BAD };

struct EvalArgs {
    const int64_t* matches0;   // [B][N]
    const int64_t* matches1;   // [B][M]
    const int64_t* gt0;        // [B][N]
    const int64_t* gt1;        // [B][M]
    const float* kpts0;        // [B][N][3]
    const float* kpts1;        // [B][M][3]
    const double* T_gt;        // [B][4][4] or NULL
    double* metrics;           // [B][MDGAT_EVAL_COLS]
    double* T;                 // [B][4][4]
    unsigned* bad_index;       // or NULL
    int N, M;
    double inlier_dist;
    const int* cnt0;           // optional (device int32 [B], both or neither): a ragged batch - pair b has cnt0[b] / cnt1[b] keypoints in slots
    const int* cnt1;           // of N / M: the strides stay N / M, everything counted, scanned or divided by follows the pair's own counts
};

// workgroup-wide sums of the counters -> every thread gets the totals (red: [4][EVAL_NCOUNT])
__device__ __forceinline__ void block_sum_counts(int (&c)[EVAL_NCOUNT], int* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < EVAL_NCOUNT; ++k)
        for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_xor(c[k], o, 64);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < EVAL_NCOUNT; ++k) red[wave * EVAL_NCOUNT + k] = c[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EVAL_NCOUNT; ++k) c[k] = red[k] + red[EVAL_NCOUNT + k] + red[2 * EVAL_NCOUNT + k] + red[3 * EVAL_NCOUNT + k];
}

__global__ __launch_bounds__(256) void eval_metrics_kernel(EvalArgs a) {
    __shared__ int match[EVAL_NMAX + 1];           // the checked matches0 of the pair: -1 or an index below M
    __shared__ int red[4 * EVAL_NCOUNT];
    __shared__ double scratch[4 * 16];
    __shared__ double Rt[12];
    const int b = blockIdx.x, tid = threadIdx.x, Ns = a.N, Ms = a.M;
    int N = Ns, M = Ms;
    if (a.cnt0) { N = a.cnt0[b]; M = a.cnt1[b]; }
    const int64_t* m0 = a.matches0 + (size_t)b * Ns;
    const int64_t* g0 = a.gt0 + (size_t)b * Ns;

    int c[EVAL_NCOUNT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < N; i += 256) {
        const int64_t mr = m0[i], gr = g0[i];
        c[C_BAD] += (mr < -1 || mr >= M) || (gr < -1 || gr > M);
        const int m = (mr >= 0 && mr < M) ? (int)mr : -1;
        const int g = (gr >= 0 && gr < M) ? (int)gr : -1;       // the dustbin M reads -1 (test.py:237)
        match[i] = m;
        const bool valid = m > -1, valid_gt = g > -1, same = m == g;      // test.py:215, 239
        c[C_VALID] += valid;
        c[C_VALID_GT] += valid_gt;
        c[C_GT_NEG] += !valid_gt;                               // matches_gt == -1 (:288)
        c[C_TP] += same && valid;                               // :277
        c[C_TN] += same && !valid;                              // :278
        c[C_FP] += valid && !valid_gt;                          // :279
        c[C_VALID_GTPOS] += valid && valid_gt;                  // :289
        c[C_FP_REG] += valid && !same;                          // test_registration_metric.py:239
        c[C_FN] += !valid && valid_gt;                          // test_registration_metric.py:241
    }
    {   // matches1 / gt1 enter no metric (the scripts only rewrite gt1's dustbin): their range is checked, nothing else
        const int64_t* m1 = a.matches1 + (size_t)b * Ms;
        const int64_t* g1 = a.gt1 + (size_t)b * Ms;
        for (int j = tid; j < M; j += 256) {
            const int64_t mr = m1[j], gr = g1[j];
            c[C_BAD] += (mr < -1 || mr >= N) || (gr < -1 || gr > N);
        }
    }
    block_sum_counts(c, red);          // (its barrier also publishes match[])

    double st[5];
    pose_of_pair(a.kpts0 + (size_t)b * Ns * 3, a.kpts1 + (size_t)b * Ms * 3, [&](int i) { return (int64_t)match[i]; }, N, M,
                 a.T_gt ? a.T_gt + (size_t)b * 16 : nullptr, a.inlier_dist, a.T + (size_t)b * 16, scratch, Rt, st);
    if (tid != 0) return;

    double* row = a.metrics + (size_t)b * MDGAT_EVAL_COLS;
    const double nan = __builtin_nan("");
    if (c[C_BAD]) {
        for (int k = 0; k < MDGAT_EVAL_COLS; ++k) row[k] = nan;
        double* T = a.T + (size_t)b * 16;
        for (int k = 0; k < 16; ++k) T[k] = nan;
        if (a.bad_index) atomicOr(a.bad_index, 1u);
        return;
    }
    const double n_valid = c[C_VALID], n_valid_gt = c[C_VALID_GT], n_gt_neg = c[C_GT_NEG], tp = c[C_TP], tn = c[C_TN], fp = c[C_FP];
    const double n_vgp = c[C_VALID_GTPOS], fp_reg = c[C_FP_REG], fn = c[C_FN], n_all = N;
    row[MDGAT_EVAL_N_VALID] = n_valid;
    row[MDGAT_EVAL_N_VALID_GT] = n_valid_gt;
    row[MDGAT_EVAL_N_GT_NEGATIVE] = n_gt_neg;
    row[MDGAT_EVAL_TRUE_POSITIVE] = tp;
    row[MDGAT_EVAL_TRUE_NEGATIVE] = tn;
    row[MDGAT_EVAL_FALSE_POSITIVE] = fp;
    row[MDGAT_EVAL_N_VALID_AND_GT_POSITIVE] = n_vgp;
    row[MDGAT_EVAL_FALSE_POSITIVE_REG] = fp_reg;
    row[MDGAT_EVAL_FALSE_NEGATIVE] = fn;
    row[MDGAT_EVAL_REPEATABILITY] = n_valid_gt / n_all;
    row[MDGAT_EVAL_PRECISION] = c[C_VALID] > 0 ? tp / n_valid : 0.0;
    row[MDGAT_EVAL_RECALL] = c[C_VALID] > 0 ? tp / n_valid_gt : 0.0;          // guarded by valid, not valid_gt, as in the script
    row[MDGAT_EVAL_MATCHING_SCORE] = tp / n_all;                               // (N > 0 here: the script's guard never fires)
    row[MDGAT_EVAL_ACCURACY] = (tp + tn) / n_all;
    row[MDGAT_EVAL_FP_RATE] = fp / n_gt_neg;
    row[MDGAT_EVAL_TP_RATE] = n_vgp / n_valid_gt;
    row[MDGAT_EVAL_TP_RATE2] = tp / n_valid_gt;
    row[MDGAT_EVAL_FP_RATE_REG] = fp_reg / (fp_reg + tn);
    row[MDGAT_EVAL_TP_RATE_REG] = tp / (tp + fn);
    // the pose of no match at all is the mean of an empty set in the reference (NaN throughout), not the zero matrix
    const bool none = c[C_VALID] == 0;
    const double rte = none ? nan : st[3], rre = none ? nan : st[4];
    if (none) {
        double* T = a.T + (size_t)b * 16;
        for (int k = 0; k < 16; ++k) T[k] = nan;
    }
    row[MDGAT_EVAL_INLIERS] = st[1];
    row[MDGAT_EVAL_INLIER_RATIO] = none ? nan : st[2];
    row[MDGAT_EVAL_TRANS_ERROR] = rte;
    row[MDGAT_EVAL_ROT_ERROR] = rre;
    unsigned status = 0;
    if (n_valid_gt < n_all * 0.1) status |= MDGAT_EVAL_BANNED;
    if (c[C_VALID] < 4) status |= MDGAT_EVAL_TOO_FEW_MATCHES;
    if (rte > 2.0 || rre > 5.0 || rte != rte || rre != rre) status |= MDGAT_EVAL_REGISTRATION_FAIL;
    const double five_deg = 3.141592653589793 / 180 * 5;                       // np.pi / 180 * 5
    if (rte < 2.0) status |= MDGAT_EVAL_RTE_OK;
    if (rre == rre && rre < five_deg) status |= MDGAT_EVAL_RRE_OK;
    row[MDGAT_EVAL_STATUS] = (double)status;
}

}  // namespace

int launch_eval_metrics(int B, int N, int M, const int64_t* matches0, const int64_t* matches1, const int64_t* gt0, const int64_t* gt1,
                        const float* kpts0, const float* kpts1, const double* T_gt, double inlier_dist, double* metrics, double* T,
                        unsigned* bad_index, hipStream_t s, const int* cnt0, const int* cnt1) {
    if ((cnt0 != nullptr) != (cnt1 != nullptr)) { mdgat_set_error("mdgat_eval_metrics: per-pair counts for one frame only"); return MDGAT_ERR_BAD_ARG; }
    if (N > EVAL_NMAX || M > EVAL_NMAX) {
        mdgat_set_error("mdgat_eval_metrics: %d x %d keypoints are beyond the fp64 tail's limit (%d)", N, M, EVAL_NMAX);
        return MDGAT_ERR_UNSUPPORTED;
    }
    if (B <= 0) return MDGAT_OK;
    EvalArgs a{matches0, matches1, gt0, gt1, kpts0, kpts1, T_gt, metrics, T, bad_index, N, M, inlier_dist, cnt0, cnt1};
    hipLaunchKernelGGL(eval_metrics_kernel, dim3(B), dim3(256), 0, s, a);
    return mdgat_check_hip(hipGetLastError(), "eval_metrics launch");
}
