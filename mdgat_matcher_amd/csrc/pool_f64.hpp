// pool_f64.hip: the frame maximum of the pooled descriptor encoder (descriptor = 'FPFH_gloabal'), its broadcast epilogue and its backward.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

// g[unit][128] = max over the unit's rows of e, idx[unit][128] (optional) the first row that holds it.
//   M > 0: the forward's layout - e [B][N + M][128], pair-major, frame 0 then frame 1; unit = 2 pair + frame (2B units).
//   M == 0: e [B][N][128], unit = pair (the training op).
// cnt0 / cnt1 (device int32 [B], both or neither; M > 0 only): a ragged batch - pair b's frames hold cnt0[b] / cnt1[b] keypoints in slots
// of N / M; the rows beyond are not read.  The caller has checked 1 <= cnt <= slot on the host.
struct FrameMaxArgs {
    const double* e;
    int B, N, M;
    const int *cnt0, *cnt1;
    double* g;
    int64_t* idx;
};
int launch_frame_max_f64(const FrameMaxArgs& a, hipStream_t s);
// hid [B (N + M)][C] = max(hid + add[2 pair + frame], 0) in place; add [2B][C]; guard: as GemmF64Args::guard, tested on the sum
int launch_add_rows_relu_f64(double* hid, const double* add, int C, int B, int N, int M, unsigned* guard, hipStream_t s);
// de [B][n][128] = dg [B][128] at row idx [B][128], zero elsewhere
int launch_frame_max_backward_f64(int B, int n, const double* dg, const int64_t* idx, double* de, hipStream_t s);
