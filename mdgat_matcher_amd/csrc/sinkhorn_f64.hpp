// fp64 Sinkhorn of the reference-exact mode (sinkhorn_f64.hip): declarations shared with api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

class CoopGroup;      // coop_chain.hpp

// scores [B][N][M] fp64 -> Z (mdgat.py:279-308) as fp64 and / or its fp32 rounding, and / or the arg-maxes the match extraction needs
// (rbest [B][N]: per row over the columns - the inner M ones when `inner`, else including the dustbin; cbest [B][M] per column over the
// rows, the slabs of a pair merged in fp64; both decided on the fp64 values, the values handed on as fp32).  workspace: 256-byte aligned,
// sinkhorn_f64_workspace_bytes.  error_word: bit 0 raised when a workgroup gave up waiting for a partner (optional).
// cnt0 / cnt1 (device int32 [B], both or neither): a RAGGED batch - pair b has cnt0[b] x cnt1[b] keypoints (1 <= cnt0[b] <= N, 1 <= cnt1[b] <= M,
// checked by the caller) and is stored in slots padded to N x M, which are then the strides of every array here and must fit the
// register-resident form (at most 575).  Pair b's block Z[b, :cnt0[b]+1, :cnt1[b]+1] and its arg-maxes have the bits of the pair run alone;
// the rest of its Z slot is zero, rbest / cbest beyond its counts are not written.
size_t sinkhorn_f64_workspace_bytes(int B, int N, int M);
bool sinkhorn_f64_supported(int N, int M);
bool sinkhorn_f64_ragged_supported(int N, int M);      // per-pair counts: the register-resident form only (padded sizes <= 575, form not forced to streaming)
int launch_sinkhorn_f64(int B, int N, int M, const double* scores, double alpha, int iters, double* Z64, float* Z32, int inner, int* rbest_idx,
                        float* rbest_val, int* cbest_idx, float* cbest_val, void* workspace, size_t workspace_bytes, unsigned* error_word,
                        CoopGroup& group, const double* alpha_dev = nullptr,       // on the group's stream; alpha_dev: the bin score on the device (replaces alpha)
                        const int* cnt0 = nullptr, const int* cnt1 = nullptr);
// A RAGGED batch on the STREAMING form (its kernels' RAGGED instantiations): the same arguments and outputs as launch_sinkhorn_f64 with
// counts, in slots of N, M <= 2175, whatever mdgat_set_f64_sinkhorn_form says.  Pair b's bits are those of the pair run alone through
// the uniform streaming form.  No workgroup waits for another: no error word, no CoopGroup.  The workspace is carved by the slot (K is
// [B][N][Mp]: 35.6 MB per pair at 2048), 256-byte aligned.
bool sinkhorn_f64_stream_ragged_supported(int N, int M);
size_t sinkhorn_f64_stream_ragged_workspace_bytes(int B, int N, int M);
int launch_sinkhorn_f64_stream_ragged(int B, int N, int M, const int* cnt0, const int* cnt1, const double* scores, double alpha, int iters, double* Z64,
                                      float* Z32, int inner, int* rbest_idx, float* rbest_val, int* cbest_idx, float* cbest_val, void* workspace,
                                      size_t workspace_bytes, hipStream_t s, const double* alpha_dev = nullptr);
// rbest / cbest (idx + val each) for the extraction, carved behind the kernel's own workspace (a null base: their size only)
struct Sk64Bests { int* ri; float* rv; int* ci; float* cv; size_t bytes; };
Sk64Bests sinkhorn_f64_bests(void* base, int B, int N, int M);
// The streaming form's init and iterations alone, with the potential history written through (the backward, sinkhorn_grad.hip):
// a_1 .. a_T (a_N last in each) into rows 1, 3, .. of hist_a [B][2T][hist_lda], b_0 .. b_{T-1} into rows 0, 2, .. of hist_b
// [B][2T][Mp] (zero beyond column M).  Left in the workspace: K [B][N][Mp] (rows padded with zeros, the dustbin column at M; the
// dustbin row, all ones, is not stored) and b_T [B][Mp].  P: [B][2][G][Mp] doubles the iterations are done with.  N, M <= 2175.
struct Sk64Stream { double* K; double* P; double* bvec; int Mp, G; size_t bytes; };
Sk64Stream sinkhorn_f64_stream_carve(void* base, int B, int N, int M);       // (a null base: its size only)
int sinkhorn_f64_stream_history(int B, int N, int M, const double* scores, double alpha, int iters, double* hist_a, int hist_lda, double* hist_b,
                                void* workspace, hipStream_t s);
