// fp64 Sinkhorn of the reference-exact mode (sinkhorn_f64.hip): declarations shared with api.hip and sinkhorn_grad.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

class CoopGroup;      // coop_chain.hpp

// rbest / cbest (idx + val each) for the extraction, carved behind the kernel's own workspace (a null base: their size only)
struct Sk64Bests { int* ri; float* rv; int* ci; float* cv; size_t bytes; };
Sk64Bests sinkhorn_f64_bests(void* base, int B, int N, int M);

// ONE CALL: scores [B][N][M] fp64 -> Z (mdgat.py:279-308) as fp64 (Z64) and / or its fp32 rounding (Z32), and / or the arg-maxes the
// match extraction needs (bests, all null or all set: ri / rv [B][N] per row over the columns - the inner M ones when `inner`, else
// including the dustbin; ci / cv [B][M] per column over the rows, the slabs of a pair merged in fp64; both decided on the fp64 values,
// the values handed on as fp32).  alpha: the bin score, or alpha_dev: where it lives on the device (replaces alpha).
// cnt0 / cnt1 (device int32 [B], both or neither): a RAGGED batch - pair b has cnt0[b] x cnt1[b] keypoints (1 <= cnt0[b] <= N,
// 1 <= cnt1[b] <= M, checked by the caller) and is stored in slots padded to N x M, which are then the strides of every array here.
// Pair b's block Z[b, :cnt0[b]+1, :cnt1[b]+1] and its arg-maxes have the bits of the pair run alone on the same form; the rest of its
// Z slot is zero, the arg-maxes beyond its counts are not written.
struct Sk64Call {
    int B, N, M;
    const double* scores; double alpha; const double* alpha_dev; int iters;
    double* Z64; float* Z32;
    int inner;
    Sk64Bests bests;
    const int* cnt0; const int* cnt1;
};

// WHICH FORM runs a call is decided here and nowhere else.  resident: the register-resident kernel, whose workgroups wait for each other
// (N <= 576, M <= 575; with counts N <= 575 too, MDGAT_RAGGED_MAX_KEYPOINTS).  streaming: K in memory, one launch per iteration, no
// workgroup waits (N, M <= 2175, with or without counts).  A uniform call runs the resident form wherever it holds the shape unless
// mdgat_set_f64_sinkhorn_form(1) forces the streaming one.  A ragged call follows ragged_mode (mdgat_set_ragged_sinkhorn; the per-op
// entries pass 0 or 2): 0 the resident form or none (none under the forced form as well), 2 the streaming form, 1 the resident form
// where mode 0 has it and the streaming one elsewhere.
enum class Sk64Form { unsupported, resident, streaming };
Sk64Form sinkhorn_f64_form(int N, int M, bool ragged, int ragged_mode);
inline bool sinkhorn_f64_supported(int N, int M) { return sinkhorn_f64_form(N, M, false, 0) != Sk64Form::unsupported; }
// Which of the eleven forms a call runs - the two above with and without counts, the streaming one by its instantiation <5 | 9 | 17>, and
// the history run below (mdgat_sinkhorn_f64_plan, include/mdgat_hip.h: the table and the arguments) - from the code the launchers
// branch on, and how many calls have run in each in this process (mdgat_sinkhorn_f64_launches).  Host code only; no HIP call.
int sinkhorn_f64_plan(int N, int M, int ragged, int ragged_mode, int form, int history, int* slabs, int* chunks);
void sinkhorn_f64_launches(uint64_t counts[MDGAT_SINKHORN_F64_FORMS]);
// the form's workspace, carved by the padded sizes (streaming: K is [B][N][Mp], 35.6 MB per pair at 2048); 0 for Sk64Form::unsupported
size_t sinkhorn_f64_workspace_bytes(int B, int N, int M, Sk64Form form);

// Runs call c on `form` - the caller's decision (sinkhorn_f64_form), refused if the form does not hold the call - on stream s.
// workspace: 256-byte aligned, sinkhorn_f64_workspace_bytes of the form.  The resident form alone uses group (on stream s; it admits the
// launch behind the device's previous waiting one) and error_word (optional: bit 0 raised when a workgroup gave up waiting for a partner).
int launch_sinkhorn_f64(const Sk64Call& c, Sk64Form form, void* workspace, size_t workspace_bytes, hipStream_t s, CoopGroup* group, unsigned* error_word);

// The streaming form's init and iterations alone, with the potential history written through (the backward, sinkhorn_grad.hip; c: a
// uniform call that names no output): a_1 .. a_T (a_N last in each) into rows 1, 3, .. of hist_a [B][2T][hist_lda],
// b_0 .. b_{T-1} into rows 0, 2, .. of hist_b [B][2T][Mp] (zero beyond column M).  Left in the workspace: K [B][N][Mp] (rows padded with
// zeros, the dustbin column at M; the dustbin row, all ones, is not stored) and b_T [B][Mp].  P: [B][2][G][Mp] doubles the iterations
// are done with.  N, M <= 2175.
struct Sk64Stream { double* K; double* P; double* bvec; int Mp, G; size_t bytes; };
Sk64Stream sinkhorn_f64_stream_carve(void* base, int B, int N, int M);       // (a null base: its size only)
int sinkhorn_f64_stream_history(const Sk64Call& c, double* hist_a, int hist_lda, double* hist_b, void* workspace, hipStream_t s);
