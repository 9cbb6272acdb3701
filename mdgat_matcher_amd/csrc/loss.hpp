// Evaluation losses of MDGAT.forward (loss.hip): declarations shared with api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// workspace of launch_loss (256-byte aligned): per-row terms [B][N] and the per-tile column partials [B][tiles][M], in doubles
size_t loss_workspace_bytes(int B, int N, int M);

// Z [B][N+1][M+1] (float or double) + gt0 [B][N] / gt1 [B][M] (int64, -1 = dustbin) -> loss [B] fp64, one value per pair
// (superglue / triplet: the pair's ratio / mean; gap: the pair's loss).  A gt index outside [-1, M] / [-1, N] makes that pair's
// loss NaN and sets bit 0 of *bad_index (optional).  No allocation, no synchronisation.
template <typename T>
int launch_loss(int B, int N, int M, const T* Z, const int64_t* gt0, const int64_t* gt1, int method, double gamma, double* loss,
                unsigned* bad_index, void* workspace, size_t workspace_bytes, hipStream_t s);
