// Evaluation losses of MDGAT.forward (loss.hip) and their gradient (loss_grad.hip): declarations shared with api.hip and between the two.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

constexpr int LOSS_TR = 16;        // rows per workgroup of the tile kernel
constexpr int LOSS_THREADS = 256;
constexpr int LOSS_GAP_MAX_ROWS = 15000;     // the gap prologue holds N + 2 row counters in LDS (at most 64 KB per workgroup)

// t(z) = -log(exp(z)) as the reference applies it: -z where exp(z) is a normal number, literal below
__device__ inline double loss_t(double z) { return z < -708.0 ? -log(exp(z)) : -z; }
// torch.clamp(x, min=0): NaN stays NaN
__device__ inline double loss_clamp0(double x) { return x < 0.0 ? 0.0 : x; }
// gt index -> row / column of Z: -1 is the dustbin (`dust`), [0, dust] as is, anything else -1 (an indexing error in the reference)
__device__ inline int loss_gt_index(int64_t g, int dust) { return g == -1 ? dust : (g >= 0 && g <= dust ? (int)g : -1); }

inline size_t loss_tiles_of(int N) { return (size_t)(N + 1 + LOSS_TR - 1) / LOSS_TR; }

// workspace of launch_loss (256-byte aligned): per-row terms [B][N] and the per-tile column partials [B][tiles][M], in doubles
size_t loss_workspace_bytes(int B, int N, int M);

// Z [B][N+1][M+1] (float or double) + gt0 [B][N] / gt1 [B][M] (int64, -1 = dustbin) -> loss [B] fp64, one value per pair
// (superglue / triplet: the pair's ratio / mean; gap: the pair's loss).  A gt index outside [-1, M] / [-1, N] makes that pair's
// loss NaN and sets bit 0 of *bad_index (optional).  No allocation, no synchronisation.
template <typename T>
int launch_loss(int B, int N, int M, const T* Z, const int64_t* gt0, const int64_t* gt1, int method, double gamma, double* loss,
                unsigned* bad_index, void* workspace, size_t workspace_bytes, hipStream_t s);

// ---- the statistics pass of the gradient (loss_grad.hip): the forward's tile kernel (and gap's ordering prologue) leaving the raw
// per-row / per-tile records instead of the terms.  Per pair:
//   triplet: rowterm [N] the row term's clamp argument t(pos) - t(neg) + gamma, rowaux [N] the negative's column (lowest on ties);
//            slab [tiles][M] the tile's column maximum over the rows other than the positive, slabaux [tiles][M] its row (lowest);
//   gap:     rowterm [N] S_i, rowaux [N] the row's active count; slab / slabaux [tiles][M] the tile's share of S_c and of the active
//            count of column c of V; tpos [M] t(P[c]), cols [M] the columns in P's order, A [N+2] the positives in rows < i.
struct LossStats {
    double *rowterm, *slab, *tpos;
    int *cols, *A, *rowaux, *slabaux;
    int tiles;
    size_t total;
};
LossStats loss_stats_carve(void* base, int B, int N, int M);
// triplet / gap only (superglue needs no statistics); `ws` holds loss_stats_carve(nullptr, B, N, M).total bytes, 256-byte aligned
template <typename T>
int launch_loss_stats(int B, int N, int M, const T* Z, const int64_t* gt0, const int64_t* gt1, int method, double gamma, const LossStats& ws,
                      hipStream_t s);
