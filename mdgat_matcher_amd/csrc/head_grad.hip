// The matching head (mdgat.py:397 final_proj, 430-431 the score matrix) as a call of its own, and its backward, in fp64.
//
// Point-major: desc0 [B][N][128], desc1 [B][M][128], W [128 out][128 in], b [128], s = 1 / sqrt(128).
//      md0 = desc0 W^T + b,  md1 = desc1 W^T + b,  scores[z] = s md0[z] md1[z]^T                         [B][N][M]
// and with G = dL/dscores (tests/head_grad_ref.py restates it in numpy):
//      dmd0[z] = s G[z] md1[z]  [N][128] (over M)        dmd1[z] = s G[z]^T md0[z]  [M][128] (over N)
//      ddesc0 = dmd0 W,  ddesc1 = dmd1 W                  (over the 128 output channels)
//      dW[c][k] = sum over every point p of every pair, both frames, of dmd[p][c] desc[p][k];   db[c] = the same sum of dmd[p][c]
//
// The forward is tail64's (api.hip): launch_gemm_f64 for final_proj - one launch per frame, the frames being separate arrays here -
// and the batched scaled product.  The backward recomputes md0 / md1 with the same launches, then, all on v_mfma_f64_16x16x4_f64:
//   1. hg_dmd_kernel<FRAME>: a workgroup owns 64 points of a (pair, frame) x the 128 channels, four waves of 32 x 64 (eight
//      accumulators each), and walks the contraction in chunks of 32 through LDS, the next chunk in flight in registers
//      (gemm_f64_kernel's shape).  G is read TWICE, once per frame, both times by 8-byte loads that run along a row of G (a row of
//      M doubles is not 16-byte aligned in general): frame 0 stages [64 i][32 j] and reads the A fragment along j, frame 1 stages
//      [32 i][64 j] and reads it along i - the transpose happens in the LDS read, not in the global one.  Pitches: the half-waves of
//      a ds_read_b64 (k = lane >> 4 in {0, 1} or {2, 3}) must fall on different halves of the 64 banks - 34 for rows read along k,
//      a pitch of 16 mod 32 (80, 144) for rows read across (the md chunk [32][128] is the B operand: k = row).
//      Epilogue: the tile times s goes to the workspace (dW's operand) and to LDS [64][130], and ddesc = tile x W is formed from
//      there: A from LDS, B = W[c][k] straight from L2 (contracted over its ROWS: 16 consecutive doubles per k, 128 KB that every
//      workgroup shares).  66.6 KB of LDS: two workgroups per CU.
//   2. hg_dw_kernel: per pair dW_pair = dmd^T desc over the pair's points, frame 0 then frame 1, points ascending - ONE chain per
//      output element, no split of the contraction.  Both operands are contracted over their rows, so both fragments are coalesced
//      loads from L2 and there is no LDS: sixteen waves of 32 x 32 per pair.  db_pair rides along: every lane adds up the A
//      fragment values it loads (a quarter of the points each), the four quarters are combined as (0 + 1) + (2 + 3).  (The MLP's
//      dw_f64_kernel, dw_f64.hip, is this kernel generalised - ragged tiles, two column sources, a BN in front; run here its
//      per-load predicates cost 4 to 9 % of the backward, measured, so the head keeps the whole-tile kernel.)
//   3. launch_dw_reduce_f64 (dw_f64.hip): dW = pair 0's partial + pair 1's + ... in pair order, db likewise.  No value atomics and
//      no workgroup waits for another: the bits are the same from run to run, ddesc of a pair does not depend on its batch, and for
//      B = 2 dW(batch) == dW(pair 0 alone) + dW(pair 1 alone).
// Workspace: md0, md1, dmd0, dmd1 ([B][N + M][128] twice) and the per-pair partials [B][128 x 128 + 128].
#include "common.hpp"
#include "f64.hpp"
#include "f64_dev.hpp"

namespace {

constexpr int HG_D = 128;                         // descriptor_dim
constexpr double HG_SCALE = 0.08838834764831845;  // 1 / sqrt(128), tail64's
constexpr int HG_KC = 32;                         // contraction chunk
constexpr int HG_LDG0 = 34;                       // frame 0: G chunk [64 i][32 j]
constexpr int HG_LDG1 = 80;                       // frame 1: G chunk [32 i][64 j]
constexpr int HG_LDM = 144;                       // md chunk [32][128]
constexpr int HG_LDT = 130;                       // dmd tile [64][128]
constexpr int HG_PART = HG_D * HG_D + HG_D;       // a pair's partial: dW then db
constexpr size_t HG_LDS = 64 * HG_LDT * sizeof(double);
static_assert((32 * HG_LDG1 + HG_KC * HG_LDM) * sizeof(double) <= HG_LDS && (64 * HG_LDG0 + HG_KC * HG_LDM) * sizeof(double) <= HG_LDS,
              "the chunks of phase 1 live in the tile's room");

struct HgArgs {
    int B, N, M;
    const double* G;                  // [B][N][M]
    const double *desc0, *desc1;      // [B][N][128], [B][M][128]
    const double* W;                  // [128][128]
    const double *md0, *md1;          // the recomputed projections
    double *dmd0, *dmd1;              // workspace, or nullptr when neither dW nor db is wanted
    double *ddesc0, *ddesc1;          // or nullptr
    double* P;                        // [B][HG_PART]
};

template <int FRAME>
__global__ __launch_bounds__(256) void hg_dmd_kernel(HgArgs a) {
    extern __shared__ __attribute__((aligned(16))) double hg_lds[];
    constexpr int LDG = FRAME == 0 ? HG_LDG0 : HG_LDG1;
    double* Gs = hg_lds;
    double* Ms = hg_lds + (FRAME == 0 ? 64 * HG_LDG0 : 32 * HG_LDG1);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int wm = wave & 1, wn = wave >> 1;
    const int N = a.N, M = a.M;
    const int P = FRAME == 0 ? N : M;              // this frame's points
    const int Kc = FRAME == 0 ? M : N;             // the contraction: the other frame's points
    const int tiles = (P + 63) >> 6;
    const int pair = blockIdx.x / tiles, p0 = (blockIdx.x % tiles) * 64;
    const double* Gp = a.G + (size_t)pair * N * M;
    const double* mdo = FRAME == 0 ? a.md1 + (size_t)pair * M * HG_D : a.md0 + (size_t)pair * N * HG_D;
    double rg[8];
    f64x2 rm[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = tid + 256 * u;
            const int i = FRAME == 0 ? p0 + (idx >> 5) : k0 + (idx >> 6);
            const int j = FRAME == 0 ? k0 + (idx & 31) : p0 + (idx & 63);
            rg[u] = (i < N && j < M) ? Gp[(size_t)i * M + j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = tid + 256 * u, row = k0 + (idx >> 6);
            rm[u] = row < Kc ? *reinterpret_cast<const f64x2*>(mdo + (size_t)row * HG_D + (idx & 63) * 2) : f64x2{0.0, 0.0};
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = tid + 256 * u;
            Gs[FRAME == 0 ? (idx >> 5) * LDG + (idx & 31) : (idx >> 6) * LDG + (idx & 63)] = rg[u];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = tid + 256 * u;
            *reinterpret_cast<f64x2*>(Ms + (idx >> 6) * HG_LDM + (idx & 63) * 2) = rm[u];
        }
    };
    f64x4 acc[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = f64x4{0.0, 0.0, 0.0, 0.0};
    fetch(0);
    stash();
    __syncthreads();
    // A: row = the output point (l15), k = g; frame 0 along a staged row, frame 1 across the staged rows
    const double* ap = FRAME == 0 ? Gs + (wm * 32 + l15) * LDG + g : Gs + g * LDG + wm * 32 + l15;
    constexpr int A_RB = FRAME == 0 ? 16 * LDG : 16, A_K = FRAME == 0 ? 4 : 4 * LDG;
    const double* bp = Ms + g * HG_LDM + wn * 64 + l15;
    for (int k0 = 0; k0 < Kc; k0 += HG_KC) {
        const bool more = k0 + HG_KC < Kc;
        if (more) fetch(k0 + HG_KC);
        for (int j = 0; j < HG_KC / 4; ++j) {
            double fa[2], fb[4];
#pragma unroll
            for (int r = 0; r < 2; ++r) fa[r] = ap[r * A_RB + j * A_K];
#pragma unroll
            for (int c = 0; c < 4; ++c) fb[c] = bp[j * 4 * HG_LDM + c * 16];
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = mfma64(fa[r], fb[c], acc[r][c]);
        }
        __syncthreads();
        if (more) {
            stash();
            __syncthreads();
        }
    }
    // D: lane (column l15, g), register i -> row g + 4 i.  The tile times s: to the workspace and to LDS (rows beyond P are zero)
    double* dmd = FRAME == 0 ? a.dmd0 : a.dmd1;
    double* T = hg_lds;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int p = wm * 32 + r * 16 + g + 4 * i, ch = wn * 64 + c * 16 + l15;
                const double v = acc[r][c][i] * HG_SCALE;
                if (dmd && p0 + p < P) dmd[((size_t)pair * P + p0 + p) * HG_D + ch] = v;
                T[p * HG_LDT + ch] = v;
            }
    double* dd = FRAME == 0 ? a.ddesc0 : a.ddesc1;
    if (!dd) return;
    __syncthreads();
    // ddesc tile = T W: A from LDS (row = point, k = channel), B = W[channel][k] from L2
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = f64x4{0.0, 0.0, 0.0, 0.0};
    const double* tp = T + (wm * 32 + l15) * HG_LDT + g;
    const double* wp = a.W + (size_t)g * HG_D + wn * 64 + l15;
#pragma unroll 4
    for (int c0 = 0; c0 < HG_D; c0 += 4) {
        double fa[2], fb[4];
#pragma unroll
        for (int r = 0; r < 2; ++r) fa[r] = tp[r * 16 * HG_LDT + c0];
#pragma unroll
        for (int c = 0; c < 4; ++c) fb[c] = wp[(size_t)c0 * HG_D + c * 16];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = mfma64(fa[r], fb[c], acc[r][c]);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int p = p0 + wm * 32 + r * 16 + g + 4 * i;
                if (p < P) dd[((size_t)pair * P + p) * HG_D + wn * 64 + c * 16 + l15] = acc[r][c][i];
            }
}

// a pair's partial of dW and db: grid (B, 4), sixteen waves of 32 channels x 32 inputs per pair
__global__ __launch_bounds__(256) void hg_dw_kernel(HgArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int id = blockIdx.y * 4 + wave, rt = id >> 2, ct = id & 3;
    const int pair = blockIdx.x;
    f64x4 acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[r][c] = f64x4{0.0, 0.0, 0.0, 0.0};
    double s0 = 0.0, s1 = 0.0;
    auto step = [&](double a0, double a1, double b0, double b1) {
        acc[0][0] = mfma64(a0, b0, acc[0][0]);
        acc[0][1] = mfma64(a0, b1, acc[0][1]);
        acc[1][0] = mfma64(a1, b0, acc[1][0]);
        acc[1][1] = mfma64(a1, b1, acc[1][1]);
        s0 += a0;
        s1 += a1;
    };
    auto frame = [&](const double* dmd, const double* desc, int cnt) {
        const double* ap = dmd + (size_t)g * HG_D + rt * 32 + l15;       // A: row = channel (l15), k = point (g)
        const double* bp = desc + (size_t)g * HG_D + ct * 32 + l15;      // B: k = point, column = input
        int p = 0;
        for (; p + 16 <= cnt; p += 16) {              // sixteen loads in flight in front of sixteen products
            double fa[4][2], fb[4][2];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                fa[u][0] = ap[(size_t)(p + 4 * u) * HG_D]; fa[u][1] = ap[(size_t)(p + 4 * u) * HG_D + 16];
                fb[u][0] = bp[(size_t)(p + 4 * u) * HG_D]; fb[u][1] = bp[(size_t)(p + 4 * u) * HG_D + 16];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) step(fa[u][0], fa[u][1], fb[u][0], fb[u][1]);
        }
        for (; p + 4 <= cnt; p += 4) step(ap[(size_t)p * HG_D], ap[(size_t)p * HG_D + 16], bp[(size_t)p * HG_D], bp[(size_t)p * HG_D + 16]);
        if (p < cnt) {
            const bool in = p + g < cnt;
            step(in ? ap[(size_t)p * HG_D] : 0.0, in ? ap[(size_t)p * HG_D + 16] : 0.0, in ? bp[(size_t)p * HG_D] : 0.0, in ? bp[(size_t)p * HG_D + 16] : 0.0);
        }
    };
    frame(a.dmd0 + (size_t)pair * a.N * HG_D, a.desc0 + (size_t)pair * a.N * HG_D, a.N);
    frame(a.dmd1 + (size_t)pair * a.M * HG_D, a.desc1 + (size_t)pair * a.M * HG_D, a.M);
    double* Pp = a.P + (size_t)pair * HG_PART;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) Pp[(rt * 32 + r * 16 + g + 4 * i) * HG_D + ct * 32 + c * 16 + l15] = acc[r][c][i];
    // db: the four quarters of the points (k = g) as (0 + 1) + (2 + 3): the same bits in the four lanes of a channel
    s0 += __shfl_xor(s0, 16, 64);
    s1 += __shfl_xor(s1, 16, 64);
    s0 += __shfl_xor(s0, 32, 64);
    s1 += __shfl_xor(s1, 32, 64);
    if (ct == 0 && g == 0) {
        Pp[HG_D * HG_D + rt * 32 + l15] = s0;
        Pp[HG_D * HG_D + rt * 32 + 16 + l15] = s1;
    }
}

struct HgWs { double *md0, *md1, *dmd0, *dmd1, *P; size_t bytes; };
HgWs hg_carve(void* base, int B, int N, int M) {
    HgWs w{};
    WsCarver c{static_cast<char*>(base)};
    c.take(w.md0, (size_t)B * N * HG_D); c.take(w.md1, (size_t)B * M * HG_D);
    c.take(w.dmd0, (size_t)B * N * HG_D); c.take(w.dmd1, (size_t)B * M * HG_D);
    c.take(w.P, (size_t)B * HG_PART);
    w.bytes = c.bytes;
    return w;
}

// final_proj of one frame: tail64's launch on the frame's rows
int hg_project(const double* desc, const double* W, const double* bias, double* md, int rows, hipStream_t s) {
    const GemmF64Args g{desc, HG_D, HG_D, nullptr, 0, W, HG_D, bias, nullptr, 0, md, HG_D, rows, HG_D, HG_D, 0, nullptr};
    return launch_gemm_f64(g, s);
}

template <int FRAME>
int hg_launch_dmd(const HgArgs& a, hipStream_t s) {
    static std::atomic<unsigned long long> optin{0};
    if (int rc = mdgat_lds_optin(reinterpret_cast<const void*>(hg_dmd_kernel<FRAME>), HG_LDS, optin, "matching head backward LDS")) return rc;
    const int P = FRAME == 0 ? a.N : a.M;
    hipLaunchKernelGGL(hg_dmd_kernel<FRAME>, dim3((unsigned)(a.B * ((P + 63) >> 6))), dim3(256), HG_LDS, s, a);
    return MDGAT_OK;
}

}  // namespace

size_t match_head_f64_workspace_bytes(int B, int N, int M) { return hg_carve(nullptr, B, N, M).bytes; }

int launch_match_head_f64(int B, int N, int M, const double* desc0, const double* desc1, const double* W, const double* bias, double* scores,
                          void* workspace, hipStream_t s) {
    const HgWs w = hg_carve(workspace, B, N, M);
    if (int rc = hg_project(desc0, W, bias, w.md0, B * N, s)) return rc;
    if (int rc = hg_project(desc1, W, bias, w.md1, B * M, s)) return rc;
    const GemmF64Args sg{w.md0, HG_D, HG_D, nullptr, 0, w.md1, HG_D, nullptr, nullptr, 0, scores, M, N, M, HG_D, 0, nullptr,
                         HG_SCALE, B, (long long)N * HG_D, (long long)M * HG_D, (long long)N * M};
    return launch_gemm_f64(sg, s);
}

int launch_match_head_backward_f64(int B, int N, int M, const double* desc0, const double* desc1, const double* W, const double* bias,
                                   const double* dscores, double* ddesc0, double* ddesc1, double* dW, double* dbias, void* workspace, hipStream_t s) {
    const bool red = dW || dbias;
    const bool f0 = ddesc0 || red, f1 = ddesc1 || red;
    if (!f0 && !f1) return MDGAT_OK;
    const HgWs w = hg_carve(workspace, B, N, M);
    if (f1) if (int rc = hg_project(desc0, W, bias, w.md0, B * N, s)) return rc;
    if (f0) if (int rc = hg_project(desc1, W, bias, w.md1, B * M, s)) return rc;
    HgArgs a{};
    a.B = B; a.N = N; a.M = M; a.G = dscores; a.desc0 = desc0; a.desc1 = desc1; a.W = W; a.md0 = w.md0; a.md1 = w.md1;
    a.dmd0 = red ? w.dmd0 : nullptr; a.dmd1 = red ? w.dmd1 : nullptr; a.ddesc0 = ddesc0; a.ddesc1 = ddesc1; a.P = w.P;
    if (f0) if (int rc = hg_launch_dmd<0>(a, s)) return rc;
    if (f1) if (int rc = hg_launch_dmd<1>(a, s)) return rc;
    if (!red) return mdgat_check_hip(hipGetLastError(), "matching head backward launch");
    hipLaunchKernelGGL(hg_dw_kernel, dim3((unsigned)B, 4), dim3(256), 0, s, a);
    return launch_dw_reduce_f64(w.P, B, HG_D * HG_D, HG_D, dW, dbias, s);
}
