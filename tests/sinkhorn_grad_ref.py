"""fp64 restatement of the gradient of log_optimal_transport (models/mdgat.py:279-308) in the scaling form, the yardstick of
csrc/sinkhorn_grad.hip.  CPU, torch float64.

C is the (N+1) x (M+1) coupling matrix (scores, the bin score alpha on the border), r_i = max_j C_ij, K = exp(C - r).  The forward
runs a_t = mu / (K b_{t-1}), b_t = nu / (K^T a_t) from b_0 = 1 (u_t = log a_t - r, v_t = log b_t).  With G = dL/dZ, gv_T = colsum(G),
d = rowsum(G), for t = T .. 1:

    gu_t     = [t == T] d - a_t * K (b_t * gv_t / nu)
    gv_{t-1} = - b_{t-1} * K^T (a_t * gu_t / mu)            (not needed at t = 1: v_0 = 0 is a constant)

and dC = G - K * sum_t [ x_t b_{t-1}^T + a_t y_t^T ] with x_t = a_t * gu_t / mu, y_t = b_t * gv_t / nu - a rank-2T sum, which the
kernel forms as one GEMM.  dscores = dC[:, :N, :M]; dalpha = the sum of dC over the dustbin row and column (corner once)."""
import math

import torch


def couplings(scores, alpha):
    B, N, M = scores.shape
    C = torch.full((B, N + 1, M + 1), float(alpha), dtype=torch.float64)
    C[:, :N, :M] = scores.to(torch.float64)
    return C


def marginals(N, M):
    nm = float(N + M)
    mu = torch.full((N + 1,), 1.0 / nm, dtype=torch.float64)
    mu[N] = M / nm
    nu = torch.full((M + 1,), 1.0 / nm, dtype=torch.float64)
    nu[M] = N / nm
    return mu, nu


def sinkhorn_grad(scores, alpha, iters, dZ):
    """scores [B, N, M], alpha (float), iters >= 0, dZ [B, N+1, M+1] -> (dscores [B, N, M], dalpha [B]) in float64."""
    scores = torch.as_tensor(scores, dtype=torch.float64)
    G = torch.as_tensor(dZ, dtype=torch.float64)
    B, N, M = scores.shape
    C = couplings(scores, alpha)
    r = C.max(dim=2, keepdim=True).values
    K = torch.exp(C - r)                                    # [B, N+1, M+1]
    mu, nu = marginals(N, M)
    T = int(iters)
    a = [None] * (T + 1)
    b = [None] * (T + 1)
    b[0] = torch.ones(B, M + 1, dtype=torch.float64)
    for t in range(1, T + 1):
        a[t] = mu / torch.einsum('bij,bj->bi', K, b[t - 1])
        b[t] = nu / torch.einsum('bij,bi->bj', K, a[t])
    S = torch.zeros_like(K)
    if T > 0:
        gv = G.sum(dim=1)
        d = G.sum(dim=2)
        for t in range(T, 0, -1):
            y = b[t] * gv / nu
            gu = (d if t == T else 0.0) - a[t] * torch.einsum('bij,bj->bi', K, y)
            x = a[t] * gu / mu
            S += x[:, :, None] * b[t - 1][:, None, :] + a[t][:, :, None] * y[:, None, :]
            if t > 1:
                gv = -b[t - 1] * torch.einsum('bij,bi->bj', K, x)
    dC = G - K * S
    dscores = dC[:, :N, :M].clone()
    dalpha = dC[:, N, :].sum(dim=1) + dC[:, :N, M].sum(dim=1)
    return dscores, dalpha


def oracle_grad(scores, alpha, iters, dZ):
    """The same gradient by torch autograd through the fp64 oracle (100 unrolled logsumexp iterations; small shapes only)."""
    from oracle import mdgat_oracle as O
    s = torch.as_tensor(scores, dtype=torch.float64).clone().requires_grad_(True)
    al = torch.tensor(float(alpha), dtype=torch.float64, requires_grad=True)
    Z = O.log_optimal_transport(s, al, int(iters))
    (Z * torch.as_tensor(dZ, dtype=torch.float64)).sum().backward()
    return s.grad.detach(), al.grad.detach()


# ---- which skg_reverse_kernel<NC2> a shape runs (the launcher of csrc/sinkhorn_grad.hip), for the coverage check of the GPU tests ----
REVERSE_VARIANTS = (5, 9, 17)


def reverse_dispatch(M):
    """(Mp, nc2, variant) for M columns: Mp = M + 1 rounded up to 128, nc2 = Mp / 128 column pairs per lane, and the instantiation
    skg_reverse_kernel<variant> the launcher picks (the first with nc2 <= variant).  Column pairs c >= nc2 are masked when nc2 < variant."""
    Mp = (M + 1 + 127) // 128 * 128
    nc2 = Mp // 128
    for v in REVERSE_VARIANTS:
        if nc2 <= v:
            return Mp, nc2, v
    raise ValueError(f'M = {M}: beyond the backward\'s {128 * REVERSE_VARIANTS[-1] - 1} columns')


# (B, N, M, T) of tests/test_gpu_sinkhorn_grad.py::test_fp64_reverse_variants: every instantiation with and without masking, both sides
# of each switch (M = 639 | 640, 1151 | 1152, 2047 | 2048), N + 1 and M + 1 on and off multiples of the coupling kernel's 64 x 64 tiles,
# N on and off the 32-row slabs, odd and even T (2T = 2 mod 4: the coupling kernel's tail), one row, one column.
# tests/test_sinkhorn_grad_ref.py::test_reverse_variant_cases_cover_every_path keeps this list honest.
VARIANT_CASES = (
    (2, 63, 639, 7),
    (1, 64, 640, 20),
    (1, 127, 1151, 1),
    (1, 128, 1152, 100),
    (1, 300, 2047, 7),
    (1, 191, 2048, 200),
    (1, 1, 2048, 5),
    (1, 2175, 1, 20),
)


def max_rel(a, b):
    """max |a - b| / max |b| (1 where b is all zero and a is not)."""
    a = torch.as_tensor(a, dtype=torch.float64)
    b = torch.as_tensor(b, dtype=torch.float64)
    den = b.abs().max().item()
    num = (a - b).abs().max().item() if a.numel() else 0.0
    return num / den if den > 0 else (0.0 if num == 0 else math.inf)
