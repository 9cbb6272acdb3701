// Device-side helpers shared by the fp64 kernels of the reference-exact mode (f64.hip, layer_f64.hip) and its backward units.
#pragma once
#include <hip/hip_runtime.h>

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// v_mfma_f64_16x16x4_f64: A 16x4, B 4x16 one double per lane (row / col = lane & 15, k = lane >> 4); C/D col = lane & 15,
// row = (lane >> 4) + 4 reg (cdna_hip_programming.md section 3)
__device__ __forceinline__ f64x4 mfma64(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// BatchNorm + ReLU of the training-mode MLP (mlp_grad.hip), z = gamma (y - mean) invstd + beta with a = gamma invstd.  The one place z
// is formed: every kernel that needs z or its sign calls this (the product behind a BN in f64.hip, dW's operand in dw_f64.hip, the
// masks of mlp_grad.hip), so the sign of z is the same everywhere.  A NaN z gives 0 under either set of flags these units are
// compiled with: as a compare and select (NaN > 0 is false) and as v_max_f64 (z comes out of an fma, hence is quiet).
__device__ __forceinline__ double bn_z(double y, double mean, double a, double beta) { return __builtin_fma(y - mean, a, beta); }
__device__ __forceinline__ double bn_relu(double y, double mean, double a, double beta) {
    const double z = bn_z(y, mean, a, beta);
    return z > 0.0 ? z : 0.0;
}

// Range guard of the exact mode, BETWEEN the layers: every output of an fp64 product (q | k | v, the hidden layer before its ReLU,
// the residual stream, the encoder stages) and every message row is tested for "not finite, or |v| >= 2^500" by its exponent field,
// and the call is refused (MDGAT_STATUS_RANGE -> mdgat_async_status / MDGAT.check raise) instead of returning plausible numbers.
// Why here: these files are compiled with -fno-honor-nans, and the reference's NaN propagation (mdgat.py:192-193: a NaN logit makes
// the whole row NaN) is not what the hardware does with one - max(NaN, 0) is 0 in a ReLU, v_max_f64 drops a NaN logit from the row
// maximum and exp_neg clamps it to exp(-745) = 0, so a NaN produced mid-stack (inf - inf in a product or in the online softmax)
// could come out as a finite, wrong message.  With every q, k, v below 2^500 a logit is a sum of 32 products below 2^1000: finite; the
// softmax statistics and P.V of finite logits and values are finite.  So the test on the GEMM outputs (before the ReLU, which
// could swallow a NaN, and after the residual is added) is sufficient, and it sits in the epilogues: two integer instructions per
// output element, none in the product loops.  (The asm hides the value's floating-point origin: a mask test the compiler can trace
// back to a double is recognised as a class test and, under the flag, reduced to "is infinite" - a NaN would pass.)
__device__ __forceinline__ bool f64_out_of_range(double v) {
    unsigned hi = (unsigned)(__builtin_bit_cast(unsigned long long, v) >> 32);
    asm("" : "+v"(hi));
    return (hi & 0x7ff00000u) >= 0x5f300000u;          // biased exponent >= 1523: |v| >= 2^500, inf, NaN
}
__device__ __forceinline__ void f64_raise(unsigned* guard) { if (guard) __hip_atomic_store(guard, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }

// ---- the row helpers and the exponential of the attention kernels (f64.hip, attention_grad.hip) ----
__device__ __forceinline__ double shfl_xor_f64(double v, int m) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)u, m, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(u >> 32), m, 64);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// a value of the four lanes (q, q + 16, q + 32, q + 48) of a row combined
__device__ __forceinline__ double quad_max(double v) { v = fmax(v, shfl_xor_f64(v, 16)); return fmax(v, shfl_xor_f64(v, 32)); }
__device__ __forceinline__ double quad_sum(double v) { v += shfl_xor_f64(v, 16); return v + shfl_xor_f64(v, 32); }

// exp(x) for the softmax numerators: x <= TAU_LAZY (x <= 0 except under the lazy reference of the full-attention loop), -inf for
// masked keys.  Table-driven: x = (256 q + j) ln2 / 256 + r, |r| <= ln2 / 512 = 1.35e-3,
//     exp(x) = 2^q T[j] (1 + r + r^2 / 2 + r^3 / 6 + r^4 / 24),      T[j] = 2^(j / 256) correctly rounded, 2 KB of LDS (exp2_tab256.hpp)
// (truncation r^5 / 120 = 3.8e-17).  n = 256 q + j falls out of the low word of x (256 / ln 2) + 1.5 2^52, the reduction is ONE fma
// against the correctly rounded ln2 / 256 (its rounding error acts like a relative perturbation of x by 2^-53: an ulp of the logit
// itself), the polynomial is a product and three fmas with at most one scalar operand each, one fma scales the table entry and
// v_ldexp_f64 applies 2^q.  Ten fp64 and three integer instructions and a ds_read_b64; the degree-12 polynomial this replaces ran 19 (+ a v_mov_b64 the compiler
// rematerialised for the leading coefficient) - on this part an fp64 vector instruction issues in the slot of a sixteenth of a
// v_mfma_f64_16x16x4 and the two share the pipe (profiles/NOTES_r5.md section 1), so the attention loops are their vector
// instruction count.  Keys masked with -inf get exp(-700) = 1e-304 instead of 0: nothing against a row's largest term, which is 1.
typedef __attribute__((address_space(3))) const double lds_cdouble;
struct ExpConst { double magic; };        // 1.5 2^52 held in a vector register pair for the whole kernel (the fma that uses it has its one
                                          // scalar slot taken by 256 / ln 2; left to the compiler the constant is rematerialised per call)
__device__ __forceinline__ ExpConst exp_const() {
    double m = 0x1.8p+52;
    asm volatile("" : "+v"(m));
    return ExpConst{m};
}
__device__ __forceinline__ double exp_fast(double x, const double* tab_, const ExpConst& ec) {
    lds_cdouble* tab = (lds_cdouble*)tab_;
    x = fmax(x, -700.0);
    double tm, r, a, b, s;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(tm) : "v"(x), "s"(0x1.71547652b82fep+8), "v"(ec.magic));       // x 256 / ln 2 + 1.5 2^52
    const int n = (int)(unsigned)__builtin_bit_cast(unsigned long long, tm);
    const double nd = tm - ec.magic;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(nd), "s"(-0x1.62e42fefa39efp-9), "v"(x));              // x - n ln2 / 256
    const double r2 = r * r;
    asm("v_fma_f64 %0, %1, %2, 0.5" : "=v"(a) : "v"(r), "s"(0x1.5555555555555p-3));                        // 1/2 + r / 6
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(b) : "v"(r2), "s"(0x1.5555555555555p-5), "v"(a));               // ... + r^2 / 24
    s = __builtin_fma(r2, b, r);                                                                          // exp(r) - 1
    const double T = tab[n & 255];
    return ldexp(__builtin_fma(T, s, T), n >> 8);       // (v_ashrrev + v_ldexp_f64; shift, mask and a 64-bit add into T's exponent field: one more, same time)
}
