// The loader's float32 L2 normalisation of one FPFH row (load_data.py:290-292: `np.linalg.norm(descs, axis=1)`, `1 / norm`), numpy's
// arithmetic to the bit: the squares rounded one by one, their sum in the order of numpy's pairwise reduction for 8 <= n <= 128 (eight
// strided partial sums, combined as a tree, the tail added last), a correctly rounded square root and reciprocal, nothing contracted
// into an FMA.  The one body behind the exact mode's assemble kernels (f64.hip) and the encoder's bank form (encoder.hip): the two cannot
// drift.  tests/test_oracle_golden.py pins the order against the reference loader's own outputs.
#pragma once

// 1 / ||f||, f the 33 floats of a row; the caller multiplies (a product of its own, not contracted either).  An all-zero row gives +inf.
// (every operation rounded by itself: plain operators - HIP's __fmul_rn / __fadd_rn ARE plain operators in this toolchain and
// __fsqrt_rn is the native approximation; `/` and __builtin_sqrtf are correctly rounded under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt)
__device__ __forceinline__ float fpfh_inv_norm(const float* f) {
#pragma clang fp contract(off)
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = f[j] * f[j];
#pragma unroll
    for (int i = 8; i < 32; i += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float q = f[i + j] * f[i + j]; r[j] = r[j] + q; }
    float sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    const float q = f[32] * f[32];
    sum = sum + q;
    return 1.f / __builtin_sqrtf(sum);
}
