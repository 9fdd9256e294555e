// mxv_divide.hpp — IEEE fp64 division by a divisor shared across several quotients, and the operand guards that say where the
// short form is exact.  Included by mxv_device.hpp (Acrobot's d1 / den2 and CartPole's ta_den on the fused rollout) and by
// mxv_subnorm.hip (the per-sub-env RunningMeanStd update); tests/device_math/primitives.hip runs these very functions against numpy `/`
// (tests/test_gpu_device_math.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mxv {

// The compiler's IEEE fp64 division is v_div_scale x2, v_rcp_f64, two Newton steps on the reciprocal, q0 = x*r, rem = fma(-d, q0, x),
// v_div_fmas (= fma(rem, r, q0)), v_div_fixup.  For operands that need no scaling or fix-up (normal, exponents far from the limits,
// x != -0) the scale factors are 1 and the fix-up is the identity, so running the reciprocal part once and the 3-instruction tail per
// dividend reproduces `/` bit for bit (tests/test_gpu_device_math.py: random and near-midpoint quotients over the divisor ranges the
// kernels feed it).
__device__ __forceinline__ double refined_rcp(double d) {
    double r = __builtin_amdgcn_rcp(d);
    double e = __fma_rn(-d, r, 1.0);
    r = __fma_rn(r, e, r);
    e = __fma_rn(-d, r, 1.0);
    return __fma_rn(r, e, r);
}
__device__ __forceinline__ double div_with_rcp(double x, double d, double r) {
    const double q0 = x * r;
    return __fma_rn(__fma_rn(-d, q0, x), r, q0);
}

// The same tail plus v_div_fixup (IEEE's answers for 0 / Inf / NaN operands, the identity otherwise): the same bits as `/` whenever the
// guards below hold.  Operands outside them (a dividend outside 2^-723 .. 2^677, a divisor outside 2^-64 .. 2^64 — v_div_scale rescales
// when the dividend's exponent is tiny, the exponents differ by 768 or more, or the quotient would be subnormal) must take the plain `/`.
// (v_frexp_exp_i32_f64 answers 0 for zero, Inf and NaN — v_div_fixup's business, accepted — and the true exponent for subnormals: one
// instruction, an add and an unsigned compare per test.)
__device__ __forceinline__ double div_shared(double x, double d, double r) {
    const double q0 = x * r;
    return __builtin_amdgcn_div_fixup(__fma_rn(__fma_rn(-d, q0, x), r, q0), d, x);
}
__device__ __forceinline__ bool plain_operand(double x) {   // finite non-zero needs 2^-723 <= |x| < 2^678
    return (uint32_t)(__builtin_amdgcn_frexp_exp(x) + 722) < 1401u;
}
// delta = row - mean: with |delta| in 2^-300 .. 2^300 (or 0 / Inf / NaN) and count in 2^-64 .. 2^64 (or 0), square(delta) * count lies in
// 2^-664 .. 2^664 (or is 0 / Inf / NaN): plain by construction, no test of its own.
__device__ __forceinline__ bool plain_delta(double x) { return (uint32_t)(__builtin_amdgcn_frexp_exp(x) + 299) < 601u; }
__device__ __forceinline__ bool plain_divisor(double d) {   // count + 1: 1.0001 .. 2^53 in any real run
    const uint32_t e = ((uint32_t)__double2hiint(d) >> 20) & 0x7ffu;
    return e - 959u < 129u;
}

}  // namespace mxv
