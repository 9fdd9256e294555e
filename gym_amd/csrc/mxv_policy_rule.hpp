// mxv_policy_rule.hpp — the bit-defined rule of the policy heads (include/mxv_policy.h, include/mxv_policy_eval.h),
// written once: its constants, EXP, LOG, SINCOS2PI, the Box-Muller pair, what makes a row degenerate, the limits and the launch shape.
//
// mxv_policy.hip, mxv_gaussian.hip and mxv_policy_eval.hip all include this text and define none of it themselves
// (tests/test_policy_host.py, test_gaussian_host.py, test_policy_eval_host.py): a stored action re-evaluated under the head that drew it
// gets the sampler's bits because both ran these lines, not copies of them.  float64, one rounding per operation (every file that includes
// this is built with -ffp-contract=off), no libm call, no __expf.  Everything is a select: no divergent branch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mxv_device.hpp"

namespace mxv {
namespace rule {

// ---- launch shape: workgroups of kThreads lanes, one row per lane, each workgroup striding over tiles of kThreads rows ----
constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;    // 256 CUs x 8 workgroups of 4 waves = every wave slot

// ---- limits ----
constexpr int kMaxActions = 64;
constexpr int kMaxDim = 4;
constexpr int64_t kMaxElems = (int64_t)1 << 40;
constexpr double kExpCut = -708.0;
constexpr double kLogStdMax = 80.0;        // sigma = EXP(+-80) is a normal float32

// ---- the constants of the rule: the output of tools/gaussian_coefficients.py, verbatim (tools/policy_coefficients.py prints its first six lines) ----
constexpr double kInvLn2 = 0x1.71547652b82fep+0;
constexpr double kLn2Hi = 0x1.62e42fee00000p-1;
constexpr double kLn2Lo = 0x1.a39ef35793c76p-33;
constexpr double kSqrtHalf = 0x1.6a09e667f3bcdp-1;
constexpr double kExpC[14] = {0x1.0000000000000p+0, 0x1.0000000000000p+0, 0x1.0000000000000p-1, 0x1.5555555555555p-3, 0x1.5555555555555p-5, 0x1.1111111111111p-7, 0x1.6c16c16c16c17p-10, 0x1.a01a01a01a01ap-13, 0x1.a01a01a01a01ap-16, 0x1.71de3a556c734p-19, 0x1.27e4fb7789f5cp-22, 0x1.ae64567f544e4p-26, 0x1.1eed8eff8d898p-29, 0x1.6124613a86d09p-33};
constexpr double kLogC[12] = {0x1.0000000000000p+0, 0x1.5555555555555p-2, 0x1.999999999999ap-3, 0x1.2492492492492p-3, 0x1.c71c71c71c71cp-4, 0x1.745d1745d1746p-4, 0x1.3b13b13b13b14p-4, 0x1.1111111111111p-4, 0x1.e1e1e1e1e1e1ep-5, 0x1.af286bca1af28p-5, 0x1.8618618618618p-5, 0x1.642c8590b2164p-5};
constexpr double kPio2Hi = 0x1.921fa00000000p+0;
constexpr double kPio2Lo = 0x1.54442d184698ap-20;
constexpr double kHalfLog2Pi = 0x1.d67f1c864beb5p-1;
constexpr double kEntC = 0x1.6b3f8e4325f5ap+0;
constexpr double kSinC[9] = {-0x1.5555555555555p-3, 0x1.1111111111111p-7, -0x1.a01a01a01a01ap-13, 0x1.71de3a556c734p-19, -0x1.ae64567f544e4p-26, 0x1.6124613a86d09p-33, -0x1.ae7f3e733b81fp-41, 0x1.952c77030ad4ap-49, -0x1.2f49b46814157p-57};
constexpr double kCosC[10] = {-0x1.0000000000000p-1, 0x1.5555555555555p-5, -0x1.6c16c16c16c17p-10, 0x1.a01a01a01a01ap-16, -0x1.27e4fb7789f5cp-22, 0x1.1eed8eff8d898p-29, -0x1.93974a8c07c9dp-37, 0x1.ae7f3e733b81fp-45, -0x1.6827863b97d97p-53, 0x1.e542ba4020225p-62};
// ---- end of the generated block ----

__device__ __forceinline__ double exp_rule(double d) {   // |d| <= 80 or -708 <= d <= 0
    const double k = __builtin_rint(d * kInvLn2);
    const double r = (d - k * kLn2Hi) - k * kLn2Lo;
    double p = kExpC[13];
#pragma unroll
    for (int j = 12; j >= 0; --j) p = p * r + kExpC[j];
    return __builtin_ldexp(p, (int)k);
}

// e_a of a categorical row: EXP(d), and exactly 0 below the cut
__device__ __forceinline__ double e_of(double d) { return d < kExpCut ? 0.0 : exp_rule(d < kExpCut ? 0.0 : d); }

__device__ __forceinline__ double log_rule(double S) {   // 2^-33 <= S <= 64
    int e;
    double f = __builtin_frexp(S, &e);
    const bool low = f < kSqrtHalf;
    f = low ? f * 2.0 : f;
    e = low ? e - 1 : e;
    const double ed = (double)e;
    const double s = (f - 1.0) / (f + 1.0);
    const double z = s * s;
    double p = kLogC[11];
#pragma unroll
    for (int j = 10; j >= 0; --j) p = p * z + kLogC[j];
    return ((ed * kLn2Hi) + (2.0 * s) * p) + ed * kLn2Lo;
}

// (sin, cos) of 2 pi (w + 0.5) 2^-32
__device__ __forceinline__ void sincos2pi_rule(uint32_t w, double &sn, double &cs) {
    const double t = 4.0 * mxv::u01(w);
    const double k = __builtin_rint(t);         // 0..4, never a tie
    const double f = t - k;                     // exact
    const double r = f * kPio2Hi + f * kPio2Lo; // the first product is exact
    const double z = r * r;
    double p = kSinC[8];
#pragma unroll
    for (int j = 7; j >= 0; --j) p = p * z + kSinC[j];
    const double s = r + r * (z * p);
    double q = kCosC[9];
#pragma unroll
    for (int j = 8; j >= 0; --j) q = q * z + kCosC[j];
    const double c = 1.0 + z * q;
    const int quad = (int)k;
    const double a = (quad & 1) ? c : s, b = (quad & 1) ? s : c;      // two-way selects: the table of the rule without a branch
    sn = (quad & 2) ? -a : a;
    cs = ((quad + 1) & 2) ? -b : b;
}

__device__ __forceinline__ void normal_pair(uint32_t wa, uint32_t wb, double &z_even, double &z_odd) {
    const double rad = sqrt(-2.0 * log_rule(mxv::u01(wa)));
    double sn, cs;
    sincos2pi_rule(wb, sn, cs);
    z_even = rad * cs;
    z_odd = rad * sn;
}

// what makes a row degenerate
__device__ __forceinline__ bool bad_logit(float x) { return x != x || x == __builtin_inff(); }                            // NaN, +Inf
__device__ __forceinline__ bool bad_mean(float x) { return !(__builtin_fabsf(x) < __builtin_inff()); }                     // NaN, +-Inf
__device__ __forceinline__ bool bad_log_std(float x) { return !(__builtin_fabsf(x) <= (float)kLogStdMax); }              // NaN, |x| > 80

}  // namespace rule
}  // namespace mxv
