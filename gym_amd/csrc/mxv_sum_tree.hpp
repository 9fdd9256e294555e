// mxv_sum_tree.hpp — the fixed sum tree of the loss headers (the PPO loss header states it), written once for
// the files that are new since: the operations, the xor butterfly of a wave, the four waves of a workgroup, and the float32 rounding
// that writes one NaN pattern.  mxv_ppo.hip and mxv_dqn.hip keep their own copies (their resource tests pin their text); mxv_c51.hip
// includes this.  Device code only; float64, one rounding per operation (every file that includes this is built with
// -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mxv {
namespace sum_tree {

__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7FF8000000000000ll); }
// round to nearest even; every NaN leaves as the one pattern
__device__ __forceinline__ float to_f32(double x) {
    const float y = (float)x;
    return y != y ? __uint_as_float(0x7FC00000u) : y;
}

struct Add {
    static __device__ __forceinline__ double identity() { return 0.0; }
    static __device__ __forceinline__ double op(double a, double b) { return a + b; }
};
struct Min {   // operands are never NaN (a NaN is skipped at its row); two zeros of either sign are one value: the finish writes +0.0
    static __device__ __forceinline__ double identity() { return (double)__builtin_inff(); }
    static __device__ __forceinline__ double op(double a, double b) { return b < a ? b : a; }
};
struct Max {
    static __device__ __forceinline__ double identity() { return -(double)__builtin_inff(); }
    static __device__ __forceinline__ double op(double a, double b) { return b > a ? b : a; }
};

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}

// The xor butterfly over lane bits 0..5 = the pairwise tree over the lane index of a wave; every lane ends with the tree's value.
// Stages 1, 2: quad permutes.  Stages 4, 8: after them every lane of a quad (of a half row) holds the same partial, so the mirror
// permutes deliver what lane ^ 4 (lane ^ 8) holds.  Stages 16, 32: v_permlane16_swap / v_permlane32_swap.  Op commutes, so the value
// is that of the lane ^ (1 << b) form of the rule.
template <class Op>
__device__ __forceinline__ double wave_tree(double v) {
    v = Op::op(v, dpp_f64<0xB1>(v));     // quad_perm [1, 0, 3, 2]
    v = Op::op(v, dpp_f64<0x4E>(v));     // quad_perm [2, 3, 0, 1]
    v = Op::op(v, dpp_f64<0x141>(v));    // row_half_mirror
    v = Op::op(v, dpp_f64<0x140>(v));    // row_mirror
    {
        const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
        const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        v = Op::op(__hiloint2double((int)b[0], (int)a[0]), __hiloint2double((int)b[1], (int)a[1]));   // rows (0, 1), (2, 3)
    }
    {
        const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
        const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false), b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        v = Op::op(__hiloint2double((int)b[0], (int)a[0]), __hiloint2double((int)b[1], (int)a[1]));   // lower half, upper half
    }
    return v;
}

// the four waves of a workgroup, each having left its V values in LDS: (w0 + w1) + (w2 + w3)
template <class Op, int V>
__device__ __forceinline__ double four_waves(const double (*sm)[V], int v) {
    return Op::op(Op::op(sm[0][v], sm[1][v]), Op::op(sm[2][v], sm[3][v]));
}

// the value of lane `lane` (uniform) in every lane
__device__ __forceinline__ double lane_value(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

}  // namespace sum_tree
}  // namespace mxv
