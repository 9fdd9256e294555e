// mxv_sum_tree.hpp — the fixed sum tree of the loss headers (include/mxv_ppo.h states it, mxv_dqn.h and mxv_c51.h refer to it; DESIGN.md
// §15, §17, §20), written once: the operations, the xor butterfly of a wave, the four waves of a workgroup, the levels of 1024 partials
// per workgroup, the float32 rounding that writes one NaN pattern — and, on the host, the workspace the levels need and their launches.
// mxv_ppo.hip, mxv_dqn.hip and mxv_c51.hip take all of it; mxv_norm.hip takes wave_tree / four_waves (its [K][leaves][V] levels with a
// run-time V are its own).  tests/norm_tree_host.py and tests/ppo_host.py restate the tree in NumPy.  Float64, one rounding per
// operation (every file that includes this is built with -ffp-contract=off).  The host helpers are templates over the caller's
// policy_host::Call and its own argument struct, so this header needs no other of the library's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mxv.h"

namespace mxv {
namespace sum_tree {

constexpr int kLeafRows = 1024;      // rows per leaf: four per lane of a workgroup of 256
constexpr int kTreeFan = 1024;       // partials folded per workgroup per tree level: four per lane

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
// permutes of the DPP unit — lane 7 - i of the half row, lane 15 - i of the row — deliver what lane ^ 4 (lane ^ 8) holds.  Stages 16,
// 32: gfx950's v_permlane16_swap / v_permlane32_swap.  Op commutes exactly, so the value is that of the lane ^ (1 << b) form of the
// rule, bit for bit.  No LDS round trips: this form replaced the six ds_bpermute stages of a __shfl_xor butterfly, which were slower
// (profiles/r4/r4n_normalize_variants.txt).
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

// the four waves of a workgroup, each having left its values in a row of LD doubles of LDS: (w0 + w1) + (w2 + w3)
template <class Op, int LD>
__device__ __forceinline__ double four_waves(const double (*sm)[LD], int v) {
    return Op::op(Op::op(sm[0][v], sm[1][v]), Op::op(sm[2][v], sm[3][v]));
}

// the value of lane `lane` (uniform) in every lane
__device__ __forceinline__ double lane_value(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// the four consecutive partials a lane takes at a level: (a0 + a1) + (a2 + a3)
template <class Op>
__device__ __forceinline__ double four_partials(const double (&a)[4]) {
    return Op::op(Op::op(a[0], a[1]), Op::op(a[2], a[3]));
}

// A lane's partials l0 .. l0 + 3 of value v out of in[count][V] (a missing one is the identity: an odd leftover passes through
// unchanged, as in a pairwise tree), folded, then the butterfly of the wave.
template <class Op, int V>
__device__ __forceinline__ double group_value(const double *in, int64_t count, int64_t l0, int v) {
    double a[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = l0 + i < count ? in[(l0 + i) * V + v] : Op::identity();
    return wave_tree<Op>(four_partials<Op>(a));
}

// The helpers below take a file's set of partials as a class K: K::V values per leaf, K::is_min(v) / K::is_max(v) name those that are a
// minimum / a maximum, every other one is a sum.  `sm` is the kernel's own __shared__ array of one row of LD >= K::V doubles per wave.

// the operation of partial v over the four waves
template <class K, int LD>
__device__ __forceinline__ double combine(const double (*sm)[LD], int v) {
    return K::is_min(v) ? four_waves<Min, LD>(sm, v) : K::is_max(v) ? four_waves<Max, LD>(sm, v) : four_waves<Add, LD>(sm, v);
}

// a leaf: lane 0 of every wave leaves the wave's N values (of the butterfly) in its row of sm; then the barrier
template <int N, int LD>
__device__ __forceinline__ void leave_wave_values(double (*sm)[LD], const double (&t)[N]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int v = 0; v < N; ++v) sm[wave][v] = t[v];
    }
    __syncthreads();
}

// a level: workgroup g folds partials g * 1024 .. of in[count][K::V], four per lane, and leaves every wave's values in sm; then the barrier
template <class K, int LD>
__device__ __forceinline__ void fold_level(double (*sm)[LD], const double *in, int64_t count) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t l0 = (int64_t)blockIdx.x * kTreeFan + (int64_t)tid * 4;
#pragma unroll
    for (int v = 0; v < K::V; ++v) {
        const double x = K::is_min(v)   ? group_value<Min, K::V>(in, count, l0, v)
                         : K::is_max(v) ? group_value<Max, K::V>(in, count, l0, v)
                                        : group_value<Add, K::V>(in, count, l0, v);
        if (lane == 0) sm[wave][v] = x;
    }
    __syncthreads();
}

// the first K::V lanes write the workgroup's values: row blockIdx.x of out[][K::V]
template <class K, int LD>
__device__ __forceinline__ void write_partials(const double (*sm)[LD], double *out) {
    const int tid = threadIdx.x;
    if (tid < K::V) out[(int64_t)blockIdx.x * K::V + tid] = combine<K, LD>(sm, tid);
}

// ---- host ----
inline int64_t leaves_of(int64_t M) { return (M + kLeafRows - 1) / kLeafRows; }

// workspace rows (of V doubles each) of a batch of M rows: the leaves, and every level of the tree that is not the last
inline int64_t workspace_slots(int64_t M) {
    int64_t count = leaves_of(M), slots = count;
    while (count > kTreeFan) {
        count = (count + kTreeFan - 1) / kTreeFan;
        slots += count;
    }
    return slots;
}

// `need` = what `bytes_fn`(M), the entry point's own mxv_*_workspace_bytes, returns
template <class Call>
int check_workspace(const Call &call, const char *bytes_fn, int64_t M, const void *workspace, int64_t workspace_bytes, int64_t need) {
    if (!workspace) return call.bad("%s: workspace pointer is NULL", call.api);
    if (workspace_bytes < need)
        return call.bad("%s: workspace_bytes = %lld is below %s(%lld) = %lld", call.api, (long long)workspace_bytes, bytes_fn, (long long)M, (long long)need);
    return MXV_OK;
}

// The levels of the tree over `leaves` partials of V values at the start of `ws`, every level's output behind the one before:
// `kernel`(t) with t.in, t.count, t.out and t.last set, one workgroup per group of kTreeFan partials; the last level is one group.
template <class Call, class TreeArgs>
int run_tree(const Call &call, const void *kernel, int V, TreeArgs t, double *ws, int64_t leaves, void *stream) {
    int64_t count = leaves, offset = leaves * V;
    const double *in = ws;
    for (;;) {
        const int64_t groups = (count + kTreeFan - 1) / kTreeFan;
        t.in = in; t.count = count; t.last = groups == 1; t.out = t.last ? nullptr : ws + offset;
        if (int rc = call.launch_blocks(kernel, t, groups, stream)) return rc;
        if (t.last) return MXV_OK;
        in = t.out; offset += groups * V; count = groups;
    }
}

}  // namespace sum_tree
}  // namespace mxv
