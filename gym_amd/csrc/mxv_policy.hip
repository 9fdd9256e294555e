// mxv_policy.hip — categorical draws from a policy's logits, with log-probabilities and entropies (include/mxv_policy.h).
//
// The result is defined bit for bit by the rule in the header: float64, one rounding per operation (this file is built with
// -ffp-contract=off like the rest of the library), EXP and LOG as the operation sequences written there — no libm call, no __expf.
// Their one text, with the constants, the limits and the launch shape, is mxv_policy_rule.hpp, which mxv_gaussian.hip and
// mxv_policy_eval.hip include too; the argument checks and the error slot are those of mxv_policy_host.hpp.
//
// Shape of the kernel (arithmetic bound: ~45 fp64 operations per logit and a Philox call per env against 4 A + 16 bytes):
//   * one lane owns one env.  For A = 2, 3, 4, 6 — the engine's own action counts — a straight-line instantiation holds the row, its
//     d_a and e_a in registers and evaluates EXP once per logit.  A row is one 4 A-byte run; the lane reads it with a single access of A
//     dwords (dwordx4 + dwordx2 for A = 6; the device takes them at any 4-byte boundary), so that with ld == A a wave's loads cover one
//     dense run of 256 A bytes.
//     Every other A runs a loop over the row that evaluates EXP twice per logit (once for S and T, once for the running sum that
//     finds the action) and keeps nothing per logit: no scratch at any A (tests/test_policy_resources.py).
//   * one Philox4x32-10 call per lane: counter (G >> 2, t), word G & 3.  env_offset may be anything, so the four envs of a counter need
//     not sit in one aligned group of lanes; no lane shares a call.
//   * t comes from the argument or, with step_dev, from device memory (a uniform load); mxv::launch_add_word behind the kernel advances it.
//   * no atomics, no LDS, no inline assembly.  Grid: at most kMaxBlocks workgroups of 256 lanes, each striding over tiles of 256 envs.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/mxv_policy.h"
#include "mxv_policy_host.hpp"
#include "mxv_policy_rule.hpp"

namespace {

using namespace mxv::rule;
using namespace mxv::policy_host;

constexpr uint32_t kStreamPolicy = 7u;   // 1-6: mxv_device.hpp (kStream*), mxv_tab.hip, mxv_bj.hip

struct PolicyArgs {
    const float *logits;
    const uint64_t *step_dev;
    void *actions;
    float *log_prob, *entropy;
    int64_t N, ld, tiles;
    uint64_t seed, env_offset, step;
    int32_t A, i64;
};

__device__ __forceinline__ float to_f32(double x) { return (float)x; }   // round to nearest even; the NaN rows are written as a pattern

struct Draw {
    int32_t action;
    double d_action, S, T;
    bool degenerate;
};

template <int AT>
__device__ __forceinline__ Draw draw_straight(const float *row, double u) {
    float x[AT];
#pragma unroll
    for (int a = 0; a < AT; ++a) x[a] = row[a];      // merged into one access of AT dwords (two for AT = 6): 4-byte alignment suffices
    Draw r;
    r.degenerate = false;
    double m = (double)x[0];
#pragma unroll
    for (int a = 0; a < AT; ++a) {
        r.degenerate |= bad_logit(x[a]);
        if (a > 0) m = (double)x[a] > m ? (double)x[a] : m;
    }
    r.degenerate |= m == -(double)__builtin_inff();
    double d[AT], c[AT];
    double acc = 0.0, T = 0.0;
#pragma unroll
    for (int a = 0; a < AT; ++a) {
        d[a] = r.degenerate ? 0.0 : (double)x[a] - m;      // a degenerate row's results are replaced: keep its arithmetic finite
        const double e = e_of(d[a]);
        acc = acc + e;
        c[a] = acc;
        T = e == 0.0 ? T : T + e * d[a];
    }
    const double thr = u * acc;
    r.action = AT - 1;
    r.d_action = d[AT - 1];
#pragma unroll
    for (int a = AT - 2; a >= 0; --a) {
        const bool hit = c[a] > thr;
        r.action = hit ? a : r.action;
        r.d_action = hit ? d[a] : r.d_action;
    }
    r.S = acc;
    r.T = T;
    return r;
}

__device__ __forceinline__ Draw draw_loop(const float *row, int A, double u) {
    Draw r;
    r.degenerate = false;
    double m = (double)row[0];
    for (int a = 0; a < A; ++a) {
        const float x = row[a];
        r.degenerate |= bad_logit(x);
        if (a > 0) m = (double)x > m ? (double)x : m;
    }
    r.degenerate |= m == -(double)__builtin_inff();
    double acc = 0.0, T = 0.0;
    for (int a = 0; a < A; ++a) {
        const double d = r.degenerate ? 0.0 : (double)row[a] - m;      // a degenerate row's results are replaced: keep its arithmetic finite
        const double e = e_of(d);
        acc = acc + e;
        T = e == 0.0 ? T : T + e * d;
    }
    r.S = acc;
    r.T = T;
    const double thr = u * acc;
    // the same sums again, in the same order: c_a has the same bits as above.  Stops at the first c_a > thr.
    r.action = A - 1;
    r.d_action = 0.0;
    double c = 0.0;
    bool found = false;
    for (int a = 0; a < A && !found; ++a) {
        const double d = r.degenerate ? 0.0 : (double)row[a] - m;
        c = c + e_of(d);
        if (c > thr || a == A - 1) {
            found = true;
            r.action = a;
            r.d_action = d;
        }
    }
    return r;
}

template <int AT>
__global__ void __launch_bounds__(kThreads) policy_kernel(const PolicyArgs a) {
    const uint64_t t = a.step_dev ? *a.step_dev : a.step;
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t i = tile * kThreads + threadIdx.x;
        if (i >= a.N) continue;
        const uint64_t G = a.env_offset + (uint64_t)i, g = G >> 2;
        mxv::U4 ctr;
        ctr.x = (uint32_t)g;
        ctr.y = (uint32_t)(g >> 32);
        ctr.z = (uint32_t)t;
        ctr.w = ((uint32_t)(t >> 32) & 0x0fffffffu) | (kStreamPolicy << 28);
        const mxv::U4 w4 = mxv::philox4x32_10(ctr, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        const uint32_t lane = (uint32_t)G & 3u;
        const uint32_t w = lane == 0 ? w4.x : lane == 1 ? w4.y : lane == 2 ? w4.z : w4.w;
        const double u = mxv::u01(w);
        const float *row = a.logits + i * a.ld;
        Draw r;
        if constexpr (AT > 0) r = draw_straight<AT>(row, u);
        else r = draw_loop(row, a.A, u);
        const int32_t action = r.degenerate ? 0 : r.action;
        if (a.i64) static_cast<int64_t *>(a.actions)[i] = action;
        else static_cast<int32_t *>(a.actions)[i] = action;
        if (a.log_prob || a.entropy) {
            const float nan = __uint_as_float(0x7FC00000u);
            const double S = r.degenerate ? 1.0 : r.S;     // keeps LOG and the division inside their ranges; the row's results are NaN
            const double L = log_rule(S);
            if (a.log_prob) a.log_prob[i] = r.degenerate ? nan : to_f32(r.d_action - L);
            if (a.entropy) a.entropy[i] = r.degenerate ? nan : to_f32(L - r.T / S);
        }
    }
}

struct LastLaunch {   // of the calling thread (mxv_policy_last_launch)
    int32_t envs_per_lane = 0, specialised_A = 0;
    uint32_t grid = 0;
};
LastLaunch &last_launch() {
    thread_local LastLaunch l;
    return l;
}

template <int AT>
const void *kernel_of() {
    return reinterpret_cast<const void *>(&policy_kernel<AT>);
}

}  // namespace

extern "C" {

int mxv_policy_sample_categorical(void *stream, int64_t N, int32_t A, const float *logits_dev, int64_t ld, uint64_t seed,
                                  uint64_t env_offset, uint64_t step, uint64_t *step_dev, void *actions_dev, int32_t actions_are_i64,
                                  float *log_prob_dev, float *entropy_dev) {
    const Call<mxv::PolicyCall> call{"mxv_policy_sample_categorical", 'N'};
    if (int rc = call.check_cat(N, A, logits_dev, ld, actions_dev)) return rc;
    const uint64_t ab = actions_are_i64 ? 8 : 4;
    const Range ins[] = {{"logits", (uintptr_t)logits_dev, rows_bytes(N, ld, A), 4}, {"step_dev", (uintptr_t)step_dev, 8, 8, ""}};
    const Range outs[] = {{"actions", (uintptr_t)actions_dev, (uint64_t)N * ab, ab}, {"log_prob", (uintptr_t)log_prob_dev, (uint64_t)N * 4, 4},
                          {"entropy", (uintptr_t)entropy_dev, (uint64_t)N * 4, 4}};
    if (int rc = call.check_ranges(N, ins, 2, outs, 3)) return rc;
    PolicyArgs a;
    a.logits = logits_dev; a.step_dev = step_dev; a.actions = actions_dev; a.log_prob = log_prob_dev; a.entropy = entropy_dev;
    a.N = N; a.ld = ld; a.tiles = (N + kThreads - 1) / kThreads;
    a.seed = seed; a.env_offset = env_offset; a.step = step;
    a.A = A; a.i64 = actions_are_i64 ? 1 : 0;
    const void *kernel;
    int32_t spec = A;
    switch (A) {
        case 2: kernel = kernel_of<2>(); break;
        case 3: kernel = kernel_of<3>(); break;
        case 4: kernel = kernel_of<4>(); break;
        case 6: kernel = kernel_of<6>(); break;
        default: kernel = kernel_of<0>(); spec = 0; break;
    }
    if (int rc = call.launch(kernel, a, stream)) return rc;
    if (int rc = call.advance(step_dev, stream)) return rc;
    last_launch() = LastLaunch{1, spec, grid_of(a.tiles).x};
    return MXV_OK;
}

const char *mxv_policy_last_error(void) { return mxv::last_error<mxv::PolicyCall>(nullptr); }

int mxv_policy_last_launch(int32_t *envs_per_lane, int32_t *specialised_A, uint32_t *grid) {
    if (!envs_per_lane || !specialised_A || !grid) return mxv::fail<mxv::PolicyCall>(nullptr, MXV_ERR_INVALID_ARG, "mxv_policy_last_launch: output pointer is NULL");
    *envs_per_lane = last_launch().envs_per_lane;
    *specialised_A = last_launch().specialised_A;
    *grid = last_launch().grid;
    return MXV_OK;
}

}  // extern "C"
