// mxv_squashed.hip — reparameterised, tanh-squashed diagonal-Gaussian draws with their log-probabilities, and the gradients of both with
// respect to mean and log_std (include/mxv_squashed.h).
//
// The result is defined bit for bit by the rule in the header: float64, one rounding per operation (this file is built with
// -ffp-contract=off like the rest of the library), EXP, E, LOG and the Box-Muller pair as mxv_policy_rule.hpp writes them — no libm call —
// and IEEE `/`.  The argument checks and the launch are those of mxv_policy_host.hpp; the error slot is this file's own.
//
// Shape of the two kernels (arithmetic bound, as mxv_gaussian.hip: a Philox call, one or two Box-Muller pairs, and per dimension an EXP,
// an E and a LOG forwards, an EXP and an E backwards):
//   * one lane owns one row; the instantiations for D = 1, 2, 3, 4 hold the row in registers.  A row of mean, log_std, actions or of a
//     gradient is one 4 D-byte run, moved with a single access of D dwords.  log_std_ld == 0 makes every lane read the one shared row.
//   * one Philox4x32-10 call per lane under stream tag 11: words 0, 1 make dims 0, 1 and words 2, 3 dims 2, 3.  A pair that no dim < D
//     uses is not computed.  The backward makes the same call and recomputes the noise: the forward saves nothing.
//   * everything in the rule is a select: no divergent branch.  A degenerate row computes on zeros and has its results replaced.
//   * the Box-Muller pair and the work of one dim are out of line (normals_of, squash_dim, squash_dim_backward) for the reason given at
//     dims_pair in mxv_gaussian.hip: the coefficient pairs are materialised where they are used, not kept live across the tile loop.
//     No scratch, no spills (tests/test_squashed_resources.py).
//   * t comes from the argument or, with step_dev, from device memory (a uniform load); the forward's row 0 stores it to step_used, and
//     mxv::launch_add_word behind the forward advances step_dev.  The backward advances nothing.
//   * no atomics, no LDS, no inline assembly.  Grid: at most kMaxBlocks workgroups of 256 lanes, each striding over tiles of 256 rows.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/mxv_squashed.h"
#include "mxv_policy_host.hpp"
#include "mxv_policy_rule.hpp"

namespace mxv {
struct SquashedCall {   // include/mxv_squashed.h: mxv_squashed_last_error
    std::string error;
};
}  // namespace mxv

namespace {

using namespace mxv::rule;
using namespace mxv::policy_host;

constexpr uint32_t kStreamSquashed = 11u;  // 1-8: see mxv_gaussian.hip; 9, 10: mxv_replay.hip, mxv_prio.hip
constexpr double kLn2 = kLn2Hi + kLn2Lo;   // rounded once
constexpr double kTiny = 0x1p-27;          // below it tanh(v) = v to float32's last place and 1 - e cancels
constexpr double kScaleMin = 0x1p-33, kScaleMax = 64.0;      // log_rule's domain

struct Affine {      // the action space of the head: action = bias + scale * tanh(u); widened exactly where it is used
    float scale[kMaxDim], bias[kMaxDim];
};

struct SquashedArgs {
    const float *mean, *log_std;
    const uint64_t *step_dev;
    uint64_t *step_used;
    float *actions, *log_prob;
    int64_t N, mean_ld, log_std_ld, actions_ld, tiles;
    uint64_t seed, env_offset, step;
    Affine af;
};

struct SquashedGradArgs {
    const float *mean, *log_std, *grad_actions, *grad_log_prob;
    const uint64_t *step_dev;
    float *grad_mean, *grad_log_std;
    int64_t N, mean_ld, log_std_ld, grad_actions_ld, grad_mean_ld, grad_log_std_ld, tiles;
    uint64_t seed, env_offset, step;
    Affine af;
};

// What forward and backward compute alike of one dim: the lines of the rule from sigma to t.
struct Squash {
    double n, v, e, q, t;
};

__device__ __forceinline__ Squash squash_of(double mu, double ls, double z) {
    Squash s;
    const double sigma = exp_rule(ls);
    s.n = sigma * z;
    const double u = mu + s.n;
    s.v = __builtin_fabs(u);
    s.e = e_of(-2.0 * s.v);
    s.q = 1.0 + s.e;
    const double th = s.v < kTiny ? s.v : (1.0 - s.e) / s.q;
    s.t = __builtin_copysign(th, u);
    return s;
}

__device__ __forceinline__ mxv::U4 words_of(uint64_t G, uint64_t t, uint64_t seed) {
    mxv::U4 ctr;
    ctr.x = (uint32_t)G;
    ctr.y = (uint32_t)(G >> 32);
    ctr.z = (uint32_t)t;
    ctr.w = ((uint32_t)(t >> 32) & 0x0fffffffu) | (kStreamSquashed << 28);
    return mxv::philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
}

struct Normals {
    double z0, z1;
};

// The Box-Muller pair of two words.  Out of line, as the per-dim work below, for the reason given at dims_pair in mxv_gaussian.hip: inlined
// into the tile loop, the coefficient pairs of LOG, SINCOS2PI and EXP are hoisted out of that loop and kept live across it, which is more
// scalar registers than a wave has; here each constant is materialised where it is used.  Arguments and results travel in registers.
__device__ __attribute__((noinline)) Normals normals_of(uint32_t wa, uint32_t wb) {
    Normals r;
    normal_pair(wa, wb, r.z0, r.z1);
    return r;
}

struct DimOut {
    float act;
    double lp;
};

// One dim of one row: its action and what it adds to the running sum lp.
__device__ __attribute__((noinline)) DimOut squash_dim(float m32, float s32, double z, float sc32, float bi32, bool degenerate, double lp) {
    const double mu = degenerate ? 0.0 : (double)m32;      // a degenerate row's results are replaced: keep its arithmetic finite
    const double ls = degenerate ? 0.0 : (double)s32;
    const double sc = (double)sc32, bi = (double)bi32;
    const Squash s = squash_of(mu, ls, z);
    DimOut r;
    r.act = (float)(bi + sc * s.t);
    const double corr = 2.0 * ((kLn2 - s.v) - log_rule(s.q));
    r.lp = lp + (((-0.5 * (z * z) - ls) - kHalfLog2Pi) - (log_rule(sc) + corr));
    return r;
}

struct DimGrad {
    float gm, gls;
};

__device__ __attribute__((noinline)) DimGrad squash_dim_backward(float m32, float s32, double z, float sc32, float ga32, float glp32,
                                                                 bool degenerate) {
    const double mu = degenerate ? 0.0 : (double)m32;
    const double ls = degenerate ? 0.0 : (double)s32;
    const double glp = (double)glp32;
    const Squash s = squash_of(mu, ls, z);
    const double sech2 = (4.0 * s.e) / (s.q * s.q);
    const double gs = ((double)ga32 * (double)sc32) * sech2;
    const double t2 = 2.0 * s.t;
    DimGrad r;
    r.gm = (float)(gs + glp * t2);
    r.gls = (float)(gs * s.n + glp * (t2 * s.n - 1.0));
    return r;
}

template <int D>
__global__ void __launch_bounds__(kThreads) squashed_kernel(const SquashedArgs a) {
    const uint64_t t = a.step_dev ? *a.step_dev : a.step;
    const float nan = __uint_as_float(0x7FC00000u);
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t i = tile * kThreads + threadIdx.x;
        if (i >= a.N) continue;
        if (i == 0 && a.step_used) *a.step_used = t;
        const mxv::U4 w4 = words_of(a.env_offset + (uint64_t)i, t, a.seed);
        const float *mrow = a.mean + i * a.mean_ld, *srow = a.log_std + i * a.log_std_ld;
        float m32[4] = {0.0f, 0.0f, 0.0f, 0.0f}, s32[4] = {0.0f, 0.0f, 0.0f, 0.0f}, act[4];
#pragma unroll
        for (int j = 0; j < D; ++j) m32[j] = mrow[j];      // merged into one access of D dwords: 4-byte alignment suffices
#pragma unroll
        for (int j = 0; j < D; ++j) s32[j] = srow[j];
        bool degenerate = false;
#pragma unroll
        for (int j = 0; j < D; ++j) degenerate |= bad_mean(m32[j]) || bad_log_std(s32[j]);
        double z[4];
        Normals nz = normals_of(w4.x, w4.y);
        z[0] = nz.z0;
        z[1] = nz.z1;
        if constexpr (D > 2) {
            nz = normals_of(w4.z, w4.w);
            z[2] = nz.z0;
            z[3] = nz.z1;
        }
        double lp = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const DimOut r = squash_dim(m32[j], s32[j], z[j], a.af.scale[j], a.af.bias[j], degenerate, lp);
            act[j] = r.act;
            lp = r.lp;
        }
        float *arow = a.actions + i * a.actions_ld;
#pragma unroll
        for (int j = 0; j < D; ++j) arow[j] = degenerate ? nan : act[j];      // one store of D dwords
        if (a.log_prob) a.log_prob[i] = degenerate ? nan : (float)lp;
    }
}

template <int D>
__global__ void __launch_bounds__(kThreads) squashed_backward_kernel(const SquashedGradArgs a) {
    const uint64_t t = a.step_dev ? *a.step_dev : a.step;
    const float nan = __uint_as_float(0x7FC00000u);
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t i = tile * kThreads + threadIdx.x;
        if (i >= a.N) continue;
        const mxv::U4 w4 = words_of(a.env_offset + (uint64_t)i, t, a.seed);
        const float *mrow = a.mean + i * a.mean_ld, *srow = a.log_std + i * a.log_std_ld;
        float m32[4] = {0.0f, 0.0f, 0.0f, 0.0f}, s32[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ga[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gm[4], gls[4];
#pragma unroll
        for (int j = 0; j < D; ++j) m32[j] = mrow[j];
#pragma unroll
        for (int j = 0; j < D; ++j) s32[j] = srow[j];
        if (a.grad_actions) {
            const float *grow = a.grad_actions + i * a.grad_actions_ld;
#pragma unroll
            for (int j = 0; j < D; ++j) ga[j] = grow[j];
        }
        const float glp = a.grad_log_prob ? a.grad_log_prob[i] : 0.0f;
        bool degenerate = false;
#pragma unroll
        for (int j = 0; j < D; ++j) degenerate |= bad_mean(m32[j]) || bad_log_std(s32[j]);
        double z[4];
        Normals nz = normals_of(w4.x, w4.y);
        z[0] = nz.z0;
        z[1] = nz.z1;
        if constexpr (D > 2) {
            nz = normals_of(w4.z, w4.w);
            z[2] = nz.z0;
            z[3] = nz.z1;
        }
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const DimGrad r = squash_dim_backward(m32[j], s32[j], z[j], a.af.scale[j], ga[j], glp, degenerate);
            gm[j] = r.gm;
            gls[j] = r.gls;
        }
        if (a.grad_mean) {
            float *row = a.grad_mean + i * a.grad_mean_ld;
#pragma unroll
            for (int j = 0; j < D; ++j) row[j] = degenerate ? nan : gm[j];
        }
        if (a.grad_log_std) {
            float *row = a.grad_log_std + i * a.grad_log_std_ld;
#pragma unroll
            for (int j = 0; j < D; ++j) row[j] = degenerate ? nan : gls[j];
        }
    }
}

template <template <int> class K>
const void *pick(int32_t D) {
    switch (D) {
        case 1: return K<1>::ptr();
        case 2: return K<2>::ptr();
        case 3: return K<3>::ptr();
        default: return K<4>::ptr();
    }
}
template <int D>
struct Fwd {
    static const void *ptr() { return reinterpret_cast<const void *>(&squashed_kernel<D>); }
};
template <int D>
struct Bwd {
    static const void *ptr() { return reinterpret_cast<const void *>(&squashed_backward_kernel<D>); }
};

using SCall = Call<mxv::SquashedCall>;

// N, D, the strides of the head, and the host arrays scale and bias -> af
int check_head(const SCall &call, int64_t N, int32_t D, const float *mean, int64_t mean_ld, const float *log_std, int64_t log_std_ld,
               const float *scale, const float *bias, Affine &af) {
    if (!mean) return call.bad("%s: mean pointer is NULL", call.api);
    if (!log_std) return call.bad("%s: log_std pointer is NULL", call.api);
    if (N < 1) return call.bad("%s: N = %lld must be at least 1", call.api, (long long)N);
    if (D < 1 || D > kMaxDim) return call.bad("%s: D = %d must be in 1..%d", call.api, (int)D, kMaxDim);
    if (mean_ld < D) return call.bad("%s: row stride mean_ld = %lld must be at least D = %d", call.api, (long long)mean_ld, (int)D);
    if (log_std_ld != 0 && log_std_ld < D)
        return call.bad("%s: row stride log_std_ld = %lld must be 0 (one shared row) or at least D = %d", call.api, (long long)log_std_ld, (int)D);
    for (const int64_t ld : {mean_ld, log_std_ld})
        if (int rc = call.check_stride(ld, N)) return rc;
    for (int j = 0; j < kMaxDim; ++j) {
        const double s = scale && j < D ? (double)scale[j] : 1.0, b = bias && j < D ? (double)bias[j] : 0.0;
        if (!(s >= kScaleMin && s <= kScaleMax)) return call.bad("%s: scale[%d] = %g must be finite and in [2^-33, 64]", call.api, j, s);
        if (!std::isfinite(b)) return call.bad("%s: bias[%d] = %g must be finite", call.api, j, b);
        af.scale[j] = (float)s;
        af.bias[j] = (float)b;
    }
    return MXV_OK;
}

// an [N][D] argument besides the head's: its stride
int check_rows(const SCall &call, const char *name, int64_t N, int32_t D, int64_t ld) {
    if (ld < D) return call.bad("%s: row stride %s_ld = %lld must be at least D = %d", call.api, name, (long long)ld, (int)D);
    return call.check_stride(ld, N);
}

}  // namespace

extern "C" int mxv_squashed_sample(void *stream, int64_t N, int32_t D, const float *mean_dev, int64_t mean_ld, const float *log_std_dev,
                                   int64_t log_std_ld, const float *scale, const float *bias, uint64_t seed, uint64_t env_offset, uint64_t step,
                                   uint64_t *step_dev, uint64_t *step_used_dev, float *actions_dev, int64_t actions_ld, float *log_prob_dev) {
    const SCall call{"mxv_squashed_sample", 'N'};
    SquashedArgs a;
    if (int rc = check_head(call, N, D, mean_dev, mean_ld, log_std_dev, log_std_ld, scale, bias, a.af)) return rc;
    if (!actions_dev) return call.bad("%s: actions pointer is NULL", call.api);
    if (int rc = check_rows(call, "actions", N, D, actions_ld)) return rc;
    const Range ins[] = {{"mean", (uintptr_t)mean_dev, rows_bytes(N, mean_ld, D), 4}, {"log_std", (uintptr_t)log_std_dev, rows_bytes(N, log_std_ld, D), 4},
                         {"step_dev", (uintptr_t)step_dev, 8, 8, ""}};
    const Range outs[] = {{"actions", (uintptr_t)actions_dev, rows_bytes(N, actions_ld, D), 4}, {"log_prob", (uintptr_t)log_prob_dev, (uint64_t)N * 4, 4},
                          {"step_used", (uintptr_t)step_used_dev, 8, 8}};
    if (int rc = call.check_ranges(N, ins, 3, outs, 3)) return rc;
    a.mean = mean_dev; a.log_std = log_std_dev; a.step_dev = step_dev; a.step_used = step_used_dev; a.actions = actions_dev; a.log_prob = log_prob_dev;
    a.N = N; a.mean_ld = mean_ld; a.log_std_ld = log_std_ld; a.actions_ld = actions_ld; a.tiles = (N + kThreads - 1) / kThreads;
    a.seed = seed; a.env_offset = env_offset; a.step = step;
    if (int rc = call.launch(pick<Fwd>(D), a, stream)) return rc;
    return call.advance(step_dev, stream);
}

extern "C" int mxv_squashed_sample_backward(void *stream, int64_t N, int32_t D, const float *mean_dev, int64_t mean_ld, const float *log_std_dev,
                                            int64_t log_std_ld, const float *scale, const float *bias, uint64_t seed, uint64_t env_offset,
                                            uint64_t step, const uint64_t *step_dev, const float *grad_actions_dev, int64_t grad_actions_ld,
                                            const float *grad_log_prob_dev, float *grad_mean_dev, int64_t grad_mean_ld, float *grad_log_std_dev,
                                            int64_t grad_log_std_ld) {
    const SCall call{"mxv_squashed_sample_backward", 'N'};
    SquashedGradArgs a;
    if (int rc = check_head(call, N, D, mean_dev, mean_ld, log_std_dev, log_std_ld, scale, bias, a.af)) return rc;
    if (!grad_mean_dev && !grad_log_std_dev) return call.bad("%s: grad_mean and grad_log_std pointers are both NULL", call.api);
    if (grad_actions_dev)
        if (int rc = check_rows(call, "grad_actions", N, D, grad_actions_ld)) return rc;
    if (grad_mean_dev)
        if (int rc = check_rows(call, "grad_mean", N, D, grad_mean_ld)) return rc;
    if (grad_log_std_dev)
        if (int rc = check_rows(call, "grad_log_std", N, D, grad_log_std_ld)) return rc;
    const Range ins[] = {{"mean", (uintptr_t)mean_dev, rows_bytes(N, mean_ld, D), 4},
                         {"log_std", (uintptr_t)log_std_dev, rows_bytes(N, log_std_ld, D), 4},
                         {"step_dev", (uintptr_t)step_dev, 8, 8, ""},
                         {"grad_actions", (uintptr_t)grad_actions_dev, grad_actions_dev ? rows_bytes(N, grad_actions_ld, D) : 0, 4},
                         {"grad_log_prob", (uintptr_t)grad_log_prob_dev, (uint64_t)N * 4, 4}};
    const Range outs[] = {{"grad_mean", (uintptr_t)grad_mean_dev, grad_mean_dev ? rows_bytes(N, grad_mean_ld, D) : 0, 4},
                          {"grad_log_std", (uintptr_t)grad_log_std_dev, grad_log_std_dev ? rows_bytes(N, grad_log_std_ld, D) : 0, 4}};
    if (int rc = call.check_ranges(N, ins, 5, outs, 2)) return rc;
    a.mean = mean_dev; a.log_std = log_std_dev; a.grad_actions = grad_actions_dev; a.grad_log_prob = grad_log_prob_dev; a.step_dev = step_dev;
    a.grad_mean = grad_mean_dev; a.grad_log_std = grad_log_std_dev;
    a.N = N; a.mean_ld = mean_ld; a.log_std_ld = log_std_ld; a.grad_actions_ld = grad_actions_ld; a.grad_mean_ld = grad_mean_ld;
    a.grad_log_std_ld = grad_log_std_ld; a.tiles = (N + kThreads - 1) / kThreads;
    a.seed = seed; a.env_offset = env_offset; a.step = step;
    return call.launch(pick<Bwd>(D), a, stream);
}

extern "C" const char *mxv_squashed_last_error(void) { return mxv::last_error<mxv::SquashedCall>(nullptr); }
