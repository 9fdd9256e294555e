// mxv_gaussian.hip — diagonal-Gaussian draws from a policy head's mean and log_std, with log-probabilities and entropies
// (include/mxv_policy.h).
//
// The result is defined bit for bit by the rule in the header: float64, one rounding per operation (this file is built with
// -ffp-contract=off like the rest of the library), LOG, SINCOS2PI and EXP as the operation sequences written there — no libm call — and
// IEEE `/` and sqrt.  Their one text, with the constants, the limits and the launch shape, is mxv_policy_rule.hpp, which mxv_policy.hip and
// mxv_policy_eval.hip include too; the argument checks are those of mxv_policy_host.hpp, and so is the error slot, which is mxv_policy.hip's.
//
// Shape of the kernel (arithmetic bound: a Philox call, one or two Box-Muller pairs of ~90 fp64 operations and ~45 per dimension, against
// 12 D + 8 bytes):
//   * one lane owns one env; the instantiations for D = 1, 2, 3, 4 hold the row in registers.  A row of mean, log_std or actions is one
//     4 D-byte run, moved with a single access of D dwords (the device takes them at any 4-byte boundary).  log_std_ld == 0 makes every
//     lane read the one shared row.
//   * one Philox4x32-10 call per lane: counter (G, t); words 0, 1 make dims 0, 1 and words 2, 3 dims 2, 3.  A pair that no dim < D uses
//     is not computed.
//   * everything in the rule is a select: no divergent branch.  A degenerate row computes on zeros and has its results replaced.
//   * the work of a pair of dims is the out-of-line dims_pair<1|2> (see there): its ~50 coefficient pairs are materialised where they are
//     used, not kept live across the tile loop.  No scratch, no spills (tests/test_gaussian_resources.py).
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

constexpr uint32_t kStreamGaussian = 8u;   // 1-7: mxv_device.hpp (kStream*), mxv_tab.hip, mxv_bj.hip, mxv_policy.hip

struct GaussianArgs {
    const float *mean, *log_std;
    const uint64_t *step_dev;
    float *actions, *log_prob, *entropy;
    int64_t N, mean_ld, log_std_ld, actions_ld, tiles;
    uint64_t seed, env_offset, step;
};

struct PairOut {
    float act[2];
    double lp, en;
};

// Dims 2p and 2p + 1 of one env (ND = 1: dim 2p alone) from the pair's two words: the Box-Muller pair, the actions and the terms they add
// to the running sums lp and en.  Deliberately out of line: inlined into the tile loop, the ~50 coefficient pairs of LOG, SINCOS2PI
// and EXP are hoisted out of that loop and kept live across it next to the kernel's arguments and the Philox key schedule, which is more
// scalar registers than a wave has; here each constant is materialised where it is used.  Arguments and results travel in registers.
template <int ND>
__device__ __attribute__((noinline)) PairOut dims_pair(uint32_t wa, uint32_t wb, float m0, float s0, float m1, float s1, bool degenerate,
                                                       double lp, double en) {
    double z[2];
    normal_pair(wa, wb, z[0], z[1]);
    const float m32[2] = {m0, m1}, s32[2] = {s0, s1};
    PairOut r;
    r.act[1] = 0.0f;
#pragma unroll
    for (int j = 0; j < ND; ++j) {
        const double mu = degenerate ? 0.0 : (double)m32[j];      // a degenerate row's results are replaced: keep its arithmetic finite
        const double ls = degenerate ? 0.0 : (double)s32[j];
        const double sigma = exp_rule(ls);
        const double aj = mu + sigma * z[j];
        r.act[j] = (float)aj;                                      // round to nearest even; +-Inf past float32's range
        const double zq = ((double)r.act[j] - mu) / sigma;
        lp = lp + ((-0.5 * (zq * zq) - ls) - kHalfLog2Pi);
        en = en + (ls + kEntC);
    }
    r.lp = lp;
    r.en = en;
    return r;
}

template <int D>
__global__ void __launch_bounds__(kThreads) gaussian_kernel(const GaussianArgs a) {
    const uint64_t t = a.step_dev ? *a.step_dev : a.step;
    const float nan = __uint_as_float(0x7FC00000u);
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t i = tile * kThreads + threadIdx.x;
        if (i >= a.N) continue;
        const uint64_t G = a.env_offset + (uint64_t)i;
        mxv::U4 ctr;
        ctr.x = (uint32_t)G;
        ctr.y = (uint32_t)(G >> 32);
        ctr.z = (uint32_t)t;
        ctr.w = ((uint32_t)(t >> 32) & 0x0fffffffu) | (kStreamGaussian << 28);
        const mxv::U4 w4 = mxv::philox4x32_10(ctr, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        const float *mrow = a.mean + i * a.mean_ld, *srow = a.log_std + i * a.log_std_ld;
        float m32[4] = {0.0f, 0.0f, 0.0f, 0.0f}, s32[4] = {0.0f, 0.0f, 0.0f, 0.0f}, act[4];
#pragma unroll
        for (int j = 0; j < D; ++j) m32[j] = mrow[j];      // merged into one access of D dwords: 4-byte alignment suffices
#pragma unroll
        for (int j = 0; j < D; ++j) s32[j] = srow[j];
        bool degenerate = false;
#pragma unroll
        for (int j = 0; j < D; ++j) degenerate |= bad_mean(m32[j]) || bad_log_std(s32[j]);
        PairOut r = dims_pair<(D < 2 ? D : 2)>(w4.x, w4.y, m32[0], s32[0], m32[1], s32[1], degenerate, 0.0, 0.0);
        act[0] = r.act[0];
        act[1] = r.act[1];
        if constexpr (D > 2) {
            r = dims_pair<D - 2>(w4.z, w4.w, m32[2], s32[2], m32[3], s32[3], degenerate, r.lp, r.en);
            act[2] = r.act[0];
            act[3] = r.act[1];
        }
        float *arow = a.actions + i * a.actions_ld;
#pragma unroll
        for (int j = 0; j < D; ++j) arow[j] = degenerate ? nan : act[j];      // one store of D dwords
        if (a.log_prob) a.log_prob[i] = degenerate ? nan : (float)r.lp;
        if (a.entropy) a.entropy[i] = degenerate ? nan : (float)r.en;
    }
}

template <int D>
const void *kernel_of() {
    return reinterpret_cast<const void *>(&gaussian_kernel<D>);
}

}  // namespace

extern "C" int mxv_policy_sample_gaussian(void *stream, int64_t N, int32_t D, const float *mean_dev, int64_t mean_ld, const float *log_std_dev,
                                          int64_t log_std_ld, uint64_t seed, uint64_t env_offset, uint64_t step, uint64_t *step_dev,
                                          float *actions_dev, int64_t actions_ld, float *log_prob_dev, float *entropy_dev) {
    const Call<mxv::PolicyCall> call{"mxv_policy_sample_gaussian", 'N'};
    if (int rc = call.check_gauss(N, D, mean_dev, mean_ld, log_std_dev, log_std_ld, actions_dev, actions_ld)) return rc;
    const Range ins[] = {{"mean", (uintptr_t)mean_dev, rows_bytes(N, mean_ld, D), 4}, {"log_std", (uintptr_t)log_std_dev, rows_bytes(N, log_std_ld, D), 4},
                         {"step_dev", (uintptr_t)step_dev, 8, 8, ""}};
    const Range outs[] = {{"actions", (uintptr_t)actions_dev, rows_bytes(N, actions_ld, D), 4}, {"log_prob", (uintptr_t)log_prob_dev, (uint64_t)N * 4, 4},
                          {"entropy", (uintptr_t)entropy_dev, (uint64_t)N * 4, 4}};
    if (int rc = call.check_ranges(N, ins, 3, outs, 3)) return rc;
    GaussianArgs a;
    a.mean = mean_dev; a.log_std = log_std_dev; a.step_dev = step_dev; a.actions = actions_dev; a.log_prob = log_prob_dev; a.entropy = entropy_dev;
    a.N = N; a.mean_ld = mean_ld; a.log_std_ld = log_std_ld; a.actions_ld = actions_ld; a.tiles = (N + kThreads - 1) / kThreads;
    a.seed = seed; a.env_offset = env_offset; a.step = step;
    const void *kernel;
    switch (D) {
        case 1: kernel = kernel_of<1>(); break;
        case 2: kernel = kernel_of<2>(); break;
        case 3: kernel = kernel_of<3>(); break;
        default: kernel = kernel_of<4>(); break;
    }
    if (int rc = call.launch(kernel, a, stream)) return rc;
    return call.advance(step_dev, stream);
}
