// mxv_gaussian.hip — diagonal-Gaussian draws from a policy head's mean and log_std, with log-probabilities and entropies
// (include/mxv_policy.h).
//
// The result is defined bit for bit by the rule in the header: float64, one rounding per operation (this file is built with
// -ffp-contract=off like the rest of the library), LOG, SINCOS2PI and EXP as the operation sequences written there — no libm call — and
// IEEE `/` and sqrt.
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
#include "mxv_device.hpp"
#include "mxv_host.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;    // 256 CUs x 8 workgroups of 4 waves = every wave slot
constexpr int kMaxDim = 4;
constexpr int64_t kMaxElems = (int64_t)1 << 40;
constexpr uint32_t kStreamGaussian = 8u;   // 1-7: mxv_device.hpp (kStream*), mxv_tab.hip, mxv_bj.hip, mxv_policy.hip
constexpr double kLogStdMax = 80.0;        // sigma = EXP(+-80) is a normal float32

// ---- the constants of the rule: the output of tools/gaussian_coefficients.py, verbatim ----
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

struct GaussianArgs {
    const float *mean, *log_std;
    const uint64_t *step_dev;
    float *actions, *log_prob, *entropy;
    int64_t N, mean_ld, log_std_ld, actions_ld, tiles;
    uint64_t seed, env_offset, step;
};

__device__ __forceinline__ double exp_rule(double d) {   // |d| <= 80
    const double k = __builtin_rint(d * kInvLn2);
    const double r = (d - k * kLn2Hi) - k * kLn2Lo;
    double p = kExpC[13];
#pragma unroll
    for (int j = 12; j >= 0; --j) p = p * r + kExpC[j];
    return __builtin_ldexp(p, (int)k);
}

__device__ __forceinline__ double log_rule(double S) {   // 2^-33 <= S < 64
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

__device__ __forceinline__ bool bad_mean(float x) { return !(__builtin_fabsf(x) < __builtin_inff()); }                     // NaN, +-Inf
__device__ __forceinline__ bool bad_log_std(float x) { return !(__builtin_fabsf(x) <= (float)kLogStdMax); }              // NaN, |x| > 80

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

template <typename... T>
int bad(const char *fmt, T... args) {   // into the error slot of include/mxv_policy.h, which lives in mxv_policy.hip
    return mxv::policy_call_fail(MXV_ERR_INVALID_ARG, fmt, args...);
}

struct Range {   // the bytes [lo, lo + bytes) of one argument; lo == 0: absent
    const char *name;
    uintptr_t lo;
    uint64_t bytes;
};
bool meet(const Range &a, const Range &b) { return a.lo && b.lo && a.lo < b.lo + b.bytes && b.lo < a.lo + a.bytes; }

uint64_t rows_bytes(int64_t N, int64_t ld, int32_t D) { return ((uint64_t)(N - 1) * (uint64_t)ld + (uint64_t)D) * 4; }

template <int D>
hipError_t launch(dim3 grid, hipStream_t st, GaussianArgs &a) {
    void *args[] = {&a};
    // hipLaunchKernel returns THIS launch's status (hipGetLastError would also report, and clear, an earlier call's error)
    return hipLaunchKernel(reinterpret_cast<const void *>(&gaussian_kernel<D>), grid, dim3(kThreads), args, 0, st);
}

}  // namespace

extern "C" int mxv_policy_sample_gaussian(void *stream, int64_t N, int32_t D, const float *mean_dev, int64_t mean_ld, const float *log_std_dev,
                                          int64_t log_std_ld, uint64_t seed, uint64_t env_offset, uint64_t step, uint64_t *step_dev,
                                          float *actions_dev, int64_t actions_ld, float *log_prob_dev, float *entropy_dev) {
    const char *api = "mxv_policy_sample_gaussian";
    if (!mean_dev) return bad("%s: mean pointer is NULL", api);
    if (!log_std_dev) return bad("%s: log_std pointer is NULL", api);
    if (!actions_dev) return bad("%s: actions pointer is NULL", api);
    if (N < 1) return bad("%s: N = %lld must be at least 1", api, (long long)N);
    if (D < 1 || D > kMaxDim) return bad("%s: D = %d must be in 1..%d", api, (int)D, kMaxDim);
    if (mean_ld < D) return bad("%s: row stride mean_ld = %lld must be at least D = %d", api, (long long)mean_ld, (int)D);
    if (log_std_ld != 0 && log_std_ld < D)
        return bad("%s: row stride log_std_ld = %lld must be 0 (one shared row) or at least D = %d", api, (long long)log_std_ld, (int)D);
    if (actions_ld < D) return bad("%s: row stride actions_ld = %lld must be at least D = %d", api, (long long)actions_ld, (int)D);
    for (const int64_t ld : {mean_ld, log_std_ld, actions_ld})
        if (ld > kMaxElems / N) return bad("%s: N * ld = %lld * %lld is beyond 2^40 elements", api, (long long)N, (long long)ld);
    const Range ins[] = {{"mean", (uintptr_t)mean_dev, rows_bytes(N, mean_ld, D)},
                         {"log_std", (uintptr_t)log_std_dev, rows_bytes(N, log_std_ld, D)},
                         {"step_dev", (uintptr_t)step_dev, 8}};
    const Range outs[] = {{"actions", (uintptr_t)actions_dev, rows_bytes(N, actions_ld, D)}, {"log_prob", (uintptr_t)log_prob_dev, (uint64_t)N * 4},
                          {"entropy", (uintptr_t)entropy_dev, (uint64_t)N * 4}};
    struct Aligned {
        const Range *r;
        uint64_t elem;
    };
    for (const Aligned &x : {Aligned{&ins[0], 4}, Aligned{&ins[1], 4}, Aligned{&ins[2], 8}, Aligned{&outs[0], 4}, Aligned{&outs[1], 4}, Aligned{&outs[2], 4}}) {
        if (x.r->lo & (x.elem - 1)) return bad("%s: %s pointer %p is not %llu-byte aligned", api, x.r->name, (void *)x.r->lo, (unsigned long long)x.elem);
        if (x.r->lo && x.r->bytes > UINTPTR_MAX - x.r->lo)
            return bad("%s: %s at %p with N = %lld does not fit the address space", api, x.r->name, (void *)x.r->lo, (long long)N);
    }
    for (int i = 0; i < 3; ++i) {
        if (meet(outs[i], ins[0])) return bad("%s: output %s overlaps the mean", api, outs[i].name);
        if (meet(outs[i], ins[1])) return bad("%s: output %s overlaps the log_std", api, outs[i].name);
        if (meet(outs[i], ins[2])) return bad("%s: output %s overlaps step_dev", api, outs[i].name);
        for (int j = i + 1; j < 3; ++j)
            if (meet(outs[i], outs[j])) return bad("%s: outputs %s and %s overlap", api, outs[i].name, outs[j].name);
    }

    GaussianArgs a;
    a.mean = mean_dev; a.log_std = log_std_dev; a.step_dev = step_dev; a.actions = actions_dev; a.log_prob = log_prob_dev; a.entropy = entropy_dev;
    a.N = N; a.mean_ld = mean_ld; a.log_std_ld = log_std_ld; a.actions_ld = actions_ld; a.tiles = (N + kThreads - 1) / kThreads;
    a.seed = seed; a.env_offset = env_offset; a.step = step;
    const dim3 grid((unsigned)(a.tiles < kMaxBlocks ? a.tiles : kMaxBlocks));
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    switch (D) {
        case 1: e = launch<1>(grid, st, a); break;
        case 2: e = launch<2>(grid, st, a); break;
        case 3: e = launch<3>(grid, st, a); break;
        default: e = launch<4>(grid, st, a); break;
    }
    if (e != hipSuccess) return mxv::policy_call_fail(MXV_ERR_HIP, "%s: kernel launch: %s", api, hipGetErrorString(e));
    if (step_dev) {
        e = mxv::launch_add_word(step_dev, 1, st);
        if (e != hipSuccess) return mxv::policy_call_fail(MXV_ERR_HIP, "%s: step counter launch: %s", api, hipGetErrorString(e));
    }
    return MXV_OK;
}
