// mxv_policy.hip — categorical draws from a policy's logits, with log-probabilities and entropies (include/mxv_policy.h).
//
// The result is defined bit for bit by the rule in the header: float64, one rounding per operation (this file is built with
// -ffp-contract=off like the rest of the library), EXP and LOG as the operation sequences written there — no libm call, no __expf.
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
#include "mxv_device.hpp"
#include "mxv_host.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;    // 256 CUs x 8 workgroups of 4 waves = every wave slot
constexpr int kMaxActions = 64;
constexpr int64_t kMaxElems = (int64_t)1 << 40;
constexpr uint32_t kStreamPolicy = 7u;   // 1-6: mxv_device.hpp (kStream*), mxv_tab.hip, mxv_bj.hip

// ---- the constants of EXP and LOG: the output of tools/policy_coefficients.py, verbatim ----
constexpr double kInvLn2 = 0x1.71547652b82fep+0;
constexpr double kLn2Hi = 0x1.62e42fee00000p-1;
constexpr double kLn2Lo = 0x1.a39ef35793c76p-33;
constexpr double kSqrtHalf = 0x1.6a09e667f3bcdp-1;
constexpr double kExpC[14] = {0x1.0000000000000p+0, 0x1.0000000000000p+0, 0x1.0000000000000p-1, 0x1.5555555555555p-3, 0x1.5555555555555p-5, 0x1.1111111111111p-7, 0x1.6c16c16c16c17p-10, 0x1.a01a01a01a01ap-13, 0x1.a01a01a01a01ap-16, 0x1.71de3a556c734p-19, 0x1.27e4fb7789f5cp-22, 0x1.ae64567f544e4p-26, 0x1.1eed8eff8d898p-29, 0x1.6124613a86d09p-33};
constexpr double kLogC[12] = {0x1.0000000000000p+0, 0x1.5555555555555p-2, 0x1.999999999999ap-3, 0x1.2492492492492p-3, 0x1.c71c71c71c71cp-4, 0x1.745d1745d1746p-4, 0x1.3b13b13b13b14p-4, 0x1.1111111111111p-4, 0x1.e1e1e1e1e1e1ep-5, 0x1.af286bca1af28p-5, 0x1.8618618618618p-5, 0x1.642c8590b2164p-5};
// ---- end of the generated block ----
constexpr double kExpCut = -708.0;

struct PolicyArgs {
    const float *logits;
    const uint64_t *step_dev;
    void *actions;
    float *log_prob, *entropy;
    int64_t N, ld, tiles;
    uint64_t seed, env_offset, step;
    int32_t A, i64;
};

__device__ __forceinline__ double exp_rule(double d) {   // -708 <= d <= 0
    const double k = __builtin_rint(d * kInvLn2);
    const double r = (d - k * kLn2Hi) - k * kLn2Lo;
    double p = kExpC[13];
#pragma unroll
    for (int j = 12; j >= 0; --j) p = p * r + kExpC[j];
    return __builtin_ldexp(p, (int)k);
}

__device__ __forceinline__ double e_of(double d) { return d < kExpCut ? 0.0 : exp_rule(d < kExpCut ? 0.0 : d); }

__device__ __forceinline__ double log_rule(double S) {   // 1 <= S <= 64
    int e;
    double f = __builtin_frexp(S, &e);
    if (f < kSqrtHalf) {
        f = f * 2.0;
        e = e - 1;
    }
    const double ed = (double)e;
    const double s = (f - 1.0) / (f + 1.0);
    const double z = s * s;
    double p = kLogC[11];
#pragma unroll
    for (int j = 10; j >= 0; --j) p = p * z + kLogC[j];
    return ((ed * kLn2Hi) + (2.0 * s) * p) + ed * kLn2Lo;
}

__device__ __forceinline__ float to_f32(double x) { return (float)x; }   // round to nearest even; the NaN rows are written as a pattern

__device__ __forceinline__ bool bad_logit(float x) { return x != x || x == __builtin_inff(); }

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

struct PolicyCall {   // the error slot of the handle-free call: one per thread (mxv::create_error)
    std::string error;
};

template <typename... T>
int bad(const char *fmt, T... args) {
    return mxv::fail<PolicyCall>(nullptr, MXV_ERR_INVALID_ARG, fmt, args...);
}

struct Range {   // the bytes [lo, lo + bytes) of one argument; lo == 0: absent
    const char *name;
    uintptr_t lo;
    uint64_t bytes;
};
bool meet(const Range &a, const Range &b) { return a.lo && b.lo && a.lo < b.lo + b.bytes && b.lo < a.lo + a.bytes; }

struct LastLaunch {   // of the calling thread (mxv_policy_last_launch)
    int32_t envs_per_lane = 0, specialised_A = 0;
    uint32_t grid = 0;
};
LastLaunch &last_launch() {
    thread_local LastLaunch l;
    return l;
}

template <int AT>
hipError_t launch(dim3 grid, hipStream_t st, PolicyArgs &a) {
    void *args[] = {&a};
    // hipLaunchKernel returns THIS launch's status (hipGetLastError would also report, and clear, an earlier call's error)
    return hipLaunchKernel(reinterpret_cast<const void *>(&policy_kernel<AT>), grid, dim3(kThreads), args, 0, st);
}

}  // namespace

int mxv::policy_call_fail(int code, const char *fmt, ...) {   // mxv_host.hpp: the same slot for mxv_gaussian.hip
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return mxv::fail<PolicyCall>(nullptr, code, "%s", buf);
}

extern "C" {

int mxv_policy_sample_categorical(void *stream, int64_t N, int32_t A, const float *logits_dev, int64_t ld, uint64_t seed,
                                  uint64_t env_offset, uint64_t step, uint64_t *step_dev, void *actions_dev, int32_t actions_are_i64,
                                  float *log_prob_dev, float *entropy_dev) {
    const char *api = "mxv_policy_sample_categorical";
    if (!logits_dev) return bad("%s: logits pointer is NULL", api);
    if (!actions_dev) return bad("%s: actions pointer is NULL", api);
    if (N < 1) return bad("%s: N = %lld must be at least 1", api, (long long)N);
    if (A < 1 || A > kMaxActions) return bad("%s: A = %d must be in 1..%d", api, (int)A, kMaxActions);
    if (ld < A) return bad("%s: row stride ld = %lld must be at least A = %d", api, (long long)ld, (int)A);
    if (ld > kMaxElems / N) return bad("%s: N * ld = %lld * %lld is beyond 2^40 elements", api, (long long)N, (long long)ld);
    const uint64_t ab = actions_are_i64 ? 8 : 4;
    const Range logits{"logits", (uintptr_t)logits_dev, ((uint64_t)(N - 1) * (uint64_t)ld + (uint64_t)A) * 4};
    const Range stepr{"step_dev", (uintptr_t)step_dev, 8};
    const Range outs[] = {{"actions", (uintptr_t)actions_dev, (uint64_t)N * ab}, {"log_prob", (uintptr_t)log_prob_dev, (uint64_t)N * 4},
                          {"entropy", (uintptr_t)entropy_dev, (uint64_t)N * 4}};
    struct Aligned {
        const Range *r;
        uint64_t elem;
    };
    for (const Aligned &x : {Aligned{&logits, 4}, Aligned{&stepr, 8}, Aligned{&outs[0], ab}, Aligned{&outs[1], 4}, Aligned{&outs[2], 4}}) {
        if (x.r->lo & (x.elem - 1)) return bad("%s: %s pointer %p is not %llu-byte aligned", api, x.r->name, (void *)x.r->lo, (unsigned long long)x.elem);
        if (x.r->lo && x.r->bytes > UINTPTR_MAX - x.r->lo)
            return bad("%s: %s at %p with N = %lld does not fit the address space", api, x.r->name, (void *)x.r->lo, (long long)N);
    }
    for (int i = 0; i < 3; ++i) {
        if (meet(outs[i], logits)) return bad("%s: output %s overlaps the logits", api, outs[i].name);
        if (meet(outs[i], stepr)) return bad("%s: output %s overlaps step_dev", api, outs[i].name);
        for (int j = i + 1; j < 3; ++j)
            if (meet(outs[i], outs[j])) return bad("%s: outputs %s and %s overlap", api, outs[i].name, outs[j].name);
    }

    PolicyArgs a;
    a.logits = logits_dev; a.step_dev = step_dev; a.actions = actions_dev; a.log_prob = log_prob_dev; a.entropy = entropy_dev;
    a.N = N; a.ld = ld; a.tiles = (N + kThreads - 1) / kThreads;
    a.seed = seed; a.env_offset = env_offset; a.step = step;
    a.A = A; a.i64 = actions_are_i64 ? 1 : 0;
    const dim3 grid((unsigned)(a.tiles < kMaxBlocks ? a.tiles : kMaxBlocks));
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    int32_t spec = A;
    switch (A) {
        case 2: e = launch<2>(grid, st, a); break;
        case 3: e = launch<3>(grid, st, a); break;
        case 4: e = launch<4>(grid, st, a); break;
        case 6: e = launch<6>(grid, st, a); break;
        default: e = launch<0>(grid, st, a); spec = 0; break;
    }
    if (e != hipSuccess) return mxv::fail<PolicyCall>(nullptr, MXV_ERR_HIP, "%s: kernel launch: %s", api, hipGetErrorString(e));
    if (step_dev) {
        e = mxv::launch_add_word(step_dev, 1, st);
        if (e != hipSuccess) return mxv::fail<PolicyCall>(nullptr, MXV_ERR_HIP, "%s: step counter launch: %s", api, hipGetErrorString(e));
    }
    last_launch() = LastLaunch{1, spec, grid.x};
    return MXV_OK;
}

const char *mxv_policy_last_error(void) { return mxv::last_error<PolicyCall>(nullptr); }

int mxv_policy_last_launch(int32_t *envs_per_lane, int32_t *specialised_A, uint32_t *grid) {
    if (!envs_per_lane || !specialised_A || !grid) return bad("mxv_policy_last_launch: output pointer is NULL");
    *envs_per_lane = last_launch().envs_per_lane;
    *specialised_A = last_launch().specialised_A;
    *grid = last_launch().grid;
    return MXV_OK;
}

}  // extern "C"
