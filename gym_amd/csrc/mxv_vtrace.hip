// mxv_vtrace.hip — V-trace value targets and policy-gradient advantages over [K][N] trajectory tensors (include/mxv_vtrace.h,
// DESIGN.md §16).
//
// The recurrence of mxv_gae.hip with truncated importance weights: backwards over the K rows, independent per env, sequential in t and
// parallel in N, evaluated as the rule states it — float64, one rounding per operation (-ffp-contract=off), t = K-1 ... 0 — because
// the result is defined bit for bit.  No scan over K: composing the affine maps acc -> delta + gc acc re-associates the sum.
//
// Shape of the kernel (26 B per env-step with float32 rewards, about 60 float64 operations of which EXP's polynomial is half):
//   * one lane owns V consecutive envs of every row.  V = 4 (16-byte accesses: one dwordx4 each of log_prob, old_log_prob, values and
//     rewards — two for float64 —, one dword of each flag row, dwordx4 stores) under mxv_gae.hip's switch-over: N >= 2^21, with N, both
//     row strides and the base addresses allowing it; otherwise V = 1 for the whole call.
//   * a register ring: the loads of rows t-1 ... t-kRing are issued before row t is consumed, and nothing derived from a load is kept
//     in the ring, so the wait in front of row t is a counted one (vmcnt(n), n > 0), never a drain.  The weights w of a row do not
//     depend on the recurrence, but they are derived values: they are formed when the row is consumed.
//   * final_values is loaded only behind (truncated && !terminated), per element: most rows never touch it.
//   * no atomics, no LDS, no inline assembly, no scratch (tests/test_vtrace_resources.py).  Grid: at most kMaxBlocks workgroups of
//     kThreads lanes, each striding over tiles of kThreads V envs.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <utility>

#include "../../include/mxv_vtrace.h"
#include "mxv_policy_host.hpp"
#include "mxv_policy_rule.hpp"

namespace {

using namespace mxv::rule;

constexpr int kRing = 4;            // rows in flight ahead of the one being consumed (gym_amd/vtrace.py: RING_DEPTH)
constexpr int64_t kVecMinN = (int64_t)4 * 256 * 32 * 64;   // 2^21: mxv_gae.hip's switch-over
constexpr double kRatioLogMax = 80.0;

struct VtArgs {
    const float *lp, *old;
    const void *reward;
    const uint8_t *term, *trunc;
    const float *values, *last_value, *final_values;
    float *vs, *pg;
    int64_t K, N, ld, ld_out, tiles;
    double gamma, lam, rho_bar, c_bar, pg_rho_bar;
};

// what the loads of one row return for a lane, and nothing derived from it
template <typename RT, int V>
struct Slot {
    float lp[V], old[V];
    RT r[V];
    float v[V];
    uint32_t ft, fu;   // V = 4: the dword of four flag bytes; V = 1: the byte
};

__device__ __forceinline__ void load4(const float *p, float (&x)[4]) {
    const float4 q = *reinterpret_cast<const float4 *>(p);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
}

template <typename RT, int V>
__device__ __forceinline__ void fetch(const VtArgs &a, int64_t row, int64_t n0, Slot<RT, V> &s) {
    const int64_t off = row * a.ld + n0;
    const RT *rew = static_cast<const RT *>(a.reward) + off;
    if constexpr (V == 4) {
        load4(a.lp + off, s.lp);
        load4(a.old + off, s.old);
        if constexpr (sizeof(RT) == 8) {
            const double2 x = reinterpret_cast<const double2 *>(rew)[0], y = reinterpret_cast<const double2 *>(rew)[1];
            s.r[0] = x.x; s.r[1] = x.y; s.r[2] = y.x; s.r[3] = y.y;
        } else {
            load4(rew, s.r);
        }
        load4(a.values + off, s.v);
        s.ft = *reinterpret_cast<const uint32_t *>(a.term + off);
        s.fu = *reinterpret_cast<const uint32_t *>(a.trunc + off);
    } else {
        s.lp[0] = a.lp[off];
        s.old[0] = a.old[off];
        s.r[0] = rew[0];
        s.v[0] = a.values[off];
        s.ft = a.term[off];
        s.fu = a.trunc[off];
    }
}

__device__ __forceinline__ float to_f32(double x) {
    const float f = (float)x;                            // round to nearest even, subnormals kept
    return f != f ? __uint_as_float(0x7FC00000u) : f;    // one NaN pattern (mxv_vtrace.h)
}

// state: acc = acc_{t+1}, vsn = vs_{t+1}, nv = nv_{t+1} (a float32 value, or last_value)
template <typename RT, bool FV, int V>
__device__ __forceinline__ void consume(const VtArgs &a, int64_t row, int64_t n0, const Slot<RT, V> &s, double (&acc)[V], double (&vsn)[V],
                                        float (&nv)[V]) {
    float ov[V], op[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const bool term = V == 1 ? s.ft != 0 : ((s.ft >> (8 * j)) & 0xffu) != 0, trunc = V == 1 ? s.fu != 0 : ((s.fu >> (8 * j)) & 0xffu) != 0;
        float boot = 0.0f;
        if constexpr (FV) {
            if (trunc && !term) boot = a.final_values[row * a.ld + n0 + j];
        }
        double d = (double)s.lp[j] - (double)s.old[j];
        d = d < -kRatioLogMax ? -kRatioLogMax : (d > kRatioLogMax ? kRatioLogMax : d);
        const bool d_nan = d != d;
        const double e = exp_rule(d_nan ? 0.0 : d);
        const double w = d_nan ? __longlong_as_double(0x7FF8000000000000ll) : e;
        const double rho = w > a.rho_bar ? a.rho_bar : w;
        const double cs = a.lam * (w > a.c_bar ? a.c_bar : w);
        const double rpg = w > a.pg_rho_bar ? a.pg_rho_bar : w;
        const bool done = term || trunc;
        const double cut = term ? 0.0 : (double)boot;     // the bootstrap of a step that ends its episode
        const double next = done ? cut : (double)nv[j];
        const double r = (double)s.r[j], v = (double)s.v[j];
        const double delta = rho * ((r + a.gamma * next) - v);
        const double gc = a.gamma * cs;
        acc[j] = done ? delta : delta + gc * acc[j];
        const double vs = acc[j] + v;
        const double nvs = done ? next : vsn[j];
        const double pg = rpg * ((r + a.gamma * nvs) - v);
        ov[j] = to_f32(vs);
        op[j] = to_f32(pg);
        vsn[j] = vs;
        nv[j] = s.v[j];
    }
    const int64_t off = row * a.ld_out + n0;
    if constexpr (V == 4) {
        *reinterpret_cast<float4 *>(a.vs + off) = make_float4(ov[0], ov[1], ov[2], ov[3]);
        *reinterpret_cast<float4 *>(a.pg + off) = make_float4(op[0], op[1], op[2], op[3]);
    } else {
        a.vs[off] = ov[0];
        a.pg[off] = op[0];
    }
}

template <typename RT, bool FV, int V>
__global__ void __launch_bounds__(kThreads) vtrace_kernel(const VtArgs a) {
    using S = Slot<RT, V>;
    constexpr int D = kRing, R = kRing + 1;
    const int64_t K = a.K;
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t n0 = (tile * kThreads + threadIdx.x) * V;
        if (n0 >= a.N) continue;       // V = 4 only when N % 4 == 0: a lane's four envs exist together
        double acc[V], vsn[V];
        float nv[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float lv = a.last_value ? a.last_value[n0 + j] : 0.0f;
            acc[j] = 0.0;
            vsn[j] = (double)lv;
            nv[j] = lv;
        }
        // step i handles row K-1-i.  R = D + 1 register sets and a loop unrolled by R, so that every set has a fixed name: set i % R
        // holds row i's loads, and the fetch of row i + D goes into the set that step i - 1 has just released (mxv_gae.hip).  A fetch
        // past the end repeats row 0: in bounds, never consumed.
        auto row_of = [&](int64_t i) { return i < K ? K - 1 - i : (int64_t)0; };
        S ring[R];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            fetch<RT, V>(a, row_of(d), n0, ring[d]);
            __builtin_amdgcn_sched_barrier(0);   // row by row: interleaved, a row's last load would stand behind the next row's first
        }
        // full groups of R steps in a body without exits; the last K % R <= D steps find their sets loaded
        int64_t i0 = 0;
        for (; i0 + R <= K; i0 += R) {
#pragma unroll
            for (int d = 0; d < R; ++d) {
                fetch<RT, V>(a, row_of(i0 + d + D), n0, ring[(d + D) % R]);
                // the scheduler may not sink these loads below the arithmetic of the group (the ring would fill and drain once per
                // group instead of staying D rows deep)
                __builtin_amdgcn_sched_barrier(0);
                consume<RT, FV, V>(a, K - 1 - (i0 + d), n0, ring[d], acc, vsn, nv);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (i0 + d < K) consume<RT, FV, V>(a, K - 1 - (i0 + d), n0, ring[d], acc, vsn, nv);
    }
}

constexpr mxv::policy_host::Call<mxv::VtraceCall> kCall{"mxv_vtrace", 'K'};

// one [K][N] argument: its first byte, the bytes of a row and from one row to the next (0: a single row)
struct Span {
    const char *name;
    uintptr_t lo;
    uint64_t row, stride, rows;
    uintptr_t hi() const { return lo + (uintptr_t)((rows - 1) * stride + row); }
};

// Do two arguments share a byte?  Disjoint whole ranges do not.  Ranges that interleave — column blocks of one wide buffer — are told
// apart when both step by the same number of bytes per row: with b starting r bytes into a's row period, every row of b lies in the
// gap behind a's row iff r >= a.row and r + b.row <= stride.  Anything else counts as shared.  (The allowance of mxv_gae.hip.)
bool shares_bytes(Span a, Span b) {
    if (!a.lo || !b.lo || a.hi() <= b.lo || b.hi() <= a.lo) return false;
    if (a.lo > b.lo) std::swap(a, b);
    if (a.stride == 0 || a.stride != b.stride) return true;
    const uint64_t r = (uint64_t)(b.lo - a.lo) % a.stride;
    return !(r >= a.row && r + b.row <= a.stride);
}

struct LastLaunch {   // of the calling thread (mxv_vtrace_last_launch)
    int32_t envs_per_lane = 0;
    uint32_t grid = 0;
};
LastLaunch &last_launch() {
    thread_local LastLaunch l;
    return l;
}

template <typename RT, bool FV>
const void *kernel_of(bool vec) {
    return vec ? reinterpret_cast<const void *>(&vtrace_kernel<RT, FV, 4>) : reinterpret_cast<const void *>(&vtrace_kernel<RT, FV, 1>);
}

}  // namespace

extern "C" {

int mxv_vtrace(void *stream, int64_t K, int64_t N, const float *lp, const float *old, const void *reward, int32_t reward_is_f64, int64_t ld,
               const uint8_t *term, const uint8_t *trunc, const float *values, const float *last_value, const float *final_values, double gamma,
               double lam, double rho_bar, double c_bar, double pg_rho_bar, float *vs, float *pg, int64_t ld_out) {
    const char *api = kCall.api;
    if (!lp) return kCall.bad("%s: log_prob pointer is NULL", api);
    if (!old) return kCall.bad("%s: old_log_prob pointer is NULL", api);
    if (!reward) return kCall.bad("%s: reward pointer is NULL", api);
    if (!term) return kCall.bad("%s: terminated pointer is NULL", api);
    if (!trunc) return kCall.bad("%s: truncated pointer is NULL", api);
    if (!values) return kCall.bad("%s: values pointer is NULL", api);
    if (!vs) return kCall.bad("%s: vs pointer is NULL", api);
    if (!pg) return kCall.bad("%s: pg_advantages pointer is NULL", api);
    if (K < 1 || N < 1) return kCall.bad("%s: K = %lld and N = %lld must be at least 1", api, (long long)K, (long long)N);
    if (ld < N || ld_out < N)
        return kCall.bad("%s: row strides ld = %lld, ld_out = %lld must be at least N = %lld", api, (long long)ld, (long long)ld_out, (long long)N);
    if (ld > kMaxElems / K || ld_out > kMaxElems / K)
        return kCall.bad("%s: K * ld = %lld * %lld (ld_out %lld) is beyond 2^40 elements", api, (long long)K, (long long)ld, (long long)ld_out);
    if (!std::isfinite(gamma) || !std::isfinite(lam)) return kCall.bad("%s: gamma = %g and lam = %g must be finite", api, gamma, lam);
    struct Level {
        const char *name;
        double x;
    };
    for (const Level &l : {Level{"rho_bar", rho_bar}, Level{"c_bar", c_bar}, Level{"pg_rho_bar", pg_rho_bar}})
        if (!std::isfinite(l.x) || !(l.x > 0.0)) return kCall.bad("%s: %s = %g must be finite and greater than 0", api, l.name, l.x);
    const uint64_t rb = reward_is_f64 ? 8 : 4;
    // an output must not share a byte with an input or with the other output
    auto span = [&](const char *name, const void *p, uint64_t elem, int64_t stride_elems, int64_t rows) {
        return Span{name, (uintptr_t)p, (uint64_t)N * elem, rows > 1 ? (uint64_t)stride_elems * elem : 0, (uint64_t)rows};
    };
    constexpr int kIns = 8, kOuts = 2;
    const Span ins[kIns] = {span("log_prob", lp, 4, ld, K),       span("old_log_prob", old, 4, ld, K),   span("reward", reward, rb, ld, K),
                            span("terminated", term, 1, ld, K),   span("truncated", trunc, 1, ld, K),    span("values", values, 4, ld, K),
                            span("last_value", last_value, 4, 0, 1), span("final_values", final_values, 4, ld, K)};
    const uint64_t in_elem[kIns] = {4, 4, rb, 1, 1, 4, 4, 4};
    const Span outs[kOuts] = {span("vs", vs, 4, ld_out, K), span("pg_advantages", pg, 4, ld_out, K)};
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < (pass ? kOuts : kIns); ++i) {
            const Span &s = pass ? outs[i] : ins[i];
            const uint64_t elem = pass ? 4 : in_elem[i];
            if (s.lo & (elem - 1)) return kCall.bad("%s: %s pointer %p is not %llu-byte aligned", api, s.name, (void *)s.lo, (unsigned long long)elem);
        }
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < (pass ? kOuts : kIns); ++i) {
            const Span &s = pass ? outs[i] : ins[i];
            if (s.lo && (s.rows - 1) * s.stride + s.row > UINTPTR_MAX - s.lo)
                return kCall.bad("%s: %s at %p with K = %lld rows does not fit the address space", api, s.name, (void *)s.lo, (long long)K);
        }
    for (const Span &o : outs)
        for (const Span &i : ins)
            if (shares_bytes(o, i)) return kCall.bad("%s: output %s overlaps input %s", api, o.name, i.name);
    if (shares_bytes(outs[0], outs[1])) return kCall.bad("%s: outputs vs and pg_advantages overlap", api);

    auto al = [](const void *p, uintptr_t b) { return ((uintptr_t)p & (b - 1)) == 0; };
    const bool vec = N >= kVecMinN && N % 4 == 0 && ld % 4 == 0 && ld_out % 4 == 0 && al(lp, 16) && al(old, 16) && al(reward, 16) && al(values, 16) &&
                     al(term, 4) && al(trunc, 4) && al(vs, 16) && al(pg, 16);
    VtArgs a;
    a.lp = lp; a.old = old; a.reward = reward; a.term = term; a.trunc = trunc; a.values = values; a.last_value = last_value;
    a.final_values = final_values; a.vs = vs; a.pg = pg;
    a.K = K; a.N = N; a.ld = ld; a.ld_out = ld_out;
    const int64_t per_tile = (int64_t)kThreads * (vec ? 4 : 1);
    a.tiles = (N + per_tile - 1) / per_tile;
    a.gamma = gamma; a.lam = lam; a.rho_bar = rho_bar; a.c_bar = c_bar; a.pg_rho_bar = pg_rho_bar;
    const bool fv = final_values != nullptr;
    const void *kernel = reward_is_f64 ? (fv ? kernel_of<double, true>(vec) : kernel_of<double, false>(vec))
                                       : (fv ? kernel_of<float, true>(vec) : kernel_of<float, false>(vec));
    if (int rc = kCall.launch(kernel, a, stream)) return rc;
    last_launch() = LastLaunch{vec ? 4 : 1, mxv::policy_host::grid_of(a.tiles).x};
    return MXV_OK;
}

const char *mxv_vtrace_last_error(void) { return mxv::last_error<mxv::VtraceCall>(nullptr); }

int mxv_vtrace_last_launch(int32_t *envs_per_lane, uint32_t *grid) {
    if (!envs_per_lane || !grid) return kCall.bad("mxv_vtrace_last_launch: output pointer is NULL");
    *envs_per_lane = last_launch().envs_per_lane;
    *grid = last_launch().grid;
    return MXV_OK;
}

}  // extern "C"
