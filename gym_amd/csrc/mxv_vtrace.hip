// mxv_vtrace.hip — V-trace value targets and policy-gradient advantages over [K][N] trajectory tensors (include/mxv_vtrace.h,
// DESIGN.md §16).
//
// The recurrence of mxv_gae.hip with truncated importance weights: backwards over the K rows, independent per env, sequential in t and
// parallel in N, evaluated as the rule states it — float64, one rounding per operation (-ffp-contract=off), t = K-1 ... 0 — because
// the result is defined bit for bit.  No scan over K: composing the affine maps acc -> delta + gc acc re-associates the sum.
//
// Shape of the kernel (26 B per env-step with float32 rewards, about 60 float64 operations of which EXP's polynomial is half): the walk
// of mxv_trajectory.hpp, which GAE shares — V envs per lane, the register ring, the grid.  What is this file's own:
//   * a row's loads at V = 4: one dwordx4 each of log_prob, old_log_prob, values and rewards — two for float64 —, one dword of each flag
//     row; dwordx4 stores.
//   * the weights w of a row do not depend on the recurrence, but they are derived values: they are formed when the row is consumed,
//     not kept in the ring.
//   * final_values is loaded only behind (truncated && !terminated), per element: most rows never touch it.
//   * no scratch (tests/test_vtrace_resources.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/mxv_vtrace.h"
#include "mxv_policy_host.hpp"
#include "mxv_policy_rule.hpp"
#include "mxv_trajectory.hpp"

namespace {

using namespace mxv::rule;
using namespace mxv::trajectory;

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

template <typename RT, int V>
__device__ __forceinline__ void fetch(const VtArgs &a, int64_t row, int64_t n0, Slot<RT, V> &s) {
    const int64_t off = row * a.ld + n0;
    const RT *rew = static_cast<const RT *>(a.reward) + off;
    if constexpr (V == 4) {
        load4(a.lp + off, s.lp);
        load4(a.old + off, s.old);
        load_reward<RT, V>(rew, s.r);
        load4(a.values + off, s.v);
        s.ft = *reinterpret_cast<const uint32_t *>(a.term + off);
        s.fu = *reinterpret_cast<const uint32_t *>(a.trunc + off);
    } else {
        s.lp[0] = a.lp[off];
        s.old[0] = a.old[off];
        load_reward<RT, V>(rew, s.r);
        s.v[0] = a.values[off];
        s.ft = a.term[off];
        s.fu = a.trunc[off];
    }
}

// state: acc = acc_{t+1}, vsn = vs_{t+1}, nv = nv_{t+1} (a float32 value, or last_value)
template <typename RT, bool FV, int V>
__device__ __forceinline__ void consume(const VtArgs &a, int64_t row, int64_t n0, const Slot<RT, V> &s, double (&acc)[V], double (&vsn)[V],
                                        float (&nv)[V]) {
    float ov[V], op[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        // V = 1: the byte as loaded (a mask here becomes a derived value that the compiler carries around the loop in the ring's place)
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

template <int V>
__device__ __forceinline__ void init(int j, float last_value, double (&acc)[V], double (&vsn)[V], float (&nv)[V]) {
    acc[j] = 0.0;
    vsn[j] = (double)last_value;
    nv[j] = last_value;
}

template <typename RT, bool FV, int V>
__global__ void __launch_bounds__(kThreads) vtrace_kernel(const VtArgs a) {
    using S = Slot<RT, V>;
    double acc[V], vsn[V];
    float nv[V];
    MXV_TRAJECTORY_WALK(a, V, S, true, (fetch<RT, V>), (init<V>), (consume<RT, FV, V>), acc, vsn, nv)
}

constexpr mxv::policy_host::Call<mxv::VtraceCall> kCall{"mxv_vtrace", 'K'};

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
    if (int rc = check_shape(kCall, K, N, ld, ld_out, gamma, lam)) return rc;
    struct Level {
        const char *name;
        double x;
    };
    for (const Level &l : {Level{"rho_bar", rho_bar}, Level{"c_bar", c_bar}, Level{"pg_rho_bar", pg_rho_bar}})
        if (!std::isfinite(l.x) || !(l.x > 0.0)) return kCall.bad("%s: %s = %g must be finite and greater than 0", api, l.name, l.x);
    const uint64_t rb = reward_is_f64 ? 8 : 4;
    const Span ins[] = {span("log_prob", lp, 4, N, ld, K),           span("old_log_prob", old, 4, N, ld, K),   span("reward", reward, rb, N, ld, K),
                        span("terminated", term, 1, N, ld, K),       span("truncated", trunc, 1, N, ld, K),    span("values", values, 4, N, ld, K),
                        span("last_value", last_value, 4, N, 0, 1), span("final_values", final_values, 4, N, ld, K)};
    const Span outs[] = {span("vs", vs, 4, N, ld_out, K), span("pg_advantages", pg, 4, N, ld_out, K)};
    if (int rc = check_spans(kCall, K, ins, 8, outs, 2)) return rc;

    const bool vec = four_per_lane(N, ld, ld_out, {lp, old, reward, values, vs, pg}, {term, trunc});
    VtArgs a;
    a.lp = lp; a.old = old; a.reward = reward; a.term = term; a.trunc = trunc; a.values = values; a.last_value = last_value;
    a.final_values = final_values; a.vs = vs; a.pg = pg;
    a.K = K; a.N = N; a.ld = ld; a.ld_out = ld_out;
    a.tiles = tiles(N, vec);
    a.gamma = gamma; a.lam = lam; a.rho_bar = rho_bar; a.c_bar = c_bar; a.pg_rho_bar = pg_rho_bar;
    const bool fv = final_values != nullptr;
    const void *kernel = reward_is_f64 ? (fv ? kernel_of<double, true>(vec) : kernel_of<double, false>(vec))
                                       : (fv ? kernel_of<float, true>(vec) : kernel_of<float, false>(vec));
    if (int rc = kCall.launch(kernel, a, stream)) return rc;
    record_launch<mxv::VtraceCall>(vec, a.tiles);
    return MXV_OK;
}

const char *mxv_vtrace_last_error(void) { return mxv::last_error<mxv::VtraceCall>(nullptr); }

int mxv_vtrace_last_launch(int32_t *envs_per_lane, uint32_t *grid) { return report_last_launch(kCall, envs_per_lane, grid); }

}  // extern "C"
