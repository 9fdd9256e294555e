// mxv_gae.hip — GAE(lambda) advantages and discounted returns-to-go over [K][N] trajectory tensors (include/mxv_gae.h).
//
// The recurrence runs backwards over the K rows and is independent per env: sequential in t, parallel in N.  It is evaluated as the
// rule states it — float64, one rounding per operation (this file is built with -ffp-contract=off like the rest of the library), in
// the order t = K-1 ... 0 — because the result is defined bit for bit.  K is NOT split across lanes with a scan over the affine maps
// A -> delta + c A: composing maps re-associates the sum, and the rounded result would differ from the sequential one.
//
// Shape of the kernel (memory bound: 18 B per env-step for GAE with float32 rewards, 10 B for returns): the walk of
// mxv_trajectory.hpp, which V-trace shares — V envs per lane, the register ring, the grid.  What is this file's own:
//   * a row's loads at V = 4: one dwordx4 of rewards — two for float64 —, one of values, one dword of each flag row; dwordx4 stores.
//     The switch-over N >= 2^21 counts 32 wave slots per CU, an occupancy the V = 1 float32 kernels have and the V = 4 ones do not
//     (67-155 VGPRs: 3-7 waves per SIMD, so they fill the chip well below 2^21 envs) — DESIGN.md §11 has the one shape at which V = 4
//     was timed.
//   * kRing = 4: with every wave slot filled that is 4 rows x 10 B (V = 1) or 40 B (V = 4) x 524 288 lanes = 21 to 84 MB in flight,
//     an order of magnitude beyond bandwidth x latency of the HBM; the widest instantiation (float64 rewards, V = 4, final_values:
//     14 registers per ring entry, five entries) takes 155 VGPRs of the 512 a lane may have; at V = 1 the float32 instantiations
//     without final_values fit 64 (8 waves per SIMD, the 32 slots per CU counted above), the others at most 88 (5 waves); none has
//     any scratch (tests/test_gae_resources.py).
//   * final_values is loaded only behind (truncated && !terminated), per element: most rows never touch it.  That load is the
//     youngest in flight, so the wave that takes the branch drains its ring once; truncations are rare.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mxv_gae.h"
#include "mxv_policy_host.hpp"
#include "mxv_policy_rule.hpp"
#include "mxv_trajectory.hpp"

namespace {

using namespace mxv::rule;
using namespace mxv::trajectory;

struct GaeArgs {
    const void *reward;
    const uint8_t *term, *trunc;
    const float *values, *last_value, *final_values;
    float *adv, *ret;
    int64_t K, N, ld, ld_out, tiles;
    double gamma, c;
};

// what the loads of one row return for a lane, and nothing derived from it
template <typename RT, bool GAE, int V>
struct Slot {
    RT r[V];
    float v[GAE ? V : 1];
    uint32_t ft, fu;   // V = 4: the dword of four flag bytes; V = 1: the byte
};

template <typename RT, bool GAE, int V>
__device__ __forceinline__ void fetch(const GaeArgs &a, int64_t row, int64_t n0, Slot<RT, GAE, V> &s) {
    const int64_t off = row * a.ld + n0;
    load_reward<RT, V>(static_cast<const RT *>(a.reward) + off, s.r);
    if constexpr (V == 4) {
        if constexpr (GAE) load4(a.values + off, s.v);
        s.ft = *reinterpret_cast<const uint32_t *>(a.term + off);
        s.fu = *reinterpret_cast<const uint32_t *>(a.trunc + off);
    } else {
        if constexpr (GAE) s.v[0] = a.values[off];
        s.ft = a.term[off];
        s.fu = a.trunc[off];
    }
}

// state: GAE  acc = A_{t+1}, nv = nv_{t+1} (a float32 value, or last_value);  returns  acc = G_{t+1}
template <typename RT, bool GAE, bool FV, int V>
__device__ __forceinline__ void consume(const GaeArgs &a, int64_t row, int64_t n0, const Slot<RT, GAE, V> &s, double (&acc)[V], float (&nv)[V]) {
    float oa[V], og[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        // V = 1: the byte as loaded (a mask here becomes a derived value that the compiler carries around the loop in the ring's place)
        const bool term = V == 1 ? s.ft != 0 : ((s.ft >> (8 * j)) & 0xffu) != 0, trunc = V == 1 ? s.fu != 0 : ((s.fu >> (8 * j)) & 0xffu) != 0;
        float boot = 0.0f;
        if constexpr (FV) {
            if (trunc && !term) boot = a.final_values[row * a.ld + n0 + j];
        }
        const double cut = term ? 0.0 : (double)boot;     // the bootstrap of a step that ends its episode
        if constexpr (GAE) {
            const double next = (term || trunc) ? cut : (double)nv[j];
            const double delta = ((double)s.r[j] + a.gamma * next) - (double)s.v[j];
            acc[j] = (term || trunc) ? delta : delta + a.c * acc[j];
            oa[j] = to_f32(acc[j]);
            og[j] = to_f32(acc[j] + (double)s.v[j]);
            nv[j] = s.v[j];
        } else {
            const double next = (term || trunc) ? cut : acc[j];
            acc[j] = (double)s.r[j] + a.gamma * next;
            og[j] = to_f32(acc[j]);
        }
    }
    const int64_t off = row * a.ld_out + n0;
    if constexpr (V == 4) {
        if constexpr (GAE) *reinterpret_cast<float4 *>(a.adv + off) = make_float4(oa[0], oa[1], oa[2], oa[3]);
        *reinterpret_cast<float4 *>(a.ret + off) = make_float4(og[0], og[1], og[2], og[3]);
    } else {
        if constexpr (GAE) a.adv[off] = oa[0];
        a.ret[off] = og[0];
    }
}

template <bool GAE, int V>
__device__ __forceinline__ void init(int j, float last_value, double (&acc)[V], float (&nv)[V]) {
    acc[j] = GAE ? 0.0 : (double)last_value;
    nv[j] = last_value;
}

template <typename RT, bool GAE, bool FV, int V>
__global__ void __launch_bounds__(kThreads) gae_kernel(const GaeArgs a) {
    using S = Slot<RT, GAE, V>;
    double acc[V];
    float nv[V];
    MXV_TRAJECTORY_WALK(a, V, S, false, (fetch<RT, GAE, V>), (init<GAE, V>), (consume<RT, GAE, FV, V>), acc, nv)
}

constexpr mxv::policy_host::Call<mxv::GaeCall> kGae{"mxv_gae", 'K'}, kReturns{"mxv_discounted_returns", 'K'};

template <typename RT, bool GAE, bool FV>
const void *kernel_of(bool vec) {
    return vec ? reinterpret_cast<const void *>(&gae_kernel<RT, GAE, FV, 4>) : reinterpret_cast<const void *>(&gae_kernel<RT, GAE, FV, 1>);
}

template <bool GAE>
int run(void *stream, int64_t K, int64_t N, const void *reward, int32_t reward_is_f64, int64_t ld, const uint8_t *term, const uint8_t *trunc,
        const float *values, const float *last_value, const float *final_values, double gamma, double lam, float *adv, float *ret,
        int64_t ld_out) {
    const auto &call = GAE ? kGae : kReturns;
    const char *api = call.api;
    if (!reward) return call.bad("%s: reward pointer is NULL", api);
    if (!term) return call.bad("%s: terminated pointer is NULL", api);
    if (!trunc) return call.bad("%s: truncated pointer is NULL", api);
    if (GAE && !values) return call.bad("%s: values pointer is NULL", api);
    if (GAE && !adv) return call.bad("%s: advantages pointer is NULL", api);
    if (!ret) return call.bad("%s: returns pointer is NULL", api);
    if (int rc = check_shape(call, K, N, ld, ld_out, gamma, lam)) return rc;
    const uint64_t rb = reward_is_f64 ? 8 : 4;
    const Span ins[] = {span("reward", reward, rb, N, ld, K),     span("terminated", term, 1, N, ld, K),         span("truncated", trunc, 1, N, ld, K),
                        span("values", values, 4, N, ld, K),      span("last_value", last_value, 4, N, 0, 1), span("final_values", final_values, 4, N, ld, K)};
    const Span outs[] = {span("advantages", adv, 4, N, ld_out, K), span("returns", ret, 4, N, ld_out, K)};
    if (int rc = check_spans(call, K, ins, 6, outs, 2)) return rc;

    const bool vec = four_per_lane(N, ld, ld_out, {reward, values, adv, ret}, {term, trunc});
    GaeArgs a;
    a.reward = reward; a.term = term; a.trunc = trunc; a.values = values; a.last_value = last_value; a.final_values = final_values;
    a.adv = adv; a.ret = ret;
    a.K = K; a.N = N; a.ld = ld; a.ld_out = ld_out;
    a.tiles = tiles(N, vec);
    a.gamma = gamma;
    a.c = gamma * lam;      // formed once, in double
    const bool fv = final_values != nullptr;
    const void *kernel = reward_is_f64 ? (fv ? kernel_of<double, GAE, true>(vec) : kernel_of<double, GAE, false>(vec))
                                       : (fv ? kernel_of<float, GAE, true>(vec) : kernel_of<float, GAE, false>(vec));
    if (int rc = call.launch(kernel, a, stream)) return rc;
    record_launch<mxv::GaeCall>(vec, a.tiles);
    return MXV_OK;
}

}  // namespace

extern "C" {

int mxv_gae(void *stream, int64_t K, int64_t N, const void *reward_dev, int32_t reward_is_f64, int64_t ld, const uint8_t *terminated_dev,
            const uint8_t *truncated_dev, const float *values_dev, const float *last_value_dev, const float *final_values_dev,
            double gamma, double lam, float *advantages_dev, float *returns_dev, int64_t ld_out) {
    return run<true>(stream, K, N, reward_dev, reward_is_f64, ld, terminated_dev, truncated_dev, values_dev, last_value_dev, final_values_dev,
                     gamma, lam, advantages_dev, returns_dev, ld_out);
}

int mxv_discounted_returns(void *stream, int64_t K, int64_t N, const void *reward_dev, int32_t reward_is_f64, int64_t ld,
                           const uint8_t *terminated_dev, const uint8_t *truncated_dev, const float *last_value_dev,
                           const float *final_values_dev, double gamma, float *returns_dev, int64_t ld_out) {
    return run<false>(stream, K, N, reward_dev, reward_is_f64, ld, terminated_dev, truncated_dev, nullptr, last_value_dev, final_values_dev,
                      gamma, 0.0, nullptr, returns_dev, ld_out);
}

const char *mxv_gae_last_error(void) { return mxv::last_error<mxv::GaeCall>(nullptr); }

int mxv_gae_last_launch(int32_t *envs_per_lane, uint32_t *grid) { return report_last_launch(kGae, envs_per_lane, grid); }

}  // extern "C"
