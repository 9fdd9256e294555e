// mxv_gae.hip — GAE(lambda) advantages and discounted returns-to-go over [K][N] trajectory tensors (include/mxv_gae.h).
//
// The recurrence runs backwards over the K rows and is independent per env: sequential in t, parallel in N.  It is evaluated as the
// rule states it — float64, one rounding per operation (this file is built with -ffp-contract=off like the rest of the library), in
// the order t = K-1 ... 0 — because the result is defined bit for bit.  K is NOT split across lanes with a scan over the affine maps
// A -> delta + c A: composing maps re-associates the sum, and the rounded result would differ from the sequential one.
//
// Shape of the kernel (memory bound: 18 B per env-step for GAE with float32 rewards, 10 B for returns):
//   * one lane owns V consecutive envs of every row.  V = 4 when N, both row strides and the base addresses allow 16-byte accesses
//     (one dwordx4 of rewards — two for float64 —, one of values, one dword of each flag row, dwordx4 stores) AND N >= 2^21: the chip
//     has 256 CUs x 32 wave slots x 64 lanes = 524 288 lanes, which four envs per lane fill from 4 x 524 288 = 2^21 envs on; below that
//     V = 1, so that more waves have loads in flight.  The formula counts 32 slots per CU, an occupancy the V = 1 float32 kernels have
//     and the V = 4 ones do not (67-155 VGPRs: 3-7 waves per SIMD, so they fill the chip well below 2^21 envs): it is a conservative
//     switch-over, not a measured optimum — DESIGN.md §11 has the one shape at which V = 4 was timed.
//   * a register ring: the loads of rows t-1 ... t-kRing are issued before row t is consumed, and nothing derived from a load is kept
//     in the ring, so the wait in front of row t is a counted one (vmcnt(n), n > 0), never a drain.  The loads of a row do not depend
//     on the recurrence.  kRing = 4: with every wave slot filled that is 4 rows x 10 B (V = 1) or 40 B (V = 4) x 524 288 lanes = 21 to
//     84 MB in flight, an order of magnitude beyond bandwidth x latency of the HBM; the widest instantiation (float64 rewards, V = 4,
//     final_values: 14 registers per ring entry, five entries) takes 155 VGPRs of the 512 a lane may have; at V = 1 the float32
//     instantiations without final_values fit 64 (8 waves per SIMD, the 32 slots per CU counted above), the others at most 88 (5 waves);
//     none has any scratch (tests/test_gae_resources.py).
//   * final_values is loaded only behind (truncated && !terminated), per element: most rows never touch it.  That load is the
//     youngest in flight, so the wave that takes the branch drains its ring once; truncations are rare.
//   * no atomics, no LDS, no inline assembly.  Grid: at most kMaxBlocks workgroups of 256 lanes (all wave slots of the chip), each
//     striding over tiles of 256 V envs.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <utility>

#include "../../include/mxv_gae.h"
#include "mxv_host.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kRing = 4;            // rows in flight ahead of the one being consumed (gym_amd/returns.py: RING_DEPTH)
constexpr int kMaxBlocks = 2048;    // 256 CUs x 8 workgroups of 4 waves = every wave slot
constexpr int64_t kVecMinN = (int64_t)4 * 256 * 32 * 64;   // 2^21: see the header comment
constexpr int64_t kMaxElems = (int64_t)1 << 40;

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
    const RT *rew = static_cast<const RT *>(a.reward) + off;
    if constexpr (V == 4) {
        if constexpr (sizeof(RT) == 8) {
            const double2 x = reinterpret_cast<const double2 *>(rew)[0], y = reinterpret_cast<const double2 *>(rew)[1];
            s.r[0] = x.x; s.r[1] = x.y; s.r[2] = y.x; s.r[3] = y.y;
        } else {
            const float4 x = *reinterpret_cast<const float4 *>(rew);
            s.r[0] = x.x; s.r[1] = x.y; s.r[2] = x.z; s.r[3] = x.w;
        }
        if constexpr (GAE) {
            const float4 x = *reinterpret_cast<const float4 *>(a.values + off);
            s.v[0] = x.x; s.v[1] = x.y; s.v[2] = x.z; s.v[3] = x.w;
        }
        s.ft = *reinterpret_cast<const uint32_t *>(a.term + off);
        s.fu = *reinterpret_cast<const uint32_t *>(a.trunc + off);
    } else {
        s.r[0] = rew[0];
        if constexpr (GAE) s.v[0] = a.values[off];
        s.ft = a.term[off];
        s.fu = a.trunc[off];
    }
}

__device__ __forceinline__ float to_f32(double x) {
    const float f = (float)x;                            // round to nearest even, subnormals kept
    return f != f ? __uint_as_float(0x7FC00000u) : f;    // one NaN pattern (mxv_gae.h)
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

template <typename RT, bool GAE, bool FV, int V>
__global__ void __launch_bounds__(kThreads) gae_kernel(const GaeArgs a) {
    using S = Slot<RT, GAE, V>;
    constexpr int D = kRing, R = kRing + 1;
    const int64_t K = a.K;
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t n0 = (tile * kThreads + threadIdx.x) * V;
        if (n0 >= a.N) continue;       // V = 4 only when N % 4 == 0: a lane's four envs exist together
        double acc[V];
        float nv[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float lv = a.last_value ? a.last_value[n0 + j] : 0.0f;
            acc[j] = GAE ? 0.0 : (double)lv;
            nv[j] = lv;
        }
        // step i handles row K-1-i.  The ring has R = D + 1 register sets and the loop is unrolled by R, so that every set has a fixed
        // name: set i % R holds row i's loads, and the fetch of row i + D goes into the set that step i - 1 has just released.  (With D
        // sets and a copy of the current one the loop-carried values change registers, and the copies wait for loads in flight.)
        // A fetch past the end repeats row 0: in bounds, never consumed.
        auto row_of = [&](int64_t i) { return i < K ? K - 1 - i : (int64_t)0; };
        S ring[R];
#pragma unroll
        for (int d = 0; d < D; ++d) fetch<RT, GAE, V>(a, row_of(d), n0, ring[d]);
        // full groups of R steps in a body without exits (an exit between the unrolled steps would put a join, and a drain of the
        // ring, there); the last K % R <= D steps find their sets loaded
        int64_t i0 = 0;
        for (; i0 + R <= K; i0 += R) {
#pragma unroll
            for (int d = 0; d < R; ++d) {
                fetch<RT, GAE, V>(a, row_of(i0 + d + D), n0, ring[(d + D) % R]);
                // the scheduler may not sink these loads below the arithmetic of the group (it does, left alone: the ring then
                // fills and drains once per group instead of staying D rows deep)
                __builtin_amdgcn_sched_barrier(0);
                consume<RT, GAE, FV, V>(a, K - 1 - (i0 + d), n0, ring[d], acc, nv);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (i0 + d < K) consume<RT, GAE, FV, V>(a, K - 1 - (i0 + d), n0, ring[d], acc, nv);
    }
}

struct GaeCall {   // the error slot of the two handle-free calls: one per thread (mxv::create_error)
    std::string error;
};

template <typename... A>
int bad(const char *fmt, A... args) {
    return mxv::fail<GaeCall>(nullptr, MXV_ERR_INVALID_ARG, fmt, args...);
}

// one [K][N] argument: its first byte, the bytes of a row and from one row to the next (0: a single row)
struct Span {
    const char *name;
    uintptr_t lo;
    uint64_t row, stride, rows;
    uintptr_t hi() const { return lo + (uintptr_t)((rows - 1) * stride + row); }
};

// Do two arguments share a byte?  Disjoint whole ranges do not.  Ranges that interleave — column blocks of one wide buffer, the use
// strided views invite — are told apart when both step by the same number of bytes per row: with b starting r bytes into a's row
// period, every row of b lies in the gap behind a's row iff r >= a.row and r + b.row <= stride.  Anything else counts as shared.
bool shares_bytes(Span a, Span b) {
    if (!a.lo || !b.lo || a.hi() <= b.lo || b.hi() <= a.lo) return false;
    if (a.lo > b.lo) std::swap(a, b);
    if (a.stride == 0 || a.stride != b.stride) return true;
    const uint64_t r = (uint64_t)(b.lo - a.lo) % a.stride;
    return !(r >= a.row && r + b.row <= a.stride);
}

struct LastLaunch {   // of the calling thread (mxv_gae_last_launch)
    int32_t envs_per_lane = 0;
    uint32_t grid = 0;
};
LastLaunch &last_launch() {
    thread_local LastLaunch l;
    return l;
}

template <typename RT, bool GAE, bool FV>
hipError_t launch_v(bool vec, dim3 grid, hipStream_t st, GaeArgs &a) {
    void *args[] = {&a};
    // hipLaunchKernel returns THIS launch's status (hipGetLastError would also report, and clear, an earlier call's error)
    if (vec) return hipLaunchKernel(reinterpret_cast<const void *>(&gae_kernel<RT, GAE, FV, 4>), grid, dim3(kThreads), args, 0, st);
    return hipLaunchKernel(reinterpret_cast<const void *>(&gae_kernel<RT, GAE, FV, 1>), grid, dim3(kThreads), args, 0, st);
}

template <bool GAE>
int run(const char *api, void *stream, int64_t K, int64_t N, const void *reward, int32_t reward_is_f64, int64_t ld, const uint8_t *term,
        const uint8_t *trunc, const float *values, const float *last_value, const float *final_values, double gamma, double lam,
        float *adv, float *ret, int64_t ld_out) {
    if (!reward) return bad("%s: reward pointer is NULL", api);
    if (!term) return bad("%s: terminated pointer is NULL", api);
    if (!trunc) return bad("%s: truncated pointer is NULL", api);
    if (GAE && !values) return bad("%s: values pointer is NULL", api);
    if (GAE && !adv) return bad("%s: advantages pointer is NULL", api);
    if (!ret) return bad("%s: returns pointer is NULL", api);
    if (K < 1 || N < 1) return bad("%s: K = %lld and N = %lld must be at least 1", api, (long long)K, (long long)N);
    if (ld < N || ld_out < N) return bad("%s: row strides ld = %lld, ld_out = %lld must be at least N = %lld", api, (long long)ld, (long long)ld_out, (long long)N);
    if (ld > kMaxElems / K || ld_out > kMaxElems / K)
        return bad("%s: K * ld = %lld * %lld (ld_out %lld) is beyond 2^40 elements", api, (long long)K, (long long)ld, (long long)ld_out);
    if (!std::isfinite(gamma) || !std::isfinite(lam)) return bad("%s: gamma = %g and lam = %g must be finite", api, gamma, lam);
    const size_t rb = reward_is_f64 ? 8 : 4;
    struct Aligned {
        const char *name;
        const void *p;
        size_t bytes;
    };
    for (const Aligned &x : {Aligned{"reward", reward, rb}, Aligned{"values", values, 4}, Aligned{"last_value", last_value, 4},
                             Aligned{"final_values", final_values, 4}, Aligned{"advantages", adv, 4}, Aligned{"returns", ret, 4}})
        if ((uintptr_t)x.p & (x.bytes - 1)) return bad("%s: %s pointer %p is not %zu-byte aligned", api, x.name, x.p, x.bytes);
    // an output must not share a byte with an input or with the other output
    auto span = [&](const char *name, const void *p, uint64_t elem, int64_t stride_elems, int64_t rows) {
        return Span{name, (uintptr_t)p, (uint64_t)N * elem, rows > 1 ? (uint64_t)stride_elems * elem : 0, (uint64_t)rows};
    };
    const Span ins[] = {span("reward", reward, rb, ld, K), span("terminated", term, 1, ld, K), span("truncated", trunc, 1, ld, K),
                        span("values", values, 4, ld, K), span("last_value", last_value, 4, 0, 1), span("final_values", final_values, 4, ld, K)};
    const Span outs[] = {span("advantages", adv, 4, ld_out, K), span("returns", ret, 4, ld_out, K)};
    for (const Span *list : {ins, outs})
        for (int i = 0; i < (list == ins ? 6 : 2); ++i)
            if (list[i].lo && (list[i].rows - 1) * list[i].stride + list[i].row > UINTPTR_MAX - list[i].lo)
                return bad("%s: %s at %p with K = %lld rows does not fit the address space", api, list[i].name, (void *)list[i].lo, (long long)K);
    for (const Span &o : outs)
        for (const Span &i : ins)
            if (shares_bytes(o, i)) return bad("%s: output %s overlaps input %s", api, o.name, i.name);
    if (shares_bytes(outs[0], outs[1])) return bad("%s: outputs advantages and returns overlap", api);

    auto al = [](const void *p, uintptr_t b) { return ((uintptr_t)p & (b - 1)) == 0; };
    const bool vec = N >= kVecMinN && N % 4 == 0 && ld % 4 == 0 && ld_out % 4 == 0 && al(reward, 16) && al(values, 16) && al(term, 4) && al(trunc, 4) &&
                     al(adv, 16) && al(ret, 16);
    GaeArgs a;
    a.reward = reward; a.term = term; a.trunc = trunc; a.values = values; a.last_value = last_value; a.final_values = final_values;
    a.adv = adv; a.ret = ret;
    a.K = K; a.N = N; a.ld = ld; a.ld_out = ld_out;
    const int64_t per_tile = (int64_t)kThreads * (vec ? 4 : 1);
    a.tiles = (N + per_tile - 1) / per_tile;
    a.gamma = gamma;
    a.c = gamma * lam;      // formed once, in double
    const dim3 grid((unsigned)(a.tiles < kMaxBlocks ? a.tiles : kMaxBlocks));
    hipStream_t st = (hipStream_t)stream;
    const bool fv = final_values != nullptr;
    hipError_t e;
    if (reward_is_f64) e = fv ? launch_v<double, GAE, true>(vec, grid, st, a) : launch_v<double, GAE, false>(vec, grid, st, a);
    else e = fv ? launch_v<float, GAE, true>(vec, grid, st, a) : launch_v<float, GAE, false>(vec, grid, st, a);
    if (e != hipSuccess) return mxv::fail<GaeCall>(nullptr, MXV_ERR_HIP, "%s: kernel launch: %s", api, hipGetErrorString(e));
    last_launch() = LastLaunch{vec ? 4 : 1, grid.x};
    return MXV_OK;
}

}  // namespace

extern "C" {

int mxv_gae(void *stream, int64_t K, int64_t N, const void *reward_dev, int32_t reward_is_f64, int64_t ld, const uint8_t *terminated_dev,
            const uint8_t *truncated_dev, const float *values_dev, const float *last_value_dev, const float *final_values_dev,
            double gamma, double lam, float *advantages_dev, float *returns_dev, int64_t ld_out) {
    return run<true>("mxv_gae", stream, K, N, reward_dev, reward_is_f64, ld, terminated_dev, truncated_dev, values_dev, last_value_dev,
                     final_values_dev, gamma, lam, advantages_dev, returns_dev, ld_out);
}

int mxv_discounted_returns(void *stream, int64_t K, int64_t N, const void *reward_dev, int32_t reward_is_f64, int64_t ld,
                           const uint8_t *terminated_dev, const uint8_t *truncated_dev, const float *last_value_dev,
                           const float *final_values_dev, double gamma, float *returns_dev, int64_t ld_out) {
    return run<false>("mxv_discounted_returns", stream, K, N, reward_dev, reward_is_f64, ld, terminated_dev, truncated_dev, nullptr,
                      last_value_dev, final_values_dev, gamma, 0.0, nullptr, returns_dev, ld_out);
}

const char *mxv_gae_last_error(void) { return mxv::last_error<GaeCall>(nullptr); }

int mxv_gae_last_launch(int32_t *envs_per_lane, uint32_t *grid) {
    if (!envs_per_lane || !grid) return bad("mxv_gae_last_launch: output pointer is NULL");
    *envs_per_lane = last_launch().envs_per_lane;
    *grid = last_launch().grid;
    return MXV_OK;
}

}  // extern "C"
