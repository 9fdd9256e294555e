// mxv_trajectory.hpp — what the two [K][N] trajectory recurrences share (mxv_gae.hip: include/mxv_gae.h; mxv_vtrace.hip:
// include/mxv_vtrace.h), written once: how a lane walks the K rows of its envs behind a register ring, the loads and the
// float32 conversion of the rule, and the host checks of [K][N] arguments.  Each file keeps what is its own: its argument struct, what
// a row's loads are (Slot, fetch) and the recurrence (consume).
//
// The walk.  One lane owns V consecutive envs of every row and goes backwards over the rows, t = K-1 ... 0: sequential in t, parallel
// in N.  V = 4 when N, both row strides and the base addresses allow 16-byte accesses AND N >= kVecMinN = 2^21: the chip has 256 CUs x
// 32 wave slots x 64 lanes = 524 288 lanes, which four envs per lane fill from 4 x 524 288 = 2^21 envs on; below that V = 1, so that
// more waves have loads in flight.  It is a conservative switch-over, not a measured optimum.  The loads of rows
// t-1 ... t-kRing are issued before row t is consumed, and nothing derived from a load is kept in the ring, so the wait in front of row
// t is a counted one (vmcnt(n), n > 0), never a drain (tests/test_gae_resources.py, tests/test_vtrace_resources.py).  Grid: at most
// kMaxBlocks workgroups of kThreads lanes, each striding over tiles of kThreads V envs.  No atomics, no LDS, no inline assembly.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <utility>

#include "mxv_policy_host.hpp"
#include "mxv_policy_rule.hpp"

namespace mxv {
namespace trajectory {

constexpr int kRing = 4;            // rows in flight ahead of the one being consumed (gym_amd/_trajectory_args.py: RING_DEPTH)
constexpr int64_t kVecMinN = (int64_t)4 * 256 * 32 * 64;   // 2^21: see the header comment (VECTOR_MIN_ENVS)

// ---- device: the pieces of a row ----
__device__ __forceinline__ float to_f32(double x) {
    const float f = (float)x;                            // round to nearest even, subnormals kept
    return f != f ? __uint_as_float(0x7FC00000u) : f;    // one NaN pattern (mxv_gae.h, mxv_vtrace.h)
}

__device__ __forceinline__ void load4(const float *p, float (&x)[4]) {
    const float4 q = *reinterpret_cast<const float4 *>(p);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
}

// V rewards: one dwordx4 of float32, two of float64
template <typename RT, int V>
__device__ __forceinline__ void load_reward(const RT *rew, RT (&r)[V]) {
    if constexpr (V == 4) {
        if constexpr (sizeof(RT) == 8) {
            const double2 x = reinterpret_cast<const double2 *>(rew)[0], y = reinterpret_cast<const double2 *>(rew)[1];
            r[0] = x.x; r[1] = x.y; r[2] = y.x; r[3] = y.y;
        } else {
            load4(rew, r);
        }
    } else {
        r[0] = rew[0];
    }
}

// ---- device: the tile / ring walk ----
// The body of a __global__ function, as one text.  A macro, because every function this body was put into (the struct by value or by
// reference; lambdas, capturing or not; fetch and consume as template arguments; the whole walk or one tile of it) came out of the
// compiler as other code in all 24 instantiations, and the text in the kernel itself does not (profiles/trajectory_refactor).
//   a         the kernel's argument struct: K, N, tiles, last_value
//   V, S      envs per lane; what the loads of one row return for a lane
//   BARRIER   true: a sched_barrier behind each fetch of the prologue, row by row (interleaved, a row's last load would stand behind
//             the next row's first).  V-trace has it and GAE does not, each as it was tuned.
//   FETCH     (a, row, n0, slot)
//   INIT      (j, last_value of lane-env j, state...), once per tile for each of the lane's envs
//   CONSUME   (a, row, n0, slot, state...)
//   ...       the state: what the recurrence carries from row t+1 to row t, plain arrays that the kernel declares in front (gathered
//             into one struct they come out in other registers)
// Every argument that names a template-id is passed parenthesised, so that a comma in its template arguments cannot split it.  The
// body declares D, R, K, tile, n0, j, d, i0, row_of and ring in a block of its own: a kernel that uses the macro keeps these names out
// of the arguments it passes (an argument named K or n0 would be read as the body's).
// Step i handles row K-1-i.  The ring has R = D + 1 register sets and the loop is unrolled by R, so that every set has a fixed name: set
// i % R holds row i's loads, and the fetch of row i + D goes into the set that step i - 1 has just released.  (With D sets and a copy of
// the current one the loop-carried values change registers, and the copies wait for loads in flight.)  A fetch past the end repeats row
// 0: in bounds, never consumed.  Full groups of R steps run in a body without exits (an exit between the unrolled steps would put a
// join, and a drain of the ring, there); the last K % R <= D steps find their sets loaded.  The sched_barrier behind a group's fetch:
// the scheduler may not sink these loads below the arithmetic of the group (it does, left alone: the ring then fills and drains once
// per group instead of staying D rows deep).  The n0 >= N skip: V = 4 only when N % 4 == 0, so a lane's four envs exist together.
#define MXV_TRAJECTORY_WALK(a, V, S, BARRIER, FETCH, INIT, CONSUME, ...)                                                      \
    {                                                                                                                         \
        constexpr int D = mxv::trajectory::kRing, R = mxv::trajectory::kRing + 1;                                             \
        const int64_t K = (a).K;                                                                                              \
        for (int64_t tile = blockIdx.x; tile < (a).tiles; tile += gridDim.x) {                                                \
            const int64_t n0 = (tile * mxv::rule::kThreads + threadIdx.x) * V;                                                \
            if (n0 >= (a).N) continue;                                                                                        \
            _Pragma("unroll") for (int j = 0; j < V; ++j) INIT(j, (a).last_value ? (a).last_value[n0 + j] : 0.0f, __VA_ARGS__);\
            auto row_of = [&](int64_t i) { return i < K ? K - 1 - i : (int64_t)0; };                                          \
            S ring[R];                                                                                                        \
            _Pragma("unroll") for (int d = 0; d < D; ++d) {                                                                   \
                FETCH((a), row_of(d), n0, ring[d]);                                                                           \
                if constexpr (BARRIER) __builtin_amdgcn_sched_barrier(0);                                                     \
            }                                                                                                                 \
            int64_t i0 = 0;                                                                                                   \
            for (; i0 + R <= K; i0 += R) {                                                                                    \
                _Pragma("unroll") for (int d = 0; d < R; ++d) {                                                               \
                    FETCH((a), row_of(i0 + d + D), n0, ring[(d + D) % R]);                                                    \
                    __builtin_amdgcn_sched_barrier(0);                                                                        \
                    CONSUME((a), K - 1 - (i0 + d), n0, ring[d], __VA_ARGS__);                                                 \
                    __builtin_amdgcn_sched_barrier(0);                                                                        \
                }                                                                                                             \
            }                                                                                                                 \
            _Pragma("unroll") for (int d = 0; d < D; ++d) if (i0 + d < K) CONSUME((a), K - 1 - (i0 + d), n0, ring[d], __VA_ARGS__);\
        }                                                                                                                     \
    }

// ---- host: the checks of [K][N] arguments, before the device is touched ----
// one [K][N] argument: its first byte, the bytes of a row and from one row to the next (0: a single row), of elements of `elem` bytes
struct Span {
    const char *name;
    uintptr_t lo;
    uint64_t row, stride, rows, elem;
    uintptr_t hi() const { return lo + (uintptr_t)((rows - 1) * stride + row); }
};
inline Span span(const char *name, const void *p, uint64_t elem, int64_t N, int64_t stride_elems, int64_t rows) {
    return Span{name, (uintptr_t)p, (uint64_t)N * elem, rows > 1 ? (uint64_t)stride_elems * elem : 0, (uint64_t)rows, elem};
}

// Do two arguments share a byte?  Disjoint whole ranges do not.  Ranges that interleave — column blocks of one wide buffer, the use
// strided views invite — are told apart when both step by the same number of bytes per row: with b starting r bytes into a's row
// period, every row of b lies in the gap behind a's row iff r >= a.row and r + b.row <= stride.  Anything else counts as shared.
inline bool shares_bytes(Span a, Span b) {
    if (!a.lo || !b.lo || a.hi() <= b.lo || b.hi() <= a.lo) return false;
    if (a.lo > b.lo) std::swap(a, b);
    if (a.stride == 0 || a.stride != b.stride) return true;
    const uint64_t r = (uint64_t)(b.lo - a.lo) % a.stride;
    return !(r >= a.row && r + b.row <= a.stride);
}

// alignment of every span, then the address-space fit of every span; then no output may share a byte with an input or with another output
template <class Slot>
int check_spans(const policy_host::Call<Slot> &call, int64_t K, const Span *ins, int n_in, const Span *outs, int n_out) {
    for (int pass = 0; pass < 4; ++pass) {
        const Span *list = pass % 2 ? outs : ins;
        for (int i = 0; i < (pass % 2 ? n_out : n_in); ++i) {
            const Span &s = list[i];
            if (pass < 2 && (s.lo & (s.elem - 1)))
                return call.bad("%s: %s pointer %p is not %llu-byte aligned", call.api, s.name, (void *)s.lo, (unsigned long long)s.elem);
            if (pass >= 2 && s.lo && (s.rows - 1) * s.stride + s.row > UINTPTR_MAX - s.lo)
                return call.bad("%s: %s at %p with K = %lld rows does not fit the address space", call.api, s.name, (void *)s.lo, (long long)K);
        }
    }
    for (int o = 0; o < n_out; ++o)
        for (int i = 0; i < n_in; ++i)
            if (shares_bytes(outs[o], ins[i])) return call.bad("%s: output %s overlaps input %s", call.api, outs[o].name, ins[i].name);
    for (int o = 0; o < n_out; ++o)
        for (int p = o + 1; p < n_out; ++p)
            if (shares_bytes(outs[o], outs[p])) return call.bad("%s: outputs %s and %s overlap", call.api, outs[o].name, outs[p].name);
    return MXV_OK;
}

template <class Slot>
int check_shape(const policy_host::Call<Slot> &call, int64_t K, int64_t N, int64_t ld, int64_t ld_out, double gamma, double lam) {
    const char *api = call.api;
    if (K < 1 || N < 1) return call.bad("%s: K = %lld and N = %lld must be at least 1", api, (long long)K, (long long)N);
    if (ld < N || ld_out < N)
        return call.bad("%s: row strides ld = %lld, ld_out = %lld must be at least N = %lld", api, (long long)ld, (long long)ld_out, (long long)N);
    if (ld > rule::kMaxElems / K || ld_out > rule::kMaxElems / K)
        return call.bad("%s: K * ld = %lld * %lld (ld_out %lld) is beyond 2^40 elements", api, (long long)K, (long long)ld, (long long)ld_out);
    if (!std::isfinite(gamma) || !std::isfinite(lam)) return call.bad("%s: gamma = %g and lam = %g must be finite", api, gamma, lam);
    return MXV_OK;
}

// V = 4 for the whole call?  p16: the pointers read and written 16 bytes at a time, p4: the flag rows (a dword of four); NULL passes
inline bool four_per_lane(int64_t N, int64_t ld, int64_t ld_out, std::initializer_list<const void *> p16, std::initializer_list<const void *> p4) {
    bool ok = N >= kVecMinN && N % 4 == 0 && ld % 4 == 0 && ld_out % 4 == 0;
    for (const void *p : p16) ok = ok && ((uintptr_t)p & 15) == 0;
    for (const void *p : p4) ok = ok && ((uintptr_t)p & 3) == 0;
    return ok;
}

inline int64_t tiles(int64_t N, bool vec) {
    const int64_t per_tile = (int64_t)rule::kThreads * (vec ? 4 : 1);
    return (N + per_tile - 1) / per_tile;
}

// the calling thread's last launch of the family whose error slot is `Slot`: one record per family (mxv_gae_last_launch,
// mxv_vtrace_last_launch)
struct LastLaunch {
    int32_t envs_per_lane = 0;
    uint32_t grid = 0;
};
template <class Slot>
LastLaunch &last_launch() {
    thread_local LastLaunch l;
    return l;
}
template <class Slot>
void record_launch(bool vec, int64_t tiles) {
    last_launch<Slot>() = LastLaunch{vec ? 4 : 1, policy_host::grid_of(tiles).x};
}
template <class Slot>
int report_last_launch(const policy_host::Call<Slot> &call, int32_t *envs_per_lane, uint32_t *grid) {
    if (!envs_per_lane || !grid) return call.bad("%s_last_launch: output pointer is NULL", call.api);
    *envs_per_lane = last_launch<Slot>().envs_per_lane;
    *grid = last_launch<Slot>().grid;
    return MXV_OK;
}

}  // namespace trajectory
}  // namespace mxv
