// mxv_nstep.hip — n-step returns for the replay ring: the fused insert of a [K, N] rollout chunk that walks each row's window of up to n
// steps inside the kernel, and the gather of the per-row discount for a drawn batch (include/mxv_nstep.h).
//
// The observation rows, the action and the slot are moved exactly as mxv_replay.hip moves them, with the row copiers of
// mxv_replay_rows.hpp; what is new is the walk: float64 accumulation of the discounted return, one rounding per operation, cut by a
// branch at the first step that ended.  The results are defined bit for bit by the rule in the header (tests/nstep_host.py); which
// launch shape runs changes none of them.  The argument checks are those of mxv_policy_host.hpp.
//
// Shape of the kernels (no LDS, no barrier, no read-modify-write of memory; state_dev is an ordinary uniform load):
//   * narrow rows, W <= 8 — nstep_insert_rows<WT>: one lane per transition, workgroups of 256 striding over tiles of 256 rows.  The lane
//     walks its own window: lane i reads reward / terminated / truncated at (t + j) * N + i, so at every step of the walk a wave reads 64
//     consecutive elements, and the rows t-1 .. t-n+1 read the same lines again from the cache.  WT = 2, 3, 4, 6 are straight-line
//     copies of W dwords, chosen by the host only where every base and row stride keeps that alignment; WT = 0 is the loop over W.
//   * wide rows, W > 8 — nstep_insert_wide<VEC>: a workgroup per (row, piece of 1024 dwords), blockIdx.x the piece and blockIdx.y striding
//     over the rows.  Every lane walks the row's window from uniform addresses, so its end e — and with it the source row — is uniform
//     in the workgroup.  Both rows of a transition are loaded before either is stored.  The first lane of piece 0 stores the row's action,
//     return, flag and discount.
//   * nstep_gather_rows: one lane per drawn row, the same tile striding.
//   * no lane divides: the walk steps the row index by N, and e + 1 < K is r + (e - t + 1) N < R.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/mxv_nstep.h"
#include "../../include/mxv_replay.h"
#include "mxv_policy_host.hpp"
#include "mxv_policy_rule.hpp"
#include "mxv_replay_rows.hpp"

namespace {

using namespace mxv::rule;
using namespace mxv::policy_host;
using namespace mxv::replay_rows;

constexpr int64_t kMaxCapacity = MXV_REPLAY_MAX_CAPACITY;
constexpr uint64_t kMaxCount = (uint64_t)1 << 63;
constexpr uint32_t kNaN = 0x7FC00000u;

struct NStepArgs {
    const uint32_t *first_obs, *obs, *final_obs;
    const uint32_t *actions;         // dwords: an int64 action is two of them
    const void *reward;
    const uint8_t *terminated, *truncated;
    const uint64_t *state_dev;
    uint32_t *ring_obs, *ring_next, *ring_action, *ring_reward, *ring_discount;
    uint8_t *ring_term;
    double gamma;
    uint64_t count;
    int64_t first_ld, obs_ld, final_ld;
    uint32_t C, N, R, tiles;      // C, R <= 2^31: rows, slots and tiles are 32-bit; only a row's address is 64-bit
    int32_t W, a64, r64, n;
};

struct GatherArgs {
    const uint32_t *ring_discount;
    const int64_t *indices;
    uint32_t *out;
    int64_t C, B, tiles;
};

// round to nearest even; every NaN leaves as the one pattern
__device__ __forceinline__ uint32_t f64_to_f32_bits(double x) {
    const float y = (float)x;
    return y != y ? kNaN : __float_as_uint(y);
}

// ---- the rule's pieces ----
__device__ __forceinline__ double reward_of(const NStepArgs &p, uint32_t r) {
    return p.r64 ? static_cast<const double *>(p.reward)[r] : (double)static_cast<const float *>(p.reward)[r];
}
__device__ __forceinline__ bool done_of(const NStepArgs &p, uint32_t r) {
    return p.terminated[r] != 0 || (p.truncated != nullptr && p.truncated[r] != 0);
}

struct Window {   // row r's window: where its two observation rows come from and its four scalars
    const uint32_t *pre, *nxt;
    uint32_t reward, discount, term;
};
__device__ __forceinline__ Window walk(const NStepArgs &p, uint32_t r) {
    uint32_t re = r;                                       // re = e * N + i: e + 1 < K is re + N < R <= 2^31
    int32_t steps = 1;                                     // e - t + 1
    double G = reward_of(p, r), g = 1.0;
    bool done = done_of(p, r);
    while (steps < p.n && re + p.N < p.R && !done) {       // cut by the branch: nothing behind a step that ended is read
        steps += 1;
        re += p.N;
        g = g * p.gamma;
        G = G + g * reward_of(p, re);
        done = done_of(p, re);
    }
    Window w;
    w.pre = r < p.N ? p.first_obs + (int64_t)r * p.first_ld : p.obs + (int64_t)(r - p.N) * p.obs_ld;
    w.nxt = (done && p.final_obs != nullptr) ? p.final_obs + (int64_t)re * p.final_ld : p.obs + (int64_t)re * p.obs_ld;
    w.reward = f64_to_f32_bits(G);
    w.discount = f64_to_f32_bits(g * p.gamma);
    w.term = p.terminated[re] != 0 ? 1u : 0u;
    return w;
}
// c mod C: the slot of row 0
__device__ __forceinline__ uint32_t first_slot(const NStepArgs &p) {
    const uint64_t c = p.state_dev ? p.state_dev[0] : p.count;
    return (uint32_t)(c % (uint64_t)p.C);
}
// (c + r) mod C from c mod C: r < R <= C <= 2^31, so the sum is below 2^32
__device__ __forceinline__ uint32_t slot_of(uint32_t s0, uint32_t r, uint32_t C) {
    const uint32_t s = s0 + r;
    return s >= C ? s - C : s;
}
__device__ __forceinline__ void store_scalars(const NStepArgs &p, uint32_t r, uint32_t s, const Window &w) {
    p.ring_action[s] = p.a64 ? p.actions[2 * (uint64_t)r] : p.actions[r];      // the low dword
    p.ring_reward[s] = w.reward;
    p.ring_term[s] = (uint8_t)w.term;
    p.ring_discount[s] = w.discount;
}

// ---- narrow rows: one lane per transition ----
template <int WT>
__global__ void __launch_bounds__(kThreads) nstep_insert_rows(const NStepArgs p) {
    const int W = WT > 0 ? WT : p.W;
    const uint32_t s0 = first_slot(p);
    for (uint32_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const uint32_t r = tile * kThreads + threadIdx.x;      // tiles <= 2^23
        if (r >= p.R) continue;
        const Window w = walk(p, r);
        const int64_t s = slot_of(s0, r, p.C);
        copy_rows<WT>(p.ring_obs + s * W, w.pre, p.ring_next + s * W, w.nxt, W, true);
        store_scalars(p, r, (uint32_t)s, w);
    }
}

// ---- wide rows: a workgroup per (row, piece) ----
template <bool VEC>
__global__ void __launch_bounds__(kThreads) nstep_insert_wide(const NStepArgs p) {
    const int piece = blockIdx.x;
    const uint32_t s0 = first_slot(p);
    for (uint32_t r = blockIdx.y; r < p.R; r += gridDim.y) {     // r, and so the window's end, is the workgroup's
        const Window w = walk(p, r);
        const int64_t s = slot_of(s0, r, p.C);
        copy_pieces<VEC>(p.ring_obs + s * p.W, w.pre, p.ring_next + s * p.W, w.nxt, p.W, piece);
        if (piece == 0 && threadIdx.x == 0) store_scalars(p, r, (uint32_t)s, w);
    }
}

// ---- the gather: one lane per drawn row ----
__global__ void __launch_bounds__(kThreads) nstep_gather_rows(const GatherArgs p) {
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t j = tile * kThreads + threadIdx.x;
        if (j >= p.B) continue;
        const int64_t k = p.indices[j];
        uint32_t d = k == -1 ? 0u : kNaN;
        if (k >= 0 && k < p.C) d = p.ring_discount[k];
        p.out[j] = d;
    }
}

// ---- host ----
using NCall = Call<mxv::NStepCall>;

template <int WT> const void *insert_rows() { return reinterpret_cast<const void *>(&nstep_insert_rows<WT>); }
const void *pick(int32_t W, bool aligned) {
    if (!aligned) return insert_rows<0>();
    switch (W) {
        case 2: return insert_rows<2>();
        case 3: return insert_rows<3>();
        case 4: return insert_rows<4>();
        case 6: return insert_rows<6>();
        default: return insert_rows<0>();
    }
}

int check_rows_ld(const NCall &call, const char *name, int64_t ld, int64_t rows, int32_t W) {
    if (ld < W) return call.bad("%s: row stride %s = %lld must be at least W = %d", call.api, name, (long long)ld, (int)W);
    return call.check_stride(ld, rows);
}

}  // namespace

extern "C" {

int mxv_nstep_insert(void *stream, int64_t C, int32_t W, int64_t K, int64_t N, const void *first_obs_dev, int64_t first_obs_ld,
                     const void *obs_dev, int64_t obs_ld, const void *final_obs_dev, int64_t final_obs_ld, const void *actions_dev,
                     int32_t action_bytes, const void *reward_dev, int32_t reward_bytes, const uint8_t *terminated_dev,
                     const uint8_t *truncated_dev, uint64_t count, uint64_t *state_dev, void *ring_obs_dev, void *ring_next_dev,
                     void *ring_action_dev, float *ring_reward_dev, uint8_t *ring_term_dev, int32_t n, double gamma,
                     float *ring_discount_dev) {
    const NCall call{"mxv_nstep_insert", 'n'};
    if (!first_obs_dev) return call.bad("%s: first_obs pointer is NULL", call.api);
    if (!obs_dev) return call.bad("%s: obs pointer is NULL", call.api);
    if (!actions_dev) return call.bad("%s: actions pointer is NULL", call.api);
    if (!reward_dev) return call.bad("%s: reward pointer is NULL", call.api);
    if (!terminated_dev) return call.bad("%s: terminated pointer is NULL", call.api);
    if (!ring_obs_dev) return call.bad("%s: ring_obs pointer is NULL", call.api);
    if (!ring_next_dev) return call.bad("%s: ring_next pointer is NULL", call.api);
    if (!ring_action_dev) return call.bad("%s: ring_action pointer is NULL", call.api);
    if (!ring_reward_dev) return call.bad("%s: ring_reward pointer is NULL", call.api);
    if (!ring_term_dev) return call.bad("%s: ring_term pointer is NULL", call.api);
    if (!ring_discount_dev) return call.bad("%s: ring_discount pointer is NULL", call.api);
    if (C < 1 || C > kMaxCapacity) return call.bad("%s: C = %lld must be in 1..2^31", call.api, (long long)C);
    if (W < 1 || W > MXV_REPLAY_MAX_WIDTH) return call.bad("%s: W = %d must be in 1..%d", call.api, (int)W, MXV_REPLAY_MAX_WIDTH);
    if (W > kMaxElems / C) return call.bad("%s: C * W = %lld * %d is beyond 2^40 dwords", call.api, (long long)C, (int)W);
    if (K < 1) return call.bad("%s: K = %lld must be at least 1", call.api, (long long)K);
    if (N < 1) return call.bad("%s: N = %lld must be at least 1", call.api, (long long)N);
    if (K > C / N) return call.bad("%s: K * N = %lld * %lld rows exceed C = %lld: two rows of one launch would share a slot", call.api, (long long)K, (long long)N, (long long)C);
    if (n < 1 || n > MXV_NSTEP_MAX) return call.bad("%s: n = %d must be in 1..%d", call.api, (int)n, MXV_NSTEP_MAX);
    if (!(gamma >= 0.0 && gamma <= 1.0)) return call.bad("%s: gamma = %g must be in [0, 1]", call.api, gamma);
    const int64_t R = K * N;
    if (int rc = check_rows_ld(call, "first_obs_ld", first_obs_ld, N, W)) return rc;
    if (int rc = check_rows_ld(call, "obs_ld", obs_ld, R, W)) return rc;
    if (final_obs_dev)
        if (int rc = check_rows_ld(call, "final_obs_ld", final_obs_ld, R, W)) return rc;
    if (action_bytes != 4 && action_bytes != 8) return call.bad("%s: action_bytes = %d must be 4 (int32, float32) or 8 (int64)", call.api, (int)action_bytes);
    if (reward_bytes != 4 && reward_bytes != 8) return call.bad("%s: reward_bytes = %d must be 4 (float32) or 8 (float64)", call.api, (int)reward_bytes);
    if (truncated_dev && !final_obs_dev)
        return call.bad("%s: truncated is given without final_obs: a truncated step would store the observation after the reset", call.api);
    if (count > kMaxCount) return call.bad("%s: count = %llu is above 2^63", call.api, (unsigned long long)count);
    const uint64_t ab = (uint64_t)action_bytes, rb = (uint64_t)reward_bytes, ring_row_bytes = (uint64_t)C * (uint64_t)W * 4;
    const Range ins[] = {{"first_obs", (uintptr_t)first_obs_dev, rows_bytes(N, first_obs_ld, W), 4},
                         {"obs", (uintptr_t)obs_dev, rows_bytes(R, obs_ld, W), 4},
                         {"final_obs", (uintptr_t)final_obs_dev, final_obs_dev ? rows_bytes(R, final_obs_ld, W) : 0, 4},
                         {"actions", (uintptr_t)actions_dev, (uint64_t)R * ab, ab},
                         {"reward", (uintptr_t)reward_dev, (uint64_t)R * rb, rb},
                         {"terminated", (uintptr_t)terminated_dev, (uint64_t)R, 1},
                         {"truncated", (uintptr_t)truncated_dev, (uint64_t)R, 1},
                         {"state_dev", (uintptr_t)state_dev, 16, 8, ""}};
    const Range outs[] = {{"ring_obs", (uintptr_t)ring_obs_dev, ring_row_bytes, 4}, {"ring_next", (uintptr_t)ring_next_dev, ring_row_bytes, 4},
                          {"ring_action", (uintptr_t)ring_action_dev, (uint64_t)C * 4, 4}, {"ring_reward", (uintptr_t)ring_reward_dev, (uint64_t)C * 4, 4},
                          {"ring_term", (uintptr_t)ring_term_dev, (uint64_t)C, 1}, {"ring_discount", (uintptr_t)ring_discount_dev, (uint64_t)C * 4, 4}};
    if (int rc = call.check_ranges(R, ins, 8, outs, 6)) return rc;
    NStepArgs p{};
    p.first_obs = static_cast<const uint32_t *>(first_obs_dev); p.obs = static_cast<const uint32_t *>(obs_dev);
    p.final_obs = static_cast<const uint32_t *>(final_obs_dev); p.actions = static_cast<const uint32_t *>(actions_dev); p.reward = reward_dev;
    p.terminated = terminated_dev; p.truncated = truncated_dev; p.state_dev = state_dev;
    p.ring_obs = static_cast<uint32_t *>(ring_obs_dev); p.ring_next = static_cast<uint32_t *>(ring_next_dev);
    p.ring_action = static_cast<uint32_t *>(ring_action_dev); p.ring_reward = reinterpret_cast<uint32_t *>(ring_reward_dev);
    p.ring_discount = reinterpret_cast<uint32_t *>(ring_discount_dev); p.ring_term = ring_term_dev;
    p.gamma = gamma; p.count = count; p.C = (uint32_t)C; p.N = (uint32_t)N; p.R = (uint32_t)R; p.first_ld = first_obs_ld; p.obs_ld = obs_ld;
    p.final_ld = final_obs_dev ? final_obs_ld : 0;
    p.tiles = (uint32_t)((R + kThreads - 1) / kThreads); p.W = W; p.a64 = action_bytes == 8; p.r64 = reward_bytes == 8; p.n = n;
    Aligned al{wanted_alignment(W)};
    al.base(first_obs_dev); al.base(obs_dev); al.base(final_obs_dev); al.base(ring_obs_dev); al.base(ring_next_dev);
    al.stride(first_obs_ld); al.stride(obs_ld); al.stride(p.final_ld); al.stride(W);
    if (W > kNarrow) {
        const void *kernel = al.ok && al.align == 16 ? reinterpret_cast<const void *>(&nstep_insert_wide<true>) : reinterpret_cast<const void *>(&nstep_insert_wide<false>);
        if (int rc = launch_wide(call, kernel, p, R, stream)) return rc;
    } else {
        if (int rc = call.launch(pick(W, al.ok), p, stream)) return rc;
    }
    if (state_dev) {
        const hipError_t e = mxv::launch_add_word(&state_dev[0], (uint64_t)R, (hipStream_t)stream);
        if (e != hipSuccess) return call.hip_failed("row counter launch", e);
    }
    return MXV_OK;
}

int mxv_nstep_gather(void *stream, int64_t C, int64_t B, const float *ring_discount_dev, const int64_t *indices_dev,
                     float *discount_out_dev) {
    const NCall call{"mxv_nstep_gather", 'B'};
    if (!ring_discount_dev) return call.bad("%s: ring_discount pointer is NULL", call.api);
    if (!indices_dev) return call.bad("%s: indices pointer is NULL", call.api);
    if (!discount_out_dev) return call.bad("%s: discount_out pointer is NULL", call.api);
    if (C < 1 || C > kMaxCapacity) return call.bad("%s: C = %lld must be in 1..2^31", call.api, (long long)C);
    if (B < 1) return call.bad("%s: B = %lld must be at least 1", call.api, (long long)B);
    if (int rc = call.check_stride(1, B)) return rc;
    const Range ins[] = {{"ring_discount", (uintptr_t)ring_discount_dev, (uint64_t)C * 4, 4}, {"indices", (uintptr_t)indices_dev, (uint64_t)B * 8, 8}};
    const Range outs[] = {{"discount_out", (uintptr_t)discount_out_dev, (uint64_t)B * 4, 4}};
    if (int rc = call.check_ranges(B, ins, 2, outs, 1)) return rc;
    GatherArgs p{};
    p.ring_discount = reinterpret_cast<const uint32_t *>(ring_discount_dev); p.indices = indices_dev;
    p.out = reinterpret_cast<uint32_t *>(discount_out_dev); p.C = C; p.B = B; p.tiles = (B + kThreads - 1) / kThreads;
    return call.launch(reinterpret_cast<const void *>(&nstep_gather_rows), p, stream);
}

const char *mxv_nstep_last_error(void) { return mxv::last_error<mxv::NStepCall>(nullptr); }

}  // extern "C"
