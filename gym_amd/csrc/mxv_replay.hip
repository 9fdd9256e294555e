// mxv_replay.hip — the uniform replay buffer on the device: the fused insert of a [K, N] rollout chunk into a caller-owned ring and the
// Philox-keyed uniform draw with its gather (include/mxv_replay.h).
//
// Pure data movement plus one Philox call per drawn row: integer arithmetic only, except the one conversion of a float64 reward.  The
// results are defined bit for bit by the rule in the header (tests/replay_host.py); which launch shape runs changes none of them.  The
// argument checks are those of mxv_policy_host.hpp.
//
// Shape of the kernels (no LDS, no barrier, no read-modify-write of memory; state_dev is an ordinary uniform load):
//   * narrow rows, W <= 8 — replay_insert_rows<WT>, replay_sample_rows<WT>: one lane per transition, workgroups of 256 striding over
//     tiles of 256 rows as the policy kernels do.  WT = 2, 3, 4, 6 are straight-line: a row is read into registers and written as one
//     access of W dwords (W = 4: 16 bytes, W = 2: 8, W = 6: 8 + 16, W = 3: dwords merged by the compiler), chosen by the host only
//     where every base and row stride keeps that alignment; WT = 0 is the loop over W for everything else.  Consecutive lanes write
//     consecutive slots (insert) or consecutive output rows (sample): a wave's stores are 64 W consecutive dwords, save where the ring
//     wraps.
//   * wide rows, W > 8 — replay_insert_wide<VEC>, replay_sample_wide<VEC>: a workgroup per (row, piece of 1024 dwords), blockIdx.x the
//     piece and blockIdx.y striding over the rows, so the row's index — the Philox draw, the slot — is uniform in the workgroup and a
//     batch of few rows still fills the machine.  VEC: lane t copies the 16 bytes at dword 4 t of the piece (W % 4 == 0, every base and
//     stride on 16 bytes); otherwise lanes copy dwords t, t + 256, t + 512, t + 768.  Either way every wave access is a dense burst
//     inside one row, and both rows of a transition are loaded before either is stored.  The first lane of piece 0 moves the row's
//     action, reward and flag.
//   * (c + r) mod C is one 64-bit remainder per lane — c mod C — and a conditional subtraction per row: r < R <= C.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/mxv_replay.h"
#include "mxv_policy_host.hpp"
#include "mxv_policy_rule.hpp"
#include "mxv_replay_rows.hpp"

namespace {

using namespace mxv::rule;
using namespace mxv::policy_host;
using namespace mxv::replay_rows;

constexpr uint32_t kStreamReplay = MXV_REPLAY_STREAM_TAG;   // 1-8: mxv_device.hpp (kStream*), mxv_tab.hip, mxv_bj.hip, mxv_policy.hip, mxv_gaussian.hip
constexpr int64_t kMaxCapacity = MXV_REPLAY_MAX_CAPACITY;
constexpr uint64_t kMaxCount = (uint64_t)1 << 63;

struct InsertArgs {
    const uint32_t *first_obs, *obs, *final_obs;
    const uint32_t *actions;         // dwords: an int64 action is two of them
    const void *reward;
    const uint8_t *terminated, *truncated;
    const uint64_t *state_dev;
    uint32_t *ring_obs, *ring_next, *ring_action, *ring_reward;
    uint8_t *ring_term;
    uint64_t count;
    int64_t C, N, R, first_ld, obs_ld, final_ld, tiles;
    int32_t W, a64, r64;
};

struct SampleArgs {
    const uint32_t *ring_obs, *ring_next, *ring_action, *ring_reward;
    const uint8_t *ring_term;
    const uint64_t *state_dev;
    int64_t *indices;
    uint32_t *obs_out, *next_out, *reward_out;
    void *action_out;
    uint8_t *term_out;
    uint64_t seed, count, step;
    int64_t C, B, tiles;
    int32_t W, a64;
};

// round to nearest even; every NaN leaves as the one pattern
__device__ __forceinline__ uint32_t f64_to_f32_bits(double x) {
    const float y = (float)x;
    return y != y ? 0x7FC00000u : __float_as_uint(y);
}

// ---- the rule's pieces ----
struct Source {   // where row r of a chunk comes from, and its flag
    const uint32_t *pre, *nxt;
    uint32_t term;
};
__device__ __forceinline__ Source source_of(const InsertArgs &p, int64_t r) {
    Source s;
    const bool term = p.terminated[r] != 0;
    const bool done = term || (p.truncated != nullptr && p.truncated[r] != 0);
    s.term = term ? 1u : 0u;
    s.pre = r < p.N ? p.first_obs + r * p.first_ld : p.obs + (r - p.N) * p.obs_ld;
    s.nxt = (done && p.final_obs != nullptr) ? p.final_obs + r * p.final_ld : p.obs + r * p.obs_ld;
    return s;
}
// c mod C: the slot of row 0
__device__ __forceinline__ uint64_t first_slot(const InsertArgs &p) {
    const uint64_t c = p.state_dev ? p.state_dev[0] : p.count;
    return c % (uint64_t)p.C;
}
// (c + r) mod C from c mod C: r < R <= C
__device__ __forceinline__ int64_t slot_of(uint64_t s0, int64_t r, int64_t C) {
    const uint64_t s = s0 + (uint64_t)r;
    return (int64_t)(s >= (uint64_t)C ? s - (uint64_t)C : s);
}
__device__ __forceinline__ void store_scalars(const InsertArgs &p, int64_t r, int64_t s, uint32_t term) {
    p.ring_action[s] = p.a64 ? p.actions[2 * r] : p.actions[r];      // the low dword
    p.ring_reward[s] = p.r64 ? f64_to_f32_bits(static_cast<const double *>(p.reward)[r]) : static_cast<const uint32_t *>(p.reward)[r];
    p.ring_term[s] = (uint8_t)term;
}

// n = min(c, C) and the sample step
__device__ __forceinline__ void live_rows(const SampleArgs &p, uint64_t &n, uint64_t &t) {
    const uint64_t c = p.state_dev ? p.state_dev[0] : p.count;
    t = p.state_dev ? p.state_dev[1] : p.step;
    n = c < (uint64_t)p.C ? c : (uint64_t)p.C;
}
// k of row j: 0 <= k < n
__device__ __forceinline__ int64_t draw(const SampleArgs &p, uint64_t t, uint64_t n, int64_t j) {
    const uint64_t g = (uint64_t)j >> 2;
    mxv::U4 ctr;
    ctr.x = (uint32_t)g;
    ctr.y = (uint32_t)(g >> 32);
    ctr.z = (uint32_t)t;
    ctr.w = ((uint32_t)(t >> 32) & 0x0fffffffu) | (kStreamReplay << 28);
    const mxv::U4 w4 = mxv::philox4x32_10(ctr, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
    const uint32_t lane = (uint32_t)j & 3u;
    const uint32_t w = lane == 0 ? w4.x : lane == 1 ? w4.y : lane == 2 ? w4.z : w4.w;
    return (int64_t)(((uint64_t)w * n) >> 32);      // n <= 2^31: the product is below 2^63
}
__device__ __forceinline__ void gather_scalars(const SampleArgs &p, int64_t j, int64_t k, bool live) {
    const uint32_t a = live ? p.ring_action[k] : 0u;
    p.indices[j] = live ? k : -1;
    if (p.a64) static_cast<int64_t *>(p.action_out)[j] = (int64_t)(int32_t)a;
    else static_cast<uint32_t *>(p.action_out)[j] = a;
    p.reward_out[j] = live ? p.ring_reward[k] : 0u;
    p.term_out[j] = live ? p.ring_term[k] : (uint8_t)0;
}

// ---- narrow rows: one lane per transition ----
template <int WT>
__global__ void __launch_bounds__(kThreads) replay_insert_rows(const InsertArgs p) {
    const int W = WT > 0 ? WT : p.W;
    const uint64_t s0 = first_slot(p);
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t r = tile * kThreads + threadIdx.x;
        if (r >= p.R) continue;
        const Source src = source_of(p, r);
        const int64_t s = slot_of(s0, r, p.C);
        copy_rows<WT>(p.ring_obs + s * W, src.pre, p.ring_next + s * W, src.nxt, W, true);
        store_scalars(p, r, s, src.term);
    }
}

template <int WT>
__global__ void __launch_bounds__(kThreads) replay_sample_rows(const SampleArgs p) {
    const int W = WT > 0 ? WT : p.W;
    uint64_t n, t;
    live_rows(p, n, t);
    const bool live = n != 0;      // uniform
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t j = tile * kThreads + threadIdx.x;
        if (j >= p.B) continue;
        const int64_t k = live ? draw(p, t, n, j) : 0;
        copy_rows<WT>(p.obs_out + j * W, p.ring_obs + k * W, p.next_out + j * W, p.ring_next + k * W, W, live);
        gather_scalars(p, j, k, live);
    }
}

// ---- wide rows: a workgroup per (row, piece) ----
template <bool VEC>
__global__ void __launch_bounds__(kThreads) replay_insert_wide(const InsertArgs p) {
    const int piece = blockIdx.x;
    const uint64_t s0 = first_slot(p);
    for (int64_t r = blockIdx.y; r < p.R; r += gridDim.y) {      // r is the workgroup's
        const Source src = source_of(p, r);
        const int64_t s = slot_of(s0, r, p.C);
        copy_pieces<VEC>(p.ring_obs + s * p.W, src.pre, p.ring_next + s * p.W, src.nxt, p.W, piece);
        if (piece == 0 && threadIdx.x == 0) store_scalars(p, r, s, src.term);
    }
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) replay_sample_wide(const SampleArgs p) {
    const int piece = blockIdx.x;
    uint64_t n, t;
    live_rows(p, n, t);
    const bool live = n != 0;      // uniform
    for (int64_t j = blockIdx.y; j < p.B; j += gridDim.y) {      // j, and so k, is the workgroup's
        const int64_t k = live ? draw(p, t, n, j) : 0;
        copy_pieces<VEC>(p.obs_out + j * p.W, live ? p.ring_obs + k * p.W : nullptr, p.next_out + j * p.W, live ? p.ring_next + k * p.W : nullptr,
                         p.W, piece);
        if (piece == 0 && threadIdx.x == 0) gather_scalars(p, j, k, live);
    }
}

// ---- host ----
using RCall = Call<mxv::ReplayCall>;

template <int WT> struct InsertRows { static const void *ptr() { return reinterpret_cast<const void *>(&replay_insert_rows<WT>); } };
template <int WT> struct SampleRows { static const void *ptr() { return reinterpret_cast<const void *>(&replay_sample_rows<WT>); } };
template <template <int> class K>
const void *pick(int32_t W, bool aligned) {
    if (!aligned) return K<0>::ptr();
    switch (W) {
        case 2: return K<2>::ptr();
        case 3: return K<3>::ptr();
        case 4: return K<4>::ptr();
        case 6: return K<6>::ptr();
        default: return K<0>::ptr();
    }
}

int check_ring(const RCall &call, int64_t C, int32_t W) {
    if (C < 1 || C > kMaxCapacity) return call.bad("%s: C = %lld must be in 1..2^31", call.api, (long long)C);
    if (W < 1 || W > MXV_REPLAY_MAX_WIDTH) return call.bad("%s: W = %d must be in 1..%d", call.api, (int)W, MXV_REPLAY_MAX_WIDTH);
    if (W > kMaxElems / C) return call.bad("%s: C * W = %lld * %d is beyond 2^40 dwords", call.api, (long long)C, (int)W);
    return MXV_OK;
}

int check_rows_ld(const RCall &call, const char *name, int64_t ld, int64_t rows, int32_t W) {
    if (ld < W) return call.bad("%s: row stride %s = %lld must be at least W = %d", call.api, name, (long long)ld, (int)W);
    return call.check_stride(ld, rows);
}

}  // namespace

extern "C" {

int mxv_replay_insert(void *stream, int64_t C, int32_t W, int64_t K, int64_t N, const void *first_obs_dev, int64_t first_obs_ld,
                      const void *obs_dev, int64_t obs_ld, const void *final_obs_dev, int64_t final_obs_ld, const void *actions_dev,
                      int32_t action_bytes, const void *reward_dev, int32_t reward_bytes, const uint8_t *terminated_dev,
                      const uint8_t *truncated_dev, uint64_t count, uint64_t *state_dev, void *ring_obs_dev, void *ring_next_dev,
                      void *ring_action_dev, float *ring_reward_dev, uint8_t *ring_term_dev) {
    const RCall call{"mxv_replay_insert", 'n'};
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
    if (int rc = check_ring(call, C, W)) return rc;
    if (K < 1) return call.bad("%s: K = %lld must be at least 1", call.api, (long long)K);
    if (N < 1) return call.bad("%s: N = %lld must be at least 1", call.api, (long long)N);
    if (K > C / N) return call.bad("%s: K * N = %lld * %lld rows exceed C = %lld: two rows of one launch would share a slot", call.api, (long long)K, (long long)N, (long long)C);
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
                          {"ring_term", (uintptr_t)ring_term_dev, (uint64_t)C, 1}};
    if (int rc = call.check_ranges(R, ins, 8, outs, 5)) return rc;
    InsertArgs p{};
    p.first_obs = static_cast<const uint32_t *>(first_obs_dev); p.obs = static_cast<const uint32_t *>(obs_dev);
    p.final_obs = static_cast<const uint32_t *>(final_obs_dev); p.actions = static_cast<const uint32_t *>(actions_dev); p.reward = reward_dev;
    p.terminated = terminated_dev; p.truncated = truncated_dev; p.state_dev = state_dev;
    p.ring_obs = static_cast<uint32_t *>(ring_obs_dev); p.ring_next = static_cast<uint32_t *>(ring_next_dev);
    p.ring_action = static_cast<uint32_t *>(ring_action_dev); p.ring_reward = reinterpret_cast<uint32_t *>(ring_reward_dev); p.ring_term = ring_term_dev;
    p.count = count; p.C = C; p.N = N; p.R = R; p.first_ld = first_obs_ld; p.obs_ld = obs_ld; p.final_ld = final_obs_dev ? final_obs_ld : 0;
    p.tiles = (R + kThreads - 1) / kThreads; p.W = W; p.a64 = action_bytes == 8; p.r64 = reward_bytes == 8;
    Aligned al{wanted_alignment(W)};
    al.base(first_obs_dev); al.base(obs_dev); al.base(final_obs_dev); al.base(ring_obs_dev); al.base(ring_next_dev);
    al.stride(first_obs_ld); al.stride(obs_ld); al.stride(p.final_ld); al.stride(W);
    if (W > kNarrow) {
        const void *kernel = al.ok && al.align == 16 ? reinterpret_cast<const void *>(&replay_insert_wide<true>) : reinterpret_cast<const void *>(&replay_insert_wide<false>);
        if (int rc = launch_wide(call, kernel, p, R, stream)) return rc;
    } else {
        if (int rc = call.launch(pick<InsertRows>(W, al.ok), p, stream)) return rc;
    }
    if (state_dev) {
        const hipError_t e = mxv::launch_add_word(&state_dev[0], (uint64_t)R, (hipStream_t)stream);
        if (e != hipSuccess) return call.hip_failed("row counter launch", e);
    }
    return MXV_OK;
}

int mxv_replay_sample(void *stream, int64_t C, int32_t W, int64_t B, const void *ring_obs_dev, const void *ring_next_dev,
                      const void *ring_action_dev, const float *ring_reward_dev, const uint8_t *ring_term_dev, uint64_t seed, uint64_t count,
                      uint64_t step, uint64_t *state_dev, int64_t *indices_dev, void *obs_out_dev, void *next_out_dev, void *action_out_dev,
                      int32_t action_bytes, float *reward_out_dev, uint8_t *term_out_dev) {
    const RCall call{"mxv_replay_sample", 'B'};
    if (!ring_obs_dev) return call.bad("%s: ring_obs pointer is NULL", call.api);
    if (!ring_next_dev) return call.bad("%s: ring_next pointer is NULL", call.api);
    if (!ring_action_dev) return call.bad("%s: ring_action pointer is NULL", call.api);
    if (!ring_reward_dev) return call.bad("%s: ring_reward pointer is NULL", call.api);
    if (!ring_term_dev) return call.bad("%s: ring_term pointer is NULL", call.api);
    if (!indices_dev) return call.bad("%s: indices pointer is NULL", call.api);
    if (!obs_out_dev) return call.bad("%s: obs_out pointer is NULL", call.api);
    if (!next_out_dev) return call.bad("%s: next_out pointer is NULL", call.api);
    if (!action_out_dev) return call.bad("%s: action_out pointer is NULL", call.api);
    if (!reward_out_dev) return call.bad("%s: reward_out pointer is NULL", call.api);
    if (!term_out_dev) return call.bad("%s: term_out pointer is NULL", call.api);
    if (int rc = check_ring(call, C, W)) return rc;
    if (B < 1) return call.bad("%s: B = %lld must be at least 1", call.api, (long long)B);
    if (B > kMaxElems / W) return call.bad("%s: B * W = %lld * %d is beyond 2^40 dwords", call.api, (long long)B, (int)W);
    if (action_bytes != 4 && action_bytes != 8) return call.bad("%s: action_bytes = %d must be 4 (int32, float32) or 8 (int64)", call.api, (int)action_bytes);
    if (count > kMaxCount) return call.bad("%s: count = %llu is above 2^63", call.api, (unsigned long long)count);
    const uint64_t ab = (uint64_t)action_bytes, ring_row_bytes = (uint64_t)C * (uint64_t)W * 4, out_row_bytes = (uint64_t)B * (uint64_t)W * 4;
    const Range ins[] = {{"ring_obs", (uintptr_t)ring_obs_dev, ring_row_bytes, 4}, {"ring_next", (uintptr_t)ring_next_dev, ring_row_bytes, 4},
                         {"ring_action", (uintptr_t)ring_action_dev, (uint64_t)C * 4, 4}, {"ring_reward", (uintptr_t)ring_reward_dev, (uint64_t)C * 4, 4},
                         {"ring_term", (uintptr_t)ring_term_dev, (uint64_t)C, 1}, {"state_dev", (uintptr_t)state_dev, 16, 8, ""}};
    const Range outs[] = {{"indices", (uintptr_t)indices_dev, (uint64_t)B * 8, 8}, {"obs_out", (uintptr_t)obs_out_dev, out_row_bytes, 4},
                          {"next_out", (uintptr_t)next_out_dev, out_row_bytes, 4}, {"action_out", (uintptr_t)action_out_dev, (uint64_t)B * ab, ab},
                          {"reward_out", (uintptr_t)reward_out_dev, (uint64_t)B * 4, 4}, {"term_out", (uintptr_t)term_out_dev, (uint64_t)B, 1}};
    if (int rc = call.check_ranges(B, ins, 6, outs, 6)) return rc;
    SampleArgs p{};
    p.ring_obs = static_cast<const uint32_t *>(ring_obs_dev); p.ring_next = static_cast<const uint32_t *>(ring_next_dev);
    p.ring_action = static_cast<const uint32_t *>(ring_action_dev); p.ring_reward = reinterpret_cast<const uint32_t *>(ring_reward_dev);
    p.ring_term = ring_term_dev; p.state_dev = state_dev; p.indices = indices_dev;
    p.obs_out = static_cast<uint32_t *>(obs_out_dev); p.next_out = static_cast<uint32_t *>(next_out_dev);
    p.reward_out = reinterpret_cast<uint32_t *>(reward_out_dev); p.action_out = action_out_dev; p.term_out = term_out_dev;
    p.seed = seed; p.count = count; p.step = step; p.C = C; p.B = B; p.tiles = (B + kThreads - 1) / kThreads; p.W = W; p.a64 = action_bytes == 8;
    Aligned al{wanted_alignment(W)};
    al.base(ring_obs_dev); al.base(ring_next_dev); al.base(obs_out_dev); al.base(next_out_dev); al.stride(W);
    if (W > kNarrow) {
        const void *kernel = al.ok && al.align == 16 ? reinterpret_cast<const void *>(&replay_sample_wide<true>) : reinterpret_cast<const void *>(&replay_sample_wide<false>);
        if (int rc = launch_wide(call, kernel, p, B, stream)) return rc;
    } else {
        if (int rc = call.launch(pick<SampleRows>(W, al.ok), p, stream)) return rc;
    }
    return call.advance(state_dev ? &state_dev[1] : nullptr, stream);
}

const char *mxv_replay_last_error(void) { return mxv::last_error<mxv::ReplayCall>(nullptr); }

}  // extern "C"
