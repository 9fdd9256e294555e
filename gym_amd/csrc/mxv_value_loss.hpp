// mxv_value_loss.hpp — what the three value-based losses share around their own rows (include/mxv_dqn.h, mxv_c51.h, mxv_qr.h; DESIGN.md §17,
// §20, §23), written once: the eight partials of a leaf and their finish, the body of a tree level, the six columns that a row of
// mxv_c51.hip and mxv_qr.hip leaves in the workspace and the leaf that sums them, the row-per-wave launch shape of those two — and, on
// the host, the argument checks that mxv_dqn_loss, mxv_c51_loss and mxv_qr_loss (and their backwards) make alike.  A file keeps its own
// rows (row_of, soft, first_max, the backward stores), its __global__ kernels and their LDS, which it passes to the bodies here as
// mxv_sum_tree.hpp's helpers take it, and the checks of its own head.  Float64, one rounding per operation (every file that includes
// this is built with -ffp-contract=off).  The host helpers are templates over the caller's policy_host::Call.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "mxv_policy_rule.hpp"
#include "mxv_sum_tree.hpp"

namespace mxv {
namespace value_loss {

using namespace mxv::sum_tree;
using rule::kMaxActions;
using rule::kMaxElems;
using rule::kThreads;

constexpr int kWaves = kThreads / 64;    // rows per tile of the kernels in which a wave owns a row (c51, qr: rows, bwd and q)
constexpr int kV = 8;                    // partials of a leaf, in the slots of the headers' stats: sums in 0..4, a maximum in 5, a minimum in 6,
                                         // a maximum in 7 (each file ties its MXV_*_ macros to them by static_assert)
constexpr int kCols = 6;                 // columns a row of c51 / qr leaves in the workspace: the sums' terms of slots 0..4, then what slot 5 takes
constexpr int kGridX = 1 << 16;          // the rows and bwd kernels of c51 / qr: tiles along x of the grid; beyond, y counts slices of kGridX
constexpr int kGridY = 1 << 15;          // tiles, and z slices of kGridY of those (2^38 tiles of 2^40 rows fit)

struct LeafArgs {
    const double *cols;              // [6][M]
    double *partials;                // [leaves][8]
    int64_t M;
    int32_t last;                    // one leaf: finish here
    float *loss, *stats;
};

struct TreeArgs {
    const double *in;                // [count][8]
    double *out;                     // [groups][8]; unused by the last level
    int64_t count, M;
    int32_t last;
    float *loss, *stats;
};

// which of a leaf's partials is a minimum, which a maximum; the others are sums
struct Partials {
    static constexpr int V = kV;
    static constexpr bool is_min(int v) { return v == 6; }
    static constexpr bool is_max(int v) { return v == 5 || v == 7; }
};

// the loss and the diagnostics from the last group's four waves, by slot: loss_out and slot 0 the first sum / M, slots 1..4 a sum / M,
// slots 5..7 the extremum + 0.0 (a zero of either sign leaves as +0.0); for one lane
__device__ __forceinline__ void finish(const double (*sm)[kV], int64_t M, float *loss_out, float *stats) {
    const double Mf = (double)M;
    const double loss = four_waves<Add>(sm, 0) / Mf;
    loss_out[0] = to_f32(loss);
    stats[0] = to_f32(loss);
    stats[1] = to_f32(four_waves<Add>(sm, 1) / Mf);
    stats[2] = to_f32(four_waves<Add>(sm, 2) / Mf);
    stats[3] = to_f32(four_waves<Add>(sm, 3) / Mf);
    stats[4] = to_f32(four_waves<Add>(sm, 4) / Mf);
    stats[5] = to_f32(four_waves<Max>(sm, 5) + 0.0);
    stats[6] = to_f32(four_waves<Min>(sm, 6) + 0.0);
    stats[7] = to_f32(four_waves<Max>(sm, 7) + 0.0);
}

// one level of the tree, for a workgroup per group of kTreeFan partials; the last level (one group) finishes in its first lane
__device__ __forceinline__ void tree_level(double (*sm)[kV], const TreeArgs t) {
    fold_level<Partials>(sm, t.in, t.count);
    if (!t.last) {
        write_partials<Partials>(sm, t.out);
        return;
    }
    if (threadIdx.x == 0) finish(sm, t.M, t.loss, t.stats);
}

// a leaf of kLeafRows rows of the six columns, for a workgroup per leaf: column v is the term of sum v (v < 5), column 1 also what the
// minimum and the last maximum take, column 5 what the first maximum takes; a batch of one leaf finishes here.  The arguments by value,
// as the kernel has them: through a reference the compiler orders the two branches on `last` differently (the same instructions).
__device__ __forceinline__ void leaf_columns(double (*sm)[kV], const LeafArgs a) {
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kLeafRows;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, mx5 = Max::identity(), mn1 = Min::identity(), mx1 = Max::identity();
#pragma unroll
    for (int j = 0; j < kLeafRows / kThreads; ++j) {
        const int64_t i = row0 + j * kThreads + tid;
        if (i >= a.M) continue;
        const double *c = a.cols + i;
        const double c1 = c[a.M], c5 = c[5 * a.M];
        s0 = s0 + c[0];
        s1 = s1 + c1;
        s2 = s2 + c[2 * a.M];
        s3 = s3 + c[3 * a.M];
        s4 = s4 + c[4 * a.M];
        mx5 = c5 > mx5 ? c5 : mx5;      // a NaN compares false: skipped
        mn1 = c1 < mn1 ? c1 : mn1;
        mx1 = c1 > mx1 ? c1 : mx1;
    }
    // a batch of one leaf: the one tree level it would pass through adds +0.0 to every sum and nothing else
    const double zero = a.last ? 0.0 : -0.0;
    const double t[kV] = {wave_tree<Add>(s0) + zero, wave_tree<Add>(s1) + zero, wave_tree<Add>(s2) + zero, wave_tree<Add>(s3) + zero,
                          wave_tree<Add>(s4) + zero, wave_tree<Max>(mx5),       wave_tree<Min>(mn1),       wave_tree<Max>(mx1)};
    leave_wave_values(sm, t);
    if (!a.last) {
        write_partials<Partials>(sm, a.partials);
        return;
    }
    if (tid == 0) finish(sm, a.M, a.loss, a.stats);
}

__device__ __forceinline__ int wave_of_block() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
// the tile of a workgroup of a rows or bwd kernel (grid_rows below)
__device__ __forceinline__ int64_t tile_of_block() { return ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * kGridX + blockIdx.x; }

// ---- host: the launches ----
// doubles of workspace where a wave owns a row: the six columns of the rows, the leaves' partials, and every level of the tree that is not the last
inline int64_t workspace_doubles(int64_t M) { return kCols * M + workspace_slots(M) * kV; }

// One tile per workgroup, not workgroups striding over tiles: inside a tile loop the compiler keeps the 32 float64 constants of EXP and
// LOG (mxv_c51.hip) in scalar registers across the whole loop beside the kernel's arguments, and 10 to 16 of those spill (DESIGN.md
// §20).  The grid grows along y beyond kGridX tiles and along z beyond kGridX * kGridY.
inline dim3 grid_rows(int64_t tiles) {
    const int64_t slices = (tiles + kGridX - 1) / kGridX;
    return dim3((unsigned)(tiles < kGridX ? tiles : kGridX), (unsigned)(slices < kGridY ? slices : kGridY), (unsigned)((slices + kGridY - 1) / kGridY));
}

template <class Call, class Args>
int launch_rows(const Call &call, const void *kernel, Args &a, void *stream) {
    void *args[] = {&a};
    const hipError_t e = hipLaunchKernel(kernel, grid_rows(a.tiles), dim3(kThreads), args, 0, (hipStream_t)stream);
    return e == hipSuccess ? MXV_OK : call.hip_failed("kernel launch", e);
}

// the levels of the tree over the `leaves` partials at `partials`, the last of which writes the loss and the stats
template <class Call>
int finish_tree(const Call &call, const void *tree, double *partials, int64_t leaves, int64_t M, float *loss, float *stats, void *stream) {
    TreeArgs t{};
    t.M = M; t.loss = loss; t.stats = stats;
    return run_tree(call, tree, kV, t, partials, leaves, stream);
}

// the leaves over the six columns at `cols` (a batch of one leaf finishes there), then the levels of the tree
template <class Call>
int sum_columns(const Call &call, const void *leaf, const void *tree, double *cols, int64_t M, float *loss, float *stats, void *stream) {
    const int64_t leaves = leaves_of(M);
    LeafArgs l{};
    l.cols = cols; l.partials = cols + kCols * M; l.M = M; l.last = leaves == 1; l.loss = loss; l.stats = stats;
    if (int rc = call.launch_blocks(leaf, l, leaves, stream)) return rc;
    return l.last ? MXV_OK : finish_tree(call, tree, l.partials, leaves, M, loss, stats, stream);
}

// ---- host: the checks ----
// how a header calls its rows, its direct target, the next rows of its bootstrap mode and their online selector
struct ArgNames {
    const char *rows, *direct, *next, *online;
};

// the row and action counts; also of the *_q_values calls
template <class Call>
int check_counts(const Call &call, int64_t M, int32_t A) {
    if (M < 1) return call.bad("%s: M = %lld must be at least 1", call.api, (long long)M);
    if (M > kMaxElems) return call.bad("%s: M = %lld is beyond 2^40 rows", call.api, (long long)M);
    if (A < 1 || A > kMaxActions) return call.bad("%s: A = %d must be in 1..%d", call.api, (int)A, kMaxActions);
    return MXV_OK;
}

// what a loss and its backward check first: the two pointers every mode reads, then the counts.  The file's own head follows
// (check_support, N and kappa), then the stride of its rows.
template <class Call>
int check_batch(const Call &call, const ArgNames &n, const void *rows, const void *actions, int64_t M, int32_t A) {
    if (!rows) return call.bad("%s: %s pointer is NULL", call.api, n.rows);
    if (!actions) return call.bad("%s: actions pointer is NULL", call.api);
    return check_counts(call, M, A);
}

// ... and what they check behind the stride of the rows: action_bytes, exactly one target mode, the pointers and the strides of the
// bootstrap mode — check_ld(name, ld) is the file's own check of a row stride — and gamma.  discount: the per-row discount of the
// bootstrap mode, NULL where a header has none (or the call passes none).
template <class Call, class CheckLd>
int check_targets(const Call &call, const ArgNames &n, int32_t action_bytes, const void *direct, const void *reward, const void *terminated,
                  const void *next, int64_t next_ld, const void *online, int64_t online_ld, const void *discount, double gamma, CheckLd check_ld) {
    if (action_bytes != 4 && action_bytes != 8) return call.bad("%s: action_bytes = %d must be 4 (int32) or 8 (int64)", call.api, (int)action_bytes);
    const bool any_boot = reward || terminated || next;
    if (direct && any_boot)
        return call.bad("%s: %s is given together with reward, terminated or %s: exactly one target mode", call.api, n.direct, n.next);
    if (direct && online) return call.bad("%s: %s is given with %s: it belongs to the bootstrap mode", call.api, n.online, n.direct);
    if (direct && discount) return call.bad("%s: discount is given with %s: it belongs to the bootstrap mode", call.api, n.direct);
    if (!direct && !any_boot)
        return call.bad("%s: neither %s nor reward, terminated and %s are given: exactly one target mode", call.api, n.direct, n.next);
    if (!direct) {
        if (!reward) return call.bad("%s: reward pointer is NULL in the bootstrap mode", call.api);
        if (!terminated) return call.bad("%s: terminated pointer is NULL in the bootstrap mode", call.api);
        if (!next) return call.bad("%s: %s pointer is NULL in the bootstrap mode", call.api, n.next);
        if (int rc = check_ld((std::string(n.next) + "_ld").c_str(), next_ld)) return rc;
        if (online)
            if (int rc = check_ld((std::string(n.online) + "_ld").c_str(), online_ld)) return rc;
    }
    if (!std::isfinite(gamma)) return call.bad("%s: gamma = %g must be finite", call.api, gamma);
    return MXV_OK;
}

}  // namespace value_loss
}  // namespace mxv
