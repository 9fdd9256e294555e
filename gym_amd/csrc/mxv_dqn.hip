// mxv_dqn.hip — the Q-learning loss of a batch: TD targets (given, or the one-step bootstrap of DQN / double DQN), the Huber loss of the
// TD errors, its diagnostics and its dense gradient with respect to q (include/mxv_dqn.h).
//
// The results are defined bit for bit by the rule in the header: float64, one rounding per operation (this file is built with
// -ffp-contract=off like the rest of the library), and every sum the fixed tree of mxv_sum_tree.hpp over the row index — nothing here depends
// on the order in which lanes or workgroups arrive.  The argument checks are those of mxv_policy_host.hpp.
//
// Shape of the kernels (about 12 fp64 operations for 25 + 4 A bytes a row forwards, 8 for 21 + 8 A backwards: bound by memory):
//   * dqn_leaf<AT>: one workgroup of 256 lanes per leaf of 1024 consecutive rows; lane t takes rows t, t + 256, t + 512, t + 768.  One
//     lane owns a row: q[i, a_i] is one dword (read at column 0 when the action is out of range, and then replaced), a row of the
//     selector is one access of A dwords for A = 2, 3, 4, 6 (the straight-line instantiations, as in mxv_policy_eval.hip) and a loop
//     that keeps nothing per column for every other A (AT = 0).  Then the xor butterfly of each wave (DPP / permlane: no LDS round
//     trips) and the four waves through LDS: 4 x 8 doubles.  A leaf writes its 8 partials to the workspace and, if asked, td_error.
//   * dqn_tree: one workgroup per group of 1024 partials; the last level (one group) also finishes the loss and the diagnostics in its
//     first lane.  So a forward is 2 launches up to 2^20 rows, 3 up to 2^30.
//   * dqn_bwd<AT>: recomputes the row and writes the dense [M, A] gradient.  A = 2, 3, 4, 6: a lane holds its row of the gradient in
//     registers and stores it as one access of A dwords — consecutive lanes, consecutive rows: a wave's stores are 64 A consecutive
//     dwords.  Every other A: a lane leaves its row's one value and its column in LDS (256 x 8 bytes), and the workgroup then writes the
//     tile's 256 A consecutive floats with lane t taking elements t, t + 256, ...: every wave store is a dense burst of 64 dwords,
//     whatever A is.
//   * everything in the rule is a select; which optional inputs there are is a uniform branch.
//   * the tree — butterfly, four waves, levels, workspace — is mxv_sum_tree.hpp's; here are the rows, the leaf's sums and the finish.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/mxv_dqn.h"
#include "mxv_policy_host.hpp"
#include "mxv_policy_rule.hpp"
#include "mxv_sum_tree.hpp"
#include "mxv_value_loss.hpp"

namespace {

using namespace mxv::rule;
using namespace mxv::policy_host;
using namespace mxv::sum_tree;
using namespace mxv::value_loss;

// the slots of mxv_value_loss.hpp's partials and finish: sums of term, ae, qa, y, lin; max ae, min qa, max qa
static_assert(MXV_DQN_STATS == kV && MXV_DQN_LOSS_TERM == 0 && MXV_DQN_TD_ABS_MEAN == 1 && MXV_DQN_Q_TAKEN_MEAN == 2 && MXV_DQN_TARGET_MEAN == 3 &&
                  MXV_DQN_LINEAR_FRACTION == 4 && MXV_DQN_TD_ABS_MAX == 5 && MXV_DQN_Q_TAKEN_MIN == 6 && MXV_DQN_Q_TAKEN_MAX == 7,
              "mxv_dqn.h's stats are the slots of mxv_value_loss.hpp");

struct DqnArgs {
    const float *q, *targets, *reward, *next_q, *online, *weights;
    const void *actions;
    const uint8_t *terminated;
    const float *g;                  // backward: the incoming gradient of the loss, one float32
    double *partials;                // forward: [leaves][8]
    float *td_error;                 // forward, optional
    float *grad;                     // backward: [M][A], contiguous
    double gamma, delta;
    int64_t M, q_ld, next_ld, online_ld, tiles;
    int32_t A, i64;
};

// ---- one row of the rule ----
struct Row {
    double qa, y, e, ae, h, dh;
    int32_t col;      // the stored action, or -1 for anything outside 0..A-1
};

// the first maximum of a selector row and whether the row holds a NaN
template <int AT>
__device__ __forceinline__ void first_max(const float *sel, int A, float &best, int &jmax, bool &bad) {
    if constexpr (AT > 0) {
        float x[AT];
#pragma unroll
        for (int k = 0; k < AT; ++k) x[k] = sel[k];      // merged into one access of AT dwords (two for AT = 6): 4-byte alignment suffices
        best = x[0];
        jmax = 0;
        bad = x[0] != x[0];
#pragma unroll
        for (int k = 1; k < AT; ++k) {
            bad |= x[k] != x[k];
            const bool up = x[k] > best;
            best = up ? x[k] : best;
            jmax = up ? k : jmax;
        }
    } else {
        best = sel[0];
        jmax = 0;
        bad = best != best;
        for (int k = 1; k < A; ++k) {
            const float x = sel[k];
            bad |= x != x;
            const bool up = x > best;
            best = up ? x : best;
            jmax = up ? k : jmax;
        }
    }
}

template <int AT>
__device__ __forceinline__ Row row_of(const DqnArgs &p, int64_t i) {
    const int A = AT > 0 ? AT : p.A;
    Row w;
    const int64_t v = p.i64 ? static_cast<const int64_t *>(p.actions)[i] : (int64_t) static_cast<const int32_t *>(p.actions)[i];
    const bool ok = v >= 0 && v < (int64_t)A;
    w.col = ok ? (int32_t)v : -1;
    const float qf = p.q[i * p.q_ld + (ok ? v : 0)];      // one dword; a bad action reads column 0 and is replaced
    w.qa = ok ? (double)qf : nan64();
    if (p.targets) {      // uniform: the target mode
        w.y = (double)p.targets[i];
    } else {
        const bool dbl = p.online != nullptr;      // uniform
        const float *sel = dbl ? p.online + i * p.online_ld : p.next_q + i * p.next_ld;
        float best;
        int jmax;
        bool bad;
        first_max<AT>(sel, A, best, jmax, bad);
        // one dword, also when next_q itself selects (the row was just read: a cache hit).  `dbl ? load : best` makes the compiler select
        // between the two ADDRESSES and park best in scratch for it.
        const float nq = p.next_q[i * p.next_ld + jmax];
        const double nv = bad ? nan64() : (double)nq;
        const double r = (double)p.reward[i];
        const double boot = r + p.gamma * nv;
        w.y = p.terminated[i] ? r : boot;
    }
    w.e = w.qa - w.y;
    w.ae = __builtin_fabs(w.e);
    const bool nan_e = w.e != w.e, quad = w.ae <= p.delta;
    const double h = quad ? 0.5 * (w.e * w.e) : p.delta * (w.ae - 0.5 * p.delta);
    const double dh = quad ? w.e : (w.e < 0.0 ? -p.delta : p.delta);
    w.h = nan_e ? nan64() : h;
    w.dh = nan_e ? nan64() : dh;
    return w;
}

// ---- forward: the leaves ----
template <int AT>
__global__ void __launch_bounds__(kThreads) dqn_leaf(const DqnArgs p) {
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kLeafRows;
    const bool has_w = p.weights != nullptr;      // uniform
    double s = 0.0, sa = 0.0, sq = 0.0, sy = 0.0, sl = 0.0, mx_ae = Max::identity(), mn_q = Min::identity(), mx_q = Max::identity();
#pragma unroll
    for (int j = 0; j < kLeafRows / kThreads; ++j) {
        const int64_t i = row0 + j * kThreads + tid;
        if (i >= p.M) continue;
        const Row w = row_of<AT>(p, i);
        const double term = has_w ? (double)p.weights[i] * w.h : w.h;
        s = s + term;
        sa = sa + w.ae;
        sq = sq + w.qa;
        sy = sy + w.y;
        sl = sl + (w.ae > p.delta ? 1.0 : 0.0);
        mx_ae = w.ae > mx_ae ? w.ae : mx_ae;      // a NaN compares false: skipped
        mn_q = w.qa < mn_q ? w.qa : mn_q;
        mx_q = w.qa > mx_q ? w.qa : mx_q;
        if (p.td_error) p.td_error[i] = to_f32(w.e);
    }
    __shared__ double sm[kThreads / 64][kV];
    const double t[kV] = {wave_tree<Add>(s), wave_tree<Add>(sa), wave_tree<Add>(sq), wave_tree<Add>(sy),
                          wave_tree<Add>(sl), wave_tree<Max>(mx_ae), wave_tree<Min>(mn_q), wave_tree<Max>(mx_q)};
    leave_wave_values(sm, t);
    write_partials<Partials>(sm, p.partials);
}

// ---- forward: one level of the tree; the last one finishes (mxv_value_loss.hpp) ----
__global__ void __launch_bounds__(kThreads) dqn_tree(const TreeArgs t) {
    __shared__ double sm[kThreads / 64][kV];
    tree_level(sm, t);
}

// ---- backward ----
// the one value of row i's gradient that is not a zero (its column: w.col; every column is NaN where w.col < 0)
__device__ __forceinline__ float taken_grad(const DqnArgs &p, const Row &w, int64_t i, double gs, bool has_w) {
    return to_f32(gs * (has_w ? (double)p.weights[i] * w.dh : w.dh));
}

template <int AT>
__global__ void __launch_bounds__(kThreads) dqn_bwd(const DqnArgs p) {
    const float nan = __uint_as_float(0x7FC00000u);
    const bool has_w = p.weights != nullptr;      // uniform
    const double gs = (double)p.g[0] / (double)p.M;
    if constexpr (AT > 0) {
        for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
            const int64_t i = tile * kThreads + threadIdx.x;
            if (i >= p.M) continue;
            const Row w = row_of<AT>(p, i);
            const float val = taken_grad(p, w, i, gs, has_w);
            float g[AT];
#pragma unroll
            for (int k = 0; k < AT; ++k) g[k] = w.col < 0 ? nan : (w.col == k ? val : 0.0f);
            float *out = p.grad + i * AT;
#pragma unroll
            for (int k = 0; k < AT; ++k) out[k] = g[k];      // one store of AT dwords (two for AT = 6)
        }
    } else {
        __shared__ float s_val[kThreads];
        __shared__ int32_t s_col[kThreads];
        const int tid = threadIdx.x, A = p.A;
        const float inv_A = 1.0f / (float)A;
        for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {      // the trip count is the workgroup's: the barriers are uniform
            const int64_t r0 = tile * kThreads, i = r0 + tid;
            if (i < p.M) {
                const Row w = row_of<0>(p, i);
                s_val[tid] = taken_grad(p, w, i, gs, has_w);
                s_col[tid] = w.col;
            }
            __syncthreads();
            const int64_t left = p.M - r0;
            const int n = (int)(left < kThreads ? left : kThreads) * A;      // the tile's elements: at most 256 x 64
            float *out = p.grad + r0 * A;
            for (int k = tid; k < n; k += kThreads) {
                // k / A: (k + 0.5) / A is at least 1 / 128 away from an integer and the two float roundings move it by less than 2^-9
                const int r = (int)(((float)k + 0.5f) * inv_A);
                const int c = k - r * A, col = s_col[r];
                out[k] = col < 0 ? nan : (c == col ? s_val[r] : 0.0f);
            }
            __syncthreads();
        }
    }
}

// ---- host ----
using DCall = Call<mxv::DqnCall>;

template <int AT> struct Leaf { static const void *ptr() { return reinterpret_cast<const void *>(&dqn_leaf<AT>); } };
template <int AT> struct Bwd { static const void *ptr() { return reinterpret_cast<const void *>(&dqn_bwd<AT>); } };
template <template <int> class K>
const void *pick(int32_t A) {
    switch (A) {
        case 2: return K<2>::ptr();
        case 3: return K<3>::ptr();
        case 4: return K<4>::ptr();
        case 6: return K<6>::ptr();
        default: return K<0>::ptr();
    }
}

int check_rows_ld(const DCall &call, const char *name, int64_t ld, int64_t M, int32_t A) {
    if (ld < A) return call.bad("%s: row stride %s = %lld must be at least A = %d", call.api, name, (long long)ld, (int)A);
    return call.check_stride(ld, M);
}

constexpr ArgNames kNames = {"q", "targets", "next_q", "next_q_online"};

// what the forward and the backward check alike; fills the inputs of `p`
int check_loss(const DCall &call, int64_t M, int32_t A, const float *q, int64_t q_ld, const void *actions, int32_t action_bytes,
               const float *targets, const float *reward, const uint8_t *terminated, const float *next_q, int64_t next_q_ld, const float *online,
               int64_t online_ld, double gamma, double delta, const float *weights, DqnArgs &p) {
    if (int rc = check_batch(call, kNames, q, actions, M, A)) return rc;
    const auto check_ld = [&](const char *name, int64_t stride) { return check_rows_ld(call, name, stride, M, A); };
    if (int rc = check_ld("q_ld", q_ld)) return rc;
    if (int rc = check_targets(call, kNames, action_bytes, targets, reward, terminated, next_q, next_q_ld, online, online_ld, nullptr, gamma, check_ld))
        return rc;
    if (!(delta > 0.0)) return call.bad("%s: delta = %g must be above 0 (+Inf: the half squared error)", call.api, delta);
    p.q = q; p.actions = actions; p.targets = targets; p.reward = reward; p.terminated = terminated; p.next_q = next_q; p.online = online;
    p.weights = weights; p.gamma = gamma; p.delta = delta;
    p.M = M; p.q_ld = q_ld; p.next_ld = next_q_ld; p.online_ld = online_ld; p.tiles = (M + kThreads - 1) / kThreads;
    p.A = A; p.i64 = action_bytes == 8;
    return MXV_OK;
}

constexpr int kInputs = 9;
// the byte ranges of the inputs, in the order of the arguments; an absent one has lo == 0
void input_ranges(const DqnArgs &p, const float *g, Range *r) {
    const uint64_t mb = (uint64_t)p.M * 4, ab = p.i64 ? 8 : 4;
    r[0] = {"q", (uintptr_t)p.q, rows_bytes(p.M, p.q_ld, p.A), 4};
    r[1] = {"actions", (uintptr_t)p.actions, (uint64_t)p.M * ab, ab};
    r[2] = {"targets", (uintptr_t)p.targets, mb, 4};
    r[3] = {"reward", (uintptr_t)p.reward, mb, 4};
    r[4] = {"terminated", (uintptr_t)p.terminated, (uint64_t)p.M, 1};
    r[5] = {"next_q", (uintptr_t)p.next_q, p.next_q ? rows_bytes(p.M, p.next_ld, p.A) : 0, 4};
    r[6] = {"next_q_online", (uintptr_t)p.online, p.online ? rows_bytes(p.M, p.online_ld, p.A) : 0, 4};
    r[7] = {"weights", (uintptr_t)p.weights, mb, 4};
    r[8] = {"grad_loss", (uintptr_t)g, 4, 4};
}

}  // namespace

extern "C" {

int64_t mxv_dqn_workspace_bytes(int64_t M) { return M < 1 || M > kMaxElems ? 0 : workspace_slots(M) * kV * (int64_t)sizeof(double); }

int mxv_dqn_loss(void *stream, int64_t M, int32_t A, const float *q_dev, int64_t q_ld, const void *actions_dev, int32_t action_bytes,
                 const float *targets_dev, const float *reward_dev, const uint8_t *terminated_dev, const float *next_q_dev, int64_t next_q_ld,
                 const float *next_q_online_dev, int64_t next_q_online_ld, double gamma, double delta, const float *weights_dev,
                 void *workspace_dev, int64_t workspace_bytes, float *td_error_dev, float *loss_out_dev, float *stats_out_dev) {
    const DCall call{"mxv_dqn_loss", 'M'};
    DqnArgs p{};
    if (int rc = check_loss(call, M, A, q_dev, q_ld, actions_dev, action_bytes, targets_dev, reward_dev, terminated_dev, next_q_dev, next_q_ld,
                            next_q_online_dev, next_q_online_ld, gamma, delta, weights_dev, p))
        return rc;
    if (!loss_out_dev) return call.bad("%s: loss_out pointer is NULL", call.api);
    if (!stats_out_dev) return call.bad("%s: stats_out pointer is NULL", call.api);
    const int64_t need = mxv_dqn_workspace_bytes(M);
    if (int rc = check_workspace(call, "mxv_dqn_workspace_bytes", M, workspace_dev, workspace_bytes, need)) return rc;
    Range ins[kInputs];
    input_ranges(p, nullptr, ins);
    const Range outs[] = {{"workspace", (uintptr_t)workspace_dev, (uint64_t)need, 8}, {"td_error", (uintptr_t)td_error_dev, (uint64_t)M * 4, 4},
                          {"loss_out", (uintptr_t)loss_out_dev, 4, 4}, {"stats_out", (uintptr_t)stats_out_dev, MXV_DQN_STATS * 4, 4}};
    if (int rc = call.check_ranges(M, ins, kInputs, outs, 4)) return rc;
    const int64_t leaves = leaves_of(M);
    p.partials = static_cast<double *>(workspace_dev);
    p.td_error = td_error_dev;
    if (int rc = call.launch_blocks(pick<Leaf>(A), p, leaves, stream)) return rc;
    return finish_tree(call, reinterpret_cast<const void *>(&dqn_tree), p.partials, leaves, M, loss_out_dev, stats_out_dev, stream);
}

int mxv_dqn_loss_backward(void *stream, int64_t M, int32_t A, const float *q_dev, int64_t q_ld, const void *actions_dev, int32_t action_bytes,
                          const float *targets_dev, const float *reward_dev, const uint8_t *terminated_dev, const float *next_q_dev,
                          int64_t next_q_ld, const float *next_q_online_dev, int64_t next_q_online_ld, double gamma, double delta,
                          const float *weights_dev, const float *grad_loss_dev, float *grad_q_dev) {
    const DCall call{"mxv_dqn_loss_backward", 'M'};
    DqnArgs p{};
    if (int rc = check_loss(call, M, A, q_dev, q_ld, actions_dev, action_bytes, targets_dev, reward_dev, terminated_dev, next_q_dev, next_q_ld,
                            next_q_online_dev, next_q_online_ld, gamma, delta, weights_dev, p))
        return rc;
    if (!grad_loss_dev) return call.bad("%s: grad_loss pointer is NULL", call.api);
    if (!grad_q_dev) return call.bad("%s: grad_q pointer is NULL", call.api);
    Range ins[kInputs];
    input_ranges(p, grad_loss_dev, ins);
    const Range outs[] = {{"grad_q", (uintptr_t)grad_q_dev, (uint64_t)M * (uint64_t)A * 4, 4}};
    if (int rc = call.check_ranges(M, ins, kInputs, outs, 1)) return rc;
    p.g = grad_loss_dev; p.grad = grad_q_dev;
    return call.launch(pick<Bwd>(A), p, stream);
}

const char *mxv_dqn_last_error(void) { return mxv::last_error<mxv::DqnCall>(nullptr); }

}  // extern "C"
