// mxv_c51.hip — the categorical (C51) Q-learning loss of a batch: the target distribution (given, or the one-step bootstrap of DQN /
// double DQN projected onto the support), the cross-entropy of the taken action's distribution against it, its diagnostics and its dense
// gradient with respect to the logits; and the expected action values of a categorical head (include/mxv_c51.h).
//
// The results are defined bit for bit by the rule in the header: float64, one rounding per operation (this file is built with
// -ffp-contract=off like the rest of the library), EXP and LOG the sequences of mxv_policy_rule.hpp, every sum over the atoms the xor
// butterfly of one wave and every sum over the rows the fixed tree of mxv_sum_tree.hpp — nothing here depends on the order in which
// lanes or workgroups arrive.  The argument checks are those of mxv_policy_host.hpp.
//
// Shape of the kernels:
//   * one WAVE owns a row, lane k = atom k (Z <= 64; lanes k >= Z hold the +0.0 slots of ATOMSUM).  A row of logits is one coalesced
//     load of Z dwords, ATOMSUM is the butterfly (DPP / permlane: no LDS), the selecting pass a uniform loop over the A actions, and the
//     projection a uniform loop over j that reads b_j and pn_j from lane j (v_readlane) and accumulates into the lane's own m_k in
//     ascending j: no scatter, no LDS, nothing that arrives in an order.  The row index, the action, the terminated flag and j* are
//     wave-uniform: a terminated row skips the selecting pass by a uniform branch (the rule's select ignores what it would compute).
//   * c51_rows: one workgroup of 4 waves per tile of 4 rows (no tile loop: see grid_rows); a row leaves its six scalars (term, qa, y,
//     ent, cm, ce) in the workspace as six columns of M doubles, and row_loss / projected if asked.
//   * c51_leaf: one workgroup per leaf of 1024 rows sums the columns exactly as the DQN loss's leaves do; a batch of one leaf finishes
//     there (2 launches up to 1024 rows).  c51_tree: one workgroup per group of 1024 partials; the last level finishes.  So a forward is
//     3 launches up to 2^20 rows, 4 up to 2^30.
//   * c51_bwd: recomputes the row and writes its [A, Z] gradient: Z consecutive dwords per action, the actions consecutive.
//   * c51_q: one wave per (row, action); workgroups stride over tiles of 4 pairs.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/mxv_c51.h"
#include "mxv_policy_host.hpp"
#include "mxv_policy_rule.hpp"
#include "mxv_sum_tree.hpp"
#include "mxv_value_loss.hpp"

namespace {

using namespace mxv::rule;
using namespace mxv::policy_host;
using namespace mxv::sum_tree;
using namespace mxv::value_loss;

constexpr int kMaxAtoms = 64;
// the slots of mxv_value_loss.hpp's partials and finish: sums of term, qa, y, ent, cm; max ce, min qa, max qa; a row's columns are term,
// qa, y, ent, cm, ce
static_assert(MXV_C51_STATS == kV && MXV_C51_LOSS_TERM == 0 && MXV_C51_Q_TAKEN_MEAN == 1 && MXV_C51_TARGET_MEAN == 2 && MXV_C51_ENTROPY_MEAN == 3 &&
                  MXV_C51_CLIPPED_MASS_MEAN == 4 && MXV_C51_ROW_LOSS_MAX == 5 && MXV_C51_Q_TAKEN_MIN == 6 && MXV_C51_Q_TAKEN_MAX == 7,
              "mxv_c51.h's stats are the slots of mxv_value_loss.hpp");

struct C51Args {
    const float *logits, *target_probs, *reward, *next, *online, *weights;
    const void *actions;
    const uint8_t *terminated;
    const float *g;                  // backward: the incoming gradient of the loss, one float32
    double *cols;                    // forward: [6][M]
    float *row_loss, *projected;     // forward, optional
    float *grad;                     // backward: [M][A][Z], contiguous
    float *q_out;                    // c51_q: [M][A], contiguous
    double gamma, v_min, v_max, dz, z_top;      // dz = (v_max - v_min) / (Z - 1); z_top = (double)(Z - 1)
    int64_t M, ld, next_ld, online_ld, tiles;
    int32_t A, Z, i64;
};

__device__ __forceinline__ bool any_lane(bool c) { return __builtin_amdgcn_ballot_w64(c) != 0; }

// ---- SOFT of one row of Z logits: lane k holds atom k ----
struct Soft {
    double d, e, p, S;
    bool bad;
};

__device__ __forceinline__ Soft soft(const float *row, int k, int Z) {
    const bool in = k < Z;
    float xf = -__builtin_inff();
    if (in) xf = row[k];
    Soft s;
    s.bad = any_lane(in && bad_logit(xf)) || !any_lane(in && xf != -__builtin_inff());
    const double xs = s.bad ? (in ? 0.0 : -(double)__builtin_inff()) : (double)xf;      // a bad row computes on zeros and is replaced
    const double mx = wave_tree<Max>(xs) + 0.0;
    const double d = xs - mx;
    s.e = e_of(d);
    s.S = wave_tree<Add>(s.e);
    const double p = s.e / s.S;
    s.d = s.bad ? nan64() : d;
    s.p = s.bad ? nan64() : p;
    return s;
}

// ---- one row of the rule; every field but p, m and lp is the same in every lane ----
struct Row {
    double p, m, lp;      // lane k: the taken action's probability, the target mass and the log-probability of atom k
    double sm, qa, y, ent, cm, ce;
    int32_t col;          // the stored action, or -1 for anything outside 0..A-1
};

__device__ __forceinline__ Row row_of(const C51Args &p, int64_t i, int k) {
    const int Z = p.Z, A = p.A;
    const bool in = k < Z;
    const double kd = (double)k;
    const double z = p.v_min + kd * p.dz;
    Row w;
    const int64_t v = p.i64 ? static_cast<const int64_t *>(p.actions)[i] : (int64_t) static_cast<const int32_t *>(p.actions)[i];
    const bool ok = v >= 0 && v < (int64_t)A;
    w.col = ok ? (int32_t)v : -1;
    const Soft s = soft(p.logits + i * p.ld + (ok ? v : 0) * Z, k, Z);      // a bad action reads action 0 and is replaced
    const double L = log_rule(s.S);
    w.p = s.p;
    w.lp = s.d - L;
    const double qa = wave_tree<Add>(s.p * z);
    const double ent = L - wave_tree<Add>(s.e == 0.0 ? 0.0 : s.e * s.d) / s.S;
    double m = 0.0;
    if (p.target_probs) {      // uniform: the target mode
        if (in) m = (double)p.target_probs[i * Z + k];
        w.cm = 0.0;
    } else {
        const bool term = p.terminated[i] != 0;      // uniform: one row per wave
        double pn = k == 0 ? 1.0 : 0.0;
        if (!term) {      // a terminated row ignores both next tensors entirely
            const float *sel = p.online ? p.online + i * p.online_ld : p.next + i * p.next_ld;
            double best = 0.0;
            int jmax = 0;
            bool selbad = false;
            for (int a = 0; a < A; ++a) {
                const Soft sa = soft(sel + a * Z, k, Z);
                const double Q = wave_tree<Add>(sa.p * z);
                selbad |= sa.bad;
                const bool up = a == 0 || Q > best;      // strict >: the first maximum wins
                best = up ? Q : best;
                jmax = up ? a : jmax;
            }
            jmax = __builtin_amdgcn_readfirstlane(jmax);
            const Soft st = soft(p.next + i * p.next_ld + jmax * Z, k, Z);
            pn = selbad ? nan64() : st.p;
        }
        const double r = (double)p.reward[i];
        const double boot = r + p.gamma * z;
        const double tz = term ? r : boot;
        double c = tz < p.v_min ? p.v_min : tz;
        c = c > p.v_max ? p.v_max : c;      // a NaN stays
        double b = (c - p.v_min) / p.dz;
        b = b > p.z_top ? p.z_top : b;
        w.cm = wave_tree<Add>(in && (tz < p.v_min || tz > p.v_max) ? pn : 0.0);
        for (int j = 0; j < Z; ++j) {      // ascending j: the rule's order
            const double bj = lane_value(b, j), pj = lane_value(pn, j);
            double wk = 1.0 - __builtin_fabs(bj - kd);
            wk = wk < 0.0 ? 0.0 : wk;
            m = m + pj * wk;
        }
        m = in ? m : 0.0;
    }
    w.m = m;
    w.sm = wave_tree<Add>(m);
    w.y = wave_tree<Add>(m * z);
    const double ce = -wave_tree<Add>(m == 0.0 ? 0.0 : m * w.lp);
    w.qa = ok ? qa : nan64();
    w.ent = ok ? ent : nan64();
    w.ce = ok ? ce : nan64();
    return w;
}

// ---- forward: the rows ----
__global__ void __launch_bounds__(kThreads) c51_rows(const C51Args p) {
    const int wave = wave_of_block(), lane = threadIdx.x & 63;
    const bool has_w = p.weights != nullptr;      // uniform
    {
        const int64_t i = tile_of_block() * kWaves + wave;
        if (i >= p.M) return;      // a whole wave
        const Row w = row_of(p, i, lane);
        const double term = has_w ? (double)p.weights[i] * w.ce : w.ce;
        if (lane == 0) {
            double *c = p.cols + i;
            c[0] = term;
            c[p.M] = w.qa;
            c[2 * p.M] = w.y;
            c[3 * p.M] = w.ent;
            c[4 * p.M] = w.cm;
            c[5 * p.M] = w.ce;
            if (p.row_loss) p.row_loss[i] = to_f32(w.ce);
        }
        if (p.projected && lane < p.Z) p.projected[i * p.Z + lane] = to_f32(w.m);
    }
}

// ---- forward: the leaves and the tree (mxv_value_loss.hpp) ----
__global__ void __launch_bounds__(kThreads) c51_leaf(const LeafArgs a) {
    __shared__ double sm[kThreads / 64][kV];
    leaf_columns(sm, a);
}

__global__ void __launch_bounds__(kThreads) c51_tree(const TreeArgs t) {
    __shared__ double sm[kThreads / 64][kV];
    tree_level(sm, t);
}

// ---- backward ----
__global__ void __launch_bounds__(kThreads) c51_bwd(const C51Args p) {
    const float nan = __uint_as_float(0x7FC00000u);
    const int wave = wave_of_block(), lane = threadIdx.x & 63;
    const bool has_w = p.weights != nullptr;      // uniform
    const double gs = (double)p.g[0] / (double)p.M;
    {
        const int64_t i = tile_of_block() * kWaves + wave;
        if (i >= p.M) return;      // a whole wave
        const Row w = row_of(p, i, lane);
        const double dl = w.p * w.sm - w.m;
        const float val = to_f32(gs * (has_w ? (double)p.weights[i] * dl : dl));
        if (lane < p.Z) {
            float *out = p.grad + i * p.A * p.Z + lane;
            for (int a = 0; a < p.A; ++a) out[a * p.Z] = w.col < 0 ? nan : (a == w.col ? val : 0.0f);
        }
    }
}

// ---- the expected values of every (row, action) ----
__global__ void __launch_bounds__(kThreads) c51_q(const C51Args p) {
    const int wave = wave_of_block(), lane = threadIdx.x & 63;
    const int64_t pairs = p.M * p.A;
    const double z = p.v_min + (double)lane * p.dz;
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t n = tile * kWaves + wave;
        if (n >= pairs) continue;      // a whole wave
        const int64_t i = n / p.A, a = n - i * p.A;
        const Soft s = soft(p.logits + i * p.ld + a * p.Z, lane, p.Z);
        const double Q = wave_tree<Add>(s.p * z);      // NaN where the row is bad
        if (lane == 0) p.q_out[n] = to_f32(Q);
    }
}

// ---- host ----
using CCall = Call<mxv::C51Call>;

int check_support(const CCall &call, int32_t Z, double v_min, double v_max) {
    if (Z < 2 || Z > kMaxAtoms) return call.bad("%s: Z = %d must be in 2..%d", call.api, (int)Z, kMaxAtoms);
    if (!std::isfinite(v_min) || !std::isfinite(v_max)) return call.bad("%s: v_min = %g and v_max = %g must be finite", call.api, v_min, v_max);
    if (!(v_min < v_max)) return call.bad("%s: v_min = %g must be below v_max = %g", call.api, v_min, v_max);
    return MXV_OK;
}

int check_rows_ld(const CCall &call, const char *name, int64_t ld, int64_t M, int32_t A, int32_t Z) {
    if (ld < (int64_t)A * Z) return call.bad("%s: row stride %s = %lld must be at least A * Z = %d", call.api, name, (long long)ld, (int)(A * Z));
    return call.check_stride(ld, M);
}

void fill_support(C51Args &p, int32_t A, int32_t Z, double v_min, double v_max) {
    p.A = A; p.Z = Z; p.v_min = v_min; p.v_max = v_max;
    p.z_top = (double)(Z - 1);
    p.dz = (v_max - v_min) / p.z_top;
}

constexpr ArgNames kNames = {"logits", "target_probs", "next_logits", "next_logits_online"};

// what the forward and the backward check alike; fills the inputs of `p`
int check_loss(const CCall &call, int64_t M, int32_t A, int32_t Z, const float *logits, int64_t ld, const void *actions, int32_t action_bytes,
               const float *target_probs, const float *reward, const uint8_t *terminated, const float *next, int64_t next_ld, const float *online,
               int64_t online_ld, double gamma, double v_min, double v_max, const float *weights, C51Args &p) {
    if (int rc = check_batch(call, kNames, logits, actions, M, A)) return rc;
    if (int rc = check_support(call, Z, v_min, v_max)) return rc;
    const auto check_ld = [&](const char *name, int64_t stride) { return check_rows_ld(call, name, stride, M, A, Z); };
    if (int rc = check_ld("logits_ld", ld)) return rc;
    if (int rc = check_targets(call, kNames, action_bytes, target_probs, reward, terminated, next, next_ld, online, online_ld, nullptr, gamma, check_ld))
        return rc;
    p.logits = logits; p.actions = actions; p.target_probs = target_probs; p.reward = reward; p.terminated = terminated; p.next = next;
    p.online = online; p.weights = weights; p.gamma = gamma;
    p.M = M; p.ld = ld; p.next_ld = next_ld; p.online_ld = online_ld; p.tiles = (M + kWaves - 1) / kWaves;
    p.i64 = action_bytes == 8;
    fill_support(p, A, Z, v_min, v_max);
    return MXV_OK;
}

constexpr int kInputs = 9;
// the byte ranges of the inputs, in the order of the arguments; an absent one has lo == 0
void input_ranges(const C51Args &p, const float *g, Range *r) {
    const uint64_t mb = (uint64_t)p.M * 4, ab = p.i64 ? 8 : 4;
    const int32_t W = p.A * p.Z;
    r[0] = {"logits", (uintptr_t)p.logits, rows_bytes(p.M, p.ld, W), 4};
    r[1] = {"actions", (uintptr_t)p.actions, (uint64_t)p.M * ab, ab};
    r[2] = {"target_probs", (uintptr_t)p.target_probs, mb * (uint64_t)p.Z, 4};
    r[3] = {"reward", (uintptr_t)p.reward, mb, 4};
    r[4] = {"terminated", (uintptr_t)p.terminated, (uint64_t)p.M, 1};
    r[5] = {"next_logits", (uintptr_t)p.next, p.next ? rows_bytes(p.M, p.next_ld, W) : 0, 4};
    r[6] = {"next_logits_online", (uintptr_t)p.online, p.online ? rows_bytes(p.M, p.online_ld, W) : 0, 4};
    r[7] = {"weights", (uintptr_t)p.weights, mb, 4};
    r[8] = {"grad_loss", (uintptr_t)g, 4, 4};
}

}  // namespace

extern "C" {

int64_t mxv_c51_workspace_bytes(int64_t M) { return M < 1 || M > kMaxElems ? 0 : workspace_doubles(M) * (int64_t)sizeof(double); }

int mxv_c51_loss(void *stream, int64_t M, int32_t A, int32_t Z, const float *logits_dev, int64_t logits_ld, const void *actions_dev,
                 int32_t action_bytes, const float *target_probs_dev, const float *reward_dev, const uint8_t *terminated_dev,
                 const float *next_logits_dev, int64_t next_logits_ld, const float *next_logits_online_dev, int64_t next_logits_online_ld,
                 double gamma, double v_min, double v_max, const float *weights_dev, void *workspace_dev, int64_t workspace_bytes,
                 float *row_loss_dev, float *projected_dev, float *loss_out_dev, float *stats_out_dev) {
    const CCall call{"mxv_c51_loss", 'M'};
    C51Args p{};
    if (int rc = check_loss(call, M, A, Z, logits_dev, logits_ld, actions_dev, action_bytes, target_probs_dev, reward_dev, terminated_dev,
                            next_logits_dev, next_logits_ld, next_logits_online_dev, next_logits_online_ld, gamma, v_min, v_max, weights_dev, p))
        return rc;
    if (!loss_out_dev) return call.bad("%s: loss_out pointer is NULL", call.api);
    if (!stats_out_dev) return call.bad("%s: stats_out pointer is NULL", call.api);
    const int64_t need = mxv_c51_workspace_bytes(M);
    if (int rc = check_workspace(call, "mxv_c51_workspace_bytes", M, workspace_dev, workspace_bytes, need)) return rc;
    Range ins[kInputs];
    input_ranges(p, nullptr, ins);
    const Range outs[] = {{"workspace", (uintptr_t)workspace_dev, (uint64_t)need, 8},
                          {"row_loss", (uintptr_t)row_loss_dev, (uint64_t)M * 4, 4},
                          {"projected", (uintptr_t)projected_dev, (uint64_t)M * (uint64_t)Z * 4, 4},
                          {"loss_out", (uintptr_t)loss_out_dev, 4, 4},
                          {"stats_out", (uintptr_t)stats_out_dev, MXV_C51_STATS * 4, 4}};
    if (int rc = call.check_ranges(M, ins, kInputs, outs, 5)) return rc;
    p.cols = static_cast<double *>(workspace_dev);
    p.row_loss = row_loss_dev;
    p.projected = projected_dev;
    if (int rc = launch_rows(call, reinterpret_cast<const void *>(&c51_rows), p, stream)) return rc;
    return sum_columns(call, reinterpret_cast<const void *>(&c51_leaf), reinterpret_cast<const void *>(&c51_tree), p.cols, M, loss_out_dev,
                       stats_out_dev, stream);
}

int mxv_c51_loss_backward(void *stream, int64_t M, int32_t A, int32_t Z, const float *logits_dev, int64_t logits_ld, const void *actions_dev,
                          int32_t action_bytes, const float *target_probs_dev, const float *reward_dev, const uint8_t *terminated_dev,
                          const float *next_logits_dev, int64_t next_logits_ld, const float *next_logits_online_dev,
                          int64_t next_logits_online_ld, double gamma, double v_min, double v_max, const float *weights_dev,
                          const float *grad_loss_dev, float *grad_logits_dev) {
    const CCall call{"mxv_c51_loss_backward", 'M'};
    C51Args p{};
    if (int rc = check_loss(call, M, A, Z, logits_dev, logits_ld, actions_dev, action_bytes, target_probs_dev, reward_dev, terminated_dev,
                            next_logits_dev, next_logits_ld, next_logits_online_dev, next_logits_online_ld, gamma, v_min, v_max, weights_dev, p))
        return rc;
    if (!grad_loss_dev) return call.bad("%s: grad_loss pointer is NULL", call.api);
    if (!grad_logits_dev) return call.bad("%s: grad_logits pointer is NULL", call.api);
    Range ins[kInputs];
    input_ranges(p, grad_loss_dev, ins);
    const Range outs[] = {{"grad_logits", (uintptr_t)grad_logits_dev, (uint64_t)M * (uint64_t)(A * Z) * 4, 4}};
    if (int rc = call.check_ranges(M, ins, kInputs, outs, 1)) return rc;
    p.g = grad_loss_dev; p.grad = grad_logits_dev;
    return launch_rows(call, reinterpret_cast<const void *>(&c51_bwd), p, stream);
}

int mxv_c51_q_values(void *stream, int64_t M, int32_t A, int32_t Z, const float *logits_dev, int64_t logits_ld, double v_min, double v_max,
                     float *q_out_dev) {
    const CCall call{"mxv_c51_q_values", 'M'};
    if (!logits_dev) return call.bad("%s: logits pointer is NULL", call.api);
    if (!q_out_dev) return call.bad("%s: q_out pointer is NULL", call.api);
    if (int rc = check_counts(call, M, A)) return rc;
    if (int rc = check_support(call, Z, v_min, v_max)) return rc;
    if (int rc = check_rows_ld(call, "logits_ld", logits_ld, M, A, Z)) return rc;
    C51Args p{};
    fill_support(p, A, Z, v_min, v_max);
    p.logits = logits_dev; p.ld = logits_ld; p.M = M; p.q_out = q_out_dev;
    p.tiles = (M * A + kWaves - 1) / kWaves;
    const Range ins[] = {{"logits", (uintptr_t)logits_dev, rows_bytes(M, logits_ld, A * Z), 4}};
    const Range outs[] = {{"q_out", (uintptr_t)q_out_dev, (uint64_t)M * (uint64_t)A * 4, 4}};
    if (int rc = call.check_ranges(M, ins, 1, outs, 1)) return rc;
    return call.launch(reinterpret_cast<const void *>(&c51_q), p, stream);
}

const char *mxv_c51_last_error(void) { return mxv::last_error<mxv::C51Call>(nullptr); }

}  // extern "C"
