// mxv_qr.hip — the quantile-regression (QR-DQN) Q-learning loss of a batch: the target quantiles (given, or the bootstrap of DQN / double
// DQN with a scalar gamma or a per-row discount), the quantile Huber loss of the taken action's quantiles against them, its diagnostics
// and its dense gradient with respect to the quantiles; and the expected action values of a quantile head (include/mxv_qr.h, DESIGN.md
// §23).
//
// The results are defined bit for bit by the rule in the header: float64, one rounding per operation (this file is built with
// -ffp-contract=off like the rest of the library), every sum over the quantiles the xor butterfly of one wave and every sum over the
// rows the fixed tree of mxv_sum_tree.hpp — nothing here depends on the order in which lanes or workgroups arrive.  The argument checks
// are those of mxv_policy_host.hpp.
//
// Shape of the kernels (that of mxv_c51.hip):
//   * one WAVE owns a row, lane k = quantile k (N <= 64; lanes k >= N hold the +0.0 slots of ATOMSUM).  A row of quantiles is one
//     coalesced load of N dwords, ATOMSUM is the butterfly (DPP / permlane: no LDS), the selecting pass a uniform loop over the A
//     actions, and the pairwise pass a uniform loop over j that reads T_j from lane j (v_readlane) and accumulates into the lane's own
//     s_k and d_k in ascending j: the [N, N] errors never exist in memory.  The row index, the action, the terminated flag, the
//     discount and j* are wave-uniform: a terminated row skips the selecting pass by a uniform branch (the rule's select ignores what it
//     would compute).
//   * qr_rows: one workgroup of 4 waves per tile of 4 rows (no tile loop; the grid grows along y beyond kGridX tiles); a row leaves its
//     six scalars (term, qa, y, ae, cr, ql) in the workspace as six columns of M doubles, and row_loss / targets_out if asked.
//   * qr_leaf: one workgroup per leaf of 1024 rows sums the columns exactly as the other losses' leaves do; a batch of one leaf finishes
//     there (2 launches up to 1024 rows).  qr_tree: one workgroup per group of 1024 partials; the last level finishes.  So a forward is
//     3 launches up to 2^20 rows, 4 up to 2^30.
//   * qr_bwd: recomputes the row and writes its [A, N] gradient: N consecutive dwords per action, the actions consecutive.
//   * qr_q: one wave per (row, action); workgroups stride over tiles of 4 pairs.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/mxv_qr.h"
#include "mxv_policy_host.hpp"
#include "mxv_policy_rule.hpp"
#include "mxv_sum_tree.hpp"
#include "mxv_value_loss.hpp"

namespace {

using namespace mxv::rule;
using namespace mxv::policy_host;
using namespace mxv::sum_tree;
using namespace mxv::value_loss;

constexpr int kMaxQuantiles = 64;
// the slots of mxv_value_loss.hpp's partials and finish: sums of term, qa, y, ae, cr; max ql, min qa, max qa; a row's columns are term,
// qa, y, ae, cr, ql
static_assert(MXV_QR_STATS == kV && MXV_QR_LOSS_TERM == 0 && MXV_QR_Q_TAKEN_MEAN == 1 && MXV_QR_TARGET_MEAN == 2 && MXV_QR_TD_ABS_MEAN == 3 &&
                  MXV_QR_CROSSING_FRACTION == 4 && MXV_QR_ROW_LOSS_MAX == 5 && MXV_QR_Q_TAKEN_MIN == 6 && MXV_QR_Q_TAKEN_MAX == 7,
              "mxv_qr.h's stats are the slots of mxv_value_loss.hpp");

struct QrArgs {
    const float *quantiles, *target_quantiles, *reward, *next, *online, *discount, *weights;
    const void *actions;
    const uint8_t *terminated;
    const float *g;                  // backward: the incoming gradient of the loss, one float32
    double *cols;                    // forward: [6][M]
    float *row_loss, *targets_out;   // forward, optional
    float *grad;                     // backward: [M][A][N], contiguous
    float *q_out;                    // qr_q: [M][A], contiguous
    double gamma, kappa, Nf;         // Nf = (double)N
    int64_t M, ld, next_ld, online_ld, tiles;
    int32_t A, N, i64;
};

// ---- Q of one action: lane k holds quantile k, lanes k >= N the +0.0 slots ----
__device__ __forceinline__ double mean_of(const float *row, int k, int N, double Nf) {
    double x = 0.0;
    if (k < N) x = (double)row[k];
    return wave_tree<Add>(x) / Nf;
}

// ---- one row of the rule; every field but T, s and d is the same in every lane ----
struct Row {
    double T, s, d;       // lane k: the target quantile k, and the lane's sums of the weighted Huber terms and of their derivatives
    double qa, y, ae, cr, ql;
    int32_t col;          // the stored action, or -1 for anything outside 0..A-1
};

__device__ __forceinline__ Row row_of(const QrArgs &p, int64_t i, int k) {
    const int N = p.N, A = p.A;
    const bool in = k < N;
    const double Nf = p.Nf, kappa = p.kappa;
    Row w;
    const int64_t v = p.i64 ? static_cast<const int64_t *>(p.actions)[i] : (int64_t) static_cast<const int32_t *>(p.actions)[i];
    const bool ok = v >= 0 && v < (int64_t)A;
    w.col = ok ? (int32_t)v : -1;
    const float *row = p.quantiles + i * p.ld + (ok ? v : 0) * N;      // a bad action reads action 0 and is replaced
    double th = 0.0;
    if (in) th = (double)row[k];
    const double qa = wave_tree<Add>(th) / Nf;
    double T = 0.0;
    if (p.target_quantiles) {      // uniform: the target mode
        if (in) T = (double)p.target_quantiles[i * N + k];
    } else {
        const bool term = p.terminated[i] != 0;      // uniform: one row per wave
        const double r = (double)p.reward[i];
        T = r;
        if (!term) {      // a terminated row ignores both next tensors and the discount entirely
            const float *sel = p.online ? p.online + i * p.online_ld : p.next + i * p.next_ld;
            double best = 0.0;
            int jmax = 0;
            bool selbad = false;
            for (int a = 0; a < A; ++a) {
                const double Q = mean_of(sel + a * N, k, N, Nf);
                selbad |= Q != Q;
                const bool up = a == 0 || Q > best;      // strict >: the first maximum wins
                best = up ? Q : best;
                jmax = up ? a : jmax;
            }
            jmax = __builtin_amdgcn_readfirstlane(jmax);
            double nv = 0.0;
            if (in) nv = (double)p.next[i * p.next_ld + jmax * N + k];
            nv = selbad ? nan64() : nv;
            const double g = p.discount ? (double)p.discount[i] : p.gamma;
            T = r + g * nv;
        }
        T = in ? T : 0.0;
    }
    w.T = T;
    w.y = wave_tree<Add>(T) / Nf;
    const double ae = __builtin_fabs(qa - w.y);
    const double tau = (double)(2 * k + 1) / (double)(2 * N), ctau = 1.0 - tau;
    const double hk = 0.5 * kappa;
    double s = 0.0, d = 0.0;
    for (int j = 0; j < N; ++j) {      // ascending j: the rule's order
        const double u = lane_value(T, j) - th;
        const double au = __builtin_fabs(u);
        const bool small = au <= kappa;      // false for a NaN: h is then NaN by arithmetic, dh by the select below
        const double h = small ? 0.5 * (u * u) : kappa * (au - hk);
        double dh = small ? u : (u < 0.0 ? -kappa : kappa);
        dh = u != u ? nan64() : dh;
        const double wg = u < 0.0 ? ctau : tau;
        s = s + wg * (h / kappa);
        d = d + wg * (dh / kappa);
    }
    w.s = in ? s : 0.0;
    w.d = d;
    const double ql = wave_tree<Add>(w.s) / Nf;
    double c = 0.0;
    if (k + 1 < N) c = (double)row[k + 1] < th ? 1.0 : 0.0;      // lane k reads th_{k+1} from memory again
    const double cs = wave_tree<Add>(c);
    const double cr = N > 1 ? cs / (double)(N - 1) : 0.0;
    w.qa = ok ? qa : nan64();
    w.ae = ok ? ae : nan64();
    w.cr = ok ? cr : nan64();
    w.ql = ok ? ql : nan64();
    return w;
}

// ---- forward: the rows ----
__global__ void __launch_bounds__(kThreads) qr_rows(const QrArgs p) {
    const int wave = wave_of_block(), lane = threadIdx.x & 63;
    const bool has_w = p.weights != nullptr;      // uniform
    const int64_t i = tile_of_block() * kWaves + wave;
    if (i >= p.M) return;      // a whole wave
    const Row w = row_of(p, i, lane);
    const double term = has_w ? (double)p.weights[i] * w.ql : w.ql;
    if (lane == 0) {
        double *c = p.cols + i;
        c[0] = term;
        c[p.M] = w.qa;
        c[2 * p.M] = w.y;
        c[3 * p.M] = w.ae;
        c[4 * p.M] = w.cr;
        c[5 * p.M] = w.ql;
        if (p.row_loss) p.row_loss[i] = to_f32(w.ql);
    }
    if (p.targets_out && lane < p.N) p.targets_out[i * p.N + lane] = to_f32(w.T);
}

// ---- forward: the leaves and the tree (mxv_value_loss.hpp) ----
__global__ void __launch_bounds__(kThreads) qr_leaf(const LeafArgs a) {
    __shared__ double sm[kThreads / 64][kV];
    leaf_columns(sm, a);
}

__global__ void __launch_bounds__(kThreads) qr_tree(const TreeArgs t) {
    __shared__ double sm[kThreads / 64][kV];
    tree_level(sm, t);
}

// ---- backward ----
__global__ void __launch_bounds__(kThreads) qr_bwd(const QrArgs p) {
    const float nan = __uint_as_float(0x7FC00000u);
    const int wave = wave_of_block(), lane = threadIdx.x & 63;
    const bool has_w = p.weights != nullptr;      // uniform
    const double gs = (double)p.g[0] / (double)p.M;
    const int64_t i = tile_of_block() * kWaves + wave;
    if (i >= p.M) return;      // a whole wave
    const Row w = row_of(p, i, lane);
    const double dl = -(w.d / p.Nf);
    const float val = to_f32(gs * (has_w ? (double)p.weights[i] * dl : dl));
    if (lane < p.N) {
        float *out = p.grad + i * p.A * p.N + lane;
        for (int a = 0; a < p.A; ++a) out[a * p.N] = w.col < 0 ? nan : (a == w.col ? val : 0.0f);
    }
}

// ---- the expected values of every (row, action) ----
__global__ void __launch_bounds__(kThreads) qr_q(const QrArgs p) {
    const int wave = wave_of_block(), lane = threadIdx.x & 63;
    const int64_t pairs = p.M * p.A;
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t n = tile * kWaves + wave;
        if (n >= pairs) continue;      // a whole wave
        const int64_t i = n / p.A, a = n - i * p.A;
        const double Q = mean_of(p.quantiles + i * p.ld + a * p.N, lane, p.N, p.Nf);
        if (lane == 0) p.q_out[n] = to_f32(Q);
    }
}

// ---- host ----
using QCall = Call<mxv::QrCall>;

int check_quantiles(const QCall &call, int32_t N) {
    if (N < 1 || N > kMaxQuantiles) return call.bad("%s: N = %d must be in 1..%d", call.api, (int)N, kMaxQuantiles);
    return MXV_OK;
}

int check_rows_ld(const QCall &call, const char *name, int64_t ld, int64_t M, int32_t A, int32_t N) {
    if (ld < (int64_t)A * N) return call.bad("%s: row stride %s = %lld must be at least A * N = %d", call.api, name, (long long)ld, (int)(A * N));
    return call.check_stride(ld, M);
}

constexpr ArgNames kNames = {"quantiles", "target_quantiles", "next_quantiles", "next_quantiles_online"};

// what the forward and the backward check alike; fills the inputs of `p`
int check_loss(const QCall &call, int64_t M, int32_t A, int32_t N, const float *quantiles, int64_t ld, const void *actions, int32_t action_bytes,
               const float *target_quantiles, const float *reward, const uint8_t *terminated, const float *next, int64_t next_ld,
               const float *online, int64_t online_ld, double gamma, const float *discount, double kappa, const float *weights, QrArgs &p) {
    if (int rc = check_batch(call, kNames, quantiles, actions, M, A)) return rc;
    if (int rc = check_quantiles(call, N)) return rc;
    if (!std::isfinite(kappa) || !(kappa > 0.0)) return call.bad("%s: kappa = %g must be finite and above 0", call.api, kappa);
    const auto check_ld = [&](const char *name, int64_t stride) { return check_rows_ld(call, name, stride, M, A, N); };
    if (int rc = check_ld("quantiles_ld", ld)) return rc;
    if (int rc = check_targets(call, kNames, action_bytes, target_quantiles, reward, terminated, next, next_ld, online, online_ld, discount, gamma,
                               check_ld))
        return rc;
    p.quantiles = quantiles; p.actions = actions; p.target_quantiles = target_quantiles; p.reward = reward; p.terminated = terminated;
    p.next = next; p.online = online; p.discount = discount; p.weights = weights; p.gamma = gamma; p.kappa = kappa;
    p.M = M; p.ld = ld; p.next_ld = next_ld; p.online_ld = online_ld; p.tiles = (M + kWaves - 1) / kWaves;
    p.i64 = action_bytes == 8;
    p.A = A; p.N = N; p.Nf = (double)N;
    return MXV_OK;
}

constexpr int kInputs = 10;
// the byte ranges of the inputs, in the order of the arguments; an absent one has lo == 0
void input_ranges(const QrArgs &p, const float *g, Range *r) {
    const uint64_t mb = (uint64_t)p.M * 4, ab = p.i64 ? 8 : 4;
    const int32_t W = p.A * p.N;
    r[0] = {"quantiles", (uintptr_t)p.quantiles, rows_bytes(p.M, p.ld, W), 4};
    r[1] = {"actions", (uintptr_t)p.actions, (uint64_t)p.M * ab, ab};
    r[2] = {"target_quantiles", (uintptr_t)p.target_quantiles, mb * (uint64_t)p.N, 4};
    r[3] = {"reward", (uintptr_t)p.reward, mb, 4};
    r[4] = {"terminated", (uintptr_t)p.terminated, (uint64_t)p.M, 1};
    r[5] = {"next_quantiles", (uintptr_t)p.next, p.next ? rows_bytes(p.M, p.next_ld, W) : 0, 4};
    r[6] = {"next_quantiles_online", (uintptr_t)p.online, p.online ? rows_bytes(p.M, p.online_ld, W) : 0, 4};
    r[7] = {"discount", (uintptr_t)p.discount, mb, 4};
    r[8] = {"weights", (uintptr_t)p.weights, mb, 4};
    r[9] = {"grad_loss", (uintptr_t)g, 4, 4};
}

}  // namespace

extern "C" {

int64_t mxv_qr_workspace_bytes(int64_t M) { return M < 1 || M > kMaxElems ? 0 : workspace_doubles(M) * (int64_t)sizeof(double); }

int mxv_qr_loss(void *stream, int64_t M, int32_t A, int32_t N, const float *quantiles_dev, int64_t quantiles_ld, const void *actions_dev,
                int32_t action_bytes, const float *target_quantiles_dev, const float *reward_dev, const uint8_t *terminated_dev,
                const float *next_quantiles_dev, int64_t next_quantiles_ld, const float *next_quantiles_online_dev,
                int64_t next_quantiles_online_ld, double gamma, const float *discount_dev, double kappa, const float *weights_dev,
                void *workspace_dev, int64_t workspace_bytes, float *row_loss_dev, float *targets_out_dev, float *loss_out_dev,
                float *stats_out_dev) {
    const QCall call{"mxv_qr_loss", 'M'};
    QrArgs p{};
    if (int rc = check_loss(call, M, A, N, quantiles_dev, quantiles_ld, actions_dev, action_bytes, target_quantiles_dev, reward_dev, terminated_dev,
                            next_quantiles_dev, next_quantiles_ld, next_quantiles_online_dev, next_quantiles_online_ld, gamma, discount_dev, kappa,
                            weights_dev, p))
        return rc;
    if (!loss_out_dev) return call.bad("%s: loss_out pointer is NULL", call.api);
    if (!stats_out_dev) return call.bad("%s: stats_out pointer is NULL", call.api);
    const int64_t need = mxv_qr_workspace_bytes(M);
    if (int rc = check_workspace(call, "mxv_qr_workspace_bytes", M, workspace_dev, workspace_bytes, need)) return rc;
    Range ins[kInputs];
    input_ranges(p, nullptr, ins);
    const Range outs[] = {{"workspace", (uintptr_t)workspace_dev, (uint64_t)need, 8},
                          {"row_loss", (uintptr_t)row_loss_dev, (uint64_t)M * 4, 4},
                          {"targets_out", (uintptr_t)targets_out_dev, (uint64_t)M * (uint64_t)N * 4, 4},
                          {"loss_out", (uintptr_t)loss_out_dev, 4, 4},
                          {"stats_out", (uintptr_t)stats_out_dev, MXV_QR_STATS * 4, 4}};
    if (int rc = call.check_ranges(M, ins, kInputs, outs, 5)) return rc;
    p.cols = static_cast<double *>(workspace_dev);
    p.row_loss = row_loss_dev;
    p.targets_out = targets_out_dev;
    if (int rc = launch_rows(call, reinterpret_cast<const void *>(&qr_rows), p, stream)) return rc;
    return sum_columns(call, reinterpret_cast<const void *>(&qr_leaf), reinterpret_cast<const void *>(&qr_tree), p.cols, M, loss_out_dev,
                       stats_out_dev, stream);
}

int mxv_qr_loss_backward(void *stream, int64_t M, int32_t A, int32_t N, const float *quantiles_dev, int64_t quantiles_ld,
                         const void *actions_dev, int32_t action_bytes, const float *target_quantiles_dev, const float *reward_dev,
                         const uint8_t *terminated_dev, const float *next_quantiles_dev, int64_t next_quantiles_ld,
                         const float *next_quantiles_online_dev, int64_t next_quantiles_online_ld, double gamma, const float *discount_dev,
                         double kappa, const float *weights_dev, const float *grad_loss_dev, float *grad_quantiles_dev) {
    const QCall call{"mxv_qr_loss_backward", 'M'};
    QrArgs p{};
    if (int rc = check_loss(call, M, A, N, quantiles_dev, quantiles_ld, actions_dev, action_bytes, target_quantiles_dev, reward_dev, terminated_dev,
                            next_quantiles_dev, next_quantiles_ld, next_quantiles_online_dev, next_quantiles_online_ld, gamma, discount_dev, kappa,
                            weights_dev, p))
        return rc;
    if (!grad_loss_dev) return call.bad("%s: grad_loss pointer is NULL", call.api);
    if (!grad_quantiles_dev) return call.bad("%s: grad_quantiles pointer is NULL", call.api);
    Range ins[kInputs];
    input_ranges(p, grad_loss_dev, ins);
    const Range outs[] = {{"grad_quantiles", (uintptr_t)grad_quantiles_dev, (uint64_t)M * (uint64_t)(A * N) * 4, 4}};
    if (int rc = call.check_ranges(M, ins, kInputs, outs, 1)) return rc;
    p.g = grad_loss_dev; p.grad = grad_quantiles_dev;
    return launch_rows(call, reinterpret_cast<const void *>(&qr_bwd), p, stream);
}

int mxv_qr_q_values(void *stream, int64_t M, int32_t A, int32_t N, const float *quantiles_dev, int64_t quantiles_ld, float *q_out_dev) {
    const QCall call{"mxv_qr_q_values", 'M'};
    if (!quantiles_dev) return call.bad("%s: quantiles pointer is NULL", call.api);
    if (!q_out_dev) return call.bad("%s: q_out pointer is NULL", call.api);
    if (int rc = check_counts(call, M, A)) return rc;
    if (int rc = check_quantiles(call, N)) return rc;
    if (int rc = check_rows_ld(call, "quantiles_ld", quantiles_ld, M, A, N)) return rc;
    QrArgs p{};
    p.quantiles = quantiles_dev; p.ld = quantiles_ld; p.M = M; p.A = A; p.N = N; p.Nf = (double)N; p.q_out = q_out_dev;
    p.tiles = (M * A + kWaves - 1) / kWaves;
    const Range ins[] = {{"quantiles", (uintptr_t)quantiles_dev, rows_bytes(M, quantiles_ld, A * N), 4}};
    const Range outs[] = {{"q_out", (uintptr_t)q_out_dev, (uint64_t)M * (uint64_t)A * 4, 4}};
    if (int rc = call.check_ranges(M, ins, 1, outs, 1)) return rc;
    return call.launch(reinterpret_cast<const void *>(&qr_q), p, stream);
}

const char *mxv_qr_last_error(void) { return mxv::last_error<mxv::QrCall>(nullptr); }

}  // extern "C"
