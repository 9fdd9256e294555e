// mxv_ppo.hip — the PPO clipped-surrogate loss of a batch, its diagnostics and its gradients, and the moments the advantages are
// normalised with (include/mxv_ppo.h).
//
// The results are defined bit for bit by the rule in the header: float64, one rounding per operation (this file is built with
// -ffp-contract=off like the rest of the library), EXP the text of mxv_policy_rule.hpp, IEEE `/` and sqrt, and every sum the fixed tree
// of mxv_sum_tree.hpp over the row index — no atomics: a float atomic would make a sum depend on the order of arrival.  The argument checks are those of
// mxv_policy_host.hpp.
//
// Shape of the kernels (~40 fp64 operations for 12-24 bytes a row):
//   * ppo_leaf / moments_leaf: one workgroup of 256 lanes per leaf of 1024 consecutive rows; lane t takes rows t, t + 256, t + 512,
//     t + 768 — every wave load is a dense burst of 64 dwords — then the xor butterfly of each wave (DPP / permlane:
//     no LDS round trips) and the four waves through LDS, the only LDS there is: 4 x 8 doubles.  One leaf writes its
//     8 (2) partials to the workspace.
//   * ppo_tree: one workgroup per group of 1024 partials; the last level (one group) also finishes the loss and the diagnostics (the
//     moments) in its first lane.  So a forward is 2 launches up to 2^20 rows, 3 up to 2^30.
//   * ppo_bwd: one lane per row, workgroups striding over tiles of 256 rows; recomputes the row, reads the incoming gradient and the
//     moments from device memory.
//   * everything in the rule is a select; which optional inputs there are is a uniform branch.  No inline assembly.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/mxv_ppo.h"
#include "mxv_policy_host.hpp"
#include "mxv_policy_rule.hpp"
#include "mxv_sum_tree.hpp"

namespace {

using namespace mxv::rule;
using namespace mxv::policy_host;
using namespace mxv::sum_tree;

constexpr int kLossV = MXV_PPO_STATS, kMomentsV = 2;
constexpr double kRatioLogMax = 80.0;

struct PpoArgs {
    const float *lp, *old, *adv, *ent, *val, *ret;
    const double *moments;
    const float *g;                  // backward: the incoming gradient of the loss, one float32
    double *partials;                // forward: [leaves][8]
    float *g_lp, *g_ent, *g_val;     // backward
    double lo, hi, ecoef, vcoef;
    int64_t M, tiles;
};

struct MomentsArgs {
    const float *adv;
    double *partials;                // [leaves][2]
    int64_t M;
};

struct TreeArgs {
    const double *in;                // [count][V]
    double *out;                     // [groups][V]; unused by the last level
    int64_t count, M;
    int32_t last, has_ent, has_val;
    double ecoef, vcoef, eps;
    float *loss, *stats;             // the last level of the loss
    double *moments;                 // the last level of the moments
};

__device__ __forceinline__ double canonical(double x) { return x != x ? nan64() : x; }

// the N partials of a leaf of the loss (N = 8: the ratio's minimum and maximum are not sums) or of the moments (N = 2: both are sums).
// A ratio is never NaN here (a NaN ratio is skipped at its row) and never zero: the selects commute.
template <int N>
struct Partials {
    static constexpr int V = N;
    static constexpr bool is_min(int v) { return v == MXV_PPO_RATIO_MIN; }
    static constexpr bool is_max(int v) { return v == MXV_PPO_RATIO_MAX; }
};

// ---- one row of the rule ----
struct Row {
    double a, d, r, s;
    bool pass, nan_row, clipped;
};

__device__ __forceinline__ Row row_of(const PpoArgs &p, int64_t i, bool has_m, double mean, double inv) {
    Row w;
    const double adv = (double)p.adv[i];
    w.a = has_m ? (adv - mean) * inv : adv;
    double d = (double)p.lp[i] - (double)p.old[i];
    d = d < -kRatioLogMax ? -kRatioLogMax : (d > kRatioLogMax ? kRatioLogMax : d);
    const bool d_nan = d != d;
    const double e = exp_rule(d_nan ? 0.0 : d);
    w.d = d;
    w.r = d_nan ? nan64() : e;
    const double rc = w.r < p.lo ? p.lo : (w.r > p.hi ? p.hi : w.r);
    const double s1 = w.r * w.a, s2 = rc * w.a;
    w.nan_row = s1 != s1 || s2 != s2;
    w.s = w.nan_row ? nan64() : (s2 < s1 ? s2 : s1);
    w.pass = (w.r >= p.lo && w.r <= p.hi) || s1 < s2;
    w.clipped = w.r < p.lo || w.r > p.hi;
    return w;
}

// ---- forward: the leaves ----
__global__ void __launch_bounds__(kThreads) ppo_leaf(const PpoArgs p) {
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kLeafRows;
    const bool has_m = p.moments != nullptr, has_ent = p.ent != nullptr, has_val = p.val != nullptr;      // uniform
    const double mean = has_m ? p.moments[0] : 0.0, inv = has_m ? p.moments[1] : 0.0;
    double s = 0.0, v2 = 0.0, en = 0.0, k1 = 0.0, k3 = 0.0, cf = 0.0, mn = Min::identity(), mx = Max::identity();
#pragma unroll
    for (int j = 0; j < kLeafRows / kThreads; ++j) {
        const int64_t i = row0 + j * kThreads + tid;
        if (i >= p.M) continue;
        const Row w = row_of(p, i, has_m, mean, inv);
        s = s + w.s;
        k1 = k1 + (-w.d);
        k3 = k3 + ((w.r - 1.0) - w.d);
        cf = cf + (w.clipped ? 1.0 : 0.0);
        mn = w.r < mn ? w.r : mn;      // a NaN ratio compares false: skipped
        mx = w.r > mx ? w.r : mx;
        if (has_val) {
            const double err = (double)p.val[i] - (double)p.ret[i];
            v2 = v2 + err * err;
        }
        if (has_ent) en = en + (double)p.ent[i];
    }
    __shared__ double sm[kThreads / 64][kLossV];
    const double t[kLossV] = {wave_tree<Add>(s), has_val ? wave_tree<Add>(v2) : 0.0, has_ent ? wave_tree<Add>(en) : 0.0, wave_tree<Add>(k1),
                              wave_tree<Add>(k3), wave_tree<Add>(cf), wave_tree<Min>(mn), wave_tree<Max>(mx)};
    leave_wave_values(sm, t);
    write_partials<Partials<kLossV>>(sm, p.partials);
}

__global__ void __launch_bounds__(kThreads) moments_leaf(const MomentsArgs p) {
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kLeafRows;
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int j = 0; j < kLeafRows / kThreads; ++j) {
        const int64_t i = row0 + j * kThreads + tid;
        if (i >= p.M) continue;
        const double x = (double)p.adv[i];
        s = s + x;
        q = q + x * x;      // the product is exact: 24-bit significands
    }
    __shared__ double sm[kThreads / 64][kLossV];
    const double t[kMomentsV] = {wave_tree<Add>(s), wave_tree<Add>(q)};
    leave_wave_values(sm, t);
    write_partials<Partials<kMomentsV>>(sm, p.partials);
}

// ---- forward: one level of the tree; the last one finishes ----
template <bool LOSS>
__global__ void __launch_bounds__(kThreads) ppo_tree(const TreeArgs t) {
    using K = Partials<LOSS ? kLossV : kMomentsV>;
    __shared__ double sm[kThreads / 64][kLossV];
    fold_level<K>(sm, t.in, t.count);
    if (!t.last) {
        write_partials<K>(sm, t.out);
        return;
    }
    if (threadIdx.x != 0) return;
    const double Mf = (double)t.M;
    if constexpr (LOSS) {
        const double policy_loss = -(four_waves<Add>(sm, 0) / Mf);
        double loss = policy_loss, value_loss = 0.0, ent = 0.0;
        if (t.has_val) {
            value_loss = 0.5 * (four_waves<Add>(sm, 1) / Mf);
            loss = loss + t.vcoef * value_loss;
        }
        if (t.has_ent) {
            ent = four_waves<Add>(sm, 2) / Mf;
            loss = loss - t.ecoef * ent;
        }
        t.loss[0] = to_f32(loss);
        t.stats[MXV_PPO_POLICY_LOSS] = to_f32(policy_loss);
        t.stats[MXV_PPO_VALUE_LOSS] = to_f32(value_loss);
        t.stats[MXV_PPO_ENTROPY] = to_f32(ent);
        t.stats[MXV_PPO_APPROX_KL] = to_f32(four_waves<Add>(sm, 3) / Mf);
        t.stats[MXV_PPO_APPROX_KL3] = to_f32(four_waves<Add>(sm, 4) / Mf);
        t.stats[MXV_PPO_CLIP_FRACTION] = to_f32(four_waves<Add>(sm, 5) / Mf);
        t.stats[MXV_PPO_RATIO_MIN] = to_f32(four_waves<Min>(sm, 6));
        t.stats[MXV_PPO_RATIO_MAX] = to_f32(four_waves<Max>(sm, 7));
    } else {
        const double S = four_waves<Add>(sm, 0), Q = four_waves<Add>(sm, 1);
        const double mean = S / Mf;
        double var = (Q - S * mean) / (Mf - 1.0);
        var = var < 0.0 ? 0.0 : var;
        const double inv = 1.0 / (sqrt(var) + t.eps);
        t.moments[0] = canonical(mean);
        t.moments[1] = canonical(inv);
    }
}

// ---- backward ----
__global__ void __launch_bounds__(kThreads) ppo_bwd(const PpoArgs p) {
    const bool has_m = p.moments != nullptr;      // uniform
    const double mean = has_m ? p.moments[0] : 0.0, inv = has_m ? p.moments[1] : 0.0;
    const double gs = (double)p.g[0] / (double)p.M;
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t i = tile * kThreads + threadIdx.x;
        if (i >= p.M) continue;
        if (p.g_lp) {
            const Row w = row_of(p, i, has_m, mean, inv);
            p.g_lp[i] = w.nan_row ? __uint_as_float(0x7FC00000u) : to_f32(-(gs * (w.pass ? w.a * w.r : 0.0)));
        }
        if (p.g_val) p.g_val[i] = to_f32(gs * (p.vcoef * ((double)p.val[i] - (double)p.ret[i])));
        if (p.g_ent) p.g_ent[i] = to_f32(-(gs * p.ecoef));
    }
}

// ---- host ----
using PCall = Call<mxv::PpoCall>;

int check_rows(const PCall &call, int64_t M) {
    if (M < 1) return call.bad("%s: M = %lld must be at least 1", call.api, (long long)M);
    if (M > kMaxElems) return call.bad("%s: M = %lld is beyond 2^40 rows", call.api, (long long)M);
    return MXV_OK;
}

int check_finite(const PCall &call, const char *name, double v) {
    if (!std::isfinite(v)) return call.bad("%s: %s = %g must be finite", call.api, name, v);
    return MXV_OK;
}

int check_workspace(const PCall &call, int64_t M, const void *workspace, int64_t workspace_bytes) {
    return mxv::sum_tree::check_workspace(call, "mxv_ppo_workspace_bytes", M, workspace, workspace_bytes, mxv_ppo_workspace_bytes(M));
}

// what the forward and the backward of the loss check alike; fills the inputs of `p`
int check_loss(const PCall &call, int64_t M, const float *lp, const float *old, const float *adv, const double *moments, const float *ent,
               const float *val, const float *ret, double clip, double ecoef, double vcoef, PpoArgs &p) {
    if (!lp) return call.bad("%s: log_prob pointer is NULL", call.api);
    if (!old) return call.bad("%s: old_log_prob pointer is NULL", call.api);
    if (!adv) return call.bad("%s: advantages pointer is NULL", call.api);
    if (int rc = check_rows(call, M)) return rc;
    if ((val == nullptr) != (ret == nullptr)) return call.bad("%s: values and returns must both be given or both be NULL", call.api);
    if (int rc = check_finite(call, "clip", clip)) return rc;
    if (clip < 0.0 || clip >= 1.0) return call.bad("%s: clip = %g must be in [0, 1)", call.api, clip);
    if (int rc = check_finite(call, "entropy_coef", ecoef)) return rc;
    if (int rc = check_finite(call, "value_coef", vcoef)) return rc;
    p.lp = lp; p.old = old; p.adv = adv; p.moments = moments; p.ent = ent; p.val = val; p.ret = ret;
    p.lo = 1.0 - clip; p.hi = 1.0 + clip; p.ecoef = ecoef; p.vcoef = vcoef;
    p.M = M; p.tiles = (M + kThreads - 1) / kThreads;
    return MXV_OK;
}

}  // namespace

extern "C" {

int64_t mxv_ppo_workspace_bytes(int64_t M) { return M < 1 || M > kMaxElems ? 0 : workspace_slots(M) * kLossV * (int64_t)sizeof(double); }

int mxv_ppo_advantage_moments(void *stream, int64_t M, const float *advantages_dev, double eps, void *workspace_dev, int64_t workspace_bytes,
                              double *moments_out_dev) {
    const PCall call{"mxv_ppo_advantage_moments", 'M'};
    if (!advantages_dev) return call.bad("%s: advantages pointer is NULL", call.api);
    if (!moments_out_dev) return call.bad("%s: moments_out pointer is NULL", call.api);
    if (int rc = check_rows(call, M)) return rc;
    if (int rc = check_finite(call, "eps", eps)) return rc;
    if (eps < 0.0) return call.bad("%s: eps = %g must not be negative", call.api, eps);
    if (int rc = check_workspace(call, M, workspace_dev, workspace_bytes)) return rc;
    const Range ins[] = {{"advantages", (uintptr_t)advantages_dev, (uint64_t)M * 4, 4}};
    const Range outs[] = {{"workspace", (uintptr_t)workspace_dev, (uint64_t)mxv_ppo_workspace_bytes(M), 8},
                          {"moments_out", (uintptr_t)moments_out_dev, 2 * sizeof(double), 8}};
    if (int rc = call.check_ranges(M, ins, 1, outs, 2)) return rc;
    const int64_t leaves = leaves_of(M);
    MomentsArgs a{advantages_dev, static_cast<double *>(workspace_dev), M};
    if (int rc = call.launch_blocks(reinterpret_cast<const void *>(&moments_leaf), a, leaves, stream)) return rc;
    TreeArgs t{};
    t.M = M; t.eps = eps; t.moments = moments_out_dev;
    return run_tree(call, reinterpret_cast<const void *>(&ppo_tree<false>), kMomentsV, t, a.partials, leaves, stream);
}

int mxv_ppo_clip_loss(void *stream, int64_t M, const float *log_prob_dev, const float *old_log_prob_dev, const float *advantages_dev,
                      const double *moments_dev, const float *entropy_dev, const float *values_dev, const float *returns_dev, double clip,
                      double entropy_coef, double value_coef, void *workspace_dev, int64_t workspace_bytes, float *loss_out_dev,
                      float *stats_out_dev) {
    const PCall call{"mxv_ppo_clip_loss", 'M'};
    PpoArgs p{};
    if (int rc = check_loss(call, M, log_prob_dev, old_log_prob_dev, advantages_dev, moments_dev, entropy_dev, values_dev, returns_dev, clip,
                            entropy_coef, value_coef, p))
        return rc;
    if (!loss_out_dev) return call.bad("%s: loss_out pointer is NULL", call.api);
    if (!stats_out_dev) return call.bad("%s: stats_out pointer is NULL", call.api);
    if (int rc = check_workspace(call, M, workspace_dev, workspace_bytes)) return rc;
    const uint64_t mb = (uint64_t)M * 4;
    const Range ins[] = {{"log_prob", (uintptr_t)log_prob_dev, mb, 4}, {"old_log_prob", (uintptr_t)old_log_prob_dev, mb, 4},
                         {"advantages", (uintptr_t)advantages_dev, mb, 4}, {"moments", (uintptr_t)moments_dev, 2 * sizeof(double), 8},
                         {"entropy", (uintptr_t)entropy_dev, mb, 4}, {"values", (uintptr_t)values_dev, mb, 4}, {"returns", (uintptr_t)returns_dev, mb, 4}};
    const Range outs[] = {{"workspace", (uintptr_t)workspace_dev, (uint64_t)mxv_ppo_workspace_bytes(M), 8},
                          {"loss_out", (uintptr_t)loss_out_dev, 4, 4}, {"stats_out", (uintptr_t)stats_out_dev, MXV_PPO_STATS * 4, 4}};
    if (int rc = call.check_ranges(M, ins, 7, outs, 3)) return rc;
    const int64_t leaves = leaves_of(M);
    p.partials = static_cast<double *>(workspace_dev);
    if (int rc = call.launch_blocks(reinterpret_cast<const void *>(&ppo_leaf), p, leaves, stream)) return rc;
    TreeArgs t{};
    t.M = M; t.has_ent = entropy_dev != nullptr; t.has_val = values_dev != nullptr; t.ecoef = entropy_coef; t.vcoef = value_coef;
    t.loss = loss_out_dev; t.stats = stats_out_dev;
    return run_tree(call, reinterpret_cast<const void *>(&ppo_tree<true>), kLossV, t, p.partials, leaves, stream);
}

int mxv_ppo_clip_loss_backward(void *stream, int64_t M, const float *log_prob_dev, const float *old_log_prob_dev, const float *advantages_dev,
                               const double *moments_dev, const float *entropy_dev, const float *values_dev, const float *returns_dev,
                               double clip, double entropy_coef, double value_coef, const float *grad_loss_dev, float *grad_log_prob_dev,
                               float *grad_entropy_dev, float *grad_values_dev) {
    const PCall call{"mxv_ppo_clip_loss_backward", 'M'};
    PpoArgs p{};
    if (int rc = check_loss(call, M, log_prob_dev, old_log_prob_dev, advantages_dev, moments_dev, entropy_dev, values_dev, returns_dev, clip,
                            entropy_coef, value_coef, p))
        return rc;
    if (!grad_loss_dev) return call.bad("%s: grad_loss pointer is NULL", call.api);
    if (!grad_log_prob_dev && !grad_entropy_dev && !grad_values_dev)
        return call.bad("%s: grad_log_prob, grad_entropy and grad_values are all NULL: there is nothing to compute", call.api);
    if (grad_entropy_dev && !entropy_dev) return call.bad("%s: grad_entropy is given but entropy is NULL", call.api);
    if (grad_values_dev && !values_dev) return call.bad("%s: grad_values is given but values is NULL", call.api);
    const uint64_t mb = (uint64_t)M * 4;
    const Range ins[] = {{"log_prob", (uintptr_t)log_prob_dev, mb, 4}, {"old_log_prob", (uintptr_t)old_log_prob_dev, mb, 4},
                         {"advantages", (uintptr_t)advantages_dev, mb, 4}, {"moments", (uintptr_t)moments_dev, 2 * sizeof(double), 8},
                         {"entropy", (uintptr_t)entropy_dev, mb, 4}, {"values", (uintptr_t)values_dev, mb, 4}, {"returns", (uintptr_t)returns_dev, mb, 4},
                         {"grad_loss", (uintptr_t)grad_loss_dev, 4, 4}};
    const Range outs[] = {{"grad_log_prob", (uintptr_t)grad_log_prob_dev, mb, 4}, {"grad_entropy", (uintptr_t)grad_entropy_dev, mb, 4},
                          {"grad_values", (uintptr_t)grad_values_dev, mb, 4}};
    if (int rc = call.check_ranges(M, ins, 8, outs, 3)) return rc;
    p.g = grad_loss_dev; p.g_lp = grad_log_prob_dev; p.g_ent = grad_entropy_dev; p.g_val = grad_values_dev;
    return call.launch(reinterpret_cast<const void *>(&ppo_bwd), p, stream);
}

const char *mxv_ppo_last_error(void) { return mxv::last_error<mxv::PpoCall>(nullptr); }

}  // extern "C"
