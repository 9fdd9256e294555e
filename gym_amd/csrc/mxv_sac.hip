// mxv_sac.hip — the losses of the continuous-control learners over a batch of M rows of C critic values: the soft twin-critic target
// y = r + g (min_c Q'_c - alpha log pi') of SAC (TD3's and DDPG's without the entropy term), the loss of the C critics against it with its
// diagnostics and its dense gradient, and the actor's loss alpha log pi - min_c Q_c with its diagnostics and both gradients
// (include/mxv_sac.h).
//
// The results are defined bit for bit by the rule in the header: float64, one rounding per operation (this file is built with
// -ffp-contract=off like the rest of the library), and every sum over the rows the fixed tree of mxv_sum_tree.hpp over the row index —
// nothing here depends on the order in which lanes or workgroups arrive.  The argument checks are those of mxv_policy_host.hpp and
// mxv_value_loss.hpp.
//
// Shape of the kernels (a handful of fp64 operations a column for 4 C bytes: bound by memory):
//   * one LANE owns a row everywhere, as in mxv_dqn.hip.  CT = 1, 2 are the straight-line instantiations: a lane's row is one access of
//     CT dwords and consecutive lanes take consecutive rows; every other C runs the loops of CT = 0, which keep nothing per column.
//   * sac_targets<CT>: workgroups stride over tiles of 256 rows; one launch, no workspace, no LDS.
//   * sac_q_leaf<CT>, sac_pi_leaf<CT>: one workgroup of 256 lanes per leaf of 1024 consecutive rows; lane t takes rows t, t + 256,
//     t + 512, t + 768.  Then the xor butterfly of each wave and the four waves through LDS: 4 x 8 doubles.  A leaf writes its 8 partials
//     to the workspace (and, the critics' leaf, td_error if asked).
//   * sac_tree: one workgroup per group of 1024 partials; the last level (one group) also finishes the loss and the diagnostics in its
//     first lane.  So a forward is 2 launches up to 2^20 rows, 3 up to 2^30.
//   * sac_q_bwd<CT>: the dense [M, C] gradient, every element its own value.  CT = 1, 2: a lane stores its row as one access of CT
//     dwords.  CT = 0: a lane leaves its row's y (float64, unrounded) and weight in LDS (256 x 12 bytes), and the workgroup then walks
//     the tile's 256 C consecutive elements with lane t taking elements t, t + 256, ...: it reads q[i, c] and writes grad_q[i, c] in
//     dense bursts of 64 dwords, whatever C is.
//   * sac_pi_bwd<CT>: grad_log_prob is one dword a lane; grad_q has one value a row (the column of the first minimum) and zeros, so CT = 0
//     stages that value and its column through LDS (256 x 8 bytes) exactly as dqn_bwd<0> of mxv_dqn.hip does.
//   * everything in a row is a select; which optional inputs there are is a uniform branch.
//   * the tree — butterfly, four waves, levels, workspace, partials and finish — is mxv_sum_tree.hpp's and mxv_value_loss.hpp's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/mxv_sac.h"
#include "mxv_policy_host.hpp"
#include "mxv_policy_rule.hpp"
#include "mxv_sum_tree.hpp"
#include "mxv_value_loss.hpp"

namespace {

using namespace mxv::rule;
using namespace mxv::policy_host;
using namespace mxv::sum_tree;
using namespace mxv::value_loss;

// the slots of mxv_value_loss.hpp's partials and finish: five sums, a maximum, a minimum, a maximum
static_assert(MXV_SAC_STATS == kV && MXV_SAC_Q_LOSS_TERM == 0 && MXV_SAC_Q_TD_ABS_MEAN == 1 && MXV_SAC_Q_MEAN == 2 && MXV_SAC_Q_TARGET_MEAN == 3 &&
                  MXV_SAC_Q_CRITIC_GAP_MEAN == 4 && MXV_SAC_Q_TD_ABS_MAX == 5 && MXV_SAC_Q_MIN == 6 && MXV_SAC_Q_MAX == 7,
              "mxv_sac.h's critic stats are the slots of mxv_value_loss.hpp");
static_assert(MXV_SAC_PI_LOSS_TERM == 0 && MXV_SAC_PI_LOG_PROB_MEAN == 1 && MXV_SAC_PI_Q_PI_MEAN == 2 && MXV_SAC_PI_CRITIC_GAP_MEAN == 3 &&
                  MXV_SAC_PI_LATER_CRITIC_FRACTION == 4 && MXV_SAC_PI_LOG_PROB_MAX == 5 && MXV_SAC_PI_Q_PI_MIN == 6 && MXV_SAC_PI_Q_PI_MAX == 7,
              "mxv_sac.h's actor stats are the slots of mxv_value_loss.hpp");

struct SacArgs {
    const float *q, *targets, *reward, *next_q, *next_lp, *discount, *alpha_dev, *weights, *log_prob;
    const uint8_t *terminated;
    const float *g;                  // backward: the incoming gradient of the loss, one float32
    double *partials;                // forward: [leaves][8]
    float *out;                      // sac_targets: [M]; the critics' leaf: td_error, optional
    float *grad;                     // backward: [M][C], contiguous
    float *grad_lp;                  // the actor's backward: [M]
    double alpha, gamma, delta;
    int64_t M, q_ld, next_ld, tiles;
    int32_t C;
};

__device__ __forceinline__ float nan32() { return __uint_as_float(0x7FC00000u); }
__device__ __forceinline__ double alpha_of(const SacArgs &p) { return p.alpha_dev ? (double)p.alpha_dev[0] : p.alpha; }      // uniform

// ---- the first minimum of a row, its maximum and whether it holds a NaN ----
struct Ends {
    float mn, mx;
    int jmin;
    bool bad;
};

__device__ __forceinline__ void ends_first(Ends &m, float x) {
    m.mn = x;
    m.mx = x;
    m.jmin = 0;
    m.bad = x != x;
}
__device__ __forceinline__ void ends_next(Ends &m, float x, int c) {
    m.bad |= x != x;
    const bool down = x < m.mn;      // strict <: the first minimum wins, and -0.0 < +0.0 is false
    m.mn = down ? x : m.mn;
    m.jmin = down ? c : m.jmin;
    m.mx = x > m.mx ? x : m.mx;
}

template <int CT>
__device__ __forceinline__ Ends ends_of(const float *row, int C) {
    Ends m;
    if constexpr (CT > 0) {
        float x[CT];
#pragma unroll
        for (int k = 0; k < CT; ++k) x[k] = row[k];      // merged into one access of CT dwords: 4-byte alignment suffices
        ends_first(m, x[0]);
#pragma unroll
        for (int k = 1; k < CT; ++k) ends_next(m, x[k], k);
    } else {
        ends_first(m, row[0]);
        for (int k = 1; k < C; ++k) ends_next(m, row[k], k);
    }
    return m;
}

__device__ __forceinline__ double gap_of(const Ends &m) { return m.bad ? nan64() : (double)m.mx - (double)m.mn; }

// ---- the target of row i: given, or the soft bootstrap ----
template <int CT>
__device__ __forceinline__ double soft_target(const SacArgs &p, int64_t i, double al) {
    const Ends m = ends_of<CT>(p.next_q + i * p.next_ld, p.C);
    const double nv = m.bad ? nan64() : (double)m.mn;
    double v = nv;
    if (p.next_lp) v = nv - al * (double)p.next_lp[i];      // uniform
    double g = p.gamma;
    if (p.discount) g = (double)p.discount[i];      // uniform
    const double r = (double)p.reward[i];
    const double boot = r + g * v;
    return p.terminated[i] ? r : boot;      // a select: a terminated row ignores what was read
}

template <int CT>
__device__ __forceinline__ double target_of(const SacArgs &p, int64_t i, double al) {
    return p.targets ? (double)p.targets[i] : soft_target<CT>(p, i, al);      // uniform: the target mode
}

__global__ void __launch_bounds__(kThreads) sac_tree(const TreeArgs t) {
    __shared__ double sm[kThreads / 64][kV];
    tree_level(sm, t);
}

// ---- the soft target alone ----
template <int CT>
__global__ void __launch_bounds__(kThreads) sac_targets(const SacArgs p) {
    const double al = alpha_of(p);
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t i = tile * kThreads + threadIdx.x;
        if (i >= p.M) continue;
        p.out[i] = to_f32(soft_target<CT>(p, i, al));
    }
}

// ---- the critics ----
__device__ __forceinline__ double huber(double e, double ae, double delta) {
    const double h = ae <= delta ? 0.5 * (e * e) : delta * (ae - 0.5 * delta);
    return e != e ? nan64() : h;
}
__device__ __forceinline__ double huber_slope(double e, double ae, double delta) {
    const double dh = ae <= delta ? e : (e < 0.0 ? -delta : delta);
    return e != e ? nan64() : dh;
}

// what the columns of a row of q leave: the row's sums, the farthest error, and the lane's extrema over rows and columns
struct Cols {
    double h, sa, sq, far, fa;
    bool nan_e;
};
struct Extrema {
    double mx_ae, mn_q, mx_q;
};

__device__ __forceinline__ void col_next(Cols &w, Extrema &x, float qf, double y, double delta, bool first) {
    const double qd = (double)qf;
    const double e = qd - y;
    const double ae = __builtin_fabs(e);
    w.h = w.h + huber(e, ae, delta);
    w.sa = w.sa + ae;
    w.sq = w.sq + qd;
    const bool farther = first || ae > w.fa;      // strict >: the first of equal errors stays
    w.far = farther ? e : w.far;
    w.fa = farther ? ae : w.fa;
    w.nan_e |= e != e;
    x.mx_ae = ae > x.mx_ae ? ae : x.mx_ae;      // a NaN compares false: skipped
    x.mn_q = qd < x.mn_q ? qd : x.mn_q;
    x.mx_q = qd > x.mx_q ? qd : x.mx_q;
}

template <int CT>
__global__ void __launch_bounds__(kThreads) sac_q_leaf(const SacArgs p) {
    const int tid = threadIdx.x, C = CT > 0 ? CT : p.C;
    const int64_t row0 = (int64_t)blockIdx.x * kLeafRows;
    const bool has_w = p.weights != nullptr;      // uniform
    const double al = alpha_of(p), Cf = (double)C;
    double s = 0.0, sa = 0.0, sq = 0.0, sy = 0.0, sg = 0.0;
    Extrema x{Max::identity(), Min::identity(), Max::identity()};
#pragma unroll
    for (int j = 0; j < kLeafRows / kThreads; ++j) {
        const int64_t i = row0 + j * kThreads + tid;
        if (i >= p.M) continue;
        const double y = target_of<CT>(p, i, al);
        const float *row = p.q + i * p.q_ld;
        Cols w{0.0, 0.0, 0.0, 0.0, 0.0, false};
        Ends m;
        if constexpr (CT > 0) {
            float v[CT];
#pragma unroll
            for (int k = 0; k < CT; ++k) v[k] = row[k];      // one access of CT dwords
            ends_first(m, v[0]);
            col_next(w, x, v[0], y, p.delta, true);
#pragma unroll
            for (int k = 1; k < CT; ++k) {
                ends_next(m, v[k], k);
                col_next(w, x, v[k], y, p.delta, false);
            }
        } else {
            const float v0 = row[0];
            ends_first(m, v0);
            col_next(w, x, v0, y, p.delta, true);
            for (int k = 1; k < C; ++k) {
                const float v = row[k];
                ends_next(m, v, k);
                col_next(w, x, v, y, p.delta, false);
            }
        }
        const double term = has_w ? (double)p.weights[i] * w.h : w.h;
        s = s + term;
        sa = sa + w.sa / Cf;
        sq = sq + w.sq / Cf;
        sy = sy + y;
        sg = sg + gap_of(m);
        if (p.out) p.out[i] = to_f32(w.nan_e ? nan64() : w.far);
    }
    __shared__ double sm[kThreads / 64][kV];
    const double t[kV] = {wave_tree<Add>(s),  wave_tree<Add>(sa),      wave_tree<Add>(sq),     wave_tree<Add>(sy),
                          wave_tree<Add>(sg), wave_tree<Max>(x.mx_ae), wave_tree<Min>(x.mn_q), wave_tree<Max>(x.mx_q)};
    leave_wave_values(sm, t);
    write_partials<Partials>(sm, p.partials);
}

// grad_q[i, c] of the critics
__device__ __forceinline__ float q_grad(float qf, double y, double delta, double gs, bool has_w, double wi) {
    const double e = (double)qf - y;
    const double dh = huber_slope(e, __builtin_fabs(e), delta);
    return to_f32(gs * (has_w ? wi * dh : dh));
}

template <int CT>
__global__ void __launch_bounds__(kThreads) sac_q_bwd(const SacArgs p) {
    const bool has_w = p.weights != nullptr;      // uniform
    const double gs = (double)p.g[0] / (double)p.M, al = alpha_of(p);
    if constexpr (CT > 0) {
        for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
            const int64_t i = tile * kThreads + threadIdx.x;
            if (i >= p.M) continue;
            const double y = target_of<CT>(p, i, al);
            const double wi = has_w ? (double)p.weights[i] : 0.0;
            const float *row = p.q + i * p.q_ld;
            float v[CT], g[CT];
#pragma unroll
            for (int k = 0; k < CT; ++k) v[k] = row[k];
#pragma unroll
            for (int k = 0; k < CT; ++k) g[k] = q_grad(v[k], y, p.delta, gs, has_w, wi);
            float *out = p.grad + i * CT;
#pragma unroll
            for (int k = 0; k < CT; ++k) out[k] = g[k];      // one store of CT dwords
        }
    } else {
        __shared__ double s_y[kThreads];
        __shared__ float s_w[kThreads];
        const int tid = threadIdx.x, C = p.C;
        const float inv_C = 1.0f / (float)C;
        for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {      // the trip count is the workgroup's: the barriers are uniform
            const int64_t r0 = tile * kThreads, i = r0 + tid;
            if (i < p.M) {
                s_y[tid] = target_of<0>(p, i, al);
                s_w[tid] = has_w ? p.weights[i] : 0.0f;
            }
            __syncthreads();
            const int64_t left = p.M - r0;
            const int n = (int)(left < kThreads ? left : kThreads) * C;      // the tile's elements: at most 256 x 64
            float *out = p.grad + r0 * C;
            for (int k = tid; k < n; k += kThreads) {
                // k / C: (k + 0.5) / C is at least 1 / 128 away from an integer and the two float roundings move it by less than 2^-9
                const int r = (int)(((float)k + 0.5f) * inv_C);
                const int c = k - r * C;
                out[k] = q_grad(p.q[(r0 + r) * p.q_ld + c], s_y[r], p.delta, gs, has_w, (double)s_w[r]);
            }
            __syncthreads();
        }
    }
}

// ---- the actor ----
template <int CT>
__global__ void __launch_bounds__(kThreads) sac_pi_leaf(const SacArgs p) {
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kLeafRows;
    const bool has_w = p.weights != nullptr;      // uniform
    const double al = alpha_of(p);
    double s = 0.0, sl = 0.0, sq = 0.0, sg = 0.0, sj = 0.0, mx_lp = Max::identity(), mn_q = Min::identity(), mx_q = Max::identity();
#pragma unroll
    for (int j = 0; j < kLeafRows / kThreads; ++j) {
        const int64_t i = row0 + j * kThreads + tid;
        if (i >= p.M) continue;
        const Ends m = ends_of<CT>(p.q + i * p.q_ld, p.C);
        const double qp = m.bad ? nan64() : (double)m.mn;
        const double lp = (double)p.log_prob[i];
        const double t = al * lp - qp;
        const double term = has_w ? (double)p.weights[i] * t : t;
        s = s + term;
        sl = sl + lp;
        sq = sq + qp;
        sg = sg + gap_of(m);
        sj = sj + (m.jmin != 0 ? 1.0 : 0.0);
        mx_lp = lp > mx_lp ? lp : mx_lp;      // a NaN compares false: skipped
        mn_q = qp < mn_q ? qp : mn_q;
        mx_q = qp > mx_q ? qp : mx_q;
    }
    __shared__ double sm[kThreads / 64][kV];
    const double t[kV] = {wave_tree<Add>(s),  wave_tree<Add>(sl),    wave_tree<Add>(sq),   wave_tree<Add>(sg),
                          wave_tree<Add>(sj), wave_tree<Max>(mx_lp), wave_tree<Min>(mn_q), wave_tree<Max>(mx_q)};
    leave_wave_values(sm, t);
    write_partials<Partials>(sm, p.partials);
}

template <int CT>
__global__ void __launch_bounds__(kThreads) sac_pi_bwd(const SacArgs p) {
    const bool has_w = p.weights != nullptr;      // uniform
    const double gs = (double)p.g[0] / (double)p.M, al = alpha_of(p);
    if constexpr (CT > 0) {
        for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
            const int64_t i = tile * kThreads + threadIdx.x;
            if (i >= p.M) continue;
            const Ends m = ends_of<CT>(p.q + i * p.q_ld, CT);
            const double wi = has_w ? (double)p.weights[i] : 0.0;
            p.grad_lp[i] = to_f32(gs * (has_w ? wi * al : al));
            const float val = to_f32(-(has_w ? gs * wi : gs));
            float g[CT];
#pragma unroll
            for (int k = 0; k < CT; ++k) g[k] = m.bad ? nan32() : (m.jmin == k ? val : 0.0f);
            float *out = p.grad + i * CT;
#pragma unroll
            for (int k = 0; k < CT; ++k) out[k] = g[k];      // one store of CT dwords
        }
    } else {
        __shared__ float s_val[kThreads];
        __shared__ int32_t s_col[kThreads];
        const int tid = threadIdx.x, C = p.C;
        const float inv_C = 1.0f / (float)C;
        for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {      // the trip count is the workgroup's: the barriers are uniform
            const int64_t r0 = tile * kThreads, i = r0 + tid;
            if (i < p.M) {
                const Ends m = ends_of<0>(p.q + i * p.q_ld, C);
                const double wi = has_w ? (double)p.weights[i] : 0.0;
                p.grad_lp[i] = to_f32(gs * (has_w ? wi * al : al));
                s_val[tid] = to_f32(-(has_w ? gs * wi : gs));
                s_col[tid] = m.bad ? -1 : m.jmin;
            }
            __syncthreads();
            const int64_t left = p.M - r0;
            const int n = (int)(left < kThreads ? left : kThreads) * C;      // the tile's elements: at most 256 x 64
            float *out = p.grad + r0 * C;
            for (int k = tid; k < n; k += kThreads) {
                // k / C: (k + 0.5) / C is at least 1 / 128 away from an integer and the two float roundings move it by less than 2^-9
                const int r = (int)(((float)k + 0.5f) * inv_C);
                const int c = k - r * C, col = s_col[r];
                out[k] = col < 0 ? nan32() : (c == col ? s_val[r] : 0.0f);
            }
            __syncthreads();
        }
    }
}

// ---- host ----
using SCall = Call<mxv::SacCall>;

template <int CT> struct Targets { static const void *ptr() { return reinterpret_cast<const void *>(&sac_targets<CT>); } };
template <int CT> struct QLeaf { static const void *ptr() { return reinterpret_cast<const void *>(&sac_q_leaf<CT>); } };
template <int CT> struct QBwd { static const void *ptr() { return reinterpret_cast<const void *>(&sac_q_bwd<CT>); } };
template <int CT> struct PiLeaf { static const void *ptr() { return reinterpret_cast<const void *>(&sac_pi_leaf<CT>); } };
template <int CT> struct PiBwd { static const void *ptr() { return reinterpret_cast<const void *>(&sac_pi_bwd<CT>); } };
template <template <int> class K>
const void *pick(int32_t C) {
    switch (C) {
        case 1: return K<1>::ptr();
        case 2: return K<2>::ptr();
        default: return K<0>::ptr();
    }
}

constexpr ArgNames kNames = {"q", "targets", "next_q", "next_q_online"};      // (there is no online selector: the name is never printed)

// the row and critic counts
int check_sizes(const SCall &call, int64_t M, int32_t C) {
    if (M < 1) return call.bad("%s: M = %lld must be at least 1", call.api, (long long)M);
    if (M > kMaxElems) return call.bad("%s: M = %lld is beyond 2^40 rows", call.api, (long long)M);
    if (C < 1 || C > kMaxActions) return call.bad("%s: C = %d must be in 1..%d", call.api, (int)C, kMaxActions);
    return MXV_OK;
}

int check_rows_ld(const SCall &call, const char *name, int64_t ld, int64_t M, int32_t C) {
    if (ld < C) return call.bad("%s: row stride %s = %lld must be at least C = %d", call.api, name, (long long)ld, (int)C);
    return call.check_stride(ld, M);
}

// the temperature: it belongs to next_log_prob, and the scalar is read only without alpha_dev
int check_alpha(const SCall &call, const void *log_prob, const char *log_prob_name, double alpha, const void *alpha_dev) {
    if (alpha_dev && !log_prob) return call.bad("%s: alpha_dev is given without %s: the temperature weighs the entropy term", call.api, log_prob_name);
    if (log_prob && !alpha_dev && !std::isfinite(alpha)) return call.bad("%s: alpha = %g must be finite", call.api, alpha);
    return MXV_OK;
}

// what the critics' forward and backward check alike; fills the inputs of `p`
int check_loss(const SCall &call, int64_t M, int32_t C, const float *q, int64_t q_ld, const float *targets, const float *reward,
               const uint8_t *terminated, const float *next_q, int64_t next_q_ld, const float *next_lp, double alpha, const float *alpha_dev,
               double gamma, const float *discount, double delta, const float *weights, SacArgs &p) {
    if (!q) return call.bad("%s: q pointer is NULL", call.api);
    if (int rc = check_sizes(call, M, C)) return rc;
    const auto check_ld = [&](const char *name, int64_t stride) { return check_rows_ld(call, name, stride, M, C); };
    if (int rc = check_ld("q_ld", q_ld)) return rc;
    if (int rc = check_targets(call, kNames, 4, targets, reward, terminated, next_q, next_q_ld, nullptr, 0, discount, gamma, check_ld)) return rc;
    if (targets && next_lp) return call.bad("%s: next_log_prob is given with targets: it belongs to the bootstrap mode", call.api);
    if (targets && alpha_dev) return call.bad("%s: alpha_dev is given with targets: it belongs to the bootstrap mode", call.api);
    if (int rc = check_alpha(call, next_lp, "next_log_prob", alpha, alpha_dev)) return rc;
    if (!(delta > 0.0)) return call.bad("%s: delta = %g must be above 0 (+Inf: the half squared error)", call.api, delta);
    p.q = q; p.targets = targets; p.reward = reward; p.terminated = terminated; p.next_q = next_q; p.next_lp = next_lp; p.alpha_dev = alpha_dev;
    p.discount = discount; p.weights = weights; p.alpha = alpha; p.gamma = gamma; p.delta = delta;
    p.M = M; p.q_ld = q_ld; p.next_ld = next_q_ld; p.tiles = (M + kThreads - 1) / kThreads; p.C = C;
    return MXV_OK;
}

constexpr int kLossInputs = 10;
// the byte ranges of the critics' inputs, in the order of the arguments; an absent one has lo == 0
void loss_ranges(const SacArgs &p, const float *g, Range *r) {
    const uint64_t mb = (uint64_t)p.M * 4;
    r[0] = {"q", (uintptr_t)p.q, rows_bytes(p.M, p.q_ld, p.C), 4};
    r[1] = {"targets", (uintptr_t)p.targets, mb, 4};
    r[2] = {"reward", (uintptr_t)p.reward, mb, 4};
    r[3] = {"terminated", (uintptr_t)p.terminated, (uint64_t)p.M, 1};
    r[4] = {"next_q", (uintptr_t)p.next_q, p.next_q ? rows_bytes(p.M, p.next_ld, p.C) : 0, 4};
    r[5] = {"next_log_prob", (uintptr_t)p.next_lp, mb, 4};
    r[6] = {"alpha_dev", (uintptr_t)p.alpha_dev, 4, 4, ""};
    r[7] = {"discount", (uintptr_t)p.discount, mb, 4};
    r[8] = {"weights", (uintptr_t)p.weights, mb, 4};
    r[9] = {"grad_loss", (uintptr_t)g, 4, 4};
}

// what the actor's forward and backward check alike; fills the inputs of `p`
int check_policy(const SCall &call, int64_t M, int32_t C, const float *log_prob, const float *q, int64_t q_ld, double alpha, const float *alpha_dev,
                 const float *weights, SacArgs &p) {
    if (!log_prob) return call.bad("%s: log_prob pointer is NULL", call.api);
    if (!q) return call.bad("%s: q pointer is NULL", call.api);
    if (int rc = check_sizes(call, M, C)) return rc;
    if (int rc = check_rows_ld(call, "q_ld", q_ld, M, C)) return rc;
    if (int rc = check_alpha(call, log_prob, "log_prob", alpha, alpha_dev)) return rc;
    p.log_prob = log_prob; p.q = q; p.alpha = alpha; p.alpha_dev = alpha_dev; p.weights = weights;
    p.M = M; p.q_ld = q_ld; p.tiles = (M + kThreads - 1) / kThreads; p.C = C;
    return MXV_OK;
}

constexpr int kPolicyInputs = 5;
void policy_ranges(const SacArgs &p, const float *g, Range *r) {
    const uint64_t mb = (uint64_t)p.M * 4;
    r[0] = {"log_prob", (uintptr_t)p.log_prob, mb, 4};
    r[1] = {"q", (uintptr_t)p.q, rows_bytes(p.M, p.q_ld, p.C), 4};
    r[2] = {"alpha_dev", (uintptr_t)p.alpha_dev, 4, 4, ""};
    r[3] = {"weights", (uintptr_t)p.weights, mb, 4};
    r[4] = {"grad_loss", (uintptr_t)g, 4, 4};
}

// loss_out, stats_out and the workspace of a forward; -> the bytes the workspace needs in `need`
int check_forward(const SCall &call, int64_t M, const void *workspace, int64_t workspace_bytes, const float *loss_out, const float *stats_out,
                  int64_t &need) {
    if (!loss_out) return call.bad("%s: loss_out pointer is NULL", call.api);
    if (!stats_out) return call.bad("%s: stats_out pointer is NULL", call.api);
    need = mxv_sac_workspace_bytes(M);
    return check_workspace(call, "mxv_sac_workspace_bytes", M, workspace, workspace_bytes, need);
}

}  // namespace

extern "C" {

int mxv_sac_targets(void *stream, int64_t M, int32_t C, const float *next_q_dev, int64_t next_q_ld, const float *reward_dev,
                    const uint8_t *terminated_dev, const float *next_log_prob_dev, double alpha, const float *alpha_dev, double gamma,
                    const float *discount_dev, float *targets_out_dev) {
    const SCall call{"mxv_sac_targets", 'M'};
    if (!next_q_dev) return call.bad("%s: next_q pointer is NULL", call.api);
    if (!reward_dev) return call.bad("%s: reward pointer is NULL", call.api);
    if (!terminated_dev) return call.bad("%s: terminated pointer is NULL", call.api);
    if (!targets_out_dev) return call.bad("%s: targets_out pointer is NULL", call.api);
    if (int rc = check_sizes(call, M, C)) return rc;
    if (int rc = check_rows_ld(call, "next_q_ld", next_q_ld, M, C)) return rc;
    if (!std::isfinite(gamma)) return call.bad("%s: gamma = %g must be finite", call.api, gamma);
    if (int rc = check_alpha(call, next_log_prob_dev, "next_log_prob", alpha, alpha_dev)) return rc;
    const uint64_t mb = (uint64_t)M * 4;
    const Range ins[] = {{"next_q", (uintptr_t)next_q_dev, rows_bytes(M, next_q_ld, C), 4},
                         {"reward", (uintptr_t)reward_dev, mb, 4},
                         {"terminated", (uintptr_t)terminated_dev, (uint64_t)M, 1},
                         {"next_log_prob", (uintptr_t)next_log_prob_dev, mb, 4},
                         {"alpha_dev", (uintptr_t)alpha_dev, 4, 4, ""},
                         {"discount", (uintptr_t)discount_dev, mb, 4}};
    const Range outs[] = {{"targets_out", (uintptr_t)targets_out_dev, mb, 4}};
    if (int rc = call.check_ranges(M, ins, 6, outs, 1)) return rc;
    SacArgs p{};
    p.next_q = next_q_dev; p.reward = reward_dev; p.terminated = terminated_dev; p.next_lp = next_log_prob_dev; p.alpha = alpha;
    p.alpha_dev = alpha_dev; p.gamma = gamma; p.discount = discount_dev; p.out = targets_out_dev;
    p.M = M; p.next_ld = next_q_ld; p.tiles = (M + kThreads - 1) / kThreads; p.C = C;
    return call.launch(pick<Targets>(C), p, stream);
}

int64_t mxv_sac_workspace_bytes(int64_t M) { return M < 1 || M > kMaxElems ? 0 : workspace_slots(M) * kV * (int64_t)sizeof(double); }

int mxv_sac_loss(void *stream, int64_t M, int32_t C, const float *q_dev, int64_t q_ld, const float *targets_dev, const float *reward_dev,
                 const uint8_t *terminated_dev, const float *next_q_dev, int64_t next_q_ld, const float *next_log_prob_dev, double alpha,
                 const float *alpha_dev, double gamma, const float *discount_dev, double delta, const float *weights_dev, void *workspace_dev,
                 int64_t workspace_bytes, float *td_error_dev, float *loss_out_dev, float *stats_out_dev) {
    const SCall call{"mxv_sac_loss", 'M'};
    SacArgs p{};
    if (int rc = check_loss(call, M, C, q_dev, q_ld, targets_dev, reward_dev, terminated_dev, next_q_dev, next_q_ld, next_log_prob_dev, alpha,
                            alpha_dev, gamma, discount_dev, delta, weights_dev, p))
        return rc;
    int64_t need = 0;
    if (int rc = check_forward(call, M, workspace_dev, workspace_bytes, loss_out_dev, stats_out_dev, need)) return rc;
    Range ins[kLossInputs];
    loss_ranges(p, nullptr, ins);
    const Range outs[] = {{"workspace", (uintptr_t)workspace_dev, (uint64_t)need, 8}, {"td_error", (uintptr_t)td_error_dev, (uint64_t)M * 4, 4},
                          {"loss_out", (uintptr_t)loss_out_dev, 4, 4}, {"stats_out", (uintptr_t)stats_out_dev, MXV_SAC_STATS * 4, 4}};
    if (int rc = call.check_ranges(M, ins, kLossInputs, outs, 4)) return rc;
    const int64_t leaves = leaves_of(M);
    p.partials = static_cast<double *>(workspace_dev);
    p.out = td_error_dev;
    if (int rc = call.launch_blocks(pick<QLeaf>(C), p, leaves, stream)) return rc;
    return finish_tree(call, reinterpret_cast<const void *>(&sac_tree), p.partials, leaves, M, loss_out_dev, stats_out_dev, stream);
}

int mxv_sac_loss_backward(void *stream, int64_t M, int32_t C, const float *q_dev, int64_t q_ld, const float *targets_dev,
                          const float *reward_dev, const uint8_t *terminated_dev, const float *next_q_dev, int64_t next_q_ld,
                          const float *next_log_prob_dev, double alpha, const float *alpha_dev, double gamma, const float *discount_dev,
                          double delta, const float *weights_dev, const float *grad_loss_dev, float *grad_q_dev) {
    const SCall call{"mxv_sac_loss_backward", 'M'};
    SacArgs p{};
    if (int rc = check_loss(call, M, C, q_dev, q_ld, targets_dev, reward_dev, terminated_dev, next_q_dev, next_q_ld, next_log_prob_dev, alpha,
                            alpha_dev, gamma, discount_dev, delta, weights_dev, p))
        return rc;
    if (!grad_loss_dev) return call.bad("%s: grad_loss pointer is NULL", call.api);
    if (!grad_q_dev) return call.bad("%s: grad_q pointer is NULL", call.api);
    Range ins[kLossInputs];
    loss_ranges(p, grad_loss_dev, ins);
    const Range outs[] = {{"grad_q", (uintptr_t)grad_q_dev, (uint64_t)M * (uint64_t)C * 4, 4}};
    if (int rc = call.check_ranges(M, ins, kLossInputs, outs, 1)) return rc;
    p.g = grad_loss_dev; p.grad = grad_q_dev;
    return call.launch(pick<QBwd>(C), p, stream);
}

int mxv_sac_policy_loss(void *stream, int64_t M, int32_t C, const float *log_prob_dev, const float *q_dev, int64_t q_ld, double alpha,
                        const float *alpha_dev, const float *weights_dev, void *workspace_dev, int64_t workspace_bytes, float *loss_out_dev,
                        float *stats_out_dev) {
    const SCall call{"mxv_sac_policy_loss", 'M'};
    SacArgs p{};
    if (int rc = check_policy(call, M, C, log_prob_dev, q_dev, q_ld, alpha, alpha_dev, weights_dev, p)) return rc;
    int64_t need = 0;
    if (int rc = check_forward(call, M, workspace_dev, workspace_bytes, loss_out_dev, stats_out_dev, need)) return rc;
    Range ins[kPolicyInputs];
    policy_ranges(p, nullptr, ins);
    const Range outs[] = {{"workspace", (uintptr_t)workspace_dev, (uint64_t)need, 8}, {"loss_out", (uintptr_t)loss_out_dev, 4, 4},
                          {"stats_out", (uintptr_t)stats_out_dev, MXV_SAC_STATS * 4, 4}};
    if (int rc = call.check_ranges(M, ins, kPolicyInputs, outs, 3)) return rc;
    const int64_t leaves = leaves_of(M);
    p.partials = static_cast<double *>(workspace_dev);
    if (int rc = call.launch_blocks(pick<PiLeaf>(C), p, leaves, stream)) return rc;
    return finish_tree(call, reinterpret_cast<const void *>(&sac_tree), p.partials, leaves, M, loss_out_dev, stats_out_dev, stream);
}

int mxv_sac_policy_loss_backward(void *stream, int64_t M, int32_t C, const float *log_prob_dev, const float *q_dev, int64_t q_ld, double alpha,
                                 const float *alpha_dev, const float *weights_dev, const float *grad_loss_dev, float *grad_log_prob_dev,
                                 float *grad_q_dev) {
    const SCall call{"mxv_sac_policy_loss_backward", 'M'};
    SacArgs p{};
    if (int rc = check_policy(call, M, C, log_prob_dev, q_dev, q_ld, alpha, alpha_dev, weights_dev, p)) return rc;
    if (!grad_loss_dev) return call.bad("%s: grad_loss pointer is NULL", call.api);
    if (!grad_log_prob_dev) return call.bad("%s: grad_log_prob pointer is NULL", call.api);
    if (!grad_q_dev) return call.bad("%s: grad_q pointer is NULL", call.api);
    Range ins[kPolicyInputs];
    policy_ranges(p, grad_loss_dev, ins);
    const Range outs[] = {{"grad_log_prob", (uintptr_t)grad_log_prob_dev, (uint64_t)M * 4, 4},
                          {"grad_q", (uintptr_t)grad_q_dev, (uint64_t)M * (uint64_t)C * 4, 4}};
    if (int rc = call.check_ranges(M, ins, kPolicyInputs, outs, 2)) return rc;
    p.g = grad_loss_dev; p.grad_lp = grad_log_prob_dev; p.grad = grad_q_dev;
    return call.launch(pick<PiBwd>(C), p, stream);
}

const char *mxv_sac_last_error(void) { return mxv::last_error<mxv::SacCall>(nullptr); }

}  // extern "C"
