// mxv_policy_eval.hip — log pi and entropy of STORED actions under the current head, and the gradients of both with respect to the
// head's outputs: categorical (logits) and diagonal-Gaussian (mean, log_std) heads (include/mxv_policy_eval.h).
//
// The results are defined bit for bit by the rule in the header: float64, one rounding per operation (this file is built with
// -ffp-contract=off like the rest of the library), EXP and LOG as the operation sequences of include/mxv_policy.h — no libm call — and
// IEEE `/`.  EXP, LOG, the constants and the degenerate-row tests are the text that mxv_policy.hip and mxv_gaussian.hip include as well
// (mxv_policy_rule.hpp), and the forward lines around them are the samplers', so a stored action re-evaluated under the head that drew
// it gets the sampler's bits.  The argument checks are those of mxv_policy_host.hpp.
//
// Shape of the kernels (arithmetic bound: ~45 fp64 operations per logit, ~45 per Gaussian dim, against 4 A + 12 or 12 D + 8 bytes a row):
//   * one lane owns one row.  Categorical, A = 2, 3, 4, 6: a straight-line instantiation holds the row, its d_a and e_a in registers and
//     evaluates EXP once per logit, forwards and backwards; a row of logits or of gradients is one access of A dwords (dwordx4 + dwordx2
//     for A = 6; the device takes them at any 4-byte boundary).  Every other A runs loops over the row that keep nothing per logit: the
//     backward evaluates EXP a second time in its last pass, where q_a needs S.  No scratch at any A
//     (tests/test_policy_eval_resources.py).
//   * the stored action is only compared with the index of a logit — never used as one: a bad action reads and writes nothing of its own.
//   * Gaussian, D = 1..4: one access of D dwords per row of mean, log_std, actions and of each gradient.  log_std_ld == 0 makes every
//     lane read the one shared row.
//   * everything in the rule is a select: a degenerate row computes on zeros and has its results replaced.
//   * the backward kernels recompute the row; nothing is saved by the forward.  A NULL incoming gradient is a term left out (a uniform
//     branch), not a zero factor.
//   * no atomics, no LDS, no inline assembly.  Grid: at most kMaxBlocks workgroups of 256 lanes, each striding over tiles of 256 rows.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/mxv_policy_eval.h"
#include "mxv_policy_host.hpp"
#include "mxv_policy_rule.hpp"

namespace {

using namespace mxv::rule;
using namespace mxv::policy_host;

struct CatArgs {
    const float *logits;
    const void *actions;
    const float *gl, *gh;         // backward: incoming gradients of log_prob and of entropy; NULL: the term is left out
    float *log_prob, *entropy;    // forward
    float *grad;                  // backward
    int64_t M, ld, grad_ld, tiles;
    int32_t A, i64;
};

struct GaussArgs {
    const float *mean, *log_std, *actions;
    const float *gl, *gh;
    float *log_prob, *entropy;
    float *grad_mean, *grad_log_std;
    int64_t M, mean_ld, log_std_ld, actions_ld, grad_mean_ld, grad_log_std_ld, tiles;
};

// LOG out of line (once per row).  Inlined, its 15 constants are hoisted out of the tile loop and kept live across it next to those of EXP
// and the kernel's arguments: more scalar registers than the loop instantiations have without spilling one, and one wave per SIMD less for
// the forward ones.  The straight-line backward instantiations inline it instead: there the call costs vector registers (every d_a and
// e_a is live across it), 82 against 68 at A = 6.
__device__ __attribute__((noinline)) double log_call(double S) { return log_rule(S); }

// round to nearest even; every NaN leaves as the one pattern
__device__ __forceinline__ float to_f32(double x) {
    const float y = (float)x;
    return y != y ? __uint_as_float(0x7FC00000u) : y;
}

// the stored action of row i, or -1 for anything outside 0..A-1
__device__ __forceinline__ int32_t action_of(const CatArgs &a, int64_t i, int A) {
    const int64_t v = a.i64 ? static_cast<const int64_t *>(a.actions)[i] : (int64_t) static_cast<const int32_t *>(a.actions)[i];
    return v >= 0 && v < (int64_t)A ? (int32_t)v : -1;
}

// gl * dlp + gh * dH with an absent term left out (HL, HH: which incoming gradients there are; at least one)
template <bool HL, bool HH>
__device__ __forceinline__ float cat_grad(double gl, double gh, double dlp, double dH) {
    if constexpr (HL && HH) return to_f32(gl * dlp + gh * dH);
    else if constexpr (HL) return to_f32(gl * dlp);
    else return to_f32(gh * dH);
}

struct Row {   // what both passes need of a row
    double m, S, T;
    bool degenerate;
};

// ---- categorical, straight line ----
template <int AT, bool BWD, bool HL, bool HH>
__device__ __forceinline__ void cat_straight(const CatArgs &a, int64_t i) {
    const float nan = __uint_as_float(0x7FC00000u);
    const float *row = a.logits + i * a.ld;
    float x[AT];
#pragma unroll
    for (int k = 0; k < AT; ++k) x[k] = row[k];      // merged into one access of AT dwords (two for AT = 6): 4-byte alignment suffices
    const int32_t act = action_of(a, i, AT);
    bool degenerate = act < 0;
    double m = (double)x[0];
#pragma unroll
    for (int k = 0; k < AT; ++k) {
        degenerate |= bad_logit(x[k]);
        if (k > 0) m = (double)x[k] > m ? (double)x[k] : m;
    }
    degenerate |= m == -(double)__builtin_inff();
    double d[AT], e[AT];
    double S = 0.0, T = 0.0;
#pragma unroll
    for (int k = 0; k < AT; ++k) {
        d[k] = degenerate ? 0.0 : (double)x[k] - m;      // a degenerate row's results are replaced: keep its arithmetic finite
        e[k] = e_of(d[k]);
        S = S + e[k];
        T = e[k] == 0.0 ? T : T + e[k] * d[k];
    }
    const double L = BWD ? log_rule(S) : log_call(S);
    const double H = L - T / S;
    if constexpr (!BWD) {
        double d_action = d[0];
#pragma unroll
        for (int k = 1; k < AT; ++k) d_action = act == k ? d[k] : d_action;
        if (a.log_prob) a.log_prob[i] = degenerate ? nan : to_f32(d_action - L);
        if (a.entropy) a.entropy[i] = degenerate ? nan : to_f32(H);
    } else {
        const double gl = HL ? (double)a.gl[i] : 0.0, gh = HH ? (double)a.gh[i] : 0.0;
        float g[AT];
#pragma unroll
        for (int k = 0; k < AT; ++k) {
            const double q = e[k] / S;
            const double lp = d[k] - L;
            const double dlp = (act == k ? 1.0 : 0.0) - q;
            const double dH = e[k] == 0.0 ? 0.0 : -(q * (lp + H));
            g[k] = degenerate ? nan : cat_grad<HL, HH>(gl, gh, dlp, dH);
        }
        float *out = a.grad + i * a.grad_ld;
#pragma unroll
        for (int k = 0; k < AT; ++k) out[k] = g[k];      // one store of AT dwords (two for AT = 6)
    }
}

// ---- categorical, any A: loops that keep nothing per logit ----
__device__ __forceinline__ Row row_loop(const float *row, int A, bool degenerate, double &d_action, int32_t act) {
    Row r;
    r.degenerate = degenerate;
    double m = (double)row[0];
    for (int k = 0; k < A; ++k) {
        const float x = row[k];
        r.degenerate |= bad_logit(x);
        if (k > 0) m = (double)x > m ? (double)x : m;
    }
    r.degenerate |= m == -(double)__builtin_inff();
    r.m = m;
    double S = 0.0, T = 0.0;
    d_action = 0.0;
    for (int k = 0; k < A; ++k) {
        const double d = r.degenerate ? 0.0 : (double)row[k] - m;
        const double e = e_of(d);
        S = S + e;
        T = e == 0.0 ? T : T + e * d;
        d_action = k == act ? d : d_action;
    }
    r.S = S;
    r.T = T;
    return r;
}

template <bool BWD, bool HL, bool HH>
__device__ __forceinline__ void cat_loop(const CatArgs &a, int64_t i) {
    const float nan = __uint_as_float(0x7FC00000u);
    const int A = a.A;
    const float *row = a.logits + i * a.ld;
    const int32_t act = action_of(a, i, A);
    double d_action;
    const Row r = row_loop(row, A, act < 0, d_action, act);
    const double L = log_call(r.S);
    const double H = L - r.T / r.S;
    if constexpr (!BWD) {
        if (a.log_prob) a.log_prob[i] = r.degenerate ? nan : to_f32(d_action - L);
        if (a.entropy) a.entropy[i] = r.degenerate ? nan : to_f32(H);
    } else {
        const double gl = HL ? (double)a.gl[i] : 0.0, gh = HH ? (double)a.gh[i] : 0.0;
        float *out = a.grad + i * a.grad_ld;
        for (int k = 0; k < A; ++k) {
            const double d = r.degenerate ? 0.0 : (double)row[k] - r.m;
            const double e = e_of(d);      // the same operations on the same operands as in row_loop: the same bits
            const double q = e / r.S;
            const double lp = d - L;
            const double dlp = (act == k ? 1.0 : 0.0) - q;
            const double dH = e == 0.0 ? 0.0 : -(q * (lp + H));
            out[k] = r.degenerate ? nan : cat_grad<HL, HH>(gl, gh, dlp, dH);
        }
    }
}

template <int AT>
__global__ void __launch_bounds__(kThreads) eval_cat_fwd(const CatArgs a) {
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t i = tile * kThreads + threadIdx.x;
        if (i >= a.M) continue;
        if constexpr (AT > 0) cat_straight<AT, false, false, false>(a, i);
        else cat_loop<false, false, false>(a, i);
    }
}

template <int AT>
__global__ void __launch_bounds__(kThreads) eval_cat_bwd(const CatArgs a) {
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t i = tile * kThreads + threadIdx.x;
        if (i >= a.M) continue;
        if (a.gl && a.gh) {      // uniform: which incoming gradients there are
            if constexpr (AT > 0) cat_straight<AT, true, true, true>(a, i);
            else cat_loop<true, true, true>(a, i);
        } else if (a.gl) {
            if constexpr (AT > 0) cat_straight<AT, true, true, false>(a, i);
            else cat_loop<true, true, false>(a, i);
        } else {
            if constexpr (AT > 0) cat_straight<AT, true, false, true>(a, i);
            else cat_loop<true, false, true>(a, i);
        }
    }
}

// ---- Gaussian ----
template <int D, bool BWD>
__device__ __forceinline__ void gauss_row(const GaussArgs &a, int64_t i) {
    const float nan = __uint_as_float(0x7FC00000u);
    const float *mrow = a.mean + i * a.mean_ld, *srow = a.log_std + i * a.log_std_ld, *arow = a.actions + i * a.actions_ld;
    float m32[D], s32[D], a32[D];
#pragma unroll
    for (int j = 0; j < D; ++j) m32[j] = mrow[j];      // merged into one access of D dwords: 4-byte alignment suffices
#pragma unroll
    for (int j = 0; j < D; ++j) s32[j] = srow[j];
#pragma unroll
    for (int j = 0; j < D; ++j) a32[j] = arow[j];
    bool degenerate = false;
#pragma unroll
    for (int j = 0; j < D; ++j) degenerate |= bad_mean(m32[j]) || bad_log_std(s32[j]);
    if constexpr (!BWD) {
        double lp = 0.0, en = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const double mu = degenerate ? 0.0 : (double)m32[j];      // a degenerate row's results are replaced: keep EXP inside its domain
            const double ls = degenerate ? 0.0 : (double)s32[j];
            const double sigma = exp_rule(ls);
            const double zq = ((double)a32[j] - mu) / sigma;
            lp = lp + ((-0.5 * (zq * zq) - ls) - kHalfLog2Pi);
            en = en + (ls + kEntC);
        }
        if (a.log_prob) a.log_prob[i] = degenerate ? nan : to_f32(lp);
        if (a.entropy) a.entropy[i] = degenerate ? nan : to_f32(en);
    } else {
        const bool hl = a.gl != nullptr, hh = a.gh != nullptr;      // uniform
        const double gl = hl ? (double)a.gl[i] : 0.0, gh = hh ? (double)a.gh[i] : 0.0;
        float gm[D], gs[D];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const double mu = degenerate ? 0.0 : (double)m32[j];
            const double ls = degenerate ? 0.0 : (double)s32[j];
            const double sigma = exp_rule(ls);
            const double zq = ((double)a32[j] - mu) / sigma;
            const double tm = gl * (zq / sigma);
            const double tl = gl * (zq * zq - 1.0);
            gm[j] = degenerate ? nan : hl ? to_f32(tm) : 0.0f;
            gs[j] = degenerate ? nan : hl ? to_f32(hh ? tl + gh : tl) : to_f32(gh);
        }
        if (a.grad_mean) {
            float *out = a.grad_mean + i * a.grad_mean_ld;
#pragma unroll
            for (int j = 0; j < D; ++j) out[j] = gm[j];      // one store of D dwords
        }
        if (a.grad_log_std) {
            float *out = a.grad_log_std + i * a.grad_log_std_ld;
#pragma unroll
            for (int j = 0; j < D; ++j) out[j] = gs[j];
        }
    }
}

template <int D>
__global__ void __launch_bounds__(kThreads) eval_gauss_fwd(const GaussArgs a) {
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t i = tile * kThreads + threadIdx.x;
        if (i >= a.M) continue;
        gauss_row<D, false>(a, i);
    }
}

template <int D>
__global__ void __launch_bounds__(kThreads) eval_gauss_bwd(const GaussArgs a) {
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t i = tile * kThreads + threadIdx.x;
        if (i >= a.M) continue;
        gauss_row<D, true>(a, i);
    }
}

// ---- host: which instantiation ----
template <template <int> class K>
const void *pick_cat(int32_t A) {
    switch (A) {
        case 2: return K<2>::ptr();
        case 3: return K<3>::ptr();
        case 4: return K<4>::ptr();
        case 6: return K<6>::ptr();
        default: return K<0>::ptr();
    }
}
template <template <int> class K>
const void *pick_gauss(int32_t D) {
    switch (D) {
        case 1: return K<1>::ptr();
        case 2: return K<2>::ptr();
        case 3: return K<3>::ptr();
        default: return K<4>::ptr();
    }
}
template <int AT> struct CatFwd { static const void *ptr() { return reinterpret_cast<const void *>(&eval_cat_fwd<AT>); } };
template <int AT> struct CatBwd { static const void *ptr() { return reinterpret_cast<const void *>(&eval_cat_bwd<AT>); } };
template <int D> struct GaussFwd { static const void *ptr() { return reinterpret_cast<const void *>(&eval_gauss_fwd<D>); } };
template <int D> struct GaussBwd { static const void *ptr() { return reinterpret_cast<const void *>(&eval_gauss_bwd<D>); } };

}  // namespace

extern "C" {

int mxv_policy_eval_categorical(void *stream, int64_t M, int32_t A, const float *logits_dev, int64_t ld, const void *actions_dev,
                                int32_t actions_are_i64, float *log_prob_dev, float *entropy_dev) {
    const Call<mxv::EvalCall> call{"mxv_policy_eval_categorical", 'M'};
    if (int rc = call.check_cat(M, A, logits_dev, ld, actions_dev)) return rc;
    const uint64_t ab = actions_are_i64 ? 8 : 4;
    const Range ins[] = {{"logits", (uintptr_t)logits_dev, rows_bytes(M, ld, A), 4}, {"actions", (uintptr_t)actions_dev, (uint64_t)M * ab, ab}};
    const Range outs[] = {{"log_prob", (uintptr_t)log_prob_dev, (uint64_t)M * 4, 4}, {"entropy", (uintptr_t)entropy_dev, (uint64_t)M * 4, 4}};
    if (int rc = call.check_ranges(M, ins, 2, outs, 2)) return rc;
    CatArgs a{};
    a.logits = logits_dev; a.actions = actions_dev; a.log_prob = log_prob_dev; a.entropy = entropy_dev;
    a.M = M; a.ld = ld; a.tiles = (M + kThreads - 1) / kThreads; a.A = A; a.i64 = actions_are_i64 ? 1 : 0;
    return call.launch(pick_cat<CatFwd>(A), a, stream);
}

int mxv_policy_eval_categorical_backward(void *stream, int64_t M, int32_t A, const float *logits_dev, int64_t ld, const void *actions_dev,
                                         int32_t actions_are_i64, const float *grad_log_prob_dev, const float *grad_entropy_dev,
                                         float *grad_logits_dev, int64_t grad_ld) {
    const Call<mxv::EvalCall> call{"mxv_policy_eval_categorical_backward", 'M'};
    if (int rc = call.check_cat(M, A, logits_dev, ld, actions_dev)) return rc;
    if (!grad_logits_dev) return call.bad("%s: grad_logits pointer is NULL", call.api);
    if (!grad_log_prob_dev && !grad_entropy_dev) return call.bad("%s: grad_log_prob and grad_entropy are both NULL: there is nothing to propagate", call.api);
    if (grad_ld < A) return call.bad("%s: row stride grad_ld = %lld must be at least A = %d", call.api, (long long)grad_ld, (int)A);
    if (int rc = call.check_stride(grad_ld, M)) return rc;
    const uint64_t ab = actions_are_i64 ? 8 : 4;
    const Range ins[] = {{"logits", (uintptr_t)logits_dev, rows_bytes(M, ld, A), 4}, {"actions", (uintptr_t)actions_dev, (uint64_t)M * ab, ab},
                         {"grad_log_prob", (uintptr_t)grad_log_prob_dev, (uint64_t)M * 4, 4}, {"grad_entropy", (uintptr_t)grad_entropy_dev, (uint64_t)M * 4, 4}};
    const Range outs[] = {{"grad_logits", (uintptr_t)grad_logits_dev, rows_bytes(M, grad_ld, A), 4}};
    if (int rc = call.check_ranges(M, ins, 4, outs, 1)) return rc;
    CatArgs a{};
    a.logits = logits_dev; a.actions = actions_dev; a.gl = grad_log_prob_dev; a.gh = grad_entropy_dev; a.grad = grad_logits_dev;
    a.M = M; a.ld = ld; a.grad_ld = grad_ld; a.tiles = (M + kThreads - 1) / kThreads; a.A = A; a.i64 = actions_are_i64 ? 1 : 0;
    return call.launch(pick_cat<CatBwd>(A), a, stream);
}

int mxv_policy_eval_gaussian(void *stream, int64_t M, int32_t D, const float *mean_dev, int64_t mean_ld, const float *log_std_dev,
                             int64_t log_std_ld, const float *actions_dev, int64_t actions_ld, float *log_prob_dev, float *entropy_dev) {
    const Call<mxv::EvalCall> call{"mxv_policy_eval_gaussian", 'M'};
    if (int rc = call.check_gauss(M, D, mean_dev, mean_ld, log_std_dev, log_std_ld, actions_dev, actions_ld)) return rc;
    const Range ins[] = {{"mean", (uintptr_t)mean_dev, rows_bytes(M, mean_ld, D), 4}, {"log_std", (uintptr_t)log_std_dev, rows_bytes(M, log_std_ld, D), 4},
                         {"actions", (uintptr_t)actions_dev, rows_bytes(M, actions_ld, D), 4}};
    const Range outs[] = {{"log_prob", (uintptr_t)log_prob_dev, (uint64_t)M * 4, 4}, {"entropy", (uintptr_t)entropy_dev, (uint64_t)M * 4, 4}};
    if (int rc = call.check_ranges(M, ins, 3, outs, 2)) return rc;
    GaussArgs a{};
    a.mean = mean_dev; a.log_std = log_std_dev; a.actions = actions_dev; a.log_prob = log_prob_dev; a.entropy = entropy_dev;
    a.M = M; a.mean_ld = mean_ld; a.log_std_ld = log_std_ld; a.actions_ld = actions_ld; a.tiles = (M + kThreads - 1) / kThreads;
    return call.launch(pick_gauss<GaussFwd>(D), a, stream);
}

int mxv_policy_eval_gaussian_backward(void *stream, int64_t M, int32_t D, const float *mean_dev, int64_t mean_ld, const float *log_std_dev,
                                      int64_t log_std_ld, const float *actions_dev, int64_t actions_ld, const float *grad_log_prob_dev,
                                      const float *grad_entropy_dev, float *grad_mean_dev, int64_t grad_mean_ld, float *grad_log_std_dev,
                                      int64_t grad_log_std_ld) {
    const Call<mxv::EvalCall> call{"mxv_policy_eval_gaussian_backward", 'M'};
    if (int rc = call.check_gauss(M, D, mean_dev, mean_ld, log_std_dev, log_std_ld, actions_dev, actions_ld)) return rc;
    if (!grad_log_prob_dev && !grad_entropy_dev) return call.bad("%s: grad_log_prob and grad_entropy are both NULL: there is nothing to propagate", call.api);
    if (grad_mean_dev && grad_mean_ld < D)
        return call.bad("%s: row stride grad_mean_ld = %lld must be at least D = %d", call.api, (long long)grad_mean_ld, (int)D);
    if (grad_log_std_dev && grad_log_std_ld < D)
        return call.bad("%s: row stride grad_log_std_ld = %lld must be at least D = %d", call.api, (long long)grad_log_std_ld, (int)D);
    if (!grad_mean_dev) grad_mean_ld = D;      // an absent output has no layout
    if (!grad_log_std_dev) grad_log_std_ld = D;
    for (const int64_t ld : {grad_mean_ld, grad_log_std_ld})
        if (int rc = call.check_stride(ld, M)) return rc;
    const Range ins[] = {{"mean", (uintptr_t)mean_dev, rows_bytes(M, mean_ld, D), 4}, {"log_std", (uintptr_t)log_std_dev, rows_bytes(M, log_std_ld, D), 4},
                         {"actions", (uintptr_t)actions_dev, rows_bytes(M, actions_ld, D), 4},
                         {"grad_log_prob", (uintptr_t)grad_log_prob_dev, (uint64_t)M * 4, 4}, {"grad_entropy", (uintptr_t)grad_entropy_dev, (uint64_t)M * 4, 4}};
    const Range outs[] = {{"grad_mean", (uintptr_t)grad_mean_dev, rows_bytes(M, grad_mean_ld, D), 4},
                          {"grad_log_std", (uintptr_t)grad_log_std_dev, rows_bytes(M, grad_log_std_ld, D), 4}};
    if (int rc = call.check_ranges(M, ins, 5, outs, 2)) return rc;
    GaussArgs a{};
    a.mean = mean_dev; a.log_std = log_std_dev; a.actions = actions_dev; a.gl = grad_log_prob_dev; a.gh = grad_entropy_dev;
    a.grad_mean = grad_mean_dev; a.grad_log_std = grad_log_std_dev;
    a.M = M; a.mean_ld = mean_ld; a.log_std_ld = log_std_ld; a.actions_ld = actions_ld; a.grad_mean_ld = grad_mean_ld;
    a.grad_log_std_ld = grad_log_std_ld; a.tiles = (M + kThreads - 1) / kThreads;
    return call.launch(pick_gauss<GaussBwd>(D), a, stream);
}

const char *mxv_policy_eval_last_error(void) { return mxv::last_error<mxv::EvalCall>(nullptr); }

}  // extern "C"
