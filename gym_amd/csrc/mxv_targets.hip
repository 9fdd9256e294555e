// mxv_targets.hip — the bootstrap targets of the three value-based losses as operations of their own, with a scalar gamma or a per-row
// discount: the TD targets of the scalar Q-learning loss, the projected target distribution of the categorical loss and the target
// quantiles of the quantile-regression loss (include/mxv_targets.h).  What a call writes is what the given-targets mode of
// the matching loss reads.
//
// The results are defined bit for bit by the rule in the header: float64, one rounding per operation (this file is built with
// -ffp-contract=off like the rest of the library), EXP the sequence of mxv_policy_rule.hpp, every sum over the atoms or quantiles the
// xor butterfly of one wave.  There is no sum over the rows, so no workspace and no tree: each call is one launch.  The argument checks
// are those of mxv_policy_host.hpp and mxv_value_loss.hpp.
//
// Shape of the kernels:
//   * targets_c51, targets_qr: one WAVE owns a row, lane k = atom or quantile k, one workgroup of 4 waves per tile of 4 rows launched
//     through grid_rows — the rows kernels of mxv_c51.hip and mxv_qr.hip without their loss half.  The selecting pass is a uniform loop
//     over the A actions, the projection a uniform loop over j that reads b_j and pn_j from lane j and accumulates into the lane's own
//     m_k in ascending j.  A terminated row skips the selecting pass by a uniform branch.  No LDS.
//   * targets_dqn: one LANE owns a row, as dqn_leaf of mxv_dqn.hip reads its rows; workgroups stride over tiles of 256 rows.
//   * soft() and the projection loop are copies of the twenty-odd lines that mxv_c51.hip keeps in its anonymous namespace: that file's
//     kernels are pinned instruction for instruction by its resource test, so the lines are not moved out of it (DESIGN.md §24 notes
//     the fold for later).  The copies are held to the originals bit for bit by tests/test_gpu_targets.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/mxv_targets.h"
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
constexpr int kMaxQuantiles = 64;

struct TargetsArgs {
    const float *next, *online, *reward, *discount;
    const uint8_t *terminated;
    float *out;                      // [M], [M][Z] or [M][N], contiguous
    float *clipped;                  // targets_c51: [M], optional
    double gamma, v_min, v_max, dz, z_top;      // dz = (v_max - v_min) / (Z - 1); z_top = (double)(Z - 1)
    double Nf;                       // targets_qr: (double)N
    int64_t M, next_ld, online_ld, tiles;
    int32_t A, W;                    // W: the atoms Z or the quantiles N of a row
};

__device__ __forceinline__ bool any_lane(bool c) { return __builtin_amdgcn_ballot_w64(c) != 0; }

// ---- SOFT of one row of Z logits: lane k holds atom k (the p and the bad of mxv_c51.hip's soft) ----
struct Soft {
    double p;
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
    const double e = e_of(d);
    const double S = wave_tree<Add>(e);
    const double p = e / S;
    s.p = s.bad ? nan64() : p;
    return s;
}

// ---- the categorical head: the projected target distribution of a row ----
__global__ void __launch_bounds__(kThreads) targets_c51(const TargetsArgs p) {
    const int wave = wave_of_block(), k = threadIdx.x & 63;
    const int64_t i = tile_of_block() * kWaves + wave;
    if (i >= p.M) return;      // a whole wave
    const int Z = p.W, A = p.A;
    const bool in = k < Z;
    const double kd = (double)k;
    const double z = p.v_min + kd * p.dz;
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
    const double g = p.discount ? (double)p.discount[i] : p.gamma;      // a terminated row's is selected away below
    const double boot = r + g * z;
    const double tz = term ? r : boot;
    double c = tz < p.v_min ? p.v_min : tz;
    c = c > p.v_max ? p.v_max : c;      // a NaN stays
    double b = (c - p.v_min) / p.dz;
    b = b > p.z_top ? p.z_top : b;
    const double cm = wave_tree<Add>(in && (tz < p.v_min || tz > p.v_max) ? pn : 0.0);
    double m = 0.0;
    for (int j = 0; j < Z; ++j) {      // ascending j: the rule's order
        const double bj = lane_value(b, j), pj = lane_value(pn, j);
        double wk = 1.0 - __builtin_fabs(bj - kd);
        wk = wk < 0.0 ? 0.0 : wk;
        m = m + pj * wk;
    }
    if (in) p.out[i * Z + k] = to_f32(m);
    if (p.clipped && k == 0) p.clipped[i] = to_f32(cm);
}

// ---- the quantile head: the target quantiles of a row ----
__global__ void __launch_bounds__(kThreads) targets_qr(const TargetsArgs p) {
    const int wave = wave_of_block(), k = threadIdx.x & 63;
    const int64_t i = tile_of_block() * kWaves + wave;
    if (i >= p.M) return;      // a whole wave
    const int N = p.W, A = p.A;
    const bool in = k < N;
    const bool term = p.terminated[i] != 0;      // uniform: one row per wave
    const double r = (double)p.reward[i];
    double T = r;
    if (!term) {      // a terminated row ignores both next tensors and the discount entirely
        const float *sel = p.online ? p.online + i * p.online_ld : p.next + i * p.next_ld;
        double best = 0.0;
        int jmax = 0;
        bool selbad = false;
        for (int a = 0; a < A; ++a) {
            double x = 0.0;
            if (in) x = (double)sel[a * N + k];
            const double Q = wave_tree<Add>(x) / p.Nf;
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
    if (in) p.out[i * N + k] = to_f32(T);
}

// ---- the scalar head: the TD target of a row, one lane per row ----
__global__ void __launch_bounds__(kThreads) targets_dqn(const TargetsArgs p) {
    const int A = p.A;
    const bool dbl = p.online != nullptr, has_d = p.discount != nullptr;      // uniform
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t i = tile * kThreads + threadIdx.x;
        if (i >= p.M) continue;
        const float *sel = dbl ? p.online + i * p.online_ld : p.next + i * p.next_ld;
        float best = sel[0];
        int jmax = 0;
        bool bad = best != best;
        for (int a = 1; a < A; ++a) {
            const float x = sel[a];
            bad |= x != x;
            const bool up = x > best;      // strict >: the first maximum wins
            best = up ? x : best;
            jmax = up ? a : jmax;
        }
        const float nq = p.next[i * p.next_ld + jmax];      // one dword, also when next_q itself selects (the row was just read)
        const double nv = bad ? nan64() : (double)nq;
        const double r = (double)p.reward[i];
        double g = p.gamma;
        if (has_d) g = (double)p.discount[i];
        const double boot = r + g * nv;
        p.out[i] = to_f32(p.terminated[i] ? r : boot);      // a select: a terminated row ignores what was read
    }
}

// ---- host ----
using TCall = Call<mxv::TargetsCall>;

// how a call names its next rows, its online selector and its output (ArgNames: rows and next are the same tensor here)
struct Names {
    ArgNames in;
    const char *out;
};
constexpr Names kDqn = {{"next_q", "targets_out", "next_q", "next_q_online"}, "targets_out"};
constexpr Names kC51 = {{"next_logits", "target_probs_out", "next_logits", "next_logits_online"}, "target_probs_out"};
constexpr Names kQr = {{"next_quantiles", "target_quantiles_out", "next_quantiles", "next_quantiles_online"}, "target_quantiles_out"};

// what the three calls check alike, for rows of `W` floats an action (`width`: "A", "A * Z", "A * N"); fills `p`
int check_call(const TCall &call, const Names &n, int64_t M, int32_t A, int32_t W, const char *width, const float *next, int64_t next_ld,
               const float *online, int64_t online_ld, const float *reward, const uint8_t *terminated, double gamma, const float *discount,
               float *out, TargetsArgs &p) {
    if (!next) return call.bad("%s: %s pointer is NULL", call.api, n.in.next);
    if (!reward) return call.bad("%s: reward pointer is NULL", call.api);
    if (!terminated) return call.bad("%s: terminated pointer is NULL", call.api);
    if (!out) return call.bad("%s: %s pointer is NULL", call.api, n.out);
    if (int rc = check_counts(call, M, A)) return rc;
    const int64_t row = (int64_t)A * W;
    const auto check_ld = [&](const char *name, int64_t ld) {
        if (ld < row) return call.bad("%s: row stride %s_ld = %lld must be at least %s = %d", call.api, name, (long long)ld, width, (int)row);
        return call.check_stride(ld, M);
    };
    if (int rc = check_ld(n.in.next, next_ld)) return rc;
    if (online)
        if (int rc = check_ld(n.in.online, online_ld)) return rc;
    if (!std::isfinite(gamma)) return call.bad("%s: gamma = %g must be finite", call.api, gamma);
    p.next = next; p.online = online; p.reward = reward; p.terminated = terminated; p.discount = discount; p.out = out; p.gamma = gamma;
    p.M = M; p.next_ld = next_ld; p.online_ld = online_ld; p.A = A; p.W = W;
    return MXV_OK;
}

// alignment, address-space fit and overlap of the five inputs and the two outputs (`out_row` floats a row of the first)
int check_memory(const TCall &call, const Names &n, const TargetsArgs &p, int32_t out_row) {
    const uint64_t mb = (uint64_t)p.M * 4;
    const int32_t row = p.A * p.W;
    const Range ins[] = {{n.in.next, (uintptr_t)p.next, rows_bytes(p.M, p.next_ld, row), 4},
                         {n.in.online, (uintptr_t)p.online, p.online ? rows_bytes(p.M, p.online_ld, row) : 0, 4},
                         {"reward", (uintptr_t)p.reward, mb, 4},
                         {"terminated", (uintptr_t)p.terminated, (uint64_t)p.M, 1},
                         {"discount", (uintptr_t)p.discount, mb, 4}};
    const Range outs[] = {{n.out, (uintptr_t)p.out, mb * (uint64_t)out_row, 4}, {"clipped_mass_out", (uintptr_t)p.clipped, mb, 4}};
    return call.check_ranges(p.M, ins, 5, outs, 2);
}

}  // namespace

extern "C" {

int mxv_targets_dqn(void *stream, int64_t M, int32_t A, const float *next_q_dev, int64_t next_q_ld, const float *next_q_online_dev,
                    int64_t next_q_online_ld, const float *reward_dev, const uint8_t *terminated_dev, double gamma, const float *discount_dev,
                    float *targets_out_dev) {
    const TCall call{"mxv_targets_dqn", 'M'};
    TargetsArgs p{};
    if (int rc = check_call(call, kDqn, M, A, 1, "A", next_q_dev, next_q_ld, next_q_online_dev, next_q_online_ld, reward_dev, terminated_dev, gamma,
                            discount_dev, targets_out_dev, p))
        return rc;
    if (int rc = check_memory(call, kDqn, p, 1)) return rc;
    p.tiles = (M + kThreads - 1) / kThreads;
    return call.launch(reinterpret_cast<const void *>(&targets_dqn), p, stream);
}

int mxv_targets_c51(void *stream, int64_t M, int32_t A, int32_t Z, const float *next_logits_dev, int64_t next_logits_ld,
                    const float *next_logits_online_dev, int64_t next_logits_online_ld, const float *reward_dev, const uint8_t *terminated_dev,
                    double gamma, const float *discount_dev, double v_min, double v_max, float *target_probs_out_dev,
                    float *clipped_mass_out_dev) {
    const TCall call{"mxv_targets_c51", 'M'};
    if (Z < 2 || Z > kMaxAtoms) return call.bad("%s: Z = %d must be in 2..%d", call.api, (int)Z, kMaxAtoms);
    if (!std::isfinite(v_min) || !std::isfinite(v_max)) return call.bad("%s: v_min = %g and v_max = %g must be finite", call.api, v_min, v_max);
    if (!(v_min < v_max)) return call.bad("%s: v_min = %g must be below v_max = %g", call.api, v_min, v_max);
    TargetsArgs p{};
    if (int rc = check_call(call, kC51, M, A, Z, "A * Z", next_logits_dev, next_logits_ld, next_logits_online_dev, next_logits_online_ld, reward_dev,
                            terminated_dev, gamma, discount_dev, target_probs_out_dev, p))
        return rc;
    p.clipped = clipped_mass_out_dev;
    if (int rc = check_memory(call, kC51, p, Z)) return rc;
    p.v_min = v_min; p.v_max = v_max;
    p.z_top = (double)(Z - 1);
    p.dz = (v_max - v_min) / p.z_top;
    p.tiles = (M + kWaves - 1) / kWaves;
    return launch_rows(call, reinterpret_cast<const void *>(&targets_c51), p, stream);
}

int mxv_targets_qr(void *stream, int64_t M, int32_t A, int32_t N, const float *next_quantiles_dev, int64_t next_quantiles_ld,
                   const float *next_quantiles_online_dev, int64_t next_quantiles_online_ld, const float *reward_dev,
                   const uint8_t *terminated_dev, double gamma, const float *discount_dev, float *target_quantiles_out_dev) {
    const TCall call{"mxv_targets_qr", 'M'};
    if (N < 1 || N > kMaxQuantiles) return call.bad("%s: N = %d must be in 1..%d", call.api, (int)N, kMaxQuantiles);
    TargetsArgs p{};
    if (int rc = check_call(call, kQr, M, A, N, "A * N", next_quantiles_dev, next_quantiles_ld, next_quantiles_online_dev, next_quantiles_online_ld,
                            reward_dev, terminated_dev, gamma, discount_dev, target_quantiles_out_dev, p))
        return rc;
    if (int rc = check_memory(call, kQr, p, N)) return rc;
    p.Nf = (double)N;
    p.tiles = (M + kWaves - 1) / kWaves;
    return launch_rows(call, reinterpret_cast<const void *>(&targets_qr), p, stream);
}

const char *mxv_targets_last_error(void) { return mxv::last_error<mxv::TargetsCall>(nullptr); }

}  // extern "C"
