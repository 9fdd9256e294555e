/* mxv_targets.h — OPTIONAL learner-side pass: the bootstrap targets of the three value-based losses as operations of their own, with a
 * scalar gamma or a per-row discount (gamma^(steps taken), what the n-step replay rings emit) — the TD targets of the scalar Q-learning
 * loss, the projected target distribution of the categorical (51-atom) loss and the target quantiles of the quantile-regression loss
 * (must be included by itself, mxv.h does not include it).  What a call writes is what the given-targets mode of the matching loss
 * header reads: targets, then the loss, is the n-step update of every head, and the loss's backward no longer repeats the selecting
 * pass.
 * Part of the C ABI of libmxv.so (see mxv.h for the status codes).  Handle-free: every call takes the HIP stream it runs on.
 *
 * The rule (tests/targets_host.py).  All arithmetic is IEEE float64, one rounding per operation, no FMA, in the order
 * written.  float32 inputs are widened exactly.  float32() rounds to nearest even.  Every NaN written is the one pattern 0x7FC00000.
 * EXP is the operation sequence of the policy header's rule.  Everything is a select.
 *
 * Common to the three calls, per row i:
 *   term = terminated[i] != 0
 *   g    = discount ? (double)discount[i] : gamma      (with discount, gamma is not read; it must still be finite)
 *   r    = reward[i]
 * A terminated row ignores both next tensors and its discount entirely, NaN or not.
 *
 * mxv_targets_dqn — the bootstrap lines of the scalar Q-learning loss header, with g for gamma:
 *   sel = next_q_online ? next_q_online[i, :] : next_q[i, :]
 *   j* = 0; best = sel[0]; for a = 1 .. A-1: if sel[a] > best: best = sel[a], j* = a     (strict >: the first maximum wins)
 *   bad = any sel[a] is NaN
 *   nv  = bad ? NaN : next_q[i, j*]
 *   y   = term ? r : r + g * nv
 *   targets_out[i] = float32(y)
 *
 * mxv_targets_c51 — the bootstrap lines of the categorical loss header, with g for gamma.  The support, ATOMSUM and SOFT are that
 * header's:
 *   dz = (v_max - v_min) / (double)(Z - 1);   z_k = v_min + (double)k * dz,   k = 0 .. Z-1
 *   ATOMSUM(v): 64 slots, slots k >= Z holding +0.0, summed as the pairwise tree s[k] <- s[2k] + s[2k+1] six times
 *   SOFT(x) of a row of Z logits:
 *     bad = any x_k is NaN or +Inf, or every x_k is -Inf         (a bad row computes on x_k = 0 and its p_k are replaced by NaN)
 *     mx  = max_k x_k + 0.0
 *     d_k = x_k - mx
 *     e_k = d_k < -708 ? 0 : EXP(d_k)
 *     S   = ATOMSUM(e)
 *     p_k = e_k / S
 * and per row:
 *   sel = next_logits_online ? next_logits_online[i] : next_logits[i]
 *   Q_a = ATOMSUM(p_k * z_k) of SOFT(sel[a, :]),   a = 0 .. A-1
 *   j* = 0; best = Q_0; for a = 1 .. A-1: if Q_a > best: best = Q_a, j* = a      (strict >: the first maximum wins)
 *   selbad = any action's row of sel is bad
 *   tp   = the p of SOFT(next_logits[i, j*, :])
 *   pn_j = term ? (j == 0 ? 1 : 0) : (selbad ? NaN : tp_j)
 *   per atom j:
 *     tz_j = term ? r : r + g * z_j
 *     c = tz_j < v_min ? v_min : tz_j;   c = c > v_max ? v_max : c       (a NaN stays)
 *     b_j = (c - v_min) / dz;   b_j = b_j > Z-1 ? Z-1 : b_j
 *   m_k = +0.0; for j = 0 .. Z-1 in ascending order:
 *     w = 1 - |b_j - (double)k|;   w = w < 0 ? 0 : w;   m_k = m_k + pn_j * w
 *   cm = ATOMSUM_j((tz_j < v_min or tz_j > v_max) ? pn_j : 0)
 *   target_probs_out[i, k] = float32(m_k);   clipped_mass_out[i] = float32(cm)      (the latter when asked for)
 * The triangular weight w is the projection without floor, ceil, scatter or atomic: a b_j exactly on an atom gives that atom the weight 1
 * and its neighbours 0, so no mass is lost there.  A discount of 0 (the row a sampler returns from an empty ring) puts every tz_j on r,
 * as a terminated row does, but with the mass pn of the next distribution: the two agree when that mass sums to 1.
 *
 * mxv_targets_qr — the bootstrap lines of the quantile-regression loss header, which already has g:
 *   sel = next_quantiles_online ? next_quantiles_online[i] : next_quantiles[i]
 *   Q_a = ATOMSUM(sel[a, :]) / (double)N,   a = 0 .. A-1      (ATOMSUM as above with N for Z)
 *   j* = 0; best = Q_0; for a = 1 .. A-1: if Q_a > best: best = Q_a, j* = a      (strict >: the first maximum wins)
 *   selbad = any Q_a is NaN
 *   nv_j = selbad ? NaN : next_quantiles[i, j*, j]
 *   T_j = term ? r : r + g * nv_j
 *   target_quantiles_out[i, j] = float32(T_j)
 *
 * Layout.  next_q and next_q_online are float32 [M, A]; next_logits and next_logits_online float32 [M, A, Z]; next_quantiles and
 * next_quantiles_online float32 [M, A, N]; in each the dims behind the first are contiguous and the rows are *_ld floats apart (at least
 * A, A * Z, A * N); 1 <= A <= 64, 2 <= Z <= 64, 1 <= N <= 64 (more atoms or quantiles than a wave has lanes are out of scope).  reward and
 * discount are float32 [M]; terminated is uint8 [M] (nonzero = set); targets_out is float32 [M], target_probs_out float32 [M, Z],
 * target_quantiles_out float32 [M, N] and clipped_mass_out float32 [M], all contiguous.  discount, the online selector (double DQN: the
 * online network chooses, the target network evaluates) and clipped_mass_out may be NULL.  A truncated step is not an argument: the
 * caller evaluates the next rows on the final observation there.
 *
 * Each call is one kernel launch without a workspace.  Stream-ordered on `stream` (a hipStream_t; NULL = the null stream) of the current
 * device: no synchronisation, no allocation — recordable into a caller's hipGraph.  Every call returns MXV_ERR_INVALID_ARG (message:
 * mxv_targets_last_error), before the device is touched, for: a NULL required pointer; M < 1 or M beyond 2^40; A outside 1..64; Z outside
 * 2..64; N outside 1..64; a non-finite v_min or v_max, or v_min not below v_max; a row stride below the row or M * ld beyond 2^40; a
 * non-finite gamma; a pointer off its element's boundary; a range that would wrap past the top of the address space; an output sharing a
 * byte with an input or with the other output.  A failed launch returns MXV_ERR_HIP. */
#ifndef MXV_TARGETS_H
#define MXV_TARGETS_H

#include "mxv.h"

#ifdef __cplusplus
extern "C" {
#endif

int mxv_targets_dqn(void *stream, int64_t M, int32_t A, const float *next_q_dev, int64_t next_q_ld, const float *next_q_online_dev,
                    int64_t next_q_online_ld, const float *reward_dev, const uint8_t *terminated_dev, double gamma, const float *discount_dev,
                    float *targets_out_dev);

int mxv_targets_c51(void *stream, int64_t M, int32_t A, int32_t Z, const float *next_logits_dev, int64_t next_logits_ld,
                    const float *next_logits_online_dev, int64_t next_logits_online_ld, const float *reward_dev, const uint8_t *terminated_dev,
                    double gamma, const float *discount_dev, double v_min, double v_max, float *target_probs_out_dev,
                    float *clipped_mass_out_dev);

int mxv_targets_qr(void *stream, int64_t M, int32_t A, int32_t N, const float *next_quantiles_dev, int64_t next_quantiles_ld,
                   const float *next_quantiles_online_dev, int64_t next_quantiles_online_ld, const float *reward_dev,
                   const uint8_t *terminated_dev, double gamma, const float *discount_dev, float *target_quantiles_out_dev);

/* The message of the calling thread's last failed call of this header ("" before the first). */
const char *mxv_targets_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MXV_TARGETS_H */
