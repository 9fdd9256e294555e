/* mxv_policy.h — OPTIONAL learner-side pass from a policy head to actions, their log-probabilities and the entropy of every row, in one
 * launch (must be included by itself, mxv.h does not include it): categorical draws from logits (first), diagonal-Gaussian draws from
 * mean and log_std (mxv_policy_sample_gaussian, below).
 * Part of the C ABI of libmxv.so (see mxv.h for the status codes).  Handle-free: the call takes the HIP stream it runs on.
 *
 * The rule (tests/policy_host.py).  Per env i with global index G = env_offset + i and its A logits x_0..x_{A-1}
 * (float32, widened exactly).  All arithmetic is IEEE float64, one rounding per operation, no FMA, in the order written:
 *   m    = max_a x_a                                  (m = x_0; m = x_a > m ? x_a : m for a = 1..A-1)
 *   d_a  = x_a - m                                    (<= 0)
 *   e_a  = d_a < -708 ? 0.0 : EXP(d_a)
 *   c_a  = c_{a-1} + e_a,  c_{-1} = 0                 (index order)      S = c_{A-1}   (1 <= S <= A)
 *   w    = word [G & 3] of Philox4x32-10(key = seed, ctr = (g_lo, g_hi, t_lo, (t_hi & 0x0fffffff) | 7 << 28)),  g = G >> 2
 *   u    = (w + 0.5) * 2^-32   (the engine's u01)     thr = u * S
 *   action   = the smallest a with c_a > thr          (A-1 if none)
 *   T    = T + e_a * d_a over a in index order, T = 0 first, the terms with e_a == 0 skipped
 *   L    = LOG(S)
 *   log_prob = float32(d_action - L)
 *   entropy  = float32(L - T / S)                     (`/`: IEEE division)
 * float32() rounds to nearest even.  7 << 28 is the stream tag of these draws (mxv.h, RNG contract): the draw of env G at step t
 * depends on (seed, G, t) alone — not on N, on env_offset, or on how calls are grouped into launches or graphs.
 *
 * Masks.  An action whose e_a is 0 can never be selected: c_a does not move there, and thr > 0.  A logit of -Inf (or one more than 708
 * below the largest) therefore masks its action; it adds nothing to S or to the entropy either.
 *
 * Degenerate rows — any NaN, any +Inf, or every logit -Inf — yield action = 0 and log_prob = entropy = NaN, written as the one pattern
 * 0x7FC00000 (as mxv_gae.h fixes it), and no error: the action stays valid for the env, the NaNs tell the learner.
 *
 * EXP and LOG are these operation sequences, not calls into a math library (tools/policy_coefficients.py generates the constants:
 * exact fractions, or ln 2 / 1/ln 2 / sqrt(1/2), rounded once to double; they are listed in gym_amd/csrc/mxv_policy_rule.hpp):
 *   EXP(d), -708 <= d <= 0:
 *     k = rint(d * inv_ln2)                           (round half to even)
 *     r = (d - k * ln2_hi) - k * ln2_lo               (ln2_hi: the first 32 bits of ln 2, so k * ln2_hi is exact)
 *     p = Horner in r with 1/j!, j = 13..0:  p = 1/13!;  p = p * r + 1/j!  for j = 12..0
 *     EXP = ldexp(p, k)                               (exact: with the -708 cut every result is a normal number)
 *   LOG(S), 1 <= S <= 64:
 *     (f, e) = frexp(S);  if f < sqrt_half: f = 2 f, e = e - 1          (f in [sqrt 1/2, sqrt 2))
 *     s = (f - 1) / (f + 1)                           (IEEE division)
 *     z = s * s
 *     p = Horner in z with 1/(2j+1), j = 11..0:  p = 1/23;  p = p * z + 1/(2j+1)  for j = 10..0
 *     LOG = ((e * ln2_hi) + (2 s) * p) + e * ln2_lo
 * Measured against 200-bit arithmetic (tests/test_policy_host.py, before the float32 rounding): |log_prob - exact| <= 7.70 * 2^-53 and
 * |entropy - exact| <= 6.14 * 2^-53 over 15 000 rows with A in {2, 3, 4, 6, 17}; EXP within 1.09 ulp.
 *
 * logits is row-major [N][A] with row stride ld >= A in elements (views into wider buffers work), 1 <= A <= 64.  actions is int64 [N]
 * when actions_are_i64 is nonzero, int32 [N] otherwise.  log_prob_dev and entropy_dev (float32 [N]) may each be NULL.
 * step_dev == NULL: t = step.  Otherwise the kernel reads t from *step_dev (`step` is ignored) and the same call enqueues a single-lane
 * kernel behind it that stores t + 1 there: a captured graph's replays continue the stream, as mxv_set_device_clock does for the engine.
 *
 * Stream-ordered on `stream` (a hipStream_t; NULL = the null stream) of the current device: one kernel launch, two with step_dev, no
 * synchronisation, no allocation — recordable into a caller's hipGraph.  Returns MXV_ERR_INVALID_ARG, before the device is touched,
 * for: a NULL logits or actions pointer; N < 1; A outside 1..64; ld < A; N * ld beyond 2^40; a pointer off its element's boundary
 * (step_dev: 8 bytes); a range that would wrap past the top of the address space; an output that shares a byte with the range of the
 * logits [logits, logits + (N-1) ld + A), with step_dev, or with another output.  A failed launch returns MXV_ERR_HIP. */
#ifndef MXV_POLICY_H
#define MXV_POLICY_H

#include "mxv.h"

#ifdef __cplusplus
extern "C" {
#endif

int mxv_policy_sample_categorical(void *stream, int64_t N, int32_t A, const float *logits_dev, int64_t ld, uint64_t seed,
                                  uint64_t env_offset, uint64_t step, uint64_t *step_dev, void *actions_dev, int32_t actions_are_i64,
                                  float *log_prob_dev, float *entropy_dev);

/* Diagonal-Gaussian draws for Box action spaces: from a policy head's mean and log_std to actions, log pi(action) and the entropy of every
 * row, in one launch (tests/gaussian_host.py).
 *
 * The rule.  Per env i with global index G = env_offset + i and dims j = 0..D-1, 1 <= D <= 4; mu_j and ls_j are the row's mean and log_std
 * (float32, widened exactly).  All arithmetic is IEEE float64, one rounding per operation, no FMA, in the order written:
 *   (w0,w1,w2,w3) = Philox4x32-10(key = seed, ctr = (G_lo, G_hi, t_lo, (t_hi & 0x0fffffff) | 8 << 28))      one call per env
 *   pair p = 0 (dims 0, 1) uses (wa, wb) = (w0, w1);  pair p = 1 (dims 2, 3) uses (w2, w3)
 *   u    = (wa + 0.5) * 2^-32                         (the engine's u01; 0 < u < 1)
 *   rad  = sqrt(-2.0 * LOG(u))                        (IEEE sqrt; LOG as above with its domain widened to 2^-33 <= S < 64: e may be negative)
 *   (sn, cs) = SINCOS2PI(wb)
 *   z_{2p} = rad * cs        z_{2p+1} = rad * sn      (a dim >= D is not computed)
 *   sigma_j = EXP(ls_j)                               (EXP as above with its domain widened to |d| <= 80)
 *   a_j   = mu_j + sigma_j * z_j          act_j = float32(a_j)
 *   zq_j  = ((double)act_j - mu_j) / sigma_j          (IEEE division)
 *   log_prob = float32( sum_j ((-0.5 * (zq_j * zq_j) - ls_j) - HALF_LOG_2PI) )        index order, from 0.0
 *   entropy  = float32( sum_j (ls_j + ENT_C) )                                        index order, from 0.0
 * HALF_LOG_2PI = 1/2 ln(2 pi) and ENT_C = 1/2 + 1/2 ln(2 pi), each rounded once to double.  8 << 28 is the stream tag of these draws
 * (mxv.h, RNG contract): the draw of env G at policy step t depends on (seed, G, t) alone.  log_prob is that of the float32 action
 * actually returned — zq is recovered from act_j, not taken from z_j — so a learner that re-evaluates the density of the stored action
 * under the same head gets the probability ratio 1.
 *
 *   SINCOS2PI(w) = (sin, cos) of 2 pi v, v = (w + 0.5) * 2^-32:
 *     t = 4.0 * v                                     (exact)
 *     k = rint(t)                                     (one of 0..4; never a tie: 2 w + 1 is odd)
 *     f = t - k                                       (exact; 2^-31 <= |f| < 1/2)
 *     r = f * PIO2_HI + f * PIO2_LO                   (PIO2_HI = floor(pi/2 * 2^19) / 2^19 has 20 significant bits: the first product is
 *                                                      exact;  PIO2_LO = pi/2 - PIO2_HI, rounded once)
 *     z = r * r
 *     s = r + r * (z * P(z)),  P Horner in z with (-1)^j / (2j+1)!, j = 9..1:   P = -1/19!;  P = P * z + (-1)^j / (2j+1)!  for j = 8..1
 *     c = 1.0 + z * Q(z),      Q Horner in z with (-1)^j / (2j)!,   j = 10..1:  Q = 1/20!;   Q = Q * z + (-1)^j / (2j)!    for j = 9..1
 *     (sn, cs) by k & 3:   0: (s, c)    1: (c, -s)    2: (-s, -c)    3: (-c, s)
 * Everything is a select; there is no divergent branch in the rule.  tools/gaussian_coefficients.py generates the constants (they are
 * listed in gym_amd/csrc/mxv_policy_rule.hpp, the one text that all the kernels of this rule include).
 *
 * Range.  With 32-bit uniforms u >= 2^-33, so |z_j| <= sqrt(2 * 33 ln 2) = 6.7639...: the tails beyond 6.76 sigma (probability 1.4e-11)
 * are not drawn.
 *
 * Degenerate rows — any non-finite mean or log_std, or any |log_std| > 80 (sigma outside float32's normal range) — write the one NaN
 * pattern 0x7FC00000 to all D actions, to log_prob and to entropy, and no error.  Anything else follows from the arithmetic: an act_j that
 * rounds to +-Inf gives log_prob = -Inf.
 *
 * Measured against 200-bit arithmetic (tests/test_gaussian_host.py, before the float32 rounding): LOG on the uniforms within 1.93 ulp,
 * sin / cos within 1.21 / 1.10 ulp, EXP on [-80, 80] within 1.05 ulp, z within 2.59 ulp and 7.78 * 2^-53, |log_prob - exact| <=
 * 83.32 * 2^-53 and |entropy - exact| <= 2.61 * 2^-53 over 12 000 rows with D in {1, 2, 3, 4} and log_std in [-5, 2].
 *
 * mean and actions are row-major [N][D] with row strides mean_ld, actions_ld >= D in elements (views into wider buffers work).  log_std is
 * [N][D] with row stride log_std_ld >= D, or, with log_std_ld == 0, one row [D] shared by all envs (a state-independent log_std).
 * log_prob_dev and entropy_dev (float32 [N]) may each be NULL.  step / step_dev, the stream and the launch count are those of
 * mxv_policy_sample_categorical.  Returns MXV_ERR_INVALID_ARG (message: mxv_policy_last_error), before the device is touched, for: a NULL
 * mean, log_std or actions pointer; N < 1; D outside 1..4; a stride below D (except log_std_ld == 0); N * ld beyond 2^40; a pointer off
 * its element's boundary (step_dev: 8 bytes); a range that would wrap past the top of the address space; an output that shares a byte
 * with the range of the mean, of the log_std, with step_dev, or with another output.  A failed launch returns MXV_ERR_HIP. */
int mxv_policy_sample_gaussian(void *stream, int64_t N, int32_t D, const float *mean_dev, int64_t mean_ld, const float *log_std_dev,
                               int64_t log_std_ld, uint64_t seed, uint64_t env_offset, uint64_t step, uint64_t *step_dev,
                               float *actions_dev, int64_t actions_ld, float *log_prob_dev, float *entropy_dev);

/* The message of the calling thread's last failed call of this header ("" before the first). */
const char *mxv_policy_last_error(void);

/* Diagnostic: the instantiation of the calling thread's last successful launch — envs per lane (1; 0 before the first launch), the
 * action count of the straight-line instantiation that ran (2, 3, 4 or 6; 0: the loop for any A) and the number of workgroups. */
int mxv_policy_last_launch(int32_t *envs_per_lane, int32_t *specialised_A, uint32_t *grid);

#ifdef __cplusplus
}
#endif
#endif /* MXV_POLICY_H */
