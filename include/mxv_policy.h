/* mxv_policy.h — OPTIONAL learner-side pass from a policy's logits to actions: categorical draws, their log-probabilities and the
 * entropy of every row, in one launch (must be included by itself, mxv.h does not include it).
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
 * exact fractions, or ln 2 / 1/ln 2 / sqrt(1/2), rounded once to double; they are listed in gym_amd/csrc/mxv_policy.hip):
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

/* The message of the calling thread's last failed call of this header ("" before the first). */
const char *mxv_policy_last_error(void);

/* Diagnostic: the instantiation of the calling thread's last successful launch — envs per lane (1; 0 before the first launch), the
 * action count of the straight-line instantiation that ran (2, 3, 4 or 6; 0: the loop for any A) and the number of workgroups. */
int mxv_policy_last_launch(int32_t *envs_per_lane, int32_t *specialised_A, uint32_t *grid);

#ifdef __cplusplus
}
#endif
#endif /* MXV_POLICY_H */
