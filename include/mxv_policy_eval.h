/* mxv_policy_eval.h — OPTIONAL learner-side passes that re-evaluate STORED actions under the current policy head: log pi(action) and the
 * entropy of every row, and the gradients of both with respect to the head's outputs (must be included by itself, mxv.h does not include
 * it).  The update half of what mxv_policy.h samples: categorical heads (logits) and diagonal-Gaussian heads (mean, log_std).
 * Part of the C ABI of libmxv.so (see mxv.h for the status codes).  Handle-free: every call takes the HIP stream it runs on.
 *
 * The rule (tests/policy_eval_host.py).  All arithmetic is IEEE float64, one rounding per operation, no FMA, in the order
 * written.  EXP and LOG are the operation sequences of mxv_policy.h with the widened domains of its Gaussian rule (|d| <= 80 or
 * -708 <= d <= 0 for EXP, 2^-33 <= S <= 64 for LOG).  float32() rounds to nearest even; every NaN written is the one pattern 0x7FC00000.
 * No random number is drawn and no stream tag is used: the passes are functions of their arguments alone.
 *
 * Categorical, forward — mxv_policy_eval_categorical.  Per row i with its A logits x_0..x_{A-1} (float32, widened exactly) and the
 * stored action `action` (int32 or int64):
 *   m, d_a, e_a, c_a, S, T, L   exactly as in mxv_policy.h:   m = max_a x_a;  d_a = x_a - m;  e_a = d_a < -708 ? 0.0 : EXP(d_a);
 *                                S = the sum of e_a in index order from 0;  T = the sum of e_a * d_a in index order from 0, the terms
 *                                with e_a == 0 skipped;  L = LOG(S)
 *   log_prob = float32(d_action - L)
 *   entropy  = float32(L - T / S)                     (`/`: IEEE division)
 * For the logits and the action of one mxv_policy_sample_categorical call both outputs therefore have that call's bits: the probability
 * ratio of a learner that has not moved is exactly 1.
 * Degenerate rows — any NaN, any +Inf, every logit -Inf, or a stored action outside 0..A-1 — yield NaN for both outputs, and no error.
 * The action is only ever compared with the index of a logit: a bad action reads nothing outside its row.  A chosen action whose e_a
 * is 0 (a masked one) follows the arithmetic: log_prob is d_action - L, below -708 or -Inf.
 *
 * Categorical, backward — mxv_policy_eval_categorical_backward.  Recomputes the row (nothing is saved by the forward).  gl and gh are
 * the row's incoming gradients of log_prob and of entropy (float32, widened exactly).  Per logit a:
 *   q_a   = e_a / S
 *   lp_a  = d_a - L
 *   H     = L - T / S                                 (the float64 value, before any float32 rounding)
 *   dlp_a = (a == action ? 1.0 : 0.0) - q_a
 *   dH_a  = e_a == 0 ? 0.0 : -(q_a * (lp_a + H))
 *   grad_a = float32(gl * dlp_a + gh * dH_a)
 * A NULL grad_log_prob or grad_entropy leaves its term out altogether — it is not multiplied by zero: grad_a = float32(gh * dH_a) or
 * float32(gl * dlp_a).  Both NULL is an argument error.  A masked logit (e_a == 0) gets no entropy term and gl * (0.0 - q_a) with q_a = 0
 * from the log_prob term; if it is also the chosen action, gl * 1.0.  Degenerate rows (as above) write NaN to all A gradients; non-finite
 * incoming gradients follow the arithmetic.
 *
 * Gaussian, forward — mxv_policy_eval_gaussian.  Per row i and dims j = 0..D-1, 1 <= D <= 4, with mu_j, ls_j (float32, widened) and the
 * stored float32 action act_j:
 *   sigma_j = EXP(ls_j)
 *   zq_j    = ((double)act_j - mu_j) / sigma_j        (IEEE division)
 *   log_prob = float32( sum_j ((-0.5 * (zq_j * zq_j) - ls_j) - HALF_LOG_2PI) )        index order, from 0.0
 *   entropy  = float32( sum_j (ls_j + ENT_C) )                                        index order, from 0.0
 * — the lines of the Gaussian rule of mxv_policy.h, so for the mean, log_std and actions of one mxv_policy_sample_gaussian call both
 * outputs have that call's bits.  Degenerate rows are those of that rule — a non-finite mean or log_std, or |log_std| > 80 — and yield
 * NaN.  A non-finite stored action follows the arithmetic (+-Inf: log_prob = -Inf; NaN: NaN; the entropy does not depend on it).
 *
 * Gaussian, backward — mxv_policy_eval_gaussian_backward.  With gl, gh as above:
 *   grad_mean_j    = float32(gl * (zq_j / sigma_j))
 *   grad_log_std_j = float32(gl * (zq_j * zq_j - 1.0) + gh)
 * A NULL grad_log_prob leaves its term out: grad_mean_j = 0.0 and grad_log_std_j = float32(gh); a NULL grad_entropy gives
 * grad_log_std_j = float32(gl * (zq_j * zq_j - 1.0)).  Both NULL is an argument error.  grad_log_std is always per row, [M][D], also
 * when log_std is one shared row: reducing it over the rows is the caller's (gym_amd.evaluate_gaussian sums it with torch).
 * Degenerate rows write NaN to all D entries of both gradients.
 *
 * Layout.  logits / grad_logits are row-major [M][A] with row strides ld, grad_ld >= A in elements (views into wider buffers work),
 * 1 <= A <= 64.  actions is int64 [M] when actions_are_i64 is nonzero, int32 [M] otherwise.  mean, actions (Gaussian), grad_mean and
 * grad_log_std are row-major [M][D] with row strides >= D; log_std is [M][D] with log_std_ld >= D, or, with log_std_ld == 0, one row [D]
 * shared by all rows.  log_prob, entropy, grad_log_prob and grad_entropy are float32 [M].  log_prob and entropy may each be NULL, and so
 * may grad_mean and grad_log_std: a NULL output is not computed.
 *
 * Stream-ordered on `stream` (a hipStream_t; NULL = the null stream) of the current device: one kernel launch per call, no
 * synchronisation, no allocation — recordable into a caller's hipGraph.  Every call returns MXV_ERR_INVALID_ARG (message:
 * mxv_policy_eval_last_error), before the device is touched, for: a NULL logits / mean / log_std / actions / grad_logits pointer; both
 * incoming gradients NULL; M < 1; A outside 1..64; D outside 1..4; a row stride below the row's width (except log_std_ld == 0); M * ld
 * beyond 2^40; a pointer off its element's boundary; a range that would wrap past the top of the address space; an output that shares a
 * byte with the range of an input or with another output.  A failed launch returns MXV_ERR_HIP. */
#ifndef MXV_POLICY_EVAL_H
#define MXV_POLICY_EVAL_H

#include "mxv.h"

#ifdef __cplusplus
extern "C" {
#endif

int mxv_policy_eval_categorical(void *stream, int64_t M, int32_t A, const float *logits_dev, int64_t ld, const void *actions_dev,
                                int32_t actions_are_i64, float *log_prob_dev, float *entropy_dev);

int mxv_policy_eval_categorical_backward(void *stream, int64_t M, int32_t A, const float *logits_dev, int64_t ld, const void *actions_dev,
                                         int32_t actions_are_i64, const float *grad_log_prob_dev, const float *grad_entropy_dev,
                                         float *grad_logits_dev, int64_t grad_ld);

int mxv_policy_eval_gaussian(void *stream, int64_t M, int32_t D, const float *mean_dev, int64_t mean_ld, const float *log_std_dev,
                             int64_t log_std_ld, const float *actions_dev, int64_t actions_ld, float *log_prob_dev, float *entropy_dev);

int mxv_policy_eval_gaussian_backward(void *stream, int64_t M, int32_t D, const float *mean_dev, int64_t mean_ld, const float *log_std_dev,
                                      int64_t log_std_ld, const float *actions_dev, int64_t actions_ld, const float *grad_log_prob_dev,
                                      const float *grad_entropy_dev, float *grad_mean_dev, int64_t grad_mean_ld, float *grad_log_std_dev,
                                      int64_t grad_log_std_ld);

/* The message of the calling thread's last failed call of this header ("" before the first). */
const char *mxv_policy_eval_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MXV_POLICY_EVAL_H */
