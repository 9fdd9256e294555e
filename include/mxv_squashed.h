/* mxv_squashed.h — OPTIONAL learner-side pass: reparameterised, tanh-squashed diagonal-Gaussian draws from a policy head's mean and
 * log_std — bounded actions, the log-probability of each, and the gradients of both with respect to mean and log_std — in one launch
 * forwards and one backwards (must be included by itself, mxv.h does not include it).  What SAC, and every bounded-action actor after
 * it, asks of the engine.
 * Part of the C ABI of libmxv.so (see mxv.h for the status codes).  Handle-free: every call takes the HIP stream it runs on.
 *
 * The rule (tests/squashed_host.py).  Per row i with global index G = env_offset + i at draw step t, dims j = 0..D-1,
 * 1 <= D <= 4; mu and ls are the row's mean_j and log_std_j (float32, widened exactly).  All arithmetic is IEEE float64, one rounding per
 * operation, no FMA, in the order written.  float32() rounds to nearest even.  Every NaN written is the one pattern 0x7FC00000.  EXP, E
 * (EXP, and exactly 0 below the cut -708), LOG and the Box-Muller pair are the operation sequences of the policy header's rule
 * (gym_amd/csrc/mxv_policy_rule.hpp: exp_rule, e_of, log_rule, normal_pair), as they stand.  Everything is a select.
 *
 *   (w0,w1,w2,w3) = Philox4x32-10(key = seed, ctr = (G_lo, G_hi, t_lo, (t_hi & 0x0fffffff) | 11 << 28))      one call per row
 *   (z_0, z_1) = normal_pair(w0, w1);   (z_2, z_3) = normal_pair(w2, w3)      (a pair that no dim < D uses is not computed)
 *   per dim j, with z = z_j:
 *     sigma = EXP(ls);  n = sigma * z;  u = mu + n;  v = |u|
 *     e  = E(-2 v)
 *     q  = 1 + e
 *     th = v < 2^-27 ? v : (1 - e) / q
 *     t  = copysign(th, u)
 *     action_j = float32(bias_j + scale_j * t)
 *     corr = 2 * ((LN2 - v) - LOG(q))
 *     lp  += ((-0.5 * (z * z) - ls) - kHalfLog2Pi) - (LOG(scale_j) + corr)
 *   log_prob = float32(lp)                            (lp from 0.0, dims in index order)
 * 11 << 28 is the stream tag of these draws (mxv.h, RNG contract; the counter layout is that of tag 8): the draw of row G at step t
 * depends on (seed, G, t) alone.  `/` is the IEEE divide; the select on 2^-27 keeps th = tanh(v) within one float32 ulp where 1 - e
 * cancels.  LN2 = kLn2Hi + kLn2Lo rounded once; kHalfLog2Pi = 1/2 ln(2 pi).  corr = log(1 - tanh(u)^2) is finite for every finite u,
 * and e == 0 (v > 354) gives th = 1 exactly: action_j = float32(bias_j +- scale_j).  log_prob is the density of the returned action,
 * expressed through the unrounded u; it is not recovered from the float32 action, where 1 - a^2 would be 0 for |u| > 9.
 *
 * scale and bias are HOST arrays of D floats (read before the call returns); NULL means 1 and 0.  An action space [low, high] is
 * scale = (high - low) / 2, bias = (high + low) / 2.
 *
 * Degenerate rows — any non-finite mean_j or log_std_j, or any |log_std_j| > 80 (bad_mean, bad_log_std) — compute on zeros and have NaN
 * written to every output and every gradient of that row, and to nothing else; no error.
 *
 * Backward — mxv_squashed_sample_backward.  Nothing is saved by the forward: z, n, e, q, t are recomputed by the lines above from
 * (seed, G, t), with ga_j = grad_actions[i, j] and glp = grad_log_prob[i] (float32, widened; a NULL pointer means zeros):
 *     s  = (4 * e) / (q * q)
 *     grad_mean_j    = float32((ga_j * scale_j) * s + glp * (2 * t))
 *     grad_log_std_j = float32(((ga_j * scale_j) * s) * n + glp * ((2 * t) * n - 1))
 * s = 1 - tanh(u)^2.  z is the reparameterisation noise and carries no gradient.  With log_std_ld == 0 (one shared row) grad_log_std
 * is still per row, [N][D]: the caller sums it.
 *
 * Step.  step_dev == NULL: t = step.  Otherwise the kernel reads t from *step_dev (`step` is ignored).  Behind the FORWARD the same call
 * enqueues a single-lane kernel that stores t + 1 there, so a captured graph's replays continue the stream.  step_used_dev, when not
 * NULL, is a uint64[1] that receives the t the forward used (an ordinary store from one lane): given to the backward as its step_dev it
 * reproduces the forward's noise, however many draws were made in between.  The backward never advances anything.
 *
 * Layout.  mean, actions, grad_actions, grad_mean and grad_log_std are row-major [N][D] float32 with row strides of at least D elements
 * (views into wider buffers work); log_std likewise, or with log_std_ld == 0 one row [D] shared by all rows.  log_prob and
 * grad_log_prob are float32 [N].  log_prob_dev, step_used_dev, grad_actions_dev and grad_log_prob_dev may be NULL; of grad_mean_dev and
 * grad_log_std_dev one may be NULL (it is not written).
 *
 * Stream-ordered on `stream` (a hipStream_t; NULL = the null stream) of the current device: one kernel launch (two for a forward with
 * step_dev), no synchronisation, no allocation — recordable into a caller's hipGraph.  Every call returns MXV_ERR_INVALID_ARG (message:
 * mxv_squashed_last_error), before the device is touched, for: a NULL mean, log_std or actions pointer (forward), both gradient outputs
 * NULL (backward); N < 1; D outside 1..4; a row stride below D (except log_std_ld == 0); N * ld beyond 2^40; a scale_j that is not
 * finite or outside [2^-33, 64] (LOG's domain); a bias_j that is not finite; a pointer off its element's boundary (step_dev,
 * step_used_dev: 8 bytes); a range that would wrap past the top of the address space; an output sharing a byte with an input or with
 * another output.  A failed launch returns MXV_ERR_HIP. */
#ifndef MXV_SQUASHED_H
#define MXV_SQUASHED_H

#include "mxv.h"

#ifdef __cplusplus
extern "C" {
#endif

int mxv_squashed_sample(void *stream, int64_t N, int32_t D, const float *mean_dev, int64_t mean_ld, const float *log_std_dev,
                        int64_t log_std_ld, const float *scale, const float *bias, uint64_t seed, uint64_t env_offset, uint64_t step,
                        uint64_t *step_dev, uint64_t *step_used_dev, float *actions_dev, int64_t actions_ld, float *log_prob_dev);

int mxv_squashed_sample_backward(void *stream, int64_t N, int32_t D, const float *mean_dev, int64_t mean_ld, const float *log_std_dev,
                                 int64_t log_std_ld, const float *scale, const float *bias, uint64_t seed, uint64_t env_offset,
                                 uint64_t step, const uint64_t *step_dev, const float *grad_actions_dev, int64_t grad_actions_ld,
                                 const float *grad_log_prob_dev, float *grad_mean_dev, int64_t grad_mean_ld, float *grad_log_std_dev,
                                 int64_t grad_log_std_ld);

/* The message of the calling thread's last failed call of this header ("" before the first). */
const char *mxv_squashed_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MXV_SQUASHED_H */
