/* mxv_sac.h — OPTIONAL learner-side pass: the three losses of the continuous-control learners over a batch of M rows of C critic values —
 * the soft twin-critic target of SAC (TD3's clipped double-Q target without the entropy term, DDPG's with one critic), the loss of the C
 * critics against it with its diagnostics and its dense gradient, and the actor's loss alpha * log pi - min_c Q with its diagnostics and
 * both gradients (must be included by itself, mxv.h does not include it).  Column c of a row is critic c's value: C = 2 is SAC / TD3,
 * C = 1 is DDPG, more columns are an ensemble whose minimum is over all of them.
 * Part of the C ABI of libmxv.so (see mxv.h for the status codes).  Handle-free: every call takes the HIP stream it runs on.
 *
 * The rule (tests/sac_host.py).  All arithmetic is IEEE float64, one rounding per operation, no FMA, in the order
 * written.  float32 inputs are widened exactly.  float32() rounds to nearest even.  Every NaN written is the one pattern 0x7FC00000.
 * Everything in a row is a select; which optional inputs are present is a uniform branch.
 *
 * Common to the calls, per row i, with r = (double)reward[i], w_i = (double)weights[i], Mf = (double)M, and x the rows the minimum is
 * taken of (next_q for the target, q for the diagnostics of the critics and for the actor):
 *   term = terminated[i] != 0
 *   g    = discount ? (double)discount[i] : gamma      (with discount, gamma is not read; it must still be finite)
 *   al   = alpha_dev ? (double)alpha_dev[0] : alpha      (one float32 in device memory, read by the kernel: no host read)
 *   mn = x[i, 0], jmin = 0;  for c = 1 .. C-1:  if x[i, c] < mn: mn = x[i, c], jmin = c     (float32 compares, strict <: ties take the first)
 *   mx = x[i, 0];  for c = 1 .. C-1:  if x[i, c] > mx: mx = x[i, c]
 *   bad = any x[i, c] is NaN
 *   gap = bad ? NaN : (double)mx - (double)mn
 * -0.0 < +0.0 is false: of two zeros the first is the minimum.
 *
 * mxv_sac_targets — the soft target (x = next_q):
 *   nv  = bad ? NaN : (double)mn
 *   v   = next_log_prob ? nv - al * (double)next_log_prob[i] : nv
 *   y   = term ? r : r + g * v                   (a terminated row ignores next_q, next_log_prob and its discount, NaN or not)
 *   targets_out[i] = float32(y)
 * Without next_log_prob (and then without alpha) it is TD3's clipped double-Q target.
 *
 * mxv_sac_loss — the critics.  targets mode: y = (double)targets[i]; bootstrap mode: the y above, unrounded.  Per column c, ascending:
 *   e_c = (double)q[i, c] - y;  ae_c = |e_c|
 *   H(e_c)  = ae_c <= delta ? 0.5 * (e_c * e_c) : delta * (ae_c - 0.5 * delta);   NaN if e_c is NaN
 *   dH(e_c) = ae_c <= delta ? e_c : (e_c < 0 ? -delta : delta);   NaN if e_c is NaN      (the inclusive edge: ae == delta is quadratic)
 *   h   = +0.0;  for c ascending: h = h + H(e_c)
 *   sa  = +0.0;  for c ascending: sa = sa + ae_c
 *   sq  = +0.0;  for c ascending: sq = sq + (double)q[i, c]
 * and per row:
 *   term_i = weights ? w_i * h : h                (an absent weight is a factor left out, not a factor of 1)
 *   am = sa / (double)C;  qm = sq / (double)C
 *   far = e_0, fa = ae_0;  for c = 1 .. C-1:  if ae_c > fa: far = e_c, fa = ae_c;  far = NaN if any e_c is NaN
 *   td_error[i] = float32(far)                    (when asked for: the error of the critic farthest from the target, first on ties)
 * Five sums over the rows — of term_i, am, qm, y, gap (x = q) — and three extrema over all rows AND columns — the maximum of ae_c, the
 * minimum and the maximum of (double)q[i, c] — by selects that skip a NaN; the extrema start at -Inf, +Inf and -Inf.
 *
 * mxv_sac_policy_loss — the actor (x = q, the critics at the reparameterised action):
 *   qp = bad ? NaN : (double)mn
 *   t  = al * (double)log_prob[i] - qp
 *   term_i = weights ? w_i * t : t
 *   later = jmin != 0 ? 1.0 : 0.0
 * Five sums over the rows — of term_i, (double)log_prob[i], qp, gap, later — and three extrema — the maximum of log_prob, the minimum and
 * the maximum of qp — by selects that skip a NaN.
 *
 * Order of additions over the rows: that of the PPO loss header and of the Q-learning loss header, exactly — a leaf of 1024 consecutive
 * rows, lane t of 256 accumulating rows t, t + 256, t + 512, t + 768 in that order from +0.0, the xor butterfly of each wave, the four
 * waves as (w0 + w1) + (w2 + w3), then levels of groups of 1024 leaves until one group is left (at least one level).  No float atomic
 * anywhere.  2 launches up to 2^20 rows, 3 up to 2^30, 4 beyond.  The last launch also finishes:
 *   loss_out  = float32(sum_0 / Mf)
 *   stats_out = float32 of (sum_0 / Mf, sum_1 / Mf, sum_2 / Mf, sum_3 / Mf, sum_4 / Mf, max_5 + 0.0, min_6 + 0.0, max_7 + 0.0)
 *
 * Backward.  Both recompute every row (nothing is saved by the forward).  gs = (double)g[0] / (double)M, g the float32 at grad_loss_dev:
 *   mxv_sac_loss_backward:
 *     grad_q[i, c] = float32(gs * (weights ? w_i * dH(e_c) : dH(e_c)))
 *   mxv_sac_policy_loss_backward:
 *     grad_log_prob[i] = float32(gs * (weights ? w_i * al : al))
 *     grad_q[i, c]     = bad ? NaN : (c == jmin ? float32(-(weights ? gs * w_i : gs)) : +0.0)
 * Every element of the gradients is written.  On a tie the first minimum takes the whole gradient (an elementwise minimum of two
 * tensors under automatic differentiation would split it in halves).
 *
 * Layout.  q and next_q are float32 [M, C] with rows q_ld, next_q_ld floats apart (each at least C), 1 <= C <= 64; targets, reward,
 * next_log_prob, discount, weights, log_prob, td_error, targets_out and grad_log_prob are float32 [M]; terminated is uint8 [M] (nonzero =
 * set); grad_q is float32 [M, C], contiguous.  alpha_dev is one float32 in device memory or NULL (then the scalar alpha is the
 * temperature); a temperature belongs to next_log_prob: alpha_dev without it is refused, and without it the scalar is not read.
 * mxv_sac_loss has exactly one target mode: targets, or all of reward, terminated and next_q; next_log_prob, alpha_dev and discount only
 * with the latter.  A truncated step is not an argument: the caller evaluates next_q on the final observation there.  discount,
 * next_log_prob, weights and td_error may be NULL.  loss_out is one float32, stats_out float32 [8], grad_loss_dev one float32, all in
 * device memory.  workspace is device memory of at least mxv_sac_workspace_bytes(M) bytes on an 8-byte boundary, for the leaves' partial
 * sums; its contents mean nothing between calls.
 *
 * mxv_sac_targets is one launch without a workspace.  Stream-ordered on `stream` (a hipStream_t; NULL = the null stream) of the current
 * device: no synchronisation, no allocation — recordable into a caller's hipGraph.  Every call returns MXV_ERR_INVALID_ARG (message:
 * mxv_sac_last_error), before the device is touched, for: a NULL required pointer; M < 1 or M beyond 2^40; C outside 1..64; a row stride
 * below C or M * ld beyond 2^40; both target modes, neither, or a bootstrap mode without all three of its inputs; next_log_prob,
 * alpha_dev or discount with targets; alpha_dev without next_log_prob; a non-finite gamma; a non-finite alpha where it is read; a delta
 * that is NaN or not above 0 (+Inf is the plain half squared error); a workspace that is too small or off an 8-byte boundary; a pointer
 * off its element's boundary; a range that would wrap past the top of the address space; an output or the workspace sharing a byte with
 * an input or with another output.  A failed launch returns MXV_ERR_HIP.  mxv_sac_workspace_bytes returns 0 for an M outside 1..2^40. */
#ifndef MXV_SAC_H
#define MXV_SAC_H

#include "mxv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* indices into stats_out of mxv_sac_loss */
#define MXV_SAC_Q_LOSS_TERM 0
#define MXV_SAC_Q_TD_ABS_MEAN 1
#define MXV_SAC_Q_MEAN 2
#define MXV_SAC_Q_TARGET_MEAN 3
#define MXV_SAC_Q_CRITIC_GAP_MEAN 4
#define MXV_SAC_Q_TD_ABS_MAX 5
#define MXV_SAC_Q_MIN 6
#define MXV_SAC_Q_MAX 7
/* indices into stats_out of mxv_sac_policy_loss */
#define MXV_SAC_PI_LOSS_TERM 0
#define MXV_SAC_PI_LOG_PROB_MEAN 1
#define MXV_SAC_PI_Q_PI_MEAN 2
#define MXV_SAC_PI_CRITIC_GAP_MEAN 3
#define MXV_SAC_PI_LATER_CRITIC_FRACTION 4
#define MXV_SAC_PI_LOG_PROB_MAX 5
#define MXV_SAC_PI_Q_PI_MIN 6
#define MXV_SAC_PI_Q_PI_MAX 7
#define MXV_SAC_STATS 8

int mxv_sac_targets(void *stream, int64_t M, int32_t C, const float *next_q_dev, int64_t next_q_ld, const float *reward_dev,
                    const uint8_t *terminated_dev, const float *next_log_prob_dev, double alpha, const float *alpha_dev, double gamma,
                    const float *discount_dev, float *targets_out_dev);

int64_t mxv_sac_workspace_bytes(int64_t M);

int mxv_sac_loss(void *stream, int64_t M, int32_t C, const float *q_dev, int64_t q_ld, const float *targets_dev, const float *reward_dev,
                 const uint8_t *terminated_dev, const float *next_q_dev, int64_t next_q_ld, const float *next_log_prob_dev, double alpha,
                 const float *alpha_dev, double gamma, const float *discount_dev, double delta, const float *weights_dev, void *workspace_dev,
                 int64_t workspace_bytes, float *td_error_dev, float *loss_out_dev, float *stats_out_dev);

int mxv_sac_loss_backward(void *stream, int64_t M, int32_t C, const float *q_dev, int64_t q_ld, const float *targets_dev,
                          const float *reward_dev, const uint8_t *terminated_dev, const float *next_q_dev, int64_t next_q_ld,
                          const float *next_log_prob_dev, double alpha, const float *alpha_dev, double gamma, const float *discount_dev,
                          double delta, const float *weights_dev, const float *grad_loss_dev, float *grad_q_dev);

int mxv_sac_policy_loss(void *stream, int64_t M, int32_t C, const float *log_prob_dev, const float *q_dev, int64_t q_ld, double alpha,
                        const float *alpha_dev, const float *weights_dev, void *workspace_dev, int64_t workspace_bytes, float *loss_out_dev,
                        float *stats_out_dev);

int mxv_sac_policy_loss_backward(void *stream, int64_t M, int32_t C, const float *log_prob_dev, const float *q_dev, int64_t q_ld, double alpha,
                                 const float *alpha_dev, const float *weights_dev, const float *grad_loss_dev, float *grad_log_prob_dev,
                                 float *grad_q_dev);

/* The message of the calling thread's last failed call of this header ("" before the first). */
const char *mxv_sac_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MXV_SAC_H */
