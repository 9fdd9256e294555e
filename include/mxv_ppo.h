/* mxv_ppo.h — OPTIONAL learner-side pass: the PPO clipped-surrogate loss of a batch of M rows, its diagnostics and its gradients, and the
 * mean and inverse deviation of the advantages it normalises with (must be included by itself, mxv.h does not include it).  The last
 * stage of an update after mxv_gae.h (advantages) and mxv_policy_eval.h (log pi and entropy of the stored actions).
 * Part of the C ABI of libmxv.so (see mxv.h for the status codes).  Handle-free: every call takes the HIP stream it runs on.
 *
 * The rule (tests/ppo_host.py).  All arithmetic is IEEE float64, one rounding per operation, no FMA, in the order
 * written.  float32 inputs are widened exactly.  EXP is the operation sequence of mxv_policy.h on its widened domain |d| <= 80.
 * float32() rounds to nearest even.  Every NaN written is the one pattern 0x7FC00000 (float32) or 0x7FF8000000000000 (float64).
 *
 * Per row i, with lp = log_prob_i, old = old_log_prob_i, adv = advantages_i and, where given, ent = entropy_i, v = values_i,
 * ret = returns_i; (mean, inv) = the two float64 of `moments`; lo = 1.0 - clip and hi = 1.0 + clip, formed once on the host:
 *   a    = moments ? (adv - mean) * inv : adv
 *   d    = lp - old;   d = d < -80 ? -80 : (d > 80 ? 80 : d)          (a NaN d stays NaN; EXP then runs on 0 and r = NaN by select)
 *   r    = EXP(d)
 *   rc   = r < lo ? lo : (r > hi ? hi : r)
 *   s1   = r * a;  s2 = rc * a;  s = s2 < s1 ? s2 : s1;  s = NaN if s1 or s2 is NaN
 *   pass = (r >= lo && r <= hi) || s1 < s2                            (the tie split of a minimum and the inclusive gradient of a clamp, folded)
 *   k1   = -d          k3 = (r - 1.0) - d          cf = (r < lo || r > hi) ? 1.0 : 0.0
 *   err  = v - ret     v2 = err * err
 * Six sums over the rows — of s, v2, ent, k1, k3, cf — and two extrema of r, by selects that skip a NaN r; the extrema start at +Inf
 * and -Inf, which is what is written when no row has a ratio.  The sum of an absent input (entropy; values and returns) is not formed.
 *
 * Order of additions.  A leaf is 1024 consecutive rows: lane t of 256 accumulates rows t, t + 256, t + 512, t + 768 of the leaf in that
 * order from +0.0 (rows past M are skipped), then the xor butterfly over lane bits 0..5 of each wave of 64 lanes (stage b: every lane
 * adds the value of lane ^ (1 << b)), then the four waves as (w0 + w1) + (w2 + w3).  Leaves are combined in levels of groups of 1024:
 * lane t of 256 takes leaves 4 t .. 4 t + 3 of its group as (a0 + a1) + (a2 + a3), a missing leaf counting +0.0, then the butterfly
 * and the four waves as before; levels repeat until one group is left, and there is at least one.  The extrema follow the same tree
 * with the select in place of the addition (a missing leaf counting +Inf or -Inf).  So the sums are functions of the inputs and their
 * positions: 2 launches up to 2^20 rows, 3 up to 2^30, 4 beyond.  The last launch also finishes, with Mf = (double)M:
 *   policy_loss = -(sum_s / Mf)        value_loss = 0.5 * (sum_v2 / Mf)        ent = sum_ent / Mf
 *   loss = (policy_loss + value_coef * value_loss) - entropy_coef * ent        (an absent term is left out, not multiplied by zero)
 *   loss_out  = float32(loss)
 *   stats_out = float32 of (policy_loss, value_loss or 0, ent or 0, sum_k1 / Mf, sum_k3 / Mf, sum_cf / Mf, ratio_min, ratio_max)
 *
 * Advantage moments — mxv_ppo_advantage_moments.  The same tree over x = adv_i and over x * x (exact: the product of two widened
 * float32), giving S and Q; then
 *   mean = S / Mf      var = (Q - S * mean) / (Mf - 1.0)      var = var < 0 ? 0 : var      inv = 1.0 / (sqrt(var) + eps)
 * (`/` and sqrt: IEEE), moments_out = (mean, inv).  M = 1 gives a NaN inv by the arithmetic, as the unbiased deviation of one value is.
 *
 * Backward — mxv_ppo_clip_loss_backward.  Recomputes every row (nothing is saved by the forward).  g = the float32 at grad_loss_dev,
 * widened; gs = g / Mf:
 *   grad_log_prob_i = float32(-(gs * (pass ? a * r : 0.0)))      and NaN where s1 or s2 is NaN
 *   grad_values_i   = float32(gs * (value_coef * err))
 *   grad_entropy_i  = float32(-(gs * entropy_coef))
 * A NULL gradient output is not computed.  The clamp of d at +-80 is treated as the identity.
 *
 * Layout.  log_prob, old_log_prob, advantages, entropy, values, returns and the three gradient outputs are float32 [M], contiguous.
 * entropy may be NULL; values and returns are both given or both NULL; grad_entropy needs entropy, grad_values needs values.  moments is
 * float64 [2] in device memory or NULL (the advantages are used as given): it is read by the kernels, so a call may follow
 * mxv_ppo_advantage_moments on the same stream with no synchronisation in between.  loss_out is one float32, stats_out float32 [8],
 * grad_loss_dev one float32, all in device memory.  workspace is device memory of at least mxv_ppo_workspace_bytes(M) bytes on an 8-byte
 * boundary, for the leaves' partial sums; its contents mean nothing between calls.
 *
 * Stream-ordered on `stream` (a hipStream_t; NULL = the null stream) of the current device: no synchronisation, no allocation —
 * recordable into a caller's hipGraph.  Every call returns MXV_ERR_INVALID_ARG (message: mxv_ppo_last_error), before the device is
 * touched, for: a NULL required pointer; M < 1 or M beyond 2^40; values without returns or the reverse; clip outside [0, 1); a
 * non-finite clip, eps, entropy_coef or value_coef; eps < 0; a workspace that is too small or off an 8-byte boundary; a float32
 * pointer off a 4-byte boundary (moments: 8); a range that would wrap past the top of the address space; an output or the workspace
 * sharing a byte with an input or with another output; all three gradient outputs NULL, or one whose input is absent.  A failed
 * launch returns MXV_ERR_HIP.  mxv_ppo_workspace_bytes returns 0 for an M outside 1..2^40. */
#ifndef MXV_PPO_H
#define MXV_PPO_H

#include "mxv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* indices into stats_out */
#define MXV_PPO_POLICY_LOSS 0
#define MXV_PPO_VALUE_LOSS 1
#define MXV_PPO_ENTROPY 2
#define MXV_PPO_APPROX_KL 3
#define MXV_PPO_APPROX_KL3 4
#define MXV_PPO_CLIP_FRACTION 5
#define MXV_PPO_RATIO_MIN 6
#define MXV_PPO_RATIO_MAX 7
#define MXV_PPO_STATS 8

int64_t mxv_ppo_workspace_bytes(int64_t M);

int mxv_ppo_advantage_moments(void *stream, int64_t M, const float *advantages_dev, double eps, void *workspace_dev, int64_t workspace_bytes,
                              double *moments_out_dev);

int mxv_ppo_clip_loss(void *stream, int64_t M, const float *log_prob_dev, const float *old_log_prob_dev, const float *advantages_dev,
                      const double *moments_dev, const float *entropy_dev, const float *values_dev, const float *returns_dev, double clip,
                      double entropy_coef, double value_coef, void *workspace_dev, int64_t workspace_bytes, float *loss_out_dev,
                      float *stats_out_dev);

int mxv_ppo_clip_loss_backward(void *stream, int64_t M, const float *log_prob_dev, const float *old_log_prob_dev, const float *advantages_dev,
                               const double *moments_dev, const float *entropy_dev, const float *values_dev, const float *returns_dev,
                               double clip, double entropy_coef, double value_coef, const float *grad_loss_dev, float *grad_log_prob_dev,
                               float *grad_entropy_dev, float *grad_values_dev);

/* The message of the calling thread's last failed call of this header ("" before the first). */
const char *mxv_ppo_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MXV_PPO_H */
