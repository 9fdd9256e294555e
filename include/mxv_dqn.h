/* mxv_dqn.h — OPTIONAL learner-side pass: the Q-learning loss of a batch of M rows of A action values — TD targets (given, or the one-step
 * bootstrap of DQN / double DQN), the Huber loss of the TD errors, its diagnostics and its gradient with respect to q (must be included
 * by itself, mxv.h does not include it).  The value-based counterpart of the PPO loss header; Peng's Q(lambda) targets over a [K, N] chunk are the
 * `returns` of mxv_gae.h called with values = max_a Q.
 * Part of the C ABI of libmxv.so (see mxv.h for the status codes).  Handle-free: every call takes the HIP stream it runs on.
 *
 * The rule (tests/dqn_host.py).  All arithmetic is IEEE float64, one rounding per operation, no FMA, in the order
 * written.  float32 inputs are widened exactly.  float32() rounds to nearest even.  Every NaN written is the one pattern 0x7FC00000.
 *
 * Per row i, with a_i the stored action, Mf = (double)M:
 *   ok   = 0 <= a_i < A                          (the action indexes the row only after this test; a bad one reads nothing of its own)
 *   qa   = ok ? q[i, a_i] : NaN
 *   targets mode:    y = targets[i]
 *   bootstrap mode:  sel = next_q_online ? next_q_online[i, :] : next_q[i, :]
 *                    j* = 0; best = sel[0]; for a = 1 .. A-1: if sel[a] > best: best = sel[a], j* = a     (strict >: the first maximum wins)
 *                    bad = any sel[a] is NaN
 *                    nv  = bad ? NaN : next_q[i, j*]
 *                    y   = terminated[i] ? reward[i] : reward[i] + gamma * nv      (a select: a terminated row ignores next_q entirely)
 *   e    = qa - y;   ae = |e|
 *   h    = ae <= delta ? 0.5 * (e * e) : delta * (ae - 0.5 * delta);   h = NaN if e is NaN
 *   term = weights ? weights[i] * h : h          (an absent weight is a factor left out, not a factor of 1)
 *   dh   = ae <= delta ? e : (e < 0 ? -delta : delta);   dh = NaN if e is NaN      (the inclusive edge: ae == delta is quadratic)
 *   lin  = ae > delta ? 1.0 : 0.0
 *   td_error[i] = float32(e)                     (when asked for)
 * Five sums over the rows — of term, ae, qa, y, lin — and three extrema — the maximum of ae, the minimum and the maximum of qa — by
 * selects that skip a NaN; the extrema start at -Inf, +Inf and -Inf, which is what is written when no row has a value.  A zero
 * extremum is written as +0.0 (the finish adds +0.0).
 *
 * Order of additions: that of the PPO loss header, exactly.  A leaf is 1024 consecutive rows: lane t of 256 accumulates rows t, t + 256, t + 512,
 * t + 768 of the leaf in that order from +0.0 (rows past M are skipped), then the xor butterfly over lane bits 0..5 of each wave of 64
 * lanes (stage b: every lane adds the value of lane ^ (1 << b)), then the four waves as (w0 + w1) + (w2 + w3).  Leaves are combined in
 * levels of groups of 1024: lane t of 256 takes leaves 4 t .. 4 t + 3 of its group as (a0 + a1) + (a2 + a3), a missing leaf counting
 * +0.0, then the butterfly and the four waves as before; levels repeat until one group is left, and there is at least one.  The extrema
 * follow the same tree with the select in place of the addition.  No float atomic anywhere: the sums are functions of the inputs and
 * their positions.  2 launches up to 2^20 rows, 3 up to 2^30, 4 beyond.  The last launch also finishes:
 *   loss_out  = float32(sum_term / Mf)
 *   stats_out = float32 of (sum_term / Mf, sum_ae / Mf, sum_qa / Mf, sum_y / Mf, sum_lin / Mf, max_ae + 0.0, min_qa + 0.0, max_qa + 0.0)
 *
 * Backward — mxv_dqn_loss_backward.  Recomputes every row (nothing is saved by the forward).  g = the float32 at grad_loss_dev,
 * widened; gs = g / Mf:
 *   grad_q[i, a_i] = float32(gs * (weights ? weights[i] * dh : dh))
 *   grad_q[i, a]   = +0.0 for every other column a
 *   a row whose action is outside 0..A-1 gets NaN in all A columns (its loss is NaN; its gradient must not be silently zero)
 * Every element of grad_q is written.
 *
 * Layout.  q, next_q and next_q_online are float32 [M, A] with rows q_ld, next_q_ld, next_q_online_ld floats apart (each at least A);
 * actions is int32 or int64 [M] (action_bytes = 4 or 8); targets, reward, weights and td_error are float32 [M]; terminated is uint8 [M]
 * (nonzero = set); grad_q is float32 [M, A], contiguous.  Exactly one target mode: targets, or all of reward, terminated and next_q;
 * next_q_online (double DQN: the online network chooses, the target network evaluates) only with the latter.  A truncated step is not
 * an argument: the caller evaluates next_q on the final observation there.  weights and td_error may be NULL.  loss_out is one float32,
 * stats_out float32 [8], grad_loss_dev one float32, all in device memory.  workspace is device memory of at least
 * mxv_dqn_workspace_bytes(M) bytes on an 8-byte boundary, for the leaves' partial sums; its contents mean nothing between calls.
 *
 * Stream-ordered on `stream` (a hipStream_t; NULL = the null stream) of the current device: no synchronisation, no allocation —
 * recordable into a caller's hipGraph.  Every call returns MXV_ERR_INVALID_ARG (message: mxv_dqn_last_error), before the device is
 * touched, for: a NULL required pointer; M < 1 or M beyond 2^40; A outside 1..64; a row stride below A or M * ld beyond 2^40;
 * action_bytes other than 4 or 8; both target modes, neither, or a bootstrap mode without all three of its inputs; next_q_online with
 * targets; a non-finite gamma; a delta that is NaN or not above 0 (+Inf is the plain half squared error); a workspace that is too
 * small or off an 8-byte boundary; a pointer off its element's boundary; a range that would wrap past the top of the address space;
 * an output (td_error, loss_out, stats_out, grad_q) or the workspace sharing a byte with an input or with another output.  A failed
 * launch returns MXV_ERR_HIP.  mxv_dqn_workspace_bytes returns 0 for an M outside 1..2^40. */
#ifndef MXV_DQN_H
#define MXV_DQN_H

#include "mxv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* indices into stats_out */
#define MXV_DQN_LOSS_TERM 0
#define MXV_DQN_TD_ABS_MEAN 1
#define MXV_DQN_Q_TAKEN_MEAN 2
#define MXV_DQN_TARGET_MEAN 3
#define MXV_DQN_LINEAR_FRACTION 4
#define MXV_DQN_TD_ABS_MAX 5
#define MXV_DQN_Q_TAKEN_MIN 6
#define MXV_DQN_Q_TAKEN_MAX 7
#define MXV_DQN_STATS 8

int64_t mxv_dqn_workspace_bytes(int64_t M);

int mxv_dqn_loss(void *stream, int64_t M, int32_t A, const float *q_dev, int64_t q_ld, const void *actions_dev, int32_t action_bytes,
                 const float *targets_dev, const float *reward_dev, const uint8_t *terminated_dev, const float *next_q_dev, int64_t next_q_ld,
                 const float *next_q_online_dev, int64_t next_q_online_ld, double gamma, double delta, const float *weights_dev,
                 void *workspace_dev, int64_t workspace_bytes, float *td_error_dev, float *loss_out_dev, float *stats_out_dev);

int mxv_dqn_loss_backward(void *stream, int64_t M, int32_t A, const float *q_dev, int64_t q_ld, const void *actions_dev, int32_t action_bytes,
                          const float *targets_dev, const float *reward_dev, const uint8_t *terminated_dev, const float *next_q_dev,
                          int64_t next_q_ld, const float *next_q_online_dev, int64_t next_q_online_ld, double gamma, double delta,
                          const float *weights_dev, const float *grad_loss_dev, float *grad_q_dev);

/* The message of the calling thread's last failed call of this header ("" before the first). */
const char *mxv_dqn_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MXV_DQN_H */
