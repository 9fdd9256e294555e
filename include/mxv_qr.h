/* mxv_qr.h — OPTIONAL learner-side pass: the quantile-regression (QR-DQN; Dabney, Rowland, Bellemare, Munos 2018) Q-learning loss of a
 * batch of M rows of A actions with N quantiles each — the target quantiles (given, or the bootstrap of DQN / double DQN with a scalar
 * gamma or a per-row discount, which is what the n-step replay rings emit), the quantile Huber loss of the taken action's quantiles
 * against them, its diagnostics and its gradient with respect to the quantiles — and the expected action values of such a head (must be
 * included by itself, mxv.h does not include it).  The third value-based loss beside the scalar Q-learning loss header and the
 * categorical (51-atom) loss header; unlike the latter it needs no support bounds.
 * Part of the C ABI of libmxv.so (see mxv.h for the status codes).  Handle-free: every call takes the HIP stream it runs on.
 *
 * The rule (tests/qr_host.py).  All arithmetic is IEEE float64, one rounding per operation, no FMA, in the order
 * written.  float32 inputs are widened exactly.  float32() rounds to nearest even.  Every NaN written is the one pattern 0x7FC00000.
 * Everything is a select.
 *
 * ATOMSUM(v): 64 slots, slots k >= N holding +0.0, summed as the pairwise tree s[k] <- s[2k] + s[2k+1] six times (the xor butterfly over
 * lane bits 0..5 of the loss trees: one wave computes it with lane = quantile).  It is the ATOMSUM of the categorical loss header.
 *
 * The head:  Nf = (double)N;   tau_k = (double)(2k + 1) / (double)(2N),   k = 0 .. N-1;   kappa finite and > 0.
 *
 * Per row i, with a_i the stored action, Mf = (double)M:
 *   ok   = 0 <= a_i < A                          (the action indexes the row only after this test; a bad one reads action 0 and is replaced)
 *   th_k = quantiles[i, ok ? a_i : 0, k]
 *   qa   = ATOMSUM(th) / Nf
 *   given mode:      T_j = target_quantiles[i, j]
 *   bootstrap mode:  sel = next_quantiles_online ? next_quantiles_online[i] : next_quantiles[i]
 *                    Q_a = ATOMSUM(sel[a, :]) / Nf,   a = 0 .. A-1
 *                    j* = 0; best = Q_0; for a = 1 .. A-1: if Q_a > best: best = Q_a, j* = a      (strict >: the first maximum wins)
 *                    selbad = any Q_a is NaN
 *                    g = discount ? (double)discount[i] : gamma
 *                    nv_j = selbad ? NaN : next_quantiles[i, j*, j]
 *                    T_j = terminated[i] ? reward[i] : reward[i] + g * nv_j
 *                    (a select: a terminated row ignores both next tensors and the discount entirely, NaN or not)
 *   y    = ATOMSUM(T) / Nf
 *   ae   = |qa - y|
 *   lane k: s_k = +0.0; d_k = +0.0; for j = 0 .. N-1 in ascending order:
 *     u = T_j - th_k;   au = |u|
 *     h = au <= kappa ? 0.5 * (u * u) : kappa * (au - 0.5 * kappa)          (a NaN u falls through to NaN)
 *     dh = au <= kappa ? u : (u < 0 ? -kappa : kappa)                       (dh is NaN if u is NaN)
 *     wg = u < 0 ? 1 - tau_k : tau_k
 *     s_k = s_k + wg * (h / kappa)
 *     d_k = d_k + wg * (dh / kappa)
 *   ql   = ATOMSUM(s) / Nf                        (the paper's form: a sum over the head's quantiles of the mean over the target's)
 *   cr   = N > 1 ? ATOMSUM(k + 1 < N && th_{k+1} < th_k ? 1 : 0) / (double)(N - 1) : 0
 *          (the share of adjacent quantile pairs out of order: it tells a head that has not learned its ordering)
 *   qa, ae, cr and ql are NaN if not ok
 *   term = weights ? weights[i] * ql : ql        (an absent weight is a factor left out, not a factor of 1)
 *   row_loss[i] = float32(ql);   targets_out[i, j] = float32(T_j)      (when asked for)
 * Five sums over the rows — of term, qa, y, ae, cr — and three extrema — the maximum of ql, the minimum and the maximum of qa — by
 * selects that skip a NaN; the extrema start at -Inf, +Inf and -Inf, which is what is written when no row has a value.  A zero
 * extremum is written as +0.0 (the finish adds +0.0).
 *
 * Order of additions over the rows: that of the clipped-surrogate, the scalar Q-learning and the categorical loss headers, exactly.  A
 * leaf is 1024 consecutive rows: lane t of 256 accumulates rows t, t + 256, t + 512, t + 768 of the leaf in that order from +0.0 (rows
 * past M are skipped), then the xor butterfly over lane bits 0..5 of each wave of 64 lanes, then the four waves as (w0 + w1) + (w2 + w3).
 * Leaves are combined in levels of groups of 1024: lane t of 256 takes leaves 4 t .. 4 t + 3 of its group as (a0 + a1) + (a2 + a3), a
 * missing leaf counting +0.0, then the butterfly and the four waves as before; levels repeat until one group is left, and there is at
 * least one.  The extrema follow the same tree with the select in place of the addition.  No float atomic anywhere: the sums are
 * functions of the inputs and their positions.  One launch computes the rows, one the leaves, one each level: a batch of one leaf is
 * finished by the launch of the leaves (the level it would pass through only adds +0.0), so 2 launches up to 1024 rows, 3 up to 2^20,
 * 4 up to 2^30.  The last launch finishes:
 *   loss_out  = float32(sum_term / Mf)
 *   stats_out = float32 of (sum_term / Mf, sum_qa / Mf, sum_y / Mf, sum_ae / Mf, sum_cr / Mf, max_ql + 0.0, min_qa + 0.0, max_qa + 0.0)
 *
 * Backward — mxv_qr_loss_backward.  Recomputes every row (nothing is saved by the forward).  g_loss = the float32 at grad_loss_dev,
 * widened; gs = g_loss / Mf:
 *   grad_quantiles[i, a_i, k] = float32(gs * (weights ? weights[i] * (-(d_k / Nf)) : -(d_k / Nf)))
 *   grad_quantiles[i, a, k]   = +0.0 for every other action a
 *   a row whose action is outside 0..A-1 gets NaN in all A * N elements (its loss is NaN; its gradient must not be silently zero)
 * Every element of grad_quantiles is written.
 *
 * mxv_qr_q_values: q_out[i, a] = float32(ATOMSUM(quantiles[i, a, :]) / Nf): the lines of Q_a above, so the greedy action taken from it
 * is the j* the loss selects.
 *
 * Layout.  quantiles, next_quantiles and next_quantiles_online are float32 [M, A, N], the last two dims contiguous, rows quantiles_ld,
 * next_quantiles_ld, next_quantiles_online_ld floats apart (each at least A * N); 1 <= A <= 64, 1 <= N <= 64 (more quantiles than a
 * wave has lanes are out of scope).  actions is int32 or int64 [M] (action_bytes = 4 or 8); target_quantiles and targets_out are
 * float32 [M, N]; reward, discount, weights and row_loss are float32 [M]; terminated is uint8 [M] (nonzero = set); grad_quantiles is
 * float32 [M, A, N] and q_out float32 [M, A], contiguous.  Exactly one target mode: target_quantiles, or all of reward, terminated and
 * next_quantiles; next_quantiles_online (double DQN: the online network chooses, the target network evaluates) and discount only with
 * the latter.  discount is the per-row gamma^(steps taken) of an n-step ring; with it gamma is not read (it must still be finite).  A
 * truncated step is not an argument: the caller evaluates next_quantiles on the final observation there.  discount, weights, row_loss
 * and targets_out may be NULL.  loss_out is one float32, stats_out float32 [8], grad_loss_dev one float32, all in device memory.
 * workspace is device memory of at least mxv_qr_workspace_bytes(M) bytes on an 8-byte boundary, for the rows' scalars and the leaves'
 * partial sums; its contents mean nothing between calls.
 *
 * Stream-ordered on `stream` (a hipStream_t; NULL = the null stream) of the current device: no synchronisation, no allocation —
 * recordable into a caller's hipGraph.  Every call returns MXV_ERR_INVALID_ARG (message: mxv_qr_last_error), before the device is
 * touched, for: a NULL required pointer; M < 1 or M beyond 2^40; A outside 1..64; N outside 1..64; a kappa that is not finite and > 0;
 * a row stride below A * N or M * ld beyond 2^40; action_bytes other than 4 or 8; both target modes, neither, or a bootstrap mode
 * without all three of its inputs; next_quantiles_online or discount with target_quantiles; a non-finite gamma; a workspace that is too
 * small or off an 8-byte boundary; a pointer off its element's boundary; a range that would wrap past the top of the address space;
 * an output (row_loss, targets_out, loss_out, stats_out, grad_quantiles, q_out) or the workspace sharing a byte with an input or with
 * another output.  A failed launch returns MXV_ERR_HIP.  mxv_qr_workspace_bytes returns 0 for an M outside 1..2^40. */
#ifndef MXV_QR_H
#define MXV_QR_H

#include "mxv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* indices into stats_out */
#define MXV_QR_LOSS_TERM 0
#define MXV_QR_Q_TAKEN_MEAN 1
#define MXV_QR_TARGET_MEAN 2
#define MXV_QR_TD_ABS_MEAN 3
#define MXV_QR_CROSSING_FRACTION 4
#define MXV_QR_ROW_LOSS_MAX 5
#define MXV_QR_Q_TAKEN_MIN 6
#define MXV_QR_Q_TAKEN_MAX 7
#define MXV_QR_STATS 8

int64_t mxv_qr_workspace_bytes(int64_t M);

int mxv_qr_loss(void *stream, int64_t M, int32_t A, int32_t N, const float *quantiles_dev, int64_t quantiles_ld, const void *actions_dev,
                int32_t action_bytes, const float *target_quantiles_dev, const float *reward_dev, const uint8_t *terminated_dev,
                const float *next_quantiles_dev, int64_t next_quantiles_ld, const float *next_quantiles_online_dev,
                int64_t next_quantiles_online_ld, double gamma, const float *discount_dev, double kappa, const float *weights_dev,
                void *workspace_dev, int64_t workspace_bytes, float *row_loss_dev, float *targets_out_dev, float *loss_out_dev,
                float *stats_out_dev);

int mxv_qr_loss_backward(void *stream, int64_t M, int32_t A, int32_t N, const float *quantiles_dev, int64_t quantiles_ld,
                         const void *actions_dev, int32_t action_bytes, const float *target_quantiles_dev, const float *reward_dev,
                         const uint8_t *terminated_dev, const float *next_quantiles_dev, int64_t next_quantiles_ld,
                         const float *next_quantiles_online_dev, int64_t next_quantiles_online_ld, double gamma, const float *discount_dev,
                         double kappa, const float *weights_dev, const float *grad_loss_dev, float *grad_quantiles_dev);

int mxv_qr_q_values(void *stream, int64_t M, int32_t A, int32_t N, const float *quantiles_dev, int64_t quantiles_ld, float *q_out_dev);

/* The message of the calling thread's last failed call of this header ("" before the first). */
const char *mxv_qr_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MXV_QR_H */
