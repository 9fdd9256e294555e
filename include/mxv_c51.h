/* mxv_c51.h — OPTIONAL learner-side pass: the categorical (C51; Bellemare, Dabney, Munos 2017) Q-learning loss of a batch of M rows of A
 * actions with Z atoms each — the target distribution (given, or the one-step bootstrap of DQN / double DQN projected onto the support),
 * the cross-entropy of the taken action's distribution against it, its diagnostics and its gradient with respect to the logits — and
 * the expected action values of such a head (must be included by itself, mxv.h does not include it).  The distributional counterpart of
 * the DQN loss header.
 * Part of the C ABI of libmxv.so (see mxv.h for the status codes).  Handle-free: every call takes the HIP stream it runs on.
 *
 * The rule (tests/c51_host.py).  All arithmetic is IEEE float64, one rounding per operation, no FMA, in the order
 * written.  float32 inputs are widened exactly.  float32() rounds to nearest even.  Every NaN written is the one pattern 0x7FC00000.
 * EXP and LOG are the operation sequences of the policy header's rule.  Everything is a select.
 *
 * The support:  dz = (v_max - v_min) / (double)(Z - 1);   z_k = v_min + (double)k * dz,   k = 0 .. Z-1.
 *
 * ATOMSUM(v): 64 slots, slots k >= Z holding +0.0, summed as the pairwise tree s[k] <- s[2k] + s[2k+1] six times (the xor butterfly over
 * lane bits 0..5 of the loss trees: one wave computes it with lane = atom).
 *
 * SOFT(x) of a row of Z logits:
 *   bad = any x_k is NaN or +Inf, or every x_k is -Inf         (a bad row computes on x_k = 0 and its d_k and p_k are replaced by NaN)
 *   mx  = max_k x_k + 0.0
 *   d_k = x_k - mx
 *   e_k = d_k < -708 ? 0 : EXP(d_k)
 *   S   = ATOMSUM(e)
 *   p_k = e_k / S
 *
 * Per row i, with a_i the stored action, Mf = (double)M:
 *   ok   = 0 <= a_i < A                          (the action indexes the row only after this test; a bad one reads action 0 and is replaced)
 *   x    = logits[i, ok ? a_i : 0, :] through SOFT
 *   L    = LOG(S);   lp_k = d_k - L
 *   qa   = ATOMSUM(p_k * z_k)
 *   ent  = L - ATOMSUM(e_k == 0 ? 0 : e_k * d_k) / S
 *   given mode:      m_k = target_probs[i, k];   cm = 0
 *   bootstrap mode:  sel = next_logits_online ? next_logits_online[i] : next_logits[i]
 *                    Q_a = ATOMSUM(p_k * z_k) of SOFT(sel[a, :]),   a = 0 .. A-1
 *                    j* = 0; best = Q_0; for a = 1 .. A-1: if Q_a > best: best = Q_a, j* = a      (strict >: the first maximum wins)
 *                    selbad = any action's row of sel is bad
 *                    tp   = the p of SOFT(next_logits[i, j*, :])
 *                    pn_j = terminated[i] ? (j == 0 ? 1 : 0) : (selbad ? NaN : tp_j)      (a terminated row ignores both next tensors)
 *                    r = reward[i];   per atom j:
 *                      tz_j = terminated[i] ? r : r + gamma * z_j
 *                      c = tz_j < v_min ? v_min : tz_j;   c = c > v_max ? v_max : c       (a NaN stays)
 *                      b_j = (c - v_min) / dz;   b_j = b_j > Z-1 ? Z-1 : b_j
 *                    m_k = +0.0; for j = 0 .. Z-1 in ascending order:
 *                      w = 1 - |b_j - (double)k|;   w = w < 0 ? 0 : w;   m_k = m_k + pn_j * w
 *                    cm = ATOMSUM_j((tz_j < v_min or tz_j > v_max) ? pn_j : 0)
 *   The triangular weight w is the projection without floor / ceil: a b_j exactly on an atom gives that atom the weight 1 and its
 *   neighbours 0, so no mass is lost there.
 *   sm   = ATOMSUM(m_k);   y = ATOMSUM(m_k * z_k)
 *   ce   = -ATOMSUM(m_k == 0 ? 0 : m_k * lp_k)   (a -Inf logit under zero target mass costs nothing; under positive mass ce is +Inf)
 *   qa, ent and ce are NaN if not ok
 *   term = weights ? weights[i] * ce : ce        (an absent weight is a factor left out, not a factor of 1)
 *   row_loss[i] = float32(ce);   projected[i, k] = float32(m_k)      (when asked for)
 * Five sums over the rows — of term, qa, y, ent, cm — and three extrema — the maximum of ce, the minimum and the maximum of qa — by
 * selects that skip a NaN; the extrema start at -Inf, +Inf and -Inf, which is what is written when no row has a value.  A zero
 * extremum is written as +0.0 (the finish adds +0.0).
 *
 * Order of additions over the rows: that of the PPO loss header and the DQN loss header, exactly.  A leaf is 1024 consecutive rows:
 * lane t of 256 accumulates rows t, t + 256, t + 512, t + 768 of the leaf in that order from +0.0 (rows past M are skipped), then the
 * xor butterfly over lane bits 0..5 of each wave of 64 lanes, then the four waves as (w0 + w1) + (w2 + w3).  Leaves are combined in
 * levels of groups of 1024: lane t of 256 takes leaves 4 t .. 4 t + 3 of its group as (a0 + a1) + (a2 + a3), a missing leaf counting
 * +0.0, then the butterfly and the four waves as before; levels repeat until one group is left, and there is at least one.  The extrema
 * follow the same tree with the select in place of the addition.  No float atomic anywhere: the sums are functions of the inputs and
 * their positions.  One launch computes the rows, one the leaves, one each level: a batch of one leaf is finished by the launch of the
 * leaves (the level it would pass through only adds +0.0), so 2 launches up to 1024 rows, 3 up to 2^20, 4 up to 2^30.  The last
 * launch finishes:
 *   loss_out  = float32(sum_term / Mf)
 *   stats_out = float32 of (sum_term / Mf, sum_qa / Mf, sum_y / Mf, sum_ent / Mf, sum_cm / Mf, max_ce + 0.0, min_qa + 0.0, max_qa + 0.0)
 *
 * Backward — mxv_c51_loss_backward.  Recomputes every row (nothing is saved by the forward).  g = the float32 at grad_loss_dev,
 * widened; gs = g / Mf:
 *   grad_logits[i, a_i, k] = float32(gs * (weights ? weights[i] * (p_k * sm - m_k) : (p_k * sm - m_k)))
 *   grad_logits[i, a, k]   = +0.0 for every other action a
 *   a row whose action is outside 0..A-1 gets NaN in all A * Z elements (its loss is NaN; its gradient must not be silently zero)
 * Every element of grad_logits is written.
 *
 * mxv_c51_q_values: q_out[i, a] = float32(ATOMSUM(p_k * z_k)) of SOFT(logits[i, a, :]), NaN where that row is bad: the lines of Q_a
 * above, so the greedy action taken from it is the j* the loss selects.
 *
 * Layout.  logits, next_logits and next_logits_online are float32 [M, A, Z], the last two dims contiguous, rows logits_ld,
 * next_logits_ld, next_logits_online_ld floats apart (each at least A * Z); 1 <= A <= 64, 2 <= Z <= 64 (more atoms than a wave has
 * lanes are out of scope).  actions is int32 or int64 [M] (action_bytes = 4 or 8); target_probs and projected are float32 [M, Z];
 * reward, weights and row_loss are float32 [M]; terminated is uint8 [M] (nonzero = set); grad_logits is float32 [M, A, Z] and q_out
 * float32 [M, A], contiguous.  Exactly one target mode: target_probs, or all of reward, terminated and next_logits;
 * next_logits_online (double DQN: the online network chooses, the target network evaluates) only with the latter.  A truncated step is
 * not an argument: the caller evaluates next_logits on the final observation there.  weights, row_loss and projected may be NULL.
 * loss_out is one float32, stats_out float32 [8], grad_loss_dev one float32, all in device memory.  workspace is device memory of at
 * least mxv_c51_workspace_bytes(M) bytes on an 8-byte boundary, for the rows' scalars and the leaves' partial sums; its contents mean
 * nothing between calls.
 *
 * Stream-ordered on `stream` (a hipStream_t; NULL = the null stream) of the current device: no synchronisation, no allocation —
 * recordable into a caller's hipGraph.  Every call returns MXV_ERR_INVALID_ARG (message: mxv_c51_last_error), before the device is
 * touched, for: a NULL required pointer; M < 1 or M beyond 2^40; A outside 1..64; Z outside 2..64; a non-finite v_min or v_max, or
 * v_min not below v_max; a row stride below A * Z or M * ld beyond 2^40; action_bytes other than 4 or 8; both target modes, neither, or
 * a bootstrap mode without all three of its inputs; next_logits_online with target_probs; a non-finite gamma; a workspace that is too
 * small or off an 8-byte boundary; a pointer off its element's boundary; a range that would wrap past the top of the address space;
 * an output (row_loss, projected, loss_out, stats_out, grad_logits, q_out) or the workspace sharing a byte with an input or with
 * another output.  A failed launch returns MXV_ERR_HIP.  mxv_c51_workspace_bytes returns 0 for an M outside 1..2^40. */
#ifndef MXV_C51_H
#define MXV_C51_H

#include "mxv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* indices into stats_out */
#define MXV_C51_LOSS_TERM 0
#define MXV_C51_Q_TAKEN_MEAN 1
#define MXV_C51_TARGET_MEAN 2
#define MXV_C51_ENTROPY_MEAN 3
#define MXV_C51_CLIPPED_MASS_MEAN 4
#define MXV_C51_ROW_LOSS_MAX 5
#define MXV_C51_Q_TAKEN_MIN 6
#define MXV_C51_Q_TAKEN_MAX 7
#define MXV_C51_STATS 8

int64_t mxv_c51_workspace_bytes(int64_t M);

int mxv_c51_loss(void *stream, int64_t M, int32_t A, int32_t Z, const float *logits_dev, int64_t logits_ld, const void *actions_dev,
                 int32_t action_bytes, const float *target_probs_dev, const float *reward_dev, const uint8_t *terminated_dev,
                 const float *next_logits_dev, int64_t next_logits_ld, const float *next_logits_online_dev, int64_t next_logits_online_ld,
                 double gamma, double v_min, double v_max, const float *weights_dev, void *workspace_dev, int64_t workspace_bytes,
                 float *row_loss_dev, float *projected_dev, float *loss_out_dev, float *stats_out_dev);

int mxv_c51_loss_backward(void *stream, int64_t M, int32_t A, int32_t Z, const float *logits_dev, int64_t logits_ld, const void *actions_dev,
                          int32_t action_bytes, const float *target_probs_dev, const float *reward_dev, const uint8_t *terminated_dev,
                          const float *next_logits_dev, int64_t next_logits_ld, const float *next_logits_online_dev,
                          int64_t next_logits_online_ld, double gamma, double v_min, double v_max, const float *weights_dev,
                          const float *grad_loss_dev, float *grad_logits_dev);

int mxv_c51_q_values(void *stream, int64_t M, int32_t A, int32_t Z, const float *logits_dev, int64_t logits_ld, double v_min, double v_max,
                     float *q_out_dev);

/* The message of the calling thread's last failed call of this header ("" before the first). */
const char *mxv_c51_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MXV_C51_H */
