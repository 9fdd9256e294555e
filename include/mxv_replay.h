/* mxv_replay.h — OPTIONAL learner-side pass: a uniform replay buffer on the device — a ring of C transitions that the caller owns, a
 * fused insert of a [K, N] rollout chunk and a Philox-keyed uniform draw with its gather (must be included by itself, mxv.h does not
 * include it).  What lies between a rollout and the Q-learning loss of a batch.
 * Part of the C ABI of libmxv.so (see mxv.h for the status codes).  Handle-free: every call takes the HIP stream it runs on.
 *
 * The rule (tests/replay_host.py).  Pure data movement and integer arithmetic: the only floating-point operation is the
 * conversion of a float64 reward.  An observation row is W raw dwords that are copied and never interpreted.
 *
 * The ring is five device arrays of capacity C, contiguous: ring_obs and ring_next [C, W] dwords (rows W dwords apart), ring_action
 * [C] dwords, ring_reward float32 [C], ring_term uint8 [C].  1 <= W <= 65536, 1 <= C <= 2^31, C * W <= 2^40.
 *
 * Insert — mxv_replay_insert stores a [K, N] chunk, R = K * N <= C rows.  Row r = t * N + i:
 *   c    = state_dev ? state_dev[0] : count          (rows ever inserted, uint64)
 *   s    = (c + r) mod C                             (64-bit arithmetic)
 *   pre  = t == 0 ? first_obs[i, :] : obs[t-1, i, :] (the observation the action of step t was taken FROM)
 *   done = terminated[r] != 0 || (truncated && truncated[r] != 0)
 *   nxt  = (done && final_obs) ? final_obs[r, :] : obs[r, :]      (a select of the SOURCE ROW: the other row's dwords are not copied;
 *                                                                  final_obs rows of steps that did not end may hold anything)
 *   ring_obs[s, :] = pre;  ring_next[s, :] = nxt
 *   ring_action[s] = the low 32 bits of actions[r]   (action_bytes 4: int32 or float32 copied as bits; 8: int64)
 *   ring_reward[s] = float32(reward[r])              (reward_bytes 4: the float32 copied as bits; 8: the float64 rounded to nearest
 *                                                     even, NaN -> 0x7FC00000)
 *   ring_term[s]   = terminated[r] != 0 ? 1 : 0
 * Because nxt is the final observation at a truncated step, the stored flag alone is what a one-step bootstrap needs.  K = 1 with
 * first_obs = the observations before the step, obs = those after it and neither final_obs nor truncated is the flat
 * add(obs, action, reward, terminated, next_obs) of an ordinary buffer.  With state_dev the call enqueues state_dev[0] += R behind the
 * kernel: one launch, or two with state_dev.  Slots outside the R written ones are not touched.
 *
 * Sample — mxv_replay_sample draws B rows uniformly, with replacement, from the live part of the ring and gathers them.  Row j:
 *   c = state_dev ? state_dev[0] : count;   t = state_dev ? state_dev[1] : step;   n = min(c, C)
 *   w = word [j & 3] of Philox4x32-10(key = seed, ctr = (g_lo, g_hi, t_lo, (t_hi & 0x0fffffff) | 9 << 28)),  g = j >> 2
 *   k = (uint64(w) * n) >> 32                        (integer multiply-high: 0 <= k < n, no float, no modulo)
 *   indices[j] = k;   obs_out[j, :] = ring_obs[k, :];  next_out[j, :] = ring_next[k, :];  reward_out[j] = ring_reward[k];
 *   term_out[j] = ring_term[k];  action_out[j] = ring_action[k]   (action_bytes 4: the dword; 8: the dword as int32, sign-extended to int64)
 *   n == 0:  indices[j] = -1 and every other output dword / byte of row j is 0  (no error: under graph replay the host cannot know)
 * Row j at sample step t depends on (seed, j, t, n) alone, not on B.  Slot probabilities are floor-counts / 2^32: they differ by at most
 * 2^-32.  With state_dev the call enqueues state_dev[1] += 1 behind the kernel.  indices is what a later prioritised variant updates.
 *
 * Layout.  first_obs is [N, W] dwords, obs [K, N, W] = [R, W] and final_obs [R, W], with rows first_obs_ld, obs_ld, final_obs_ld dwords
 * apart (each at least W; an ld of an absent array is ignored); actions is [R] of action_bytes, reward [R] of reward_bytes, terminated
 * and truncated uint8 [R] (nonzero = set).  final_obs and truncated may be NULL, truncated only together with final_obs: a truncated
 * step without final_obs would silently store the observation after the reset.  The outputs of a sample are contiguous: indices int64
 * [B], obs_out and next_out [B, W] dwords, action_out [B] of action_bytes, reward_out float32 [B], term_out uint8 [B]; none may be
 * NULL.  state_dev is uint64 [2] in device memory on an 8-byte boundary — { rows ever inserted, sample steps taken } — or NULL.
 *
 * Stream-ordered on `stream` (a hipStream_t; NULL = the null stream) of the current device: no synchronisation, no allocation —
 * recordable into a caller's hipGraph.  Every call returns MXV_ERR_INVALID_ARG (message: mxv_replay_last_error), before the device is
 * touched, for: a NULL required pointer; C outside 1..2^31, W outside 1..65536 or C * W beyond 2^40; K, N or B below 1, B * W beyond
 * 2^40; K * N above C (two rows of one launch would share a slot); a row stride below W or rows * ld beyond 2^40; action_bytes or
 * reward_bytes other than 4 or 8; truncated without final_obs; count above 2^63; a pointer off its element's boundary (dwords: 4,
 * state_dev: 8); a range that would wrap past the top of the address space; an output (for insert the five ring arrays, for sample the
 * six outputs) sharing a byte with an input, with state_dev or with another output.  A failed launch returns MXV_ERR_HIP. */
#ifndef MXV_REPLAY_H
#define MXV_REPLAY_H

#include "mxv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MXV_REPLAY_MAX_WIDTH 65536          /* dwords of an observation row */
#define MXV_REPLAY_MAX_CAPACITY (1LL << 31) /* rows of a ring */
#define MXV_REPLAY_STREAM_TAG 9             /* ctr[3] >> 28 of the index draws */

int mxv_replay_insert(void *stream, int64_t C, int32_t W, int64_t K, int64_t N, const void *first_obs_dev, int64_t first_obs_ld,
                      const void *obs_dev, int64_t obs_ld, const void *final_obs_dev, int64_t final_obs_ld, const void *actions_dev,
                      int32_t action_bytes, const void *reward_dev, int32_t reward_bytes, const uint8_t *terminated_dev,
                      const uint8_t *truncated_dev, uint64_t count, uint64_t *state_dev, void *ring_obs_dev, void *ring_next_dev,
                      void *ring_action_dev, float *ring_reward_dev, uint8_t *ring_term_dev);

int mxv_replay_sample(void *stream, int64_t C, int32_t W, int64_t B, const void *ring_obs_dev, const void *ring_next_dev,
                      const void *ring_action_dev, const float *ring_reward_dev, const uint8_t *ring_term_dev, uint64_t seed, uint64_t count,
                      uint64_t step, uint64_t *state_dev, int64_t *indices_dev, void *obs_out_dev, void *next_out_dev, void *action_out_dev,
                      int32_t action_bytes, float *reward_out_dev, uint8_t *term_out_dev);

/* The message of the calling thread's last failed call of this header ("" before the first). */
const char *mxv_replay_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MXV_REPLAY_H */
