/* mxv_nstep.h — OPTIONAL learner-side pass: n-step returns for the replay ring — a fused insert of a [K, N] rollout chunk that walks
 * each row's window of up to n steps inside the kernel and stores the discounted return, the window's last observation and flag and a
 * per-row discount, and the gather of that discount for a drawn batch (must be included by itself, mxv.h does not include it).  What a
 * multi-step Q-learning target needs between a rollout and the loss:  target = reward + discount * (1 - terminated) * max_a Q(next_obs, a).
 * Part of the C ABI of libmxv.so (see mxv.h for the status codes).  Handle-free: every call takes the HIP stream it runs on.
 *
 * The rule (tests/nstep_host.py).  The ring is the replay ring's five device arrays of capacity C, contiguous — ring_obs
 * and ring_next [C, W] dwords (rows W dwords apart), ring_action [C] dwords, ring_reward float32 [C], ring_term uint8 [C] — and a sixth,
 * ring_discount float32 [C].  1 <= W <= 65536, 1 <= C <= 2^31, C * W <= 2^40.  An observation row is W raw dwords that are copied and
 * never interpreted.  The return is accumulated in float64, every operation rounded once (no fused multiply-add).
 *
 * Insert — mxv_nstep_insert stores a [K, N] chunk, R = K * N <= C rows, with 1 <= n <= MXV_NSTEP_MAX and a finite 0 <= gamma <= 1.
 * Row r = t * N + i:
 *   done[u]  = terminated[u, i] != 0 || (truncated && truncated[u, i] != 0)
 *   G = float64(reward[t, i]);  g = 1;  e = t
 *   while e - t + 1 < n  and  e + 1 < K  and  not done[e]:
 *       e = e + 1;  g = g * gamma;  G = G + g * float64(reward[e, i])
 *   s    = (c + r) mod C                      c = state_dev ? state_dev[0] : count      (rows ever inserted, uint64; 64-bit arithmetic)
 *   pre  = t == 0 ? first_obs[i, :] : obs[t-1, i, :]                                    (the observation the action of step t was taken FROM)
 *   nxt  = (done[e] && final_obs) ? final_obs[e, i, :] : obs[e, i, :]                   (a select of the SOURCE ROW)
 *   ring_obs[s, :] = pre;  ring_next[s, :] = nxt
 *   ring_action[s]   = the low 32 bits of actions[t, i]   (action_bytes 4: int32 or float32 copied as bits; 8: int64)
 *   ring_reward[s]   = float32(G)             NaN -> 0x7FC00000                         (rounded to nearest even)
 *   ring_term[s]     = terminated[e, i] != 0 ? 1 : 0
 *   ring_discount[s] = float32(g * gamma)     = gamma^(e - t + 1); exactly gamma when the window is one step
 *   state_dev[0] += R                         (enqueued behind the kernel when state_dev is given: one launch, or two with state_dev)
 * The window ends at whichever comes first: n steps, an episode end, or the end of the chunk.  A window cut by the chunk end is a correct
 * transition of a shorter horizon — its discount says so — so nothing is carried from one call to the next.  The walk stops by a branch
 * at done[e]: a reward of a later episode, NaN or infinite, is never read into G, and a product with a zero flag never stands in for the
 * cut.  With n == 1 every ring but ring_discount receives exactly what the one-step insert of the replay ring writes, for float64
 * rewards, for float32 rewards that are not NaN and for the NaN 0x7FC00000 (another float32 NaN is stored as that one).  Slots outside
 * the R written ones are not touched.
 *
 * Gather — mxv_nstep_gather reads the discounts of a drawn batch, one launch behind either sampler of the ring.  Row j, k = indices[j]:
 *   discount_out[j] = ring_discount[k]        for 0 <= k < C
 *   discount_out[j] = 0                       for k == -1          (what the samplers write for an empty ring)
 *   discount_out[j] = NaN (0x7FC00000)        for any other k
 *
 * Layout.  first_obs is [N, W] dwords, obs [K, N, W] = [R, W] and final_obs [R, W], with rows first_obs_ld, obs_ld, final_obs_ld dwords
 * apart (each at least W; an ld of an absent array is ignored); actions is [R] of action_bytes, reward [R] of reward_bytes (4: float32,
 * 8: float64), terminated and truncated uint8 [R] (nonzero = set).  final_obs and truncated may be NULL, truncated only together with
 * final_obs: a truncated step without final_obs would silently store the observation after the reset.  indices is int64 [B] and
 * discount_out float32 [B], contiguous.  state_dev is uint64 [2] in device memory on an 8-byte boundary — { rows ever inserted, sample
 * steps taken }, the ring's own counters — or NULL.
 *
 * Stream-ordered on `stream` (a hipStream_t; NULL = the null stream) of the current device: no synchronisation, no allocation —
 * recordable into a caller's hipGraph.  Every call returns MXV_ERR_INVALID_ARG (message: mxv_nstep_last_error), before the device is
 * touched, for: a NULL required pointer; C outside 1..2^31, W outside 1..65536 or C * W beyond 2^40; K, N or B below 1, B beyond 2^40;
 * K * N above C (two rows of one launch would share a slot); n outside 1..MXV_NSTEP_MAX; gamma NaN, below 0 or above 1; a row stride
 * below W or rows * ld beyond 2^40; action_bytes or reward_bytes other than 4 or 8; truncated without final_obs; count above 2^63; a
 * pointer off its element's boundary (dwords: 4, indices and state_dev: 8); a range that would wrap past the top of the address space;
 * an output (for insert the six ring arrays, for gather discount_out) sharing a byte with an input, with state_dev or with another
 * output.  A failed launch returns MXV_ERR_HIP. */
#ifndef MXV_NSTEP_H
#define MXV_NSTEP_H

#include "mxv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MXV_NSTEP_MAX 64 /* steps of a window at most */

int mxv_nstep_insert(void *stream, int64_t C, int32_t W, int64_t K, int64_t N, const void *first_obs_dev, int64_t first_obs_ld,
                     const void *obs_dev, int64_t obs_ld, const void *final_obs_dev, int64_t final_obs_ld, const void *actions_dev,
                     int32_t action_bytes, const void *reward_dev, int32_t reward_bytes, const uint8_t *terminated_dev,
                     const uint8_t *truncated_dev, uint64_t count, uint64_t *state_dev, void *ring_obs_dev, void *ring_next_dev,
                     void *ring_action_dev, float *ring_reward_dev, uint8_t *ring_term_dev, int32_t n, double gamma,
                     float *ring_discount_dev);

int mxv_nstep_gather(void *stream, int64_t C, int64_t B, const float *ring_discount_dev, const int64_t *indices_dev,
                     float *discount_out_dev);

/* The message of the calling thread's last failed call of this header ("" before the first). */
const char *mxv_nstep_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MXV_NSTEP_H */
