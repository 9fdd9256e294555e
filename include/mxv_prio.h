/* mxv_prio.h — OPTIONAL learner-side pass: prioritised experience replay (Schaul et al. 2016) on the device — an exact integer sum tree
 * over the slots of a replay ring, its insert and update, and a Philox-keyed proportional draw with the gather and the importance
 * weights (must be included by itself: mxv.h does not include it, and it does not include mxv_replay.h).
 * Part of the C ABI of libmxv.so (see mxv.h for the status codes).  Handle-free: every call takes the HIP stream it runs on.
 *
 * The rule (tests/prio_host.py).  Priorities are fixed-point integers: a leaf is a uint32, every inner node a uint64 sum.
 * Integer sums are exact and commute, so the tree has the same bits whatever order the device's integer atomic adds arrive in; there is
 * no float atomic anywhere.  The only floating-point arithmetic is the quantisation of a TD error and the importance weight, in float64
 * with the written-out LOG and EXP of the policy heads (mxv_policy.h), one rounding per operation.
 *
 * Layout.  All tree memory is caller-owned, zero-initialised and little-endian.
 *   level 0 holds n_0 = C leaves of uint32 (leaf_dev)
 *   level l+1 holds n_{l+1} = ceil(n_l / 16) nodes of uint64, up to the first level H >= 1 with n_H = 1: the root, which holds the total
 *   every level is padded with zeros to a multiple of 16 entries: the 16 children of a node are one aligned run (64 bytes of leaves,
 *   128 bytes of nodes)
 *   levels 1..H lie one after another in node_dev
 *   mxv_prio_layout(C, &leaf_words, &node_words, &levels) returns the sizes (host only): leaf_words uint32, node_words uint64, levels = H
 *   1 <= C <= 2^31, so total < 2^63
 *   after every call each node equals the sum of its 16 children
 *
 * Quantise — q of a TD error td (float32) under 0 <= alpha <= 1 and 2^-64 <= eps <= 1:
 *   x = float64(|float32 td|) + eps
 *   !(x < 2^128) (NaN, +-Inf): q = QMAX
 *   e = alpha * LOG(x);  !(e < 80): q = QMAX
 *   s = rint(EXP(e) * 2^20);  q = s >= 2^32 - 1 ? QMAX : s < 1 ? 1 : uint32(s)
 * alpha = 0 gives 2^20 everywhere: the draw is then uniform over the written slots.
 *
 * Insert — mxv_prio_insert gives the R = K * N <= C slots of a chunk the largest priority seen (call it BEFORE mxv_replay_insert of the
 * same chunk, with the same count / state_dev, so that both read the same count).  Row r:
 *   c = state_dev ? state_dev[0] : count;   s = (c + r) mod C
 *   leaf[s] = *qmax_dev                              (qmax_dev: a uint32 device word, initially 2^20 = priority 1.0)
 *   every ancestor of s receives q - old leaf
 * One launch.  The counter is not advanced (mxv_replay_insert does that).
 *
 * Update — mxv_prio_update sets the priorities of B drawn rows from their TD errors.  Row j, k = indices[j]:
 *   skipped when k < 0 or k >= min(c, C)             (the -1 of an empty draw, a slot never written: a dead slot never becomes drawable)
 *   leaf[k] = max over the rows j' with indices[j'] == k of quantise(td_error[j'])
 *   *qmax_dev = max(*qmax_dev, every q written)
 * Two launches: the first exchanges each leaf for 0 and keeps what it held in workspace_dev[j] (B uint32; only the first arrival at a
 * slot sees a non-zero leaf), the second raises the leaf to q by an integer atomic max and adds to the ancestors what it rose by less
 * workspace_dev[j]; over the rows of a slot the rises telescope to the new leaf and the exchanges sum to the old one, so leaves and sums
 * end consistent in any arrival order.  A slot overwritten between the draw and the update gets the stale row's priority.
 *
 * Sample — mxv_prio_sample draws B rows with P(slot k) = q_k / total (up to the total / 2^64 of one multiply-high) and gathers them.
 * Row j at sample step t = step_dev ? *step_dev : step:
 *   total = the root;  total == 0: indices[j] = -1 and every other output of row j is 0, the weight included
 *   u64 = hi << 32 | lo, the words 2(j & 1) + 1 and 2(j & 1) of Philox4x32-10(key = seed, ctr = (g_lo, g_hi, t_lo, (t_hi & 0x0fffffff) | 10 << 28)),  g = j >> 1
 *   u = mulhi64(u64, total)
 *   for l = H - 1 ... 0: among the 16 children of the current node the smallest i whose inclusive prefix sum exceeds u; u -= the prefix before it; step into child i
 *   indices[j] = k, the leaf reached                 (always a leaf with q_k > u >= 0: never a dead slot, no clamp)
 *   the five ring arrays are gathered at k exactly as mxv_replay_sample gathers them
 *   qmin = the integer minimum over the batch of the drawn leaves
 *   weights[j] = float32(EXP(beta * (LOG(float64 qmin) - LOG(float64 q_k))))          (0 <= beta <= 1)
 * The weight is (N P)^-beta over its batch maximum: exactly 1.0 at the minimum, a function of integers alone.  Row j depends on
 * (seed, j, t, tree) alone, not on B.  Two launches — the draw, which leaves the minima of its workgroups in workspace_dev
 * (MXV_PRIO_WORKSPACE_WORDS uint32), and the gather with the weights — and with step_dev one more, *step_dev += 1.
 *
 * The ring is mxv_replay.h's: ring_obs, ring_next [C, W] dwords, ring_action [C] dwords, ring_reward float32 [C], ring_term uint8 [C];
 * outputs contiguous: indices int64 [B], obs_out, next_out [B, W], action_out [B] of action_bytes (4, or 8: sign-extended), reward_out
 * float32 [B], term_out uint8 [B], weights_out float32 [B].  1 <= W <= 65536, C * W <= 2^40, B * W <= 2^40.
 *
 * Stream-ordered on `stream` (a hipStream_t; NULL = the null stream) of the current device: no synchronisation, no allocation —
 * recordable into a caller's hipGraph.  Every call returns MXV_ERR_INVALID_ARG (message: mxv_prio_last_error), before the device is
 * touched, for: a NULL required pointer; C outside 1..2^31; K, N or B below 1; K * N above C; W outside 1..65536, C * W or B * W beyond
 * 2^40; alpha or beta outside 0..1, eps outside 2^-64..1, or a NaN; leaf_words or node_words other than mxv_prio_layout's; count above
 * 2^63; action_bytes other than 4 or 8; a pointer off its element's boundary (node_dev, indices, state_dev, step_dev: 8; the others 4);
 * a range that would wrap past the top of the address space; an output sharing a byte with an input or with another output.  A failed
 * launch returns MXV_ERR_HIP. */
#ifndef MXV_PRIO_H
#define MXV_PRIO_H

#include "mxv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MXV_PRIO_FANOUT 16
#define MXV_PRIO_FRAC_BITS 20
#define MXV_PRIO_QMAX 4294967295
#define MXV_PRIO_STREAM_TAG 10
#define MXV_PRIO_WORKSPACE_WORDS 2048 /* uint32 words of workspace_dev */

/* Host only: the sizes of the tree of a ring of C slots.  Any of the three outputs may be NULL. */
int mxv_prio_layout(int64_t C, int64_t *leaf_words, int64_t *node_words, int32_t *levels);

int mxv_prio_insert(void *stream, int64_t C, int64_t K, int64_t N, uint64_t count, const uint64_t *state_dev, uint32_t *leaf_dev,
                    int64_t leaf_words, uint64_t *node_dev, int64_t node_words, const uint32_t *qmax_dev);

int mxv_prio_update(void *stream, int64_t C, int64_t B, const int64_t *indices_dev, const float *td_error_dev, double alpha, double eps,
                    uint64_t count, const uint64_t *state_dev, uint32_t *leaf_dev, int64_t leaf_words, uint64_t *node_dev,
                    int64_t node_words, uint32_t *qmax_dev, uint32_t *workspace_dev);

int mxv_prio_sample(void *stream, int64_t C, int32_t W, int64_t B, const void *ring_obs_dev, const void *ring_next_dev,
                    const void *ring_action_dev, const float *ring_reward_dev, const uint8_t *ring_term_dev, const uint32_t *leaf_dev,
                    int64_t leaf_words, const uint64_t *node_dev, int64_t node_words, uint64_t seed, uint64_t step, uint64_t *step_dev,
                    double beta, uint32_t *workspace_dev, int64_t *indices_dev, void *obs_out_dev, void *next_out_dev,
                    void *action_out_dev, int32_t action_bytes, float *reward_out_dev, uint8_t *term_out_dev, float *weights_out_dev);

/* The message of the calling thread's last failed call of this header ("" before the first). */
const char *mxv_prio_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MXV_PRIO_H */
