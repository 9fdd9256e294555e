/* mxv_gae.h — OPTIONAL learner-side pass over [K, N] trajectory tensors: GAE(lambda) advantages and discounted returns-to-go (must be
 * included by itself, mxv.h does not include it).
 * Part of the C ABI of libmxv.so (see mxv.h for the status codes).  Handle-free: the calls take the HIP stream they run on.
 *
 * The rule (tests/gae_host.py).  Inputs are row-major [K][N] with one row stride `ld` in elements (ld >= N: views into
 * wider buffers work), outputs likewise with `ld_out`:
 *   reward       float32, or float64 when reward_is_f64 is nonzero
 *   terminated   uint8, nonzero = set          truncated   uint8, nonzero = set
 *   values       float32: V of the observation the action of step t was taken from
 *   last_value   float32 [N]: V of the observation after step K-1; NULL = 0
 *   final_values float32 [K][N], NULL = absent: V(final_obs[t]); READ only where truncated[t] is set and terminated[t] is not
 * All arithmetic is IEEE float64, one rounding per operation, no FMA; inputs are widened exactly.  With c = gamma * lam formed once on
 * the host, A_K = 0 and nv_K = last_value, for t = K-1 ... 0 of every env:
 *   nv    = terminated ? 0.0 : truncated ? (final_values ? final_values[t] : 0.0) : nv_{t+1}
 *   delta = (reward[t] + gamma * nv) - values[t]
 *   A_t   = (terminated | truncated) ? delta : delta + c * A_{t+1}
 *   advantages[t] = float32(A_t)     returns[t] = float32(A_t + values[t])     nv_t = values[t]
 * The episode cut is a select: a NaN or Inf of a later episode never reaches the rows before the boundary.  float32() rounds to nearest
 * even, subnormal results included; a NaN result is written as the one pattern 0x7FC00000 (IEEE 754 leaves the sign and payload of a
 * generated NaN to the implementation, so the rule fixes them).
 *
 * mxv_discounted_returns has no values: G_K = last_value (or 0), and
 *   G_t = (terminated | truncated) ? reward[t] + gamma * nv : reward[t] + gamma * G_{t+1},   nv as above;   returns[t] = float32(G_t).
 *
 * Both calls are stream-ordered on `stream` (a hipStream_t; NULL = the null stream) of the current device: one kernel launch, no
 * synchronisation, no allocation — recordable into a caller's hipGraph.  They return MXV_ERR_INVALID_ARG, before the device is
 * touched, for: a NULL required pointer (reward, terminated, truncated, values, the outputs); K < 1 or N < 1; ld < N or ld_out < N;
 * K * ld or K * ld_out beyond 2^40; a non-finite gamma or lam; a pointer off its element's boundary or a range that would wrap past
 * the top of the address space; an output that shares a byte with
 * an input or with the other output.  Two arguments whose byte ranges [p, p + ((K-1) ld + N) elements) do not meet share nothing; of
 * ranges that interleave, only those that step by the same number of bytes per row are told apart (column blocks of one wide buffer,
 * e.g. advantages = buf[:, :N] and returns = buf[:, N:2N], are accepted); any other interleaving is refused as overlapping.  A failed
 * launch returns MXV_ERR_HIP.  16-byte
 * accesses, four envs per lane, are used when N >= 2^21, N, ld and ld_out are multiples of 4, reward / values / outputs are 16-byte
 * and the flags 4-byte aligned; every other call takes the element path: same results. */
#ifndef MXV_GAE_H
#define MXV_GAE_H

#include "mxv.h"

#ifdef __cplusplus
extern "C" {
#endif

int mxv_gae(void *stream, int64_t K, int64_t N, const void *reward_dev, int32_t reward_is_f64, int64_t ld, const uint8_t *terminated_dev,
            const uint8_t *truncated_dev, const float *values_dev, const float *last_value_dev, const float *final_values_dev,
            double gamma, double lam, float *advantages_dev, float *returns_dev, int64_t ld_out);

int mxv_discounted_returns(void *stream, int64_t K, int64_t N, const void *reward_dev, int32_t reward_is_f64, int64_t ld,
                           const uint8_t *terminated_dev, const uint8_t *truncated_dev, const float *last_value_dev,
                           const float *final_values_dev, double gamma, float *returns_dev, int64_t ld_out);

/* The message of the calling thread's last failed call of the two above ("" before the first). */
const char *mxv_gae_last_error(void);

/* Diagnostic: the instantiation of the calling thread's last successful launch of the two above — envs per lane (4: the 16-byte path,
 * 1: the element path; 0 before the first launch) and the number of workgroups. */
int mxv_gae_last_launch(int32_t *envs_per_lane, uint32_t *grid);

#ifdef __cplusplus
}
#endif
#endif /* MXV_GAE_H */
