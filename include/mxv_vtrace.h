/* mxv_vtrace.h — OPTIONAL learner-side pass over [K, N] trajectory tensors: V-trace value targets and policy-gradient advantages
 * (Espeholt et al. 2018) for batches that were not drawn by the policy being updated (must be included by itself, mxv.h does not
 * include it).
 * Part of the C ABI of libmxv.so (see mxv.h for the status codes).  Handle-free: the call takes the HIP stream it runs on.
 *
 * The rule (tests/vtrace_host.py).  Inputs are row-major [K][N] with one row stride `ld` in elements (ld >= N: views into
 * wider buffers work), outputs likewise with `ld_out`:
 *   log_prob     float32: the target policy's log pi(a_t)          old_log_prob  float32: the behaviour policy's
 *   reward       float32, or float64 when reward_is_f64 is nonzero
 *   terminated   uint8, nonzero = set          truncated   uint8, nonzero = set
 *   values       float32: V of the observation the action of step t was taken from
 *   last_value   float32 [N]: V of the observation after step K-1; NULL = 0
 *   final_values float32 [K][N], NULL = absent: V(final_obs[t]); READ only where truncated[t] is set and terminated[t] is not
 * gamma, lam, rho_bar > 0, c_bar > 0 and pg_rho_bar > 0 are finite.  All arithmetic is IEEE float64, one rounding per operation, no
 * FMA, in the order written; inputs are widened exactly.  EXP is the operation sequence of mxv_policy.h on its widened domain
 * |d| <= 80.  With acc_K = 0 and nv_K = vs_K = last_value (or 0), for t = K-1 ... 0 of every env:
 *   d     = log_prob[t] - old_log_prob[t];  d = d < -80 ? -80 : (d > 80 ? 80 : d)
 *   w     = isnan(d) ? NaN : EXP(isnan(d) ? 0.0 : d)
 *   rho   = w > rho_bar ? rho_bar : w          cs = lam * (w > c_bar ? c_bar : w)          rpg = w > pg_rho_bar ? pg_rho_bar : w
 *   done  = terminated | truncated
 *   nv    = terminated ? 0.0 : truncated ? (final_values ? final_values[t] : 0.0) : nv_{t+1}
 *   delta = rho * ((reward[t] + gamma * nv) - values[t])
 *   gc    = gamma * cs
 *   acc_t = done ? delta : delta + gc * acc_{t+1}
 *   vs_t  = acc_t + values[t]
 *   nvs   = done ? nv : vs_{t+1}
 *   pg_t  = rpg * ((reward[t] + gamma * nvs) - values[t])
 *   vs[t] = float32(vs_t)     pg_advantages[t] = float32(pg_t)     nv_t = values[t]
 * The selects are written so that a NaN w stays NaN in rho, cs and rpg (a comparison with a NaN is false).  The episode cut is a
 * select, never a multiplication by (1 - done): a NaN or Inf of a later episode never reaches the rows before the boundary.
 * float32() rounds to nearest even, subnormal results included; a NaN result is written as the one pattern 0x7FC00000.
 *
 * Two properties follow from the rule:
 *   * EXP(0) is exactly 1.  With log_prob bit-equal to old_log_prob (and finite) and rho_bar, c_bar >= 1, rho = 1 and cs = lam * 1.0,
 *     so vs has the bits of the `returns` of mxv_gae at the same gamma and lam: gc = gamma * (lam * 1.0) is the c that GAE forms on the
 *     host, and a product with 1.0 is exact.
 *   * w has the bits of the ratio r of the PPO clipped-surrogate loss on the same two inputs: the d, clamp, NaN and EXP
 *     lines are that rule's.
 *
 * The call is stream-ordered on `stream` (a hipStream_t; NULL = the null stream) of the current device: one kernel launch, no
 * synchronisation, no allocation — recordable into a caller's hipGraph.  It returns MXV_ERR_INVALID_ARG (message:
 * mxv_vtrace_last_error), before the device is touched, for: a NULL required pointer (log_prob, old_log_prob, reward, terminated,
 * truncated, values, either output); K < 1 or N < 1; ld < N or ld_out < N; K * ld or K * ld_out beyond 2^40; a non-finite gamma, lam,
 * rho_bar, c_bar or pg_rho_bar; a clip level <= 0; a pointer off its element's boundary or a range that would wrap past the top of the
 * address space; an output that shares a byte with an input or with the other output.  Two arguments whose byte ranges
 * [p, p + ((K-1) ld + N) elements) do not meet share nothing; of ranges that interleave, only those that step by the same number of
 * bytes per row are told apart (column blocks of one wide buffer are accepted); any other interleaving is refused as overlapping.  A
 * failed launch returns MXV_ERR_HIP.  16-byte accesses, four envs per lane, are used when N >= 2^21, N, ld and ld_out are multiples of
 * 4, the float arrays are 16-byte and the flags 4-byte aligned; every other call takes the element path: same results. */
#ifndef MXV_VTRACE_H
#define MXV_VTRACE_H

#include "mxv.h"

#ifdef __cplusplus
extern "C" {
#endif

int mxv_vtrace(void *stream, int64_t K, int64_t N, const float *log_prob_dev, const float *old_log_prob_dev, const void *reward_dev,
               int32_t reward_is_f64, int64_t ld, const uint8_t *terminated_dev, const uint8_t *truncated_dev, const float *values_dev,
               const float *last_value_dev, const float *final_values_dev, double gamma, double lam, double rho_bar, double c_bar,
               double pg_rho_bar, float *vs_dev, float *pg_advantages_dev, int64_t ld_out);

/* The message of the calling thread's last failed call of this header ("" before the first). */
const char *mxv_vtrace_last_error(void);

/* Diagnostic: the instantiation of the calling thread's last successful launch of mxv_vtrace — envs per lane (4: the 16-byte path,
 * 1: the element path; 0 before the first launch) and the number of workgroups. */
int mxv_vtrace_last_launch(int32_t *envs_per_lane, uint32_t *grid);

#ifdef __cplusplus
}
#endif
#endif /* MXV_VTRACE_H */
