"""NumPy float64 twin of the rule in include/mxv_vtrace.h: V-trace value targets and policy-gradient advantages over
[K, N] arrays.  Every operation below is one IEEE float64 operation on whole rows (NumPy neither fuses nor re-associates them), in the
order the rule states; EXP is the operation sequence of tests/policy_host.py, not libm.  The device must produce the same bits
(tests/test_gpu_vtrace.py), and tests/test_vtrace_host.py holds this file to an independent scalar loop and to the paper's definition
in 200-bit mpmath.

Not a test module.  Nothing under gym_amd/ imports it."""
import numpy as np

import policy_host as ph

EXP, to_f32, bits = ph.EXP, ph.to_f32, ph.bits
RATIO_LOG_MAX = 80.0
# measured on this rule with the input of tests/test_vtrace_host.py (K = 24, N = 400, three seeds: done probability 0.1, |d| up to 3,
# lam in 0.9, 0.95, 1, clip levels 0.8 to 1.5) against the paper's definition in 200-bit mpmath, before the float32 rounding, in units
# of 2^-53 * (sum of the magnitudes of the terms of the element's expansion); the tests hold twice that, rounded up
B_VS = 2.26
B_PG = 2.39
BAR_VS = int(np.ceil(2 * B_VS))
BAR_PG = int(np.ceil(2 * B_PG))


def weights(log_prob, old_log_prob):
    """w [K, N] float64: the importance weight pi / mu before truncation — the ratio lines of the PPO loss rule (tests/ppo_host.py)."""
    lp, old = np.asarray(log_prob, np.float32).astype(np.float64), np.asarray(old_log_prob, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        d = lp - old
        d = np.where(d < -RATIO_LOG_MAX, -RATIO_LOG_MAX, np.where(d > RATIO_LOG_MAX, RATIO_LOG_MAX, d))
        d_nan = np.isnan(d)
        return np.where(d_nan, np.nan, EXP(np.where(d_nan, 0.0, d)))


def vtrace_f64(log_prob, old_log_prob, reward, terminated, truncated, values, last_value=None, *, gamma=0.99, lam=1.0, rho_bar=1.0,
               c_bar=1.0, pg_rho_bar=None, final_values=None):
    """-> (vs, pg_advantages) float64 [K, N], before the float32 rounding."""
    r = np.asarray(reward)
    assert r.ndim == 2 and r.dtype in (np.float32, np.float64)
    K, N = r.shape
    r = r.astype(np.float64)
    term, trunc = np.asarray(terminated).reshape(K, N) != 0, np.asarray(truncated).reshape(K, N) != 0
    v = np.asarray(values, np.float32).reshape(K, N).astype(np.float64)
    nv = np.zeros(N, np.float64) if last_value is None else np.asarray(last_value, np.float32).reshape(N).astype(np.float64)
    fv = None if final_values is None else np.asarray(final_values, np.float32).reshape(K, N).astype(np.float64)
    gamma, lam, rho_bar, c_bar = np.float64(gamma), np.float64(lam), np.float64(rho_bar), np.float64(c_bar)
    pg_rho_bar = rho_bar if pg_rho_bar is None else np.float64(pg_rho_bar)
    w = weights(log_prob, old_log_prob).reshape(K, N)
    acc, vs_next = np.zeros(N, np.float64), nv
    vs, pg = np.empty((K, N), np.float64), np.empty((K, N), np.float64)
    with np.errstate(all="ignore"):
        for t in range(K - 1, -1, -1):
            rho = np.where(w[t] > rho_bar, rho_bar, w[t])
            cs = lam * np.where(w[t] > c_bar, c_bar, w[t])
            rpg = np.where(w[t] > pg_rho_bar, pg_rho_bar, w[t])
            done = term[t] | trunc[t]
            boot = np.zeros(N, np.float64) if fv is None else np.where(trunc[t] & ~term[t], fv[t], 0.0)
            nxt = np.where(done, np.where(term[t], 0.0, boot), nv)
            delta = rho * ((r[t] + gamma * nxt) - v[t])
            gc = gamma * cs
            acc = np.where(done, delta, delta + gc * acc)
            vs[t] = acc + v[t]
            nvs = np.where(done, nxt, vs_next)
            pg[t] = rpg * ((r[t] + gamma * nvs) - v[t])
            vs_next, nv = vs[t], v[t]
    return vs, pg


def vtrace(*args, **kw):
    """-> (vs, pg_advantages) as the device writes them: float32 [K, N], NaNs canonical."""
    vs, pg = vtrace_f64(*args, **kw)
    return to_f32(vs), to_f32(pg)
