"""NumPy float64 twin of the four passes of include/mxv_policy_eval.h: log pi and entropy of stored actions under a
categorical or a diagonal-Gaussian head, and the gradients of both with respect to the head's outputs.  Every line below is one IEEE
float64 operation on whole columns (NumPy neither fuses nor re-associates them), in the order the rule states; EXP and LOG are the
operation sequences of tests/policy_host.py / tests/gaussian_host.py (the same constants, the Gaussian rule's widened domains), not
libm.  The device must produce the same bits (tests/test_gpu_policy_eval.py), and tests/test_policy_eval_host.py holds this file to
200-bit mpmath."""
import numpy as np

import gaussian_host as gh
import policy_host as ph

CANONICAL_NAN = ph.CANONICAL_NAN
EXP_CUT = ph.EXP_CUT
EXP, LOG, to_f32, bits = gh.EXP, gh.LOG, ph.to_f32, ph.bits
HALF_LOG_2PI, ENT_C, LOG_STD_MAX = gh.HALF_LOG_2PI, gh.ENT_C, gh.LOG_STD_MAX
# measured on these rules with the input of tests/test_policy_eval_host.py, against 200-bit mpmath, on the float64 gradients before their
# float32 rounding; the tests hold twice that, rounded up.  Units of 2^-53: absolute for the categorical ones (d log_prob / d logit
# with gl = 1 alone, d entropy / d logit with gh = 1 alone); relative to |exact| for d log_prob / d mean, and relative to zq^2 + 1 — the
# magnitude of its two terms — for d log_prob / d log_std = zq^2 - 1.
B_GRAD_LOG_PROB = 6.92
B_GRAD_ENTROPY = 5.88
B_GRAD_MEAN = 3.73
B_GRAD_LOG_STD = 3.72


def bar(b):
    return int(np.ceil(2 * b))


def _f64(g, M):
    return None if g is None else np.asarray(g, np.float32).reshape(M).astype(np.float64)


def categorical_parts(logits, actions):
    """The row quantities of the rule on float32 logits [M, A] and integer actions [M] -> dict of float64 arrays: d, e [M, A]; S, T, L,
    H (the float64 entropy), d_action [M]; onehot [M, A]; degenerate [M]."""
    x32 = np.asarray(logits, np.float32)
    M, A = x32.shape
    act = np.asarray(actions).astype(np.int64).reshape(M)
    x = x32.astype(np.float64)
    with np.errstate(all="ignore"):
        bad_action = (act < 0) | (act >= A)
        degenerate = np.isnan(x).any(1) | (x == np.inf).any(1) | (x == -np.inf).all(1) | bad_action
        m = x[:, 0].copy()
        for a in range(1, A):
            m = np.where(x[:, a] > m, x[:, a], m)
        m = np.where(degenerate, 0.0, m)
        xs = np.where(degenerate[:, None], 0.0, x)           # keep the arithmetic of degenerate rows quiet; their results are replaced
        d = xs - m[:, None]
        live = ~(d < EXP_CUT)
        e = np.where(live, EXP(np.where(live, d, 0.0)), 0.0)
        S = np.zeros(M, np.float64)
        T = np.zeros(M, np.float64)
        for a in range(A):
            S = S + e[:, a]
            T = np.where(e[:, a] == 0.0, T, T + e[:, a] * np.where(live[:, a], d[:, a], 0.0))
        L = LOG(S)
        H = L - T / S
    onehot = (np.arange(A)[None, :] == act[:, None]).astype(np.float64)      # all zero for an action outside the row: nothing is indexed
    d_action = np.where(bad_action, 0.0, d[np.arange(M), np.where(bad_action, 0, act)])
    return dict(d=d, e=e, S=S, T=T, L=L, H=H, d_action=d_action, onehot=onehot, degenerate=degenerate)


def categorical(logits, actions):
    """-> (log_prob, entropy) float64 [M], before the float32 rounding; NaN on degenerate rows."""
    p = categorical_parts(logits, actions)
    with np.errstate(all="ignore"):
        log_prob = p["d_action"] - p["L"]
    return np.where(p["degenerate"], np.nan, log_prob), np.where(p["degenerate"], np.nan, p["H"])


def categorical_backward(logits, actions, grad_log_prob=None, grad_entropy=None):
    """-> grad_logits float64 [M, A], before the float32 rounding; None for an absent incoming gradient (its term is left out)."""
    assert grad_log_prob is not None or grad_entropy is not None
    p = categorical_parts(logits, actions)
    M = p["S"].shape[0]
    gl, gH = _f64(grad_log_prob, M), _f64(grad_entropy, M)
    with np.errstate(all="ignore"):
        q = p["e"] / p["S"][:, None]
        lp = p["d"] - p["L"][:, None]
        dlp = p["onehot"] - q
        dH = np.where(p["e"] == 0.0, 0.0, -(q * (lp + p["H"][:, None])))
        if gl is not None and gH is not None:
            g = gl[:, None] * dlp + gH[:, None] * dH
        elif gl is not None:
            g = gl[:, None] * dlp
        else:
            g = gH[:, None] * dH
    return np.where(p["degenerate"][:, None], np.nan, g)


def gaussian_parts(mean, log_std, actions):
    """float32 mean [M, D], log_std [M, D] or [D], actions [M, D] -> dict of float64 arrays: mu, ls, sigma, zq [M, D]; degenerate [M]."""
    mu32 = np.asarray(mean, np.float32)
    M, D = mu32.shape
    assert 1 <= D <= gh.MAX_DIM
    ls32 = np.broadcast_to(np.asarray(log_std, np.float32), (M, D))
    act = np.asarray(actions, np.float32).reshape(M, D).astype(np.float64)
    mu, ls = mu32.astype(np.float64), ls32.astype(np.float64)
    with np.errstate(all="ignore"):
        degenerate = (~np.isfinite(mu)).any(1) | (~np.isfinite(ls)).any(1) | (np.abs(ls) > LOG_STD_MAX).any(1)
        mu = np.where(degenerate[:, None], 0.0, mu)
        ls = np.where(degenerate[:, None], 0.0, ls)
        sigma = EXP(ls)
        zq = (act - mu) / sigma
    return dict(mu=mu, ls=ls, sigma=sigma, zq=zq, degenerate=degenerate)


def gaussian(mean, log_std, actions):
    """-> (log_prob, entropy) float64 [M], before the float32 rounding; NaN on degenerate rows."""
    p = gaussian_parts(mean, log_std, actions)
    M, D = p["mu"].shape
    log_prob, entropy = np.zeros(M, np.float64), np.zeros(M, np.float64)
    with np.errstate(all="ignore"):
        for j in range(D):
            zq, ls = p["zq"][:, j], p["ls"][:, j]
            log_prob = log_prob + ((-0.5 * (zq * zq) - ls) - HALF_LOG_2PI)
            entropy = entropy + (ls + ENT_C)
    return np.where(p["degenerate"], np.nan, log_prob), np.where(p["degenerate"], np.nan, entropy)


def gaussian_backward(mean, log_std, actions, grad_log_prob=None, grad_entropy=None):
    """-> (grad_mean, grad_log_std) float64 [M, D] — per row also for a shared log_std — before the float32 rounding."""
    assert grad_log_prob is not None or grad_entropy is not None
    p = gaussian_parts(mean, log_std, actions)
    M, D = p["mu"].shape
    gl, gH = _f64(grad_log_prob, M), _f64(grad_entropy, M)
    with np.errstate(all="ignore"):
        if gl is not None:
            g_mean = gl[:, None] * (p["zq"] / p["sigma"])
            g_ls = gl[:, None] * (p["zq"] * p["zq"] - 1.0)
            if gH is not None:
                g_ls = g_ls + gH[:, None]
        else:
            g_mean = np.zeros((M, D), np.float64)
            g_ls = np.broadcast_to(gH[:, None], (M, D)).copy()
    return np.where(p["degenerate"][:, None], np.nan, g_mean), np.where(p["degenerate"][:, None], np.nan, g_ls)
