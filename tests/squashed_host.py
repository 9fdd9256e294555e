"""NumPy float64 twin of the rule in include/mxv_squashed.h: reparameterised, tanh-squashed diagonal-Gaussian draws,
their log-probabilities, and the gradients of both with respect to mean and log_std.  Every line below is one IEEE float64 operation on
whole columns (NumPy neither fuses nor re-associates them), in the order the rule states; LOG, EXP and the normals are
tests/gaussian_host.py's (the policy header's operation sequences, not libm); `/` is IEEE.  The device must produce the same bits
(tests/test_gpu_squashed.py), and tests/test_squashed_host.py holds this file to 200-bit mpmath.  The Philox words are those of
gaussian_host.words under stream tag 11, computed on whole columns by replay_host's Philox4x32-10 and held to the oracle's on the first
and last row of every call."""
import numpy as np

import replay_host as rh
from gaussian_host import EXP, HALF_LOG_2PI, LN2_HI, LN2_LO, LOG, LOG_STD_MAX, MAX_DIM, Z_MAX, bar, bits, normal_pair, to_f32      # noqa: F401
from policy_host import EXP_CUT

STREAM_SQUASHED = 11
LN2 = np.float64(LN2_HI + LN2_LO)     # rounded once
TINY = np.float64(2.0 ** -27)
E_CUT_V = 354.0                       # e == 0 for v > 354: -2 v < -708
SCALE_MIN, SCALE_MAX = 2.0 ** -33, 64.0
# measured on this rule with the input of tests/test_squashed_host.py, against 200-bit mpmath, before the float32 rounding; the tests
# hold twice that, rounded up.  Units: 2^-53 for TANH (th against tanh(v), absolute: the ulp of a result near 1, and 2^-26 relative at
# the switch v = 2^-27, under half a float32 ulp); 2^-53 * (1 + |exact|) for CORR; for
# LOG_PROB and the gradients 2^-53 times the magnitude of the terms that are added, which test_squashed_host.py's _scales writes out.
B_TANH = 1.42
B_CORR = 3.43
B_LOG_PROB = 2.10
B_GRAD_MEAN = 3.03
B_GRAD_LOG_STD = 1.71


def E(d):
    """EXP(d), and exactly 0 below the cut (e_of)."""
    d = np.asarray(d, np.float64)
    cut = d < EXP_CUT
    return np.where(cut, 0.0, EXP(np.where(cut, 0.0, d)))


def words(seed, G, t):
    """The four Philox words [len(G), 4] of the global row indices G at draw step t: one call per row, stream tag 11."""
    from oracle import oracle

    seed, t = int(seed) & (2 ** 64 - 1), int(t) & (2 ** 64 - 1)
    G = np.asarray([int(g) & (2 ** 64 - 1) for g in G] if not isinstance(G, np.ndarray) else G, np.uint64)
    c2, c3 = t & 0xFFFFFFFF, ((t >> 32) & 0x0FFFFFFF) | (STREAM_SQUASHED << 28)
    w4 = np.stack(rh.philox4x32_10(G & np.uint64(0xFFFFFFFF), G >> np.uint64(32), c2, c3, seed & 0xFFFFFFFF, seed >> 32), axis=1)
    for i in {0, len(G) - 1}:
        g = int(G[i])
        assert np.array_equal(w4[i], oracle.philox4x32_10((g & 0xFFFFFFFF, g >> 32, c2, c3), (seed & 0xFFFFFFFF, seed >> 32)))
    return w4


def affine(D, scale=None, bias=None):
    """scale and bias as the library takes them: float32 [D], None -> 1 and 0; widened exactly."""
    sc = np.ones(D, np.float32) if scale is None else np.broadcast_to(np.asarray(scale, np.float32), (D,))
    bi = np.zeros(D, np.float32) if bias is None else np.broadcast_to(np.asarray(bias, np.float32), (D,))
    assert np.all((sc >= SCALE_MIN) & (sc <= SCALE_MAX)) and np.all(np.isfinite(bi))
    return sc.astype(np.float64), bi.astype(np.float64)


def normals(w4, D):
    """z [N, D] of the words w4 [N, 4]: words 0, 1 make dims 0, 1 and words 2, 3 dims 2, 3."""
    N = len(w4)
    z = np.empty((N, D), np.float64)
    for p in range((D + 1) // 2):
        ze, zo = normal_pair(w4[:, 2 * p], w4[:, 2 * p + 1])
        z[:, 2 * p] = ze
        if 2 * p + 1 < D:
            z[:, 2 * p + 1] = zo
    return z


def squash(mu, ls, z):
    """The lines of the rule from sigma to t, which forward and backward share, on float64 columns -> dict."""
    sigma = EXP(ls)
    n = sigma * z
    u = mu + n
    v = np.abs(u)
    e = E(-2.0 * v)
    q = 1.0 + e
    th = np.where(v < TINY, v, (1.0 - e) / q)
    t = np.copysign(th, u)
    return dict(sigma=sigma, n=n, u=u, v=v, e=e, q=q, th=th, t=t)


def _inputs(mean, log_std):
    mu32 = np.asarray(mean, np.float32)
    N, D = mu32.shape
    assert 1 <= D <= MAX_DIM
    ls32 = np.broadcast_to(np.asarray(log_std, np.float32), (N, D))
    mu, ls = mu32.astype(np.float64), ls32.astype(np.float64)
    degenerate = (~np.isfinite(mu)).any(1) | (~np.isfinite(ls)).any(1) | (np.abs(ls) > LOG_STD_MAX).any(1)
    mu = np.where(degenerate[:, None], 0.0, mu)           # keep the arithmetic of degenerate rows quiet; their results are replaced
    ls = np.where(degenerate[:, None], 0.0, ls)
    return mu, ls, degenerate


def evaluate(mean, log_std, w4, scale=None, bias=None, z=None):
    """The forward rule on float32 mean [N, D], log_std [N, D] or [D], words w4 [N, 4] (or the normals z themselves) -> dict, float64
    before the float32 rounding of log_prob: the values of squash() [N, D], z, a (float64 actions), act (float32), corr, log_prob,
    degenerate."""
    with np.errstate(all="ignore"):
        mu, ls, degenerate = _inputs(mean, log_std)
        N, D = mu.shape
        sc, bi = affine(D, scale, bias)
        z = normals(np.asarray(w4, np.uint32).reshape(N, 4), D) if z is None else np.asarray(z, np.float64)
        r = squash(mu, ls, z)
        a = bi + sc * r["t"]
        corr = 2.0 * ((LN2 - r["v"]) - LOG(r["q"]))
        lsc = LOG(sc)
        log_prob = np.zeros(N, np.float64)
        for j in range(D):
            log_prob = log_prob + (((-0.5 * (z[:, j] * z[:, j]) - ls[:, j]) - HALF_LOG_2PI) - (lsc[j] + corr[:, j]))
        act = np.where(degenerate[:, None], np.float32(np.nan), a.astype(np.float32))
        log_prob = np.where(degenerate, np.nan, log_prob)
    return dict(r, z=z, a=a, act=act, corr=corr, log_prob=log_prob, degenerate=degenerate, mu=mu, ls=ls, scale=sc, bias=bi)


def gradients(mean, log_std, w4, grad_actions=None, grad_log_prob=None, scale=None, z=None):
    """The backward rule -> dict: grad_mean, grad_log_std [N, D] in float64 before their float32 rounding (NaN in degenerate rows), s
    and the values of squash().  grad_actions float32 [N, D] and grad_log_prob float32 [N]; None means zeros."""
    with np.errstate(all="ignore"):
        mu, ls, degenerate = _inputs(mean, log_std)
        N, D = mu.shape
        sc, _ = affine(D, scale, None)
        z = normals(np.asarray(w4, np.uint32).reshape(N, 4), D) if z is None else np.asarray(z, np.float64)
        ga = np.zeros((N, D)) if grad_actions is None else np.asarray(grad_actions, np.float32).astype(np.float64)
        glp = (np.zeros(N) if grad_log_prob is None else np.asarray(grad_log_prob, np.float32).astype(np.float64))[:, None]
        r = squash(mu, ls, z)
        s = (4.0 * r["e"]) / (r["q"] * r["q"])
        gs = (ga * sc) * s
        t2 = 2.0 * r["t"]
        gm = gs + glp * t2
        gls = gs * r["n"] + glp * (t2 * r["n"] - 1.0)
        gm = np.where(degenerate[:, None], np.nan, gm)
        gls = np.where(degenerate[:, None], np.nan, gls)
    return dict(r, z=z, s=s, grad_mean=gm, grad_log_std=gls, degenerate=degenerate, ga=ga, glp=glp, scale=sc)


def _rows_of(mean, env_offset):
    N = np.asarray(mean).shape[0]
    return (np.uint64(int(env_offset) & (2 ** 64 - 1)) + np.arange(N, dtype=np.uint64))      # wraps modulo 2^64


def sample(mean, log_std, *, seed, step, env_offset=0, scale=None, bias=None):
    """-> (actions float32 [N, D], log_prob float32 [N]); NaNs are the canonical pattern."""
    mu = np.asarray(mean, np.float32)
    with np.errstate(over="ignore"):
        r = evaluate(mu, log_std, words(seed, _rows_of(mu, env_offset), step), scale, bias)
    return to_f32(r["act"]).reshape(mu.shape), to_f32(r["log_prob"])


def sample_backward(mean, log_std, *, seed, step, env_offset=0, scale=None, grad_actions=None, grad_log_prob=None):
    """-> (grad_mean float32 [N, D], grad_log_std float32 [N, D]); NaNs are the canonical pattern."""
    mu = np.asarray(mean, np.float32)
    with np.errstate(over="ignore"):
        r = gradients(mu, log_std, words(seed, _rows_of(mu, env_offset), step), grad_actions, grad_log_prob, scale)
    return to_f32(r["grad_mean"]).reshape(mu.shape), to_f32(r["grad_log_std"]).reshape(mu.shape)
