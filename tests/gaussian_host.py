"""NumPy float64 twin of the Gaussian rule in include/mxv_policy.h: diagonal-Gaussian draws from a policy head's mean
and log_std, their log-probabilities and the entropy.  Every line below is one IEEE float64 operation on whole columns (NumPy neither
fuses nor re-associates them), in the order the rule states; LOG, SINCOS2PI and EXP are the header's operation sequences, not libm;
`/` and sqrt are IEEE.  The device must produce the same bits (tests/test_gpu_gaussian.py), and tests/test_gaussian_host.py holds this
file to 200-bit mpmath.  The Philox words come from oracle.philox4x32_10, the constants from tools/gaussian_coefficients.py.  What the rule
shares with the categorical one — EXP, LOG, their constants, u01 and the float32 helpers — is tests/policy_host.py's, under the same names."""
import os
import sys

import numpy as np

from conftest import ROOT
from policy_host import CANONICAL_NAN, EXP, EXP_C, INV_LN2, LN2_HI, LN2_LO, LOG, LOG_C, SQRT_HALF, bits, rule_block, to_f32, u01      # noqa: F401

sys.path.insert(0, os.path.join(ROOT, "tools"))
try:
    import gaussian_coefficients as _coef
finally:
    sys.path.pop(0)

STREAM_GAUSSIAN = 8
MAX_DIM = 4
LOG_STD_MAX = 80.0
Z_MAX = 6.77          # |z| <= sqrt(2 * 33 ln 2) = 6.7639...: 32-bit uniforms
# measured on this rule with the input of tests/test_gaussian_host.py, against 200-bit mpmath, before the float32 rounding; the tests
# hold twice that, rounded up.  Units: ulps of the result for LOG, SIN, COS, EXP and Z_REL; 2^-53 for Z_ABS, LOG_PROB and ENTROPY
# (absolute); 2^-53 * (|mu| + sigma |z|) for ACT, the float64 action before its float32 rounding.
B_LOG = 1.93
B_SIN = 1.21
B_COS = 1.10
B_EXP = 1.05
B_Z_REL = 2.59
B_Z_ABS = 7.78
B_ACT = 3.59
B_LOG_PROB = 83.32
B_ENTROPY = 2.61


def bar(b):
    return int(np.ceil(2 * b))


_C = _coef.constants()
PIO2_HI, PIO2_LO, HALF_LOG_2PI, ENT_C = (np.float64(_C[k]) for k in ("pio2_hi", "pio2_lo", "half_log_2pi", "ent_c"))
SIN_C = [np.float64(x) for x in _C["sin_c"]]
COS_C = [np.float64(x) for x in _C["cos_c"]]


def sincos_parts(w):
    """The intermediate values of SINCOS2PI(w): t, k, f, f * PIO2_HI, r."""
    v = u01(w)
    t = 4.0 * v
    k = np.rint(t)
    f = t - k
    hi = f * PIO2_HI
    r = hi + f * PIO2_LO
    return t, k, f, hi, r


def SINCOS2PI(w):
    """(sin, cos) of 2 pi (w + 0.5) 2^-32 for uint32 words w."""
    _, k, _, _, r = sincos_parts(w)
    z = r * r
    p = np.full_like(r, SIN_C[-1])
    for c in SIN_C[-2::-1]:
        p = p * z + c
    s = r + r * (z * p)
    q = np.full_like(r, COS_C[-1])
    for c in COS_C[-2::-1]:
        q = q * z + c
    c = 1.0 + z * q
    q4 = k.astype(np.int64) & 3
    sn = np.where(q4 == 0, s, np.where(q4 == 1, c, np.where(q4 == 2, -s, -c)))
    cs = np.where(q4 == 0, c, np.where(q4 == 1, -s, np.where(q4 == 2, -c, s)))
    return sn, cs


def normal_pair(wa, wb):
    """(z_even, z_odd) of one pair of words."""
    u = u01(wa)
    rad = np.sqrt(-2.0 * LOG(u))
    sn, cs = SINCOS2PI(wb)
    return rad * cs, rad * sn


_words_cache = {}


def words(seed, G, t):
    """The four Philox words [len(G), 4] of the global env indices G at policy step t: one call per env."""
    from oracle import oracle

    seed, t = int(seed) & (2 ** 64 - 1), int(t) & (2 ** 64 - 1)
    key = (seed & 0xffffffff, seed >> 32)
    G = [int(g) & (2 ** 64 - 1) for g in G]
    out = np.empty((len(G), 4), np.uint32)
    for i, g in enumerate(G):
        ck = (seed, g, t)
        w4 = _words_cache.get(ck)
        if w4 is None:
            ctr = (g & 0xffffffff, g >> 32, t & 0xffffffff, ((t >> 32) & 0x0fffffff) | (STREAM_GAUSSIAN << 28))
            w4 = oracle.philox4x32_10(ctr, key)
            if len(_words_cache) > (1 << 18):
                _words_cache.clear()
            _words_cache[ck] = w4
        out[i] = w4
    return out


def evaluate(mean, log_std, w4):
    """The rule on float32 mean [N, D], log_std [N, D] or [D], words w4 [N, 4] -> dict (float64, before the float32 rounding of
    log_prob and entropy): z [N, D], sigma, a (float64 actions), act (float32), zq, log_prob, entropy, degenerate."""
    mu32 = np.asarray(mean, np.float32)
    N, D = mu32.shape
    assert 1 <= D <= MAX_DIM
    ls32 = np.broadcast_to(np.asarray(log_std, np.float32), (N, D))
    w4 = np.asarray(w4, np.uint32).reshape(N, 4)
    mu, ls = mu32.astype(np.float64), ls32.astype(np.float64)
    with np.errstate(all="ignore"):
        degenerate = (~np.isfinite(mu)).any(1) | (~np.isfinite(ls)).any(1) | (np.abs(ls) > LOG_STD_MAX).any(1)
        mu = np.where(degenerate[:, None], 0.0, mu)           # keep the arithmetic of degenerate rows quiet; their results are replaced
        ls = np.where(degenerate[:, None], 0.0, ls)
        z = np.empty((N, D), np.float64)
        for p in range((D + 1) // 2):
            ze, zo = normal_pair(w4[:, 2 * p], w4[:, 2 * p + 1])
            z[:, 2 * p] = ze
            if 2 * p + 1 < D:
                z[:, 2 * p + 1] = zo
        sigma = EXP(ls)
        a = mu + sigma * z
        act = a.astype(np.float32)
        zq = (act.astype(np.float64) - mu) / sigma
        log_prob = np.zeros(N, np.float64)
        entropy = np.zeros(N, np.float64)
        for j in range(D):
            log_prob = log_prob + ((-0.5 * (zq[:, j] * zq[:, j]) - ls[:, j]) - HALF_LOG_2PI)
            entropy = entropy + (ls[:, j] + ENT_C)
    act = np.where(degenerate[:, None], np.float32(np.nan), act)
    log_prob = np.where(degenerate, np.nan, log_prob)
    entropy = np.where(degenerate, np.nan, entropy)
    return dict(z=z, sigma=sigma, a=a, act=act, zq=zq, log_prob=log_prob, entropy=entropy, degenerate=degenerate)


def sample_gaussian(mean, log_std, *, seed, step, env_offset=0):
    """-> (actions float32 [N, D], log_prob float32 [N], entropy float32 [N]); NaNs are the canonical pattern."""
    mu = np.asarray(mean, np.float32)
    G = [(int(env_offset) + i) & (2 ** 64 - 1) for i in range(mu.shape[0])]
    r = evaluate(mu, log_std, words(seed, G, step))
    return to_f32(r["act"]).reshape(mu.shape), to_f32(r["log_prob"]), to_f32(r["entropy"])
