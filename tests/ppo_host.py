"""NumPy float64 twin of include/mxv_ppo.h: the PPO clipped-surrogate loss of a batch, its diagnostics, its gradients and
the moments the advantages are normalised with.  Every line below is one IEEE float64 operation on whole columns (NumPy neither fuses
nor re-associates them), in the order the rule states; EXP is the operation sequence of tests/policy_host.py, not libm; `/` and sqrt
are IEEE.  The sums are the fixed trees of the rule: the leaves below, then tests/norm_tree_host.py's `tree`.  The device must produce
the same bits (tests/test_gpu_ppo.py), and tests/test_ppo_host.py holds this file to torch's float64 autograd and to exact sums.

Not a test module.  Nothing under gym_amd/ imports it."""
import numpy as np

import norm_tree_host as nt
import policy_host as ph
from gaussian_host import B_EXP

EXP, to_f32, bits = ph.EXP, ph.to_f32, ph.bits
LEAF_ROWS = 1024                 # rows per leaf: lane t of 256 takes rows t, t + 256, t + 512, t + 768
RATIO_LOG_MAX = 80.0
CANONICAL_NAN64 = np.uint64(0x7FF8000000000000)
STAT_NAMES = ("policy_loss", "value_loss", "entropy", "approx_kl", "approx_kl3", "clip_fraction", "ratio_min", "ratio_max")
# measured with the input of tests/test_ppo_host.py (20 000 rows, with and without the normalisation) against torch's float64 autograd of
# the literal expression of examples/ppo_clip.py, in units of 2^-53 of the reference's magnitude (for the loss: of the sum of the
# magnitudes of its three terms; for the moments: against exact rational arithmetic, at the sizes of that test).  The tests hold the
# derived bars — B_EXP for the ratio, sum_error_bound(depth(M), sum |term|) for a sum, half a float32 ulp for a float32 output — and
# these record what is used of them.
B_LOSS = 2.64
B_STATS = 11.24
B_GRAD_LOG_PROB = 16.38
B_GRAD_VALUES = 0.0
B_GRAD_ENTROPY = 0.0
B_MOMENTS = 0.0


def depth(M):
    """Additions a term of a sum passes through: a lane's rows (at most four), six butterfly stages, two for the four waves, then ten
    per tree level (two for a lane's four leaves, six, two)."""
    rows = min(int(M), LEAF_ROWS)
    return -(-rows // nt.THREADS) + 6 + 2 + 10 * nt.tree_levels(-(-int(M) // LEAF_ROWS))


def launches(M):
    """Kernel launches of one forward: the leaves, then one per tree level."""
    return 1 + nt.tree_levels(-(-int(M) // LEAF_ROWS))


def leaf_sums(x):
    """x [M] float64 -> [ceil(M / 1024)]: a lane's rows in order from +0.0 (rows past the end padded with +0.0, which changes nothing:
    tests/norm_tree_host.py), the butterfly of each wave, then (w0 + w1) + (w2 + w3)."""
    x = np.asarray(x, np.float64)
    leaves = -(-x.shape[0] // LEAF_ROWS)
    v = nt._pad_rows(x, leaves * LEAF_ROWS).reshape(leaves, LEAF_ROWS // nt.THREADS, nt.THREADS)
    with np.errstate(all="ignore"):
        s = np.zeros((leaves, nt.THREADS))
        for j in range(v.shape[1]):
            s = s + v[:, j]
        w = nt.wave_tree_sum(s.reshape(leaves, nt.THREADS // nt.LANES, nt.LANES))
        return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def tree_sum(x):
    """x [M] -> the float64 sum the rule defines."""
    with np.errstate(all="ignore"):
        return nt.tree(leaf_sums(x)[:, None])[0]


def _f64(x):
    return None if x is None else np.asarray(x, np.float32).reshape(-1).astype(np.float64)


def canonical64(x):
    b = np.array(x, np.float64).reshape(-1).view(np.uint64).copy()
    b[np.isnan(b.view(np.float64))] = CANONICAL_NAN64
    return b.view(np.float64)


def advantage_moments(advantages, eps=1e-8):
    """-> float64 [2]: (mean, inv)."""
    x = _f64(advantages)
    Mf = np.float64(x.shape[0])
    with np.errstate(all="ignore"):
        S, Q = tree_sum(x), tree_sum(x * x)
        mean = S / Mf
        var = (Q - S * mean) / (Mf - 1.0)
        var = np.where(var < 0.0, 0.0, var)
        inv = 1.0 / (np.sqrt(var) + np.float64(eps))
    return canonical64([mean, inv])


def rows(log_prob, old_log_prob, advantages, moments=None, clip=0.2):
    """The per-row quantities of the rule -> dict of float64 / bool arrays [M]."""
    lp, old, adv = _f64(log_prob), _f64(old_log_prob), _f64(advantages)
    lo, hi = np.float64(1.0) - np.float64(clip), np.float64(1.0) + np.float64(clip)
    with np.errstate(all="ignore"):
        a = adv if moments is None else (adv - np.float64(moments[0])) * np.float64(moments[1])
        d = lp - old
        d = np.where(d < -RATIO_LOG_MAX, -RATIO_LOG_MAX, np.where(d > RATIO_LOG_MAX, RATIO_LOG_MAX, d))
        d_nan = np.isnan(d)
        r = np.where(d_nan, np.nan, EXP(np.where(d_nan, 0.0, d)))
        rc = np.where(r < lo, lo, np.where(r > hi, hi, r))
        s1 = r * a
        s2 = rc * a
        nan_row = np.isnan(s1) | np.isnan(s2)
        s = np.where(nan_row, np.nan, np.where(s2 < s1, s2, s1))
        passes = ((r >= lo) & (r <= hi)) | (s1 < s2)
        k1 = -d
        k3 = (r - 1.0) - d
        cf = np.where((r < lo) | (r > hi), 1.0, 0.0)
    return dict(a=a, d=d, r=r, rc=rc, s1=s1, s2=s2, s=s, nan_row=nan_row, passes=passes, k1=k1, k3=k3, cf=cf, lo=lo, hi=hi)


def clip_loss(log_prob, old_log_prob, advantages, *, clip=0.2, moments=None, entropy=None, entropy_coef=0.0, values=None, returns=None,
              value_coef=0.5):
    """-> (loss float64, stats float64 [8]), before the float32 rounding, and the sums in a dict."""
    p = rows(log_prob, old_log_prob, advantages, moments, clip)
    Mf = np.float64(p["s"].shape[0])
    ent, val, ret = _f64(entropy), _f64(values), _f64(returns)
    assert (val is None) == (ret is None)
    sums = {k: tree_sum(p[k]) for k in ("s", "k1", "k3", "cf")}
    with np.errstate(all="ignore"):
        policy_loss = -(sums["s"] / Mf)
        loss, value_loss, en = policy_loss, np.float64(0.0), np.float64(0.0)
        if val is not None:
            err = val - ret
            sums["v2"] = tree_sum(err * err)
            value_loss = 0.5 * (sums["v2"] / Mf)
            loss = loss + np.float64(value_coef) * value_loss
        if ent is not None:
            sums["ent"] = tree_sum(ent)
            en = sums["ent"] / Mf
            loss = loss - np.float64(entropy_coef) * en
        # the extrema skip a NaN ratio; a minimum and a maximum of numbers do not depend on the order of the selects
        ratio_min = np.fmin.reduce(p["r"], initial=np.inf)
        ratio_max = np.fmax.reduce(p["r"], initial=-np.inf)
        stats = np.array([policy_loss, value_loss, en, sums["k1"] / Mf, sums["k3"] / Mf, sums["cf"] / Mf, ratio_min, ratio_max], np.float64)
    return np.float64(loss), stats, sums


def clip_loss_f32(*args, **kw):
    """-> (loss, stats) as the device writes them: float32, NaNs canonical."""
    loss, stats, _ = clip_loss(*args, **kw)
    return to_f32(np.array([loss]))[0], to_f32(stats)


def clip_loss_backward(log_prob, old_log_prob, advantages, grad_loss, *, clip=0.2, moments=None, entropy=None, entropy_coef=0.0, values=None,
                       returns=None, value_coef=0.5):
    """-> (grad_log_prob, grad_entropy or None, grad_values or None) float64 [M], before the float32 rounding; grad_loss: the float32
    incoming gradient of the loss."""
    p = rows(log_prob, old_log_prob, advantages, moments, clip)
    M = p["s"].shape[0]
    val, ret = _f64(values), _f64(returns)
    with np.errstate(all="ignore"):
        gs = np.float64(np.float32(grad_loss)) / np.float64(M)
        g_lp = -(gs * np.where(p["passes"], p["a"] * p["r"], 0.0))
        g_lp = np.where(p["nan_row"], np.nan, g_lp)
        g_val = None if val is None else gs * (np.float64(value_coef) * (val - ret))
        g_ent = None if entropy is None else np.full(M, -(gs * np.float64(entropy_coef)))
    return g_lp, g_ent, g_val
