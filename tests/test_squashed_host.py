"""tests/squashed_host.py — the NumPy twin of the rule in include/mxv_squashed.h, which the device is compared with bit for bit — held
to 200-bit mpmath: tanh, the correction log(1 - tanh^2), log_prob and both gradients before their float32 rounding, over |u| from 2^-40
to 2^9 with the switch at 2^-27, the cut of E at v = 354, log_std = +-80 and |z| at Z_MAX; what the rule promises structurally, checked
exactly; and the closed-form gradients against torch's float64 autograd of the textbook formula."""
import mpmath as mp
import numpy as np
import pytest

import squashed_host as sh

DIMS = (1, 2, 3, 4)
TWO53 = 2.0 ** 53


def _measured(name, worst):
    """The named constant is what was measured on this input (to its two decimals, rounded up)."""
    b = getattr(sh, "B_" + name)
    print(f"measured B_{name}: {worst:.4f}")
    assert worst <= b < worst + 0.01, (name, worst, b)
    assert worst <= sh.bar(b)


def _ulp32(v):
    v = float(v)
    return float(np.spacing(np.abs(np.float32(v)))) if np.float32(v) != 0 else float(np.float32(2.0 ** -149))


def _pred(x):
    return float(np.nextafter(np.float64(x), 0.0))


def _succ(x):
    return float(np.nextafter(np.float64(x), np.inf))


def _grid():
    """|u| over 2^-40 .. 2^9, log-uniform, with the points where the rule changes its path."""
    rng = np.random.default_rng(11)
    v = 2.0 ** rng.uniform(-40, 9, 3000)
    special = [2.0 ** -40, 2.0 ** -27, _pred(2.0 ** -27), _succ(2.0 ** -27), 2.0 ** -26, 354.0, _pred(354.0), _succ(354.0), 353.0, 355.0,
               512.0, 18.0, 19.0, 0.5 * np.log(2.0), 1.0, 9.0, 9.5]
    return np.sort(np.concatenate((v, special)))


def test_tanh_and_the_correction_on_their_whole_range():
    v = _grid()
    r = sh.squash(np.zeros_like(v), np.zeros_like(v), v)      # sigma = 1 exactly, u = v
    assert np.array_equal(r["v"], v) and sh.EXP(0.0) == 1.0
    th, q = r["th"], r["q"]
    corr = 2.0 * ((sh.LN2 - v) - sh.LOG(q))
    worst_t = worst_c = 0.0
    with mp.workprec(200):
        for i, vi in enumerate(v.tolist()):
            t = mp.tanh(mp.mpf(vi))
            worst_t = max(worst_t, float(abs(mp.mpf(float(th[i])) - t) * TWO53))
            c = mp.log(1 - t * t) if vi < 30 else mp.log(4) - 2 * mp.mpf(vi) - 2 * mp.log1p(mp.exp(-2 * mp.mpf(vi)))
            worst_c = max(worst_c, float(abs(mp.mpf(float(corr[i])) - c) / (1 + abs(c)) * TWO53))
            # the float32 tanh: within one float32 ulp everywhere, also where the select takes v itself
            assert abs(mp.mpf(float(np.float32(th[i]))) - t) <= _ulp32(float(t)), vi
    _measured("TANH", worst_t)
    _measured("CORR", worst_c)
    # structure, exactly: th is monotone in v, never above 1, exactly 1 once e == 0, and v itself below 2^-27
    assert np.all(np.diff(th) >= 0) and np.all((th >= 0) & (th <= 1.0))
    assert np.all(th[v < 2.0 ** -27] == v[v < 2.0 ** -27])
    assert np.all(r["e"][v > sh.E_CUT_V] == 0.0) and np.all(r["e"][v <= sh.E_CUT_V] > 0.0) and np.all(th[v > sh.E_CUT_V] == 1.0)
    assert np.all(np.isfinite(corr)) and np.all(corr <= 4 * 2.0 ** -53)      # log(1 - tanh^2) <= 0, up to the roundings of its terms near 0
    # corr is finite for every finite u: up to the largest double a float32 mean and sigma = EXP(80) can give
    big = np.asarray([1e3, 1e30, 3.5e38, float(np.finfo(np.float32).max) + float(sh.EXP(80.0)) * sh.Z_MAX])
    rb = sh.squash(big, np.zeros(4), np.zeros(4))
    cb = 2.0 * ((sh.LN2 - rb["v"]) - sh.LOG(rb["q"]))
    assert np.all(np.isfinite(cb)) and np.all(rb["t"] == 1.0) and np.all(cb == 2.0 * (sh.LN2 - big))


def _rows(D):
    """The input the bars were measured on: pre-squash values over the whole range — the mean carries +-2^k, k in [-40, 9], the noise
    is sigma z with log_std over [-5, 2] — and, at the end, rows with log_std = +-80, |z| at Z_MAX, the switch and the cut."""
    rng = np.random.default_rng(300 + D)
    n = 1200
    mean = (np.sign(rng.standard_normal((n, D))) * 2.0 ** rng.uniform(-40, 9, (n, D))).astype(np.float32)
    log_std = rng.uniform(-5.0, 2.0, (n, D)).astype(np.float32)
    log_std[n // 2:] -= 40.0                                  # half the rows: u = mean up to a tiny noise, the grid of the mean itself
    z = rng.standard_normal((n, D))
    edge_mu = np.asarray([0.0, 0.0, 354.0, -354.0, 355.0, 2.0 ** -27, _pred(2.0 ** -27), -2.0 ** -27, 0.0, 0.0, 1.0, -512.0], np.float32)
    edge_ls = np.asarray([80.0, -80.0, -80.0, -80.0, 0.0, -80.0, -80.0, -80.0, 0.0, 80.0, 2.0, -3.0], np.float32)
    edge_z = np.asarray([1e-30, 1.0, 1.0, -1.0, 0.5, 1.0, -1.0, 1.0, sh.Z_MAX, -sh.Z_MAX, sh.Z_MAX, -sh.Z_MAX])
    mean = np.concatenate((mean, np.repeat(edge_mu[:, None], D, 1)))
    log_std = np.concatenate((log_std, np.repeat(edge_ls[:, None], D, 1)))
    z = np.concatenate((z, np.repeat(edge_z[:, None], D, 1)))
    N = len(mean)
    scale = np.asarray([2.0, 1.0, 0.375, 64.0][:D], np.float32)
    bias = np.asarray([0.0, -0.5, 3.0, 100.0][:D], np.float32)
    ga = rng.standard_normal((N, D)).astype(np.float32)
    glp = rng.standard_normal(N).astype(np.float32)
    return mean, log_std, z, scale, bias, ga, glp


def _scales(f, b):
    """What the errors of log_prob and of the gradients are measured in, per row (log_prob) or element, times 2^-53: the magnitudes of the
    terms that are added, and the first-order effect of the rounding of u = mu + sigma z, which is |n| + |u| ulps' worth, on each."""
    z, ls, n, u, corr = f["z"], f["ls"], np.abs(f["n"]), np.abs(f["u"]), np.abs(f["corr"])
    lp = (0.5 * z * z + np.abs(ls) + 1.0 + np.abs(sh.LOG(f["scale"])) + corr + n + u).sum(1)
    w = np.abs(b["ga"] * b["scale"]) * b["s"] + np.abs(b["glp"])
    return lp, w * (1.0 + n + u), w * (1.0 + n) * (1.0 + n + u)


def _accuracy(D):
    mean, log_std, z, scale, bias, ga, glp = _rows(D)
    f = sh.evaluate(mean, log_std, None, scale, bias, z=z)
    b = sh.gradients(mean, log_std, None, ga, glp, scale, z=z)
    assert not f["degenerate"].any() and np.all(np.isfinite(f["log_prob"])) and np.all(np.isfinite(b["grad_mean"]))
    v = f["v"]
    assert v.min() < 2.0 ** -39 and v.max() > 2.0 ** 9 and (v > sh.E_CUT_V).any() and (v < 2.0 ** -27).any()
    s_lp, s_gm, s_gls = _scales(f, b)
    worst = dict(LOG_PROB=0.0, GRAD_MEAN=0.0, GRAD_LOG_STD=0.0)
    lp32 = sh.to_f32(f["log_prob"])
    with mp.workprec(200):
        for i in range(len(mean)):
            lp = mp.mpf(0)
            for j in range(D):
                mu, ls, zz, sc = (mp.mpf(float(x)) for x in (mean[i, j], log_std[i, j], z[i, j], scale[j]))
                n = mp.exp(ls) * zz
                u = mu + n
                t = mp.tanh(u)
                va = abs(u)
                corr = mp.log(1 - t * t) if va < 30 else mp.log(4) - 2 * va - 2 * mp.log1p(mp.exp(-2 * va))
                s = 1 - t * t if va < 30 else 4 * mp.exp(-2 * va) / (1 + mp.exp(-2 * va)) ** 2
                lp += -zz * zz / 2 - ls - mp.log(2 * mp.pi) / 2 - mp.log(sc) - corr
                g, gl = mp.mpf(float(ga[i, j])) * sc, mp.mpf(float(glp[i]))
                gm = g * s + gl * 2 * t
                gls = g * s * n + gl * (2 * t * n - 1)
                worst["GRAD_MEAN"] = max(worst["GRAD_MEAN"], float(abs(mp.mpf(float(b["grad_mean"][i, j])) - gm) / mp.mpf(float(s_gm[i, j])) * TWO53))
                worst["GRAD_LOG_STD"] = max(worst["GRAD_LOG_STD"],
                                            float(abs(mp.mpf(float(b["grad_log_std"][i, j])) - gls) / mp.mpf(float(s_gls[i, j])) * TWO53))
            worst["LOG_PROB"] = max(worst["LOG_PROB"], float(abs(mp.mpf(float(f["log_prob"][i])) - lp) / mp.mpf(float(s_lp[i])) * TWO53))
            assert abs(mp.mpf(float(lp32[i])) - lp) <= mp.mpf(_ulp32(float(lp))) / 2 + sh.bar(sh.B_LOG_PROB) * s_lp[i] / TWO53, (D, i)
    return worst


def test_log_prob_and_gradients_are_accurate():
    worst = {}
    for D in DIMS:
        w = _accuracy(D)
        print(D, w)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
    for name, w in worst.items():
        _measured(name, w)


@pytest.mark.parametrize("D", DIMS)
def test_structural_promises(D):
    mean, log_std, z, scale, bias, ga, glp = _rows(D)
    f = sh.evaluate(mean, log_std, None, scale, bias, z=z)
    assert np.all(np.abs(f["t"]) <= 1.0) and np.all(np.sign(f["t"]) == np.sign(f["u"]))
    sc, bi = scale.astype(np.float64), bias.astype(np.float64)
    # every action lies within [bias - scale, bias + scale] as float32 rounds the ends, and is exactly an end once e == 0
    lo, hi = (bi - sc).astype(np.float32), (bi + sc).astype(np.float32)
    assert np.all((f["act"] >= lo) & (f["act"] <= hi))
    sat = f["e"] == 0.0
    assert sat.any() and np.array_equal(f["act"][sat], np.where(f["u"] > 0, hi, lo)[sat])
    assert np.all(np.isfinite(f["corr"]))
    # absent gradients are zeros, bit for bit
    N = len(mean)
    for kw_none, kw_zero in ((dict(grad_actions=None, grad_log_prob=glp), dict(grad_actions=np.zeros((N, D), np.float32), grad_log_prob=glp)),
                             (dict(grad_actions=ga, grad_log_prob=None), dict(grad_actions=ga, grad_log_prob=np.zeros(N, np.float32)))):
        a, b = sh.gradients(mean, log_std, None, scale=scale, z=z, **kw_none), sh.gradients(mean, log_std, None, scale=scale, z=z, **kw_zero)
        for k in ("grad_mean", "grad_log_std"):
            assert np.array_equal(sh.bits(sh.to_f32(a[k])), sh.bits(sh.to_f32(b[k]))), k


def test_degenerate_rows_are_nan_and_only_they():
    inf, nan = np.inf, np.nan
    D = 3
    rng = np.random.default_rng(5)
    mean = rng.standard_normal((40, D)).astype(np.float32)
    ls = rng.uniform(-2, 1, (40, D)).astype(np.float32)
    bad = {}
    for k, (mv, sv) in enumerate(((nan, None), (inf, None), (-inf, None), (None, nan), (None, 80.0001), (None, -80.0001), (None, inf), (None, -inf))):
        row, at = 3 + 4 * k, k % D
        if mv is not None:
            mean[row, at] = mv
        else:
            ls[row, at] = sv
        bad[row] = True
    ls[1, 0], ls[2, 1] = 80.0, -80.0                           # the ends of the range are good rows
    mean[5, 0] = np.finfo(np.float32).max
    is_bad = np.asarray([i in bad for i in range(40)])
    act, lp = sh.sample(mean, ls, seed=3, step=4, env_offset=2, scale=[2.0, 1.0, 0.5], bias=[0.0, 1.0, -1.0])
    gm, gls = sh.sample_backward(mean, ls, seed=3, step=4, env_offset=2, scale=[2.0, 1.0, 0.5], grad_actions=np.ones((40, D), np.float32),
                                 grad_log_prob=np.ones(40, np.float32))
    for x in (act, gm, gls):
        assert np.all(sh.bits(x)[is_bad] == 0x7FC00000) and not np.isnan(x[~is_bad]).any()
    assert np.all(sh.bits(lp)[is_bad] == 0x7FC00000) and not np.isnan(lp[~is_bad]).any()
    assert lp[5] == np.inf      # u at float32's largest: the density of the saturated action is past float32's range, which is what is written
    # a shared log_std row that is bad makes every row degenerate
    act, lp = sh.sample(mean[:4], np.asarray([0.0, nan, 0.0], np.float32), seed=3, step=4)
    assert np.all(sh.bits(act) == 0x7FC00000) and np.all(sh.bits(lp) == 0x7FC00000)


def test_a_draw_depends_on_seed_row_and_step_alone_under_tag_11():
    import gaussian_host as gh

    mean = np.zeros((6, 4), np.float32)
    ls = np.zeros(4, np.float32)
    whole = sh.sample(mean, ls, seed=9, step=2 ** 32 + 1, env_offset=0)
    part = sh.sample(mean[:3], ls, seed=9, step=2 ** 32 + 1, env_offset=3)
    assert np.array_equal(sh.bits(whole[0][3:]), sh.bits(part[0])) and np.array_equal(sh.bits(whole[1][3:]), sh.bits(part[1]))
    assert not np.array_equal(whole[0], sh.sample(mean, ls, seed=9, step=2 ** 32 + 2)[0])
    assert not np.array_equal(whole[0], sh.sample(mean, ls, seed=10, step=2 ** 32 + 1)[0])
    # the counter layout of tag 8 under tag 11: other words than the Gaussian sampler's, and the high step bits below the tag count
    assert sh.STREAM_SQUASHED == 11 and not np.array_equal(sh.words(9, range(6), 5), gh.words(9, range(6), 5))
    assert not np.array_equal(sh.words(9, range(6), 5), sh.words(9, range(6), 5 + 2 ** 32))
    assert np.array_equal(sh.words(9, range(6), 5), sh.words(9, range(6), 5 + 2 ** 60))
    # with mean 0, log_std 0, scale 1: the action is tanh(z), and atanh recovers standard normals
    act, _ = sh.sample(np.zeros((4000, 2), np.float32), np.zeros(2, np.float32), seed=1, step=0)
    zr = np.arctanh(act.astype(np.float64)[np.abs(act) < 1])
    assert abs(zr.mean()) < 5 / np.sqrt(zr.size) and abs(zr.var() - 1) < 0.05


@pytest.mark.parametrize("D", DIMS)
def test_gradients_agree_with_torch_autograd_of_the_textbook_formula(D):
    """grad_mean and grad_log_std against torch's float64 autograd of
        u = mu + exp(ls) z;  a = bias + scale tanh(u);  lp = sum_j Normal(mu, exp ls).log_prob(u) - log scale - log(1 - tanh(u)^2)
    on the twin's own z, with the loss sum(ga * a) + sum(glp * lp).

    Tolerance, with eps = 2^-53.  The twin is within bar(B_GRAD_*) eps of the exact value in the units of _scales (held above):
    (|ga scale| s + |glp|) (1 + |n| + |u|) for grad_mean, and (1 + |n|) times that for grad_log_std.  torch reaches the same derivatives
    by the chain rule in float64: exp, tanh and log from libm (1 ulp each), about ten multiplications and additions per path, and the
    same first-order sensitivity to the rounding of u — each at most eps times the same magnitudes, fewer than 16 of them.  Two things
    are torch's alone.  (1) Its log(1 - tanh^2) passes the gradient through 1 / (1 - t^2) and tanh's own (1 - t^2), two roundings of
    one quantity whose relative error eps / s grows as the tanh saturates: the rows are kept to |u| <= 15 (s >= 3.7e-13), and the
    term |glp| 2 |t| carries 2 eps / s relative, which the bound below writes as 4 eps |glp| / s.  (2) Normal.log_prob sees u and mu as
    separate arguments and recovers the noise as u - mu = n (1 + d), |d| <= eps |u| / |n| (u was rounded at its own magnitude).  The
    gradient with respect to mu arrives as +(u - mu) / sigma^2 directly and as its negative through u: two quotients of magnitude
    |z| / sigma that cancel to eps times that, 4 eps |glp| |z| / sigma with their roundings.  With respect to log_std it arrives as
    (u - mu)^2 / sigma^2 through sigma and as -(u - mu) z / sigma through u: z^2 (1 + 2 d) - z^2 (1 + d) = z^2 d, that is
    eps |glp| |z| |u| / sigma, doubled for the second order, next to 4 eps |glp| z^2 for the roundings of the quotients.  That is why
    the rows are those with log_std in [-5, 2]: at log_std = -45 torch's own gradient is rounding noise.  (3) tanh's backward forms
    1 - y * y from the rounded y = tanh(u): y carries eps, y * y 2 eps and the subtraction eps / 2 more, absolute, whatever s is — under
    4 eps |ga scale| on grad_mean and |n| times that on grad_log_std, where the twin's s = 4 e / q^2 keeps its relative accuracy.  So
        |twin - torch| <= eps ((bar(B) + 16) scale + 4 |glp| (1 / s + |z| / sigma) + 4 |ga scale|)                            for grad_mean,
                          eps ((bar(B) + 16) scale + 4 |glp| (|n| / s + z^2) + 2 |glp| |z| |u| / sigma + 4 |ga scale| |n|)    for grad_log_std."""
    import torch

    mean, log_std, z, scale, bias, ga, glp = _rows(D)
    f = sh.evaluate(mean, log_std, None, scale, bias, z=z)
    keep = (np.abs(f["u"]) <= 15.0).all(1) & (log_std >= -5.0).all(1)
    assert keep.sum() > 300
    mean, log_std, z, ga, glp = mean[keep], log_std[keep], z[keep], ga[keep], glp[keep]
    f = sh.evaluate(mean, log_std, None, scale, bias, z=z)
    b = sh.gradients(mean, log_std, None, ga, glp, scale, z=z)
    mu = torch.from_numpy(mean.astype(np.float64)).requires_grad_()
    ls = torch.from_numpy(log_std.astype(np.float64)).requires_grad_()
    zt, sc, bi = torch.from_numpy(z), torch.from_numpy(scale.astype(np.float64)), torch.from_numpy(bias.astype(np.float64))
    u = mu + ls.exp() * zt
    a = bi + sc * torch.tanh(u)
    lp = (torch.distributions.Normal(mu, ls.exp()).log_prob(u) - sc.log() - torch.log(1 - torch.tanh(u) ** 2)).sum(-1)
    ((torch.from_numpy(ga.astype(np.float64)) * a).sum() + (torch.from_numpy(glp.astype(np.float64)) * lp).sum()).backward()
    _, s_gm, s_gls = _scales(f, b)
    eps = 2.0 ** -53
    absz, glp_c = np.abs(z), np.abs(glp.astype(np.float64))[:, None]
    gas = np.abs(b["ga"] * b["scale"])
    tol_m = eps * ((sh.bar(sh.B_GRAD_MEAN) + 16) * s_gm + 4 * glp_c * (1 / b["s"] + absz / f["sigma"]) + 4 * gas)
    tol_s = eps * ((sh.bar(sh.B_GRAD_LOG_STD) + 16) * s_gls + 4 * glp_c * (np.abs(f["n"]) / b["s"] + absz * absz)
                   + 2 * glp_c * absz * np.abs(f["u"]) / f["sigma"] + 4 * gas * np.abs(f["n"]))
    err_m = np.abs(b["grad_mean"] - mu.grad.numpy())
    err_s = np.abs(b["grad_log_std"] - ls.grad.numpy())
    print(f"D={D}: worst grad_mean error / tolerance {np.max(err_m / tol_m):.3f}, grad_log_std {np.max(err_s / tol_s):.3f}; "
          f"absolute {err_m.max():.2e}, {err_s.max():.2e}")
    assert np.all(err_m <= tol_m), np.max(err_m / tol_m)
    assert np.all(err_s <= tol_s), np.max(err_s / tol_s)
    # and the float64 action is torch's to the same standard: |a - torch| <= 4 eps (|bias| + scale)
    assert np.all(np.abs(f["a"] - a.detach().numpy()) <= 4 * eps * (np.abs(bias) + scale))
