"""tests/gaussian_host.py — the NumPy twin of the Gaussian rule in include/mxv_policy.h, which the device is compared with bit for
bit — held to 200-bit mpmath: LOG, SINCOS2PI and EXP on their domains, the normals z, the float64 action, log_prob and entropy; the
exact steps of the argument reduction; the distribution of the draws; degenerate rows; what the rule promises structurally.  Also: the
constants in the kernel source are the generator's, and the Python front end validates without a device."""
import os
import re
import sys

import mpmath as mp
import numpy as np
import pytest

import gaussian_host as gh
from conftest import ROOT

DIMS = (1, 2, 3, 4)
ROWS = 3000
EXTREME_WORDS = (0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1)
QUADRANT_EDGES = tuple(sorted({(q * 2 ** 30 - 1) % 2 ** 32 for q in range(5)} | {(q * 2 ** 30) % 2 ** 32 for q in range(5)}))


def _ulps(got, exact):
    """|got - exact| in ulps of got (float64)."""
    got = float(got)
    return float(abs(mp.mpf(got) - exact) / mp.mpf(float(np.spacing(abs(got)))))


def _ulp32(v):
    v = float(v)
    if not np.isfinite(np.float32(v)):
        return float(np.spacing(np.finfo(np.float32).max))
    return float(np.spacing(np.abs(np.float32(v)))) if np.float32(v) != 0 else float(np.float32(2.0 ** -149))


def _measured(name, worst):
    """The named constant is what was measured on this input (to its two decimals, rounded up)."""
    b = getattr(gh, "B_" + name)
    print(f"measured B_{name}: {worst:.4f}")
    assert worst <= b < worst + 0.01, (name, worst, b)
    assert worst <= gh.bar(b)


def _words(n, seed, extra=()):
    w = np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64)
    return np.concatenate((w, np.asarray(extra, np.uint64))).astype(np.uint32)


def test_log_sequence_on_the_uniforms():
    w = _words(4000, 1, EXTREME_WORDS)
    u = gh.u01(w)
    assert np.all((u > 0) & (u < 1)) and u.min() == 2.0 ** -33
    L = gh.LOG(u)
    assert np.all(L < 0)
    with mp.workprec(200):
        worst = max(_ulps(b, mp.log(mp.mpf(float(a)))) for a, b in zip(u, L))
    _measured("LOG", worst)
    # the sequence of §12 on its own domain still gives what it gave
    assert gh.LOG(1.0) == 0.0 and gh.LOG(2.0) == float(gh.LN2_HI + gh.LN2_LO)


def test_sincos2pi_sequence_and_its_exact_steps():
    w = _words(4000, 2, EXTREME_WORDS + QUADRANT_EDGES)
    t, k, f, hi, r = gh.sincos_parts(w)
    sn, cs = gh.SINCOS2PI(w)
    worst_s = worst_c = 0.0
    with mp.workprec(200):
        for i, wi in enumerate(w.tolist()):
            v = (mp.mpf(wi) + mp.mpf("0.5")) / mp.mpf(2) ** 32
            assert mp.mpf(float(t[i])) == 4 * v                                                   # t = 4 v is exact
            assert float(k[i]) in (0.0, 1.0, 2.0, 3.0, 4.0) and abs(4 * v - mp.mpf(float(k[i]))) < mp.mpf("0.5")      # never a tie
            assert mp.mpf(float(f[i])) == 4 * v - mp.mpf(float(k[i]))                             # t - k is exact
            assert 2.0 ** -31 <= abs(float(f[i])) < 0.5
            assert mp.mpf(float(hi[i])) == mp.mpf(float(f[i])) * mp.mpf(float(gh.PIO2_HI))        # f * PIO2_HI is exact
            ang = 2 * mp.pi * v
            worst_s = max(worst_s, _ulps(sn[i], mp.sin(ang)))
            worst_c = max(worst_c, _ulps(cs[i], mp.cos(ang)))
    _measured("SIN", worst_s)
    _measured("COS", worst_c)
    assert float(gh.PIO2_HI) * 2 ** 19 == int(float(gh.PIO2_HI) * 2 ** 19) and 2 ** 19 <= float(gh.PIO2_HI) * 2 ** 19 < 2 ** 20
    assert np.all(np.abs(r) < 0.7854)


def test_exp_sequence_on_the_widened_domain():
    rng = np.random.default_rng(3)
    d = np.concatenate((rng.uniform(-80, 80, 4000), rng.uniform(-5, 2, 1000), [0.0, 80.0, -80.0, 1e-300, -1e-300, 0.5 * np.log(2.0)]))
    d = np.concatenate((d, d.astype(np.float32).astype(np.float64)))
    e = gh.EXP(d)
    with mp.workprec(200):
        worst = max(_ulps(b, mp.exp(mp.mpf(float(a)))) for a, b in zip(d, e))
    _measured("EXP", worst)
    assert gh.EXP(0.0) == 1.0
    f32 = np.finfo(np.float32)
    assert f32.tiny < gh.EXP(-80.0) and gh.EXP(80.0) < f32.max                                    # sigma stays a normal float32


def _rows(D):
    """The input the bars were measured on: means of scale 0.1 / 1 / 10, log_std uniform over [-5, 2], cast to float32."""
    rng = np.random.default_rng(200 + D)
    mean = (rng.standard_normal((ROWS, D)) * np.repeat((0.1, 1.0, 10.0), ROWS // 3)[:, None]).astype(np.float32)
    log_std = rng.uniform(-5.0, 2.0, (ROWS, D)).astype(np.float32)
    w4 = rng.integers(0, 2 ** 32, (ROWS, 4), dtype=np.uint64).astype(np.uint32)
    w4[:len(EXTREME_WORDS), 0] = EXTREME_WORDS
    w4[:len(EXTREME_WORDS), 2] = EXTREME_WORDS[::-1]
    w4[10:10 + len(QUADRANT_EDGES), 1] = QUADRANT_EDGES
    w4[10:10 + len(QUADRANT_EDGES), 3] = QUADRANT_EDGES[::-1]
    return mean, log_std, w4


@pytest.fixture(scope="module")
def exact():
    """Per D: the input, the twin's results and per row the exact (200-bit) z, float64 action, log_prob of the twin's float32 action
    and entropy."""
    out = {}
    with mp.workprec(200):
        for D in DIMS:
            mean, log_std, w4 = _rows(D)
            r = gh.evaluate(mean, log_std, w4)
            rows = []
            for i in range(ROWS):
                zs, acts, lp, en = [], [], mp.mpf(0), mp.mpf(0)
                for j in range(D):
                    wa, wb = int(w4[i, 2 * (j // 2)]), int(w4[i, 2 * (j // 2) + 1])
                    rad = mp.sqrt(-2 * mp.log((mp.mpf(wa) + mp.mpf("0.5")) / mp.mpf(2) ** 32))
                    ang = 2 * mp.pi * (mp.mpf(wb) + mp.mpf("0.5")) / mp.mpf(2) ** 32
                    z = rad * (mp.sin(ang) if j & 1 else mp.cos(ang))
                    mu, ls = mp.mpf(float(mean[i, j])), mp.mpf(float(log_std[i, j]))
                    sigma = mp.exp(ls)
                    zs.append(z)
                    acts.append((mu + sigma * z, abs(mu) + sigma * abs(z)))
                    zq = (mp.mpf(float(r["act"][i, j])) - mu) / sigma
                    lp += -zq * zq / 2 - ls - mp.log(2 * mp.pi) / 2
                    en += ls + mp.mpf("0.5") + mp.log(2 * mp.pi) / 2
                rows.append((zs, acts, lp, en))
            out[D] = (mean, log_std, w4, r, rows)
    return out


def test_normals_actions_log_prob_and_entropy_are_accurate(exact):
    worst = dict(Z_REL=0.0, Z_ABS=0.0, ACT=0.0, LOG_PROB=0.0, ENTROPY=0.0)
    two53 = mp.mpf(2) ** 53
    with mp.workprec(200):
        for D in DIMS:
            mean, log_std, w4, r, rows = exact[D]
            assert not r["degenerate"].any() and np.all(np.abs(r["z"]) < gh.Z_MAX)
            act32, lp32, en32 = gh.to_f32(r["act"]), gh.to_f32(r["log_prob"]), gh.to_f32(r["entropy"])
            for i, (zs, acts, lp, en) in enumerate(rows):
                for j in range(D):
                    worst["Z_REL"] = max(worst["Z_REL"], _ulps(r["z"][i, j], zs[j]))
                    worst["Z_ABS"] = max(worst["Z_ABS"], float(abs(mp.mpf(float(r["z"][i, j])) - zs[j]) * two53))
                    a, mag = acts[j]
                    worst["ACT"] = max(worst["ACT"], float(abs(mp.mpf(float(r["a"][i, j])) - a) / mag * two53))
                    # the float32 action: half a float32 ulp of the exact value plus the float64 bar
                    assert abs(mp.mpf(float(act32[i, j])) - a) <= mp.mpf(_ulp32(float(a))) / 2 + gh.bar(gh.B_ACT) * mag / two53, (D, i, j)
                worst["LOG_PROB"] = max(worst["LOG_PROB"], float(abs(mp.mpf(float(r["log_prob"][i])) - lp) * two53))
                worst["ENTROPY"] = max(worst["ENTROPY"], float(abs(mp.mpf(float(r["entropy"][i])) - en) * two53))
                assert abs(mp.mpf(float(lp32[i])) - lp) <= mp.mpf(_ulp32(float(lp))) / 2 + gh.bar(gh.B_LOG_PROB) / two53, (D, i)
                assert abs(mp.mpf(float(en32[i])) - en) <= mp.mpf(_ulp32(float(en))) / 2 + gh.bar(gh.B_ENTROPY) / two53, (D, i)
    for name, v in worst.items():
        _measured(name, v)


def test_the_range_of_the_normals():
    """|z| <= sqrt(2 * 33 ln 2) < 6.77: the smallest uniform is 2^-33, and |sin|, |cos| <= 1 up to their last bit."""
    w = np.asarray(EXTREME_WORDS + QUADRANT_EDGES, np.uint32)
    ze, zo = gh.normal_pair(np.zeros_like(w), w)
    assert max(np.abs(ze).max(), np.abs(zo).max()) < gh.Z_MAX and np.sqrt(2 * 33 * np.log(2.0)) < gh.Z_MAX
    assert np.abs(ze).max() > 6.76                                       # w = 0 next to a quadrant edge reaches the bound
    sn, cs = gh.SINCOS2PI(_words(20000, 9, EXTREME_WORDS + QUADRANT_EDGES))
    assert np.all(np.abs(sn) <= 1.0) and np.all(np.abs(cs) <= 1.0)


# the 8 equiprobable bins of a standard normal: the edges are its octiles
_OCTILES = (-1.1503493803760079, -0.6744897501960817, -0.31863936396437514, 0.0, 0.31863936396437514, 0.6744897501960817, 1.1503493803760079)


def _check_normals(z, what):
    n = z.size
    with mp.workprec(100):
        assert all(abs(float(mp.ncdf(e)) - (i + 1) / 8) < 1e-12 for i, e in enumerate(_OCTILES))
    assert abs(z.mean()) <= 5 / np.sqrt(n), (what, z.mean())
    assert abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / n), (what, z.var())                 # var of z^2 is 2
    counts = np.bincount(np.searchsorted(_OCTILES, z), minlength=8)
    assert np.all(np.abs(counts - n / 8) <= 5 * np.sqrt(n * (1 / 8) * (7 / 8))), (what, counts)


def test_distribution_over_envs_and_over_steps():
    n = 1 << 16
    over_envs = gh.words(2024, range(5, 5 + n), 3)
    over_steps = np.concatenate([gh.words(99, [77], t) for t in range(n)])
    for what, w4 in (("envs", over_envs), ("steps", over_steps)):
        z0, z1 = gh.normal_pair(w4[:, 0], w4[:, 1])
        z2, z3 = gh.normal_pair(w4[:, 2], w4[:, 3])
        for k, z in enumerate((z0, z1, z2, z3)):
            _check_normals(z, (what, k))
        for a, b in ((z0, z1), (z2, z3), (z0, z2), (z1, z3)):
            assert abs(np.corrcoef(a, b)[0, 1]) <= 5 / np.sqrt(n), what
    # through the rule: a = mu + sigma z, so (a - mu) / sigma is z up to the float32 rounding of the action
    mu = np.full((n, 2), 0.5, np.float32)
    r = gh.evaluate(mu, np.asarray([-1.0, 0.25], np.float32), over_envs)
    _check_normals(r["zq"][:, 0], "zq0")
    _check_normals(r["zq"][:, 1], "zq1")


def test_a_draw_depends_on_seed_env_and_step_alone():
    rng = np.random.default_rng(11)
    mean = rng.standard_normal((301, 3)).astype(np.float32)
    ls = rng.uniform(-2, 1, (301, 3)).astype(np.float32)
    off, cut = 1001, 130
    whole = gh.sample_gaussian(mean, ls, seed=9, step=12, env_offset=off)
    a = gh.sample_gaussian(mean[:cut], ls[:cut], seed=9, step=12, env_offset=off)
    b = gh.sample_gaussian(mean[cut:], ls[cut:], seed=9, step=12, env_offset=off + cut)
    for k in range(3):
        assert np.array_equal(gh.bits(whole[k]), np.concatenate((gh.bits(a[k]), gh.bits(b[k]))))
    # dims 0..D-1 of a narrower head are the first D of a wider one's
    narrow = gh.sample_gaussian(mean[:, :2], ls[:, :2], seed=9, step=12, env_offset=off)
    assert np.array_equal(gh.bits(narrow[0]), gh.bits(whole[0][:, :2]))
    # a shared [D] row is the [N, D] one broadcast
    shared = gh.sample_gaussian(mean, ls[0], seed=9, step=12, env_offset=off)
    full = gh.sample_gaussian(mean, np.broadcast_to(ls[0], ls.shape), seed=9, step=12, env_offset=off)
    assert all(np.array_equal(gh.bits(x), gh.bits(y)) for x, y in zip(shared, full))
    G = list(range(64))
    assert not np.array_equal(gh.words(9, G, 12), gh.words(10, G, 12))
    assert not np.array_equal(gh.words(9, G, 12), gh.words(9, G, 13))
    assert not np.array_equal(gh.words(9, G, 12), gh.words(9, [g + 64 for g in G], 12))


def test_the_high_words_and_the_stream_tag():
    from oracle import oracle

    import policy_host as ph

    for G, t in ((3, 5), (2 ** 32 + 3, 2 ** 32 + 5), (2 ** 63 + 1, 2 ** 61 + 2 ** 32 + 5)):
        ctr = (G & 0xffffffff, G >> 32, t & 0xffffffff, ((t >> 32) & 0x0fffffff) | (8 << 28))
        assert np.array_equal(gh.words(1, [G], t)[0], oracle.philox4x32_10(ctr, (1, 0)))
    assert not np.array_equal(gh.words(1, [3], 5), gh.words(1, [3], 2 ** 32 + 5))
    assert not np.array_equal(gh.words(1, [3], 5), gh.words(1, [2 ** 32 + 3], 5))
    assert np.array_equal(gh.words(1, [3], 5), gh.words(1, [3], 2 ** 60 + 5))          # bits 28 and up of t_hi belong to the stream tag
    # the categorical draws (tag 7) and the engine's action stream (tag 1) under the same key and counter are other streams
    assert gh.STREAM_GAUSSIAN == 8 != ph.STREAM_POLICY
    assert not np.array_equal(oracle.philox4x32_10((3, 0, 5, 7 << 28), (1, 0)), gh.words(1, [3], 5)[0])
    assert not np.array_equal(oracle.philox4x32_10((3, 0, 5, 1 << 28), (1, 0)), gh.words(1, [3], 5)[0])


def test_degenerate_and_extreme_rows():
    inf, nan = np.inf, np.nan
    mean = np.asarray([[nan, 0], [0, inf], [-inf, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [1e30, 0], [3e38, -3e38], [1.5, -2.5]], np.float32)
    ls = np.asarray([[0, 0], [0, 0], [0, 0], [nan, 0], [0, 80.0001], [-80.0001, 0], [inf, 0], [0, -inf], [0, 0], [2, 2], [80, -80]], np.float32)
    act, lp, en = gh.sample_gaussian(mean, ls, seed=4, step=1)
    bad = np.arange(8)
    assert np.all(gh.bits(act[bad]) == gh.CANONICAL_NAN) and np.all(gh.bits(lp[bad]) == gh.CANONICAL_NAN)
    assert np.all(gh.bits(en[bad]) == gh.CANONICAL_NAN)
    r = gh.evaluate(mean, ls, gh.words(4, range(11), 1))
    assert np.array_equal(r["degenerate"], np.arange(11) < 8)
    assert np.all(np.isfinite(r["sigma"])) and np.all(np.isfinite(r["z"]))             # the rows' own arithmetic stays finite
    # 1e30 swallows sigma z: the action is the mean, zq = 0
    assert act[8, 0] == np.float32(1e30) and np.isfinite(lp[8]) and en[8] == np.float32(2 * float(gh.ENT_C))
    # 3e38 + sigma z stays finite here (|sigma z| < 50); the row is ordinary
    assert np.all(np.isfinite(act[9])) and np.isfinite(lp[9])
    # log_std = +-80 is inside the domain: sigma = EXP(+-80) is a normal float32, the action finite, the entropy that of ls = 80 - 80
    assert np.all(np.isfinite(act[10])) and np.isfinite(lp[10])
    e10 = (np.float64(0.0) + (np.float64(80.0) + gh.ENT_C)) + (np.float64(-80.0) + gh.ENT_C)
    assert en[10] == np.float32(e10)
    # an action that rounds to +-Inf follows from the arithmetic: log_prob = -Inf, no NaN
    big = gh.evaluate(np.asarray([[3.4e38]], np.float32), np.asarray([[80.0]], np.float32), np.asarray([[0, 0, 0, 0]], np.uint32))
    assert big["z"][0, 0] > 6.7 and np.isposinf(big["act"][0, 0]) and np.isneginf(big["log_prob"][0]) and not big["degenerate"][0]
    assert gh.bits(gh.to_f32(big["log_prob"]))[0] == 0xFF800000


def test_the_kernel_source_carries_the_generated_constants():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gaussian_coefficients
        import policy_coefficients
    finally:
        sys.path.pop(0)
    block, src = gh.rule_block("mxv_gaussian.hip")
    assert block == gaussian_coefficients.block() and block.startswith(policy_coefficients.block() + "\n")
    # the shared constants are the categorical rule's, value for value
    g, p = gaussian_coefficients.constants(), policy_coefficients.constants()
    assert all(g[k] == p[k] for k in p) and gaussian_coefficients.block().startswith(policy_coefficients.block())
    with mp.workprec(300):
        for name, want in (("pio2_lo", mp.pi / 2 - mp.mpf(g["pio2_hi"])), ("half_log_2pi", mp.log(2 * mp.pi) / 2),
                           ("ent_c", mp.mpf("0.5") + mp.log(2 * mp.pi) / 2)):
            assert abs(mp.mpf(g[name]) - want) <= mp.mpf(float(np.spacing(abs(g[name])))) / 2, name      # rounded once
        assert mp.mpf(g["pio2_hi"]) == mp.floor(mp.pi / 2 * 2 ** 19) / 2 ** 19
    tag = re.search(r"kStreamGaussian = (\d+)u", src)
    assert tag and int(tag.group(1)) == gh.STREAM_GAUSSIAN == 8
    assert "8<<28" in open(os.path.join(ROOT, "include", "mxv.h")).read().replace(" ", "")
    assert "8<<28" in open(os.path.join(ROOT, "include", "mxv_policy.h")).read().replace(" ", "")


def test_the_front_end_validates_without_a_device():
    import subprocess

    code = ("import sys; import gym_amd.policy as p; assert 'torch' not in sys.modules; import gym_amd; "
            "assert gym_amd.sample_gaussian is p.sample_gaussian and gym_amd.GaussianSampler is p.GaussianSampler; "
            "assert 'torch' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
    import torch

    from gym_amd import _native, policy
    from gym_amd.returns import GAE_EXPORTS

    assert "mxv_policy_sample_gaussian" in policy.POLICY_EXPORTS and len(policy.POLICY_EXPORTS) == 4
    assert not set(policy.POLICY_EXPORTS) & (set(_native.EXPORTS) | set(GAE_EXPORTS))
    m, s = torch.zeros((4, 3)), torch.zeros((4, 3))
    f32 = torch.float32
    for kw, what in ((dict(mean=m.double()), "float32"), (dict(mean=m[0]), "shape"), (dict(mean=torch.zeros((4, 5)), log_std=torch.zeros((4, 5))), "shape"),
                     (dict(mean=torch.zeros((0, 3))), "shape"), (dict(mean=torch.zeros((3, 4)).t()), "contiguous"),
                     (dict(log_std=s.double()), "float32"), (dict(log_std=torch.zeros((4, 2))), "log_std"), (dict(log_std=torch.zeros(4)), "log_std"),
                     (dict(log_std=torch.zeros((3, 4)).t()), "contiguous"), (dict(log_std=torch.zeros(6)[::2]), "contiguous"),
                     (dict(log_std=[0.0, 0.0, 0.0]), "torch tensor"),
                     (dict(seed=-1), "seed"), (dict(seed=1.5), "seed"), (dict(step=True), "step"),
                     (dict(step=torch.zeros(1, dtype=torch.int32)), "int64"), (dict(env_offset=2 ** 64), "env_offset"),
                     (dict(out=(torch.zeros((4, 3)),)), "3 entries"), (dict(out=(torch.zeros((5, 3)), None, None)), "shape"),
                     (dict(out=(torch.zeros((4, 3), dtype=torch.float64), None, None)), "float32"),
                     (dict(out=(torch.zeros((3, 4)).t(), None, None)), "contiguous"),
                     (dict(out=(torch.zeros((4, 3)), torch.zeros(4, dtype=torch.float64), None)), "float32"),
                     (dict(out=(torch.zeros((4, 3)), None, torch.zeros(5, dtype=f32))), "shape"),
                     (dict(), "device tensor")):
        args = dict(mean=m, log_std=s, seed=0, step=0)
        args.update(kw)
        mean, log_std = args.pop("mean"), args.pop("log_std")
        with pytest.raises(ValueError, match=what):
            policy.sample_gaussian(mean, log_std, **args)
    for bad in (0, 5, True, 2.0):
        with pytest.raises(ValueError, match="action_dim"):
            policy.GaussianSampler(bad)
