"""A NumPy twin of gym_amd/csrc/mxv_subnorm.hip: the rule, the guards, the two kernels' walks, and the input lists of the edge tests.

  update / normalise     the reference's update_mean_var_count_from_moments (gym/wrappers/normalize.py:32-47) with a batch of one row,
                         written literally — m_b included, one NumPy float64 operation per reference operation — and :93 / :145.
  plain_* / short_count  the guards of mxv_divide.hpp and the kernels' count test, restated on the host.
  obs_walk / rew_walk    what the kernels do with those: per wave of 64 envs, iteration i handles event i of every lane that still has one;
                         the path of that wave-iteration follows from the guards over the lanes at work.
  div_shared_host        mxv_divide.hpp's div_shared with exact rational arithmetic under every fma: finds operands on which the short form and
                         `/` differ (an input on which they agree cannot test a guard).
  *_cases                the inputs that tests/test_subnorm_host.py (oracle against this twin, path conditions; no GPU) and
                         tests/test_gpu_subnorm_edges.py (device against the oracle) share.

Both walks return a report: one (wave, iteration, path, mixed) per wave-iteration.  `mixed` says that unanimity was not a given:
  PLAIN   some lane at work passes the first vote alone (the others drag it down the plain path);
  M2      some lane at work passes the second vote alone;
  SHORT   every lane at work passes both votes, and the wave either took another path at an earlier iteration of the call (the vote is taken
          again at every iteration) or holds a lane that is through whose count alone fails the first vote (the votes count the lanes at work).
"""
from fractions import Fraction

import numpy as np

WAVE = 64
SHORT, PLAIN, M2 = "short", "plain", "m2"
PATHS = (SHORT, PLAIN, M2)


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
def update(mean, var, count, row):
    """update_mean_var_count_from_moments(mean, var, count, batch_mean=row, batch_var=float32 0, batch_count=1), normalize.py:36-46."""
    batch_mean, batch_var, batch_count = row, np.float32(0.0), 1
    with np.errstate(all="ignore"):
        delta = batch_mean - mean
        tot_count = count + batch_count
        new_mean = mean + delta * batch_count / tot_count
        m_a = var * count
        m_b = batch_var * batch_count
        M2_ = m_a + m_b + np.square(delta) * count * batch_count / tot_count
        new_var = M2_ / tot_count
    return new_mean, new_var, tot_count


def normalise(row, mean, var, epsilon):
    with np.errstate(all="ignore"):
        return (row - mean) / np.sqrt(var + epsilon)


# ---- the guards ---------------------------------------------------------------------------------------------------------------------
def _frexp_exp(x):
    """v_frexp_exp_i32_f64: C frexp's exponent (the true one for subnormals), 0 for zero, Inf and NaN."""
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)
    return np.where(np.isfinite(x) & (x != 0), e, 0).astype(np.int64)


def _in_window(v, lo, width):
    return ((v + lo) & 0xFFFFFFFF) < width          # (uint32_t)(v + lo) < width


def plain_operand(x):
    return _in_window(_frexp_exp(x), 722, 1401)


def plain_delta(x):
    return _in_window(_frexp_exp(x), 299, 601)


def plain_divisor(d):
    e = (np.asarray(d, np.float64).view(np.uint64) >> np.uint64(52)).astype(np.int64) & 0x7FF
    return _in_window(e, -959, 129)


def short_count(c):
    """The count the short path takes: all-zero bits, or positive with plain_divisor's exponent window (a set sign bit fails)."""
    b = np.asarray(c, np.float64).view(np.uint64)
    return _in_window((b >> np.uint64(52)).astype(np.int64), -959, 129) | (b == 0)


# ---- div_shared on the host ---------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))      # exact, rounded once (subnormal results included)


def div_shared_host(x, d):
    """div_shared(x, d, refined_rcp(d)) for finite non-zero operands (v_div_fixup is the identity there); v_rcp_f64's estimate is taken
    to be 1 / d rounded, which the two Newton steps leave as it is."""
    r = 1.0 / d
    for _ in range(2):
        r = _fma(r, _fma(-d, r, 1.0), r)
    q0 = x * r
    return _fma(_fma(-d, q0, x), r, q0)


def differing_dividends(rng, d, how_many, times=1.0, exponent=-1035):
    """Subnormal v such that div_shared(v * times, d) and (v * times) / d differ (the remainder fma(-d, q0, x) rounds)."""
    out = []
    while len(out) < how_many:
        v = float(np.ldexp(rng.uniform(1.0, 2.0), exponent))
        if div_shared_host(v * times, d) != (v * times) / d:
            out.append(v)
    return np.array(out)


# ---- the walks ----------------------------------------------------------------------------------------------------------------------
def _wave_report(report, it, at_work, p1, p2, bad_idle, failed_before):
    n = at_work.size
    for w in range((n + WAVE - 1) // WAVE):
        s = slice(w * WAVE, min(n, (w + 1) * WAVE))
        a = at_work[s]
        if not a.any():
            continue
        if not p1[s][a].all():
            report.append((w, it, PLAIN, bool(p1[s][a].any())))
            failed_before[w] = True
        elif not p2[s][a].all():
            report.append((w, it, M2, bool(p2[s][a].any())))
            failed_before[w] = True
        else:
            report.append((w, it, SHORT, bool(failed_before[w] or bad_idle[s][~a].any())))


def _votes(mean, var, count, row):
    """Per lane: would it pass the first vote, and the second (on the M2 the kernel forms)."""
    c = count[:, None]
    with np.errstate(all="ignore"):
        tot = c + 1.0
        delta = row - mean
        m2 = var * c + np.square(delta) * c / tot
    p1 = plain_divisor(tot[:, 0]) & short_count(count) & plain_delta(delta).all(axis=1)
    return p1, plain_operand(m2).all(axis=1)


def obs_walk(mean, var, count, x, fin, te, tr, epsilon):
    """subnorm_obs_kernel on [K][n][D] float32 rows.  Returns y, final_y (float64; rows of events that did not happen stay 0), the mask of
    final_y rows written, (mean, var, count) and the report."""
    x = np.asarray(x, np.float32)
    K, n, D = x.shape
    mean, var, count = np.array(mean, np.float64).reshape(n, D), np.array(var, np.float64).reshape(n, D), np.array(count, np.float64).reshape(n)
    has_fin = te is not None and fin is not None
    done = ((np.asarray(te) | np.asarray(tr)) != 0).reshape(K, n) if has_fin else np.zeros((K, n), bool)
    y, yfin, wrote = np.zeros((K, n, D)), np.zeros((K, n, D)), np.zeros((K, n), bool)
    kl, fin_done, lanes = np.zeros(n, np.int64), np.zeros(n, bool), np.arange(n)
    report, failed_before, it = [], {w: False for w in range((n + WAVE - 1) // WAVE)}, 0
    while (kl < K).any():
        at_work = kl < K
        k = np.minimum(kl, K - 1)
        use_fin = at_work & ~fin_done & done[k, lanes]
        row = np.where(use_fin[:, None], np.asarray(fin, np.float32)[k, lanes] if has_fin else 0, x[k, lanes]).astype(np.float64)
        p1, p2 = _votes(mean, var, count, row)
        with np.errstate(all="ignore"):
            bad_idle = ~(plain_divisor(count + 1.0) & short_count(count))
        _wave_report(report, it, at_work, p1, p2, bad_idle, failed_before)
        nm, nv, nc = update(mean, var, count[:, None], row)
        mean[at_work], var[at_work], count[at_work] = nm[at_work], nv[at_work], nc[at_work, 0]
        out = normalise(row, mean, var, epsilon)
        f, b = use_fin, at_work & ~use_fin
        yfin[k[f], lanes[f]], wrote[k[f], lanes[f]] = out[f], True
        y[k[b], lanes[b]] = out[b]
        fin_done = f
        kl = kl + b
        it += 1
    return y, yfin, wrote, (mean, var, count), report


def rew_walk(mean, var, count, returns, rew, te, tr, gamma, epsilon):
    """subnorm_rew_kernel on [K][n] rewards (float32 or float64).  Returns out (float64, before the cast to the reward dtype),
    (mean, var, count, returns) and the report."""
    rew = np.asarray(rew)
    K, n = rew.shape
    mean, var, count, ret = (np.array(a, np.float64).reshape(n) for a in (mean, var, count, returns))
    done = ((np.asarray(te) | np.asarray(tr)) != 0).reshape(K, n)
    out, report, failed_before = np.zeros((K, n)), [], {w: False for w in range((n + WAVE - 1) // WAVE)}
    everyone, nobody = np.ones(n, bool), np.zeros(n, bool)
    for k in range(K):
        rw = rew[k].astype(np.float64)
        with np.errstate(all="ignore"):
            ret = ret * gamma + rw
        p1, p2 = _votes(mean[:, None], var[:, None], count, ret[:, None])
        _wave_report(report, k, everyone, p1, p2, nobody, failed_before)
        mean, var, count = update(mean, var, count, ret)
        with np.errstate(all="ignore"):
            out[k] = rw / np.sqrt(var + epsilon)
        ret = np.where(done[k], 0.0, ret)
    return out, (mean, var, count, ret), report


def paths_taken(report):
    """{(path, mixed)} over a report."""
    return {(p, m) for _, _, p, m in report}


EVERY_PATH_BOTH_WAYS = {(p, m) for p in PATHS for m in (False, True)}


# ---- comparison ---------------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, ref):
    """Equal bit patterns (-0.0 is not +0.0), any NaN matching any NaN (x86 and gfx950 sign their default NaN differently)."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return False
    gn, rn = np.isnan(got), np.isnan(ref)
    return bool(np.array_equal(gn, rn) and np.array_equal(bits(got)[~gn], bits(ref)[~rn]))


def nan_envs(*arrays_env_axis):
    """The envs at which any of the (array, env axis) pairs holds a NaN."""
    out = set()
    for a, axis in arrays_env_axis:
        a = np.moveaxis(np.asarray(a), axis, 0)
        out |= set(np.flatnonzero(np.isnan(a.reshape(a.shape[0], -1)).any(axis=1)).tolist())
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 255, 256, 257, 4099)
DIMS = (1, 2, 3, 4, 6)
STEPS = (1, 2, 7, 33)
FLAG_PATTERNS = ("none", "all", "step0", "last", "terminated", "truncated", "both", "byte2", "byte0x80", "byte0xff", "drift", "alternating")
DRIFT_LANE = 5   # the one env of every wave that ends at every step under "drift"


def flags(pattern, K, n, rng):
    """(terminated, truncated) uint8 [K][n]."""
    te, tr = np.zeros((K, n), np.uint8), np.zeros((K, n), np.uint8)
    hit = rng.random((K, n)) < 0.3 if rng is not None else None     # (the fixed patterns need no generator)
    if pattern == "all":
        te[:, 0::2], tr[:, 1::2] = 1, 1
    elif pattern == "step0":
        te[0] = 1
    elif pattern == "last":
        tr[K - 1] = 1
    elif pattern == "terminated":
        te[hit] = 1
    elif pattern == "truncated":
        tr[hit] = 1
    elif pattern == "both":
        te[hit], tr[hit] = 1, 1
    elif pattern.startswith("byte"):
        b = int(pattern[4:], 0)
        te[hit & (np.arange(n) % 2 == 0)], tr[hit & (np.arange(n) % 2 == 1)] = b, b
    elif pattern == "drift":
        te[:, DRIFT_LANE % n::WAVE] = 1
    elif pattern == "alternating":
        te[1::2, 1::2] = 1
    else:
        assert pattern == "none", pattern
    return te, tr


_ROWS = {}


def rows(D, K, n):
    """Ordinary float32 rows and terminal rows [K][n][D], slices of one array per D (per-component scales from 0.01 to 6)."""
    if D not in _ROWS:
        rng = np.random.default_rng(1000 + D)
        scale = rng.uniform(0.01, 6.0, (1, 1, D))
        _ROWS[D] = ((rng.standard_normal((max(STEPS), max(SIZES), D)) * scale).astype(np.float32),
                    (rng.standard_normal((max(STEPS), max(SIZES), D)) * 3).astype(np.float32))
    x, fin = _ROWS[D]
    return np.ascontiguousarray(x[:K, :n]), np.ascontiguousarray(fin[:K, :n])


def ordinary_state(rng, n, D):
    return rng.standard_normal((n, D)), rng.random((n, D)) + 0.05, np.floor(rng.random(n) * 100) + 2.0


GUARD_N, GUARD_WAVES = 7 * WAVE, 7
# wave 0 ordinary | 1 extremes among ordinary lanes | 2 one lane whose M2 alone fails the second vote | 3 every count 1e300 |
# 4 ordinary | 5 lanes whose delta alone fails the first vote | 6 every lane's M2 fails the second vote
OK2_LANE = 2 * WAVE + 7
DELTA_LANES = (5 * WAVE + 3, 5 * WAVE + 40)
EXTREME = {"count_tiny": WAVE + 3, "count_huge": WAVE + 9, "count_minus_one": WAVE + 17, "mean_huge": WAVE + 21, "mean_nan": WAVE + 33,
           "count_minus_zero": WAVE + 40, "count_minus_half": WAVE + 45, "var_inf": WAVE + 50, "var_subnormal": WAVE + 52}
GUARD_NAN_ENVS = {EXTREME["mean_nan"], EXTREME["count_minus_one"]}


def _guard_state(rng, D, first_row):
    """Statistics that walk every path (see the wave list above), given the first row every env meets ([n][D], float32-representable).
    The short form and `/` differ on the dividends of the lanes that fail a vote alone (tot = 6, subnormal dividends), so a guard that
    lets them through changes the stored bits."""
    n = GUARD_N
    mean, var, count = ordinary_state(rng, n, D)
    w1 = slice(WAVE, 2 * WAVE)
    e = EXTREME
    count[e["count_tiny"]], count[e["count_huge"]], count[e["count_minus_one"]] = 1e-300, 1e300, -1.0
    mean[e["mean_huge"]], mean[e["mean_nan"], 0] = 1e300, np.nan
    count[e["count_minus_zero"]] = -0.0
    count[e["count_minus_half"]], var[e["count_minus_half"]], mean[e["count_minus_half"]] = -0.5, 0.0, first_row[e["count_minus_half"]]
    var[e["var_inf"], D - 1], var[e["var_subnormal"]] = np.inf, 1e-310
    assert w1.start <= min(e.values()) and max(e.values()) < w1.stop
    # the second vote alone: delta = 0 (the mean is the row), count = 5, var * 5 a subnormal on which the two division forms differ
    for lane, dims in [(OK2_LANE, [min(1, D - 1)])] + [(l, list(range(D))) for l in range(6 * WAVE, 7 * WAVE)]:
        mean[lane], count[lane] = first_row[lane], 5.0
        var[lane, dims] = differing_dividends(rng, 6.0, len(dims), times=5.0)
    count[3 * WAVE:4 * WAVE] = 1e300
    # the delta test alone: the row is 0 and the mean a subnormal on which delta / 6 differs between the two forms
    for lane in DELTA_LANES:
        mean[lane], count[lane] = 0.0, 5.0
        mean[lane, D - 1] = -differing_dividends(rng, 6.0, 1)[0]
    return mean, var, count


def obs_guard_case(D, K, seed=7):
    """(mean, var, count), x, fin, te, tr for the guard-path runs: GUARD_N envs; lane 0 of every wave ends at step 0 (its terminal row is
    its batch row, so every env's first row is x[0]); from step 1 on episodes end at random."""
    rng = np.random.default_rng(seed + 10 * D)
    x, fin = rows(D, K, GUARD_N)
    x, fin = x.copy(), fin.copy()
    x[0, list(DELTA_LANES)] = 0.0
    fin[0] = x[0]
    te, tr = np.zeros((K, GUARD_N), np.uint8), np.zeros((K, GUARD_N), np.uint8)
    te[1:], tr[1:] = rng.random((K - 1, GUARD_N)) < 0.08, rng.random((K - 1, GUARD_N)) < 0.04
    te[0, 0::WAVE] = 1
    return _guard_state(rng, D, x[0].astype(np.float64)), x, fin, te, tr


def rew_guard_case(K, f32, seed=11):
    """(mean, var, count, returns), rewards, te, tr, gamma for the reward kernel's guard-path runs: returns start at 0, so the first
    return of every env is its first reward; one lane of wave 1 meets a reward of 1e200 (float64) / 3e38 (float32)."""
    rng = np.random.default_rng(seed)
    rew = rng.standard_normal((K, GUARD_N)) * 3
    rew[0, list(DELTA_LANES)] = 0.0
    rew[0, WAVE + 60] = 3e38 if f32 else 1e200
    rew = rew.astype(np.float32 if f32 else np.float64)
    te, tr = (rng.random((K, GUARD_N)) < 0.1).astype(np.uint8), (rng.random((K, GUARD_N)) < 0.05).astype(np.uint8)
    mean, var, count = _guard_state(rng, 1, rew[0].astype(np.float64)[:, None])
    return (mean[:, 0], var[:, 0], count, np.zeros(GUARD_N)), rew, te, tr, 0.97


EDGE_N, EDGE_LANES, EDGE_K = 130, (0, 63, 64), 2


def obs_edge_cases(D):
    """name -> ((mean, var, count), x, epsilon, NaN envs): an edge row (and, where it takes them, edge statistics) at lanes 0, 63 and 64 of a
    130-env batch of ordinary envs, K = 2 steps (the second step runs on the statistics the first one left)."""
    out = {}
    L = list(EDGE_LANES)

    def case(name, epsilon=1e-8, nan=False, fresh=False, **put):
        rng = np.random.default_rng(len(out) + 100 * D)
        x, _ = rows(D, EDGE_K, EDGE_N)
        x = x.copy()
        mean, var, count = (np.zeros((EDGE_N, D)), np.ones((EDGE_N, D)), np.full(EDGE_N, 1e-4)) if fresh else ordinary_state(rng, EDGE_N, D)
        if "row" in put:
            x[0, L] = put["row"]
        if "component" in put:
            x[0, L, D - 1] = put["component"]
        if put.get("mean_is_row"):
            mean[L] = x[0, L]
        for key, arr in (("var", var), ("count", count)):
            if key in put:
                arr[L] = put[key]
        out[name] = ((mean, var, count), x, epsilon, set(L) if nan else set())

    case("plus_inf", nan=True, component=np.inf)
    case("minus_inf", nan=True, component=-np.inf)
    case("nan", nan=True, component=np.nan)
    case("minus_zero_on_fresh_statistics", fresh=True, row=-0.0)
    case("row_equals_mean", mean_is_row=True)
    case("float32_subnormal_result", var=1e80, count=1e200)          # |delta| / 1e40 < 2^-126: rounded once into float32's subnormals
    case("float32_overflow_result", epsilon=0.0, var=1e-90, count=1e200)   # |delta| * 1e45 > float32's maximum: Inf
    case("epsilon_0_var_0", epsilon=0.0, nan=True, mean_is_row=True, var=0.0, count=10.0)      # 0 / sqrt(0)
    case("epsilon_0_var_negative", epsilon=0.0, nan=True, var=-1e6, count=10.0)                # sqrt of a negative variance
    case("count_minus_zero", fresh=True, count=-0.0)                                           # m_b: M2 = -0.0 + 0.0 + -0.0
    case("count_minus_half_var_0", mean_is_row=True, var=0.0, count=-0.5)                      # m_b again, a divisor of 0.5
    return out


REWARD_GAMMAS = (0.0, 0.97, 1.0, -0.5)


def rew_edge_cases(f32):
    """name -> (rewards [9][130], gamma, starting returns [130], NaN envs); edge rewards at lanes 0, 63 and 64 among ordinary envs on
    fresh statistics."""
    K, L = 9, list(EDGE_LANES)
    rng = np.random.default_rng(77)
    base = (rng.standard_normal((K, EDGE_N)) * 3).astype(np.float32 if f32 else np.float64)
    zero = np.zeros(EDGE_N)
    out = {f"gamma_{g}": (base.copy(), g, zero, set()) for g in REWARD_GAMMAS}
    big, start = base.copy(), zero.copy()
    big[:, L], start[L] = 3e38, 1e306        # gamma = 2: the returns pass float64's maximum at the second step and are Inf, then NaN
    out["gamma_2_overflow"] = (big, 2.0, start, set(L))
    z = base.copy()
    z[:, L] = -0.0
    out["minus_zero_rewards"] = (z, 0.97, zero, set())
    nn = base.copy()
    nn[3, L[1]] = np.nan
    out["nan_reward"] = (nn, 0.97, zero, {L[1]})
    return out


def obs_grid(n, D):
    """The (flag pattern, K, float32 output) runs of one size and dim: every flag pattern once, the eight (K, dtype) pairs dealt round
    so that over all sizes and dims every pattern meets every pair."""
    pairs = [(K, f32) for K in STEPS for f32 in (True, False)]
    off = SIZES.index(n) * len(DIMS) + DIMS.index(D)
    return [(p, *pairs[(i + off) % len(pairs)]) for i, p in enumerate(FLAG_PATTERNS)]


def rew_grid(n):
    """(flag pattern, K, float32 rewards, in place, gamma) runs of one size."""
    combos = [(K, f32, inplace) for K in (1, 9) for f32 in (True, False) for inplace in (True, False)]
    off = SIZES.index(n)
    return [(p, *combos[(i + off) % len(combos)], REWARD_GAMMAS[(i + off) % len(REWARD_GAMMAS)]) for i, p in enumerate(FLAG_PATTERNS)]


def rewards_for(K, n, f32):
    rng = np.random.default_rng(5000 + n)
    return (rng.standard_normal((K, n)) * 3).astype(np.float32 if f32 else np.float64)


# ---- the oracle, called the way the device is ---------------------------------------------------------------------------------------
def oracle_obs(state, x, fin, te, tr, epsilon, f32, final_y=True):
    """oracle.SubEnvNorm on one call: y (float32 / float64), final_y (float64, 0 where no episode ended) or None, (mean, var, count)."""
    from oracle.oracle import SubEnvNorm

    K, n, D = x.shape
    o = SubEnvNorm(D, n)
    if state is not None:
        o.set_state(*state)
    y = np.zeros((K, n, D), np.float32 if f32 else np.float64)
    yf = np.zeros((K, n, D)) if final_y and fin is not None else None
    with np.errstate(all="ignore"):
        o.observations(K, x, fin, te, tr, y, f32, yf, epsilon)
    return y, yf, o.get_state()[:3]


def oracle_rew(state, rew, te, tr, gamma, epsilon):
    from oracle.oracle import SubEnvNorm

    K, n = rew.shape
    o = SubEnvNorm(1, n)
    if state is not None:
        o.set_state(state[0][:, None], state[1][:, None], state[2], state[3])
    out = np.zeros((K, n), rew.dtype)
    with np.errstate(all="ignore"):
        o.rewards(K, rew, rew.dtype == np.float32, te, tr, out, gamma, epsilon)
    m, v, c, r = o.get_state()
    return out, (m[:, 0], v[:, 0], c, r)
