"""The device math helpers of gym_amd/csrc/mxv_device.hpp and mxv_divide.hpp, as shipped, against exact or high-precision references.

tests/device_math/primitives.hip wraps each helper (and each template instantiation the engine uses) in one element-wise kernel; it is built
here with the library's flags and called through ctypes.  "Bit-equal" means equal as uint64 / uint32 patterns: the sign of zero counts.
  division    numpy `/` (correctly rounded)
  sin / cos   np.longdouble sin / cos (x87 80-bit, glibc's sinl / cosl with a full argument reduction), cross-checked by mpmath at 128 bits
  remainders  np.fmod and numpy `%` (exact by definition)
  clamps      np.clip and the reference's `if x > hi` / `if x < lo` chain
  powf        tools/powf_variants.py's NumPy twin of glibc's powf(u, 2.0f), which tests/test_exact_trig.py pins to libm
The measured sin / cos maxima are printed (pytest -s shows them)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from helpers import build_device_math

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RNG_SEED = 20261016
PI = np.pi
TWO_PI = 2 * np.pi
F3 = {"cartpole": 0, "mcc": 1, "acrobot": 2, "pendulum": 3}   # fma3_for<ENV>() of primitives.hip's instantiations


@pytest.fixture(scope="module")
def dm(tmp_path_factory):
    lib = ctypes.CDLL(build_device_math(tmp_path_factory.mktemp("device_math")))

    def call(name, a, b=None, c=None, dtype=np.float64):
        f = getattr(lib, name)
        ct = ctypes.POINTER(ctypes.c_double if dtype == np.float64 else ctypes.c_float)
        f.restype = ctypes.c_int
        f.argtypes = [ct, ct, ct, ct, ct, ctypes.c_int64]
        a = np.ascontiguousarray(a, dtype=dtype)
        ins = [a] + [None if x is None else np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=dtype), a.shape)) for x in (b, c)]
        o, p = np.empty_like(a), np.empty_like(a)
        ptr = lambda x: None if x is None else x.ctypes.data_as(ct)  # noqa: E731
        err = f(*(ptr(x) for x in ins), ptr(o), ptr(p), a.size)
        assert err == 0, f"{name}: hipError {err}"
        return o, p

    return call


def bits(x):
    x = np.asarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def assert_bit_equal(got, ref, what, nan_payload=False):
    """Bit-equal, signed zeros included; NaN positions must agree, NaN payloads only when asked."""
    got, ref = np.asarray(got), np.asarray(ref)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: NaN at {np.flatnonzero(gn != rn)[:5]}"
    sel = np.ones(got.shape, bool) if nan_payload else ~rn
    bad = np.flatnonzero(bits(got)[sel] != bits(ref)[sel])
    assert bad.size == 0, f"{what}: {bad.size} of {int(sel.sum())} differ, e.g. got={got[sel][bad[:4]].tolist()} ref={ref[sel][bad[:4]].tolist()}"


def neighbours(x, k):
    """x and its k nearest doubles on each side."""
    x = np.asarray(x, np.float64)
    out = [x]
    up, dn = x.copy(), x.copy()
    for _ in range(k):
        up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
        out += [up, dn]
    return np.concatenate(out)


def log_uniform(rng, n, e_lo, e_hi, signed=True):
    x = np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(e_lo, e_hi + 1, n))
    return x * rng.choice([-1.0, 1.0], n) if signed else x


# ============================================ division ===============================================================================
def midpoint_dividends(rng, d, n, e_lo, e_hi):
    """x = RN(d * m) for quotient midpoints m = q + ulp(q) / 2, and the doubles next to each x: quotients within a fraction of an ulp of a
    rounding boundary, where a short-cut division that is off by a little shows."""
    q = log_uniform(rng, n, e_lo, e_hi)
    m = q.astype(np.longdouble) + np.spacing(np.abs(q)).astype(np.longdouble) / 2 * np.sign(q)
    x = (np.asarray(d, np.longdouble) * m).astype(np.float64)
    return neighbours(x, 1)


def near_midpoint_count(x, d):
    """How many quotients x / d lie within 2^-60 (relative) of a rounding midpoint, measured in 80-bit."""
    qd = x.astype(np.longdouble) / np.asarray(d, np.longdouble)
    q = (x / d)
    half = np.spacing(np.abs(q)).astype(np.longdouble) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.abs(np.abs(qd - q.astype(np.longdouble)) - half) / np.abs(qd)
    return int((frac < 2.0 ** -60).sum())


def test_div_par_finite_is_ieee_division_on_its_domain(dm):
    """div_par<PM_DEFAULT, true> (the fused rollout's x / total_mass, Markstein's sequence): bit-equal to `/` for finite x with
    |x / c| > 2^-969; its documented deviations, x = -0 (gives +0) and x = +-Inf (gives NaN), pinned as they are."""
    rng = np.random.default_rng(RNG_SEED)
    c = 0.1 + 1.0
    x = np.concatenate([log_uniform(rng, 10_000_000, -968, 1023), rng.uniform(-50, 50, 1_000_000),
                        midpoint_dividends(rng, c, 1_000_000, -968, 1022), [np.finfo(np.float64).max, -np.finfo(np.float64).max, 1.0, 0.0]])
    x = x[np.isfinite(x) & ((x == 0) | (np.abs(x / c) > 2.0 ** -969))]
    assert near_midpoint_count(x, c) > 1000
    got, _ = dm("div_par_finite", x)
    assert_bit_equal(got, x / c, "div_par<PM_DEFAULT, true>")
    got, _ = dm("div_par_finite", np.array([-0.0, np.inf, -np.inf]))
    assert bits(got[0]) == bits(np.float64(0.0)), "documented: -0 / c gives +0 on the finite-dividend form"
    assert np.isnan(got[1:]).all(), "documented: Inf * rc - c * Inf is a NaN on the finite-dividend form"


def test_div_par_with_fixup_is_ieee_division_everywhere(dm):
    """div_par<PM_DEFAULT, false> (step(actions) and injected states: Markstein + v_div_fixup): bit-equal to `/` on every double —
    +-0, +-Inf, NaN, subnormal dividends, quotients that overflow — except quotients below 2^-969, held to one ulp (the header says so)."""
    rng = np.random.default_rng(RNG_SEED + 1)
    c = 0.1 + 1.0
    tiny = np.finfo(np.float64).smallest_subnormal
    x = np.concatenate([rng.integers(0, 2 ** 64, 4_000_000, dtype=np.uint64).view(np.float64), log_uniform(rng, 4_000_000, -1074, 1023),
                        midpoint_dividends(rng, c, 500_000, -1070, 1022), neighbours([tiny, 2.0 ** -1022, 2.0 ** -969, np.finfo(np.float64).max], 20),
                        [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan]])
    x = np.concatenate([x, -x])
    with np.errstate(all="ignore"):
        ref = x / c
    got, _ = dm("div_par_fixup", x)
    small = np.isfinite(ref) & (np.abs(ref) <= 2.0 ** -969) & (ref != 0)
    assert_bit_equal(got[~small], ref[~small], "div_par<PM_DEFAULT, false>")
    # documented: a quotient below 2^-969 (the Markstein steps meet subnormals) may be one ulp off `/`, never more
    off = np.abs(got[small].view(np.int64) - ref[small].view(np.int64))
    print(f"div_par<PM_DEFAULT, false>: {int((off > 0).sum())} of {int(small.sum())} quotients below 2^-969 one ulp off")
    assert off.max() <= 1 and np.array_equal(np.signbit(got[small]), np.signbit(ref[small]))


@pytest.mark.parametrize("lo,hi,who", [(0.62, 0.67, "CartPole ta_den"), (2.5, 4.5, "Acrobot d1"), (0.57, 1.25, "Acrobot den2")])
def test_shared_reciprocal_division_is_ieee_division(dm, lo, hi, who):
    """div_with_rcp(x, d, refined_rcp(d)) over the divisor range the kernel feeds it, dividends over the whole exponent range on which the
    sequence needs no scaling (2^-968 <= |x| < 2^1022: no intermediate leaves the normal range): bit-equal to `/`.  x = -0 and +-Inf are
    the documented deviations (+0, NaN), pinned."""
    rng = np.random.default_rng(RNG_SEED + int(lo * 100))
    n = 3_000_000
    d = np.concatenate([rng.uniform(lo, hi, n), rng.uniform(lo, hi, n // 3)])
    x = np.concatenate([log_uniform(rng, n, -968, 1021), rng.uniform(-20, 20, n // 3)])
    dm_ = rng.uniform(lo, hi, 600_000)
    xm = midpoint_dividends(rng, dm_, 600_000, -960, 1020)
    x, d = np.concatenate([x, xm]), np.concatenate([d, np.tile(dm_, 3)])
    assert near_midpoint_count(xm, np.tile(dm_, 3)) > 500
    got, _ = dm("div_with_rcp_op", x, d)
    assert_bit_equal(got, x / d, who)
    got, _ = dm("div_with_rcp_op", np.array([-0.0, np.inf, -np.inf]), np.full(3, (lo + hi) / 2))
    assert bits(got[0]) == bits(np.float64(0.0)) and np.isnan(got[1:]).all()


# ============================================ the per-sub-env normaliser's guards ====================================================
def _edge_samples(rng, edges, k=8):
    """Doubles on both sides of 2^e for every e in edges: the k neighbours of the power itself and random mantissas in the two binades
    around it, both signs."""
    pw = np.ldexp(1.0, np.asarray(edges))
    x = np.concatenate([neighbours(pw, k), np.ldexp(rng.uniform(1, 2, 40 * len(edges)), np.repeat(np.asarray(edges), 40)),
                        np.ldexp(rng.uniform(1, 2, 40 * len(edges)), np.repeat(np.asarray(edges) - 1, 40))])
    return np.concatenate([x, -x])


def _guard_truth(x, lo_e, hi_e):
    """plain_* contract: True for 0, +-Inf, NaN, and for 2^lo_e <= |x| < 2^hi_e."""
    ax = np.abs(x)
    return (x == 0) | ~np.isfinite(x) | ((ax >= 2.0 ** lo_e) & (ax < 2.0 ** hi_e))


def test_subnorm_guards_sit_at_their_documented_edges(dm):
    """plain_operand: 2^-723 <= |x| < 2^678; plain_delta: 2^-300 <= |x| < 2^301; plain_divisor: 2^-64 <= |d| < 2^65 (no zero / Inf / NaN
    pass-through).  Off by one in 1401u, 601u or 129u moves an edge by a binade and fails here."""
    rng = np.random.default_rng(RNG_SEED + 7)
    tiny = np.finfo(np.float64).smallest_subnormal
    x = np.concatenate([_edge_samples(rng, [-723, 678, -300, 301, -64, 65, -1022]), log_uniform(rng, 200_000, -1074, 1023),
                        neighbours([tiny, 2.0 ** -1030], 3), [0.0, -0.0, np.inf, -np.inf, np.nan]])
    _, g = dm("plain_guards", x)
    g = g.astype(np.int64)
    assert np.array_equal((g & 1) != 0, _guard_truth(x, -723, 678)), "plain_operand"
    assert np.array_equal((g & 4) != 0, _guard_truth(x, -300, 301)), "plain_delta"
    ax = np.abs(x)
    assert np.array_equal((g & 2) != 0, np.isfinite(x) & (ax >= 2.0 ** -64) & (ax < 2.0 ** 65)), "plain_divisor"


def test_div_shared_is_ieee_division_wherever_the_guards_pass(dm):
    """mxv_subnorm.hip's claim: whenever plain_operand(x) && plain_divisor(d), div_shared(x, d, refined_rcp(d)) == x / d bit for bit —
    on both sides of every guard edge, with subnormals, +-0, +-Inf and NaN among the dividends."""
    rng = np.random.default_rng(RNG_SEED + 8)
    tiny = np.finfo(np.float64).smallest_subnormal
    xs = np.concatenate([_edge_samples(rng, [-723, 678, -300, 301], 6), log_uniform(rng, 3000, -1074, 1023), log_uniform(rng, 1000, -5, 60),
                         neighbours([tiny, 2.0 ** -1022], 2), [0.0, -0.0, np.inf, -np.inf, np.nan]])
    ds = np.concatenate([_edge_samples(rng, [-64, 65], 6), log_uniform(rng, 300, -64, 64), rng.uniform(1.0, 3.0, 200), 1.0 + np.arange(1, 100),
                         [2.0 ** 53, 0.0, np.inf, np.nan, tiny]])
    x, d = np.repeat(xs, ds.size), np.tile(ds, xs.size)
    _, gx = dm("plain_guards", x)
    _, gd = dm("plain_guards", d)
    ok = ((gx.astype(np.int64) & 1) != 0) & ((gd.astype(np.int64) & 2) != 0)
    assert ok.sum() > 1_000_000 and (~ok).sum() > 100_000
    got, _ = dm("div_shared_op", x[ok], d[ok])
    with np.errstate(all="ignore"):
        assert_bit_equal(got, x[ok] / d[ok], "div_shared where plain_operand && plain_divisor")


# ============================================ sin / cos ==============================================================================
def ulp_error(got, ref):
    """|got - ref| in units of the double ulp at ref (ref in 80-bit)."""
    _, e = np.frexp(ref)
    return (np.abs(got.astype(np.longdouble) - ref) / np.ldexp(np.longdouble(1), e - 53)).astype(np.float64)


HALF_PI_80 = np.longdouble("1.57079632679489661923132169163975144")


def near_half_pi_multiples(k_max, k_min=0, width=1):
    """For every k_min <= k < k_max: the double nearest k pi / 2 (80-bit product, rounded) and its `width` neighbours, both signs."""
    k = np.arange(max(k_min, 1), k_max).astype(np.longdouble)
    x = neighbours((k * HALF_PI_80).astype(np.float64), width)
    return np.concatenate([x, -x])


def reference(x):
    xl = x.astype(np.longdouble)
    return np.sin(xl), np.cos(xl)


def max_errors(dm, op, x):
    s, c = dm(op, x)
    rs, rc = reference(x)
    return float(ulp_error(s, rs).max()), float(ulp_error(c, rc).max())


@pytest.fixture(scope="module")
def sc_inputs():
    rng = np.random.default_rng(RNG_SEED + 11)
    n = 10_000_000
    return {
        "quarter": np.concatenate([rng.uniform(-PI / 4, PI / 4, n), log_uniform(rng, 100_000, -60, -2)]),
        "128": np.concatenate([rng.uniform(-128, 128, n), near_half_pi_multiples(82, width=64)]),
        "256": np.concatenate([rng.uniform(-256, 256, n), near_half_pi_multiples(164, width=32)]),
        "4096": np.concatenate([rng.uniform(-4096, 4096, n), near_half_pi_multiples(2608, width=4)]),
        "2^19": np.concatenate([rng.uniform(4096, 2.0 ** 19, n // 2) * rng.choice([-1, 1], n // 2), near_half_pi_multiples(333_800, 2600)]),
        "2^20k": near_half_pi_multiples(2 ** 20, 333_700),
        "huge": np.concatenate([log_uniform(rng, 2_000_000, 19, 1000), log_uniform(rng, 1_000_000, 12, 19)]),
    }


def test_longdouble_sin_cos_is_a_sound_reference_near_multiples_of_half_pi():
    """The 80-bit reference where cancellation is worst (x next to k pi / 2 for large k): within 0.01 double ulp of mpmath at 128 bits."""
    import mpmath

    rng = np.random.default_rng(RNG_SEED + 12)
    x = near_half_pi_multiples(2 ** 20, 1)
    x = np.concatenate([x[rng.integers(0, x.size, 3000)], log_uniform(rng, 500, 0, 999)])
    rs, rc = reference(x)
    mpmath.mp.prec = 128
    exact_s = np.array([mpmath.sin(mpmath.mpf(float(v))) for v in x])
    exact_c = np.array([mpmath.cos(mpmath.mpf(float(v))) for v in x])
    for ref, exact in ((rs, exact_s), (rc, exact_c)):
        _, e = np.frexp(ref)
        err = [float(abs(mpmath.mpf(str(r)) - t) / mpmath.ldexp(1, int(k) - 53)) for r, t, k in zip(ref, exact, e)]
        assert max(err) < 0.01, max(err)


def test_sincos_kernel_polynomials_within_their_stated_bounds(dm, sc_inputs):
    """(a) sincos_kernel on |x| <= pi/4, both coefficient forms: sin < 1 ulp (fdlibm's bound), cos < 0.884 ulp (the header's figure for
    the plain Horner tail)."""
    x = sc_inputs["quarter"]
    for op in ("sincos_kernel_f0", "sincos_kernel_f1"):
        es, ec = max_errors(dm, op, x)
        print(f"{op} |x| <= pi/4: sin {es:.3f} ulp, cos {ec:.3f} ulp")
        assert es < 1.0 and ec < 0.884, (op, es, ec)


@pytest.mark.parametrize("guard", ["guarded", "fast"])
@pytest.mark.parametrize("env", list(F3))
def test_mx_sincos_within_the_headers_bound_where_the_dynamics_call_it(dm, sc_inputs, guard, env):
    """(b) every mx_sincos instantiation on |x| <= 128 — every unguarded caller's range (Pendulum |theta| < 90 under a TimeLimit, Acrobot's
    wrapped angles, MountainCar's 3 * position) — including x next to every multiple of pi / 2 there: <= 1.51 ulp (the header's figure;
    measured 1.490 sin / 1.507 cos)."""
    es, ec = max_errors(dm, f"mx_sincos_{guard}_{env}", sc_inputs["128"])
    print(f"mx_sincos<{guard == 'guarded'}, {F3[env]}> |x| <= 128: sin {es:.3f} ulp, cos {ec:.3f} ulp")
    assert es <= 1.51 and ec <= 1.51, (es, ec)


def test_guarded_sincos_within_ocml_bound_on_its_medium_path(dm, sc_inputs):
    """(c) mx_sincos<true> over its whole medium-path domain (|x| < 2^8), with every double next to k pi / 2 there: <= 2 ulp, the
    bound of the ocml routine it replaces.  The medium path's error up to 2^12 and 2^19 (where the guarded form calls ocml) is printed:
    the reason for the threshold."""
    es, ec = max_errors(dm, "mx_sincos_guarded_cartpole", sc_inputs["256"])
    print(f"mx_sincos<true> |x| < 2^8: sin {es:.3f} ulp, cos {ec:.3f} ulp")
    assert es <= 2.0 and ec <= 2.0, (es, ec)
    for key in ("4096", "2^19"):
        fs, fc = max_errors(dm, "mx_sincos_fast_cartpole", sc_inputs[key])
        print(f"sincos_medium, the {key} set (unguarded form only): sin {fs:.3f} ulp, cos {fc:.3f} ulp")


def test_guarded_sincos_beyond_the_medium_path(dm, sc_inputs):
    """(d) From 2^8 on the guarded form is ocml's sincos: <= 2 ulp up to 2^1000, including every double next to k pi / 2 for k < 2^20;
    +-Inf and NaN give NaN."""
    x = np.concatenate([sc_inputs["4096"], sc_inputs["2^19"], sc_inputs["2^20k"], sc_inputs["huge"]])
    x = x[np.abs(x) >= 256.0]
    es, ec = max_errors(dm, "mx_sincos_guarded_pendulum", x)
    print(f"mx_sincos<true> 2^8 <= |x| < 2^1000 (ocml): sin {es:.3f} ulp, cos {ec:.3f} ulp")
    assert es <= 2.0 and ec <= 2.0, (es, ec)
    for env in F3:
        s, c = dm(f"mx_sincos_guarded_{env}", np.array([np.inf, -np.inf, np.nan]))
        assert np.isnan(s).all() and np.isnan(c).all(), env
    s, c = dm("sincos_small_or_general_op", np.array([np.inf, -np.inf, np.nan]))
    assert np.isnan(s).all() and np.isnan(c).all()


def test_sin_of_signed_zero_keeps_its_sign(dm):
    """(e) sin(+-0) = +-0, cos(+-0) = 1 for every instantiation an injected state reaches: mx_sincos<true, *> and
    sincos_small_or_general (CartPole's SAFE step)."""
    z = np.array([0.0, -0.0])
    for op in [f"mx_sincos_guarded_{e}" for e in F3] + ["sincos_small_or_general_op"]:
        s, c = dm(op, z)
        assert_bit_equal(s, z, f"{op}: sin(+-0)")
        assert_bit_equal(c, np.ones(2), f"{op}: cos(+-0)")


def test_coefficient_forms_are_bit_identical(dm, sc_inputs):
    """(f) fma_coef<F3> and the xor_masked sign path are "same operation, same bits": every F3 variant of sincos_kernel, sincos_medium and
    mx_sincos gives identical bits, and the guarded form equals the unguarded one on its medium path (zeros aside)."""
    x = sc_inputs["quarter"]
    a, b = dm("sincos_kernel_f0", x), dm("sincos_kernel_f1", x)
    assert_bit_equal(a[0], b[0], "sincos_kernel sin")
    assert_bit_equal(a[1], b[1], "sincos_kernel cos")
    x = np.concatenate([sc_inputs["4096"], sc_inputs["2^19"]])
    base = dm("sincos_medium_f0", x)
    for f in (1, 2, 3):
        s, c = dm(f"sincos_medium_f{f}", x)
        assert_bit_equal(s, base[0], f"sincos_medium<{f}> sin")
        assert_bit_equal(c, base[1], f"sincos_medium<{f}> cos")
    for env in F3:
        s, c = dm(f"mx_sincos_fast_{env}", x)
        assert_bit_equal(s, base[0], f"mx_sincos<false, {env}> sin")
        assert_bit_equal(c, base[1], f"mx_sincos<false, {env}> cos")
    xm = sc_inputs["256"]
    xm = xm[(xm != 0) & (np.abs(xm) < 256.0)]
    ref = dm("sincos_medium_f0", xm)
    for env in F3:
        s, c = dm(f"mx_sincos_guarded_{env}", xm)
        assert_bit_equal(s, ref[0], f"mx_sincos<true, {env}> sin")
        assert_bit_equal(c, ref[1], f"mx_sincos<true, {env}> cos")


# ============================================ remainders =============================================================================
@pytest.fixture(scope="module")
def rem_inputs():
    rng = np.random.default_rng(RNG_SEED + 20)
    b = TWO_PI
    k = np.concatenate([np.arange(-2000, 2000), rng.integers(-2 ** 20, 2 ** 20, 100_000)]).astype(np.float64)
    bound = 2.0 ** 20 * b
    return np.concatenate([
        rng.uniform(-bound, bound, 4_000_000), rng.uniform(-100, 100, 2_000_000), log_uniform(rng, 2_000_000, -1074, 22),
        log_uniform(rng, 500_000, 22, 1023),                                         # beyond the fast path: ocml's fmod
        neighbours(k * b, 2), neighbours([bound, -bound], 4), neighbours([b, -b, PI, -PI], 4),
        -np.ldexp(1.0, np.arange(-1074, -40)), np.ldexp(1.0, np.arange(-1074, -40)), [-1e-300, -5e-324, -1e-17],
        [0.0, -0.0, np.inf, -np.inf, np.nan],
    ])


def test_fmod_const_is_c_fmod(dm, rem_inputs):
    """fmod_const(a, 2 pi): bit-equal to C fmod (np.fmod) everywhere, the ocml fallback beyond 2^20 periods included."""
    got, _ = dm("fmod_const_2pi", rem_inputs)
    with np.errstate(all="ignore"):
        assert_bit_equal(got, np.fmod(rem_inputs, TWO_PI), "fmod_const")


def test_np_remainder_is_numpy_mod(dm, rem_inputs):
    """np_remainder(a, 2 pi): bit-equal to numpy `%` (the reference's angle_normalize) everywhere; tiny negatives give 2 pi itself."""
    got, _ = dm("np_remainder_2pi", rem_inputs)
    with np.errstate(all="ignore"):
        ref = np.remainder(rem_inputs, TWO_PI)
    assert_bit_equal(got, ref, "np_remainder")
    assert got[rem_inputs == -1e-300][0] == TWO_PI


def test_np_remainder_bounded_equals_np_remainder_on_its_domain(dm, rem_inputs):
    """np_remainder_bounded (the fused rollout's form, no range guard): the bits of np_remainder for |a| < 2^20 * 2 pi."""
    a = rem_inputs[np.abs(rem_inputs) < 2.0 ** 20 * TWO_PI]
    got, _ = dm("np_remainder_bounded_2pi", a)
    ref, _ = dm("np_remainder_2pi", a)
    assert_bit_equal(got, ref, "np_remainder_bounded vs np_remainder")
    assert_bit_equal(got, np.remainder(a, TWO_PI), "np_remainder_bounded vs numpy")


# ============================================ clamps =================================================================================
BOUNDS = [(-8.0, 8.0), (-2.0, 2.0), (-1.2, 0.6), (-0.07, 0.07), (0.0, 1.0), (-1.0, -0.0), (1.0, -1.0), (0.5, 0.25), (-np.inf, 3.0),
          (5e-324, 1e-310)]


def _clamp_inputs(rng, lo, hi, dtype):
    sub = np.finfo(dtype).smallest_subnormal
    x = np.concatenate([rng.uniform(-10, 10, 20_000), log_uniform(rng, 5000, -1074 if dtype == np.float64 else -149, 100),
                        neighbours([lo, hi], 3) if np.isfinite(lo) else neighbours([hi], 3),
                        [0.0, -0.0, np.inf, -np.inf, sub, -sub, 1e-310, -1e-310]]).astype(dtype)
    return x[~np.isnan(x)]


def _zero_clash(x, lo, hi):
    """x a zero and a bound the zero of the other sign: the one non-NaN case where max / min and the compare forms may differ, which the
    header rules out (no caller has such bounds)."""
    return (x == 0) & (((lo == 0) & (np.signbit(lo) != np.signbit(x))) | ((hi == 0) & (np.signbit(hi) != np.signbit(x))))


def _chain_hi_first(x, lo, hi):
    y = np.where(x > hi, hi, x)
    return np.where(y < lo, lo, y)


QNAN_PAYLOADS = [0x7FF0000000000001, 0xFFF0000000000001, 0x7FF8000000000000, 0x7FF8000100000000, 0x7FF80000DEADBEEF, 0xFFFFFFFF00000000,
                 0x7FF4000000000000]


@pytest.mark.parametrize("lo,hi", BOUNDS)
def test_double_clamps_match_the_reference_forms(dm, lo, hi):
    """clamp_range == np.clip(x, lo, hi) (lower bound first: lo > hi gives hi) and clamp_range_hi_first == `if x > hi: x = hi; if x < lo:
    x = lo` (lo > hi gives lo), bit for bit, with +-0, +-Inf, subnormals and values at the bounds; a NaN comes out with its payload
    unchanged, whichever dword holds it (0x7FF00000_00000001: ADVICE r4)."""
    rng = np.random.default_rng(RNG_SEED + 30)
    x = _clamp_inputs(rng, lo, hi, np.float64)
    x = x[~_zero_clash(x, lo, hi)]
    got, _ = dm("clamp_range_f64", x, lo, hi)
    assert_bit_equal(got, np.clip(x, lo, hi), "clamp_range")
    got, _ = dm("clamp_range_hi_first_f64", x, lo, hi)
    assert_bit_equal(got, _chain_hi_first(x, lo, hi), "clamp_range_hi_first")
    nans = np.array(QNAN_PAYLOADS, np.uint64).view(np.float64)
    for op in ("clamp_range_f64", "clamp_range_hi_first_f64"):
        got, _ = dm(op, nans, lo, hi)
        assert np.array_equal(bits(got), bits(nans)), (op, [hex(v) for v in bits(got)])


def test_nan_through_passes_every_payload(dm):
    x = np.concatenate([np.array(QNAN_PAYLOADS, np.uint64).view(np.float64), [1.0, -0.0, np.inf]])
    r = np.full(x.size, 2.5)
    got, _ = dm("nan_through_op", x, r)
    assert np.array_equal(bits(got[:len(QNAN_PAYLOADS)]), bits(x[:len(QNAN_PAYLOADS)]))
    assert (got[len(QNAN_PAYLOADS):] == 2.5).all()


@pytest.mark.parametrize("lo,hi", [b for b in BOUNDS if b[0] != 5e-324])
def test_float_clamps_match_the_reference_forms(dm, lo, hi):
    """The float32 forms (v_maximum3_f32 / v_minimum3_f32): bit-equal to np.clip and to the compare chain on non-NaN input; a quiet NaN
    stays a NaN with its sign.  Signalling NaNs: the measured behaviour is printed, not asserted."""
    rng = np.random.default_rng(RNG_SEED + 31)
    lo32, hi32 = np.float32(lo), np.float32(hi)
    x = _clamp_inputs(rng, lo32, hi32, np.float32)
    x = x[~_zero_clash(x, lo32, hi32)]
    got, _ = dm("clamp_range_f32", x, lo32, hi32, dtype=np.float32)
    assert_bit_equal(got, np.clip(x, lo32, hi32), "clamp_range f32")
    got, _ = dm("clamp_range_hi_first_f32", x, lo32, hi32, dtype=np.float32)
    assert_bit_equal(got, _chain_hi_first(x, lo32, hi32), "clamp_range_hi_first f32")
    qn = np.array([0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFFFFFFF], np.uint32).view(np.float32)
    sn = np.array([0x7F800001, 0xFF800001, 0x7FA00000], np.uint32).view(np.float32)
    for op in ("clamp_range_f32", "clamp_range_hi_first_f32"):
        got, _ = dm(op, qn, lo32, hi32, dtype=np.float32)
        assert np.isnan(got).all() and np.array_equal(np.signbit(got), np.signbit(qn)), (op, [hex(v) for v in bits(got)])
        got, _ = dm(op, sn, lo32, hi32, dtype=np.float32)
        print(f"{op}({lo}, {hi}) on signalling NaNs {[hex(v) for v in bits(sn)]}: {[hex(v) for v in bits(got)]}")


# ============================================ glibc powf(u, 2) =======================================================================
def test_glibc_powf_square_equals_its_numpy_twin(dm):
    """glibc_powf_square (the MXV_PENDULUM_GLIBC_POWF build's u ** 2) against tools/powf_variants.py's twin: every float32 in
    [2^-3, 2], every 37th float32 of [2^-126, 2^-3), both signs (the function drops the sign first); subnormals square to +0."""
    spec = importlib.util.spec_from_file_location("powf_variants", os.path.join(ROOT, "tools", "powf_variants.py"))
    twin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(twin)
    lo8, two = np.float32(0.125).view(np.uint32), np.float32(2.0).view(np.uint32)
    all_bits = [np.arange(lo8, two + 1, dtype=np.uint32), np.arange(0x00800000, lo8, 37, dtype=np.uint32)]
    for chunk in all_bits:
        for i in range(0, chunk.size, 8_000_000):
            u = chunk[i:i + 8_000_000].view(np.float32)
            u = np.concatenate([u, -u])
            got, _ = dm("glibc_powf_square_op", u, dtype=np.float32)
            assert_bit_equal(got, twin.glibc_powf_square(u), "glibc_powf_square")
    sub = np.array([1, 2, 0x7FFFFF, 0x80000001], np.uint32).view(np.float32)
    got, _ = dm("glibc_powf_square_op", np.concatenate([sub, [0.0, -0.0]]).astype(np.float32), dtype=np.float32)
    assert not bits(got).any()
