"""tests/gae_host.py — the float64 twin the device is held to bit for bit (tests/test_gpu_gae.py) — against two independent statements of
the rule (exact rational arithmetic; a scalar per-env loop written from the prose of include/mxv_gae.h), its closed forms and its NaN
isolation; then what needs no device of the product: the argument validation of gym_amd.gae / gym_amd.discounted_returns and of the two
C entry points, and the optional header itself."""
import ctypes
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import gae_host
from conftest import HAS_GPU, ROOT
from gae_host import bits


# ---- (a) exact rationals ---------------------------------------------------------------------------------------------------------------
def rational_case(K=20, N=257, seed=2024, p=0.1):
    """gamma = 1/2, lam = 1, integer rewards in [-3, 3], values / last_value / final_values multiples of 1/16 in [-4, 4]: every A_t has a
    denominator of at most 16 * 2^K and a magnitude below 2^5, so it is a float64 exactly and float32(A_t) is one rounding of it."""
    rng = np.random.default_rng(seed)
    sixteenths = lambda shape: (rng.integers(-64, 65, shape) / 16.0).astype(np.float32)
    return dict(reward=rng.integers(-3, 4, (K, N)).astype(np.float32), terminated=(rng.random((K, N)) < p).astype(np.uint8),
                truncated=(rng.random((K, N)) < p).astype(np.uint8), values=sixteenths((K, N)), last_value=sixteenths(N),
                final_values=sixteenths((K, N)), gamma=0.5, lam=1.0)


def rational_reference(case):
    """(advantages, returns) = float32 of the exact A_t and A_t + values[t], computed with fractions.Fraction per env."""
    r, te, tr, v, lv, fv = (case[k] for k in ("reward", "terminated", "truncated", "values", "last_value", "final_values"))
    K, N = r.shape
    g, c = Fraction(case["gamma"]), Fraction(case["gamma"]) * Fraction(case["lam"])
    adv, ret = np.empty((K, N), np.float32), np.empty((K, N), np.float32)
    for n in range(N):
        A, nv = Fraction(0), Fraction(float(lv[n]))
        for t in range(K - 1, -1, -1):
            if te[t, n]:
                boot = Fraction(0)
            elif tr[t, n]:
                boot = Fraction(float(fv[t, n]))
            else:
                boot = nv
            delta = Fraction(float(r[t, n])) + g * boot - Fraction(float(v[t, n]))
            A = delta if (te[t, n] or tr[t, n]) else delta + c * A
            G = A + Fraction(float(v[t, n]))
            assert Fraction(float(A)) == A and Fraction(float(G)) == G, "not a float64: the case is not exact"
            adv[t, n], ret[t, n] = np.float32(float(A)), np.float32(float(G))
            nv = Fraction(float(v[t, n]))
    return adv, ret


def test_twin_equals_exact_rational_arithmetic():
    case = rational_case()
    both = int((case["terminated"].astype(bool) & case["truncated"].astype(bool)).sum())
    print(f"elements carrying both flags: {both}")
    assert both > 0 and case["terminated"].sum() > 100 and case["truncated"].sum() > 100
    want_adv, want_ret = rational_reference(case)
    adv, ret = gae_host.gae(**case)
    mism = int((bits(adv) != bits(want_adv)).sum() + (bits(ret) != bits(want_ret)).sum())
    print(f"mismatches against float32(Fraction): {mism}")
    assert mism == 0


# ---- (b) a scalar loop, from the prose ---------------------------------------------------------------------------------------------------
def scalar_gae(reward, terminated, truncated, values, last_value, final_values, gamma, lam):
    """One env at a time, Python floats (IEEE float64, one rounding per operation)."""
    K, N = reward.shape
    adv, ret = np.empty((K, N), np.float32), np.empty((K, N), np.float32)
    c = float(gamma) * float(lam)
    for n in range(N):
        advantage_after, value_after = 0.0, (0.0 if last_value is None else float(last_value[n]))
        for t in reversed(range(K)):
            v = float(values[t, n])
            if terminated[t, n]:
                bootstrap, ends = 0.0, True
            elif truncated[t, n]:
                bootstrap, ends = (0.0 if final_values is None else float(final_values[t, n])), True
            else:
                bootstrap, ends = value_after, False
            delta = (float(reward[t, n]) + float(gamma) * bootstrap) - v
            advantage_after = delta if ends else delta + c * advantage_after
            adv[t, n] = np.float32(advantage_after)
            ret[t, n] = np.float32(advantage_after + v)
            value_after = v
    return adv, ret


def scalar_returns(reward, terminated, truncated, last_value, final_values, gamma):
    K, N = reward.shape
    ret = np.empty((K, N), np.float32)
    for n in range(N):
        G = 0.0 if last_value is None else float(last_value[n])
        for t in reversed(range(K)):
            if terminated[t, n]:
                G = float(reward[t, n]) + float(gamma) * 0.0
            elif truncated[t, n]:
                G = float(reward[t, n]) + float(gamma) * (0.0 if final_values is None else float(final_values[t, n]))
            else:
                G = float(reward[t, n]) + float(gamma) * G
            ret[t, n] = np.float32(G)
    return ret


def random_case(K, N, seed, reward_dtype=np.float32, p=0.1):
    rng = np.random.default_rng(seed)
    return dict(reward=rng.standard_normal((K, N)).astype(reward_dtype), terminated=(rng.random((K, N)) < p).astype(np.uint8),
                truncated=(rng.random((K, N)) < p).astype(np.uint8), values=rng.standard_normal((K, N)).astype(np.float32),
                last_value=rng.standard_normal(N).astype(np.float32), final_values=rng.standard_normal((K, N)).astype(np.float32))


@pytest.mark.parametrize("reward_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("with_final, with_last", [(True, True), (False, True), (True, False), (False, False)])
def test_twin_equals_a_scalar_loop(reward_dtype, with_final, with_last):
    c = random_case(23, 67, 7, reward_dtype)
    fv, lv = (c["final_values"] if with_final else None), (c["last_value"] if with_last else None)
    adv, ret = gae_host.gae(c["reward"], c["terminated"], c["truncated"], c["values"], lv, gamma=0.99, lam=0.95, final_values=fv)
    want_adv, want_ret = scalar_gae(c["reward"], c["terminated"], c["truncated"], c["values"], lv, fv, 0.99, 0.95)
    assert np.array_equal(bits(adv), bits(want_adv)) and np.array_equal(bits(ret), bits(want_ret))
    got = gae_host.discounted_returns(c["reward"], c["terminated"], c["truncated"], gamma=0.99, last_value=lv, final_values=fv)
    assert np.array_equal(bits(got), bits(scalar_returns(c["reward"], c["terminated"], c["truncated"], lv, fv, 0.99)))


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------------
def test_constant_reward_gives_the_geometric_sum():
    K, N, g = 40, 5, 0.9
    z = np.zeros((K, N), np.uint8)
    adv, ret = gae_host.gae(np.ones((K, N), np.float32), z, z, np.zeros((K, N), np.float32), gamma=g, lam=1.0)
    want = np.array([(1 - g ** (K - t)) / (1 - g) for t in range(K)])
    assert np.allclose(adv[:, 0], want, rtol=1e-6, atol=0) and np.array_equal(bits(adv), bits(ret))
    assert np.array_equal(adv, np.repeat(adv[:, :1], N, axis=1))
    assert np.allclose(gae_host.discounted_returns(np.ones((K, N), np.float32), z, z, gamma=g)[:, 0], want, rtol=1e-6, atol=0)


def test_lambda_zero_gives_one_step_td_errors():
    c = random_case(17, 33, 11)
    adv, ret = gae_host.gae(c["reward"], c["terminated"], c["truncated"], c["values"], c["last_value"], gamma=0.97, lam=0.0,
                            final_values=c["final_values"])
    r, v = c["reward"].astype(np.float64), c["values"].astype(np.float64)
    te, tr = c["terminated"] != 0, c["truncated"] != 0
    nxt = np.vstack([v[1:], c["last_value"].astype(np.float64)[None]])
    nxt = np.where(te, 0.0, np.where(tr, c["final_values"].astype(np.float64), nxt))
    delta = (r + 0.97 * nxt) - v
    # c = gamma * 0 = 0: A_t = delta + 0 * A_{t+1} = delta (every A finite here)
    assert np.array_equal(bits(adv), bits(delta.astype(np.float32))) and np.array_equal(bits(ret), bits((delta + v).astype(np.float32)))


def test_discounted_returns_is_gae_with_zero_values_and_lambda_one():
    c = random_case(19, 41, 13, np.float64)
    zero = np.zeros((19, 41), np.float32)
    for fv in (None, c["final_values"]):
        want = gae_host.gae(c["reward"], c["terminated"], c["truncated"], zero, c["last_value"], gamma=0.99, lam=1.0, final_values=fv)[1]
        got = gae_host.discounted_returns(c["reward"], c["terminated"], c["truncated"], gamma=0.99, last_value=c["last_value"], final_values=fv)
        assert np.array_equal(bits(got), bits(want))


# ---- NaN isolation -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["terminated", "truncated"])
def test_a_nan_never_crosses_an_episode_boundary(flag):
    c = random_case(16, 9, 17, p=0.0)
    n = 4
    c["reward"][10, n] = np.nan
    c[flag][7, n] = 1
    adv, ret = gae_host.gae(c["reward"], c["terminated"], c["truncated"], c["values"], c["last_value"], final_values=c["final_values"])
    G = gae_host.discounted_returns(c["reward"], c["terminated"], c["truncated"], last_value=c["last_value"], final_values=c["final_values"])
    want = np.zeros((16, 9), bool)
    want[8:11, n] = True
    for out in (adv, ret, G):
        assert np.array_equal(np.isnan(out), want)
        assert (bits(out)[want] == 0x7FC00000).all()


def test_float32_conversion_of_the_twin():
    x = np.array([1e-40, -1e-46, 1e39, -1e39, np.nan, -np.nan, 2.0 ** -149 * 0.5, 2.0 ** -149 * 1.5, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24])
    got = bits(gae_host.to_f32(x))
    assert got[0] == 71362 and got[1] == 0x80000000 and got[2] == 0x7F800000 and got[3] == 0xFF800000      # subnormal kept, -0, +-Inf
    assert got[4] == got[5] == 0x7FC00000
    assert got[6] == 0 and got[7] == 2 and got[8] == 0x3F800000 and got[9] == 0x3F800002                     # ties to even


# ---- argument validation: Python ---------------------------------------------------------------------------------------------------------
def _torch_case(K=4, N=6):
    import torch

    return dict(reward=torch.zeros(K, N), terminated=torch.zeros(K, N, dtype=torch.uint8), truncated=torch.zeros(K, N, dtype=torch.bool),
                values=torch.zeros(K, N))


@pytest.mark.parametrize("change, names", [
    (dict(reward="f16"), ["reward"]), (dict(reward="3d"), ["reward"]), (dict(terminated="f32"), ["terminated"]),
    (dict(truncated="shape"), ["truncated"]), (dict(values="f64"), ["values"]), (dict(values="shape"), ["values"]),
    (dict(values="colstride"), ["values"]), (dict(values="rowstride"), ["row stride"]), (dict(last_value="shape"), ["last_value"]),
    (dict(last_value="f64"), ["last_value"]), (dict(final_values="shape"), ["final_values"]), (dict(final_values="i32"), ["final_values"]),
    (dict(out="count"), ["out"]), (dict(out="f64"), ["out"]), (dict(gamma=float("nan")), ["gamma"]), (dict(lam=float("inf")), ["lam"]),
    (dict(reward="numpy"), ["reward"]), (dict(), ["reward", "device"]),
])
def test_python_arguments_are_checked_before_any_device_work(change, names):
    """Wrong dtype, wrong shape, a stride the ABI cannot express, a non-finite scalar, and — last — a CPU tensor: ValueError naming the
    argument.  CPU tensors throughout, so a correct call here fails at the device check and nothing reaches the library."""
    import torch

    import gym_amd

    K, N = 4, 6
    make = {"f16": lambda: torch.zeros(K, N, dtype=torch.float16), "f32": lambda: torch.zeros(K, N), "f64": lambda: torch.zeros(K, N, dtype=torch.float64),
            "i32": lambda: torch.zeros(K, N, dtype=torch.int32), "3d": lambda: torch.zeros(K, N, 1), "shape": lambda: torch.zeros(K, N + 1),
            "colstride": lambda: torch.zeros(K, 2 * N)[:, ::2], "rowstride": lambda: torch.zeros(K, N + 3)[:, :N], "numpy": lambda: np.zeros((K, N), np.float32)}
    kw = _torch_case(K, N)
    for k, v in change.items():
        if k in ("gamma", "lam"):
            kw[k] = v
        elif k == "last_value":
            kw[k] = torch.zeros(N + 1) if v == "shape" else torch.zeros(N, dtype=torch.float64)
        elif k == "out":
            kw[k] = (torch.zeros(K, N),) if v == "count" else (torch.zeros(K, N), torch.zeros(K, N, dtype=torch.float64))
        else:
            kw[k] = make[v]()
    with pytest.raises(ValueError) as ei:
        gym_amd.gae(**kw)
    assert all(n in str(ei.value) for n in names), str(ei.value)
    if set(change) & {"values", "lam"}:
        return
    kw.pop("values")
    if "out" in kw:
        kw["out"] = torch.zeros(K, N, dtype=torch.float64) if change["out"] == "f64" else (torch.zeros(K, N), torch.zeros(K, N))
    with pytest.raises(ValueError) as ei:
        gym_amd.discounted_returns(**kw)
    assert all(n in str(ei.value) for n in names), str(ei.value)


# ---- argument validation: the C entry points ------------------------------------------------------------------------------------------------
A = 1 << 20      # distinct, aligned, never dereferenced: every call below must return before the device is touched


def _c_gae(**over):
    from gym_amd import returns

    a = dict(stream=None, K=8, N=16, reward=1 * A, f64=0, ld=16, term=2 * A, trunc=3 * A, values=4 * A, last=5 * A, final=6 * A, gamma=0.99,
             lam=0.95, adv=7 * A, ret=8 * A, ld_out=16)
    a.update(over)
    rc = returns.lib.mxv_gae(a["stream"], a["K"], a["N"], a["reward"], a["f64"], a["ld"], a["term"], a["trunc"], a["values"], a["last"],
                             a["final"], a["gamma"], a["lam"], a["adv"], a["ret"], a["ld_out"])
    return rc, returns.lib.mxv_gae_last_error().decode()


def _c_ret(**over):
    from gym_amd import returns

    a = dict(stream=None, K=8, N=16, reward=1 * A, f64=1, ld=16, term=2 * A, trunc=3 * A, last=None, final=None, gamma=0.99, ret=8 * A, ld_out=16)
    a.update(over)
    rc = returns.lib.mxv_discounted_returns(a["stream"], a["K"], a["N"], a["reward"], a["f64"], a["ld"], a["term"], a["trunc"], a["last"],
                                            a["final"], a["gamma"], a["ret"], a["ld_out"])
    return rc, returns.lib.mxv_gae_last_error().decode()


BAD_BOTH = [(dict(reward=None), "reward"), (dict(term=None), "terminated"), (dict(trunc=None), "truncated"), (dict(ret=None), "returns"),
            (dict(K=0), "K"), (dict(N=0), "N"), (dict(N=-3), "N"), (dict(ld=15), "ld"), (dict(ld_out=15), "ld_out"),
            (dict(K=1 << 21, ld=(1 << 19) + 1), "2^40"), (dict(K=1 << 21, ld_out=(1 << 19) + 1), "2^40"),
            (dict(gamma=float("nan")), "gamma"), (dict(gamma=float("inf")), "gamma"), (dict(reward=A + 2), "aligned"),
            (dict(ret=8 * A + 1), "aligned"), (dict(ret=1 * A), "overlaps input reward"), (dict(ret=3 * A - 4), "overlaps input truncated"),
            (dict(ret=2 * A + 8 * 16 - 4), "overlaps input terminated"), (dict(last=8 * A + 4 * 40), "overlaps input last_value"),
            (dict(final=8 * A - 4 * 100), "overlaps input final_values")]


@pytest.mark.parametrize("over, word", BAD_BOTH + [(dict(values=None), "values"), (dict(adv=None), "advantages"), (dict(lam=float("nan")), "lam"),
                                                   (dict(adv=4 * A + 64), "overlaps input values"), (dict(adv=8 * A + 4), "outputs advantages and returns overlap"),
                                                   (dict(f64=1, reward=A + 4), "aligned")])
def test_mxv_gae_refuses_bad_arguments_before_touching_the_device(over, word):
    from gym_amd import _native

    rc, msg = _c_gae(**over)
    assert rc == _native.ERR_INVALID_ARG and msg.startswith("mxv_gae:") and word in msg, (rc, msg)


@pytest.mark.parametrize("over, word", BAD_BOTH)
def test_mxv_discounted_returns_refuses_bad_arguments_before_touching_the_device(over, word):
    from gym_amd import _native

    rc, msg = _c_ret(**over)
    assert rc == _native.ERR_INVALID_ARG and msg.startswith("mxv_discounted_returns:") and word in msg, (rc, msg)


ACCEPTED = [
    dict(f64=0, ret=1 * A + 4 * (7 * 16 + 16)),                                   # the output begins where the last input element ends
    dict(f64=0, ld=64, ld_out=64, ret=1 * A + 4 * 16),                            # column blocks of one wide buffer: reward | returns
    dict(f64=0, ld=64, ld_out=64, ret=1 * A + 4 * 48, final=1 * A + 4 * 16, last=5 * A),      # ... | final_values | . | returns
    dict(f64=1, ld=32, ld_out=64, ret=1 * A + 8 * 16),        # float64 reward | float32 returns: different elements, one 256-byte row stride
]


@pytest.mark.skipif(HAS_GPU, reason="only meaningful where no HIP device exists: with one the call would launch on invented addresses")
@pytest.mark.parametrize("over", ACCEPTED)
def test_abutting_ranges_and_column_blocks_are_not_an_overlap(over):
    """Ranges that only touch, and ranges that interleave as column blocks with one row stride, share no byte.  (The call then reaches
    the launch; without a device that fails as MXV_ERR_HIP — never as an argument error, and never by dereferencing the pointers.)"""
    from gym_amd import _native

    rc, msg = _c_ret(**over)
    assert rc == _native.ERR_HIP and "overlap" not in msg, (rc, msg)


@pytest.mark.parametrize("over, word", [
    (dict(f64=0, ld=64, ld_out=64, ret=1 * A + 4 * 8), "overlaps input reward"),          # the column blocks share 8 columns
    (dict(f64=0, ld=64, ld_out=64, ret=1 * A + 4 * 56), "overlaps input reward"),         # the block wraps into the next row's reward
    (dict(f64=0, ld=64, ld_out=48, ret=1 * A + 4 * 16), "overlaps input reward"),         # interleaved with another row stride: not told apart
])
def test_interleaved_ranges_that_share_bytes_or_cannot_be_told_apart_are_refused(over, word):
    from gym_amd import _native

    rc, msg = _c_ret(**over)
    assert rc == _native.ERR_INVALID_ARG and word in msg, (rc, msg)


def test_last_launch_refuses_null_outputs_and_reports_no_launch_without_a_device():
    from gym_amd import _native, returns

    assert returns.lib.mxv_gae_last_launch(None, None) == _native.ERR_INVALID_ARG
    if not HAS_GPU:
        assert returns.last_launch() == (0, 0)


@pytest.mark.parametrize("good", [0.5, 1, np.float32(0.5), np.float64(0.5), np.array(0.5)])
def test_real_scalars_of_any_kind_are_taken_and_bools_are_not(good):
    from gym_amd import returns

    assert returns._scalar("gamma", good) == float(good)
    for bad in (True, "0.9", None, float("nan"), np.float32("inf"), [0.5, 0.5]):
        with pytest.raises(ValueError, match="gamma"):
            returns._scalar("gamma", bad)


def test_pre_step_observations_shifts_the_trajectory_by_one_step():
    import torch

    from gym_amd import returns

    first, obs = torch.full((5, 4), -1.0), torch.arange(3 * 5 * 4, dtype=torch.float32).reshape(3, 5, 4)
    pre = returns.pre_step_observations(first, obs)
    assert pre.shape == obs.shape and torch.equal(pre[0], first) and torch.equal(pre[1:], obs[:-1])
    with pytest.raises(ValueError, match="first_obs"):
        returns.pre_step_observations(torch.zeros(4), obs)


# ---- the header and its bindings ------------------------------------------------------------------------------------------------------------
def _prototypes():
    text = open(os.path.join(ROOT, "include", "mxv_gae.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(2): (m.group(1).strip(), " ".join(m.group(3).split()))
            for m in re.finditer(r"\n\s*((?:const\s+)?[A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(mxv_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_is_optional_self_contained_and_bound_outside_the_core_exports():
    from gym_amd import _native, returns

    protos = _prototypes()
    assert sorted(protos) == sorted(returns.GAE_EXPORTS)
    assert not set(protos) & set(_native.EXPORTS)
    assert '#include "mxv_gae.h"' not in open(os.path.join(ROOT, "include", "mxv.h")).read()
    lib = ctypes.CDLL(_native.LIB_PATH)
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, (ret, args) in protos.items():
        assert hasattr(lib, name) and name in notes, name
        f = getattr(returns.lib, name)
        n_args = 0 if args in ("", "void") else len(args.split(","))
        assert len(f.argtypes) == n_args, (name, args)
        for a, t in zip(args.split(","), f.argtypes):
            want = ctypes.c_void_p if "*" in a else {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double}[a.split()[0]]
            assert t is want, (name, a, t)
        assert f.restype is (ctypes.c_char_p if "char" in ret else ctypes.c_int), name
    if shutil.which("gcc"):
        for comp, ext, std in (("gcc", "c", "-std=c99"), ("g++", "cpp", "-std=c++11")):
            p = subprocess.run([comp, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x",
                                "c" if ext == "c" else "c++", "-"], input='#include "mxv_gae.h"\nint main(void) { return 0; }\n',
                               capture_output=True, text=True)
            assert p.returncode == 0, (comp, p.stderr[-1500:])
