"""tests/vtrace_host.py — the float64 twin the device is held to bit for bit (tests/test_gpu_vtrace.py) — against an independent scalar
loop written from the prose of include/mxv_vtrace.h and against the paper's definition (Espeholt et al. 2018, eq. 1 and the policy
gradient of §4.2) in 200-bit mpmath; its two bit identities (on-policy vs = GAE returns, w = the PPO ratio); its NaN isolation and its
clamp; then what needs no device of the product: the argument validation of gym_amd.vtrace and the optional header itself."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gae_host
import policy_host as ph
import ppo_host
import vtrace_host
from conftest import ROOT
from vtrace_host import bits

HEADER = "mxv_vtrace.h"


def random_case(K, N, seed, reward_dtype=np.float32, p=0.1, spread=3.0):
    """done probability p per flag, |log_prob - old_log_prob| up to `spread`."""
    rng = np.random.default_rng(seed)
    old = -np.abs(rng.standard_normal((K, N))).astype(np.float32)
    return dict(log_prob=(old + rng.uniform(-spread, spread, (K, N))).astype(np.float32), old_log_prob=old,
                reward=rng.standard_normal((K, N)).astype(reward_dtype), terminated=(rng.random((K, N)) < p).astype(np.uint8),
                truncated=(rng.random((K, N)) < p).astype(np.uint8), values=rng.standard_normal((K, N)).astype(np.float32),
                last_value=rng.standard_normal(N).astype(np.float32), final_values=rng.standard_normal((K, N)).astype(np.float32))


def twin(c, f=vtrace_host.vtrace, with_final=True, with_last=True, **kw):
    return f(c["log_prob"], c["old_log_prob"], c["reward"], c["terminated"], c["truncated"], c["values"], c["last_value"] if with_last else None,
             final_values=c["final_values"] if with_final else None, **kw)


# ---- (a) a scalar loop, from the prose ---------------------------------------------------------------------------------------------------
def scalar_exp(d):
    """EXP on Python floats (IEEE float64, one rounding per operation); round() ties to even like rint."""
    k = float(round(d * float(ph.INV_LN2)))
    r = (d - k * float(ph.LN2_HI)) - k * float(ph.LN2_LO)
    p = float(ph.EXP_C[-1])
    for c in ph.EXP_C[-2::-1]:
        p = p * r + float(c)
    return math.ldexp(p, int(k))


def scalar_vtrace(c, with_final, with_last, gamma, lam, rho_bar, c_bar, pg_rho_bar):
    """One env at a time."""
    K, N = c["reward"].shape
    vs_out, pg_out = np.empty((K, N), np.float32), np.empty((K, N), np.float32)
    for n in range(N):
        trace = 0.0
        value_after = float(c["last_value"][n]) if with_last else 0.0
        target_after = value_after
        for t in reversed(range(K)):
            log_ratio = float(c["log_prob"][t, n]) - float(c["old_log_prob"][t, n])
            log_ratio = min(max(log_ratio, -80.0), 80.0)
            w = scalar_exp(log_ratio)
            v, r = float(c["values"][t, n]), float(c["reward"][t, n])
            if c["terminated"][t, n]:
                bootstrap, ends = 0.0, True
            elif c["truncated"][t, n]:
                bootstrap, ends = (float(c["final_values"][t, n]) if with_final else 0.0), True
            else:
                bootstrap, ends = value_after, False
            td = min(w, rho_bar) * ((r + gamma * bootstrap) - v)
            trace = td if ends else td + (gamma * (lam * min(w, c_bar))) * trace
            target = trace + v
            pg = min(w, pg_rho_bar) * ((r + gamma * (bootstrap if ends else target_after)) - v)
            vs_out[t, n], pg_out[t, n] = np.float32(target), np.float32(pg)
            value_after, target_after = v, target
    return vs_out, pg_out


@pytest.mark.parametrize("reward_dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("with_final, with_last", [(True, True), (False, True), (True, False), (False, False)])
def test_twin_equals_a_scalar_loop(reward_dtype, with_final, with_last):
    c = random_case(23, 67, 7, reward_dtype)
    done = (c["terminated"] != 0) | (c["truncated"] != 0)
    assert 0.1 < done.mean() < 0.3 and np.abs(c["log_prob"].astype(np.float64) - c["old_log_prob"]).max() > 2.9
    for kw in (dict(gamma=0.99, lam=0.95, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0), dict(gamma=0.97, lam=1.0, rho_bar=1.5, c_bar=0.8, pg_rho_bar=2.0)):
        got = twin(c, with_final=with_final, with_last=with_last, **kw)
        want = scalar_vtrace(c, with_final, with_last, **kw)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))


# ---- (b) the paper's definition, 200 bits -------------------------------------------------------------------------------------------------
def paper_reference(c, gamma, lam, rho_bar, c_bar, pg_rho_bar):
    """Per element (vs, sum |terms| of vs, pg, sum |terms| of pg) as mpmath numbers: vs_t = V_t + sum_{k >= t} gamma^(k-t) (prod_{t <= i < k}
    lam min(c_bar, w_i)) min(rho_bar, w_k) (r_k + gamma V_{k+1} - V_k) written out as that sum, the episode ending where a flag is set;
    pg_t = min(pg_rho_bar, w_t) (r_t + gamma vs_{t+1} - V_t)."""
    import mpmath as mp

    K, N = c["reward"].shape
    f = lambda x: mp.mpf(float(x))
    g, lm, rb, cb, pb = f(gamma), f(lam), f(rho_bar), f(c_bar), f(pg_rho_bar)
    out = {}
    for n in range(N):
        w = [mp.exp(f(c["log_prob"][t, n]) - f(c["old_log_prob"][t, n])) for t in range(K)]
        V = [f(c["values"][t, n]) for t in range(K)]
        r = [f(c["reward"][t, n]) for t in range(K)]
        nxt, done = [], []
        for t in range(K):
            te, tr = bool(c["terminated"][t, n]), bool(c["truncated"][t, n])
            done.append(te or tr)
            nxt.append(mp.mpf(0) if te else f(c["final_values"][t, n]) if tr else (V[t + 1] if t + 1 < K else f(c["last_value"][n])))
        vs, mag = [None] * K, [None] * K
        for t in range(K):
            total, size, coef = V[t], abs(V[t]), mp.mpf(1)
            for k in range(t, K):
                rho = min(rb, w[k])
                total += coef * rho * (r[k] + g * nxt[k] - V[k])
                size += abs(coef * rho) * (abs(r[k]) + abs(g * nxt[k]) + abs(V[k]))
                if done[k]:
                    break
                coef *= g * lm * min(cb, w[k])
            vs[t], mag[t] = total, size
        for t in range(K):
            after, after_mag = (nxt[t], abs(nxt[t])) if done[t] or t + 1 == K else (vs[t + 1], mag[t + 1])
            rpg = min(pb, w[t])
            out[t, n] = (vs[t], mag[t], rpg * (r[t] + g * after - V[t]), rpg * (abs(r[t]) + abs(g) * after_mag + abs(V[t])))
    return out


def _ulp32(x):
    x = abs(float(x))
    return float(np.spacing(np.float32(x))) if x >= float(np.finfo(np.float32).tiny) else 2.0 ** -149


def test_twin_against_the_papers_definition_in_200_bit_arithmetic():
    """The error of the float64 results in units of 2^-53 * sum |terms| stays below twice the recorded measurement, rounded up (random
    inputs do not visit the polynomial's worst cases); the float32 outputs lie within half a float32 ulp of the exact value plus that bar."""
    import mpmath as mp

    worst_vs = worst_pg = 0.0
    with mp.workprec(200):
        for seed, kw in ((11, dict(gamma=0.99, lam=0.95, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0)),
                         (12, dict(gamma=0.97, lam=1.0, rho_bar=1.5, c_bar=0.8, pg_rho_bar=1.2)),
                         (13, dict(gamma=0.995, lam=0.9, rho_bar=0.9, c_bar=1.5, pg_rho_bar=1.0))):
            c = random_case(24, 400, seed, np.float64 if seed == 12 else np.float32)
            v64, p64 = twin(c, vtrace_host.vtrace_f64, **kw)
            v32, p32 = twin(c, **kw)
            ref = paper_reference(c, **kw)
            unit = mp.mpf(2) ** -53
            for (t, n), (vs, vmag, pg, pmag) in ref.items():
                worst_vs = max(worst_vs, float(abs(mp.mpf(float(v64[t, n])) - vs) / (unit * vmag)))
                worst_pg = max(worst_pg, float(abs(mp.mpf(float(p64[t, n])) - pg) / (unit * pmag)))
                assert abs(mp.mpf(float(v32[t, n])) - vs) <= mp.mpf(_ulp32(vs)) / 2 + vtrace_host.BAR_VS * unit * vmag, (seed, t, n)
                assert abs(mp.mpf(float(p32[t, n])) - pg) <= mp.mpf(_ulp32(pg)) / 2 + vtrace_host.BAR_PG * unit * pmag, (seed, t, n)
    print(f"largest error in units of 2^-53 sum|terms|: vs {worst_vs:.2f} (recorded {vtrace_host.B_VS}), pg {worst_pg:.2f} (recorded {vtrace_host.B_PG})")
    assert worst_vs <= vtrace_host.BAR_VS and worst_pg <= vtrace_host.BAR_PG
    assert vtrace_host.BAR_VS == math.ceil(2 * vtrace_host.B_VS) and vtrace_host.BAR_PG == math.ceil(2 * vtrace_host.B_PG)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert f"B_VS = {vtrace_host.B_VS}" in design and f"B_PG = {vtrace_host.B_PG}" in design


# ---- the two bit identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 0.5, 0.9, 0.95, 1.0])
def test_on_policy_vs_has_the_bits_of_gae_returns(lam):
    for seed, dtype in ((21, np.float32), (22, np.float64)):
        c = random_case(19, 83, seed, dtype)
        c["log_prob"] = c["old_log_prob"].copy()
        for levels in (dict(), dict(rho_bar=1.0, c_bar=3.0), dict(rho_bar=2.5, c_bar=1.0, pg_rho_bar=0.5)):
            for with_final, with_last in ((True, True), (False, False)):
                vs, _ = twin(c, with_final=with_final, with_last=with_last, gamma=0.97, lam=lam, **levels)
                ret = gae_host.gae(c["reward"], c["terminated"], c["truncated"], c["values"], c["last_value"] if with_last else None, gamma=0.97,
                                   lam=lam, final_values=c["final_values"] if with_final else None)[1]
                assert np.array_equal(bits(vs), bits(ret)), (lam, levels)
    assert ph.EXP(np.float64(0.0)) == 1.0


def test_w_has_the_bits_of_the_ppo_ratio():
    c = random_case(9, 500, 31, spread=100.0)
    c["log_prob"][0, :5] = [np.nan, np.inf, -np.inf, 80.0, -80.0]
    c["old_log_prob"][0, :5] = [0.0, 0.0, 0.0, 0.0, 0.0]
    c["old_log_prob"][1, :3] = [np.nan, np.inf, -np.inf]
    c["log_prob"][1, 1:3] = [np.inf, -np.inf]                # Inf - Inf: NaN
    w = vtrace_host.weights(c["log_prob"], c["old_log_prob"])
    r = ppo_host.rows(c["log_prob"].reshape(-1), c["old_log_prob"].reshape(-1), np.zeros(c["log_prob"].size, np.float32))["r"]
    assert np.array_equal(w.reshape(-1).view(np.uint64), r.view(np.uint64))
    assert np.isnan(w[0, 0]) and np.isnan(w[1, :3]).all() and w[0, 1] == w[0, 3] == ph.EXP(np.float64(80.0)) and w[0, 2] == w[0, 4]


# ---- NaN isolation, the clamp -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["terminated", "truncated"])
@pytest.mark.parametrize("key", ["log_prob", "old_log_prob", "reward", "values", "final_values", "last_value"])
@pytest.mark.parametrize("special", [np.nan, np.inf, -np.inf])
def test_a_non_finite_value_just_after_a_boundary_leaves_the_rows_before_it_untouched(flag, key, special):
    K, N, n = 16, 9, 4
    c = random_case(K, N, 17, p=0.0)
    c[flag][7, n] = 1
    clean = twin(c, lam=0.95, c_bar=1.5)
    if key == "last_value":
        c[key][n] = special
    elif key == "final_values":
        c[key][8, n] = special            # not read: no flag there ...
        c["truncated"][12, n] = 1
        c[key][12, n] = special           # ... read here, in the later episode
    else:
        c[key][8, n] = special
    got = twin(c, lam=0.95, c_bar=1.5)
    for a, b in zip(got, clean):
        assert np.array_equal(bits(a)[:8], bits(b)[:8])               # rows 0..7, the boundary's own included: every env
        assert np.array_equal(np.delete(bits(a), n, 1), np.delete(bits(b), n, 1))
    if key in ("reward", "values", "last_value") or (key == "final_values" and flag == "terminated"):
        assert not np.isfinite(got[0][8, n])       # the case does reach row 8 (final_values: through the truncation at row 12)


def test_a_nan_log_prob_gives_nan_in_its_own_episodes_earlier_rows_only():
    K, N, n = 16, 9, 4
    c = random_case(K, N, 19, p=0.0)
    c["terminated"][3, n] = 1
    c["truncated"][11, n] = 1
    c["log_prob"][8, n] = np.nan
    vs, pg = twin(c, lam=0.95)
    want = np.zeros((K, N), bool)
    want[4:9, n] = True                       # rows 4..8: from the first row behind the boundary at row 3 up to the NaN's own row
    assert np.array_equal(np.isnan(vs), want)
    # pg_t reads vs_{t+1}: rows 7 .. 4 through it, row 8 through its own weight; row 3 ends its episode and reads nothing of row 4
    assert np.array_equal(np.isnan(pg), want)
    assert (bits(vs)[want] == 0x7FC00000).all() and (bits(pg)[want] == 0x7FC00000).all()


def test_log_ratios_beyond_80_clamp():
    c = random_case(3, 8, 23, p=0.0)
    c["old_log_prob"][:] = 0.0
    base = dict(c)
    for big, edge in ((np.float32(81.0), 80.0), (np.float32(1e30), 80.0), (np.float32(np.inf), 80.0), (np.float32(-81.0), -80.0), (np.float32(-np.inf), -80.0)):
        a, b = dict(base), dict(base)
        a["log_prob"] = np.full((3, 8), big, np.float32)
        b["log_prob"] = np.full((3, 8), edge, np.float32)
        for levels in (dict(rho_bar=1e300, c_bar=1e300), dict()):
            ga, gb = twin(a, **levels), twin(b, **levels)
            assert np.array_equal(bits(ga[0]), bits(gb[0])) and np.array_equal(bits(ga[1]), bits(gb[1]))
            assert np.isfinite(twin(a, vtrace_host.vtrace_f64, **levels)[0]).all()      # (the float32 of it may overflow)
    w = vtrace_host.weights(np.float32([[80.0, -80.0, 79.5]]), np.float32([[0.0, 0.0, 0.0]]))
    assert w[0, 0] == ph.EXP(np.float64(80.0)) > 5e34 and w[0, 1] == ph.EXP(np.float64(-80.0)) < 2e-35 and w[0, 2] < w[0, 0]


# ---- argument validation: Python ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change, names", [
    (dict(log_prob="f64"), ["log_prob"]), (dict(old_log_prob="shape"), ["old_log_prob"]), (dict(reward="f16"), ["reward"]), (dict(reward="3d"), ["reward"]),
    (dict(terminated="f32"), ["terminated"]), (dict(truncated="shape"), ["truncated"]), (dict(values="f64"), ["values"]),
    (dict(values="colstride"), ["values"]), (dict(log_prob="rowstride"), ["row stride"]), (dict(last_value="shape"), ["last_value"]),
    (dict(last_value="f64"), ["last_value"]), (dict(final_values="shape"), ["final_values"]), (dict(final_values="i32"), ["final_values"]),
    (dict(out="count"), ["out"]), (dict(out="one"), ["out"]), (dict(out="f64"), ["out"]), (dict(gamma=float("nan")), ["gamma"]), (dict(lam=float("inf")), ["lam"]),
    (dict(rho_bar=float("inf")), ["rho_bar"]), (dict(rho_bar=0.0), ["rho_bar", "greater than 0"]), (dict(c_bar=-1.0), ["c_bar", "greater than 0"]),
    (dict(c_bar=float("nan")), ["c_bar"]), (dict(pg_rho_bar=0.0), ["pg_rho_bar", "greater than 0"]), (dict(pg_rho_bar="1"), ["pg_rho_bar"]),
    (dict(reward="numpy"), ["reward"]), (dict(), ["log_prob", "device"]),
])
def test_python_arguments_are_checked_before_any_device_work(change, names):
    """Wrong dtype, wrong shape, a stride the ABI cannot express, a non-finite scalar, a clip level <= 0, a wrong number of outputs, and —
    last — a CPU tensor: ValueError naming the argument.  CPU tensors throughout, so a correct call here fails at the device check and
    nothing reaches the library."""
    import torch

    import gym_amd

    K, N = 4, 6
    make = {"f16": lambda: torch.zeros(K, N, dtype=torch.float16), "f32": lambda: torch.zeros(K, N), "f64": lambda: torch.zeros(K, N, dtype=torch.float64),
            "i32": lambda: torch.zeros(K, N, dtype=torch.int32), "3d": lambda: torch.zeros(K, N, 1), "shape": lambda: torch.zeros(K, N + 1),
            "colstride": lambda: torch.zeros(K, 2 * N)[:, ::2], "rowstride": lambda: torch.zeros(K, N + 3)[:, :N], "numpy": lambda: np.zeros((K, N), np.float32)}
    kw = dict(log_prob=torch.zeros(K, N), old_log_prob=torch.zeros(K, N), reward=torch.zeros(K, N), terminated=torch.zeros(K, N, dtype=torch.uint8),
              truncated=torch.zeros(K, N, dtype=torch.bool), values=torch.zeros(K, N))
    for k, v in change.items():
        if k in ("gamma", "lam", "rho_bar", "c_bar", "pg_rho_bar"):
            kw[k] = v
        elif k == "last_value":
            kw[k] = torch.zeros(N + 1) if v == "shape" else torch.zeros(N, dtype=torch.float64)
        elif k == "out":
            kw[k] = {"count": (torch.zeros(K, N),) * 3, "one": torch.zeros(K, N), "f64": (torch.zeros(K, N), torch.zeros(K, N, dtype=torch.float64))}[v]
        else:
            kw[k] = make[v]()
    with pytest.raises(ValueError) as ei:
        gym_amd.vtrace(**kw)
    assert all(n in str(ei.value) for n in names), str(ei.value)


def test_the_module_is_the_function_and_does_not_import_torch():
    import sys

    out = subprocess.run([sys.executable, "-c", "import sys, gym_amd\nf = gym_amd.vtrace\nimport gym_amd.vtrace as m\n"
                          "assert f is m and gym_amd.vtrace is m and callable(m) and m.vtrace.__name__ == 'vtrace'\n"
                          "from gym_amd import vtrace\nassert vtrace is m\nprint('torch' in sys.modules, m.last_launch())"],
                         capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0 and out.stdout.split()[0] == "False", out.stdout + out.stderr


# ---- the C entry point through ctypes -------------------------------------------------------------------------------------------------------
A = 1 << 20      # distinct, aligned, never dereferenced: every call below must return before the device is touched


def _c_call(**over):
    from gym_amd import vtrace as m

    a = dict(stream=None, K=8, N=16, lp=9 * A, old=10 * A, reward=1 * A, f64=0, ld=16, term=2 * A, trunc=3 * A, values=4 * A, last=5 * A, final=6 * A,
             gamma=0.99, lam=0.95, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0, vs=7 * A, pg=8 * A, ld_out=16)
    a.update(over)
    rc = m.lib.mxv_vtrace(a["stream"], a["K"], a["N"], a["lp"], a["old"], a["reward"], a["f64"], a["ld"], a["term"], a["trunc"], a["values"], a["last"],
                          a["final"], a["gamma"], a["lam"], a["rho_bar"], a["c_bar"], a["pg_rho_bar"], a["vs"], a["pg"], a["ld_out"])
    return rc, m.lib.mxv_vtrace_last_error().decode()


@pytest.mark.parametrize("over, word", [
    (dict(lp=None), "log_prob"), (dict(old=None), "old_log_prob"), (dict(reward=None), "reward"), (dict(term=None), "terminated"), (dict(trunc=None), "truncated"),
    (dict(values=None), "values"), (dict(vs=None), "vs pointer"), (dict(pg=None), "pg_advantages pointer"), (dict(K=0), "K"), (dict(N=0), "N"), (dict(N=-3), "N"),
    (dict(ld=15), "ld"), (dict(ld_out=15), "ld_out"), (dict(K=1 << 21, ld=(1 << 19) + 1), "2^40"), (dict(K=1 << 21, ld_out=(1 << 19) + 1), "2^40"),
    (dict(gamma=float("nan")), "gamma"), (dict(lam=float("inf")), "lam"), (dict(rho_bar=float("nan")), "rho_bar"), (dict(rho_bar=0.0), "rho_bar"),
    (dict(c_bar=-0.5), "c_bar"), (dict(c_bar=float("inf")), "c_bar"), (dict(pg_rho_bar=0.0), "pg_rho_bar"), (dict(pg_rho_bar=float("-inf")), "pg_rho_bar"),
    (dict(lp=9 * A + 2), "log_prob pointer"), (dict(f64=1, reward=A + 4), "aligned"), (dict(pg=8 * A + 1), "aligned"), (dict(last=5 * A + 2), "last_value pointer"),
    (dict(vs=9 * A), "overlaps input log_prob"), (dict(pg=10 * A + 64), "overlaps input old_log_prob"), (dict(vs=3 * A - 4), "overlaps input truncated"),
    (dict(last=8 * A + 4 * 40), "overlaps input last_value"), (dict(final=8 * A - 4 * 100), "overlaps input final_values"),
    (dict(pg=7 * A + 4), "outputs vs and pg_advantages overlap"),
    (dict(ld=64, ld_out=64, vs=1 * A + 4 * 8), "overlaps input reward"),          # column blocks that share 8 columns
    (dict(ld=64, ld_out=48, vs=1 * A + 4 * 16), "overlaps input reward"),         # interleaved with another row stride: not told apart
])
def test_mxv_vtrace_refuses_bad_arguments_before_touching_the_device(over, word):
    from gym_amd import _native

    rc, msg = _c_call(**over)
    assert rc == _native.ERR_INVALID_ARG and msg.startswith("mxv_vtrace:") and word in msg, (rc, msg)


def test_last_launch_refuses_null_outputs():
    from gym_amd import _native
    from gym_amd import vtrace as m

    assert m.lib.mxv_vtrace_last_launch(None, None) == _native.ERR_INVALID_ARG
    assert "mxv_vtrace_last_launch" in m.lib.mxv_vtrace_last_error().decode()


# ---- the header and its bindings ----------------------------------------------------------------------------------------------------------
def _prototypes():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(2): (m.group(1).strip(), " ".join(m.group(3).split()))
            for m in re.finditer(r"\n\s*((?:const\s+)?[A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(mxv_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_is_optional_self_contained_and_bound_outside_the_other_exports():
    from gym_amd import _native, policy, policy_eval, ppo, returns
    from gym_amd import vtrace as m

    protos = _prototypes()
    assert sorted(protos) == sorted(m.VTRACE_EXPORTS) and len(protos) == 3
    others = set(_native.EXPORTS) | set(returns.GAE_EXPORTS) | set(policy.POLICY_EXPORTS) | set(policy_eval.EVAL_EXPORTS) | set(ppo.PPO_EXPORTS)
    assert not set(protos) & others
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != HEADER:
            assert HEADER not in open(os.path.join(ROOT, "include", other)).read(), other
    lib = ctypes.CDLL(_native.LIB_PATH)
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, (ret, args) in protos.items():
        assert hasattr(lib, name) and name in notes, name
        f = getattr(m.lib, name)
        n_args = 0 if args in ("", "void") else len(args.split(","))
        assert len(f.argtypes) == n_args, (name, args)
        for a, t in zip(args.split(","), f.argtypes):
            want = ctypes.c_void_p if "*" in a else {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double}[a.split()[0]]
            assert t is want, (name, a, t)
        assert f.restype is (ctypes.c_char_p if "char" in ret else ctypes.c_int), name
    assert m.RING_DEPTH == returns.RING_DEPTH and m.VECTOR_MIN_ENVS == returns.VECTOR_MIN_ENVS      # GAE's switch-over


def test_header_compiles_on_its_own_as_c99_and_as_cpp11():
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    for comp, lang, std in (("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++11")):
        p = subprocess.run([comp, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", lang, "-"],
                           input=f'#include "{HEADER}"\nint main(void) {{ return 0; }}\n', capture_output=True, text=True)
        assert p.returncode == 0, (comp, p.stderr[-1500:])


def test_the_rule_is_stated_in_the_header_line_by_line():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    for line in ("d     = log_prob[t] - old_log_prob[t];  d = d < -80 ? -80 : (d > 80 ? 80 : d)",
                 "w     = isnan(d) ? NaN : EXP(isnan(d) ? 0.0 : d)",
                 "rho   = w > rho_bar ? rho_bar : w          cs = lam * (w > c_bar ? c_bar : w)          rpg = w > pg_rho_bar ? pg_rho_bar : w",
                 "done  = terminated | truncated",
                 "nv    = terminated ? 0.0 : truncated ? (final_values ? final_values[t] : 0.0) : nv_{t+1}",
                 "delta = rho * ((reward[t] + gamma * nv) - values[t])",
                 "gc    = gamma * cs",
                 "acc_t = done ? delta : delta + gc * acc_{t+1}",
                 "vs_t  = acc_t + values[t]",
                 "nvs   = done ? nv : vs_{t+1}",
                 "pg_t  = rpg * ((reward[t] + gamma * nvs) - values[t])",
                 "vs[t] = float32(vs_t)     pg_advantages[t] = float32(pg_t)     nv_t = values[t]",
                 "acc_K = 0 and nv_K = vs_K = last_value", "0x7FC00000", "EXP(0) is exactly 1", "gc = gamma * (lam * 1.0)",
                 "w has the bits of the ratio r"):
        assert line in text, line
    # the ratio lines are the PPO loss header's, operation for operation
    ppo = open(os.path.join(ROOT, "include", "mxv_ppo.h")).read()
    assert "d = d < -80 ? -80 : (d > 80 ? 80 : d)" in ppo and "d = d < -80 ? -80 : (d > 80 ? 80 : d)" in text
