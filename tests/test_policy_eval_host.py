"""tests/policy_eval_host.py — the NumPy twin of include/mxv_policy_eval.h, which the device is compared with bit for bit — held to its
neighbours and to 200-bit mpmath: the forward passes reproduce the samplers' twins on their own actions; the float64 gradients are
accurate; each row's categorical gradient sums to zero; masks, degenerate rows and out-of-range actions; what leaving a term out means.
Also what needs no device of the product: the optional header and its bindings, the constants in the kernel source, and the Python
front end's validation."""
import ctypes
import math
import os
import re
import shutil
import subprocess
import sys

import mpmath as mp
import numpy as np
import pytest

import gaussian_host as gh
import policy_eval_host as pe
import policy_host as ph
import test_gaussian_host as tgh
import test_policy_host as tph
from conftest import ROOT

ACTIONS = tph.ACTIONS          # 2, 3, 4, 6, 17 at scales 0.1 / 1 / 5 / 30
DIMS = tgh.DIMS                # 1..4, log_std in [-5, 2]
STRIDE = 1                     # every row of those tests' inputs: 3 000 rows per A and per D
TWO53 = 2.0 ** 53


def _u64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _measured(name, worst):
    """The named constant is what was measured on this input (to its two decimals, rounded up); the bar is twice that, rounded up."""
    b = getattr(pe, "B_" + name)
    print(f"measured B_{name}: {worst:.4f}")
    assert worst <= b < worst + 0.01, (name, worst, b)
    assert pe.bar(b) == int(np.ceil(2 * b)) >= worst


# ---- forward: the samplers' own lines ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", ACTIONS)
def test_categorical_forward_is_the_samplers_twin_on_its_own_actions(A):
    x, w = tph._rows(A)
    r = ph.evaluate(x, w)
    lp, en = pe.categorical(x, r["action"])
    assert np.array_equal(_u64(lp), _u64(r["log_prob"])) and np.array_equal(_u64(en), _u64(r["entropy"]))
    # any other stored action: its own d_a against the same L; the entropy does not depend on the action
    other = (r["action"] + 1) % A
    lp2, en2 = pe.categorical(x, other.astype(np.int32))
    assert np.array_equal(_u64(en2), _u64(en))
    assert np.array_equal(_u64(lp2), _u64(r["d"][np.arange(len(x)), other] - ph.LOG(r["S"])))


@pytest.mark.parametrize("D", DIMS)
def test_gaussian_forward_is_the_samplers_twin_on_its_own_actions(D):
    mean, log_std, w4 = tgh._rows(D)
    r = gh.evaluate(mean, log_std, w4)
    lp, en = pe.gaussian(mean, log_std, r["act"])
    assert np.array_equal(_u64(lp), _u64(r["log_prob"])) and np.array_equal(_u64(en), _u64(r["entropy"]))
    shared = gh.evaluate(mean, log_std[0], w4)
    lp, en = pe.gaussian(mean, log_std[0], shared["act"])
    assert np.array_equal(_u64(lp), _u64(shared["log_prob"])) and np.array_equal(_u64(en), _u64(shared["entropy"]))


# ---- gradients against 200-bit arithmetic ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def categorical_exact():
    """Per A: logits, the sampled actions, and per row the exact d log_prob / d logit and d entropy / d logit."""
    out = {}
    with mp.workprec(200):
        for A in ACTIONS:
            x, w = tph._rows(A)
            act = ph.evaluate(x, w)["action"][::STRIDE]
            x = x[::STRIDE]
            rows = []
            for i in range(len(x)):
                xs = [mp.mpf(float(v)) for v in x[i]]
                m = max(xs)
                e = [mp.exp(v - m) for v in xs]
                S = mp.fsum(e)
                q = [v / S for v in e]
                logq = [v - m - mp.log(S) for v in xs]
                H = -mp.fsum(a * b for a, b in zip(q, logq))
                rows.append(([(1 if a == act[i] else 0) - q[a] for a in range(A)], [-q[a] * (logq[a] + H) for a in range(A)]))
            out[A] = (x, act, rows)
    return out


def test_categorical_gradients_are_accurate_and_sum_to_zero(categorical_exact):
    worst_lp = worst_en = 0.0
    rng = np.random.default_rng(77)
    with mp.workprec(200):
        for A in ACTIONS:
            x, act, rows = categorical_exact[A]
            M = len(x)
            one = np.ones(M, np.float32)
            g_lp = pe.categorical_backward(x, act, grad_log_prob=one)
            g_en = pe.categorical_backward(x, act, grad_entropy=one)
            gl, gH = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
            g_both = pe.categorical_backward(x, act, gl, gH)
            assert np.all(np.isfinite(g_lp)) and np.all(np.isfinite(g_en))
            for i, (dlps, dHs) in enumerate(rows):
                for a in range(A):
                    dlp, dH = dlps[a], dHs[a]
                    worst_lp = max(worst_lp, float(abs(mp.mpf(float(g_lp[i, a])) - dlp) * TWO53))
                    worst_en = max(worst_en, float(abs(mp.mpf(float(g_en[i, a])) - dH) * TWO53))
                    # both terms: each within its bar times its factor, plus one rounding for each product and one for the sum
                    want = mp.mpf(float(gl[i])) * dlp + mp.mpf(float(gH[i])) * dH
                    tol = (abs(float(gl[i])) * pe.bar(pe.B_GRAD_LOG_PROB) + abs(float(gH[i])) * pe.bar(pe.B_GRAD_ENTROPY)
                           + abs(float(gl[i]) * float(dlp)) + abs(float(gH[i]) * float(dH)) + abs(float(want))) / TWO53
                    assert abs(mp.mpf(float(g_both[i, a])) - want) <= tol * (1 + 1e-9), (A, i, a)
                # every entry is within the bar of an exact gradient that sums to zero: the exact sum of a row is within A bars
                assert abs(math.fsum(g_lp[i])) * TWO53 <= A * pe.bar(pe.B_GRAD_LOG_PROB), (A, i)
                assert abs(math.fsum(g_en[i])) * TWO53 <= A * pe.bar(pe.B_GRAD_ENTROPY), (A, i)
    _measured("GRAD_LOG_PROB", worst_lp)
    _measured("GRAD_ENTROPY", worst_en)


def test_gaussian_gradients_are_accurate():
    worst_m = worst_s = 0.0
    with mp.workprec(200):
        for D in DIMS:
            mean, log_std, w4 = tgh._rows(D)
            act = gh.evaluate(mean, log_std, w4)["act"][::STRIDE]
            mean, log_std = mean[::STRIDE], log_std[::STRIDE]
            M = len(mean)
            one = np.ones(M, np.float32)
            g_mean, g_ls = pe.gaussian_backward(mean, log_std, act, grad_log_prob=one)
            g_mean2, g_ls2 = pe.gaussian_backward(mean, log_std, act, grad_log_prob=one, grad_entropy=one)
            assert np.array_equal(_u64(g_mean), _u64(g_mean2)) and np.array_equal(_u64(g_ls2), _u64(g_ls + 1.0))
            g_mean0, g_ls0 = pe.gaussian_backward(mean, log_std, act, grad_entropy=(3 * one))
            assert np.all(g_mean0 == 0.0) and np.all(g_ls0 == 3.0)                      # the entropy is sum(ls) + const
            for i in range(M):
                for j in range(D):
                    mu, ls = mp.mpf(float(mean[i, j])), mp.mpf(float(log_std[i, j]))
                    sigma = mp.exp(ls)
                    zq = (mp.mpf(float(act[i, j])) - mu) / sigma
                    want_m, want_s = zq / sigma, zq * zq - 1
                    if want_m == 0:
                        assert g_mean[i, j] == 0.0
                    else:
                        worst_m = max(worst_m, float(abs(mp.mpf(float(g_mean[i, j])) - want_m) / abs(want_m) * TWO53))
                    worst_s = max(worst_s, float(abs(mp.mpf(float(g_ls[i, j])) - want_s) / (zq * zq + 1) * TWO53))
    _measured("GRAD_MEAN", worst_m)
    _measured("GRAD_LOG_STD", worst_s)


# ---- masks, degenerate rows, absent terms -------------------------------------------------------------------------------------------------
def test_masked_logits():
    inf = np.inf
    x = np.asarray([[0.5, -inf, 0.1], [0.5, -inf, 0.1], [0.0, -709.0, -1.0], [0.0, -709.0, -1.0]], np.float32)
    act = np.asarray([0, 1, 2, 1])
    gl = np.asarray([1.5, -2.25, 0.75, 3.0], np.float32)
    gH = np.asarray([-0.5, 4.0, 2.0, -1.0], np.float32)
    lp, en = pe.categorical(x, act)
    assert np.isneginf(lp[1]) and lp[3] < -708 and np.isfinite(lp[3]) and np.all(np.isfinite(en))       # a masked chosen action follows the arithmetic
    p = pe.categorical_parts(x, act)
    q = p["e"] / p["S"][:, None]
    assert np.all(q[:, 1] == 0.0)
    g_en = pe.categorical_backward(x, act, grad_entropy=gH)
    assert np.all(g_en[:, 1] == 0.0) and np.all(g_en[:, [0, 2]] != 0.0)                 # no entropy term on a masked logit
    g_lp = pe.categorical_backward(x, act, grad_log_prob=gl)
    g = pe.categorical_backward(x, act, gl, gH)
    for i in range(4):
        for a in range(3):
            assert g_lp[i, a] == gl[i] * ((1.0 if a == act[i] else 0.0) - q[i, a])
        if act[i] == 1:                                                                  # masked and chosen: gl alone
            assert g[i, 1] == gl[i] == g_lp[i, 1] and pe.to_f32(g[i:i + 1, 1])[0] == gl[i]
        else:                                                                            # masked, not chosen: -q gl = 0
            assert g[i, 1] == 0.0
    assert np.all(np.isfinite(g))


def test_degenerate_and_out_of_range_rows_are_nan():
    inf, nan = np.inf, np.nan
    x = np.asarray([[nan, 0, 0], [0, inf, 0], [-inf, -inf, -inf], [0, 1, 2], [0, 1, 2], [0, 1, 2], [0, 1, 2]], np.float32)
    act = np.asarray([0, 0, 0, 3, -1, 2 ** 40, 2])
    lp, en = pe.categorical(x, act)
    g = pe.categorical_backward(x, act, np.ones(7, np.float32), np.ones(7, np.float32))
    bad = np.arange(7) < 6
    assert np.array_equal(np.isnan(lp), bad) and np.array_equal(np.isnan(en), bad) and np.array_equal(np.isnan(g).all(1), bad)
    assert np.all(np.isfinite(g[6]))
    assert np.all(pe.bits(pe.to_f32(lp))[bad] == pe.CANONICAL_NAN) and np.all(pe.bits(pe.to_f32(g))[bad] == pe.CANONICAL_NAN)
    assert np.all(np.isfinite(pe.categorical_parts(x, act)["S"]))                        # the rows' own arithmetic stays finite
    mean = np.asarray([[nan, 0], [0, inf], [0, 0], [0, 0], [0, 0], [1, 2], [1, 2], [1, 2]], np.float32)
    ls = np.asarray([[0, 0], [0, 0], [nan, 0], [0, 80.0001], [-inf, 0], [80, -80], [0, 0], [0, 0]], np.float32)
    a = np.asarray([[0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [1, 2], [inf, 2], [nan, 2]], np.float32)
    lp, en = pe.gaussian(mean, ls, a)
    gm, gs = pe.gaussian_backward(mean, ls, a, np.ones(8, np.float32), np.ones(8, np.float32))
    bad = np.arange(8) < 5
    assert np.array_equal(np.isnan(en), bad) and np.array_equal(np.isnan(gm).all(1), bad) and np.array_equal(np.isnan(gs).all(1), bad)
    assert np.isfinite(lp[5]) and np.isneginf(lp[6]) and np.isnan(lp[7]) and np.all(np.isnan(lp[:5]))      # a non-finite stored action follows the arithmetic
    assert np.isposinf(gm[6, 0]) and np.isposinf(gs[6, 0]) and np.isfinite(gm[6, 1]) and np.isnan(gm[7, 0]) and np.isfinite(gs[7, 1])


def test_an_absent_term_is_left_out_not_multiplied_by_zero():
    rng = np.random.default_rng(5)
    M, A = 400, 6
    x = (rng.standard_normal((M, A)) * 3).astype(np.float32)
    x[::7, 2] = -np.inf
    act = rng.integers(0, A, M)
    act[::14] = 2                                                          # some masked logits are the chosen ones
    g = rng.standard_normal(M).astype(np.float32)
    g[::5] = 0.0
    zero = np.zeros(M, np.float32)
    for kw_lone, kw_zero in ((dict(grad_log_prob=g), dict(grad_log_prob=g, grad_entropy=zero)),
                             (dict(grad_entropy=g), dict(grad_log_prob=zero, grad_entropy=g))):
        lone, both = pe.categorical_backward(x, act, **kw_lone), pe.categorical_backward(x, act, **kw_zero)
        differ = _u64(lone) != _u64(both)
        # x + (+-0) == x for every x but a zero of the other sign: the sum may only differ from the lone term where that term is a zero
        assert np.all(lone[differ] == 0.0) and np.all(both[differ] == 0.0) and np.array_equal(lone, both)
        assert differ.any()                                                # and there it does: -0 + +0 = +0
    mean = rng.standard_normal((M, 3)).astype(np.float32)
    ls = rng.uniform(-2, 1, (M, 3)).astype(np.float32)
    a = (mean + np.exp(ls) * rng.standard_normal((M, 3))).astype(np.float32)
    a[::9] = mean[::9]                                                     # zq = 0: zero gradients of the mean
    lone_m, lone_s = pe.gaussian_backward(mean, ls, a, grad_log_prob=g)
    both_m, both_s = pe.gaussian_backward(mean, ls, a, grad_log_prob=g, grad_entropy=zero)
    assert np.array_equal(_u64(lone_m), _u64(both_m))
    differ = _u64(lone_s) != _u64(both_s)
    assert np.all(lone_s[differ] == 0.0) and np.array_equal(lone_s, both_s)
    lone_m, lone_s = pe.gaussian_backward(mean, ls, a, grad_entropy=g)
    both_m, both_s = pe.gaussian_backward(mean, ls, a, grad_log_prob=zero, grad_entropy=g)
    assert np.all(_u64(lone_m) == 0) and np.all(both_m == 0.0) and np.array_equal(lone_s, both_s)      # +0.0 exactly; 0 * x may be -0
    # a zero factor is not nothing: with a stored action of +Inf, 0 * Inf is NaN — an absent term is not there
    a[0, 0] = np.inf
    lone_m, lone_s = pe.gaussian_backward(mean[:1], ls[:1], a[:1], grad_entropy=g[1:2])
    both_m, both_s = pe.gaussian_backward(mean[:1], ls[:1], a[:1], grad_log_prob=zero[:1], grad_entropy=g[1:2])
    assert lone_m[0, 0] == 0.0 and lone_s[0, 0] == g[1] and np.isnan(both_m[0, 0]) and np.isnan(both_s[0, 0])


# ---- the header, its bindings, the constants -------------------------------------------------------------------------------------------------
def _prototypes():
    text = open(os.path.join(ROOT, "include", "mxv_policy_eval.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(2): (m.group(1).strip(), " ".join(m.group(3).split()))
            for m in re.finditer(r"\n\s*((?:const\s+)?[A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(mxv_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_is_optional_self_contained_and_bound_outside_the_other_exports():
    from gym_amd import _native, policy, policy_eval
    from gym_amd.returns import GAE_EXPORTS

    protos = _prototypes()
    assert sorted(protos) == sorted(policy_eval.EVAL_EXPORTS) and len(protos) == 5
    assert not set(protos) & (set(_native.EXPORTS) | set(GAE_EXPORTS) | set(policy.POLICY_EXPORTS))
    assert "mxv_policy_eval.h" not in open(os.path.join(ROOT, "include", "mxv.h")).read()
    assert "mxv_policy_eval.h" not in open(os.path.join(ROOT, "include", "mxv_policy.h")).read()
    lib = ctypes.CDLL(_native.LIB_PATH)
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, (ret, args) in protos.items():
        assert hasattr(lib, name) and name in notes, name
        f = getattr(policy_eval.lib, name)
        n_args = 0 if args in ("", "void") else len(args.split(","))
        assert len(f.argtypes) == n_args, (name, args)
        if n_args:
            for a, t in zip(args.split(","), f.argtypes):
                want = ctypes.c_void_p if "*" in a else {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[a.split()[0]]
                assert t is want, (name, a, t)
        assert f.restype is (ctypes.c_char_p if "char" in ret else ctypes.c_int), name
    assert policy_eval.lib.mxv_policy_eval_last_error() is not None
    if shutil.which("gcc"):
        for comp, lang, std in (("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++11")):
            p = subprocess.run([comp, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", lang, "-"],
                               input='#include "mxv_policy_eval.h"\nint main(void) { return 0; }\n', capture_output=True, text=True)
            assert p.returncode == 0, (comp, p.stderr[-1500:])


def test_the_kernel_source_carries_the_generated_constants():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gaussian_coefficients
        import policy_coefficients
    finally:
        sys.path.pop(0)
    block, _ = ph.rule_block("mxv_policy_eval.hip")
    assert block == gaussian_coefficients.block() and block.startswith(policy_coefficients.block() + "\n")
    for script in ("build.sh", "build_asan.sh"):
        assert "mxv_policy_eval.hip" in open(os.path.join(ROOT, "gym_amd", "csrc", script)).read(), script


def test_c_entry_points_refuse_bad_arguments_before_touching_the_device():
    from gym_amd import _native, policy_eval

    A = 1 << 20      # distinct, aligned, never dereferenced
    lib = policy_eval.lib
    cat, cat_b, gau, gau_b = (lib.mxv_policy_eval_categorical, lib.mxv_policy_eval_categorical_backward, lib.mxv_policy_eval_gaussian,
                              lib.mxv_policy_eval_gaussian_backward)
    for f, args, word in ((cat, (None, 16, 3, None, 3, 2 * A, 1, 3 * A, 4 * A), "logits pointer is NULL"),
                          (cat, (None, 16, 65, A, 65, 2 * A, 1, 3 * A, 4 * A), "A ="),
                          (cat_b, (None, 16, 3, A, 3, 2 * A, 0, None, None, 5 * A, 3), "both NULL"),
                          (cat_b, (None, 16, 3, A, 3, 2 * A, 0, 3 * A, None, A + 8, 3), "grad_logits overlaps the logits"),
                          (gau, (None, 16, 5, A, 5, 2 * A, 5, 3 * A, 5, 4 * A, 5 * A), "D ="),
                          (gau_b, (None, 16, 2, A, 2, 2 * A, 0, 3 * A, 2, 4 * A, None, 6 * A, 1, 7 * A, 2), "grad_mean_ld =")):
        rc = f(*args)
        msg = lib.mxv_policy_eval_last_error().decode()
        assert rc == _native.ERR_INVALID_ARG and word in msg and msg.startswith(f.__name__ + ":"), (rc, msg, word)


# ---- the Python front end ------------------------------------------------------------------------------------------------------------------
def test_the_front_end_validates_without_a_device():
    code = ("import sys; import gym_amd.policy_eval as p; assert 'torch' not in sys.modules; import gym_amd; "
            "assert gym_amd.evaluate_categorical is p.evaluate_categorical and gym_amd.evaluate_gaussian is p.evaluate_gaussian; "
            "assert 'torch' not in sys.modules; import gym_amd.policy as q; "
            "assert callable(q.PolicySampler.evaluate) and callable(q.GaussianSampler.evaluate) and len(q.POLICY_EXPORTS) == 4; "
            "assert 'torch' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
    import torch

    from gym_amd import policy_eval

    x, a = torch.zeros((4, 3)), torch.zeros(4, dtype=torch.int64)
    i64 = torch.int64
    for kw, what in ((dict(logits=x.double()), "float32"), (dict(logits=x[0]), "shape"), (dict(logits=torch.zeros((4, 65))), "shape"),
                     (dict(logits=torch.zeros((0, 3)), actions=torch.zeros(0, dtype=i64)), "shape"), (dict(logits=[[0.0]]), "torch tensor"),
                     (dict(logits=torch.zeros((3, 4)).t()), "contiguous"),
                     (dict(logits=torch.zeros((3, 2, 5)).transpose(0, 1)[:, :, :3], actions=torch.zeros((2, 3), dtype=i64)), r"view\(-1, 3\)"),
                     (dict(actions=a.float()), "int64"), (dict(actions=torch.zeros(5, dtype=i64)), "shape"), (dict(actions=torch.zeros((4, 1), dtype=i64)), "shape"),
                     (dict(actions=torch.zeros(8, dtype=i64)[::2]), "contiguous"), (dict(actions=[0, 0, 0, 0]), "torch tensor"),
                     (dict(out=(torch.zeros(4),)), "2 entries"), (dict(out=(torch.zeros(5), None)), "shape"),
                     (dict(out=(None, torch.zeros(4, dtype=torch.float64))), "float32"), (dict(out=(torch.zeros(8)[::2], None)), "contiguous"),
                     (dict(logits=x.clone().requires_grad_(), out=(torch.zeros(4), None)), "requires grad"),
                     (dict(logits=torch.zeros((2, 2, 3)), actions=torch.zeros((2, 2), dtype=torch.int32)), "device tensor"),
                     (dict(), "device tensor")):
        args = dict(logits=x, actions=a)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            policy_eval.evaluate_categorical(args.pop("logits"), args.pop("actions"), **args)
    m, s, act = torch.zeros((4, 3)), torch.zeros((4, 3)), torch.zeros((4, 3))
    for kw, what in ((dict(mean=m.double()), "float32"), (dict(mean=m[0]), "shape"), (dict(mean=torch.zeros((4, 5))), "shape"),
                     (dict(mean=torch.zeros((3, 4)).t()), "contiguous"), (dict(log_std=s.double()), "float32"), (dict(log_std=torch.zeros((4, 2))), "log_std"),
                     (dict(log_std=torch.zeros(4)), "log_std"), (dict(log_std=torch.zeros(6)[::2]), "contiguous"), (dict(log_std=[0.0, 0.0, 0.0]), "torch tensor"),
                     (dict(actions=act.double()), "float32"), (dict(actions=torch.zeros((4, 2))), "actions"), (dict(actions=torch.zeros(4)), "actions"),
                     (dict(actions=act.clone().requires_grad_()), "actions must not require grad"),
                     (dict(mean=torch.zeros((3, 2, 5)).transpose(0, 1)[:, :, :3], log_std=torch.zeros(3), actions=torch.zeros((2, 3, 3))), r"view\(-1, 3\)"),
                     (dict(out=(torch.zeros(4),)), "2 entries"), (dict(out=(torch.zeros(4), torch.zeros(3))), "shape"),
                     (dict(log_std=torch.zeros(3, requires_grad=True), out=(torch.zeros(4), None)), "requires grad"),
                     (dict(mean=torch.zeros((2, 2, 3)), log_std=torch.zeros(3), actions=torch.zeros((2, 2, 3))), "device tensor"),
                     (dict(), "device tensor")):
        args = dict(mean=m, log_std=s, actions=act)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            policy_eval.evaluate_gaussian(args.pop("mean"), args.pop("log_std"), args.pop("actions"), **args)
