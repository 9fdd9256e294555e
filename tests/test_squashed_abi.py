"""include/mxv_squashed.h as a C header and its ctypes mirror in gym_amd/squashed.py: optional (mxv.h does not include it),
self-contained as C and as C++, bound outside every other export list, each prototype of the same classes as the argtypes declared for
it, its own error slot, the rule stated in full, and every argument error of the header through ctypes.  No device needed."""
import ctypes
import math
import os
import shutil
import subprocess

import test_abi
from conftest import ROOT
from test_abi import _ctypes_kind, _declared_symbols, _kind

HEADER = "mxv_squashed.h"


def _prototypes():
    """{symbol: (return type, [argument type strings])} of the header, parsed the way test_abi._header_prototypes parses mxv.h."""
    saved = test_abi.HEADERS
    test_abi.HEADERS = (HEADER,)
    try:
        return test_abi._header_prototypes()
    finally:
        test_abi.HEADERS = saved


def test_header_is_optional_and_bound_outside_the_other_exports():
    from gym_amd import _native, c51, dqn, policy, policy_eval, ppo, prioritized, replay, squashed, vtrace
    from gym_amd.returns import GAE_EXPORTS

    declared = _declared_symbols((HEADER,))
    assert declared == sorted(squashed.SQUASHED_EXPORTS) and len(declared) == 3 and all(s.startswith("mxv_squashed_") for s in declared)
    others = (set(_native.EXPORTS) | set(GAE_EXPORTS) | set(policy.POLICY_EXPORTS) | set(policy_eval.EVAL_EXPORTS) | set(ppo.PPO_EXPORTS)
              | set(dqn.DQN_EXPORTS) | set(c51.C51_EXPORTS))
    for mod in (prioritized, replay, vtrace):
        for name in dir(mod):
            if name.endswith("_EXPORTS"):
                others |= set(getattr(mod, name))
    assert not set(declared) & others and len(others) > 45
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != HEADER:
            assert HEADER not in open(os.path.join(ROOT, "include", other)).read(), other
    lib = ctypes.CDLL(_native.LIB_PATH)
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in declared + ["rsample_squashed_gaussian", "SquashedGaussianSampler", "squashed_gaussian_sampler"]:
        assert name in notes, name
    for name in declared:
        assert hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    # the rule is stated in the header in full: every line of it that the twin mirrors
    for line in ("(t_hi & 0x0fffffff) | 11 << 28", "sigma = EXP(ls);  n = sigma * z;  u = mu + n;  v = |u|", "e  = E(-2 v)", "q  = 1 + e",
                 "th = v < 2^-27 ? v : (1 - e) / q", "t  = copysign(th, u)", "action_j = float32(bias_j + scale_j * t)",
                 "corr = 2 * ((LN2 - v) - LOG(q))", "lp  += ((-0.5 * (z * z) - ls) - kHalfLog2Pi) - (LOG(scale_j) + corr)", "log_prob = float32(lp)",
                 "s  = (4 * e) / (q * q)", "grad_mean_j    = float32((ga_j * scale_j) * s + glp * (2 * t))",
                 "grad_log_std_j = float32(((ga_j * scale_j) * s) * n + glp * ((2 * t) * n - 1))", "LN2 = kLn2Hi + kLn2Lo rounded once",
                 "NULL means 1 and 0", "[2^-33, 64]", "0x7FC00000", "bad_mean, bad_log_std"):
        assert line in text, line
    for other in ("mxv_dqn.h", "mxv_ppo.h", "mxv_prio.h", "mxv_replay.h", "mxv_vtrace.h", "mxv_policy.h", "mxv_policy_eval.h", "mxv_gae.h", "mxv_c51.h"):
        assert other not in text, other      # the other headers' own tests refuse their file names here
    # the shared rule text is used as it stands: the kernel file includes it and defines none of its names
    src = open(os.path.join(ROOT, "gym_amd", "csrc", "mxv_squashed.hip")).read()
    assert '#include "mxv_policy_rule.hpp"' in src
    for name in ("exp_rule", "e_of", "log_rule", "normal_pair"):
        assert name + "(" in src and f"double {name}(" not in src and f"void {name}(" not in src, name
    for script in ("build.sh", "build_asan.sh"):
        assert "mxv_squashed.hip" in open(os.path.join(ROOT, "gym_amd", "csrc", script)).read(), script


def test_ctypes_signatures_agree_with_the_header_prototypes():
    from gym_amd import squashed

    protos = _prototypes()
    assert sorted(protos) == sorted(squashed.SQUASHED_EXPORTS)
    for name, (ret, args) in sorted(protos.items()):
        f = getattr(squashed.lib, name)
        assert f.argtypes is not None and len(f.argtypes) == len(args), (name, args, f.argtypes)
        for i, (a, t) in enumerate(zip(args, f.argtypes)):
            assert _ctypes_kind(t) == _kind(a), (name, i, a, t)
        if "char" in ret:
            assert f.restype is ctypes.c_char_p, name
        else:
            assert f.restype in (ctypes.c_int, ctypes.c_int32), (name, ret)
    assert squashed.lib.mxv_squashed_last_error() is not None
    assert len(protos["mxv_squashed_sample"][1]) == 17 and len(protos["mxv_squashed_sample_backward"][1]) == 20
    for name in ("mxv_squashed_sample", "mxv_squashed_sample_backward"):      # the shared prefix: stream .. step_dev
        kinds = [_kind(a) for a in protos[name][1]]
        assert kinds[:13] == ["pointer", "i64", "i32", "pointer", "i64", "pointer", "i64", "pointer", "pointer", "u64", "u64", "u64", "pointer"], (name, kinds)


def test_header_compiles_on_its_own_as_c_and_as_cpp():
    import pytest

    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    for comp, lang, std in (("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++11")):
        p = subprocess.run([comp, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", lang, "-"],
                           input=f'#include "{HEADER}"\nint main(void) {{ return mxv_squashed_last_error() == 0; }}\n', capture_output=True, text=True)
        assert p.returncode == 0, (comp, p.stderr[-1500:])


def test_c_entry_points_refuse_bad_arguments_before_touching_the_device():
    from gym_amd import _native, squashed

    P = 1 << 24      # distinct, aligned, never dereferenced
    lib = squashed.lib
    F4 = ctypes.c_float * 4

    keep = []      # the host arrays stay alive across the calls

    def arr(*v):
        keep.append(F4(*v))
        return ctypes.cast(keep[-1], ctypes.c_void_p)

    # mean P, log_std 2P, step_dev 3P; forward: step_used 4P, actions 5P, log_prob 6P; backward: grad_actions 4P, grad_log_prob 5P,
    # grad_mean 6P, grad_log_std 7P
    base = dict(stream=None, N=16, D=3, mean=P, mean_ld=3, log_std=2 * P, log_std_ld=3, scale=arr(2, 1, 0.5, 1), bias=arr(0, -1, 3, 0), seed=1,
                env_offset=2, step=3, step_dev=3 * P)
    fwd_tail = dict(step_used=4 * P, actions=5 * P, actions_ld=3, log_prob=6 * P)
    bwd_tail = dict(ga=4 * P, ga_ld=3, glp=5 * P, gm=6 * P, gm_ld=3, gs=7 * P, gs_ld=3)
    nan, inf = math.nan, math.inf
    shared = ((dict(mean=None), "mean pointer is NULL"), (dict(log_std=None), "log_std pointer is NULL"), (dict(N=0), "N ="), (dict(N=-3), "N ="),
              (dict(D=0), "D ="), (dict(D=5), "D ="), (dict(mean_ld=2), "mean_ld ="), (dict(log_std_ld=2), "log_std_ld ="),
              (dict(log_std_ld=-1), "log_std_ld ="), (dict(N=1 << 40, mean_ld=4), "beyond 2^40 elements"),
              (dict(N=(1 << 40) // 3 + 1, log_std_ld=0), "beyond 2^40 elements"), (dict(log_std_ld=1 << 62), "beyond 2^40 elements"),
              (dict(scale=arr(0, 1, 1, 1)), "scale[0] ="), (dict(scale=arr(1, -2, 1, 1)), "scale[1] ="), (dict(scale=arr(1, 1, 64.5, 1)), "scale[2] ="),
              (dict(scale=arr(1, 2.0 ** -34, 1, 1)), "scale[1] ="), (dict(scale=arr(nan, 1, 1, 1)), "scale[0] ="), (dict(scale=arr(1, 1, inf, 1)), "scale[2] ="),
              (dict(bias=arr(0, inf, 0, 0)), "bias[1] ="), (dict(bias=arr(0, 0, -inf, 0)), "bias[2] ="), (dict(bias=arr(nan, 0, 0, 0)), "bias[0] ="),
              (dict(D=4, mean_ld=4, log_std_ld=4, actions_ld=4, ga_ld=4, gm_ld=4, gs_ld=4, scale=arr(1, 1, 1, 65)), "scale[3] ="),
              (dict(mean=P + 2), "mean pointer"), (dict(log_std=2 * P + 1), "log_std pointer"), (dict(step_dev=3 * P + 4), "step_dev pointer"),
              (dict(mean=(1 << 64) - 16), "address space"), (dict(log_std=(1 << 64) - 8, log_std_ld=0), "address space"),
              (dict(step_dev=(1 << 64) - 8), "address space"))
    forward = ((dict(actions=None), "actions pointer is NULL"), (dict(actions_ld=2), "actions_ld ="), (dict(actions_ld=1 << 50), "beyond 2^40 elements"),
               (dict(step_used=4 * P + 4), "step_used pointer"), (dict(actions=5 * P + 2), "actions pointer"), (dict(log_prob=6 * P + 1), "log_prob pointer"),
               (dict(actions=(1 << 64) - 16), "address space"), (dict(log_prob=(1 << 64) - 4), "address space"), (dict(step_used=(1 << 64) - 8), "address space"),
               (dict(actions=P + 188), "actions overlaps the mean"), (dict(log_prob=2 * P - 60), "log_prob overlaps the log_std"),
               (dict(step_used=P + 184), "step_used overlaps the mean"), (dict(actions=3 * P - 188), "actions overlaps step_dev"),
               (dict(log_prob=3 * P + 4), "log_prob overlaps step_dev"), (dict(step_used=3 * P), "step_used overlaps step_dev"),
               (dict(log_prob=5 * P + 188), "outputs actions and log_prob overlap"), (dict(step_used=5 * P + 184), "outputs actions and step_used overlap"),
               (dict(step_used=6 * P + 56), "outputs log_prob and step_used overlap"))
    backward = ((dict(gm=None, gs=None), "both NULL"), (dict(ga_ld=2), "grad_actions_ld ="), (dict(gm_ld=0), "grad_mean_ld ="), (dict(gs_ld=2), "grad_log_std_ld ="),
                (dict(gm_ld=1 << 50), "beyond 2^40 elements"), (dict(ga=4 * P + 2), "grad_actions pointer"), (dict(glp=5 * P + 1), "grad_log_prob pointer"),
                (dict(gm=6 * P + 2), "grad_mean pointer"), (dict(gs=7 * P + 3), "grad_log_std pointer"), (dict(ga=(1 << 64) - 16), "address space"),
                (dict(gs=(1 << 64) - 16), "address space"), (dict(gm=P + 188), "grad_mean overlaps the mean"),
                (dict(gs=2 * P - 188), "grad_log_std overlaps the log_std"), (dict(gm=3 * P - 188), "grad_mean overlaps step_dev"),
                (dict(gm=4 * P + 188), "grad_mean overlaps the grad_actions"), (dict(gs=5 * P + 60), "grad_log_std overlaps the grad_log_prob"),
                (dict(gs=6 * P + 188), "outputs grad_mean and grad_log_std overlap"))
    calls = 0
    for f, tail, own in ((lib.mxv_squashed_sample, fwd_tail, forward), (lib.mxv_squashed_sample_backward, bwd_tail, backward)):
        for edit, word in shared + own:
            args = dict(base, **tail)
            args.update({k: v for k, v in edit.items() if k in args})
            rc = f(*args.values())
            msg = lib.mxv_squashed_last_error().decode()
            assert rc == _native.ERR_INVALID_ARG and word in msg and msg.startswith(f.__name__ + ":"), (f.__name__, edit, rc, msg, word)
            calls += 1
    assert calls == 2 * len(shared) + len(forward) + len(backward)
    # the slot is this header's own
    from gym_amd import policy

    before = policy.lib.mxv_policy_last_error()
    assert lib.mxv_squashed_sample(*dict(base, N=0, **fwd_tail).values()) == _native.ERR_INVALID_ARG
    assert policy.lib.mxv_policy_last_error() == before and b"mxv_squashed_sample" not in before


def test_the_front_end_validates_without_a_device():
    import pytest
    import torch

    from gym_amd import squashed

    assert tuple(squashed._affine(1, -2.0, 2.0, None, None)[0]) == (2.0,) and tuple(squashed._affine(1, -2.0, 2.0, None, None)[1]) == (0.0,)
    sc, bi = squashed._affine(3, [-1, 0, 2], [1, 4, 3], None, None)
    assert tuple(sc) == (1.0, 2.0, 0.5) and tuple(bi) == (0.0, 2.0, 2.5)
    assert tuple(squashed._affine(2, None, None, None, None)[0]) == (1.0, 1.0)
    for kw, word in ((dict(low=-1, high=1, scale=1), "not both"), (dict(low=-1), "together"), (dict(low=1, high=1), r"scale\[0\]"),
                     (dict(low=2, high=1), r"scale\[0\]"), (dict(low=-100, high=100), r"scale\[0\]"), (dict(scale=[1, 2, 3]), "2 numbers"),
                     (dict(bias=float("inf")), r"bias\[0\]"), (dict(scale=float("nan")), r"scale\[0\]"), (dict(low="a", high=1), "numbers")):
        with pytest.raises(ValueError, match=word):
            squashed._affine(2, kw.get("low"), kw.get("high"), kw.get("scale"), kw.get("bias"))
    mean, ls = torch.zeros(4, 2), torch.zeros(2)
    with pytest.raises(ValueError, match="device tensor"):
        squashed.rsample_squashed_gaussian(mean, ls, seed=0, step=0)
    with pytest.raises(ValueError, match="not both"):
        squashed.rsample_squashed_gaussian(mean, ls, seed=0, step=0, low=-1, high=1, bias=0)
    with pytest.raises(ValueError, match="shape"):
        squashed.rsample_squashed_gaussian(torch.zeros(4, 5), torch.zeros(5), seed=0, step=0)
    with pytest.raises(ValueError, match="seed"):
        squashed.rsample_squashed_gaussian(mean, ls, seed=-1, step=0)
    import gym_amd

    assert gym_amd.rsample_squashed_gaussian is squashed.rsample_squashed_gaussian and gym_amd.SquashedGaussianSampler is squashed.SquashedGaussianSampler
