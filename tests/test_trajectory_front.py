"""The front ends of GAE, returns-to-go and V-trace — gym_amd.gae, gym_amd.discounted_returns, gym_amd.vtrace and the C entry points
under them — pinned word for word (no GPU: CPU tensors and invented addresses, as in tests/test_gae_host.py and
tests/test_vtrace_host.py, whose malformed calls these are, with some more).

tests/golden/trajectory_front.json holds the full message of every case of CASES; tests/golden/make_trajectory_front.py recorded it
from the commit before the two families were folded onto gym_amd/_trajectory_args.py and gym_amd/csrc/mxv_trajectory.hpp.  A call with
two faults must report the one that the unfolded code reported: TWO_FAULTS names, for each such call, the one-fault case of CASES whose
message it must repeat."""
import json
import os

import numpy as np
import pytest
import torch

import test_gae_host as G
import test_vtrace_host as V
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "trajectory_front.json")
K, N = 4, 6
A = G.A
assert V.A == A


def _params(test):
    """The argument list of a test's (one) parametrize mark."""
    (mark,) = [m for m in test.pytestmark if m.name == "parametrize"]
    return mark.args[1]


# ---- the Python calls: the changes of the two files' test_python_arguments_are_checked_before_any_device_work, built as they build them ----
MAKE = {"f16": lambda: torch.zeros(K, N, dtype=torch.float16), "f32": lambda: torch.zeros(K, N), "f64": lambda: torch.zeros(K, N, dtype=torch.float64),
        "i32": lambda: torch.zeros(K, N, dtype=torch.int32), "3d": lambda: torch.zeros(K, N, 1), "shape": lambda: torch.zeros(K, N + 1),
        "colstride": lambda: torch.zeros(K, 2 * N)[:, ::2], "rowstride": lambda: torch.zeros(K, N + 3)[:, :N], "numpy": lambda: np.zeros((K, N), np.float32)}
SCALARS = ("gamma", "lam", "rho_bar", "c_bar", "pg_rho_bar")
OUTS = {"gae": {"count": lambda: (torch.zeros(K, N),), "f64": lambda: (torch.zeros(K, N), torch.zeros(K, N, dtype=torch.float64)),
                "bare": lambda: torch.zeros(K, N)},
        "discounted_returns": {"count": lambda: (torch.zeros(K, N), torch.zeros(K, N)), "f64": lambda: torch.zeros(K, N, dtype=torch.float64)},
        "vtrace": {"count": lambda: (torch.zeros(K, N),) * 3, "one": lambda: torch.zeros(K, N),
                   "f64": lambda: (torch.zeros(K, N), torch.zeros(K, N, dtype=torch.float64))}}


def _python_call(fn, change):
    import gym_amd

    kw = dict(reward=torch.zeros(K, N), terminated=torch.zeros(K, N, dtype=torch.uint8), truncated=torch.zeros(K, N, dtype=torch.bool))
    if fn != "discounted_returns":
        kw["values"] = torch.zeros(K, N)
    if fn == "vtrace":
        kw.update(log_prob=torch.zeros(K, N), old_log_prob=torch.zeros(K, N))
    for k, v in change.items():
        if k in SCALARS:
            kw[k] = v
        elif k == "last_value":
            kw[k] = torch.zeros(N + 1) if v == "shape" else torch.zeros(N, dtype=torch.float64)
        elif k == "out":
            kw[k] = OUTS[fn][v]()
        else:
            kw[k] = MAKE[v]()
    with pytest.raises(ValueError) as e:
        getattr(gym_amd, fn)(**kw)
    return f"ValueError: {e.value}"


def _c(call, over):
    rc, msg = call(**over)
    return f"{rc}: {msg}"


def _last_launch_null(module_name):
    import importlib

    m = importlib.import_module("gym_amd." + module_name)
    family = {"returns": "gae", "vtrace": "vtrace"}[module_name]
    rc = getattr(m.lib, f"mxv_{family}_last_launch")(None, None)
    return f"{rc}: {getattr(m.lib, f'mxv_{family}_last_error')().decode()}"


def _key(name, d):
    return f"{name}({', '.join(f'{k}={v!r}' for k, v in d.items())})"


def _cases():
    """id -> a function that makes the malformed call and returns its message"""
    cases = {}

    def add(name, d, f):
        key = _key(name, d)
        assert key not in cases, key
        cases[key] = f

    gae_changes = [c for c, _ in _params(G.test_python_arguments_are_checked_before_any_device_work)]
    for change in gae_changes + [dict(out="bare")]:          # gae iterates a bare tensor row by row: it "holds" K tensors
        add("gae", change, lambda c=change: _python_call("gae", c))
    for change in gae_changes:
        if not set(change) & {"values", "lam"}:              # what the file repeats for discounted_returns
            add("discounted_returns", change, lambda c=change: _python_call("discounted_returns", c))
    for change, _ in _params(V.test_python_arguments_are_checked_before_any_device_work):
        add("vtrace", change, lambda c=change: _python_call("vtrace", c))

    gae_only = [o for o, _ in _params(G.test_mxv_gae_refuses_bad_arguments_before_touching_the_device)]
    both = [o for o, _ in G.BAD_BOTH]
    assert gae_only[:len(both)] == both and len(gae_only) == len(both) + 6
    for over in gae_only:
        add("mxv_gae", over, lambda o=over: _c(G._c_gae, o))
    for over in both + [o for o, _ in _params(G.test_interleaved_ranges_that_share_bytes_or_cannot_be_told_apart_are_refused)]:
        add("mxv_discounted_returns", over, lambda o=over: _c(G._c_ret, o))
    for over, _ in _params(V.test_mxv_vtrace_refuses_bad_arguments_before_touching_the_device):
        add("mxv_vtrace", over, lambda o=over: _c(V._c_call, o))
    add("mxv_gae_last_launch", dict(envs_per_lane=None, grid=None), lambda: _last_launch_null("returns"))
    add("mxv_vtrace_last_launch", dict(envs_per_lane=None, grid=None), lambda: _last_launch_null("vtrace"))
    return cases


CASES = _cases()


def message_of(key):
    return CASES[key]()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_covers_every_function_and_the_golden_file_every_case(golden):
    assert sorted(golden["messages"]) == sorted(CASES)
    for name, least in (("gae", 19), ("discounted_returns", 13), ("vtrace", 26), ("mxv_gae", 26), ("mxv_discounted_returns", 23), ("mxv_vtrace", 35),
                        ("mxv_gae_last_launch", 1), ("mxv_vtrace_last_launch", 1)):
        assert sum(key.startswith(name + "(") for key in CASES) >= least, name


@pytest.mark.parametrize("key", sorted(CASES))
def test_a_malformed_call_reports_its_message_word_for_word(golden, key):
    assert message_of(key) == golden["messages"][key]


def test_the_three_out_traps_read_as_they_did(golden):
    """vtrace counts "2 tensors" and takes a bare tensor as one output; gae counts "tensor(s)" and iterates a bare tensor, so it finds K."""
    m = golden["messages"]
    assert m["vtrace(out='count')"] == "ValueError: out must hold 2 tensors (vs, pg_advantages), got 3"
    assert m["vtrace(out='one')"] == "ValueError: out must hold 2 tensors (vs, pg_advantages), got 1"
    assert m["gae(out='bare')"] == f"ValueError: out must hold 2 tensor(s) (advantages, returns), got {K}"
    assert m["gae(out='count')"] == "ValueError: out must hold 2 tensor(s) (advantages, returns), got 1"
    assert m["discounted_returns(out='count')"] == "ValueError: out must hold 1 tensor(s) (returns), got 2"


nan, inf = float("nan"), float("inf")
# (the call with two faults, the one-fault case of CASES whose message it must give): the fault that is checked first
TWO_FAULTS = [
    # gae checks its scalars before any tensor
    (lambda: _python_call("gae", dict(reward="f16", gamma=nan)), _key("gae", dict(gamma=nan))),
    # the inputs in the order of the call: terminated before values
    (lambda: _python_call("gae", dict(terminated="f32", values="f64")), _key("gae", dict(terminated="f32"))),
    # every dtype and shape before the row strides are compared
    (lambda: _python_call("gae", dict(values="rowstride", final_values="i32")), _key("gae", dict(final_values="i32"))),
    # last_value before out=
    (lambda: _python_call("gae", dict(out="count", last_value="shape")), _key("gae", dict(last_value="shape"))),
    (lambda: _python_call("discounted_returns", dict(reward="numpy", gamma=nan)), _key("discounted_returns", dict(gamma=nan))),
    (lambda: _python_call("discounted_returns", dict(truncated="shape", out="f64")), _key("discounted_returns", dict(truncated="shape"))),
    # out= of the wrong length and a last_value of the wrong dtype
    (lambda: _python_call("discounted_returns", dict(out="count", last_value="f64")), _key("discounted_returns", dict(last_value="f64"))),
    # vtrace: the scalars, then reward — which gives the shape —, then log_prob, old_log_prob and the rest in the order of the call
    (lambda: _python_call("vtrace", dict(reward="f16", rho_bar=0.0)), _key("vtrace", dict(rho_bar=0.0))),
    (lambda: _python_call("vtrace", dict(c_bar=nan, gamma=nan)), _key("vtrace", dict(gamma=nan))),
    (lambda: _python_call("vtrace", dict(log_prob="f64", reward="3d")), _key("vtrace", dict(reward="3d"))),
    (lambda: _python_call("vtrace", dict(old_log_prob="shape", log_prob="f64")), _key("vtrace", dict(log_prob="f64"))),
    (lambda: _python_call("vtrace", dict(out="one", final_values="shape")), _key("vtrace", dict(final_values="shape"))),
    # C: misaligned and overlapping — every alignment before any overlap
    (lambda: _c(G._c_gae, dict(reward=A + 2, ret=1 * A)), _key("mxv_gae", dict(reward=A + 2))),
    # C: the outputs' alignment before the inputs' overlap
    (lambda: _c(G._c_gae, dict(ret=8 * A + 1, adv=4 * A + 64)), _key("mxv_gae", dict(ret=8 * A + 1))),
    # C: K before gamma
    (lambda: _c(G._c_ret, dict(K=0, gamma=nan)), _key("mxv_discounted_returns", dict(K=0))),
    # C: NULL before K
    (lambda: _c(V._c_call, dict(lp=None, K=0)), _key("mxv_vtrace", dict(lp=None))),
    # C: the clip levels before the alignment
    (lambda: _c(V._c_call, dict(rho_bar=0.0, pg=8 * A + 1)), _key("mxv_vtrace", dict(rho_bar=0.0))),
    # C: an output against an input before the outputs against each other
    (lambda: _c(V._c_call, dict(vs=9 * A, pg=9 * A + 4)), _key("mxv_vtrace", dict(vs=9 * A))),
]


@pytest.mark.parametrize("index", range(len(TWO_FAULTS)))
def test_a_call_with_two_faults_reports_the_one_that_is_checked_first(golden, index):
    call, key = TWO_FAULTS[index]
    assert call() == golden["messages"][key]


def test_there_are_two_fault_calls_for_all_three_functions():
    assert len(TWO_FAULTS) >= 10
    for name in ("gae(", "discounted_returns(", "vtrace(", "mxv_gae(", "mxv_discounted_returns(", "mxv_vtrace("):
        assert any(key.startswith(name) for _, key in TWO_FAULTS), name


def test_the_private_helpers_stay_importable_from_returns_and_torch_stays_unimported():
    import subprocess
    import sys

    code = ("import sys; import gym_amd._trajectory_args as a, gym_amd.returns as r, gym_amd.vtrace as v, gym_amd.ppo\n"
            "assert 'torch' not in sys.modules\n"
            "assert r._scalar is a._scalar and r.RING_DEPTH == v.RING_DEPTH == a.RING_DEPTH == 4\n"
            "assert r.VECTOR_MIN_ENVS == v.VECTOR_MIN_ENVS == a.VECTOR_MIN_ENVS == 1 << 21\n"
            "assert r.last_launch is not v.last_launch and 'gae()' in r.last_launch.__doc__ and 'vtrace()' in v.last_launch.__doc__\n")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT)).returncode == 0
