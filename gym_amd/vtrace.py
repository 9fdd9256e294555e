"""V-trace value targets and policy-gradient advantages over [K, N] trajectory tensors, on the device (include/mxv_vtrace.h,
DESIGN.md §16): what gym_amd.returns.gae is for an on-policy batch, for one whose behaviour log-probabilities are stale — rollouts that
run one update behind the weights, or the later epochs of a multi-epoch update.

`log_prob` is the learner's log pi of the stored actions (evaluate_categorical / evaluate_gaussian), `old_log_prob` what the sampler
recorded; the rest is gae()'s.  One kernel launch on the caller's current stream, no synchronisation, no allocation beyond the outputs
(none with `out=`): recordable into a torch.cuda.graph.  The header is optional (mxv.h does not include it), so its symbols are bound
here, over the same library as gym_amd._native, and are not part of _native.EXPORTS.  Importing this module does not import torch.
"""
from __future__ import annotations

import ctypes as C
import sys
import types

from . import _native
from .returns import _matrix, _ptr, _row_stride, _scalar, _vector

VTRACE_EXPORTS = ("mxv_vtrace", "mxv_vtrace_last_error", "mxv_vtrace_last_launch")
RING_DEPTH = 4      # rows the kernel keeps in flight ahead of the one it consumes (kRing, gym_amd/csrc/mxv_vtrace.hip)
VECTOR_MIN_ENVS = 1 << 21   # from here on (and with 16-byte alignment throughout) a lane owns four envs (kVecMinN)

lib = _native.lib
lib.mxv_vtrace.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p,
                           C.c_void_p, C.c_int64]
lib.mxv_vtrace.restype = C.c_int
lib.mxv_vtrace_last_error.argtypes = []
lib.mxv_vtrace_last_error.restype = C.c_char_p
lib.mxv_vtrace_last_launch.argtypes = [C.c_void_p, C.c_void_p]
lib.mxv_vtrace_last_launch.restype = C.c_int


def _check(rc: int):
    if rc == _native.OK:
        return
    msg = lib.mxv_vtrace_last_error().decode()
    if rc == _native.ERR_INVALID_ARG:
        raise ValueError(msg)
    raise _native.MxvError(rc, msg)


def last_launch():
    """(envs per lane, workgroups) of this thread's last launch by vtrace(): 4 envs per lane is the 16-byte path."""
    v, g = C.c_int32(), C.c_uint32()
    _check(lib.mxv_vtrace_last_launch(C.byref(v), C.byref(g)))
    return v.value, g.value


def _level(name, v):
    f = _scalar(name, v)
    if not f > 0.0:
        raise ValueError(f"{name} must be greater than 0, got {v!r}")
    return f


def vtrace(log_prob, old_log_prob, reward, terminated, truncated, values, last_value=None, *, gamma: float = 0.99, lam: float = 1.0,
           rho_bar: float = 1.0, c_bar: float = 1.0, pg_rho_bar=None, final_values=None, out=None):
    """V-trace over a [K, N] chunk -> (vs, pg_advantages), both float32 [K, N] and without a graph: they are targets.

    log_prob, old_log_prob float32 [K, N]: log pi(a_t) under the policy being updated and under the one that drew the actions (an input
    that requires grad is read detached); reward, terminated, truncated, values, last_value, final_values: as gym_amd.gae.  The
    importance weight w = exp(log_prob - old_log_prob) (the difference clamped to +-80) is truncated at rho_bar for the TD errors, at
    c_bar (times lam) for the trace and at pg_rho_bar (None: rho_bar) for the advantages:
        vs_t = V_t + sum_k gamma^k (prod_{i<k} lam min(c_bar, w_i)) min(rho_bar, w_k) (r_k + gamma V_{k+1} - V_k)
        pg_t = min(pg_rho_bar, w_t) (r_t + gamma vs_{t+1} - V_t)
    cut where terminated | truncated is set (bootstrapping with final_values where only truncated is).  out: a pair of float32 [K, N]
    tensors to write into.  Rows may be strided views (one row stride for all inputs, one for the outputs), the last dimension is
    contiguous; an output may not share memory with an input or with the other output (ValueError), column blocks of one wide buffer
    are fine.  Float64 arithmetic, one rounding per operation, bit-equal to tests/vtrace_host.py; with log_prob bit-equal to
    old_log_prob and rho_bar, c_bar >= 1, vs has the bits of gae()'s returns.  gamma, lam: finite; the three clip levels: finite and
    > 0.  Runs on the current stream, no synchronisation."""
    import torch as t

    gamma, lam = _scalar("gamma", gamma), _scalar("lam", lam)
    rho_bar, c_bar = _level("rho_bar", rho_bar), _level("c_bar", c_bar)
    pg_rho_bar = rho_bar if pg_rho_bar is None else _level("pg_rho_bar", pg_rho_bar)
    reward = _matrix(t, reward, "reward", (t.float32, t.float64))
    shape = reward.shape
    ins = [("log_prob", _matrix(t, log_prob, "log_prob", (t.float32,), shape)),
           ("old_log_prob", _matrix(t, old_log_prob, "old_log_prob", (t.float32,), shape)), ("reward", reward),
           ("terminated", _matrix(t, terminated, "terminated", (t.uint8,), shape)),
           ("truncated", _matrix(t, truncated, "truncated", (t.uint8,), shape)), ("values", _matrix(t, values, "values", (t.float32,), shape))]
    if final_values is not None:
        ins.append(("final_values", _matrix(t, final_values, "final_values", (t.float32,), shape)))
    last_value = _vector(t, last_value, "last_value", shape[1])
    ld = _row_stride(ins, "inputs")
    names = ("vs", "pg_advantages")
    outs = None
    if out is not None:
        given = (out,) if isinstance(out, t.Tensor) else tuple(out)
        if len(given) != 2:
            raise ValueError(f"out must hold 2 tensors ({', '.join(names)}), got {len(given)}")
        outs = [(f"out ({name})", _matrix(t, x, f"out ({name})", (t.float32,), shape)) for name, x in zip(names, given)]
    dev = reward.device
    for name, x in ins + [("last_value", last_value)] + (outs or []):
        if x is None:
            continue
        if not x.is_cuda:
            raise ValueError(f"{name} must be a device tensor, got one on {x.device} (gym_amd has no CPU fallback)")
        if x.device != dev:
            raise ValueError(f"{name} is on {x.device}, reward on {dev}: all tensors must be on one device")
    if outs is None:
        outs = [(name, t.empty(tuple(shape), dtype=t.float32, device=dev)) for name in names]
    for name, x in outs:
        if x.requires_grad:
            raise ValueError(f"{name} requires grad: the targets carry no graph and are written in place")
    ld_out = _row_stride(outs, "outputs")
    i = {k: x.detach() for k, x in ins}     # the kernel reads the data; nothing is recorded for autograd
    vs, pg = outs[0][1], outs[1][1]
    K, N = shape
    with t.cuda.device(dev):
        _check(lib.mxv_vtrace(t.cuda.current_stream(dev).cuda_stream, K, N, i["log_prob"].data_ptr(), i["old_log_prob"].data_ptr(),
                              i["reward"].data_ptr(), int(reward.dtype == t.float64), ld, i["terminated"].data_ptr(), i["truncated"].data_ptr(),
                              i["values"].data_ptr(), _ptr(None if last_value is None else last_value.detach()), _ptr(i.get("final_values")),
                              gamma, lam, rho_bar, c_bar, pg_rho_bar, vs.data_ptr(), pg.data_ptr(), ld_out))
    return vs, pg


class _Module(types.ModuleType):
    """gym_amd.vtrace names this module and, as the public function, vtrace() in it — importing a sub-module binds it as the package's
    attribute of that name — so calling the module calls the function."""

    def __call__(self, *args, **kw):
        return vtrace(*args, **kw)


sys.modules[__name__].__class__ = _Module
