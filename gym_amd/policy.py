"""Policy actions sampled on the device, with their log-probabilities and the entropy of every row, in one launch
(include/mxv_policy.h): categorical draws from logits and, for the Box envs, diagonal-Gaussian draws from a mean and
a log_std (sample_gaussian / GaussianSampler; bit-equal to tests/gaussian_host.py).

The step between DeviceRollout.step(actions) and gym_amd.gae: `logits` is what the learner's policy head returns for the engine's
observations.  The draws follow the engine's Philox contract — the action of global env G at step t is a function of (seed, G, t) —
so they do not change under sharding, under how steps are grouped into launches or graphs, or across a checkpoint; the arithmetic is
float64 in a fixed order, bit-equal to tests/policy_host.py.

One kernel launch on the caller's current stream (two with a device step counter), no synchronisation, no allocation beyond the outputs
(none with `out=`): recordable into a torch.cuda.graph.  The header is optional (mxv.h does not include it), so its symbols are bound
here, over the same library as gym_amd._native, and are not part of _native.EXPORTS.  Importing this module does not import torch.
"""
from __future__ import annotations

import ctypes as C

from . import _native
from ._policy_args import MAX_ACTION_DIM, MAX_ACTIONS, STRAIGHT_LINE_ACTIONS      # noqa: F401  (the heads' limits: part of this module's surface)
from ._policy_args import _check as _raise
from ._policy_args import _index, _ld, _log_std, _one_device, _ptr, _rows, _Sampler, _step, _vector

POLICY_EXPORTS = ("mxv_policy_sample_categorical", "mxv_policy_sample_gaussian", "mxv_policy_last_error", "mxv_policy_last_launch")
lib = _native.lib
lib.mxv_policy_sample_categorical.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_uint64,
                                              C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
lib.mxv_policy_sample_categorical.restype = C.c_int
lib.mxv_policy_sample_gaussian.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64,
                                           C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
lib.mxv_policy_sample_gaussian.restype = C.c_int
lib.mxv_policy_last_error.argtypes = []
lib.mxv_policy_last_error.restype = C.c_char_p
lib.mxv_policy_last_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
lib.mxv_policy_last_launch.restype = C.c_int


def _check(rc: int):
    _raise(rc, lib.mxv_policy_last_error)


def last_launch():
    """(envs per lane, straight-line action count or 0 for the loop, workgroups) of this thread's last launch by sample_categorical()."""
    v, a, g = C.c_int32(), C.c_int32(), C.c_uint32()
    _check(lib.mxv_policy_last_launch(C.byref(v), C.byref(a), C.byref(g)))
    return v.value, a.value, g.value


def sample_categorical(logits, *, seed, step, env_offset=0, action_dtype=None, out=None):
    """Categorical draws from `logits` -> (actions [N], log_prob float32 [N], entropy float32 [N]).

    logits float32 [N, A] on the device, 1 <= A <= 64, last dimension contiguous, rows may be strided (a view into a wider buffer).
    seed, env_offset: integers; row i is global env env_offset + i.  step: a Python int, or an int64 device tensor with one element,
    which is read on the device and advanced by 1 behind the draw (so that a replayed graph continues the stream).  action_dtype:
    torch.int64 (default) or torch.int32.  out: (actions, log_prob, entropy) to write into; log_prob and entropy may each be None and are
    then not computed (None is returned in their place).  A logit of -inf masks its action; a row with a NaN, a +inf or nothing but
    -inf yields action 0 and NaN for log_prob and entropy.  Float64 arithmetic in a fixed order, bit-equal to tests/policy_host.py.
    Runs on the current stream, no synchronisation."""
    import torch as t

    seed, env_offset = _index("seed", seed), _index("env_offset", env_offset)
    x = _rows(t, logits, "logits", MAX_ACTIONS, f"[N, A] with N >= 1 and 1 <= A <= {MAX_ACTIONS}", two_d=True)
    N, A = x.shape
    step, step_t = _step(t, step)
    if action_dtype is None:
        action_dtype = out[0].dtype if out is not None and isinstance(out[0], t.Tensor) else t.int64
    if action_dtype not in (t.int64, t.int32):
        raise ValueError(f"action_dtype must be torch.int64 or torch.int32, got {action_dtype}")
    if out is not None:
        out = tuple(out)
        if len(out) != 3:
            raise ValueError(f"out must hold 3 entries (actions, log_prob, entropy), got {len(out)}")
        act = _vector(t, out[0], "out (actions)", (N,), (action_dtype,))
        lp = None if out[1] is None else _vector(t, out[1], "out (log_prob)", (N,), (t.float32,))
        en = None if out[2] is None else _vector(t, out[2], "out (entropy)", (N,), (t.float32,))
    dev = _one_device((("logits", x), ("step", step_t)) + ((("out (actions)", act), ("out (log_prob)", lp), ("out (entropy)", en)) if out is not None else ()))
    if out is None:
        act = t.empty(N, dtype=action_dtype, device=dev)
        lp = t.empty(N, dtype=t.float32, device=dev)
        en = t.empty(N, dtype=t.float32, device=dev)
    with t.cuda.device(dev):
        _check(lib.mxv_policy_sample_categorical(t.cuda.current_stream(dev).cuda_stream, N, A, x.data_ptr(), _ld(x, A), seed, env_offset, step,
                                                 _ptr(step_t), act.data_ptr(), int(action_dtype == t.int64), _ptr(lp), _ptr(en)))
    return (act, lp, en) if out is None else out      # the caller's own tensors


class PolicySampler(_Sampler):
    """sample_categorical() with the step counter kept on the device: every sample() draws step t of the stream (seed, env_offset) and
    advances t by one on the stream, so that calls recorded into a graph continue the stream at every replay.  state_dict() /
    load_state_dict() carry (seed, env_offset, step): a restored sampler continues bit-identically."""

    _WIDTH = ("num_actions", MAX_ACTIONS)

    def __init__(self, num_actions: int, *, seed: int = 0, env_offset: int = 0, action_dtype=None, device=0):
        super().__init__(num_actions, seed=seed, env_offset=env_offset, device=device)
        t = self._torch
        self.action_dtype = t.int64 if action_dtype is None else action_dtype
        if self.action_dtype not in (t.int64, t.int32):
            raise ValueError(f"action_dtype must be torch.int64 or torch.int32, got {action_dtype}")

    def sample(self, logits, out=None):
        """-> (actions, log_prob, entropy) of the next step of the stream; arguments as sample_categorical()."""
        self._columns("logits", logits, leading_dims=False)
        return sample_categorical(logits, seed=self.seed, step=self._step, env_offset=self.env_offset, action_dtype=self.action_dtype,
                                  out=out)

    def evaluate(self, logits, actions, out=None):
        """-> (log_prob, entropy) of stored `actions` under `logits`, differentiable: gym_amd.policy_eval.evaluate_categorical().  Draws
        nothing and leaves the stream where it is."""
        from .policy_eval import evaluate_categorical

        self._columns("logits", logits, leading_dims=True)
        return evaluate_categorical(logits, actions, out=out)


def sample_gaussian(mean, log_std, *, seed, step, env_offset=0, out=None):
    """Diagonal-Gaussian draws -> (actions float32 [N, D], log_prob float32 [N], entropy float32 [N]).

    mean float32 [N, D] on the device, 1 <= D <= 4, last dimension contiguous, rows may be strided (a view into a wider buffer).
    log_std float32 [N, D] likewise, or [D]: one row shared by all envs (a state-independent log_std).  seed, env_offset, step: as
    sample_categorical() — row i is global env env_offset + i, and a one-element int64 device tensor as `step` is read on the device and
    advanced by 1 behind the draw.  out: (actions, log_prob, entropy) to write into; actions may be a strided row view, log_prob and
    entropy may each be None and are then not computed (None is returned in their place).  action = mean + exp(log_std) * z with z from
    the engine's Philox streams (|z| <= 6.77); log_prob is that of the float32 action returned.  A row with a non-finite mean or
    log_std, or |log_std| > 80, yields NaN everywhere.  Float64 arithmetic in a fixed order, bit-equal to tests/gaussian_host.py.  Runs
    on the current stream, no synchronisation."""
    import torch as t

    seed, env_offset = _index("seed", seed), _index("env_offset", env_offset)
    mu = _rows(t, mean, "mean", MAX_ACTION_DIM, f"[N, D] with N >= 1 and 1 <= D <= {MAX_ACTION_DIM}", two_d=True)
    N, D = mu.shape
    ls, ls_ld = _log_std(t, log_std, mu, two_d=True)
    step, step_t = _step(t, step)
    if out is not None:
        out = tuple(out)
        if len(out) != 3:
            raise ValueError(f"out must hold 3 entries (actions, log_prob, entropy), got {len(out)}")
        act = _rows(t, out[0], "out (actions)", MAX_ACTION_DIM, f"({N}, {D})", two_d=True)
        if tuple(act.shape) != (N, D):
            raise ValueError(f"out (actions) must have shape ({N}, {D}), got {tuple(act.shape)}")
        lp = None if out[1] is None else _vector(t, out[1], "out (log_prob)", (N,), (t.float32,))
        en = None if out[2] is None else _vector(t, out[2], "out (entropy)", (N,), (t.float32,))
    dev = _one_device((("mean", mu), ("log_std", ls), ("step", step_t))
                      + ((("out (actions)", act), ("out (log_prob)", lp), ("out (entropy)", en)) if out is not None else ()))
    if out is None:
        act = t.empty((N, D), dtype=t.float32, device=dev)
        lp = t.empty(N, dtype=t.float32, device=dev)
        en = t.empty(N, dtype=t.float32, device=dev)
    with t.cuda.device(dev):
        _check(lib.mxv_policy_sample_gaussian(t.cuda.current_stream(dev).cuda_stream, N, D, mu.data_ptr(), _ld(mu, D), ls.data_ptr(), ls_ld, seed,
                                              env_offset, step, _ptr(step_t), act.data_ptr(), _ld(act, D), _ptr(lp), _ptr(en)))
    return (act, lp, en) if out is None else out      # the caller's own tensors


class GaussianSampler(_Sampler):
    """sample_gaussian() with the step counter kept on the device: every sample() draws step t of the stream (seed, env_offset) and advances
    t by one on the stream, so that calls recorded into a graph continue the stream at every replay.  state_dict() / load_state_dict()
    carry (seed, env_offset, step): a restored sampler continues bit-identically."""

    _WIDTH = ("action_dim", MAX_ACTION_DIM)

    def __init__(self, action_dim: int, *, seed: int = 0, env_offset: int = 0, device=0):
        super().__init__(action_dim, seed=seed, env_offset=env_offset, device=device)

    def sample(self, mean, log_std, out=None):
        """-> (actions, log_prob, entropy) of the next step of the stream; arguments as sample_gaussian()."""
        self._columns("mean", mean, leading_dims=False)
        return sample_gaussian(mean, log_std, seed=self.seed, step=self._step, env_offset=self.env_offset, out=out)

    def evaluate(self, mean, log_std, actions, out=None):
        """-> (log_prob, entropy) of stored `actions` under (mean, log_std), differentiable: gym_amd.policy_eval.evaluate_gaussian().  Draws
        nothing and leaves the stream where it is."""
        from .policy_eval import evaluate_gaussian

        self._columns("mean", mean, leading_dims=True)
        return evaluate_gaussian(mean, log_std, actions, out=out)
