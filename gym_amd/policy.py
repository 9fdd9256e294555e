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

POLICY_EXPORTS = ("mxv_policy_sample_categorical", "mxv_policy_sample_gaussian", "mxv_policy_last_error", "mxv_policy_last_launch")
MAX_ACTIONS = 64
MAX_ACTION_DIM = 4                      # dims of a Gaussian head: one Philox call per env yields four normals
STRAIGHT_LINE_ACTIONS = (2, 3, 4, 6)    # action counts with a register-resident instantiation (gym_amd/csrc/mxv_policy.hip)
_U64 = (1 << 64) - 1

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
    if rc == _native.OK:
        return
    msg = lib.mxv_policy_last_error().decode()
    if rc == _native.ERR_INVALID_ARG:
        raise ValueError(msg)
    raise _native.MxvError(rc, msg)


def last_launch():
    """(envs per lane, straight-line action count or 0 for the loop, workgroups) of this thread's last launch by sample_categorical()."""
    v, a, g = C.c_int32(), C.c_int32(), C.c_uint32()
    _check(lib.mxv_policy_last_launch(C.byref(v), C.byref(a), C.byref(g)))
    return v.value, a.value, g.value


def _index(name, v):
    """A non-negative integer below 2^64 as a Python int: int and NumPy integers; not bool, not float, not text."""
    ok = not isinstance(v, (bool, float, str, bytes))
    if ok:
        try:
            i = int(v)
            ok = i == v
        except (TypeError, ValueError):
            ok = False
    if not ok or not 0 <= i <= _U64:
        raise ValueError(f"{name} must be an integer in [0, 2^64), got {v!r}")
    return i


def _logits(t, x):
    if not isinstance(x, t.Tensor):
        raise ValueError(f"logits must be a torch tensor, got {type(x).__name__}")
    if x.dtype != t.float32:
        raise ValueError(f"logits must be torch.float32, got {x.dtype}")
    if x.dim() != 2 or x.shape[0] < 1 or not 1 <= x.shape[1] <= MAX_ACTIONS:
        raise ValueError(f"logits must have shape [N, A] with N >= 1 and 1 <= A <= {MAX_ACTIONS}, got {tuple(x.shape)}")
    if x.shape[1] > 1 and x.stride(1) != 1:
        raise ValueError(f"logits must be contiguous in their last dimension (stride {x.stride(1)}): rows may be strided views, elements not")
    if x.shape[0] > 1 and x.stride(0) < x.shape[1]:
        raise ValueError(f"logits have row stride {x.stride(0)} < A = {x.shape[1]}: rows overlap")
    return x


def _vector(t, x, name, n, dtypes):
    if not isinstance(x, t.Tensor):
        raise ValueError(f"{name} must be a torch tensor or None, got {type(x).__name__}")
    if x.dtype not in dtypes:
        raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {x.dtype}")
    if tuple(x.shape) != (n,):
        raise ValueError(f"{name} must have shape ({n},), got {tuple(x.shape)}")
    if n > 1 and x.stride(0) != 1:
        raise ValueError(f"{name} must be contiguous (stride {x.stride(0)})")
    return x


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
    x = _logits(t, logits)
    N, A = x.shape
    step_t = None
    if isinstance(step, t.Tensor):
        if step.dtype != t.int64 or step.numel() != 1:
            raise ValueError(f"a step tensor must be torch.int64 with one element, got {step.dtype} {tuple(step.shape)}")
        step_t, step = step, 0
    else:
        step = _index("step", step)
    if action_dtype is None:
        action_dtype = out[0].dtype if out is not None and isinstance(out[0], t.Tensor) else t.int64
    if action_dtype not in (t.int64, t.int32):
        raise ValueError(f"action_dtype must be torch.int64 or torch.int32, got {action_dtype}")
    if out is not None:
        out = tuple(out)
        if len(out) != 3:
            raise ValueError(f"out must hold 3 entries (actions, log_prob, entropy), got {len(out)}")
        act = _vector(t, out[0], "out (actions)", N, (action_dtype,))
        lp = None if out[1] is None else _vector(t, out[1], "out (log_prob)", N, (t.float32,))
        en = None if out[2] is None else _vector(t, out[2], "out (entropy)", N, (t.float32,))
    dev = x.device
    for name, y in (("logits", x), ("step", step_t)) + ((("out (actions)", act), ("out (log_prob)", lp), ("out (entropy)", en)) if out is not None else ()):
        if y is None:
            continue
        if not y.is_cuda:
            raise ValueError(f"{name} must be a device tensor, got one on {y.device} (gym_amd has no CPU fallback)")
        if y.device != dev:
            raise ValueError(f"{name} is on {y.device}, logits on {dev}: all tensors must be on one device")
    if out is None:
        act = t.empty(N, dtype=action_dtype, device=dev)
        lp = t.empty(N, dtype=t.float32, device=dev)
        en = t.empty(N, dtype=t.float32, device=dev)
    ld = x.stride(0) if N > 1 else A
    with t.cuda.device(dev):
        _check(lib.mxv_policy_sample_categorical(t.cuda.current_stream(dev).cuda_stream, N, A, x.data_ptr(), ld, seed, env_offset, step,
                                                 None if step_t is None else step_t.data_ptr(), act.data_ptr(), int(action_dtype == t.int64),
                                                 None if lp is None else lp.data_ptr(), None if en is None else en.data_ptr()))
    return act, lp, en


class PolicySampler:
    """sample_categorical() with the step counter kept on the device: every sample() draws step t of the stream (seed, env_offset) and
    advances t by one on the stream, so that calls recorded into a graph continue the stream at every replay.  state_dict() /
    load_state_dict() carry (seed, env_offset, step): a restored sampler continues bit-identically."""

    def __init__(self, num_actions: int, *, seed: int = 0, env_offset: int = 0, action_dtype=None, device=0):
        import torch as t

        if isinstance(num_actions, bool) or not isinstance(num_actions, int) or not 1 <= num_actions <= MAX_ACTIONS:
            raise ValueError(f"num_actions must be an integer in 1..{MAX_ACTIONS}, got {num_actions!r}")
        action_dtype = t.int64 if action_dtype is None else action_dtype
        if action_dtype not in (t.int64, t.int32):
            raise ValueError(f"action_dtype must be torch.int64 or torch.int32, got {action_dtype}")
        if not t.cuda.is_available():
            raise RuntimeError("PolicySampler needs a HIP device (torch.cuda.is_available() is False); gym_amd has no CPU fallback")
        self._torch = t
        self.num_actions = num_actions
        self.seed, self.env_offset = _index("seed", seed), _index("env_offset", env_offset)
        self.action_dtype = action_dtype
        self.device = device if isinstance(device, t.device) else t.device("cuda", device)
        self._step = t.zeros(1, dtype=t.int64, device=self.device)
        t.cuda.current_stream(self.device).synchronize()     # construction is rare: the counter is ready on whichever stream samples

    def sample(self, logits, out=None):
        """-> (actions, log_prob, entropy) of the next step of the stream; arguments as sample_categorical()."""
        if isinstance(logits, self._torch.Tensor) and logits.dim() == 2 and logits.shape[1] != self.num_actions:
            raise ValueError(f"logits must have {self.num_actions} columns (num_actions), got {tuple(logits.shape)}")
        return sample_categorical(logits, seed=self.seed, step=self._step, env_offset=self.env_offset, action_dtype=self.action_dtype,
                                  out=out)

    def evaluate(self, logits, actions, out=None):
        """-> (log_prob, entropy) of stored `actions` under `logits`, differentiable: gym_amd.policy_eval.evaluate_categorical().  Draws
        nothing and leaves the stream where it is."""
        from .policy_eval import evaluate_categorical

        if isinstance(logits, self._torch.Tensor) and logits.dim() >= 2 and logits.shape[-1] != self.num_actions:
            raise ValueError(f"logits must have {self.num_actions} columns (num_actions), got {tuple(logits.shape)}")
        return evaluate_categorical(logits, actions, out=out)

    def step_index(self) -> int:
        """How many draws the stream has made (synchronises)."""
        return int(self._step.item()) & _U64

    def state_dict(self) -> dict:
        return {"seed": self.seed, "env_offset": self.env_offset, "step": self.step_index(), "num_actions": self.num_actions}

    def load_state_dict(self, state: dict):
        if int(state.get("num_actions", self.num_actions)) != self.num_actions:
            raise ValueError(f"the state is of a sampler with {state['num_actions']} actions, this one has {self.num_actions}")
        self.seed, self.env_offset = _index("seed", state["seed"]), _index("env_offset", state["env_offset"])
        step = _index("step", state["step"])
        self._step.fill_(step - (1 << 64) if step >= (1 << 63) else step)


def _rows(t, x, name, max_cols, what):
    """A float32 [N, D] tensor whose rows may be strided views, elements not."""
    if not isinstance(x, t.Tensor):
        raise ValueError(f"{name} must be a torch tensor, got {type(x).__name__}")
    if x.dtype != t.float32:
        raise ValueError(f"{name} must be torch.float32, got {x.dtype}")
    if x.dim() != 2 or x.shape[0] < 1 or not 1 <= x.shape[1] <= max_cols:
        raise ValueError(f"{name} must have shape {what}, got {tuple(x.shape)}")
    if x.shape[1] > 1 and x.stride(1) != 1:
        raise ValueError(f"{name} must be contiguous in its last dimension (stride {x.stride(1)}): rows may be strided views, elements not")
    if x.shape[0] > 1 and x.stride(0) < x.shape[1]:
        raise ValueError(f"{name} has row stride {x.stride(0)} < D = {x.shape[1]}: rows overlap")
    return x


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
    mu = _rows(t, mean, "mean", MAX_ACTION_DIM, f"[N, D] with N >= 1 and 1 <= D <= {MAX_ACTION_DIM}")
    N, D = mu.shape
    if not isinstance(log_std, t.Tensor):
        raise ValueError(f"log_std must be a torch tensor, got {type(log_std).__name__}")
    if log_std.dim() == 1:
        if log_std.dtype != t.float32:
            raise ValueError(f"log_std must be torch.float32, got {log_std.dtype}")
        if log_std.shape[0] != D:
            raise ValueError(f"log_std must have shape ({N}, {D}) or ({D},), got {tuple(log_std.shape)}")
        if D > 1 and log_std.stride(0) != 1:
            raise ValueError(f"log_std must be contiguous in its last dimension (stride {log_std.stride(0)})")
        ls, ls_ld = log_std, 0
    else:
        ls = _rows(t, log_std, "log_std", MAX_ACTION_DIM, f"({N}, {D}) or ({D},)")
        if tuple(ls.shape) != (N, D):
            raise ValueError(f"log_std must have shape ({N}, {D}) or ({D},), got {tuple(ls.shape)}")
        ls_ld = ls.stride(0) if N > 1 else D
    step_t = None
    if isinstance(step, t.Tensor):
        if step.dtype != t.int64 or step.numel() != 1:
            raise ValueError(f"a step tensor must be torch.int64 with one element, got {step.dtype} {tuple(step.shape)}")
        step_t, step = step, 0
    else:
        step = _index("step", step)
    if out is not None:
        out = tuple(out)
        if len(out) != 3:
            raise ValueError(f"out must hold 3 entries (actions, log_prob, entropy), got {len(out)}")
        act = _rows(t, out[0], "out (actions)", MAX_ACTION_DIM, f"({N}, {D})")
        if tuple(act.shape) != (N, D):
            raise ValueError(f"out (actions) must have shape ({N}, {D}), got {tuple(act.shape)}")
        lp = None if out[1] is None else _vector(t, out[1], "out (log_prob)", N, (t.float32,))
        en = None if out[2] is None else _vector(t, out[2], "out (entropy)", N, (t.float32,))
    dev = mu.device
    for name, y in (("mean", mu), ("log_std", ls), ("step", step_t)) + ((("out (actions)", act), ("out (log_prob)", lp), ("out (entropy)", en)) if out is not None else ()):
        if y is None:
            continue
        if not y.is_cuda:
            raise ValueError(f"{name} must be a device tensor, got one on {y.device} (gym_amd has no CPU fallback)")
        if y.device != dev:
            raise ValueError(f"{name} is on {y.device}, mean on {dev}: all tensors must be on one device")
    if out is None:
        act = t.empty((N, D), dtype=t.float32, device=dev)
        lp = t.empty(N, dtype=t.float32, device=dev)
        en = t.empty(N, dtype=t.float32, device=dev)
    with t.cuda.device(dev):
        _check(lib.mxv_policy_sample_gaussian(t.cuda.current_stream(dev).cuda_stream, N, D, mu.data_ptr(), mu.stride(0) if N > 1 else D,
                                              ls.data_ptr(), ls_ld, seed, env_offset, step, None if step_t is None else step_t.data_ptr(),
                                              act.data_ptr(), act.stride(0) if N > 1 else D, None if lp is None else lp.data_ptr(),
                                              None if en is None else en.data_ptr()))
    return act, lp, en


class GaussianSampler:
    """sample_gaussian() with the step counter kept on the device: every sample() draws step t of the stream (seed, env_offset) and advances
    t by one on the stream, so that calls recorded into a graph continue the stream at every replay.  state_dict() / load_state_dict()
    carry (seed, env_offset, step): a restored sampler continues bit-identically."""

    def __init__(self, action_dim: int, *, seed: int = 0, env_offset: int = 0, device=0):
        if isinstance(action_dim, bool) or not isinstance(action_dim, int) or not 1 <= action_dim <= MAX_ACTION_DIM:
            raise ValueError(f"action_dim must be an integer in 1..{MAX_ACTION_DIM}, got {action_dim!r}")
        import torch as t

        if not t.cuda.is_available():
            raise RuntimeError("GaussianSampler needs a HIP device (torch.cuda.is_available() is False); gym_amd has no CPU fallback")
        self._torch = t
        self.action_dim = action_dim
        self.seed, self.env_offset = _index("seed", seed), _index("env_offset", env_offset)
        self.device = device if isinstance(device, t.device) else t.device("cuda", device)
        self._step = t.zeros(1, dtype=t.int64, device=self.device)
        t.cuda.current_stream(self.device).synchronize()     # construction is rare: the counter is ready on whichever stream samples

    def sample(self, mean, log_std, out=None):
        """-> (actions, log_prob, entropy) of the next step of the stream; arguments as sample_gaussian()."""
        if isinstance(mean, self._torch.Tensor) and mean.dim() == 2 and mean.shape[1] != self.action_dim:
            raise ValueError(f"mean must have {self.action_dim} columns (action_dim), got {tuple(mean.shape)}")
        return sample_gaussian(mean, log_std, seed=self.seed, step=self._step, env_offset=self.env_offset, out=out)

    def evaluate(self, mean, log_std, actions, out=None):
        """-> (log_prob, entropy) of stored `actions` under (mean, log_std), differentiable: gym_amd.policy_eval.evaluate_gaussian().  Draws
        nothing and leaves the stream where it is."""
        from .policy_eval import evaluate_gaussian

        if isinstance(mean, self._torch.Tensor) and mean.dim() >= 2 and mean.shape[-1] != self.action_dim:
            raise ValueError(f"mean must have {self.action_dim} columns (action_dim), got {tuple(mean.shape)}")
        return evaluate_gaussian(mean, log_std, actions, out=out)

    def step_index(self) -> int:
        """How many draws the stream has made (synchronises)."""
        return int(self._step.item()) & _U64

    def state_dict(self) -> dict:
        return {"seed": self.seed, "env_offset": self.env_offset, "step": self.step_index(), "action_dim": self.action_dim}

    def load_state_dict(self, state: dict):
        if int(state.get("action_dim", self.action_dim)) != self.action_dim:
            raise ValueError(f"the state is of a sampler with action_dim {state['action_dim']}, this one has {self.action_dim}")
        self.seed, self.env_offset = _index("seed", state["seed"]), _index("env_offset", state["env_offset"])
        step = _index("step", state["step"])
        self._step.fill_(step - (1 << 64) if step >= (1 << 63) else step)
