"""GAE(lambda) advantages and discounted returns-to-go over [K, N] trajectory tensors, on the device (include/mxv_gae.h).

The last stage of the device-resident path: `reward`, `terminated` and `truncated` are what DeviceRollout / TabularRollout /
BlackjackRollout leave in their trajectory tensors, `values` is the learner's V of the observation each action was taken from, and
`final_values` its V of `final_obs` (trajectory_buffers(want_final=True)) — read only where a step was truncated and not terminated, so
that a truncated episode bootstraps from its own last observation and never from the reset observation that follows it.

One kernel launch on the caller's current stream, no synchronisation, no allocation beyond the outputs (none with `out=`): recordable
into a torch.cuda.graph.  The header is optional (mxv.h does not include it), so its symbols are bound here, over the same library as
gym_amd._native, and are not part of _native.EXPORTS.  Importing this module does not import torch.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _native

GAE_EXPORTS = ("mxv_gae", "mxv_discounted_returns", "mxv_gae_last_error", "mxv_gae_last_launch")
RING_DEPTH = 4      # rows the kernel keeps in flight ahead of the one it consumes (kRing, gym_amd/csrc/mxv_gae.hip)
VECTOR_MIN_ENVS = 1 << 21   # from here on (and with 16-byte alignment throughout) a lane owns four envs (kVecMinN)

lib = _native.lib
lib.mxv_gae.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                        C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int64]
lib.mxv_gae.restype = C.c_int
lib.mxv_discounted_returns.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int64]
lib.mxv_discounted_returns.restype = C.c_int
lib.mxv_gae_last_error.argtypes = []
lib.mxv_gae_last_error.restype = C.c_char_p
lib.mxv_gae_last_launch.argtypes = [C.c_void_p, C.c_void_p]
lib.mxv_gae_last_launch.restype = C.c_int


def _check(rc: int):
    if rc == _native.OK:
        return
    msg = lib.mxv_gae_last_error().decode()
    if rc == _native.ERR_INVALID_ARG:
        raise ValueError(msg)
    raise _native.MxvError(rc, msg)


def last_launch():
    """(envs per lane, workgroups) of this thread's last launch by gae() / discounted_returns(): 4 envs per lane is the 16-byte path."""
    v, g = C.c_int32(), C.c_uint32()
    _check(lib.mxv_gae_last_launch(C.byref(v), C.byref(g)))
    return v.value, g.value


def pre_step_observations(first_obs, traj_obs):
    """The observations the actions of a chunk were taken FROM, which is what `values` must be the learner's V of.  The trajectory
    tensors of rollout_per_step / rollout_tape hold in traj["obs"][k] the observation AFTER step k (after an autoreset: the next
    episode's first one), so the observation before step k is `first_obs` for k = 0 — what reset() returned, or traj["obs"][K-1] of the
    previous chunk (clone it if the buffers are reused) — and traj["obs"][k-1] after that.  -> torch.cat((first_obs[None], traj_obs[:-1]));
    `last_value` is then V(traj_obs[-1])."""
    import torch as t

    if tuple(first_obs.shape) != tuple(traj_obs.shape[1:]):
        raise ValueError(f"first_obs must have the shape of one row of the trajectory's obs {tuple(traj_obs.shape[1:])}, got {tuple(first_obs.shape)}")
    return t.cat((first_obs.to(traj_obs.dtype).unsqueeze(0), traj_obs[:-1]))


def _scalar(name, v):
    """A finite real number as a Python float: int, float, NumPy scalars, 0-dim arrays and tensors; not bool, not text."""
    try:
        f = None if isinstance(v, (bool, str, bytes)) else float(v)
    except (TypeError, ValueError):
        f = None
    if f is None or not math.isfinite(f):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    return f


def _dtype_name(t, dtypes):
    return " or ".join(str(d) for d in dtypes)


def _matrix(t, x, name, dtypes, shape=None):
    """A [K, N] tensor of one of `dtypes` whose last dimension is contiguous; torch.bool is taken as a uint8 view."""
    if not isinstance(x, t.Tensor):
        raise ValueError(f"{name} must be a torch tensor, got {type(x).__name__}")
    if x.dtype == t.bool and t.uint8 in dtypes:
        x = x.view(t.uint8)
    if x.dtype not in dtypes:
        raise ValueError(f"{name} must be {_dtype_name(t, dtypes)}, got {x.dtype}")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{name} must have shape [K, N] with K, N >= 1, got {tuple(x.shape)}")
    if shape is not None and tuple(x.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)} like reward, got {tuple(x.shape)}")
    if x.shape[1] > 1 and x.stride(1) != 1:
        raise ValueError(f"{name} must be contiguous in its last dimension (stride {x.stride(1)}): rows may be strided views, elements not")
    if x.shape[0] > 1 and x.stride(0) < x.shape[1]:
        raise ValueError(f"{name} has row stride {x.stride(0)} < N = {x.shape[1]}: rows overlap")
    return x


def _vector(t, x, name, n):
    if x is None:
        return None
    if not isinstance(x, t.Tensor):
        raise ValueError(f"{name} must be a torch tensor or None, got {type(x).__name__}")
    if x.dtype != t.float32:
        raise ValueError(f"{name} must be torch.float32, got {x.dtype}")
    if tuple(x.shape) != (n,):
        raise ValueError(f"{name} must have shape ({n},), got {tuple(x.shape)}")
    if n > 1 and x.stride(0) != 1:
        raise ValueError(f"{name} must be contiguous (stride {x.stride(0)})")
    return x


def _row_stride(tensors, what):
    """The one row stride (in elements) of [K, N] tensors, which the C ABI takes once for all of them."""
    K, N = tensors[0][1].shape
    if K == 1:
        return N        # a single row has no stride to agree on
    lds = {name: x.stride(0) for name, x in tensors}
    if len(set(lds.values())) != 1:
        raise ValueError(f"the {what} must share one row stride (the C ABI takes a single one), got " +
                         ", ".join(f"{k}: {v}" for k, v in lds.items()))
    return next(iter(lds.values()))


def _prepare(with_values, reward, terminated, truncated, values, last_value, final_values, out, out_names):
    """Every check that needs no device — types, dtypes, shapes, strides — then the device of every tensor.  with_values: GAE (else
    returns-to-go, which takes no `values`)."""
    import torch as t

    reward = _matrix(t, reward, "reward", (t.float32, t.float64))
    shape = reward.shape
    ins = [("reward", reward), ("terminated", _matrix(t, terminated, "terminated", (t.uint8,), shape)),
           ("truncated", _matrix(t, truncated, "truncated", (t.uint8,), shape))]
    if with_values:
        ins.append(("values", _matrix(t, values, "values", (t.float32,), shape)))
    if final_values is not None:
        ins.append(("final_values", _matrix(t, final_values, "final_values", (t.float32,), shape)))
    last_value = _vector(t, last_value, "last_value", shape[1])
    ld = _row_stride(ins, "inputs")
    outs = None
    if out is not None:
        given = (out,) if len(out_names) == 1 and isinstance(out, t.Tensor) else tuple(out)
        if len(given) != len(out_names):
            raise ValueError(f"out must hold {len(out_names)} tensor(s) ({', '.join(out_names)}), got {len(given)}")
        outs = [(f"out ({name})", _matrix(t, x, f"out ({name})", (t.float32,), shape)) for name, x in zip(out_names, given)]
    dev = reward.device
    for name, x in ins + [("last_value", last_value)] + (outs or []):
        if x is None:
            continue
        if not x.is_cuda:
            raise ValueError(f"{name} must be a device tensor, got one on {x.device} (gym_amd has no CPU fallback)")
        if x.device != dev:
            raise ValueError(f"{name} is on {x.device}, reward on {dev}: all tensors must be on one device")
    if outs is None:
        outs = [(name, t.empty(tuple(shape), dtype=t.float32, device=dev)) for name in out_names]
    ld_out = _row_stride(outs, "outputs")
    return t, dict(ins), last_value, [x for _, x in outs], ld, ld_out


def _ptr(x):
    return None if x is None else x.data_ptr()


def gae(reward, terminated, truncated, values, last_value=None, *, gamma: float = 0.99, lam: float = 0.95, final_values=None, out=None):
    """GAE(lambda) over a [K, N] chunk -> (advantages, returns), both float32 [K, N].

    reward float32 / float64 [K, N]; terminated, truncated uint8 (nonzero = set) or bool [K, N]; values float32 [K, N]: V of the
    observation the action of step t was taken FROM — not of traj["obs"][t] of a rollout_per_step dict, which is the observation after
    step t (pre_step_observations() builds the right ones); last_value float32 [N]: V of the observation after step K-1 (None = 0);
    final_values float32 [K, N] or None: V(final_obs[t]), read only where truncated[t] is set and terminated[t] is not (None = 0 there);
    out: a pair of float32 [K, N] tensors to write into.  Rows may be strided views (one row stride for all inputs, one for the
    outputs), the last dimension is contiguous.  An output may not share memory with an input or with the other output (ValueError):
    column blocks of one wide buffer — out=(buf[:, :N], buf[:, N:2*N]) — are fine, as are views whose byte ranges do not meet at all;
    views that interleave with different row strides (in bytes) are refused even where no element coincides.  Float64 arithmetic, one
    rounding per operation, bit-equal to tests/gae_host.py; the episode cut is a select, so a NaN of a later episode never crosses a
    boundary.  gamma, lam: finite real numbers.  Runs on the current stream, no synchronisation."""
    gamma, lam = _scalar("gamma", gamma), _scalar("lam", lam)
    t, ins, lv, outs, ld, ld_out = _prepare(True, reward, terminated, truncated, values, last_value, final_values, out, ("advantages", "returns"))
    r = ins["reward"]
    K, N = r.shape
    with t.cuda.device(r.device):
        _check(lib.mxv_gae(t.cuda.current_stream(r.device).cuda_stream, K, N, r.data_ptr(), int(r.dtype == t.float64), ld,
                           ins["terminated"].data_ptr(), ins["truncated"].data_ptr(), ins["values"].data_ptr(), _ptr(lv),
                           _ptr(ins.get("final_values")), gamma, lam, outs[0].data_ptr(), outs[1].data_ptr(), ld_out))
    return outs[0], outs[1]


def discounted_returns(reward, terminated, truncated, *, gamma: float = 0.99, last_value=None, final_values=None, out=None):
    """Discounted returns-to-go over a [K, N] chunk -> returns float32 [K, N]: G_t = reward[t] + gamma * G_{t+1}, cut where
    terminated | truncated is set (bootstrapping with final_values where only truncated is), G_K = last_value (None = 0).  Arguments,
    layout and arithmetic as gae(); `out` is one float32 [K, N] tensor."""
    gamma = _scalar("gamma", gamma)
    t, ins, lv, outs, ld, ld_out = _prepare(False, reward, terminated, truncated, None, last_value, final_values, out, ("returns",))
    r = ins["reward"]
    K, N = r.shape
    with t.cuda.device(r.device):
        _check(lib.mxv_discounted_returns(t.cuda.current_stream(r.device).cuda_stream, K, N, r.data_ptr(), int(r.dtype == t.float64), ld,
                                          ins["terminated"].data_ptr(), ins["truncated"].data_ptr(), _ptr(lv),
                                          _ptr(ins.get("final_values")), gamma, outs[0].data_ptr(), ld_out))
    return outs[0]
