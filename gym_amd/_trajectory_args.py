"""What gym_amd.returns (GAE, returns-to-go) and gym_amd.vtrace check alike before they call the library — scalars, [K, N] matrices and
their one row stride, `out=`, the one-device rule — and how both bind the *_last_error / *_last_launch pair of their header.  The two
describe the same fault in the same words.  Importing this module does not import torch: every helper takes the torch module as `t`.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _native
from ._policy_args import _check, _ptr  # noqa: F401  (_ptr: for the two front ends)

RING_DEPTH = 4      # rows the kernels keep in flight ahead of the one they consume (kRing, gym_amd/csrc/mxv_trajectory.hpp)
VECTOR_MIN_ENVS = 1 << 21   # from here on (and with 16-byte alignment throughout) a lane owns four envs (kVecMinN)


def _bind(lib, family, callers):
    """Binds mxv_<family>_last_error and mxv_<family>_last_launch -> (check(rc), last_launch())."""
    last_error, launch = getattr(lib, f"mxv_{family}_last_error"), getattr(lib, f"mxv_{family}_last_launch")
    last_error.argtypes, last_error.restype = [], C.c_char_p
    launch.argtypes, launch.restype = [C.c_void_p, C.c_void_p], C.c_int

    def check(rc: int):
        if rc != _native.OK:
            _check(rc, last_error)

    def last_launch():
        v, g = C.c_int32(), C.c_uint32()
        check(launch(C.byref(v), C.byref(g)))
        return v.value, g.value

    last_launch.__doc__ = f"(envs per lane, workgroups) of this thread's last launch by {callers}: 4 envs per lane is the 16-byte path."
    return check, last_launch


def _scalar(name, v):
    """A finite real number as a Python float: int, float, NumPy scalars, 0-dim arrays and tensors; not bool, not text."""
    try:
        f = None if isinstance(v, (bool, str, bytes)) else float(v)
    except (TypeError, ValueError):
        f = None
    if f is None or not math.isfinite(f):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    return f


def _matrix(t, x, name, dtypes, shape=None):
    """A [K, N] tensor of one of `dtypes` whose last dimension is contiguous; torch.bool is taken as a uint8 view."""
    if not isinstance(x, t.Tensor):
        raise ValueError(f"{name} must be a torch tensor, got {type(x).__name__}")
    if x.dtype == t.bool and t.uint8 in dtypes:
        x = x.view(t.uint8)
    if x.dtype not in dtypes:
        raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {x.dtype}")
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


def _prepare(inputs, last_value, final_values, out, out_names, *, bare_out, count_word="tensor(s)", targets=False):
    """Every check that needs no device — types, dtypes, shapes, strides — then the device of every tensor.
    inputs: the (name, tensor) of the [K, N] inputs in the order of the C call, `reward` among them: it is checked first and gives the
    shape; final_values joins them when given.  bare_out: a tensor as `out` stands for one output (else it is iterated like any
    sequence).  targets: the outputs carry no graph — one that requires grad is refused, and the inputs are returned detached.
    -> (torch, the inputs by name, last_value, the outputs, ld, ld_out)"""
    import torch as t

    f32, u8 = (t.float32,), (t.uint8,)
    reward = _matrix(t, dict(inputs)["reward"], "reward", (t.float32, t.float64))
    shape = reward.shape
    ins = [(name, reward if name == "reward" else _matrix(t, x, name, u8 if name in ("terminated", "truncated") else f32, shape))
           for name, x in inputs]
    if final_values is not None:
        ins.append(("final_values", _matrix(t, final_values, "final_values", f32, shape)))
    last_value = _vector(t, last_value, "last_value", shape[1])
    ld = _row_stride(ins, "inputs")
    outs = None
    if out is not None:
        given = (out,) if bare_out and isinstance(out, t.Tensor) else tuple(out)
        if len(given) != len(out_names):
            raise ValueError(f"out must hold {len(out_names)} {count_word} ({', '.join(out_names)}), got {len(given)}")
        outs = [(f"out ({name})", _matrix(t, x, f"out ({name})", f32, shape)) for name, x in zip(out_names, given)]
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
    if targets:
        for name, x in outs:
            if x.requires_grad:
                raise ValueError(f"{name} requires grad: the targets carry no graph and are written in place")
    ld_out = _row_stride(outs, "outputs")
    if targets:     # the kernel reads the data; nothing is recorded for autograd
        ins = [(name, x.detach()) for name, x in ins]
        last_value = None if last_value is None else last_value.detach()
    return t, dict(ins), last_value, [x for _, x in outs], ld, ld_out
