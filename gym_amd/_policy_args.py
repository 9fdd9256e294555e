"""What gym_amd.policy (the samplers) and gym_amd.policy_eval (the evaluators) check alike before they call the library: the limits of a
head, integers, row tensors and vectors, the one-device rule, a Gaussian head's log_std, the step argument — and the device step counter
that PolicySampler and GaussianSampler keep.  A sampler and its evaluator describe the same fault in the same words.  Importing this
module does not import torch: every helper takes the torch module as `t`.
"""
from __future__ import annotations

from . import _native

MAX_ACTIONS = 64
MAX_ACTION_DIM = 4                      # dims of a Gaussian head: one Philox call per env yields four normals
STRAIGHT_LINE_ACTIONS = (2, 3, 4, 6)    # action counts with a register-resident instantiation (gym_amd/csrc/mxv_policy.hip, mxv_policy_eval.hip)
LEAF_ROWS = 1024                        # rows per leaf of the sum tree of the losses, and partials per group of a level (kLeafRows, kTreeFan of gym_amd/csrc/mxv_sum_tree.hpp)
_U64 = (1 << 64) - 1


def _check(rc: int, last_error):
    """Raises what the C call reported: `last_error` is the *_last_error function of its header."""
    if rc == _native.OK:
        return
    msg = last_error().decode()
    if rc == _native.ERR_INVALID_ARG:
        raise ValueError(msg)
    raise _native.MxvError(rc, msg)


def _ptr(x):
    return None if x is None else x.data_ptr()


def _ld(x2, W):
    return x2.stride(0) if x2.shape[0] > 1 else W


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


def _rows(t, x, name, max_cols, what, two_d=False):
    """A float32 [..., W] tensor as its [M, W] rows: 2-D tensors may have strided rows (views into wider buffers), more dims must
    flatten without a copy — or, with `two_d`, are refused."""
    if not isinstance(x, t.Tensor):
        raise ValueError(f"{name} must be a torch tensor, got {type(x).__name__}")
    if x.dtype != t.float32:
        raise ValueError(f"{name} must be torch.float32, got {x.dtype}")
    if (x.dim() != 2 if two_d else x.dim() < 2) or x.numel() == 0 or not 1 <= x.shape[-1] <= max_cols:
        raise ValueError(f"{name} must have shape {what}, got {tuple(x.shape)}")
    W = x.shape[-1]
    if x.dim() == 2:
        x2 = x
    else:
        try:
            x2 = x.view(-1, W)
        except RuntimeError:
            raise ValueError(f"{name} of shape {tuple(x.shape)} with strides {tuple(x.stride())} cannot be viewed as [M, {W}] rows "
                             f"(view(-1, {W}) fails): pass a contiguous tensor") from None
    if W > 1 and x2.stride(1) != 1:
        raise ValueError(f"{name} must be contiguous in its last dimension (stride {x2.stride(1)}): rows may be strided views, elements not")
    if x2.shape[0] > 1 and x2.stride(0) < W:
        raise ValueError(f"{name} has row stride {x2.stride(0)} < {W}: rows overlap")
    return x2


def _vector(t, x, name, lead, dtypes):
    """A tensor of shape `lead` (the rows' leading dims) as a contiguous [M] vector."""
    if not isinstance(x, t.Tensor):
        raise ValueError(f"{name} must be a torch tensor, got {type(x).__name__}")
    if x.dtype not in dtypes:
        raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {x.dtype}")
    if tuple(x.shape) != tuple(lead):
        raise ValueError(f"{name} must have shape {tuple(lead)}, got {tuple(x.shape)}")
    try:
        v = x.view(-1)
    except RuntimeError:
        v = None
    if v is None or (v.shape[0] > 1 and v.stride(0) != 1):
        raise ValueError(f"{name} must be contiguous (strides {tuple(x.stride())})")
    return v


def _tree_launches(rows):
    """Launches of the sum tree over `rows` rows: the leaves, then one per level of LEAF_ROWS partials a group until one group is left."""
    count, n = -(-int(rows) // LEAF_ROWS), 2
    while count > LEAF_ROWS:
        count, n = -(-count // LEAF_ROWS), n + 1
    return n


def _workspace(t, workspace, M, dev, need, module_name):
    """The caller's workspace (a contiguous 1-D uint8 or float64 tensor of at least `need` bytes, what gym_amd.`module_name`.workspace_bytes(M)
    gives), or a fresh one -> (tensor, its bytes)."""
    if workspace is None:
        return t.empty(need // 8, dtype=t.float64, device=dev), need
    w = _vector(t, workspace, "workspace", getattr(workspace, "shape", ()), (t.uint8, t.float64))
    if w.dim() != 1 or tuple(workspace.shape) != tuple(w.shape):
        raise ValueError(f"workspace must be 1-D, got shape {tuple(workspace.shape)}")
    have = w.numel() * w.element_size()
    if have < need:
        raise ValueError(f"workspace holds {have} bytes, {M} rows need {need} (gym_amd.{module_name}.workspace_bytes)")
    return w, have


def _one_device(named):
    """The device of the first of the (name, tensor or None) pairs, which every other one must be on."""
    first, dev = named[0][0], named[0][1].device
    for name, y in named:
        if y is None:
            continue
        if not y.is_cuda:
            raise ValueError(f"{name} must be a device tensor, got one on {y.device} (gym_amd has no CPU fallback)")
        if y.device != dev:
            raise ValueError(f"{name} is on {y.device}, {first} on {dev}: all tensors must be on one device")
    return dev


def _log_std_ld(ls, D):
    """The row stride the library takes for a checked log_std; 0: the one shared row."""
    return 0 if ls.dim() == 1 else _ld(ls, D)


def _log_std(t, log_std, mean, two_d=False):
    """A Gaussian head's log_std, of mean's shape or [D] (one row shared by all rows) -> (its rows or the shared row, row stride)."""
    D = mean.shape[-1]
    shapes = f"{tuple(mean.shape)} or ({D},)"
    if not isinstance(log_std, t.Tensor):
        raise ValueError(f"log_std must be a torch tensor, got {type(log_std).__name__}")
    if log_std.dim() == 1:
        if log_std.dtype != t.float32:
            raise ValueError(f"log_std must be torch.float32, got {log_std.dtype}")
        if log_std.shape[0] != D:
            raise ValueError(f"log_std must have shape {shapes}, got {tuple(log_std.shape)}")
        if D > 1 and log_std.stride(0) != 1:
            raise ValueError(f"log_std must be contiguous in its last dimension (stride {log_std.stride(0)})")
        ls = log_std
    else:
        ls = _rows(t, log_std, "log_std", MAX_ACTION_DIM, shapes, two_d)
        if tuple(log_std.shape) != tuple(mean.shape):
            raise ValueError(f"log_std must have shape {shapes}, got {tuple(log_std.shape)}")
    return ls, _log_std_ld(ls, D)


def _step(t, step):
    """The step argument -> (step, None) for an integer, (0, tensor) for a one-element int64 tensor, which the device reads and advances."""
    if isinstance(step, t.Tensor):
        if step.dtype != t.int64 or step.numel() != 1:
            raise ValueError(f"a step tensor must be torch.int64 with one element, got {step.dtype} {tuple(step.shape)}")
        return 0, step
    return _index("step", step), None


class _Sampler:
    """What PolicySampler and GaussianSampler keep alike: the stream (seed, env_offset), its step counter on the device, and the
    checkpoint of both.  _WIDTH names the subclass's width attribute (also its state_dict key) and its upper limit."""

    _WIDTH = (None, 0)

    def __init__(self, width, *, seed, env_offset, device):
        name, limit = self._WIDTH
        if isinstance(width, bool) or not isinstance(width, int) or not 1 <= width <= limit:
            raise ValueError(f"{name} must be an integer in 1..{limit}, got {width!r}")
        import torch as t

        if not t.cuda.is_available():
            raise RuntimeError(f"{type(self).__name__} needs a HIP device (torch.cuda.is_available() is False); gym_amd has no CPU fallback")
        self._torch = t
        setattr(self, name, width)
        self.seed, self.env_offset = _index("seed", seed), _index("env_offset", env_offset)
        self.device = device if isinstance(device, t.device) else t.device("cuda", device)
        self._step = t.zeros(1, dtype=t.int64, device=self.device)
        t.cuda.current_stream(self.device).synchronize()     # construction is rare: the counter is ready on whichever stream samples

    def _columns(self, name, x, leading_dims):
        """Refuses a head output `x` whose last dimension is not this sampler's width; anything else is for the call's own checks."""
        width = getattr(self, self._WIDTH[0])
        if isinstance(x, self._torch.Tensor) and (x.dim() >= 2 if leading_dims else x.dim() == 2) and x.shape[-1] != width:
            raise ValueError(f"{name} must have {width} columns ({self._WIDTH[0]}), got {tuple(x.shape)}")

    def step_index(self) -> int:
        """How many draws the stream has made (synchronises)."""
        return int(self._step.item()) & _U64

    def state_dict(self) -> dict:
        name = self._WIDTH[0]
        return {"seed": self.seed, "env_offset": self.env_offset, "step": self.step_index(), name: getattr(self, name)}

    def load_state_dict(self, state: dict):
        name = self._WIDTH[0]
        width = getattr(self, name)
        if int(state.get(name, width)) != width:
            raise ValueError(f"the state is of a sampler with {name} = {state[name]}, this one has {width}")
        self.seed, self.env_offset = _index("seed", state["seed"]), _index("env_offset", state["env_offset"])
        step = _index("step", state["step"])
        self._step.fill_(step - (1 << 64) if step >= (1 << 63) else step)
