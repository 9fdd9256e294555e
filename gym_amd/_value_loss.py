"""What gym_amd.dqn, gym_amd.c51 and gym_amd.qr (the three value-based losses) do alike around their own rows: binding the entry points of
their header, the workspace and the launch count, the [..., A, W] rows of a distributional head, the one target mode, out= and
workspace=, the torch.autograd.Function and everything behind the checks of a call — the device rule, the dispatch with or without
gradients, the allocations and the forward call.  gym_amd.ppo takes the binding of its workspace and out= / workspace= from here.  A
module keeps what is its own: its constants, its `_Inputs` (the arguments of its C calls), its scalars and its optional outputs.
Importing this module does not import torch: every helper takes the torch module as `t`.
"""
from __future__ import annotations

import ctypes as C

from ._policy_args import LEAF_ROWS, MAX_ACTIONS, _one_device, _ptr, _tree_launches, _vector
from ._policy_args import _check as _raise
from ._policy_args import _workspace as _shared_workspace


class Bound:
    """The entry points `prefix`_workspace_bytes and `prefix`_last_error of `lib`, bound — and, with `inputs` (the ctypes of stream ..
    weights), `prefix`_loss (inputs + forward_tail: the workspace, its bytes, `extras` optional outputs, loss, stats) and
    `prefix`_loss_backward (inputs + the incoming gradient and the dense one).  `leaf_finishes`: a rows kernel runs before the leaves,
    and a batch of one leaf finishes in the leaf launch."""

    def __init__(self, lib, prefix, inputs=None, forward_tail=(), leaf_finishes=False, stats=8):
        P, I64 = C.c_void_p, C.c_int64
        self.name, self.leaf_finishes, self.stats = prefix[len("mxv_"):], leaf_finishes, stats
        self._bytes, self._last_error = getattr(lib, prefix + "_workspace_bytes"), getattr(lib, prefix + "_last_error")
        self._bytes.argtypes, self._bytes.restype = [I64], I64
        self._last_error.argtypes, self._last_error.restype = [], C.c_char_p
        if inputs is not None:
            self.loss, self.backward = getattr(lib, prefix + "_loss"), getattr(lib, prefix + "_loss_backward")
            self.loss.argtypes, self.backward.argtypes = inputs + list(forward_tail), inputs + [P, P]
            self.loss.restype = self.backward.restype = C.c_int
            self.extras = len(forward_tail) - 4

    def check(self, rc: int):
        _raise(rc, self._last_error)

    def workspace_bytes(self, rows: int) -> int:
        """Bytes of `workspace=` that a batch of `rows` rows needs: the partial sums of its leaves and, where a wave owns a row (c51, qr),
        six float64 per row."""
        n = int(self._bytes(int(rows)))
        if n == 0:
            raise ValueError(f"rows must be in 1..2^40, got {rows!r}")
        return n

    def launches(self, rows: int) -> int:
        """Kernel launches of one forward on `rows` rows: the leaves, then one per level of the tree (2 up to 2^20 rows, 3 up to 2^30) —
        where a wave owns a row (c51, qr), the rows before them, and the leaves finish a batch of one leaf: 2 up to 1024 rows, 3 up to
        2^20, 4 up to 2^30.  The backward is always one."""
        self.workspace_bytes(rows)
        if not self.leaf_finishes:
            return _tree_launches(rows)
        return 2 if int(rows) <= LEAF_ROWS else 1 + _tree_launches(rows)

    def workspace(self, t, workspace, M, dev):
        return _shared_workspace(t, workspace, M, dev, self.workspace_bytes(M), self.name)


def _no_grad_input(t, x, name):
    if x is not None and t.is_grad_enabled() and x.requires_grad:
        raise ValueError(f"{name} must not require grad: the loss is differentiable with respect to q alone")


def _heads_checker(letter, low, high, noun):
    """The row checker _heads(t, x, name) of a head of `low` <= W <= `high` `noun`, W being called `letter`."""

    def _heads(t, x, name):
        """A float32 [..., A, W] tensor as its [M, A, W] rows: the last two dims contiguous; 3-D tensors may have strided rows (views into
        wider buffers), more dims must flatten without a copy."""
        if not isinstance(x, t.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(x).__name__}")
        if x.dtype != t.float32:
            raise ValueError(f"{name} must be torch.float32, got {x.dtype}")
        if x.dim() < 3 or x.numel() == 0 or not 1 <= x.shape[-2] <= MAX_ACTIONS or not low <= x.shape[-1] <= high:
            raise ValueError(f"{name} must have shape [..., A, {letter}] with at least one row, 1 <= A <= {MAX_ACTIONS} and {low} <= {letter} <= {high}, "
                             f"got {tuple(x.shape)}")
        A, W = x.shape[-2:]
        if x.dim() == 3:
            x3 = x
        else:
            try:
                x3 = x.view(-1, A, W)
            except RuntimeError:
                raise ValueError(f"{name} of shape {tuple(x.shape)} with strides {tuple(x.stride())} cannot be viewed as [M, {A}, {W}] rows "
                                 f"(view(-1, {A}, {W}) fails): pass a contiguous tensor") from None
        if (W > 1 and x3.stride(2) != 1) or (A > 1 and x3.stride(1) != W):
            raise ValueError(f"{name} must be contiguous in its last two dimensions (strides {tuple(x3.stride())}): rows may be strided "
                             f"views, actions and {noun} not")
        if x3.shape[0] > 1 and x3.stride(0) < A * W:
            raise ValueError(f"{name} has row stride {x3.stride(0)} < {A * W}: rows overlap")
        return x3

    return _heads


def _ld3(x3):
    return x3.stride(0) if x3.shape[0] > 1 else x3.shape[1] * x3.shape[2]


def _target_mode(t, rows, lead, like, direct, boot, online, extras=(), rows_args=()):
    """Exactly one target mode -> the checked (reward, terminated, next, online) of the bootstrap mode, None each in the direct mode.

    like, direct, online: (name, argument) of the call's first argument, of its direct target and of its online selector; boot: the three
    bootstrap arguments by name (reward, terminated, the next rows); extras: further (name, argument) that belong to the bootstrap
    mode.  rows(t, x, name, *rows_args) is the module's row checker; the next rows and the selector must have `like`'s shape."""
    b0, b1, b2 = boot
    if direct[1] is not None:
        given = [k for k, v in boot.items() if v is not None]
        if given:
            raise ValueError(f"{direct[0]} is given together with {', '.join(given)}: exactly one target mode")
        for name, x in (online,) + extras:
            if x is not None:
                raise ValueError(f"{name} is given with {direct[0]}: it belongs to the bootstrap mode ({', '.join(boot)})")
        return None, None, None, None
    missing = [k for k, v in boot.items() if v is None]
    if len(missing) == 3:
        raise ValueError(f"neither {direct[0]} nor {b0}, {b1} and {b2} are given: exactly one target mode")
    if missing:
        raise ValueError(f"the bootstrap mode needs {b0}, {b1} and {b2}: {', '.join(missing)} missing")
    reward = _vector(t, boot[b0], b0, lead, (t.float32,))
    terminated = boot[b1]
    if isinstance(terminated, t.Tensor) and terminated.dtype == t.bool:
        terminated = terminated.view(t.uint8)
    checked = [reward, _vector(t, terminated, b1, lead, (t.uint8,))]
    shape = tuple(like[1].shape)
    for name, x in ((b2, boot[b2]), online):
        if x is not None:
            x, given = rows(t, x, name, *rows_args), tuple(x.shape)
            if given != shape:
                raise ValueError(f"{name} must have shape {shape} like {like[0]}, got {given}")
        checked.append(x)
    return checked


def _outputs(t, out, workspace, grads, what, stats):
    """out= and workspace= of a call whose gradients are wanted or not (`grads`; `what` names what requires grad) -> (out as a tuple,
    its checked loss, its checked stats), or (None, None, None) without out=."""
    if (out is not None or workspace is not None) and grads:
        raise ValueError(f"out= and workspace= cannot be used when {what} requires grad: autograd owns the outputs")
    if out is None:
        return None, None, None
    out = tuple(out)
    if len(out) != 2:
        raise ValueError(f"out must hold 2 entries (loss, stats), got {len(out)}")
    return out, _vector(t, out[0], "out (loss)", (), (t.float32,)), _vector(t, out[1], "out (stats)", (stats,), (t.float32,))


def _forward(t, b, a, extras, workspace=None, loss=None, stats=None):
    """The forward call of the checked inputs `a` into the caller's workspace and outputs, or into fresh ones -> (loss, stats)."""
    ws, ws_bytes = b.workspace(t, workspace, a.M, a.dev)
    if loss is None:
        loss = t.empty((), dtype=t.float32, device=a.dev)
        stats = t.empty(b.stats, dtype=t.float32, device=a.dev)
    with t.cuda.device(a.dev):
        b.check(b.loss(*a.call_args(t), ws.data_ptr(), ws_bytes, *[_ptr(x) for x in extras], loss.data_ptr(), stats.data_ptr()))
    return loss, stats


def _make_function(name, inputs, b):
    """The torch.autograd.Function `name` of the loss bound as `b`: forward(rows, a, *extras) with `a` the checked inputs (an `inputs`,
    its rows detached) and `extras` the optional outputs; it saves only the inputs, and the backward recomputes the rows."""
    import torch as t
    from torch.autograd.function import once_differentiable

    none = (None,) * (2 + b.extras)

    def forward(ctx, rows, a, *extras):
        ctx.set_materialize_grads(False)
        loss, stats = _forward(t, b, a, extras)
        ctx.save_for_backward(*(getattr(a, k) for k in a.TENSORS))      # the inputs alone: the backward recomputes the rows
        ctx.scalars = tuple(getattr(a, k) for k in a.SCALARS)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @once_differentiable
    def backward(ctx, g_loss, _g_stats):
        if g_loss is None or not ctx.needs_input_grad[0]:
            return none
        a = inputs()
        for k, v in zip(a.TENSORS + a.SCALARS, ctx.saved_tensors + ctx.scalars):
            setattr(a, k, v)
        g = g_loss.contiguous()      # one float32 in device memory: read by the kernel, never by the host
        grad = t.empty(a.grad_shape(), dtype=t.float32, device=a.dev)      # contiguous; every element is written
        with t.cuda.device(a.dev):
            b.check(b.backward(*a.call_args(t), g.data_ptr(), grad.data_ptr()))
        return (grad,) + none[1:]

    return type(name, (t.autograd.Function,), {"forward": staticmethod(forward), "backward": staticmethod(backward), "__module__": inputs.__module__})


def _finish(t, b, function, a, named, workspace, out):
    """A call behind the checks of its inputs -> (loss, stats).  named: the (name, checked tensor or None) of every tensor argument in
    the order of the signature — the first is the one the loss is differentiable in, an attribute of `a` under its name; the last
    b.extras are the optional outputs.  function() is the module's lazy autograd Function."""
    first, rows = named[0]
    grads = t.is_grad_enabled()
    if grads:
        for name, x in named[1:]:
            if x is not None and x.requires_grad:
                _no_grad_input(t, x, name)
        grads = rows.requires_grad
    out, loss, stats = _outputs(t, out, workspace, grads, first, b.stats)
    a.dev = _one_device(named + [("out (loss)", loss), ("out (stats)", stats), ("workspace", workspace if isinstance(workspace, t.Tensor) else None)])
    extras = [x for _, x in named[-b.extras:]]
    setattr(a, first, rows.detach())
    if grads:
        return function().apply(rows, a, *extras)
    loss, stats = _forward(t, b, a, extras, workspace, loss, stats)
    return (loss, stats) if out is None else out
