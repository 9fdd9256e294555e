"""Stored actions re-evaluated under the current policy head, differentiably (include/mxv_policy_eval.h): log pi(action)
and the entropy of every row in one launch, and their gradients with respect to the head's outputs in one more — the update half of
what gym_amd.policy samples.

    log_prob, entropy = gym_amd.evaluate_categorical(logits, actions)            # logits [..., A], actions [...]
    log_prob, entropy = gym_amd.evaluate_gaussian(mean, log_std, actions)        # mean, actions [..., D]; log_std [..., D] or [D]
    loss.backward()                                                              # one backward launch, then the head's own backward

The arithmetic is float64 in a fixed order, bit-equal to tests/policy_eval_host.py, and its forward lines are the samplers': evaluated
on the logits (mean, log_std) and the actions of one sample_categorical (sample_gaussian) call, log_prob and entropy have that call's
bits, so the probability ratio of a learner that has not moved yet is exactly 1.  Each is a torch.autograd.Function that saves only
its inputs — the backward recomputes the row — and launches on the caller's current stream without a synchronisation: recordable into
a torch.cuda.graph.  The header is optional (mxv.h does not include it), so its symbols are bound here, over the same library as
gym_amd._native, and are not part of _native.EXPORTS.  Importing this module does not import torch.
"""
from __future__ import annotations

import ctypes as C

from . import _native
from .policy import MAX_ACTION_DIM, MAX_ACTIONS, STRAIGHT_LINE_ACTIONS      # the samplers' limits and register-resident action counts

EVAL_EXPORTS = ("mxv_policy_eval_categorical", "mxv_policy_eval_categorical_backward", "mxv_policy_eval_gaussian",
                "mxv_policy_eval_gaussian_backward", "mxv_policy_eval_last_error")

lib = _native.lib
lib.mxv_policy_eval_categorical.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
lib.mxv_policy_eval_categorical.restype = C.c_int
lib.mxv_policy_eval_categorical_backward.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_int64]
lib.mxv_policy_eval_categorical_backward.restype = C.c_int
lib.mxv_policy_eval_gaussian.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_void_p]
lib.mxv_policy_eval_gaussian.restype = C.c_int
lib.mxv_policy_eval_gaussian_backward.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
lib.mxv_policy_eval_gaussian_backward.restype = C.c_int
lib.mxv_policy_eval_last_error.argtypes = []
lib.mxv_policy_eval_last_error.restype = C.c_char_p


def _check(rc: int):
    if rc == _native.OK:
        return
    msg = lib.mxv_policy_eval_last_error().decode()
    if rc == _native.ERR_INVALID_ARG:
        raise ValueError(msg)
    raise _native.MxvError(rc, msg)


def _ptr(x):
    return None if x is None else x.data_ptr()


def _rows(t, x, name, max_cols, what):
    """A float32 [..., W] tensor as its [M, W] rows: 2-D tensors may have strided rows (views into wider buffers), more dims must
    flatten without a copy."""
    if not isinstance(x, t.Tensor):
        raise ValueError(f"{name} must be a torch tensor, got {type(x).__name__}")
    if x.dtype != t.float32:
        raise ValueError(f"{name} must be torch.float32, got {x.dtype}")
    if x.dim() < 2 or x.numel() == 0 or not 1 <= x.shape[-1] <= max_cols:
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


def _outputs(t, out, lead, grads):
    """out=(log_prob, entropy), each a contiguous float32 tensor of the leading shape or None (not computed)."""
    if grads:
        raise ValueError("out= cannot be used when an input requires grad: autograd owns the outputs")
    out = tuple(out)
    if len(out) != 2:
        raise ValueError(f"out must hold 2 entries (log_prob, entropy), got {len(out)}")
    return tuple(None if o is None else _vector(t, o, f"out ({n})", lead, (t.float32,)) for o, n in zip(out, ("log_prob", "entropy")))


def _one_device(named, first):
    dev = named[0][1].device
    for name, y in named:
        if y is None:
            continue
        if not y.is_cuda:
            raise ValueError(f"{name} must be a device tensor, got one on {y.device} (gym_amd has no CPU fallback)")
        if y.device != dev:
            raise ValueError(f"{name} is on {y.device}, {first} on {dev}: all tensors must be on one device")
    return dev


def _ld(x2, W):
    return x2.stride(0) if x2.shape[0] > 1 else W


def _cat_forward(t, x2, act, lp, en):
    M, A = x2.shape
    dev = x2.device
    with t.cuda.device(dev):
        _check(lib.mxv_policy_eval_categorical(t.cuda.current_stream(dev).cuda_stream, M, A, x2.data_ptr(), _ld(x2, A), act.data_ptr(),
                                               int(act.dtype == t.int64), _ptr(lp), _ptr(en)))


def _gauss_forward(t, mu2, ls, act2, lp, en):
    M, D = mu2.shape
    dev = mu2.device
    with t.cuda.device(dev):
        _check(lib.mxv_policy_eval_gaussian(t.cuda.current_stream(dev).cuda_stream, M, D, mu2.data_ptr(), _ld(mu2, D), ls.data_ptr(),
                                            0 if ls.dim() == 1 else _ld(ls, D), act2.data_ptr(), _ld(act2, D), _ptr(lp), _ptr(en)))


def _grad_vector(g):
    """An incoming gradient as the kernel reads it: float32, contiguous (autograd hands out expanded views for sums and means)."""
    return None if g is None else g.contiguous()


_FUNCTIONS = None


def _functions():
    """The two torch.autograd.Function classes, made at the first differentiable call: importing this module does not import torch."""
    global _FUNCTIONS
    if _FUNCTIONS is not None:
        return _FUNCTIONS
    import torch as t
    from torch.autograd.function import once_differentiable

    class EvaluateCategorical(t.autograd.Function):
        @staticmethod
        def forward(ctx, x2, act):
            ctx.set_materialize_grads(False)    # an output the loss does not use arrives as None and becomes a NULL pointer
            M = x2.shape[0]
            lp = t.empty(M, dtype=t.float32, device=x2.device)
            en = t.empty(M, dtype=t.float32, device=x2.device)
            _cat_forward(t, x2, act, lp, en)
            ctx.save_for_backward(x2, act)      # the inputs alone: the backward recomputes the row
            return lp, en

        @staticmethod
        @once_differentiable
        def backward(ctx, g_lp, g_en):
            if (g_lp is None and g_en is None) or not ctx.needs_input_grad[0]:
                return None, None
            x2, act = ctx.saved_tensors
            M, A = x2.shape
            dev = x2.device
            g_lp, g_en = _grad_vector(g_lp), _grad_vector(g_en)
            grad = t.empty((M, A), dtype=t.float32, device=dev)
            with t.cuda.device(dev):
                _check(lib.mxv_policy_eval_categorical_backward(t.cuda.current_stream(dev).cuda_stream, M, A, x2.data_ptr(), _ld(x2, A),
                                                                act.data_ptr(), int(act.dtype == t.int64), _ptr(g_lp), _ptr(g_en),
                                                                grad.data_ptr(), A))
            return grad, None

    class EvaluateGaussian(t.autograd.Function):
        @staticmethod
        def forward(ctx, mu2, ls, act2):
            ctx.set_materialize_grads(False)
            M = mu2.shape[0]
            lp = t.empty(M, dtype=t.float32, device=mu2.device)
            en = t.empty(M, dtype=t.float32, device=mu2.device)
            _gauss_forward(t, mu2, ls, act2, lp, en)
            ctx.save_for_backward(mu2, ls, act2)
            return lp, en

        @staticmethod
        @once_differentiable
        def backward(ctx, g_lp, g_en):
            need_mu, need_ls = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            if (g_lp is None and g_en is None) or not (need_mu or need_ls):
                return None, None, None
            mu2, ls, act2 = ctx.saved_tensors
            M, D = mu2.shape
            dev = mu2.device
            g_lp, g_en = _grad_vector(g_lp), _grad_vector(g_en)
            g_mu = t.empty((M, D), dtype=t.float32, device=dev) if need_mu else None
            g_ls = t.empty((M, D), dtype=t.float32, device=dev) if need_ls else None
            with t.cuda.device(dev):
                _check(lib.mxv_policy_eval_gaussian_backward(t.cuda.current_stream(dev).cuda_stream, M, D, mu2.data_ptr(), _ld(mu2, D),
                                                             ls.data_ptr(), 0 if ls.dim() == 1 else _ld(ls, D), act2.data_ptr(), _ld(act2, D),
                                                             _ptr(g_lp), _ptr(g_en), _ptr(g_mu), D, _ptr(g_ls), D))
            if need_ls and ls.dim() == 1:
                g_ls = g_ls.sum(dim=0)      # the shared row's gradient: a torch reduction, outside the bit-defined rule
            return g_mu, g_ls, None

    _FUNCTIONS = (EvaluateCategorical, EvaluateGaussian)
    return _FUNCTIONS


def evaluate_categorical(logits, actions, *, out=None):
    """log pi(actions) and the entropy of every row of `logits` -> (log_prob, entropy), float32 of the leading shape, differentiable
    with respect to logits.

    logits float32 [M, A] (rows may be strided views into a wider buffer) or [..., A] with any leading dims that view(-1, A) accepts,
    1 <= A <= 64, on the device.  actions int64 or int32 of the leading shape, contiguous: the stored actions.  out: (log_prob, entropy)
    to write into, each may be None and is then not computed (None is returned in its place); only when logits does not require grad.
    A row with a NaN, a +inf, nothing but -inf, or an action outside 0..A-1 yields NaN for both (and NaN gradients); -inf masks a logit.
    Float64 arithmetic in a fixed order, bit-equal to tests/policy_eval_host.py; on the logits and actions of one sample_categorical()
    call the results have that call's bits.  One launch on the current stream, and one for the backward; no synchronisation."""
    import torch as t

    x2 = _rows(t, logits, "logits", MAX_ACTIONS, f"[..., A] with at least one row and 1 <= A <= {MAX_ACTIONS}")
    lead = logits.shape[:-1]
    act = _vector(t, actions, "actions", lead, (t.int64, t.int32))
    grads = t.is_grad_enabled() and logits.requires_grad
    lp = en = None
    if out is not None:
        lp, en = _outputs(t, out, lead, grads)
    _one_device((("logits", x2), ("actions", act), ("out (log_prob)", lp), ("out (entropy)", en)), "logits")
    if grads:
        lp, en = _functions()[0].apply(x2, act)
        return lp.view(lead), en.view(lead)
    if out is None:
        lp = t.empty(x2.shape[0], dtype=t.float32, device=x2.device)
        en = t.empty(x2.shape[0], dtype=t.float32, device=x2.device)
    _cat_forward(t, x2.detach(), act, lp, en)
    if out is not None:
        return tuple(out)                       # the caller's own tensors
    return lp.view(lead), en.view(lead)


def evaluate_gaussian(mean, log_std, actions, *, out=None):
    """log pi(actions) and the entropy of every row of a diagonal-Gaussian head -> (log_prob, entropy), float32 of the leading shape,
    differentiable with respect to mean and log_std.

    mean float32 [M, D] (rows may be strided views) or [..., D] with any leading dims that view(-1, D) accepts, 1 <= D <= 4, on the
    device.  log_std of mean's shape, or [D]: one row shared by all rows (a state-independent log_std; its gradient is the per-row
    gradients summed by torch).  actions float32 of mean's shape: the stored actions.  out: (log_prob, entropy) to write into, each may
    be None and is then not computed; only when neither mean nor log_std requires grad.  A row with a non-finite mean or log_std, or
    |log_std| > 80, yields NaN (and NaN gradients).  Float64 arithmetic in a fixed order, bit-equal to tests/policy_eval_host.py; on the
    mean, log_std and actions of one sample_gaussian() call the results have that call's bits.  One launch on the current stream, and
    one for the backward; no synchronisation."""
    import torch as t

    what = f"[..., D] with at least one row and 1 <= D <= {MAX_ACTION_DIM}"
    mu2 = _rows(t, mean, "mean", MAX_ACTION_DIM, what)
    lead, D = mean.shape[:-1], mean.shape[-1]
    if not isinstance(log_std, t.Tensor):
        raise ValueError(f"log_std must be a torch tensor, got {type(log_std).__name__}")
    if log_std.dim() == 1:
        if log_std.dtype != t.float32:
            raise ValueError(f"log_std must be torch.float32, got {log_std.dtype}")
        if log_std.shape[0] != D:
            raise ValueError(f"log_std must have shape {tuple(mean.shape)} or ({D},), got {tuple(log_std.shape)}")
        if D > 1 and log_std.stride(0) != 1:
            raise ValueError(f"log_std must be contiguous in its last dimension (stride {log_std.stride(0)})")
        ls = log_std
    else:
        ls = _rows(t, log_std, "log_std", MAX_ACTION_DIM, f"{tuple(mean.shape)} or ({D},)")
        if tuple(log_std.shape) != tuple(mean.shape):
            raise ValueError(f"log_std must have shape {tuple(mean.shape)} or ({D},), got {tuple(log_std.shape)}")
    act2 = _rows(t, actions, "actions", MAX_ACTION_DIM, f"{tuple(mean.shape)}")
    if tuple(actions.shape) != tuple(mean.shape):
        raise ValueError(f"actions must have shape {tuple(mean.shape)}, got {tuple(actions.shape)}")
    if actions.requires_grad:
        raise ValueError("actions must not require grad: stored actions are data, the gradients are those of mean and log_std")
    grads = t.is_grad_enabled() and (mean.requires_grad or log_std.requires_grad)
    lp = en = None
    if out is not None:
        lp, en = _outputs(t, out, lead, grads)
    _one_device((("mean", mu2), ("log_std", ls), ("actions", act2), ("out (log_prob)", lp), ("out (entropy)", en)), "mean")
    if grads:
        lp, en = _functions()[1].apply(mu2, ls, act2)
        return lp.view(lead), en.view(lead)
    if out is None:
        lp = t.empty(mu2.shape[0], dtype=t.float32, device=mu2.device)
        en = t.empty(mu2.shape[0], dtype=t.float32, device=mu2.device)
    _gauss_forward(t, mu2.detach(), ls.detach(), act2, lp, en)
    if out is not None:
        return tuple(out)                       # the caller's own tensors
    return lp.view(lead), en.view(lead)
