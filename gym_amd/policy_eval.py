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
from ._policy_args import MAX_ACTION_DIM, MAX_ACTIONS, STRAIGHT_LINE_ACTIONS      # noqa: F401  (the heads' limits: part of this module's surface)
from ._policy_args import _check as _raise
from ._policy_args import _ld, _log_std, _log_std_ld, _one_device, _ptr, _rows, _vector

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
    _raise(rc, lib.mxv_policy_eval_last_error)


def _outputs(t, out, lead, grads):
    """out=(log_prob, entropy), each a contiguous float32 tensor of the leading shape or None (not computed)."""
    if grads:
        raise ValueError("out= cannot be used when an input requires grad: autograd owns the outputs")
    out = tuple(out)
    if len(out) != 2:
        raise ValueError(f"out must hold 2 entries (log_prob, entropy), got {len(out)}")
    return tuple(None if o is None else _vector(t, o, f"out ({n})", lead, (t.float32,)) for o, n in zip(out, ("log_prob", "entropy")))


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
                                            _log_std_ld(ls, D), act2.data_ptr(), _ld(act2, D), _ptr(lp), _ptr(en)))


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
                                                             ls.data_ptr(), _log_std_ld(ls, D), act2.data_ptr(), _ld(act2, D),
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
    _one_device((("logits", x2), ("actions", act), ("out (log_prob)", lp), ("out (entropy)", en)))
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
    ls, _ = _log_std(t, log_std, mean)
    act2 = _rows(t, actions, "actions", MAX_ACTION_DIM, f"{tuple(mean.shape)}")
    if tuple(actions.shape) != tuple(mean.shape):
        raise ValueError(f"actions must have shape {tuple(mean.shape)}, got {tuple(actions.shape)}")
    if actions.requires_grad:
        raise ValueError("actions must not require grad: stored actions are data, the gradients are those of mean and log_std")
    grads = t.is_grad_enabled() and (mean.requires_grad or log_std.requires_grad)
    lp = en = None
    if out is not None:
        lp, en = _outputs(t, out, lead, grads)
    _one_device((("mean", mu2), ("log_std", ls), ("actions", act2), ("out (log_prob)", lp), ("out (entropy)", en)))
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
