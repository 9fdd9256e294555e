"""The PPO clipped-surrogate loss of a batch, its diagnostics and its gradients, fused (include/mxv_ppo.h): the last
stage of an update after gym_amd.gae (advantages) and gym_amd.evaluate_* (log pi and entropy of the stored actions).

    moments     = gym_amd.advantage_moments(advantages)                       # float64 [2] on the device: (mean, 1 / (std + eps))
    loss, stats = gym_amd.ppo_clip_loss(log_prob, old_log_prob, advantages, clip=0.2, moments=moments,
                                        entropy=entropy, entropy_coef=0.01, values=values, returns=returns, value_coef=0.5)
    loss.backward()                                                           # one backward launch, then evaluate_*'s and the head's own

The arithmetic is float64 in a fixed order, every sum a fixed tree over the row index: bit-equal to tests/ppo_host.py, a function of
the inputs and their positions.  `stats` is one device vector of the diagnostics (POLICY_LOSS .. RATIO_MAX index it), read when the
caller chooses.  The loss is a torch.autograd.Function that saves only its inputs — the backward recomputes the rows and reads the
incoming gradient from device memory.  Everything launches on the caller's current stream without a synchronisation; `moments` is read
on the device, so the two calls need none in between.  The header is optional (mxv.h does not include it), so its symbols are bound
here, over the same library as gym_amd._native, and are not part of _native.EXPORTS.  Importing this module does not import torch.
"""
from __future__ import annotations

import ctypes as C

from . import _native
from ._policy_args import LEAF_ROWS       # rows per leaf of the sum tree, and leaves per group of a level
from ._policy_args import _one_device, _ptr, _vector
from ._value_loss import Bound, _outputs
from ._trajectory_args import _scalar

PPO_EXPORTS = ("mxv_ppo_workspace_bytes", "mxv_ppo_advantage_moments", "mxv_ppo_clip_loss", "mxv_ppo_clip_loss_backward", "mxv_ppo_last_error")
# indices into stats (MXV_PPO_* of the header)
POLICY_LOSS, VALUE_LOSS, ENTROPY, APPROX_KL, APPROX_KL3, CLIP_FRACTION, RATIO_MIN, RATIO_MAX = range(8)
STATS = 8
STAT_NAMES = ("policy_loss", "value_loss", "entropy", "approx_kl", "approx_kl3", "clip_fraction", "ratio_min", "ratio_max")

lib = _native.lib
_P, _D, _I64 = C.c_void_p, C.c_double, C.c_int64
_BOUND = Bound(lib, "mxv_ppo", stats=STATS)
_check, workspace_bytes, launches, _workspace = _BOUND.check, _BOUND.workspace_bytes, _BOUND.launches, _BOUND.workspace
lib.mxv_ppo_advantage_moments.argtypes = [_P, _I64, _P, _D, _P, _I64, _P]
lib.mxv_ppo_advantage_moments.restype = C.c_int
lib.mxv_ppo_clip_loss.argtypes = [_P, _I64, _P, _P, _P, _P, _P, _P, _P, _D, _D, _D, _P, _I64, _P, _P]
lib.mxv_ppo_clip_loss.restype = C.c_int
lib.mxv_ppo_clip_loss_backward.argtypes = [_P, _I64, _P, _P, _P, _P, _P, _P, _P, _D, _D, _D, _P, _P, _P, _P]
lib.mxv_ppo_clip_loss_backward.restype = C.c_int


def _no_grad_input(t, x, name):
    if x is not None and t.is_grad_enabled() and x.requires_grad:
        raise ValueError(f"{name} must not require grad: the loss is differentiable with respect to log_prob, entropy and values")


def _limits(clip, entropy_coef, value_coef):
    clip, entropy_coef, value_coef = _scalar("clip", clip), _scalar("entropy_coef", entropy_coef), _scalar("value_coef", value_coef)
    if not 0.0 <= clip < 1.0:
        raise ValueError(f"clip must be in [0, 1), got {clip!r}")
    return clip, entropy_coef, value_coef


def advantage_moments(advantages, *, eps=1e-8, out=None, workspace=None):
    """(mean, 1 / (std + eps)) of `advantages` -> float64 [2] on the device: what ppo_clip_loss(moments=) normalises with, the unbiased
    std as torch.std.

    advantages float32 of any shape, contiguous, on the device.  eps a finite number >= 0.  out: a float64 [2] tensor to write into;
    workspace: as for ppo_clip_loss.  Float64 sums of x and x * x in the fixed tree of the loss, bit-equal to tests/ppo_host.py; one row
    gives a NaN deviation.  2 launches up to 2^20 rows, 3 up to 2^30, on the current stream; no synchronisation."""
    import torch as t

    if not isinstance(advantages, t.Tensor):
        raise ValueError(f"advantages must be a torch tensor, got {type(advantages).__name__}")
    adv = _vector(t, advantages, "advantages", advantages.shape, (t.float32,))
    M = adv.shape[0]
    if M < 1:
        raise ValueError(f"advantages must have at least one element, got shape {tuple(advantages.shape)}")
    eps = _scalar("eps", eps)
    if eps < 0.0:
        raise ValueError(f"eps must not be negative, got {eps!r}")
    mom = None if out is None else _vector(t, out, "out", (2,), (t.float64,))
    dev = _one_device((("advantages", adv), ("out", mom), ("workspace", workspace if isinstance(workspace, t.Tensor) else None)))
    ws, ws_bytes = _workspace(t, workspace, M, dev)
    if mom is None:
        mom = t.empty(2, dtype=t.float64, device=dev)
    with t.cuda.device(dev):
        _check(lib.mxv_ppo_advantage_moments(t.cuda.current_stream(dev).cuda_stream, M, adv.detach().data_ptr(), eps, ws.data_ptr(), ws_bytes,
                                             mom.data_ptr()))
    return mom if out is None else out


def _forward(t, M, lp, old, adv, mom, en, val, ret, clip, ecoef, vcoef, ws, ws_bytes, loss, stats):
    dev = lp.device
    with t.cuda.device(dev):
        _check(lib.mxv_ppo_clip_loss(t.cuda.current_stream(dev).cuda_stream, M, lp.data_ptr(), old.data_ptr(), adv.data_ptr(), _ptr(mom), _ptr(en),
                                     _ptr(val), _ptr(ret), clip, ecoef, vcoef, ws.data_ptr(), ws_bytes, loss.data_ptr(), stats.data_ptr()))


_FUNCTION = None


def _function():
    """The torch.autograd.Function, made at the first differentiable call: importing this module does not import torch."""
    global _FUNCTION
    if _FUNCTION is not None:
        return _FUNCTION
    import torch as t
    from torch.autograd.function import once_differentiable

    class PpoClipLoss(t.autograd.Function):
        @staticmethod
        def forward(ctx, lp, old, adv, mom, en, val, ret, clip, ecoef, vcoef):
            ctx.set_materialize_grads(False)
            M, dev = lp.shape[0], lp.device
            loss = t.empty((), dtype=t.float32, device=dev)
            stats = t.empty(STATS, dtype=t.float32, device=dev)
            ws, ws_bytes = _workspace(t, None, M, dev)
            _forward(t, M, lp, old, adv, mom, en, val, ret, clip, ecoef, vcoef, ws, ws_bytes, loss, stats)
            ctx.save_for_backward(lp, old, adv, mom, en, val, ret)      # the inputs alone: the backward recomputes the rows
            ctx.scalars = (clip, ecoef, vcoef)
            ctx.mark_non_differentiable(stats)
            return loss, stats

        @staticmethod
        @once_differentiable
        def backward(ctx, g_loss, _g_stats):
            need_lp, need_en, need_val = ctx.needs_input_grad[0], ctx.needs_input_grad[4], ctx.needs_input_grad[5]
            none = (None,) * 10
            if g_loss is None or not (need_lp or need_en or need_val):
                return none
            lp, old, adv, mom, en, val, ret = ctx.saved_tensors
            clip, ecoef, vcoef = ctx.scalars
            M, dev = lp.shape[0], lp.device
            g = g_loss.contiguous()      # one float32 in device memory: read by the kernel, never by the host
            g_lp, g_en, g_val = (t.empty(M, dtype=t.float32, device=dev) if need else None for need in (need_lp, need_en, need_val))
            with t.cuda.device(dev):
                _check(lib.mxv_ppo_clip_loss_backward(t.cuda.current_stream(dev).cuda_stream, M, lp.data_ptr(), old.data_ptr(), adv.data_ptr(),
                                                      _ptr(mom), _ptr(en), _ptr(val), _ptr(ret), clip, ecoef, vcoef, g.data_ptr(), _ptr(g_lp),
                                                      _ptr(g_en), _ptr(g_val)))
            return (g_lp, None, None, None, g_en, g_val) + none[6:]

    _FUNCTION = PpoClipLoss
    return _FUNCTION


def ppo_clip_loss(log_prob, old_log_prob, advantages, *, clip=0.2, moments=None, entropy=None, entropy_coef=0.0, values=None, returns=None,
                  value_coef=0.5, workspace=None, out=None):
    """The PPO loss -mean(min(r A, clamp(r, 1 - clip, 1 + clip) A)) + value_coef * 0.5 * mean((values - returns)^2)
    - entropy_coef * mean(entropy), r = exp(log_prob - old_log_prob), and its diagnostics -> (loss, stats).

    log_prob, old_log_prob, advantages and, where given, entropy, values, returns: float32 device tensors of one shape, contiguous.
    entropy may be None (no entropy term); values and returns are both given or both None (no value term).  moments: the float64 [2]
    tensor of advantage_moments(advantages) — A = (advantages - mean) * inv, read on the device — or None: the advantages as given.
    clip in [0, 1); entropy_coef and value_coef finite numbers.

    loss is a 0-dim float32 tensor, differentiable with respect to log_prob, entropy and values (whichever require grad); stats is
    float32 [8], not differentiable: policy_loss, value_loss, entropy, approx_kl (mean of old - new), approx_kl3 (mean of (r - 1) - d),
    clip_fraction, ratio_min, ratio_max — POLICY_LOSS .. RATIO_MAX of this module.  A NaN in a row makes the loss NaN and that row's
    gradient NaN; the extrema skip it.  out=(loss, stats) and workspace= (a 1-D uint8 or float64 tensor of workspace_bytes(rows) bytes)
    are accepted only when no input requires grad; with both the call allocates nothing.  Float64 arithmetic in a fixed order and
    fixed sum trees, bit-equal to tests/ppo_host.py.  2 launches up to 2^20 rows, 3 up to 2^30, and one for the backward, on the
    current stream; no synchronisation."""
    import torch as t

    if not isinstance(log_prob, t.Tensor):
        raise ValueError(f"log_prob must be a torch tensor, got {type(log_prob).__name__}")
    lead = log_prob.shape
    f32 = (t.float32,)
    lp = _vector(t, log_prob, "log_prob", lead, f32)
    M = lp.shape[0]
    if M < 1:
        raise ValueError(f"log_prob must have at least one element, got shape {tuple(lead)}")
    old = _vector(t, old_log_prob, "old_log_prob", lead, f32)
    adv = _vector(t, advantages, "advantages", lead, f32)
    en = None if entropy is None else _vector(t, entropy, "entropy", lead, f32)
    if (values is None) != (returns is None):
        raise ValueError("values and returns must both be given or both be None")
    val = None if values is None else _vector(t, values, "values", lead, f32)
    ret = None if returns is None else _vector(t, returns, "returns", lead, f32)
    mom = None if moments is None else _vector(t, moments, "moments", (2,), (t.float64,))
    clip, entropy_coef, value_coef = _limits(clip, entropy_coef, value_coef)
    for x, name in ((old_log_prob, "old_log_prob"), (advantages, "advantages"), (returns, "returns"), (moments, "moments")):
        _no_grad_input(t, x, name)
    grads = t.is_grad_enabled() and any(x is not None and x.requires_grad for x in (log_prob, entropy, values))
    out, loss, stats = _outputs(t, out, workspace, grads, "an input", STATS)
    dev = _one_device((("log_prob", lp), ("old_log_prob", old), ("advantages", adv), ("moments", mom), ("entropy", en), ("values", val),
                       ("returns", ret), ("out (loss)", loss), ("out (stats)", stats),
                       ("workspace", workspace if isinstance(workspace, t.Tensor) else None)))
    if grads:
        return _function().apply(lp, old, adv, mom, en, val, ret, clip, entropy_coef, value_coef)
    ws, ws_bytes = _workspace(t, workspace, M, dev)
    if out is None:
        loss = t.empty((), dtype=t.float32, device=dev)
        stats = t.empty(STATS, dtype=t.float32, device=dev)
    _forward(t, M, lp.detach(), old, adv, mom, None if en is None else en.detach(), None if val is None else val.detach(), ret, clip,
             entropy_coef, value_coef, ws, ws_bytes, loss, stats)
    return out if out is not None else (loss, stats)
