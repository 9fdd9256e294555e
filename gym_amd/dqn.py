"""The Q-learning loss of a batch, its diagnostics and its gradient, fused (include/mxv_dqn.h): TD targets, the Huber loss
of the TD errors, and the dense gradient with respect to q — the value-based counterpart of gym_amd.ppo_clip_loss.

    returns     = gym_amd.gae(reward, terminated, truncated, values=q_max, ...)[1]           # Peng's Q(lambda) targets: values = max_a Q
    loss, stats = gym_amd.dqn_loss(q, actions, targets=returns)                                # or the one-step bootstrap:
    loss, stats = gym_amd.dqn_loss(q, actions, reward=r, terminated=term, next_q=q_target, next_q_online=q_next, gamma=0.99)
    loss.backward()                                                                            # one launch: d loss / d q, dense [M, A]

The arithmetic is float64 in a fixed order, every sum a fixed tree over the row index: bit-equal to tests/dqn_host.py, a function of
the inputs and their positions.  `stats` is one device vector of the diagnostics (LOSS_TERM .. Q_TAKEN_MAX index it), read when the
caller chooses.  The loss is a torch.autograd.Function that saves only its inputs — the backward recomputes the rows and reads the
incoming gradient from device memory.  Everything launches on the caller's current stream without a synchronisation.  The header is
optional (mxv.h does not include it), so its symbols are bound here, over the same library as gym_amd._native, and are not part of
_native.EXPORTS.  Importing this module does not import torch.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _native
from ._policy_args import LEAF_ROWS       # rows per leaf of the sum tree, and leaves per group of a level
from ._policy_args import MAX_ACTIONS, _ld, _ptr, _rows, _vector
from ._value_loss import Bound, _finish, _make_function, _target_mode
from ._value_loss import _no_grad_input      # noqa: F401  (gym_amd.c51 and gym_amd.qr took it from here)
from .returns import _scalar

DQN_EXPORTS = ("mxv_dqn_workspace_bytes", "mxv_dqn_loss", "mxv_dqn_loss_backward", "mxv_dqn_last_error")
# indices into stats (MXV_DQN_* of the header)
LOSS_TERM, TD_ABS_MEAN, Q_TAKEN_MEAN, TARGET_MEAN, LINEAR_FRACTION, TD_ABS_MAX, Q_TAKEN_MIN, Q_TAKEN_MAX = range(8)
STATS = 8
STAT_NAMES = ("loss_term", "td_abs_mean", "q_taken_mean", "target_mean", "linear_fraction", "td_abs_max", "q_taken_min", "q_taken_max")

lib = _native.lib
_P, _D, _I64, _I32 = C.c_void_p, C.c_double, C.c_int64, C.c_int32
_INPUTS = [_P, _I64, _I32, _P, _I64, _P, _I32, _P, _P, _P, _P, _I64, _P, _I64, _D, _D, _P]      # stream .. weights
_BOUND = Bound(lib, "mxv_dqn", _INPUTS, [_P, _I64, _P, _P, _P], stats=STATS)      # the workspace, its bytes, td_error, loss, stats
_check, workspace_bytes, launches, _workspace = _BOUND.check, _BOUND.workspace_bytes, _BOUND.launches, _BOUND.workspace


def _delta(delta):
    """A finite number above 0, or math.inf: the plain half squared error."""
    if not isinstance(delta, (bool, str, bytes)):
        try:
            if float(delta) == math.inf:
                return math.inf
        except (TypeError, ValueError):
            pass
    d = _scalar("delta", delta)
    if not d > 0.0:
        raise ValueError(f"delta must be above 0 (math.inf: the half squared error), got {delta!r}")
    return d


class _Inputs:
    """The checked inputs of one call, as the C entry points take them."""

    TENSORS = ("q", "act", "targets", "reward", "term", "next", "online", "weights")
    SCALARS = ("M", "A", "gamma", "delta", "dev")

    def call_args(self, t):
        s = self
        return (t.cuda.current_stream(s.dev).cuda_stream, s.M, s.A, s.q.data_ptr(), _ld(s.q, s.A), s.act.data_ptr(), s.act.element_size(),
                _ptr(s.targets), _ptr(s.reward), _ptr(s.term), _ptr(s.next), 0 if s.next is None else _ld(s.next, s.A), _ptr(s.online),
                0 if s.online is None else _ld(s.online, s.A), s.gamma, s.delta, _ptr(s.weights))

    def grad_shape(self):
        return self.M, self.A


_FUNCTION = None


def _function():
    """The torch.autograd.Function, made at the first differentiable call: importing this module does not import torch."""
    global _FUNCTION
    if _FUNCTION is None:
        _FUNCTION = _make_function("DqnLoss", _Inputs, _BOUND)
    return _FUNCTION


def dqn_loss(q, actions, *, targets=None, reward=None, terminated=None, next_q=None, next_q_online=None, gamma=0.99, delta=1.0, weights=None,
             td_error=None, workspace=None, out=None):
    """The Q-learning loss mean(weights * huber(q[i, actions[i]] - y[i], delta)) and its diagnostics -> (loss, stats).

    q float32 [M, A] (rows may be strided views into a wider buffer) or [..., A] with any leading dims that view(-1, A) accepts,
    1 <= A <= 64, on the device; actions int64 or int32 of the leading shape, contiguous.  Exactly one target mode:
      * targets= float32 of the leading shape: y precomputed — Peng's Q(lambda) from gym_amd.gae(..., values=max_a Q)[1], or n-step;
      * reward float32, terminated bool or uint8 (both of the leading shape) and next_q float32 of q's shape (strided rows allowed): the
        target network at the next observation, y = terminated ? reward : reward + gamma * max_a next_q.  With next_q_online (the online
        network at the next observation) the maximising action is next_q_online's and next_q evaluates it: double DQN.  Ties take the
        first action; a NaN anywhere in the selecting row makes y NaN; a terminated row ignores next_q entirely.
    There is no `truncated` argument on purpose: at a truncated step the caller evaluates next_q on the final observation (final_obs),
    which is how final_values of gym_amd.gae already works, and leaves terminated unset.
    delta: a finite number > 0, or math.inf for the plain half squared error (ae == delta is on the quadratic side, as torch's
    huber_loss).  weights: float32 of the leading shape or None — importance weights of the rows; the mean still divides by M.
    td_error: a float32 tensor of the leading shape to receive the signed q[i, a_i] - y[i], or None.  Only q may require grad.

    loss is a 0-dim float32 tensor, differentiable with respect to q: the gradient is dense [M, A] — zero outside the taken column, NaN
    in the taken column of a NaN row, NaN in all A columns of a row whose action is outside 0..A-1.  stats is float32 [8], not
    differentiable: loss_term (the loss again), td_abs_mean, q_taken_mean, target_mean, linear_fraction, td_abs_max, q_taken_min,
    q_taken_max — LOSS_TERM .. Q_TAKEN_MAX of this module; the extrema skip NaN rows.  out=(loss, stats) and workspace= (a 1-D uint8 or
    float64 tensor of workspace_bytes(rows) bytes) are accepted only when q does not require grad; with both the call allocates
    nothing.  Float64 arithmetic in a fixed order and fixed sum trees, bit-equal to tests/dqn_host.py.  2 launches up to 2^20 rows, 3
    up to 2^30, and one for the backward, on the current stream; no synchronisation."""
    import torch as t

    f32 = (t.float32,)
    what = f"[..., A] with at least one row and 1 <= A <= {MAX_ACTIONS}"
    a = _Inputs()
    a.q = _rows(t, q, "q", MAX_ACTIONS, what)
    lead = q.shape[:-1]
    a.M, a.A = a.q.shape
    a.act = _vector(t, actions, "actions", lead, (t.int64, t.int32))
    a.reward, a.term, a.next, a.online = _target_mode(t, _rows, lead, ("q", q), ("targets", targets),
                                                      {"reward": reward, "terminated": terminated, "next_q": next_q},
                                                      ("next_q_online", next_q_online), rows_args=(MAX_ACTIONS, what))
    a.targets = None if targets is None else _vector(t, targets, "targets", lead, f32)
    a.weights = None if weights is None else _vector(t, weights, "weights", lead, f32)
    a.gamma, a.delta = _scalar("gamma", gamma), _delta(delta)
    td = None if td_error is None else _vector(t, td_error, "td_error", lead, f32)
    return _finish(t, _BOUND, _function, a, [("q", a.q), ("actions", a.act), ("targets", a.targets), ("reward", a.reward), ("terminated", a.term),
                                             ("next_q", a.next), ("next_q_online", a.online), ("weights", a.weights), ("td_error", td)], workspace, out)
