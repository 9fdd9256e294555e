"""The quantile-regression (QR-DQN) Q-learning loss of a batch, its diagnostics and its gradient, fused (include/mxv_qr.h):
the target quantiles (given, or the bootstrap of DQN / double DQN with a scalar gamma or a per-row discount), the quantile Huber loss of
the taken action's quantiles against them, and the dense gradient with respect to the quantiles — the third value-based loss beside
gym_amd.dqn_loss and gym_amd.categorical_dqn_loss, and the one that takes what the n-step rings emit as it is.

    batch       = buffer.sample(256)                                                           # gym_amd.NStepPrioritizedReplayBuffer
    loss, stats = gym_amd.quantile_dqn_loss(quantiles, batch["actions"], reward=batch["reward"], terminated=batch["terminated"],
                                            next_quantiles=target_net, next_quantiles_online=online_net, discount=batch["discount"],
                                            weights=batch["weights"], row_loss=row_loss)
    loss.backward()                                                                            # one launch: d loss / d quantiles, dense [M, A, N]
    buffer.update_priorities(batch["indices"], row_loss)
    q           = gym_amd.quantile_q_values(quantiles)                                         # [..., A]: what the agent acts greedily on

The arithmetic is float64 in a fixed order, every sum a fixed tree: bit-equal to tests/qr_host.py, a function of the inputs and their
positions.  `stats` is one device vector of the diagnostics (LOSS_TERM .. Q_TAKEN_MAX index it), read when the caller chooses.  The
loss is a torch.autograd.Function that saves only its inputs — the backward recomputes the rows and reads the incoming gradient from
device memory.  Everything launches on the caller's current stream without a synchronisation.  The header is optional (mxv.h does not
include it), so its symbols are bound here, over the same library as gym_amd._native, and are not part of _native.EXPORTS.  Importing
this module does not import torch.
"""
from __future__ import annotations

import ctypes as C

from . import _native
from ._policy_args import LEAF_ROWS       # rows per leaf of the sum tree, and leaves per group of a level (kLeafRows, kTreeFan)
from ._policy_args import _one_device, _ptr, _vector
from ._value_loss import Bound, _finish, _heads_checker, _ld3, _make_function, _no_grad_input, _target_mode
from .returns import _scalar

QR_EXPORTS = ("mxv_qr_workspace_bytes", "mxv_qr_loss", "mxv_qr_loss_backward", "mxv_qr_q_values", "mxv_qr_last_error")
# indices into stats (MXV_QR_* of the header)
LOSS_TERM, Q_TAKEN_MEAN, TARGET_MEAN, TD_ABS_MEAN, CROSSING_FRACTION, ROW_LOSS_MAX, Q_TAKEN_MIN, Q_TAKEN_MAX = range(8)
STATS = 8
STAT_NAMES = ("loss_term", "q_taken_mean", "target_mean", "td_abs_mean", "crossing_fraction", "row_loss_max", "q_taken_min", "q_taken_max")
MAX_QUANTILES = 64
# the launch shape (gym_amd/csrc/mxv_qr.hip, mxv_policy_rule.hpp; LEAF_ROWS above: mxv_sum_tree.hpp)
TILE_ROWS = 4           # rows (loss, backward) or (row, action) pairs (quantile_q_values) per workgroup: one per wave (kWaves)
GRID_X = 1 << 16        # tiles along x of the grid of the rows and the backward kernels: beyond, the grid grows along y (kGridX)
MAX_BLOCKS = 2048       # workgroups of quantile_q_values, which stride over its tiles (kMaxBlocks)

lib = _native.lib
_P, _D, _I64, _I32 = C.c_void_p, C.c_double, C.c_int64, C.c_int32
_INPUTS = [_P, _I64, _I32, _I32, _P, _I64, _P, _I32, _P, _P, _P, _P, _I64, _P, _I64, _D, _P, _D, _P]      # stream .. weights
_BOUND = Bound(lib, "mxv_qr", _INPUTS, [_P, _I64, _P, _P, _P, _P], leaf_finishes=True, stats=STATS)      # .. row_loss, targets_out, loss, stats
_check, workspace_bytes, launches, _workspace = _BOUND.check, _BOUND.workspace_bytes, _BOUND.launches, _BOUND.workspace
lib.mxv_qr_q_values.argtypes = [_P, _I64, _I32, _I32, _P, _I64, _P]
lib.mxv_qr_q_values.restype = C.c_int


_heads = _heads_checker("N", 1, MAX_QUANTILES, "quantiles")      # _heads(t, x, name): a float32 [..., A, N] tensor as its [M, A, N] rows


def _kappa(kappa):
    k = _scalar("kappa", kappa)
    if not k > 0.0:
        raise ValueError(f"kappa must be above 0, got {kappa!r} (kappa = 0, the plain quantile loss, is not built)")
    return k


class _Inputs:
    """The checked inputs of one call, as the C entry points take them."""

    TENSORS = ("quantiles", "act", "target_quantiles", "reward", "term", "next", "online", "discount", "weights")
    SCALARS = ("M", "A", "N", "gamma", "kappa", "dev")

    def call_args(self, t):
        s = self
        return (t.cuda.current_stream(s.dev).cuda_stream, s.M, s.A, s.N, s.quantiles.data_ptr(), _ld3(s.quantiles), s.act.data_ptr(),
                s.act.element_size(), _ptr(s.target_quantiles), _ptr(s.reward), _ptr(s.term), _ptr(s.next), 0 if s.next is None else _ld3(s.next),
                _ptr(s.online), 0 if s.online is None else _ld3(s.online), s.gamma, _ptr(s.discount), s.kappa, _ptr(s.weights))

    def grad_shape(self):
        return self.M, self.A, self.N


_FUNCTION = None


def _function():
    """The torch.autograd.Function, made at the first differentiable call: importing this module does not import torch."""
    global _FUNCTION
    if _FUNCTION is None:
        _FUNCTION = _make_function("QuantileDqnLoss", _Inputs, _BOUND)
    return _FUNCTION


def quantile_dqn_loss(quantiles, actions, *, target_quantiles=None, reward=None, terminated=None, next_quantiles=None,
                      next_quantiles_online=None, gamma=None, discount=None, kappa=1.0, weights=None, row_loss=None, targets_out=None,
                      workspace=None, out=None):
    """The quantile-regression loss mean(weights * sum_k mean_j rho_kappa^tau_k(T[i, j] - quantiles[i, actions[i], k])) and its
    diagnostics -> (loss, stats).

    quantiles float32 [M, A, N] (the last two dims contiguous; rows may be strided views into a wider buffer) or [..., A, N] with any
    leading dims that view(-1, A, N) accepts, 1 <= A <= 64 actions, 1 <= N <= 64 quantiles at the midpoints tau_k = (2k + 1) / (2N)
    (N > 64 is out of scope: a quantile is a lane of one wave), on the device; actions int64 or int32 of the leading shape, contiguous.
    No support bounds: a quantile head places its own atoms.  Exactly one target mode:
      * target_quantiles= float32 [..., N]: the target quantiles T, built by the caller;
      * reward float32, terminated bool or uint8 (both of the leading shape) and next_quantiles float32 of quantiles' shape (strided
        rows allowed): the target network at the next observation.  The next action is the first maximum of the mean quantile of
        next_quantiles — of next_quantiles_online (the online network at the next observation) if given: double DQN — and
        T = reward + g * next_quantiles[j*], with g the scalar gamma= (0.99 when neither is passed) or the per-row discount= (float32
        of the leading shape: gamma^(steps taken), what NStepReplayBuffer.sample and NStepPrioritizedReplayBuffer.sample return as
        "discount"); passing both raises.  A terminated row's targets are its reward and it ignores both next tensors and the
        discount entirely; a NaN mean in the selecting row makes T NaN.
    There is no `truncated` argument on purpose: at a truncated step the caller evaluates next_quantiles on the final observation
    (final_obs) and leaves terminated unset, as with gym_amd.dqn_loss.
    kappa: the Huber threshold, finite and above 0 (kappa = 0 is not built).  weights: float32 of the leading shape or None —
    importance weights of the rows; the mean still divides by M.  row_loss: a float32 tensor of the leading shape to receive the
    unweighted loss of each row (>= 0; what goes to update_priorities), or None.  targets_out: a float32 [..., N] tensor to receive
    the T the kernel used, or None.  Only quantiles may require grad.

    loss is a 0-dim float32 tensor, differentiable with respect to quantiles: the gradient is dense [M, A, N] — zero outside the taken
    action, NaN in the taken action's N columns of a NaN row, NaN in all A * N elements of a row whose action is outside 0..A-1.  stats
    is float32 [8], not differentiable: loss_term (the loss again), q_taken_mean, target_mean, td_abs_mean (|mean quantile of the
    taken action - mean target|), crossing_fraction (the share of adjacent quantile pairs of the taken action that are out of order:
    it tells a head that has not learned its ordering), row_loss_max, q_taken_min, q_taken_max — LOSS_TERM .. Q_TAKEN_MAX of this
    module; the extrema skip NaN rows.  out=(loss, stats) and workspace= (a 1-D uint8 or float64 tensor of workspace_bytes(rows) bytes)
    are accepted only when quantiles does not require grad; with both the call allocates nothing.  Float64 arithmetic in a fixed order
    and fixed sum trees, bit-equal to tests/qr_host.py.  2 launches up to 1024 rows, 3 up to 2^20, 4 up to 2^30, and one for the
    backward, on the current stream; no synchronisation."""
    import torch as t

    f32 = (t.float32,)
    a = _Inputs()
    a.quantiles = _heads(t, quantiles, "quantiles")
    lead = quantiles.shape[:-2]
    a.M, a.A, a.N = a.quantiles.shape
    a.act = _vector(t, actions, "actions", lead, (t.int64, t.int32))
    if gamma is not None and discount is not None:
        raise ValueError("gamma and discount are both given: the bootstrap takes the scalar or the per-row one")
    a.reward, a.term, a.next, a.online = _target_mode(t, _heads, lead, ("quantiles", quantiles), ("target_quantiles", target_quantiles),
                                                      {"reward": reward, "terminated": terminated, "next_quantiles": next_quantiles},
                                                      ("next_quantiles_online", next_quantiles_online), (("discount", discount),))
    a.target_quantiles = None if target_quantiles is None else _vector(t, target_quantiles, "target_quantiles", tuple(lead) + (a.N,), f32)
    a.discount = None if discount is None else _vector(t, discount, "discount", lead, f32)
    a.weights = None if weights is None else _vector(t, weights, "weights", lead, f32)
    a.gamma = 0.0 if discount is not None else _scalar("gamma", 0.99 if gamma is None else gamma)      # not read beside a discount
    a.kappa = _kappa(kappa)
    rl = None if row_loss is None else _vector(t, row_loss, "row_loss", lead, f32)
    to = None if targets_out is None else _vector(t, targets_out, "targets_out", tuple(lead) + (a.N,), f32)
    return _finish(t, _BOUND, _function, a, [("quantiles", a.quantiles), ("actions", a.act), ("target_quantiles", a.target_quantiles),
                                             ("reward", a.reward), ("terminated", a.term), ("next_quantiles", a.next),
                                             ("next_quantiles_online", a.online), ("discount", a.discount), ("weights", a.weights),
                                             ("row_loss", rl), ("targets_out", to)], workspace, out)


def quantile_q_values(quantiles, out=None):
    """The expected action values of a quantile head: float32 [..., A] = the mean of quantiles[..., a, :], in one launch.

    quantiles float32 [..., A, N] as quantile_dqn_loss takes them (1 <= A <= 64, 1 <= N <= 64).  The values are the Q_a of the loss's
    selecting pass, computed by the same lines: the action an agent takes greedily from them (the first maximum) is the j* the loss
    selects.  out= a float32 tensor of the leading shape + (A,), contiguous; without it one is allocated.  Not differentiable.  On the
    current stream; no synchronisation."""
    import torch as t

    x3 = _heads(t, quantiles, "quantiles").detach()
    M, A, N = x3.shape
    shape = tuple(quantiles.shape[:-1])
    if out is None:
        _one_device((("quantiles", x3),))
        out = t.empty(shape, dtype=t.float32, device=x3.device)
        q = out.view(-1)
    else:
        q = _vector(t, out, "out", shape, (t.float32,))
        _no_grad_input(t, out, "out")
        _one_device((("quantiles", x3), ("out", q)))
    with t.cuda.device(x3.device):
        _check(lib.mxv_qr_q_values(t.cuda.current_stream(x3.device).cuda_stream, M, A, N, x3.data_ptr(), _ld3(x3), q.data_ptr()))
    return out
