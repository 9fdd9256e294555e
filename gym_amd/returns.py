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

from . import _native
# the two constants are public names of this module; dqn.py, c51.py, qr.py and tests/test_gae_host.py take _scalar from here
from ._trajectory_args import RING_DEPTH, VECTOR_MIN_ENVS, _bind, _prepare, _ptr, _scalar  # noqa: F401

GAE_EXPORTS = ("mxv_gae", "mxv_discounted_returns", "mxv_gae_last_error", "mxv_gae_last_launch")

lib = _native.lib
lib.mxv_gae.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                        C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int64]
lib.mxv_gae.restype = C.c_int
lib.mxv_discounted_returns.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int64]
lib.mxv_discounted_returns.restype = C.c_int
_check, last_launch = _bind(lib, "gae", "gae() / discounted_returns()")


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
    t, ins, lv, outs, ld, ld_out = _prepare([("reward", reward), ("terminated", terminated), ("truncated", truncated), ("values", values)],
                                            last_value, final_values, out, ("advantages", "returns"), bare_out=False)
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
    t, ins, lv, outs, ld, ld_out = _prepare([("reward", reward), ("terminated", terminated), ("truncated", truncated)], last_value,
                                            final_values, out, ("returns",), bare_out=True)
    r = ins["reward"]
    K, N = r.shape
    with t.cuda.device(r.device):
        _check(lib.mxv_discounted_returns(t.cuda.current_stream(r.device).cuda_stream, K, N, r.data_ptr(), int(r.dtype == t.float64), ld,
                                          ins["terminated"].data_ptr(), ins["truncated"].data_ptr(), _ptr(lv),
                                          _ptr(ins.get("final_values")), gamma, outs[0].data_ptr(), ld_out))
    return outs[0]
