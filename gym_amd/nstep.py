"""N-step returns for the replay buffers (include/mxv_nstep.h): gym_amd.ReplayBuffer and gym_amd.PrioritizedReplayBuffer
whose insert walks each row's window of up to n steps inside the insert kernel and stores the discounted return, the window's last
observation and flag, and a per-row discount — what a multi-step Q-learning target needs.

    buf = rollout.nstep_replay_buffer(1 << 20, n_step=3, gamma=0.99)          # or gym_amd.NStepReplayBuffer(capacity, obs_shape, 3, 0.99, ...)
    buf.add_chunk(first_obs, traj)                                             # ONE launch, as the one-step insert
    batch = buf.sample(4096)                                                   # the parent's launches + one: ..., discount
    targets = batch["reward"] + batch["discount"] * (1 - batch["terminated"].float()) * q_target(batch["next_obs"]).max(1).values
    loss, stats = gym_amd.dqn_loss(q(batch["obs"]), batch["actions"], targets=targets)

A window ends after n steps, at an episode end or at the end of the chunk, whichever comes first; `discount` is gamma to the number of
steps the window took, so a window cut short is a correct transition of a shorter horizon and nothing is carried from one chunk to the
next.  At a truncated step the stored next observation is traj["final_obs"] and `terminated` stays 0: the target bootstraps from the
final observation.  Everything is bit-equal to the NumPy twin tests/nstep_host.py and launches on the caller's current stream without a
synchronisation.  The header is optional (mxv.h does not include it), so its symbols are bound here, over the same library as
gym_amd._native, and are not part of _native.EXPORTS.  Importing this module does not import torch.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _native
from ._policy_args import _one_device, _ptr, _vector
from ._policy_args import _check as _raise
from .prioritized import PrioritizedReplayBuffer
from .replay import ReplayBuffer, _count

NSTEP_EXPORTS = ("mxv_nstep_insert", "mxv_nstep_gather", "mxv_nstep_last_error")
NSTEP_MAX = 64               # steps of a window at most (MXV_NSTEP_MAX)

lib = _native.lib
_P, _I64, _I32, _U, _D = C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_double
lib.mxv_nstep_insert.argtypes = [_P, _I64, _I32, _I64, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _I32, _P, _I32, _P, _P, _U, _P, _P, _P, _P, _P, _P,
                                 _I32, _D, _P]
lib.mxv_nstep_insert.restype = C.c_int
lib.mxv_nstep_gather.argtypes = [_P, _I64, _I64, _P, _P, _P]
lib.mxv_nstep_gather.restype = C.c_int
lib.mxv_nstep_last_error.argtypes = []
lib.mxv_nstep_last_error.restype = C.c_char_p


def _check(rc: int):
    _raise(rc, lib.mxv_nstep_last_error)


def _window(n_step, gamma):
    if isinstance(n_step, bool) or not isinstance(n_step, int) or not 1 <= n_step <= NSTEP_MAX:
        raise ValueError(f"n_step must be an integer in 1..{NSTEP_MAX}, got {n_step!r}")
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or math.isnan(gamma) or not 0.0 <= gamma <= 1.0:
        raise ValueError(f"gamma must be a number in [0, 1], got {gamma!r}")
    return n_step, float(gamma)


class NStepReplayBuffer(ReplayBuffer):
    """gym_amd.ReplayBuffer whose rows are n-step transitions: `reward` is the discounted return of the row's window, `next_obs` and
    `terminated` are those of the window's last step, and sample() adds `discount` float32 [B] = gamma^(steps of the window).

    n_step in 1..64 and gamma in [0, 1] are required (they default to None only so that the constructor chain of
    NStepPrioritizedReplayBuffer reaches this class with the values it has already set).  n_step = 1 stores what ReplayBuffer stores,
    and the discount gamma.  The other arguments are ReplayBuffer's."""

    def __init__(self, capacity, obs_shape, n_step=None, gamma=None, obs_dtype=None, action_dtype=None, seed=0, device=None):
        if n_step is None and gamma is None and hasattr(self, "n_step"):
            n_step, gamma = self.n_step, self.gamma
        self.n_step, self.gamma = _window(n_step, gamma)
        super().__init__(capacity, obs_shape, obs_dtype=obs_dtype, action_dtype=action_dtype, seed=seed, device=device)
        t = self._torch
        self._discount = t.zeros(self.capacity, dtype=t.float32, device=self.device)      # zero-filled, as the ring
        t.cuda.current_stream(self.device).synchronize()

    # ---- insert ----
    def _store(self, stream, K, N, first, first_ld, obs, obs_ld, final, final_ld, actions, reward, reward_bytes, terminated, truncated):
        _check(lib.mxv_nstep_insert(stream, self.capacity, self.W, K, N, first, first_ld, obs, obs_ld, final, final_ld, actions,
                                    self._action_bytes, reward, reward_bytes, terminated, truncated, self._count, _ptr(self._state),
                                    self._obs.data_ptr(), self._next.data_ptr(), self._action.data_ptr(), self._reward.data_ptr(),
                                    self._term.data_ptr(), self.n_step, self.gamma, self._discount.data_ptr()))

    # ---- sample ----
    def sample_buffers(self, batch_size):
        """The tensors sample(batch_size, out=...) fills, as a dict: the parent's and "discount" float32 [batch_size]."""
        out = super().sample_buffers(batch_size)
        out["discount"] = self._torch.empty(batch_size, dtype=self._torch.float32, device=self.device)
        return out

    def _gather_discount(self, B, out):
        t = self._torch
        idx = _vector(t, out["indices"], 'out["indices"]', (B,), (t.int64,))
        disc = _vector(t, out["discount"], 'out["discount"]', (B,), (t.float32,))
        dev = _one_device((("the buffer", self._discount), ('out["indices"]', idx), ('out["discount"]', disc)))
        with t.cuda.device(dev):
            _check(lib.mxv_nstep_gather(t.cuda.current_stream(dev).cuda_stream, self.capacity, B, self._discount.data_ptr(), idx.data_ptr(),
                                        disc.data_ptr()))
        return out

    def _sample_then_gather(self, parent, batch_size, out, **kw):
        B = _count("batch_size", batch_size)
        if out is not None and (not isinstance(out, dict) or "discount" not in out):
            raise ValueError('out must be a dict like sample_buffers()\'s: it has no "discount"')
        return self._gather_discount(B, parent(batch_size, out=out, **kw))

    def sample(self, batch_size, out=None):
        """ReplayBuffer.sample and one launch more: the dict also holds discount float32 [batch_size], gamma^(steps of the row's
        window); 0 where the ring was empty under device counters (indices -1)."""
        return self._sample_then_gather(super().sample, batch_size, out)

    # ---- checkpoints ----
    def state_dict(self) -> dict:
        """The parent's state with n_step, gamma and the discount ring (synchronises)."""
        state = super().state_dict()
        state.update(n_step=self.n_step, gamma=self.gamma, discount=self._discount.clone())
        return state

    def load_state_dict(self, state: dict):
        for key in ("n_step", "gamma", "discount"):
            if key not in state:
                raise ValueError(f'the state has no "{key}": it is not an n-step buffer\'s')
        n_step, gamma = _window(state["n_step"], state["gamma"])
        super().load_state_dict(state)
        self.n_step, self.gamma = n_step, gamma
        self._discount.copy_(state["discount"])


class NStepPrioritizedReplayBuffer(PrioritizedReplayBuffer, NStepReplayBuffer):
    """gym_amd.PrioritizedReplayBuffer over n-step rows: the priority insert, then the n-step ring insert (the cooperative _insert
    chain), proportional draws with importance weights, and `discount`.  Arguments: NStepReplayBuffer's, then alpha and eps."""

    def __init__(self, capacity, obs_shape, n_step, gamma, obs_dtype=None, action_dtype=None, seed=0, device=None, alpha=0.6, eps=1e-6):
        self.n_step, self.gamma = _window(n_step, gamma)
        super().__init__(capacity, obs_shape, obs_dtype=obs_dtype, action_dtype=action_dtype, seed=seed, device=device, alpha=alpha, eps=eps)

    def sample(self, batch_size, beta=0.4, out=None):
        """PrioritizedReplayBuffer.sample and one launch more: the dict also holds discount float32 [batch_size]."""
        return self._sample_then_gather(super().sample, batch_size, out, beta=beta)
