"""Prioritised experience replay on the device (include/mxv_prio.h): gym_amd.ReplayBuffer with an exact integer sum tree
over its slots — proportional draws, importance weights and update_priorities — what lies between a rollout and the `weights=` /
`td_error=` of gym_amd.dqn_loss.

    buf = rollout.prioritized_replay_buffer(1 << 20)           # or gym_amd.PrioritizedReplayBuffer(capacity, obs_shape, ..., alpha=0.6, eps=1e-6)
    buf.add_chunk(first_obs, traj)                             # new rows get the largest priority seen: one launch more than the ring's
    batch = buf.sample(4096, beta=0.4)                         # two launches: ..., indices, weights
    td = torch.empty(4096, device=dev)
    loss, stats = gym_amd.dqn_loss(q(batch["obs"]), batch["actions"], ..., weights=batch["weights"], td_error=td)
    buf.update_priorities(batch["indices"], td)                # two launches

Priorities are fixed-point integers (a uint32 leaf is (|td| + eps)^alpha in units of 2^-20) and every inner node an exact uint64 sum, so
the tree has the same bits whatever order the device's integer atomics arrive in: two runs draw the same batches, a restored
state_dict() continues bit-identically, and no torch generator is involved.  The draws follow the Philox contract under stream tag 10:
row j of sample step t depends on (seed, j, t, tree) alone.  Everything is bit-equal to the NumPy twin tests/prio_host.py and launches on
the caller's current stream without a synchronisation.  The header is optional (mxv.h does not include it), so its symbols are bound
here and are not part of _native.EXPORTS.  Importing this module does not import torch.
"""
from __future__ import annotations

import ctypes as C

from . import _native
from ._policy_args import _U64, _one_device, _ptr, _vector
from ._policy_args import _check as _raise
from .replay import ReplayBuffer, _count

PRIO_EXPORTS = ("mxv_prio_layout", "mxv_prio_insert", "mxv_prio_update", "mxv_prio_sample", "mxv_prio_last_error")
FANOUT = 16                  # MXV_PRIO_FANOUT
FRAC_BITS = 20               # MXV_PRIO_FRAC_BITS
QMAX = 4294967295            # MXV_PRIO_QMAX
STREAM_TAG = 10              # ctr[3] >> 28 of the draws (MXV_PRIO_STREAM_TAG)
WORKSPACE_WORDS = 2048       # MXV_PRIO_WORKSPACE_WORDS

lib = _native.lib
_P, _I64, _I32, _U, _D = C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_double
lib.mxv_prio_layout.argtypes = [_I64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
lib.mxv_prio_layout.restype = C.c_int
lib.mxv_prio_insert.argtypes = [_P, _I64, _I64, _I64, _U, _P, _P, _I64, _P, _I64, _P]
lib.mxv_prio_insert.restype = C.c_int
lib.mxv_prio_update.argtypes = [_P, _I64, _I64, _P, _P, _D, _D, _U, _P, _P, _I64, _P, _I64, _P, _P]
lib.mxv_prio_update.restype = C.c_int
lib.mxv_prio_sample.argtypes = [_P, _I64, _I32, _I64, _P, _P, _P, _P, _P, _P, _I64, _P, _I64, _U, _U, _P, _D, _P, _P, _P, _P, _P, _I32, _P, _P, _P]
lib.mxv_prio_sample.restype = C.c_int
lib.mxv_prio_last_error.argtypes = []
lib.mxv_prio_last_error.restype = C.c_char_p


def _check(rc: int):
    _raise(rc, lib.mxv_prio_last_error)


def layout(capacity):
    """mxv_prio_layout -> (leaf_words of uint32, node_words of uint64, levels)."""
    a, b, h = C.c_int64(), C.c_int64(), C.c_int32()
    _check(lib.mxv_prio_layout(capacity, C.byref(a), C.byref(b), C.byref(h)))
    return a.value, b.value, h.value


def _unit(name, v, lo=0.0):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not lo <= v <= 1.0:
        raise ValueError(f"{name} must be a number in [{lo:g}, 1], got {v!r}")
    return float(v)


class PrioritizedReplayBuffer(ReplayBuffer):
    """gym_amd.ReplayBuffer whose draws are proportional to priority (|td| + eps)^alpha, with the importance weights of the batch.

    alpha in [0, 1] (0: uniform over the written slots), eps in [2^-64, 1].  New rows get the largest priority any update has written
    (1.0 before the first).  The other arguments are ReplayBuffer's."""

    def __init__(self, capacity, obs_shape, obs_dtype=None, action_dtype=None, seed=0, device=None, alpha=0.6, eps=1e-6):
        self.alpha, self.eps = _unit("alpha", alpha), _unit("eps", eps, 2.0 ** -64)
        super().__init__(capacity, obs_shape, obs_dtype=obs_dtype, action_dtype=action_dtype, seed=seed, device=device)
        t, dev = self._torch, self.device
        self._leaf_words, self._node_words, self.levels = layout(self.capacity)
        # the tree: zero-filled (a slot never written cannot be drawn); uint32 leaves and uint64 nodes held as int32 / int64 bits
        self._leaf = t.zeros(self._leaf_words, dtype=t.int32, device=dev)
        self._node = t.zeros(self._node_words, dtype=t.int64, device=dev)
        self._qmax = t.full((1,), 1 << FRAC_BITS, dtype=t.int32, device=dev)
        self._work = t.zeros(WORKSPACE_WORDS, dtype=t.int32, device=dev)
        self._saved = t.zeros(WORKSPACE_WORDS, dtype=t.int32, device=dev)      # a word per row of an update: grown by the first larger batch
        t.cuda.current_stream(dev).synchronize()

    # ---- insert ----
    def _insert(self, K, N, first_obs, obs, final_obs, actions, reward, terminated, truncated):
        """The priority insert, then the ring insert: both read the same count.  A chunk that the ring insert then refuses (a tensor of
        the wrong shape or dtype) has already given its slots the insert priority."""
        t = self._torch
        R = N if K is None else K * N
        if R > self.capacity:
            raise ValueError(f"{R} rows exceed the capacity {self.capacity}: two rows of one insert would share a slot")
        with t.cuda.device(self.device):
            _check(lib.mxv_prio_insert(t.cuda.current_stream(self.device).cuda_stream, self.capacity, 1 if K is None else K, N, self._count,
                                       _ptr(self._state), self._leaf.data_ptr(), self._leaf_words, self._node.data_ptr(), self._node_words,
                                       self._qmax.data_ptr()))
        super()._insert(K, N, first_obs, obs, final_obs, actions, reward, terminated, truncated)

    # ---- sample ----
    def sample_buffers(self, batch_size):
        """The tensors sample(batch_size, out=...) fills, as a dict: ReplayBuffer's and "weights" float32 [batch_size]."""
        out = super().sample_buffers(batch_size)
        out["weights"] = self._torch.empty(batch_size, dtype=self._torch.float32, device=self.device)
        return out

    def sample(self, batch_size, beta=0.4, out=None):
        """Draws batch_size rows with probability q_k / total, with replacement -> dict of obs, actions, reward, terminated, next_obs,
        indices (int64: the slots drawn) and weights (float32: (N P)^-beta over its batch maximum, exactly 1.0 at the batch's smallest
        priority), in two launches (three after enable_graph_capture()).  beta in [0, 1].  out: a dict like sample_buffers(batch_size)'s,
        which is filled and returned.  Raises on an empty buffer by the host's mirror of the count; after enable_graph_capture() an empty
        tree yields indices -1, zeros and zero weights."""
        t = self._torch
        B = _count("batch_size", batch_size)
        beta = _unit("beta", beta)
        if self._state is None and self._count == 0:
            raise ValueError("the buffer is empty: add() or add_chunk() before sample()")
        if out is None:
            out = self.sample_buffers(B)
        elif not isinstance(out, dict) or any(k not in out for k in ("obs", "actions", "reward", "terminated", "next_obs", "indices", "weights")):
            raise ValueError("out must be a dict with obs, actions, reward, terminated, next_obs, indices and weights (sample_buffers())")
        o2, _ = self._rows_of(out["obs"], 'out["obs"]', (B,))
        n2, _ = self._rows_of(out["next_obs"], 'out["next_obs"]', (B,))
        for name, x in (('out["obs"]', o2), ('out["next_obs"]', n2)):
            if not x.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        act = _vector(t, out["actions"], 'out["actions"]', (B,), (self.action_dtype,))
        rew = _vector(t, out["reward"], 'out["reward"]', (B,), (t.float32,))
        term = _vector(t, out["terminated"], 'out["terminated"]', (B,), (t.uint8,))
        idx = _vector(t, out["indices"], 'out["indices"]', (B,), (t.int64,))
        wts = _vector(t, out["weights"], 'out["weights"]', (B,), (t.float32,))
        dev = _one_device((("the buffer", self._obs), ('out["obs"]', o2), ('out["next_obs"]', n2), ('out["actions"]', act), ('out["reward"]', rew),
                           ('out["terminated"]', term), ('out["indices"]', idx), ('out["weights"]', wts)))
        step_dev = None if self._state is None else self._state.data_ptr() + 8
        with t.cuda.device(dev):
            _check(lib.mxv_prio_sample(t.cuda.current_stream(dev).cuda_stream, self.capacity, self.W, B, self._obs.data_ptr(),
                                       self._next.data_ptr(), self._action.data_ptr(), self._reward.data_ptr(), self._term.data_ptr(),
                                       self._leaf.data_ptr(), self._leaf_words, self._node.data_ptr(), self._node_words, self.seed, self._step,
                                       step_dev, beta, self._work.data_ptr(), idx.data_ptr(), o2.data_ptr(), n2.data_ptr(), act.data_ptr(),
                                       self._action_bytes, rew.data_ptr(), term.data_ptr(), wts.data_ptr()))
        if self._state is None:
            self._step = (self._step + 1) & _U64
        return out

    # ---- update ----
    def update_priorities(self, indices, td_error):
        """Sets the priority of every drawn slot to (|td_error| + eps)^alpha, in two launches (the first call with a batch larger
        than any before it allocates a word per row: make it before recording a graph).  indices int64 [B] (batch["indices"]),
        td_error float32 [B] (what dqn_loss wrote into td_error=).  A slot drawn more than once gets the largest of its rows'
        priorities; rows with index -1 (an empty draw) or beyond the rows stored are skipped; a NaN or infinite TD error gives the
        largest priority there is.  A slot that was overwritten between the draw and the update gets the stale row's priority, as in
        every prioritised buffer."""
        t = self._torch
        if not isinstance(indices, t.Tensor) or indices.dim() != 1 or indices.shape[0] < 1:
            raise ValueError("indices must be an int64 tensor of shape [B] with at least one row")
        B = int(indices.shape[0])
        idx = _vector(t, indices, "indices", (B,), (t.int64,))
        td = _vector(t, td_error, "td_error", (B,), (t.float32,))
        dev = _one_device((("the buffer", self._obs), ("indices", idx), ("td_error", td)))
        if self._saved.numel() < B:
            self._saved = t.empty(B, dtype=t.int32, device=self.device)
        with t.cuda.device(dev):
            _check(lib.mxv_prio_update(t.cuda.current_stream(dev).cuda_stream, self.capacity, B, idx.data_ptr(), td.data_ptr(), self.alpha, self.eps,
                                       self._count, _ptr(self._state), self._leaf.data_ptr(), self._leaf_words, self._node.data_ptr(),
                                       self._node_words, self._qmax.data_ptr(), self._saved.data_ptr()))

    # ---- checkpoints ----
    def state_dict(self) -> dict:
        """ReplayBuffer's state and the tree — leaves, nodes, the largest priority — with alpha and eps (synchronises)."""
        state = super().state_dict()
        state.update(alpha=self.alpha, eps=self.eps, leaves=self._leaf.clone(), nodes=self._node.clone(), qmax=self._qmax.clone())
        return state

    def load_state_dict(self, state: dict):
        for key in ("alpha", "eps", "leaves", "nodes", "qmax"):
            if key not in state:
                raise ValueError(f'the state has no "{key}": it is not a PrioritizedReplayBuffer\'s')
        alpha, eps = _unit("alpha", state["alpha"]), _unit("eps", state["eps"], 2.0 ** -64)
        super().load_state_dict(state)
        self.alpha, self.eps = alpha, eps
        for mine, key in ((self._leaf, "leaves"), (self._node, "nodes"), (self._qmax, "qmax")):
            mine.copy_(state[key])
