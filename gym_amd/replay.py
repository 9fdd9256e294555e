"""A uniform replay buffer on the device (include/mxv_replay.h): a ring of transitions, the fused insert of a [K, N]
rollout chunk and a Philox-keyed uniform draw with its gather — what lies between a rollout and gym_amd.dqn_loss.

    buf = rollout.replay_buffer(1 << 20)                       # or gym_amd.ReplayBuffer(capacity, obs_shape, obs_dtype, action_dtype, seed)
    buf.add_chunk(first_obs, traj)                             # traj of rollout_per_step / rollout_tape, or a hand-recorded chunk: ONE launch
    batch = buf.sample(4096)                                   # ONE launch: obs, actions, reward, terminated, next_obs, indices
    loss, stats = gym_amd.dqn_loss(q(batch["obs"]), batch["actions"], reward=batch["reward"], terminated=batch["terminated"],
                                   next_q=q_target(batch["next_obs"]), next_q_online=q(batch["next_obs"]))

The stored next observation of a step that ended is the FINAL observation (traj["final_obs"]), so the stored `terminated` alone is what
the bootstrap mode of dqn_loss needs.  The draws follow the Philox contract under stream tag 9: row j of sample step t depends on
(seed, j, t, rows stored) alone — not on the batch size, not on how the work is grouped into launches — so two runs draw the same
batches and a restored state_dict() continues bit-identically.  Everything is bit-equal to the NumPy twin tests/replay_host.py and
launches on the caller's current stream without a synchronisation.  The header is optional (mxv.h does not include it), so its symbols
are bound here, over the same library as gym_amd._native, and are not part of _native.EXPORTS.  Importing this module does not import
torch.
"""
from __future__ import annotations

import ctypes as C

from . import _native
from ._policy_args import _U64, _index, _ld, _one_device, _ptr, _vector
from ._policy_args import _check as _raise

REPLAY_EXPORTS = ("mxv_replay_insert", "mxv_replay_sample", "mxv_replay_last_error")
MAX_WIDTH = 65536            # dwords of an observation row (MXV_REPLAY_MAX_WIDTH)
MAX_CAPACITY = 1 << 31       # rows of a ring (MXV_REPLAY_MAX_CAPACITY)
STREAM_TAG = 9               # ctr[3] >> 28 of the index draws (MXV_REPLAY_STREAM_TAG)

lib = _native.lib
_P, _I64, _I32, _U = C.c_void_p, C.c_int64, C.c_int32, C.c_uint64
lib.mxv_replay_insert.argtypes = [_P, _I64, _I32, _I64, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _I32, _P, _I32, _P, _P, _U, _P, _P, _P, _P, _P, _P]
lib.mxv_replay_insert.restype = C.c_int
lib.mxv_replay_sample.argtypes = [_P, _I64, _I32, _I64, _P, _P, _P, _P, _P, _U, _U, _U, _P, _P, _P, _P, _P, _I32, _P, _P]
lib.mxv_replay_sample.restype = C.c_int
lib.mxv_replay_last_error.argtypes = []
lib.mxv_replay_last_error.restype = C.c_char_p


def _check(rc: int):
    _raise(rc, lib.mxv_replay_last_error)


def _count(name, v, lo=1):
    if isinstance(v, bool) or not isinstance(v, int) or v < lo:
        raise ValueError(f"{name} must be an integer of at least {lo}, got {v!r}")
    return v


class ReplayBuffer:
    """A ring of `capacity` transitions (obs, action, reward, terminated, next_obs) in device memory with uniform draws.

    obs_shape: the shape of one observation; obs_dtype torch.float32, int32, int64 or uint8 with a row of a multiple of 4 bytes (the
    kernels move a row as raw dwords).  action_dtype torch.int32, int64 (stored as its low 32 bits and returned sign-extended) or
    float32.  Rewards are stored as float32 (a float64 reward is rounded to nearest even), `terminated` as uint8.  seed: the key of the
    draws, an integer in [0, 2^64).  Everything launches on the caller's current stream of `device`."""

    def __init__(self, capacity, obs_shape, obs_dtype=None, action_dtype=None, seed=0, device=None):
        import torch as t

        if not t.cuda.is_available():
            raise RuntimeError("ReplayBuffer needs a HIP device (torch.cuda.is_available() is False); gym_amd has no CPU fallback")
        self._torch = t
        obs_dtype = t.float32 if obs_dtype is None else obs_dtype
        action_dtype = t.int32 if action_dtype is None else action_dtype
        self.capacity = _count("capacity", capacity)
        if self.capacity > MAX_CAPACITY:
            raise ValueError(f"capacity must be at most 2^31, got {capacity!r}")
        if isinstance(obs_shape, int) and not isinstance(obs_shape, bool):
            obs_shape = (obs_shape,)
        self.obs_shape = tuple(_count("obs_shape entries", s) for s in obs_shape)
        if obs_dtype not in (t.float32, t.int32, t.int64, t.uint8):
            raise ValueError(f"obs_dtype must be torch.float32, int32, int64 or uint8, got {obs_dtype!r}")
        if action_dtype not in (t.int32, t.int64, t.float32):
            raise ValueError(f"action_dtype must be torch.int32, int64 or float32, got {action_dtype!r}")
        self.obs_dtype, self.action_dtype = obs_dtype, action_dtype
        self._elem = t.empty(0, dtype=obs_dtype).element_size()
        self._numel = 1
        for s in self.obs_shape:
            self._numel *= s
        row_bytes = self._numel * self._elem
        if row_bytes % 4:
            raise ValueError(f"an observation of shape {self.obs_shape} and {obs_dtype} is {row_bytes} bytes: rows must be a multiple of 4 bytes")
        self.W = row_bytes // 4
        if self.W > MAX_WIDTH:
            raise ValueError(f"an observation row of {self.W} dwords is beyond {MAX_WIDTH}")
        if self.capacity * self.W > 1 << 40:
            raise ValueError(f"capacity * row = {self.capacity} * {self.W} dwords is beyond 2^40")
        self.seed = _index("seed", seed)
        self.device = device if isinstance(device, t.device) else t.device("cuda", t.cuda.current_device() if device is None else device)
        self._action_bytes = 8 if action_dtype == t.int64 else 4
        cap, dev = self.capacity, self.device
        # the ring: zero-filled, so that a slot never written reads as zeros
        self._obs = t.zeros((cap, self._numel), dtype=obs_dtype, device=dev)
        self._next = t.zeros((cap, self._numel), dtype=obs_dtype, device=dev)
        self._action = t.zeros(cap, dtype=t.float32 if action_dtype == t.float32 else t.int32, device=dev)
        self._reward = t.zeros(cap, dtype=t.float32, device=dev)
        self._term = t.zeros(cap, dtype=t.uint8, device=dev)
        self._count, self._step = 0, 0          # the host's mirror: rows ever inserted, sample steps taken
        self._state = None                      # uint64 [2] on the device (as int64) once enable_graph_capture() was called
        t.cuda.current_stream(dev).synchronize()   # construction is rare: the ring is ready on whichever stream inserts

    # ---- the counters ----
    def enable_graph_capture(self):
        """Moves the row count and the sample step into a device uint64 [2] that add / add_chunk / sample read and advance with one more
        launch each: a recorded insert + sample continues the ring and the draws on every replay.  From here on the device counters
        rule: len(), count and state_dict() read them back (a synchronisation), and sample() no longer refuses an empty buffer — its rows
        then come back as indices -1 and zeros."""
        if self._state is None:
            t = self._torch
            self._state = t.tensor([self._signed(self._count), self._signed(self._step)], dtype=t.int64, device=self.device)
            t.cuda.current_stream(self.device).synchronize()
        return self

    @staticmethod
    def _signed(v):
        return v - (1 << 64) if v >= (1 << 63) else v

    def _counters(self):
        if self._state is not None:
            c, s = self._state.tolist()
            self._count, self._step = c & _U64, s & _U64
        return self._count, self._step

    @property
    def count(self) -> int:
        """Rows ever inserted (synchronises after enable_graph_capture())."""
        return self._counters()[0]

    @property
    def sample_step(self) -> int:
        """Sample steps taken (synchronises after enable_graph_capture())."""
        return self._counters()[1]

    def __len__(self) -> int:
        """Rows stored: min(count, capacity).  After enable_graph_capture() this reads the device counter and synchronises."""
        return min(self.count, self.capacity)

    # ---- insert ----
    def _rows_of(self, x, name, lead):
        """An observation tensor of shape lead + obs_shape as its [rows, W-dword] rows: (tensor, row stride in dwords)."""
        t = self._torch
        if not isinstance(x, t.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(x).__name__}")
        if x.dtype != self.obs_dtype:
            raise ValueError(f"{name} must be {self.obs_dtype}, got {x.dtype}")
        if tuple(x.shape) != tuple(lead) + self.obs_shape:
            raise ValueError(f"{name} must have shape {tuple(lead) + self.obs_shape}, got {tuple(x.shape)}")
        rows = 1
        for s in lead:
            rows *= s
        try:
            x2 = x.view(rows, self._numel)
        except RuntimeError:
            raise ValueError(f"{name} of shape {tuple(x.shape)} with strides {tuple(x.stride())} cannot be viewed as [{rows}, {self._numel}] rows: "
                             "pass a contiguous tensor") from None
        if self._numel > 1 and x2.stride(1) != 1:
            raise ValueError(f"{name} must be contiguous within an observation (stride {x2.stride(1)}): rows may be strided views, elements not")
        ld = _ld(x2, self._numel)
        if ld < self._numel:
            raise ValueError(f"{name} has row stride {ld} < {self._numel}: rows overlap")
        if (ld * self._elem) % 4:
            raise ValueError(f"{name} has a row stride of {ld * self._elem} bytes: must be a multiple of 4")
        return x2, ld * self._elem // 4

    def _insert(self, K, N, first_obs, obs, final_obs, actions, reward, terminated, truncated):
        t = self._torch
        lead = (K, N) if K is not None else (N,)
        R = N if K is None else K * N
        if R > self.capacity:
            raise ValueError(f"{R} rows exceed the capacity {self.capacity}: two rows of one insert would share a slot")
        first2, first_ld = self._rows_of(first_obs, "first_obs" if K is not None else "obs", (N,))
        obs2, obs_ld = self._rows_of(obs, 'traj["obs"]' if K is not None else "next_obs", lead)
        fin2, fin_ld = (None, 0) if final_obs is None else self._rows_of(final_obs, 'traj["final_obs"]', lead)
        act = _vector(t, actions, "actions", lead, (self.action_dtype,))
        rew = _vector(t, reward, "reward", lead, (t.float32, t.float64))
        flags = []
        for name, x in (("terminated", terminated), ("truncated", truncated)):
            if isinstance(x, t.Tensor) and x.dtype == t.bool:
                x = x.view(t.uint8)
            flags.append(None if x is None else _vector(t, x, name, lead, (t.uint8,)))
        term, trunc = flags
        if term is None:
            raise ValueError("terminated must be a torch tensor, got None")
        dev = _one_device((("the buffer", self._obs), ("first_obs" if K is not None else "obs", first2), ("obs" if K is not None else "next_obs", obs2),
                           ("final_obs", fin2), ("actions", act), ("reward", rew), ("terminated", term), ("truncated", trunc)))
        with t.cuda.device(dev):
            self._store(t.cuda.current_stream(dev).cuda_stream, 1 if K is None else K, N, first2.data_ptr(), first_ld, obs2.data_ptr(), obs_ld,
                        _ptr(fin2), fin_ld, act.data_ptr(), rew.data_ptr(), rew.element_size(), term.data_ptr(), _ptr(trunc))
        if self._state is None:
            self._count += R

    def _store(self, stream, K, N, first, first_ld, obs, obs_ld, final, final_ld, actions, reward, reward_bytes, terminated, truncated):
        """The library call of an insert, on the prepared arguments of _insert (device addresses, row strides in dwords): what a
        subclass with another insert rule overrides."""
        _check(lib.mxv_replay_insert(stream, self.capacity, self.W, K, N, first, first_ld, obs, obs_ld, final, final_ld, actions,
                                     self._action_bytes, reward, reward_bytes, terminated, truncated, self._count, _ptr(self._state),
                                     self._obs.data_ptr(), self._next.data_ptr(), self._action.data_ptr(), self._reward.data_ptr(),
                                     self._term.data_ptr()))

    def add_chunk(self, first_obs, traj):
        """Stores the K * N transitions of a [K, N] chunk in ONE launch (two after enable_graph_capture()).

        traj: the dict of rollout_per_step / rollout_tape or a hand-recorded chunk with "obs" [K, N, ...] (traj["obs"][t] is the
        observation AFTER step t), "actions", "reward" (float32 or float64), "terminated" [K, N] (uint8 or bool), and optionally
        "truncated" and "final_obs" [K, N, ...].  first_obs [N, ...]: the observation the chunk started from (reset()'s, or
        traj["obs"][K-1] of the previous chunk).  Row (t, i) stores the observation its action was taken from — first_obs[i] or
        traj["obs"][t-1, i] — and as the next observation traj["final_obs"][t, i] where the step ended, traj["obs"][t, i] elsewhere.  A
        traj with "truncated" but no "final_obs" is refused: a truncated step would store the observation after the reset."""
        if not isinstance(traj, dict):
            raise ValueError(f"traj must be a dict of tensors, got {type(traj).__name__}")
        for key in ("obs", "actions", "reward", "terminated"):
            if key not in traj:
                raise ValueError(f'traj has no "{key}"')
        final_obs, truncated = traj.get("final_obs"), traj.get("truncated")
        if truncated is not None and final_obs is None:
            raise ValueError('traj has "truncated" but no "final_obs": a truncated step would store the observation after the reset '
                             "(pass traj[\"final_obs\"] — trajectory_buffers(want_final=True) where the rollout has it — or leave "
                             "\"truncated\" out if no step of the chunk can be truncated)")
        obs = traj["obs"]
        if not isinstance(obs, self._torch.Tensor) or obs.dim() < 2:
            raise ValueError(f'traj["obs"] must be a tensor of shape [K, N] + {self.obs_shape}')
        K, N = int(obs.shape[0]), int(obs.shape[1])
        if K < 1 or N < 1:
            raise ValueError(f'traj["obs"] must hold at least one step and one env, got shape {tuple(obs.shape)}')
        self._insert(K, N, first_obs, obs, final_obs, traj["actions"], traj["reward"], traj["terminated"], truncated)

    def add(self, obs, actions, reward, terminated, next_obs):
        """Stores R flat transitions [R, ...] in ONE launch: the add of an ordinary buffer.  next_obs is stored as given: at a step that
        ended pass the final observation, not the one after the reset."""
        if not isinstance(obs, self._torch.Tensor) or obs.dim() < 1 or obs.shape[0] < 1:
            raise ValueError(f"obs must be a tensor of shape [R] + {self.obs_shape} with at least one row")
        self._insert(None, int(obs.shape[0]), obs, next_obs, None, actions, reward, terminated, None)

    # ---- sample ----
    def sample_buffers(self, batch_size):
        """The tensors sample(batch_size, out=...) fills, as a dict: allocate once, sample without allocating."""
        t, B, dev = self._torch, _count("batch_size", batch_size), self.device
        return {"obs": t.empty((B,) + self.obs_shape, dtype=self.obs_dtype, device=dev),
                "actions": t.empty(B, dtype=self.action_dtype, device=dev), "reward": t.empty(B, dtype=t.float32, device=dev),
                "terminated": t.empty(B, dtype=t.uint8, device=dev),
                "next_obs": t.empty((B,) + self.obs_shape, dtype=self.obs_dtype, device=dev), "indices": t.empty(B, dtype=t.int64, device=dev)}

    def sample(self, batch_size, out=None):
        """Draws batch_size rows uniformly with replacement from the rows stored -> dict of obs, actions, reward (float32), terminated
        (uint8), next_obs and indices (int64: the slots drawn), in ONE launch (two after enable_graph_capture()).  out: a dict like
        sample_buffers(batch_size)'s, which is filled and returned — the call then allocates nothing.  Raises on an empty buffer (by the
        host's mirror of the count; after enable_graph_capture() the device counter rules and an empty ring yields indices -1 and zeros)."""
        t = self._torch
        B = _count("batch_size", batch_size)
        if self._state is None and self._count == 0:
            raise ValueError("the buffer is empty: add() or add_chunk() before sample()")
        if out is None:
            out = self.sample_buffers(B)
        elif not isinstance(out, dict) or any(k not in out for k in ("obs", "actions", "reward", "terminated", "next_obs", "indices")):
            raise ValueError("out must be a dict with obs, actions, reward, terminated, next_obs and indices (sample_buffers())")
        o2, _ = self._rows_of(out["obs"], 'out["obs"]', (B,))
        n2, _ = self._rows_of(out["next_obs"], 'out["next_obs"]', (B,))
        for name, x in (('out["obs"]', o2), ('out["next_obs"]', n2)):
            if not x.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        act = _vector(t, out["actions"], 'out["actions"]', (B,), (self.action_dtype,))
        rew = _vector(t, out["reward"], 'out["reward"]', (B,), (t.float32,))
        term = _vector(t, out["terminated"], 'out["terminated"]', (B,), (t.uint8,))
        idx = _vector(t, out["indices"], 'out["indices"]', (B,), (t.int64,))
        dev = _one_device((("the buffer", self._obs), ('out["obs"]', o2), ('out["next_obs"]', n2), ('out["actions"]', act), ('out["reward"]', rew),
                           ('out["terminated"]', term), ('out["indices"]', idx)))
        with t.cuda.device(dev):
            _check(lib.mxv_replay_sample(t.cuda.current_stream(dev).cuda_stream, self.capacity, self.W, B, self._obs.data_ptr(),
                                         self._next.data_ptr(), self._action.data_ptr(), self._reward.data_ptr(), self._term.data_ptr(), self.seed,
                                         self._count, self._step, _ptr(self._state), idx.data_ptr(), o2.data_ptr(), n2.data_ptr(), act.data_ptr(),
                                         self._action_bytes, rew.data_ptr(), term.data_ptr()))
        if self._state is None:
            self._step = (self._step + 1) & _U64
        return out

    # ---- checkpoints ----
    def state_dict(self) -> dict:
        """The ring's contents, the counters and the seed (synchronises): a buffer that loads it continues bit-identically."""
        count, step = self._counters()
        return {"capacity": self.capacity, "obs_shape": self.obs_shape, "obs_dtype": str(self.obs_dtype), "action_dtype": str(self.action_dtype),
                "seed": self.seed, "count": count, "sample_step": step, "obs": self._obs.clone(), "next_obs": self._next.clone(),
                "actions": self._action.clone(), "reward": self._reward.clone(), "terminated": self._term.clone()}

    def load_state_dict(self, state: dict):
        for key, mine in (("capacity", self.capacity), ("obs_shape", self.obs_shape), ("obs_dtype", str(self.obs_dtype)),
                          ("action_dtype", str(self.action_dtype))):
            theirs = state[key]
            if (tuple(theirs) if key == "obs_shape" else theirs) != mine:
                raise ValueError(f"the state is of a buffer with {key} = {theirs!r}, this one has {mine!r}")
        self.seed = _index("seed", state["seed"])
        count, step = _index("count", state["count"]), _index("sample_step", state["sample_step"])
        for mine, key in ((self._obs, "obs"), (self._next, "next_obs"), (self._action, "actions"), (self._reward, "reward"), (self._term, "terminated")):
            mine.copy_(state[key])
        self._count, self._step = count, step
        if self._state is not None:
            t = self._torch
            self._state.copy_(t.tensor([self._signed(count), self._signed(step)], dtype=t.int64))
