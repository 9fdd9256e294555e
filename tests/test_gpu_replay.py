"""gym_amd.ReplayBuffer and the calls of include/mxv_replay.h on the device against tests/replay_host.py, the NumPy twin of the rule: every
array compared bit for bit.  Insert: every capacity x row width x chunk shape with inserts that wrap the ring, counts by value near
2^32, canaries in the slots not written and in the final_obs rows that must not be read, float32 / float64 rewards with NaN / Inf /
ties, int32 / int64 / float32 actions, strided and misaligned sources (both the 16-byte and the dword paths), the flat add.  Sample:
every batch size on half-full and full rings, aligned and misaligned, the empty ring.  The device counters under graph replay, the
launch counts, the checkpoint, a real CartPole chunk, the example run twice, and the front end's refusals."""
import os
import sys

import numpy as np
import pytest

import replay_host as rh
from conftest import ROOT
from test_gpu_ppo import _captured_launches, _hip

pytestmark = pytest.mark.gpu

CAPACITIES = (5, 64, 257, 1025)
WIDTHS = (1, 2, 3, 4, 6, 7, 8, 9, 16, 17, 1023, 1025, 7056)
CHUNKS = ((1, 1), (3, 5), (4, 64), (2, 257), (1, None))      # (1, None): one step of C envs
BATCHES = (1, 3, 63, 64, 65, 255, 256, 257, 1025)
CANARY, CANARY_FINAL = 0xCACACACA, 0xDEADBEEF      # both have the top bit set; the data below never does


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def up(torch, a):
    """A NumPy array on the device, unsigned types as their signed twins."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to("cuda:0")


def down(torch, x, dtype=np.uint32):
    return x.detach().contiguous().cpu().numpy().reshape(-1).view(dtype)


def rows_on_device(torch, data, pad=0, shift=0):
    """uint32 [rows, W] as a device buffer whose rows are W + pad dwords apart and whose base is `shift` dwords off the allocation:
    -> (the buffer, kept alive by the caller; the address of row 0; the stride)."""
    rows, W = data.shape
    ld = W + pad
    host = np.full(shift + rows * ld, CANARY, np.uint32)
    host[shift:].reshape(rows, ld)[:, :W] = data
    buf = up(torch, host)
    return buf, buf.data_ptr() + 4 * shift, ld


class DeviceRing:
    """The five ring arrays on the device, filled with the canary; `shift` dwords off their allocations' bases."""

    def __init__(self, torch, C, W, shift=0):
        self.C, self.W, self.shift, self.torch = C, W, shift, torch
        self.obs = up(torch, np.full(shift + C * W, CANARY, np.uint32))
        self.next = up(torch, np.full(shift + C * W, CANARY, np.uint32))
        self.action = up(torch, np.full(C, CANARY, np.uint32))
        self.reward = up(torch, np.full(C, CANARY, np.uint32))
        self.term = up(torch, np.full(C, CANARY & 0xFF, np.uint8))

    def pointers(self):
        return (self.obs.data_ptr() + 4 * self.shift, self.next.data_ptr() + 4 * self.shift, self.action.data_ptr(), self.reward.data_ptr(),
                self.term.data_ptr())

    def load(self, ring):
        t = self.torch
        self.obs[self.shift:].copy_(up(t, ring.obs.reshape(-1)))
        self.next[self.shift:].copy_(up(t, ring.next.reshape(-1)))
        self.action.copy_(up(t, ring.action))
        self.reward.copy_(up(t, ring.reward))
        self.term.copy_(up(t, ring.term))

    def same_as(self, ring, what):
        t = self.torch
        for name, mine, theirs in (("obs", down(t, self.obs)[self.shift:], ring.obs.reshape(-1)), ("next", down(t, self.next)[self.shift:], ring.next.reshape(-1)),
                                   ("action", down(t, self.action), ring.action), ("reward", down(t, self.reward), ring.reward),
                                   ("term", down(t, self.term, np.uint8), ring.term)):
            bad = np.flatnonzero(mine != theirs)
            assert bad.size == 0, (what, name, bad[:8], mine[bad[:8]], theirs[bad[:8]])
        if self.shift:
            assert (down(t, self.obs)[:self.shift] == CANARY).all() and (down(t, self.next)[:self.shift] == CANARY).all(), what


def make_chunk(rng, K, N, W, reward_dtype, action_dtype, with_final):
    """A chunk whose observation dwords never have the top bit set; final_obs rows of steps that did not end hold CANARY_FINAL."""
    obs = rng.integers(0, 1 << 31, size=(K, N, W), dtype=np.int64).astype(np.uint32)
    first = rng.integers(0, 1 << 31, size=(N, W), dtype=np.int64).astype(np.uint32)
    term = ((rng.random((K, N)) < 0.25) * rng.integers(1, 256, size=(K, N))).astype(np.uint8)
    trunc = ((rng.random((K, N)) < 0.25) * rng.integers(1, 256, size=(K, N))).astype(np.uint8) if with_final else None
    final = None
    if with_final:
        final = rng.integers(0, 1 << 31, size=(K, N, W), dtype=np.int64).astype(np.uint32)
        final[(term == 0) & (trunc == 0)] = CANARY_FINAL
    actions = rng.integers(-3, 4, size=(K, N)).astype(action_dtype)
    reward = (rng.standard_normal((K, N)) * 100).astype(reward_dtype)
    flat = reward.reshape(-1)
    flat[::5] = np.nan
    flat[1::7] = np.inf
    flat[2::11] = -np.inf
    if reward_dtype == np.float64:
        flat[3::6] = 1.0 + 2.0 ** -24           # a tie: to even, downwards
        flat[4::9] = 1.0 + 3 * 2.0 ** -24       # a tie: to even, upwards
        flat[0::13] = 1e300                     # overflows to +Inf
    return first, obs, actions, reward, term, trunc, final


def c_insert(torch, dring, count, chunk, *, pad=0, shift=0, state=None, stream=None):
    """mxv_replay_insert through ctypes on device copies of `chunk`; -> the status."""
    from gym_amd import replay

    first, obs, actions, reward, term, trunc, final = chunk
    K, N, W = obs.shape
    keep = [rows_on_device(torch, first, pad, shift), rows_on_device(torch, obs.reshape(K * N, W), pad, shift)]
    fin = rows_on_device(torch, final.reshape(K * N, W), pad, shift) if final is not None else (None, None, 0)
    a, r, te = up(torch, actions), up(torch, reward), up(torch, term)
    tr = None if trunc is None else up(torch, trunc)
    torch.cuda.synchronize()
    rc = replay.lib.mxv_replay_insert(stream, dring.C, W, K, N, keep[0][1], keep[0][2], keep[1][1], keep[1][2], fin[1], fin[2], a.data_ptr(),
                                      actions.dtype.itemsize, r.data_ptr(), reward.dtype.itemsize, te.data_ptr(), None if tr is None else tr.data_ptr(),
                                      count, None if state is None else state.data_ptr(), *dring.pointers())
    torch.cuda.synchronize()
    return rc


# ---- insert ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", WIDTHS)
def test_insert_equals_the_twin_at_every_capacity_and_chunk_shape(torch, W):
    from gym_amd import replay

    rng = np.random.default_rng(W)
    case = 0
    for C in CAPACITIES:
        for K, N in CHUNKS:
            N = C if N is None else N
            if K * N > C:
                continue
            case += 1
            # aligned and packed, or rows W + 3 dwords apart from a base 4 bytes off: both the 16-byte and the dword paths run
            pad, shift = ((0, 0), (3, 1))[case % 2]
            count = (0, (1 << 32) - 3, 7)[case % 3]
            inserts = max(3, min(5, (2 * C) // (K * N) + 1))
            twin, dring = rh.Ring(C, W, fill=CANARY), DeviceRing(torch, C, W, shift=(case // 2) % 2)
            for n in range(inserts):
                reward_dtype = (np.float64, np.float32)[(n + case) % 2]
                action_dtype = (np.int64, np.int32, np.float32)[(n + case) % 3]
                chunk = make_chunk(rng, K, N, W, reward_dtype, action_dtype, with_final=(n + case) % 3 != 0)
                rc = c_insert(torch, dring, count, chunk, pad=pad, shift=shift)
                assert rc == 0, replay.lib.mxv_replay_last_error()
                count = rh.insert(twin, count, chunk[0], chunk[1], chunk[2], chunk[3], chunk[4], chunk[5], chunk[6])
            what = (C, W, K, N, pad, shift, dring.shift)
            dring.same_as(twin, what)
            for x in (dring.obs, dring.next):
                assert not (down(torch, x) == CANARY_FINAL).any(), what      # no row of an unfinished step's final_obs was read
            if inserts * K * N < C:
                assert (twin.term == CANARY & 0xFF).any(), what               # some slots were never written: they kept the canary
    assert case >= 12


def test_a_full_wrap_is_needed_to_lose_the_canary_and_a_count_near_2_to_the_32_lands_where_the_twin_says(torch):
    from gym_amd import replay

    rng = np.random.default_rng(1)
    C, W = 64, 4
    twin, dring = rh.Ring(C, W, fill=CANARY), DeviceRing(torch, C, W)
    chunk = make_chunk(rng, 3, 5, W, np.float64, np.int64, True)
    assert c_insert(torch, dring, (1 << 32) - 3, chunk) == 0, replay.lib.mxv_replay_last_error()
    rh.insert(twin, (1 << 32) - 3, *chunk[:5], chunk[5], chunk[6])
    dring.same_as(twin, "near 2^32")
    written = sorted(((1 << 32) - 3 + r) % C for r in range(15))
    untouched = np.setdiff1d(np.arange(C), written)
    assert (down(torch, dring.action)[untouched] == CANARY).all() and (down(torch, dring.obs).reshape(C, W)[untouched] == CANARY).all()


# ---- sample ----------------------------------------------------------------------------------------------------------------------------------------
def c_sample(torch, dring, count, seed, step, B, action_bytes, *, shift=0, state=None, stream=None):
    from gym_amd import replay

    W = dring.W
    out = dict(indices=up(torch, np.full(B, 77, np.int64)), obs=up(torch, np.full(shift + B * W, CANARY, np.uint32)),
               next_obs=up(torch, np.full(shift + B * W, CANARY, np.uint32)), actions=up(torch, np.full(B * action_bytes // 4, CANARY, np.uint32)),
               reward=up(torch, np.full(B, CANARY, np.uint32)), terminated=up(torch, np.full(B, 0xCA, np.uint8)))
    torch.cuda.synchronize()
    rc = replay.lib.mxv_replay_sample(stream, dring.C, W, B, *dring.pointers(), seed, count, step, None if state is None else state.data_ptr(),
                                      out["indices"].data_ptr(), out["obs"].data_ptr() + 4 * shift, out["next_obs"].data_ptr() + 4 * shift,
                                      out["actions"].data_ptr(), action_bytes, out["reward"].data_ptr(), out["terminated"].data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, replay.lib.mxv_replay_last_error()
    got = dict(indices=down(torch, out["indices"], np.int64), obs=down(torch, out["obs"])[shift:].reshape(B, W),
               next_obs=down(torch, out["next_obs"])[shift:].reshape(B, W), reward=down(torch, out["reward"]),
               terminated=down(torch, out["terminated"], np.uint8),
               actions=down(torch, out["actions"], np.int64) if action_bytes == 8 else down(torch, out["actions"]))
    return got


def same_batch(got, want, what):
    for key in ("indices", "obs", "next_obs", "actions", "reward", "terminated"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (what, key, got[key][:8], want[key][:8])


@pytest.mark.parametrize("W", WIDTHS)
def test_sample_equals_the_twin_at_every_batch_size(torch, W):
    rng = np.random.default_rng(100 + W)
    C = 257
    ring = rh.Ring(C, W)
    ring.obs[:] = rng.integers(0, 1 << 32, size=(C, W), dtype=np.int64).astype(np.uint32)
    ring.next[:] = rng.integers(0, 1 << 32, size=(C, W), dtype=np.int64).astype(np.uint32)
    ring.action[:] = rng.integers(0, 1 << 32, size=C, dtype=np.int64).astype(np.uint32)
    ring.reward[:] = rng.integers(0, 1 << 32, size=C, dtype=np.int64).astype(np.uint32)      # any bits: NaN payloads travel unchanged
    ring.term[:] = rng.integers(0, 2, size=C).astype(np.uint8)
    for shift in (0, 1):
        dring = DeviceRing(torch, C, W, shift=shift)
        dring.load(ring)
        for i, B in enumerate(BATCHES):
            for count in (C // 2, C, 3 * C + 1):      # half full, full, wrapped
                ab = (4, 8)[(i + count) % 2]
                seed, step = 1000 + W, (1 << 33) + i
                got = c_sample(torch, dring, count, seed, step, B, ab, shift=shift)
                want = rh.sample(ring, count, seed, step, B, action_bytes=ab)
                same_batch(got, want, (W, shift, B, count))
                assert got["indices"].max() < min(count, C)
        dring.same_as(ring, "sampling writes nothing to the ring")


@pytest.mark.parametrize("W", (1, 4, 7, 16, 1025))
def test_an_empty_ring_gives_indices_minus_one_and_zeros(torch, W):
    ring = rh.Ring(5, W, fill=CANARY)
    dring = DeviceRing(torch, 5, W)
    for B, ab in ((1, 4), (65, 8), (257, 4)):
        got = c_sample(torch, dring, 0, 3, 9, B, ab)
        same_batch(got, rh.sample(ring, 0, 3, 9, B, action_bytes=ab), (W, B))
        assert (got["indices"] == -1).all() and not got["obs"].any() and not got["reward"].any() and not got["terminated"].any()


# ---- the front end ---------------------------------------------------------------------------------------------------------------------------------
def typed_chunk(torch, rng, K, N, shape, obs_dtype, action_dtype, reward_dtype, with_final=True):
    """A chunk as the tensors a rollout leaves, and the same as NumPy arrays for the twin."""
    def obs_of(lead):
        if obs_dtype == np.float32:
            return rng.standard_normal(lead + shape).astype(np.float32)
        return rng.integers(0, 200, size=lead + shape).astype(obs_dtype)

    host = dict(first=obs_of((N,)), obs=obs_of((K, N)), actions=rng.integers(0, 3, size=(K, N)).astype(action_dtype),
                reward=rng.standard_normal((K, N)).astype(reward_dtype), terminated=(rng.random((K, N)) < 0.2).astype(np.uint8))
    traj = {k: up(torch, host[k]) for k in ("obs", "actions", "reward", "terminated")}
    host["truncated"] = host["final"] = None
    if with_final:
        host["truncated"], host["final"] = (rng.random((K, N)) < 0.2).astype(np.uint8), obs_of((K, N))
        traj["truncated"], traj["final_obs"] = up(torch, host["truncated"]).bool(), up(torch, host["final"])
    return up(torch, host["first"]), traj, host


def twin_insert(ring, count, host):
    return rh.insert(ring, count, host["first"], host["obs"], host["actions"], host["reward"], host["terminated"], host["truncated"], host["final"])


def buffer_same_as(torch, buf, ring, what):
    for name, mine, theirs in (("obs", buf._obs, ring.obs), ("next", buf._next, ring.next), ("action", buf._action, ring.action),
                               ("reward", buf._reward, ring.reward)):
        assert np.array_equal(down(torch, mine.view(-1).view(torch.int32)), theirs.reshape(-1)), (what, name)
    assert np.array_equal(down(torch, buf._term, np.uint8), ring.term), what


def batch_same_as(torch, batch, want, buf, B, what):
    assert tuple(batch["obs"].shape) == (B,) + buf.obs_shape and batch["obs"].dtype == buf.obs_dtype and batch["actions"].dtype == buf.action_dtype
    assert batch["reward"].dtype == torch.float32 and batch["terminated"].dtype == torch.uint8 and batch["indices"].dtype == torch.int64
    assert np.array_equal(down(torch, batch["indices"], np.int64), want["indices"]), what
    assert np.array_equal(down(torch, batch["obs"].view(B, -1).view(torch.int32)).reshape(B, -1), want["obs"]), what
    assert np.array_equal(down(torch, batch["next_obs"].view(B, -1).view(torch.int32)).reshape(B, -1), want["next_obs"]), what
    if buf.action_dtype == torch.int64:
        assert np.array_equal(down(torch, batch["actions"], np.int64), want["actions"]), what
    else:
        assert np.array_equal(down(torch, batch["actions"].view(torch.int32)), want["actions"]), what
    assert np.array_equal(down(torch, batch["reward"].view(torch.int32)), want["reward"]), what
    assert np.array_equal(down(torch, batch["terminated"], np.uint8), want["terminated"]), what


@pytest.mark.parametrize("shape,obs_dtype,action_dtype,reward_dtype", [((4,), np.float32, np.int32, np.float64), ((6,), np.float32, np.int64, np.float32),
                                                                        ((), np.int32, np.int32, np.float32), ((), np.int64, np.int64, np.float64),
                                                                        ((3,), np.int64, np.int64, np.float64), ((4, 12, 12), np.uint8, np.int32, np.float32),
                                                                        ((1,), np.float32, np.float32, np.float64)])
def test_the_buffer_stores_and_draws_what_the_twin_does(torch, shape, obs_dtype, action_dtype, reward_dtype):
    import gym_amd

    rng = np.random.default_rng(7)
    tt = {np.float32: torch.float32, np.int32: torch.int32, np.int64: torch.int64, np.uint8: torch.uint8}
    C, K, N = 100, 3, 11
    buf = gym_amd.ReplayBuffer(C, shape, obs_dtype=tt[obs_dtype], action_dtype=tt[action_dtype], seed=21, device=0)
    ab = 8 if action_dtype == np.int64 else 4
    ring, count = rh.Ring(C, buf.W), 0
    assert len(buf) == 0 and buf.count == 0
    with pytest.raises(ValueError, match="empty"):
        buf.sample(4)
    for n in range(5):      # 165 rows: the ring wraps
        first, traj, host = typed_chunk(torch, rng, K, N, shape, obs_dtype, action_dtype, reward_dtype, with_final=n % 2 == 0)
        buf.add_chunk(first, traj)
        count = twin_insert(ring, count, host)
        assert buf.count == count and len(buf) == min(count, C)
        B = (7, 64, 257)[n % 3]
        batch_same_as(torch, buf.sample(B), rh.sample(ring, count, 21, n, B, action_bytes=ab), buf, B, (shape, n))
    # the flat add: K = 1 of the same rule
    first, traj, host = typed_chunk(torch, rng, 1, 9, shape, obs_dtype, action_dtype, reward_dtype, with_final=False)
    buf.add(first, traj["actions"][0], traj["reward"][0], traj["terminated"][0].bool(), traj["obs"][0])
    count = twin_insert(ring, count, host)
    buffer_same_as(torch, buf, ring, shape)
    # out=: the caller's tensors come back, filled
    out = buf.sample_buffers(33)
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    back = buf.sample(33, out=out)
    assert back is out and {k: v.data_ptr() for k, v in back.items()} == ptrs and buf.sample_step == 6
    batch_same_as(torch, back, rh.sample(ring, count, 21, 5, 33, action_bytes=ab), buf, 33, "out=")


def test_state_dict_round_trip_continues_bit_identically(torch):
    import gym_amd

    rng = np.random.default_rng(11)
    a = gym_amd.ReplayBuffer(50, (4,), seed=5, device=0)
    chunks = [typed_chunk(torch, rng, 2, 9, (4,), np.float32, np.int32, np.float64) for _ in range(6)]
    for first, traj, _ in chunks[:4]:
        a.add_chunk(first, traj)
        a.sample(16)
    state = a.state_dict()
    assert state["count"] == 72 and state["sample_step"] == 4 and state["seed"] == 5
    b = gym_amd.ReplayBuffer(50, (4,), seed=999, device=0)
    b.load_state_dict(state)
    c = gym_amd.ReplayBuffer(50, (4,), seed=0, device=0).enable_graph_capture()      # a restored buffer with device counters continues as well
    c.load_state_dict(state)
    for first, traj, _ in chunks[4:]:
        batches = []
        for buf in (a, b, c):
            buf.add_chunk(first, traj)
            batches.append(buf.sample(40))
        for other in batches[1:]:
            for key in batches[0]:
                assert torch.equal(batches[0][key], other[key]), key
    assert a.count == b.count == c.count == 108 and c.sample_step == 6 and len(c) == 50
    for x, y, z in zip((a._obs, a._next, a._action, a._reward, a._term), (b._obs, b._next, b._action, b._reward, b._term),
                       (c._obs, c._next, c._action, c._reward, c._term)):
        assert torch.equal(x, y) and torch.equal(x, z)
    with pytest.raises(ValueError, match="capacity"):
        gym_amd.ReplayBuffer(51, (4,), device=0).load_state_dict(state)


def test_insert_and_sample_recorded_once_and_replayed_three_times_equal_three_eager_rounds_of_the_twin(torch):
    import gym_amd

    rng = np.random.default_rng(13)
    C, K, N, B = 40, 2, 9, 65
    buf = gym_amd.ReplayBuffer(C, (6,), action_dtype=torch.int64, seed=77, device=0).enable_graph_capture()
    first, traj, host = typed_chunk(torch, rng, K, N, (6,), np.float32, np.int64, np.float64)
    out = buf.sample_buffers(B)
    side = torch.cuda.Stream()
    ring, count = rh.Ring(C, 6), 0
    with torch.cuda.stream(side):
        buf.add_chunk(first, traj)      # once outside the recording: the kernels' code is loaded
        buf.sample(B, out=out)
        side.synchronize()
        count = twin_insert(ring, count, host)
        batch_same_as(torch, out, rh.sample(ring, count, 77, 0, B, action_bytes=8), buf, B, "eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            buf.add_chunk(first, traj)
            buf.sample(B, out=out)
        for k in range(3):      # the recording itself ran nothing: the first replay is round 1
            fresh = typed_chunk(torch, rng, K, N, (6,), np.float32, np.int64, np.float64)
            first.copy_(fresh[0])
            for key in traj:
                traj[key].copy_(fresh[1][key])
            g.replay()
            side.synchronize()
            count = twin_insert(ring, count, fresh[2])
            batch_same_as(torch, out, rh.sample(ring, count, 77, 1 + k, B, action_bytes=8), buf, B, k)
    torch.cuda.current_stream().wait_stream(side)
    assert buf.count == count == 4 * K * N and buf.sample_step == 4 and len(buf) == C
    buffer_same_as(torch, buf, ring, "after the replays")


@pytest.mark.parametrize("W", (4, 7, 16, 1025))
def test_launch_counts_and_no_synchronisation(torch, W):
    """1 launch for an insert and 1 for a sample without state_dev, 2 + 2 with it — counted as the kernel nodes that the calls leave in a
    stream capture, which also shows that they neither synchronise nor allocate."""
    from gym_amd import replay

    hip = _hip()
    C, K, N, B = 64, 2, 8, 33
    i32 = dict(dtype=torch.int32, device="cuda:0")
    ring = [torch.zeros(C * W, **i32), torch.zeros(C * W, **i32), torch.zeros(C, **i32), torch.zeros(C, **i32), torch.zeros(C, dtype=torch.uint8, device="cuda:0")]
    first, obs, final = torch.zeros(N * W, **i32), torch.zeros(K * N * W, **i32), torch.zeros(K * N * W, **i32)
    act, rew = torch.zeros(K * N, dtype=torch.int64, device="cuda:0"), torch.zeros(K * N, dtype=torch.float64, device="cuda:0")
    term, trunc = (torch.zeros(K * N, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    state = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    outs = [torch.zeros(B, dtype=torch.int64, device="cuda:0"), torch.zeros(B * W, **i32), torch.zeros(B * W, **i32), torch.zeros(B, **i32),
            torch.zeros(B, **i32), torch.zeros(B, dtype=torch.uint8, device="cuda:0")]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    s, lib = side.cuda_stream, replay.lib
    rp = [x.data_ptr() for x in ring]

    def insert(st):
        return lambda: lib.mxv_replay_insert(s, C, W, K, N, first.data_ptr(), W, obs.data_ptr(), W, final.data_ptr(), W, act.data_ptr(), 8, rew.data_ptr(), 8,
                                             term.data_ptr(), trunc.data_ptr(), 0, st, *rp)

    def sample(st):
        return lambda: lib.mxv_replay_sample(s, C, W, B, *rp, 1, 16, 0, st, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), 4,
                                             outs[4].data_ptr(), outs[5].data_ptr())

    calls = ((insert(None), 1), (sample(None), 1), (insert(state.data_ptr()), 2), (sample(state.data_ptr()), 2))
    for call, _ in calls:                                                     # once outside a capture: the kernels' code is loaded
        assert call() == 0, lib.mxv_replay_last_error()
    side.synchronize()
    assert state.tolist() == [K * N, 1]
    for call, nodes in calls:
        rc, n = _captured_launches(hip, s, call)
        assert (rc, n) == (0, nodes), (rc, n, lib.mxv_replay_last_error())
    side.synchronize()


def test_a_real_chunk_stores_the_pre_step_and_the_final_observations(torch):
    from gym_amd.returns import pre_step_observations
    from gym_amd.rollout import DeviceRollout

    r = DeviceRollout("CartPole-v1", 64, seed=1, action_seed=2)
    r.reset(seed=3)
    r.synchronize()
    first = r.obs.clone()
    torch.cuda.synchronize()
    K, n = 32, r.num_envs
    traj = r.rollout_per_step(K, out=r.trajectory_buffers(K, layout="separate", want_final=True))
    buf = r.replay_buffer(K * n)
    assert buf.obs_shape == (4,) and buf.obs_dtype == torch.float32 and buf.action_dtype == r.action_dtype and buf.seed == 2
    r.ready()
    buf.add_chunk(first, traj)
    done = (traj["terminated"] != 0) | (traj["truncated"] != 0)
    assert int(done.sum()) > 0 and len(buf) == K * n
    pre = pre_step_observations(first, traj["obs"]).reshape(K * n, 4)
    nxt = torch.where(done.unsqueeze(-1), traj["final_obs"], traj["obs"]).reshape(K * n, 4)
    assert torch.equal(buf._obs.view(torch.int32), pre.view(torch.int32)) and torch.equal(buf._next.view(torch.int32), nxt.view(torch.int32))
    assert torch.equal(buf._action.long(), traj["actions"].reshape(-1).long()) and torch.equal(buf._reward, traj["reward"].reshape(-1).float())
    assert torch.equal(buf._term, (traj["terminated"].reshape(-1) != 0).to(torch.uint8))
    batch = buf.sample(256)
    k = batch["indices"]
    assert torch.equal(batch["obs"], pre[k]) and torch.equal(batch["next_obs"], nxt[k]) and torch.equal(batch["terminated"], buf._term[k])
    r.close()


def test_a_tabular_chunk_is_stored_as_two_dword_rows(torch):
    """TabularRollout.replay_buffer(): int64 state indices are rows of two dwords.  The tabular engine writes no final_obs, so its traj
    is refused as it stands and taken without "truncated" for a chunk in which no step was truncated."""
    from gym_amd.returns import pre_step_observations
    from gym_amd.toy_text import TabularRollout

    r = TabularRollout("FrozenLake-v1", 64, seed=1, action_seed=2)
    first = r.reset(seed=3).clone()
    K, n = 16, r.num_envs
    traj = r.rollout_per_step(K, out=r.trajectory_buffers(K, layout="separate"))
    r.ready()
    buf = r.replay_buffer(2 * K * n)
    assert buf.obs_shape == () and buf.obs_dtype == torch.int64 and buf.W == 2 and buf.action_dtype == torch.int64 and buf.seed == 2
    with pytest.raises(ValueError, match='no "final_obs"'):
        buf.add_chunk(first, traj)
    assert int(traj["truncated"].sum()) == 0 and int(traj["terminated"].sum()) > 0      # the time limit is 100 steps
    buf.add_chunk(first, {k: traj[k] for k in ("obs", "actions", "reward", "terminated")})
    R = K * n
    assert len(buf) == R
    assert torch.equal(buf._obs.view(-1)[:R], pre_step_observations(first, traj["obs"]).reshape(-1)) and torch.equal(buf._next.view(-1)[:R], traj["obs"].reshape(-1))
    assert torch.equal(buf._action[:R].long(), traj["actions"].reshape(-1)) and torch.equal(buf._reward[:R], traj["reward"].reshape(-1).float())
    assert not buf._obs[R:].any() and not buf._term[R:].any()
    batch = buf.sample(100)
    assert batch["obs"].dtype == torch.int64 and tuple(batch["obs"].shape) == (100,) and torch.equal(batch["obs"], buf._obs.view(-1)[batch["indices"]])
    r.close()


def test_the_example_repeats_itself(torch, capsys):
    """examples/dqn_replay_cartpole.py has no torch generator: two runs give the same history, number for number; every loss is finite."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import dqn_replay_cartpole
    finally:
        sys.path.pop(0)
    kw = dict(num_envs=64, iterations=3, K=8, updates=2, batch=128, capacity=1024)
    first = dqn_replay_cartpole.train(**kw)
    assert "sample steps drawn" in capsys.readouterr().out
    again = dqn_replay_cartpole.train(**kw, verbose=False)
    assert first == again and len(first) == 3
    for row in first:
        assert np.isfinite(list(row.values())).all() and row["td_abs_max"] >= row["td_abs_mean"] > 0.0 and row["stored"] > 0


def test_python_argument_errors(torch):
    import gym_amd

    rng = np.random.default_rng(0)
    for kw, what in ((dict(capacity=0), "capacity"), (dict(capacity=(1 << 31) + 1), "2\\^31"), (dict(obs_shape=(3,), obs_dtype=torch.uint8), "multiple of 4"),
                     (dict(obs_dtype=torch.float64), "obs_dtype"), (dict(action_dtype=torch.int16), "action_dtype"), (dict(seed=-1), "seed"),
                     (dict(obs_shape=(70000,)), "beyond 65536"), (dict(capacity=1 << 31, obs_shape=(1024,)), "2\\^40")):
        args = dict(capacity=16, obs_shape=(4,), device=0)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            gym_amd.ReplayBuffer(**args)
    buf = gym_amd.ReplayBuffer(32, (4,), device=0)
    first, traj, _ = typed_chunk(torch, rng, 2, 8, (4,), np.float32, np.int32, np.float64)
    bad = [(dict(traj={k: v for k, v in traj.items() if k != "final_obs"}), 'no "final_obs"'), (dict(traj={k: v for k, v in traj.items() if k != "reward"}), 'no "reward"'),
           (dict(first=first[:4]), "shape"), (dict(first=first.double()), "float32"), (dict(first=first.cpu()), "device tensor"),
           (dict(traj=dict(traj, actions=traj["actions"].long())), "int32"), (dict(traj=dict(traj, reward=traj["reward"].half())), "float32 or"),
           (dict(traj=dict(traj, terminated=traj["terminated"].float())), "uint8"), (dict(traj=dict(traj, obs=traj["obs"][:, :, :3])), "shape"),
           (dict(traj=dict(traj, final_obs=traj["final_obs"][:1])), "shape"), (dict(traj=[1]), "dict")]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            buf.add_chunk(kw.get("first", first), kw.get("traj", traj))
    big = typed_chunk(torch, rng, 5, 8, (4,), np.float32, np.int32, np.float64)
    with pytest.raises(ValueError, match="exceed the capacity"):
        buf.add_chunk(big[0], big[1])
    assert buf.count == 0
    buf.add_chunk(first, traj)
    for kw, what in ((dict(batch_size=0), "batch_size"), (dict(batch_size=4, out={"obs": first}), "out must be a dict"),
                     (dict(batch_size=4, out=buf.sample_buffers(5)), "shape")):
        with pytest.raises(ValueError, match=what):
            buf.sample(**kw)
    overlapping = buf.sample_buffers(4)
    overlapping["next_obs"] = overlapping["obs"]
    with pytest.raises(ValueError, match="overlap"):
        buf.sample(4, out=overlapping)
    from gym_amd.toy_text import BlackjackRollout

    bj = BlackjackRollout(64, seed=1, action_seed=2)
    with pytest.raises(ValueError, match="replay_buffer"):
        bj.replay_buffer(128)
    bj.close()
