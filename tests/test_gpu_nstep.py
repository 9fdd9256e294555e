"""gym_amd.NStepReplayBuffer / NStepPrioritizedReplayBuffer and the calls of include/mxv_nstep.h on the device against tests/nstep_host.py,
the NumPy twin of the rule: every array compared bit for bit.  Window positions (every K around n, every N around a wave and a tile, every
class of window planted and asserted from the twin's classification), every row width and alignment (the straight-line, loop, 16-byte and
dword instantiations), dtypes, the ring wrapping inside a chunk, grids that stride, n = 1 against ReplayBuffer, non-finite rewards,
sample and the gather, graph capture, checkpoints, the prioritised variant, a real CartPole chunk, the launch counts, the example."""
import os
import sys

import numpy as np
import pytest

import nstep_host as nh
import replay_host as rh
from conftest import ROOT
from test_gpu_ppo import _captured_launches, _hip
from test_gpu_replay import CANARY, CANARY_FINAL, DeviceRing, batch_same_as, buffer_same_as, down, rows_on_device, typed_chunk, up

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


class NDeviceRing(DeviceRing):
    """The six ring arrays on the device, filled with the canary."""

    def __init__(self, torch, C, W, shift=0):
        super().__init__(torch, C, W, shift)
        self.discount = up(torch, np.full(C, CANARY, np.uint32))

    def same_as(self, ring, what):
        super().same_as(ring, what)
        mine = down(self.torch, self.discount)
        bad = np.flatnonzero(mine != ring.discount)
        assert bad.size == 0, (what, "discount", bad[:8], mine[bad[:8]], ring.discount[bad[:8]])


def planted_chunk(rng, n, K, N, W, reward_dtype, action_dtype, plant, with_final=True, p=None, wild=True):
    """A chunk with random flags (probability p per step and kind) whose env 0 is planted: plant 0 — no flag at all (a full window where
    K >= n, a window cut by the chunk's end); 1 — terminated at step min(n, K) - 1 alone (done at the window's last step where K >= n,
    a cut by termination and a window done at its first step); 2 — truncated at step 0 alone.  final_obs rows of steps that did not end
    hold CANARY_FINAL: they must not be read."""
    p = min(0.25, 1.0 / n) if p is None else p
    obs = rng.integers(0, 1 << 31, size=(K, N, W), dtype=np.int64).astype(np.uint32)
    first = rng.integers(0, 1 << 31, size=(N, W), dtype=np.int64).astype(np.uint32)
    term = ((rng.random((K, N)) < p) * rng.integers(1, 256, size=(K, N))).astype(np.uint8)
    trunc = ((rng.random((K, N)) < p) * rng.integers(1, 256, size=(K, N))).astype(np.uint8) if with_final else None
    if plant is not None:
        term[:, 0] = 0
        if with_final:
            trunc[:, 0] = 0
        if plant == 1:
            term[min(n, K) - 1, 0] = 255
        elif plant == 2 and with_final:
            trunc[0, 0] = 1
    final = None
    if with_final:
        final = rng.integers(0, 1 << 31, size=(K, N, W), dtype=np.int64).astype(np.uint32)
        final[(term == 0) & (trunc == 0)] = CANARY_FINAL
    actions = rng.integers(-3, 4, size=(K, N)).astype(action_dtype)
    reward = (rng.standard_normal((K, N)) * 100).astype(reward_dtype)
    if wild:
        flat = reward.reshape(-1)
        flat[5::23] = np.nan
        flat[7::29] = np.inf
        flat[11::31] = -np.inf
        if reward_dtype == np.float64:
            flat[3::17] = 1.0 + 2.0 ** -24          # a tie of the float32 rounding where it stands alone
            flat[13::37] = 1e300                    # overflows to +Inf in float32, and to Inf in a float64 sum of two
    return first, obs, actions, reward, term, trunc, final


def c_insert(torch, dring, count, n, gamma, chunk, *, pad=0, shift=0, state=None, stream=None):
    """mxv_nstep_insert through ctypes on device copies of `chunk`; -> the status."""
    from gym_amd import nstep

    first, obs, actions, reward, term, trunc, final = chunk
    K, N, W = obs.shape
    keep = [rows_on_device(torch, first, pad, shift), rows_on_device(torch, obs.reshape(K * N, W), pad, shift)]
    fin = rows_on_device(torch, final.reshape(K * N, W), pad, shift) if final is not None else (None, None, 0)
    a, r, te = up(torch, actions), up(torch, reward), up(torch, term)
    tr = None if trunc is None else up(torch, trunc)
    torch.cuda.synchronize()
    rc = nstep.lib.mxv_nstep_insert(stream, dring.C, W, K, N, keep[0][1], keep[0][2], keep[1][1], keep[1][2], fin[1], fin[2], a.data_ptr(),
                                    actions.dtype.itemsize, r.data_ptr(), reward.dtype.itemsize, te.data_ptr(), None if tr is None else tr.data_ptr(),
                                    count, None if state is None else state.data_ptr(), *dring.pointers(), n, gamma, dring.discount.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, nstep.lib.mxv_nstep_last_error()
    return rc


def twin_insert(ring, count, n, gamma, chunk):
    first, obs, actions, reward, term, trunc, final = chunk
    return nh.insert(ring, count, n, gamma, first, obs, actions, reward, term, trunc, final)


def claimed(n, K):
    """The classes of window a chunk of K steps can hold at n, which the planted env 0 of three chunks then must show."""
    c = {"first"}
    if K >= n:
        c |= {"full", "last"}
    if n >= 2:
        c |= {"terminated", "truncated", "chunk"}
    return c


def seen(n, chunk):
    c = nh.classes(n, chunk[3], chunk[4], chunk[5])
    return {k for k, m in c.items() if m.any()}


# ---- window positions ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 3, 5, 64))
def test_every_window_position_equals_the_twin(torch, n):
    rng = np.random.default_rng(1000 + n)
    gamma = (0.99, 0.9, 0.997, 0.5, 0.98)[n % 5]
    cases = 0
    for K in sorted({1, 2, n - 1, n, n + 1} - {0}):
        for N in (1, 63, 64, 65, 257):
            cases += 1
            W = (4, 9, 3, 12)[cases % 4]      # a straight-line narrow row, a wide dword row, another narrow one, a wide 16-byte row
            R = K * N
            C = 2 * R + 3                     # the third chunk wraps
            count = ((1 << 32) - 5, 0, 7)[cases % 3]
            twin, dring = nh.Ring(C, W, fill=CANARY), NDeviceRing(torch, C, W)
            classes = set()
            for plant in range(3):            # three chunks back to back
                chunk = planted_chunk(rng, n, K, N, W, (np.float64, np.float32)[(plant + cases) % 2], (np.int64, np.int32, np.float32)[(plant + cases) % 3], plant)
                classes |= seen(n, chunk)
                c_insert(torch, dring, count, n, gamma, chunk)
                count = twin_insert(twin, count, n, gamma, chunk)
            assert classes >= claimed(n, K), (n, K, N, classes)
            dring.same_as(twin, (n, K, N, W))
            for x in (dring.obs, dring.next):
                assert not (down(torch, x) == CANARY_FINAL).any(), (n, K, N)      # no final_obs row of a step that did not end was read
    assert cases >= (10 if n == 1 else 15) and claimed(n, n + 1) == ({"first", "full", "last"} if n == 1 else {"first", "full", "last", "terminated", "truncated", "chunk"})


# ---- row widths and alignment ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", (1, 2, 3, 4, 5, 6, 8, 9, 1024, 1028, 1029, 2049))
def test_every_row_width_aligned_and_one_dword_off(torch, W):
    rng = np.random.default_rng(2000 + W)
    n, gamma, K, N = 3, 0.95, 4, 65      # 260 rows: two tiles of the narrow kernels
    R = K * N
    classes = set()
    for pad, shift, ring_shift in ((0, 0, 0), (3, 1, 0), (0, 0, 1)):      # packed and aligned; strided sources one dword off; the ring one dword off
        C = R + 7
        twin, dring = nh.Ring(C, W, fill=CANARY), NDeviceRing(torch, C, W, shift=ring_shift)
        count = C - 9
        for plant in (0, 1, 2):
            chunk = planted_chunk(rng, n, K, N, W, np.float64, np.int64, plant)
            classes |= seen(n, chunk)
            c_insert(torch, dring, count, n, gamma, chunk, pad=pad, shift=shift)
            count = twin_insert(twin, count, n, gamma, chunk)
        dring.same_as(twin, (W, pad, shift, ring_shift))
        for x in (dring.obs, dring.next):
            assert not (down(torch, x) == CANARY_FINAL).any(), (W, pad, shift)
    assert classes >= claimed(n, K) and len(claimed(n, K)) == 6


# ---- the ring --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", (4, 9))
def test_the_ring_wraps_inside_a_chunk(torch, W):
    rng = np.random.default_rng(3000 + W)
    n, gamma, K, N = 3, 0.9, 4, 33
    R = K * N
    for C in (R, R + 1):
        for count in (C - 1, C - 64, 3 * C + R // 2, (1 << 63) - R):
            twin, dring = nh.Ring(C, W, fill=CANARY), NDeviceRing(torch, C, W)
            chunk = planted_chunk(rng, n, K, N, W, np.float32, np.int32, 1)
            c_insert(torch, dring, count, n, gamma, chunk)
            twin_insert(twin, count, n, gamma, chunk)
            dring.same_as(twin, (W, C, count))
            if C > R:
                assert (twin.discount == CANARY).sum() == 1      # the one slot outside the chunk kept the canary


@pytest.mark.parametrize("W,K,N", [(1, 3, 174763), (9, 5, 3277)])
def test_a_grid_that_strides(torch, W, K, N):
    """The smallest chunks beyond the grid caps: 2048 tiles of 256 rows for the narrow kernels, 16384 rows for the wide ones."""
    assert (K * N == 2048 * 256 + 1) if W == 1 else (K * N == 16384 + 1)
    rng = np.random.default_rng(4000 + W)
    n, gamma, R = 3, 0.99, K * N
    C = R + 2
    twin, dring = nh.Ring(C, W, fill=CANARY), NDeviceRing(torch, C, W)
    chunk = planted_chunk(rng, n, K, N, W, np.float32, np.int32, 0)
    c_insert(torch, dring, 5, n, gamma, chunk)
    twin_insert(twin, 5, n, gamma, chunk)
    dring.same_as(twin, (W, K, N))
    assert seen(n, chunk) >= claimed(n, K) and len(claimed(n, K)) == 6


# ---- non-finite rewards ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", (4, 9))
def test_a_non_finite_reward_of_a_later_episode_reaches_no_earlier_row(torch, W):
    rng = np.random.default_rng(5000 + W)
    n, gamma, K, N = 4, 0.9, 9, 70
    first, obs, actions, reward, term, trunc, final = planted_chunk(rng, n, K, N, W, np.float64, np.int64, None, p=0.0, wild=False)
    term[3, :35] = 1
    trunc[3, 35:] = 9
    final[3] = rng.integers(0, 1 << 31, size=(N, W), dtype=np.int64).astype(np.uint32)
    R, early = K * N, 4 * N
    clean_twin, clean = nh.Ring(R, W, fill=CANARY), NDeviceRing(torch, R, W)
    c_insert(torch, clean, 0, n, gamma, (first, obs, actions, reward, term, trunc, final))
    twin_insert(clean_twin, 0, n, gamma, (first, obs, actions, reward, term, trunc, final))
    clean.same_as(clean_twin, "clean")
    assert np.isfinite(down(torch, clean.reward).view(np.float32)).all()
    for poison in (np.nan, np.inf, -np.inf):
        dirty_reward = reward.copy()
        dirty_reward[4] = poison      # the first step of every env's next episode
        twin, dring = nh.Ring(R, W, fill=CANARY), NDeviceRing(torch, R, W)
        c_insert(torch, dring, 0, n, gamma, (first, obs, actions, dirty_reward, term, trunc, final))
        twin_insert(twin, 0, n, gamma, (first, obs, actions, dirty_reward, term, trunc, final))
        dring.same_as(twin, poison)      # inside a window the value propagates as in the twin
        for mine, theirs in ((dring.reward, clean.reward), (dring.discount, clean.discount), (dring.action, clean.action)):
            assert np.array_equal(down(torch, mine)[:early], down(torch, theirs)[:early]), poison
        assert np.array_equal(down(torch, dring.next).reshape(R, W)[:early], down(torch, clean.next).reshape(R, W)[:early])
        assert np.array_equal(down(torch, dring.term, np.uint8)[:early], down(torch, clean.term, np.uint8)[:early])
        assert not np.isfinite(down(torch, dring.reward).view(np.float32)[early:early + N]).any()


# ---- the gather ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 63, 257, 2048 * 256 + 1))
def test_the_gather_on_hand_made_indices(torch, B):
    from gym_amd import nstep

    rng = np.random.default_rng(B)
    C = 1000
    ring = rng.integers(0, 1 << 32, size=C, dtype=np.int64).astype(np.uint32)      # any bits: NaN payloads travel unchanged
    idx = rng.integers(0, C, size=B).astype(np.int64)
    wild = np.array([-1, C, -2, C - 1, 0, 1 << 40, -(1 << 62), (1 << 63) - 1, C + 1, -1], np.int64)
    idx[:min(B, wild.size)] = wild[:B]
    d_ring, d_idx, out = up(torch, ring), up(torch, idx), up(torch, np.full(B, CANARY, np.uint32))
    torch.cuda.synchronize()
    rc = nstep.lib.mxv_nstep_gather(None, C, B, d_ring.data_ptr(), d_idx.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, nstep.lib.mxv_nstep_last_error()
    got, want = down(torch, out), nh.gather(ring, idx)
    assert np.array_equal(got, want)
    assert got[0] == 0 and (B < 2 or got[1] == 0x7FC00000) and (B < 3 or got[2] == 0x7FC00000)


# ---- the front end ---------------------------------------------------------------------------------------------------------------------------------
def nstep_twin_insert(ring, count, n, gamma, host):
    return nh.insert(ring, count, n, gamma, host["first"], host["obs"], host["actions"], host["reward"], host["terminated"], host["truncated"], host["final"])


def nstep_buffer_same_as(torch, buf, ring, what):
    buffer_same_as(torch, buf, ring, what)
    assert np.array_equal(down(torch, buf._discount.view(torch.int32)), ring.discount), (what, "discount")


@pytest.mark.parametrize("shape,obs_dtype,action_dtype,reward_dtype", [((4,), np.float32, np.int32, np.float64), ((6,), np.float32, np.int64, np.float32),
                                                                        ((), np.int64, np.int64, np.float64), ((3,), np.int64, np.int32, np.float32),
                                                                        ((4, 12, 12), np.uint8, np.int32, np.float32), ((1,), np.float32, np.float32, np.float64)])
def test_the_buffer_stores_and_draws_what_the_twin_does(torch, shape, obs_dtype, action_dtype, reward_dtype):
    import gym_amd

    rng = np.random.default_rng(7)
    tt = {np.float32: torch.float32, np.int32: torch.int32, np.int64: torch.int64, np.uint8: torch.uint8}
    C, K, N, n, gamma = 100, 3, 11, 3, 0.97
    buf = gym_amd.NStepReplayBuffer(C, shape, n, gamma, obs_dtype=tt[obs_dtype], action_dtype=tt[action_dtype], seed=21, device=0)
    assert isinstance(buf, gym_amd.ReplayBuffer) and buf.n_step == n and buf.gamma == gamma
    ab = 8 if action_dtype == np.int64 else 4
    ring, count = nh.Ring(C, buf.W), 0
    with pytest.raises(ValueError, match="empty"):
        buf.sample(4)
    for k in range(5):      # 165 rows: the ring wraps; every other chunk has neither final_obs nor truncated; bool flags throughout
        first, traj, host = typed_chunk(torch, rng, K, N, shape, obs_dtype, action_dtype, reward_dtype, with_final=k % 2 == 0)
        traj["terminated"] = traj["terminated"].bool()
        buf.add_chunk(first, traj)
        count = nstep_twin_insert(ring, count, n, gamma, host)
        assert buf.count == count and len(buf) == min(count, C)
        B = (7, 64, 257)[k % 3]
        batch = buf.sample(B)
        want = rh.sample(ring, count, 21, k, B, action_bytes=ab)
        batch_same_as(torch, batch, want, buf, B, (shape, k))
        assert batch["discount"].dtype == torch.float32 and tuple(batch["discount"].shape) == (B,)
        assert np.array_equal(down(torch, batch["discount"].view(torch.int32)), ring.discount[want["indices"]]), (shape, k)
    # the flat add: K = 1 of the same rule, so the discount is gamma itself
    first, traj, host = typed_chunk(torch, rng, 1, 9, shape, obs_dtype, action_dtype, reward_dtype, with_final=False)
    buf.add(first, traj["actions"][0], traj["reward"][0], traj["terminated"][0].bool(), traj["obs"][0])
    s = rh.slots(count, 9, C)
    count = nstep_twin_insert(ring, count, n, gamma, host)
    nstep_buffer_same_as(torch, buf, ring, shape)
    assert (ring.discount[s].view(np.float32) == np.float32(gamma)).all()
    # out=: the caller's tensors come back, filled
    out = buf.sample_buffers(33)
    assert "discount" in out
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    back = buf.sample(33, out=out)
    assert back is out and {k: v.data_ptr() for k, v in back.items()} == ptrs and buf.sample_step == 6
    want = rh.sample(ring, count, 21, 5, 33, action_bytes=ab)
    batch_same_as(torch, back, want, buf, 33, "out=")
    assert np.array_equal(down(torch, back["discount"].view(torch.int32)), ring.discount[want["indices"]])


def test_one_step_is_the_replay_buffer_bit_for_bit(torch):
    import gym_amd

    rng = np.random.default_rng(9)
    for shape, W_note in (((4,), "narrow"), ((20,), "wide")):
        one = gym_amd.ReplayBuffer(64, shape, seed=3, device=0)
        nst = gym_amd.NStepReplayBuffer(64, shape, 1, 0.99, seed=3, device=0)
        for k in range(4):
            first, traj, _ = typed_chunk(torch, rng, 3, 7, shape, np.float32, np.int32, (np.float32, np.float64)[k % 2], with_final=k != 1)
            if k == 2:
                traj["reward"].view(-1)[::4] = float("nan")
                traj["reward"].view(-1)[1::5] = float("inf")
            for buf in (one, nst):
                buf.add_chunk(first, traj)
        first, traj, _ = typed_chunk(torch, rng, 1, 9, shape, np.float32, np.int32, np.float32, with_final=False)
        for buf in (one, nst):
            buf.add(first, traj["actions"][0], traj["reward"][0], traj["terminated"][0], traj["obs"][0])
        for x, y in zip((one._obs, one._next, one._action, one._term), (nst._obs, nst._next, nst._action, nst._term)):
            assert torch.equal(x, y), W_note
        assert torch.equal(one._reward.view(torch.int32), nst._reward.view(torch.int32)), W_note
        assert one.count == nst.count == 93 and bool((nst._discount == np.float32(0.99)).all())
        a, b = one.sample(50), nst.sample(50)
        for key in a:
            assert torch.equal(a[key].view(torch.int32) if a[key].dtype == torch.float32 else a[key], b[key].view(torch.int32) if b[key].dtype == torch.float32 else b[key]), key


@pytest.mark.parametrize("prioritized", (False, True))
def test_sample_is_the_parents_with_the_discount_of_the_drawn_slots(torch, prioritized):
    import gym_amd

    rng = np.random.default_rng(11)
    kw = dict(seed=5, device=0)
    if prioritized:
        buf, parent = gym_amd.NStepPrioritizedReplayBuffer(80, (4,), 3, 0.9, alpha=0.7, **kw), gym_amd.PrioritizedReplayBuffer(80, (4,), alpha=0.1, **kw)
    else:
        buf, parent = gym_amd.NStepReplayBuffer(80, (4,), 3, 0.9, **kw), gym_amd.ReplayBuffer(80, (4,), **kw)
    for k in range(3):
        first, traj, _ = typed_chunk(torch, rng, 4, 9, (4,), np.float32, np.int32, np.float64)
        buf.add_chunk(first, traj)
        if prioritized and k == 1:
            batch = buf.sample(32)
            buf.update_priorities(batch["indices"], torch.linspace(0.0, 3.0, 32, device="cuda:0"))
    parent.load_state_dict(buf.state_dict())      # the same ring, tree, seed and step under the parent's sampler
    distinct = set()
    for B in (5, 64, 300):
        mine, theirs = buf.sample(B), parent.sample(B)
        assert set(mine) == set(theirs) | {"discount"}
        for key in theirs:
            assert torch.equal(mine[key].view(torch.int32) if mine[key].dtype == torch.float32 else mine[key],
                               theirs[key].view(torch.int32) if theirs[key].dtype == torch.float32 else theirs[key]), (key, B)
        assert torch.equal(mine["discount"].view(torch.int32), buf._discount[mine["indices"]].view(torch.int32)), B
        distinct |= set(mine["discount"].tolist())
    assert len(distinct) >= 3 and buf.sample_step == parent.sample_step      # 0.9, 0.81 and 0.729 were all drawn
    with pytest.raises(ValueError, match="discount"):
        buf.sample(4, out=parent.sample_buffers(4))


@pytest.mark.parametrize("prioritized", (False, True))
def test_an_empty_ring_under_device_counters_gives_discount_zero(torch, prioritized):
    import gym_amd

    cls = gym_amd.NStepPrioritizedReplayBuffer if prioritized else gym_amd.NStepReplayBuffer
    buf = cls(16, (4,), 2, 0.5, device=0).enable_graph_capture()
    out = buf.sample_buffers(70)
    out["discount"].fill_(7.0)
    batch = buf.sample(70, out=out)
    assert bool((batch["indices"] == -1).all()) and not batch["discount"].view(torch.int32).any() and not batch["reward"].view(torch.int32).any()


def test_insert_and_sample_recorded_once_and_replayed_three_times_equal_three_eager_rounds(torch):
    import gym_amd

    rng = np.random.default_rng(13)
    C, K, N, B, n, gamma = 40, 4, 9, 65, 3, 0.9      # 36 rows a round: the ring wraps in the second
    buf = gym_amd.NStepReplayBuffer(C, (6,), n, gamma, action_dtype=torch.int64, seed=77, device=0).enable_graph_capture()
    eager = gym_amd.NStepReplayBuffer(C, (6,), n, gamma, action_dtype=torch.int64, seed=77, device=0)
    first, traj, host = typed_chunk(torch, rng, K, N, (6,), np.float32, np.int64, np.float64)
    out = buf.sample_buffers(B)
    side = torch.cuda.Stream()
    ring, count = nh.Ring(C, 6), 0

    def check(step, what):
        want = rh.sample(ring, count, 77, step, B, action_bytes=8)
        batch_same_as(torch, out, want, buf, B, what)
        assert np.array_equal(down(torch, out["discount"].view(torch.int32)), ring.discount[want["indices"]]), what
        other = eager.sample(B)
        for key in other:
            assert torch.equal(other[key].view(torch.int32) if other[key].dtype == torch.float32 else other[key],
                               out[key].view(torch.int32) if out[key].dtype == torch.float32 else out[key]), (what, key)

    with torch.cuda.stream(side):
        buf.add_chunk(first, traj)      # once outside the recording: the kernels' code is loaded
        buf.sample(B, out=out)
        side.synchronize()
        eager.add_chunk(first, traj)
        count = nstep_twin_insert(ring, count, n, gamma, host)
        check(0, "eager")
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
            eager.add_chunk(first, traj)
            count = nstep_twin_insert(ring, count, n, gamma, fresh[2])
            check(1 + k, k)
    torch.cuda.current_stream().wait_stream(side)
    assert buf.count == count == 4 * K * N and buf.sample_step == 4 and len(buf) == C
    nstep_buffer_same_as(torch, buf, ring, "after the replays")
    nstep_buffer_same_as(torch, eager, ring, "eager")


@pytest.mark.parametrize("prioritized", (False, True))
def test_state_dict_round_trip_continues_bit_identically(torch, prioritized):
    import gym_amd

    rng = np.random.default_rng(17)
    cls = gym_amd.NStepPrioritizedReplayBuffer if prioritized else gym_amd.NStepReplayBuffer
    a = cls(50, (4,), 3, 0.95, seed=5, device=0)
    chunks = [typed_chunk(torch, rng, 2, 9, (4,), np.float32, np.int32, np.float64) for _ in range(6)]
    for first, traj, _ in chunks[:4]:
        a.add_chunk(first, traj)
        a.sample(16)
    state = a.state_dict()
    assert state["count"] == 72 and state["sample_step"] == 4 and state["n_step"] == 3 and state["gamma"] == 0.95
    assert torch.equal(state["discount"], a._discount) and state["discount"].data_ptr() != a._discount.data_ptr()
    b = cls(50, (4,), 7, 0.5, seed=999, device=0)      # another window: the state brings its own
    b.load_state_dict(state)
    c = cls(50, (4,), 1, 1.0, seed=0, device=0).enable_graph_capture()
    c.load_state_dict(state)
    assert (b.n_step, b.gamma, c.n_step, c.gamma) == (3, 0.95, 3, 0.95)
    for first, traj, _ in chunks[4:]:
        batches = []
        for buf in (a, b, c):
            buf.add_chunk(first, traj)
            batches.append(buf.sample(40))
        for other in batches[1:]:
            for key in batches[0]:
                assert torch.equal(batches[0][key].view(torch.int32) if batches[0][key].dtype == torch.float32 else batches[0][key],
                                   other[key].view(torch.int32) if other[key].dtype == torch.float32 else other[key]), key
    assert a.count == b.count == c.count == 108 and c.sample_step == 6
    for x, y, z in zip((a._obs, a._next, a._action, a._reward, a._term, a._discount), (b._obs, b._next, b._action, b._reward, b._term, b._discount),
                       (c._obs, c._next, c._action, c._reward, c._term, c._discount)):
        assert torch.equal(x, y) and torch.equal(x, z)
    plain = gym_amd.ReplayBuffer(50, (4,), device=0).state_dict()
    with pytest.raises(ValueError, match="the state has no"):
        cls(50, (4,), 3, 0.95, device=0).load_state_dict(plain)


def test_the_prioritised_variant_keeps_the_parents_tree(torch):
    import gym_amd

    rng = np.random.default_rng(19)
    kw = dict(alpha=0.6, eps=1e-6, seed=4, device=0)
    nst, one = gym_amd.NStepPrioritizedReplayBuffer(60, (4,), 3, 0.9, **kw), gym_amd.PrioritizedReplayBuffer(60, (4,), **kw)
    assert [c.__name__ for c in type(nst).__mro__[:4]] == ["NStepPrioritizedReplayBuffer", "PrioritizedReplayBuffer", "NStepReplayBuffer", "ReplayBuffer"]
    ring, count = nh.Ring(60, 4), 0
    for k in range(4):      # 108 rows: the ring wraps
        first, traj, host = typed_chunk(torch, rng, 3, 9, (4,), np.float32, np.int32, np.float64)
        for buf in (nst, one):
            buf.add_chunk(first, traj)
        count = nstep_twin_insert(ring, count, 3, 0.9, host)
        if k == 1:
            idx = torch.arange(0, 40, device="cuda:0")
            td = torch.linspace(0.0, 5.0, 40, device="cuda:0")
            for buf in (nst, one):
                buf.update_priorities(idx, td)
        assert torch.equal(nst._leaf, one._leaf) and torch.equal(nst._node, one._node) and torch.equal(nst._qmax, one._qmax), k
    nstep_buffer_same_as(torch, nst, ring, "prioritised")
    a, b = nst.sample(128, beta=0.5), one.sample(128, beta=0.5)
    assert torch.equal(a["indices"], b["indices"]) and torch.equal(a["weights"], b["weights"]) and torch.equal(a["obs"], b["obs"])
    assert torch.equal(a["discount"].view(torch.int32), nst._discount[a["indices"]].view(torch.int32))


def test_a_real_cartpole_chunk_through_the_rollouts_factory(torch):
    from gym_amd.rollout import DeviceRollout

    r = DeviceRollout("CartPole-v1", 64, seed=1, action_seed=2)
    r.reset(seed=3)
    r.synchronize()
    first = r.obs.clone()
    torch.cuda.synchronize()
    K, N, n, gamma = 32, r.num_envs, 3, 0.99
    traj = r.rollout_per_step(K, out=r.trajectory_buffers(K, layout="separate", want_final=True))
    buf = r.nstep_replay_buffer(K * N, n, gamma)
    pri = r.nstep_replay_buffer(K * N, n, gamma, prioritized=True, alpha=0.5, eps=1e-3, seed=9)
    assert type(buf).__name__ == "NStepReplayBuffer" and type(pri).__name__ == "NStepPrioritizedReplayBuffer"
    assert buf.obs_shape == (4,) and buf.obs_dtype == torch.float32 and buf.action_dtype == r.action_dtype and buf.seed == 2
    assert (pri.alpha, pri.eps, pri.seed, pri.n_step, pri.gamma) == (0.5, 1e-3, 9, n, gamma)
    r.ready()
    buf.add_chunk(first, traj)
    pri.add_chunk(first, traj)
    host = {k: traj[k].cpu().numpy() for k in ("obs", "actions", "reward", "terminated", "truncated", "final_obs")}
    done = (host["terminated"] != 0) | (host["truncated"] != 0)
    assert done.sum() > 0 and (host["terminated"] != 0).sum() > 0
    ring = nh.Ring(K * N, 4)
    nh.insert(ring, 0, n, gamma, first.cpu().numpy(), host["obs"], host["actions"], host["reward"], host["terminated"], host["truncated"], host["final_obs"])
    nstep_buffer_same_as(torch, buf, ring, "cartpole")
    nstep_buffer_same_as(torch, pri, ring, "cartpole, prioritised")
    c = nh.classes(n, host["reward"], host["terminated"], host["truncated"])
    assert c["full"].any() and c["terminated"].any() and c["chunk"].any() and c["first"].any() and c["last"].any()
    # CartPole pays 1 per step: the return of a window of m steps is 1 + gamma + .. + gamma^(m-1)
    steps = nh.windows(n, gamma, host["reward"], host["terminated"], host["truncated"])["e"] - np.arange(K)[:, None] + 1
    assert np.allclose(ring.reward.view(np.float32), ((1 - gamma ** steps) / (1 - gamma)).reshape(-1), rtol=1e-6)
    r.close()


@pytest.mark.parametrize("W", (4, 7, 16, 1025))
def test_launch_counts_and_no_synchronisation(torch, W):
    """1 launch for an insert without state_dev, 2 with it, 1 for the gather — counted as the kernel nodes that the calls leave in a
    stream capture, which also shows that they neither synchronise nor allocate."""
    from gym_amd import nstep

    hip = _hip()
    C, K, N, B = 64, 4, 8, 33
    i32 = dict(dtype=torch.int32, device="cuda:0")
    ring = [torch.zeros(C * W, **i32), torch.zeros(C * W, **i32), torch.zeros(C, **i32), torch.zeros(C, **i32), torch.zeros(C, dtype=torch.uint8, device="cuda:0")]
    disc = torch.zeros(C, dtype=torch.float32, device="cuda:0")
    first, obs, final = torch.zeros(N * W, **i32), torch.zeros(K * N * W, **i32), torch.zeros(K * N * W, **i32)
    act, rew = torch.zeros(K * N, dtype=torch.int64, device="cuda:0"), torch.zeros(K * N, dtype=torch.float64, device="cuda:0")
    term, trunc = (torch.zeros(K * N, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    state = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    idx, out = torch.zeros(B, dtype=torch.int64, device="cuda:0"), torch.zeros(B, dtype=torch.float32, device="cuda:0")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    s, lib = side.cuda_stream, nstep.lib
    rp = [x.data_ptr() for x in ring]

    def insert(st):
        return lambda: lib.mxv_nstep_insert(s, C, W, K, N, first.data_ptr(), W, obs.data_ptr(), W, final.data_ptr(), W, act.data_ptr(), 8, rew.data_ptr(), 8,
                                            term.data_ptr(), trunc.data_ptr(), 0, st, *rp, 3, 0.99, disc.data_ptr())

    def gather():
        return lib.mxv_nstep_gather(s, C, B, disc.data_ptr(), idx.data_ptr(), out.data_ptr())

    calls = ((insert(None), 1), (gather, 1), (insert(state.data_ptr()), 2))
    for call, _ in calls:                                                     # once outside a capture: the kernels' code is loaded
        assert call() == 0, lib.mxv_nstep_last_error()
    side.synchronize()
    assert state.tolist() == [K * N, 0] and bool((disc[:K * N] > 0).all())
    for call, nodes in calls:
        rc, n = _captured_launches(hip, s, call)
        assert (rc, n) == (0, nodes), (rc, n, lib.mxv_nstep_last_error())
    side.synchronize()


def test_the_example_repeats_itself(torch, capsys):
    """examples/dqn_nstep_cartpole.py has no torch generator: two runs give the same history, number for number; every loss is finite."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import dqn_nstep_cartpole
    finally:
        sys.path.pop(0)
    kw = dict(num_envs=64, iterations=3, K=8, updates=2, batch=128, capacity=1024)
    first = dqn_nstep_cartpole.train(**kw)
    assert "n-step" in capsys.readouterr().out
    again = dqn_nstep_cartpole.train(**kw, verbose=False)
    assert first == again and len(first) == 3
    for row in first:
        assert np.isfinite(list(row.values())).all() and row["td_abs_max"] >= row["td_abs_mean"] > 0.0 and row["stored"] > 0
        assert 0.0 < row["discount_min"] <= row["discount_mean"] <= 0.99 + 1e-6


def test_python_argument_errors(torch):
    import gym_amd

    for kw, what in ((dict(n_step=0), "n_step"), (dict(n_step=65), "n_step"), (dict(n_step=2.0), "n_step"), (dict(n_step=True), "n_step"), (dict(n_step=None), "n_step"),
                     (dict(gamma=float("nan")), "gamma"), (dict(gamma=-0.1), "gamma"), (dict(gamma=1.5), "gamma"), (dict(gamma="0.9"), "gamma"), (dict(gamma=None), "gamma"),
                     (dict(capacity=0), "capacity")):
        for cls in (gym_amd.NStepReplayBuffer, gym_amd.NStepPrioritizedReplayBuffer):
            args = dict(capacity=16, obs_shape=(4,), n_step=3, gamma=0.9, device=0)
            args.update(kw)
            with pytest.raises(ValueError, match=what):
                cls(**args)
    rng = np.random.default_rng(0)
    buf = gym_amd.NStepReplayBuffer(32, (4,), 3, 0.9, device=0)
    first, traj, _ = typed_chunk(torch, rng, 2, 8, (4,), np.float32, np.int32, np.float64)
    with pytest.raises(ValueError, match='no "final_obs"'):
        buf.add_chunk(first, {k: v for k, v in traj.items() if k != "final_obs"})
    big = typed_chunk(torch, rng, 5, 8, (4,), np.float32, np.int32, np.float64)
    with pytest.raises(ValueError, match="exceed the capacity"):
        buf.add_chunk(big[0], big[1])
    assert buf.count == 0 and not buf._discount.any()
    from gym_amd.toy_text import BlackjackRollout

    bj = BlackjackRollout(64, seed=1, action_seed=2)
    with pytest.raises(ValueError, match="nstep_replay_buffer"):
        bj.nstep_replay_buffer(128, 3, 0.9)
    bj.close()
