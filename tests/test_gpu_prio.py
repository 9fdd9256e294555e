"""gym_amd.PrioritizedReplayBuffer and the calls of include/mxv_prio.h on the device against tests/prio_host.py, the NumPy twin of the
rule: the leaves, every node level, qmax and every drawn array compared bit for bit after every call.  Insert / sample / update
sequences at every capacity (H = 1 .. 5), batch size and row width; updates whose indices are all equal, out of range, or whose TD
errors are NaN / Inf / 0; alpha = 0; the all-zero tree; a ring that wrapped twice; the graph replay, the launch counts, the checkpoint,
the example run twice and the front end's refusals."""
import os
import sys

import numpy as np
import pytest

import prio_host as ph
import replay_host as rh
from conftest import ROOT
from test_gpu_ppo import _captured_launches, _hip
from test_gpu_replay import batch_same_as, buffer_same_as, down, twin_insert, typed_chunk, up

pytestmark = pytest.mark.gpu

# capacity, row width in dwords: every capacity of the rule's levels with every copier (1 lane per row: the loop, 4 and 7; wide: 16, 1025)
SHAPES = ((5, 7), (16, 4), (17, 16), (257, 1025), (4097, 4), (65537, 1))
BATCHES = (1, 63, 64, 65, 257, 1025)


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def tree_same_as(torch, buf, tree, what):
    leaf, node = down(torch, buf._leaf), down(torch, buf._node, np.uint64)
    assert len(leaf) == tree.leaf_words and len(node) == tree.node_words
    bad = np.flatnonzero(leaf != tree.leaf)
    assert bad.size == 0, (what, "leaves", bad[:8], leaf[bad[:8]], tree.leaf[bad[:8]])
    at = 0
    for l, level in enumerate(tree.levels, 1):
        mine = node[at:at + len(level)]
        bad = np.flatnonzero(mine != level)
        assert bad.size == 0, (what, "level", l, bad[:8], mine[bad[:8]], level[bad[:8]])
        at += len(level)
    assert int(down(torch, buf._qmax)[0]) == tree.qmax, (what, "qmax")


def sampled_same_as(torch, batch, want, buf, B, what):
    batch_same_as(torch, batch, want, buf, B, what)
    got = down(torch, batch["weights"].view(torch.int32))
    assert batch["weights"].dtype == torch.float32 and np.array_equal(got, want["weights"].view(np.uint32)), (what, "weights")


def td_errors(rng, B):
    td = (rng.standard_normal(B) * 10.0 ** rng.integers(-4, 5, size=B)).astype(np.float32)
    td[::17] = 0.0
    return td


class Pair:
    """A device buffer and its twin, driven together."""

    def __init__(self, torch, C, W, seed, alpha=0.6, eps=1e-6, capture=False):
        import gym_amd

        self.torch, self.C, self.W, self.seed, self.alpha, self.eps = torch, C, W, seed, alpha, eps
        self.buf = gym_amd.PrioritizedReplayBuffer(C, (W,), seed=seed, device=0, alpha=alpha, eps=eps)
        if capture:
            self.buf.enable_graph_capture()
        self.ring, self.tree, self.count, self.step = rh.Ring(C, W), ph.Tree(C), 0, 0

    def twin_add(self, host):
        K, N = host["obs"].shape[:2]
        self.tree.insert(self.count, K * N)
        self.count = twin_insert(self.ring, self.count, host)

    def add(self, rng, K, N, what):
        first, traj, host = typed_chunk(self.torch, rng, K, N, (self.W,), np.float32, np.int32, np.float64)
        self.buf.add_chunk(first, traj)
        self.twin_add(host)
        tree_same_as(self.torch, self.buf, self.tree, (what, "insert"))

    def twin_sample(self, B, beta):
        want = ph.sample(self.tree, self.ring, self.seed, self.step, B, beta)
        self.step += 1
        return want

    def sample(self, B, beta, what):
        batch = self.buf.sample(B, beta=beta)
        sampled_same_as(self.torch, batch, self.twin_sample(B, beta), self.buf, B, (what, "sample"))
        tree_same_as(self.torch, self.buf, self.tree, (what, "sample"))
        return batch

    def update(self, indices, td, what):
        self.buf.update_priorities(up(self.torch, np.asarray(indices, np.int64)), up(self.torch, np.asarray(td, np.float32)))
        self.tree.update(self.count, indices, td, self.alpha, self.eps)
        tree_same_as(self.torch, self.buf, self.tree, (what, "update"))


@pytest.mark.parametrize("C,W", SHAPES)
def test_insert_sample_update_sequences_equal_the_twin(torch, C, W):
    rng = np.random.default_rng(C)
    p = Pair(torch, C, W, seed=C + 1)
    chunks = [(1, 1), (1, min(C, 3)), (2, max(C // 3, 1)), (1, C), (3, max(C // 4, 1)), (1, min(C, 300))]
    for i, ((K, N), B) in enumerate(zip(chunks, BATCHES)):
        p.add(rng, K, N, (C, i))
        batch = p.sample(B, (0.4, 1.0, 0.0)[i % 3], (C, i))
        k = down(torch, batch["indices"], np.int64)
        assert k.min() >= 0 and k.max() < min(p.count, C)
        p.update(k, td_errors(rng, B), (C, i))
        # a second update at indices of its own, duplicates and skipped rows among them
        idx = rng.integers(-3, C + 3, size=B)
        p.update(idx, td_errors(rng, B), (C, i, "own indices"))
    buffer_same_as(torch, p.buf, p.ring, C)
    assert p.buf.count == p.count and p.buf.sample_step == p.step == 6


def test_update_with_every_index_equal_keeps_the_maximum(torch):
    rng = np.random.default_rng(1)
    p = Pair(torch, 257, 4, seed=3)
    p.add(rng, 1, 200, "fill")
    for B in (1, 64, 1025):
        td = td_errors(rng, B)
        p.update(np.full(B, 77), td, B)
        assert int(p.tree.leaf[77]) == int(ph.quantise(td, 0.6, 1e-6).max()) == int(down(torch, p.buf._leaf)[77])
    p.update(np.full(300, 5), np.linspace(3.0, 1e-3, 300), "a smaller maximum lowers the leaf")
    assert p.tree.qmax > int(p.tree.leaf[5]) > 0


def test_update_out_of_range_changes_nothing(torch):
    rng = np.random.default_rng(2)
    p = Pair(torch, 4097, 4, seed=3)
    p.add(rng, 1, 100, "fill")
    before = (p.buf._leaf.clone(), p.buf._node.clone(), p.buf._qmax.clone())
    idx = np.array([-1, -5, 100, 101, 4096, 4097, 4098, 1 << 31, 1 << 40, -(1 << 62), 100000], np.int64)
    p.update(idx, np.full(len(idx), 1e9, np.float32), "skipped")
    for x, y in zip(before, (p.buf._leaf, p.buf._node, p.buf._qmax)):
        assert torch.equal(x, y)
    assert p.tree.qmax == ph.ONE


def test_update_with_nan_inf_and_zero_td_errors(torch):
    rng = np.random.default_rng(3)
    p = Pair(torch, 257, 4, seed=3)
    p.add(rng, 1, 257, "fill")
    td = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, 3.4e38, 1e30, -1e6, 1.0], np.float32)
    p.update(np.arange(10) * 20, td, "odd td errors")
    assert p.tree.leaf[np.arange(10) * 20].tolist() == [ph.QMAX] * 3 + [263] * 3 + [ph.QMAX] * 2 + [4174456245, 1048577] and p.tree.qmax == ph.QMAX
    p.add(rng, 1, 30, "new rows take the largest priority")
    assert int(p.tree.leaf[3]) == ph.QMAX
    p.sample(257, 0.5, "after the odd td errors")


def test_alpha_zero_is_the_uniform_draw_over_the_written_slots(torch):
    rng = np.random.default_rng(4)
    p = Pair(torch, 4097, 4, seed=9, alpha=0.0)
    p.add(rng, 2, 500, "fill")
    p.update(rng.integers(0, 1000, size=257), td_errors(rng, 257), "alpha 0")
    assert set(p.tree.leaf[:1000].tolist()) == {ph.ONE} and not p.tree.leaf[1000:].any()
    batch = p.sample(1025, 0.7, "alpha 0")
    assert (batch["weights"] == 1.0).all() and int(batch["indices"].max()) < 1000


@pytest.mark.parametrize("W", (1, 4, 7, 16, 1025))
def test_an_all_zero_tree_gives_indices_minus_one_zeros_and_zero_weights(torch, W):
    p = Pair(torch, 17, W, seed=1, capture=True)      # device counters: the front end does not refuse the empty buffer
    out = p.buf.sample_buffers(65)
    for x in out.values():
        x.view(-1).view(torch.uint8).fill_(0xAB)
    p.buf._obs.view(torch.int32).fill_(0x5A5A5A5A)
    batch = p.buf.sample(65, beta=0.4, out=out)
    assert (batch["indices"] == -1).all() and not batch["weights"].view(torch.int32).any()
    for key in ("obs", "next_obs", "actions", "reward", "terminated"):
        assert not batch[key].view(-1).view(torch.uint8).any(), key
    assert p.buf.sample_step == 1 and p.buf.count == 0
    tree_same_as(torch, p.buf, p.tree, "untouched")


def test_a_ring_that_wrapped_twice(torch):
    rng = np.random.default_rng(5)
    p = Pair(torch, 257, 7, seed=2)
    for i in range(9):      # 9 * 64 = 576 rows: past the end of the ring twice
        p.add(rng, 2, 32, i)
        batch = p.sample(64, 0.4, i)
        p.update(down(torch, batch["indices"], np.int64), td_errors(rng, 64), i)
    assert p.count == 576 > 2 * 257 and len(p.buf) == 257
    buffer_same_as(torch, p.buf, p.ring, "wrapped twice")


def test_recorded_once_and_replayed_three_times_equals_three_eager_rounds_of_the_twin(torch):
    rng = np.random.default_rng(6)
    C, K, N, B = 300, 2, 40, 65
    p = Pair(torch, C, 6, seed=77, capture=True)
    first, traj, host = typed_chunk(torch, rng, K, N, (6,), np.float32, np.int32, np.float64)
    out = p.buf.sample_buffers(B)
    td = up(torch, td_errors(rng, B))
    side = torch.cuda.Stream()

    def one_round():
        p.buf.add_chunk(first, traj)
        p.buf.sample(B, beta=0.4, out=out)
        p.buf.update_priorities(out["indices"], td)

    def twin_round(host, td_host, what):
        p.twin_add(host)
        want = p.twin_sample(B, 0.4)
        sampled_same_as(torch, out, want, p.buf, B, what)
        p.tree.update(p.count, want["indices"], td_host, 0.6, 1e-6)
        tree_same_as(torch, p.buf, p.tree, what)

    with torch.cuda.stream(side):
        one_round()      # once outside the recording: the kernels' code is loaded
        side.synchronize()
        twin_round(host, down(torch, td, np.float32), "eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            one_round()
        for k in range(3):
            fresh = typed_chunk(torch, rng, K, N, (6,), np.float32, np.int32, np.float64)
            first.copy_(fresh[0])
            for key in traj:
                traj[key].copy_(fresh[1][key])
            td_host = td_errors(rng, B)
            td.copy_(up(torch, td_host))
            g.replay()
            side.synchronize()
            twin_round(fresh[2], td_host, k)
    torch.cuda.current_stream().wait_stream(side)
    assert p.buf.count == p.count == 4 * K * N and p.buf.sample_step == 4
    buffer_same_as(torch, p.buf, p.ring, "after the replays")


@pytest.mark.parametrize("W", (4, 7, 16, 1025))
def test_launch_counts_and_no_synchronisation(torch, W):
    """Insert 1 launch, update 2, sample 2 — and one more for a sample with step_dev; the front end's add_chunk is 2 (3 with device
    counters: the ring's counter advance).  Counted as the kernel nodes that the calls leave in a stream capture, which also shows that
    they neither synchronise nor allocate."""
    from gym_amd import prioritized

    hip = _hip()
    C, K, N, B = 64, 2, 8, 33
    leaf_words, node_words, _ = prioritized.layout(C)
    i32 = dict(dtype=torch.int32, device="cuda:0")
    ring = [torch.zeros(C * W, **i32), torch.zeros(C * W, **i32), torch.zeros(C, **i32), torch.zeros(C, **i32), torch.zeros(C, dtype=torch.uint8, device="cuda:0")]
    leaf, node, qmax = torch.zeros(leaf_words, **i32), torch.zeros(node_words, dtype=torch.int64, device="cuda:0"), torch.full((1,), 1 << 20, **i32)
    work, state = torch.zeros(prioritized.WORKSPACE_WORDS, **i32), torch.zeros(2, dtype=torch.int64, device="cuda:0")
    outs = [torch.zeros(B, dtype=torch.int64, device="cuda:0"), torch.zeros(B * W, **i32), torch.zeros(B * W, **i32), torch.zeros(B, **i32),
            torch.zeros(B, **i32), torch.zeros(B, dtype=torch.uint8, device="cuda:0"), torch.zeros(B, **i32)]
    td, saved = torch.ones(B, dtype=torch.float32, device="cuda:0"), torch.zeros(B, **i32)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    s, lib = side.cuda_stream, prioritized.lib
    tree = (leaf.data_ptr(), leaf_words, node.data_ptr(), node_words)

    def insert(st):
        return lambda: lib.mxv_prio_insert(s, C, K, N, 0, st, *tree, qmax.data_ptr())

    def update(st):
        return lambda: lib.mxv_prio_update(s, C, B, outs[0].data_ptr(), td.data_ptr(), 0.6, 1e-6, K * N, st, *tree, qmax.data_ptr(), saved.data_ptr())

    def sample(st):
        return lambda: lib.mxv_prio_sample(s, C, W, B, *[x.data_ptr() for x in ring], *tree, 1, 0, st, 0.4, work.data_ptr(), outs[0].data_ptr(),
                                           outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), 4, outs[4].data_ptr(), outs[5].data_ptr(),
                                           outs[6].data_ptr())

    calls = ((insert(None), 1), (sample(None), 2), (update(None), 2), (insert(state.data_ptr()), 1), (sample(state.data_ptr() + 8), 3),
             (update(state.data_ptr()), 2))
    for call, _ in calls:      # once outside a capture: the kernels' code is loaded
        assert call() == 0, lib.mxv_prio_last_error()
    side.synchronize()
    assert state.tolist() == [0, 1] and int(outs[0].min()) >= 0 and int(outs[0].max()) < K * N
    for call, nodes in calls:
        rc, n = _captured_launches(hip, s, call)
        assert (rc, n) == (0, nodes), (rc, n, lib.mxv_prio_last_error())
    side.synchronize()
    if W == 4:
        import gym_amd

        rng = np.random.default_rng(0)
        first, traj, _ = typed_chunk(torch, rng, K, N, (4,), np.float32, np.int32, np.float64)
        for capture, nodes in ((False, 2), (True, 3)):
            buf = gym_amd.PrioritizedReplayBuffer(C, (4,), device=0)
            if capture:
                buf.enable_graph_capture()
            with torch.cuda.stream(side):
                buf.add_chunk(first, traj)      # once outside a capture: the kernels' code is loaded
                side.synchronize()
                rc, n = _captured_launches(hip, s, lambda: buf.add_chunk(first, traj))
            assert n == nodes, (capture, n)
        side.synchronize()


def test_state_dict_round_trip_continues_bit_identically(torch):
    import gym_amd

    rng = np.random.default_rng(11)
    a = gym_amd.PrioritizedReplayBuffer(50, (4,), seed=5, device=0, alpha=0.7, eps=1e-3)
    chunks = [typed_chunk(torch, rng, 2, 9, (4,), np.float32, np.int32, np.float64) for _ in range(6)]
    tds = [up(torch, td_errors(rng, 40)) for _ in range(6)]
    for (first, traj, _), td in zip(chunks[:4], tds):
        a.add_chunk(first, traj)
        a.update_priorities(a.sample(40)["indices"], td)
    state = a.state_dict()
    assert state["count"] == 72 and state["sample_step"] == 4 and state["alpha"] == 0.7 and state["eps"] == 1e-3
    b = gym_amd.PrioritizedReplayBuffer(50, (4,), seed=999, device=0)
    b.load_state_dict(state)
    c = gym_amd.PrioritizedReplayBuffer(50, (4,), seed=0, device=0).enable_graph_capture()
    c.load_state_dict(state)
    for (first, traj, _), td in zip(chunks[4:], tds[4:]):
        batches = []
        for buf in (a, b, c):
            buf.add_chunk(first, traj)
            batches.append(buf.sample(40, beta=0.9))
            buf.update_priorities(batches[-1]["indices"], td)
        for other in batches[1:]:
            for key in batches[0]:
                assert torch.equal(batches[0][key], other[key]), key
    assert a.count == b.count == c.count == 108 and c.sample_step == 6 and b.alpha == 0.7
    for x, y, z in zip((a._leaf, a._node, a._qmax, a._obs), (b._leaf, b._node, b._qmax, b._obs), (c._leaf, c._node, c._qmax, c._obs)):
        assert torch.equal(x, y) and torch.equal(x, z)
    with pytest.raises(ValueError, match="not a PrioritizedReplayBuffer"):
        b.load_state_dict(gym_amd.ReplayBuffer(50, (4,), device=0).state_dict())


def test_the_example_repeats_itself(torch, capsys):
    """examples/dqn_per_cartpole.py has no torch generator and no float atomic: two runs give the same history, number for number."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import dqn_per_cartpole
    finally:
        sys.path.pop(0)
    kw = dict(num_envs=64, iterations=3, K=8, updates=2, batch=128, capacity=1024)
    first = dqn_per_cartpole.train(**kw)
    assert "sample steps drawn" in capsys.readouterr().out
    again = dqn_per_cartpole.train(**kw, verbose=False)
    assert first == again and len(first) == 3 and first[0]["beta"] == 0.4 and first[-1]["beta"] == 1.0
    for row in first:
        assert np.isfinite(list(row.values())).all() and row["td_abs_max"] >= row["td_abs_mean"] > 0.0 and row["stored"] > 0


def test_a_rollouts_buffer_and_the_python_argument_errors(torch):
    import gym_amd
    from gym_amd.rollout import DeviceRollout

    r = DeviceRollout("CartPole-v1", 64, seed=1, action_seed=2)
    buf = r.prioritized_replay_buffer(256, alpha=0.5, eps=1e-4)
    assert isinstance(buf, gym_amd.PrioritizedReplayBuffer) and buf.obs_shape == (4,) and buf.seed == 2 and (buf.alpha, buf.eps) == (0.5, 1e-4)
    assert buf.levels == 2
    r.close()
    for kw, what in ((dict(alpha=-0.1), "alpha"), (dict(alpha=1.5), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(alpha="1"), "alpha"),
                     (dict(eps=0.0), "eps"), (dict(eps=2.0), "eps"), (dict(capacity=0), "capacity")):
        args = dict(capacity=16, obs_shape=(4,), device=0)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            gym_amd.PrioritizedReplayBuffer(**args)
    buf = gym_amd.PrioritizedReplayBuffer(32, (4,), device=0)
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError, match="empty"):
        buf.sample(4)
    big = typed_chunk(torch, rng, 5, 8, (4,), np.float32, np.int32, np.float64)
    with pytest.raises(ValueError, match="exceed the capacity"):
        buf.add_chunk(big[0], big[1])
    assert buf.count == 0 and not buf._leaf.any()
    first, traj, _ = typed_chunk(torch, rng, 2, 8, (4,), np.float32, np.int32, np.float64)
    buf.add_chunk(first, traj)
    plain = gym_amd.ReplayBuffer(32, (4,), device=0).sample_buffers(4)
    for kw, what in ((dict(batch_size=0), "batch_size"), (dict(batch_size=4, beta=1.5), "beta"), (dict(batch_size=4, beta=float("nan")), "beta"),
                     (dict(batch_size=4, out=plain), "weights"), (dict(batch_size=4, out=buf.sample_buffers(5)), "shape")):
        with pytest.raises(ValueError, match=what):
            buf.sample(**kw)
    shared = buf.sample_buffers(4)
    shared["weights"] = shared["reward"]
    with pytest.raises(ValueError, match="overlap"):
        buf.sample(4, out=shared)
    idx, td = torch.zeros(4, dtype=torch.int64, device="cuda:0"), torch.zeros(4, dtype=torch.float32, device="cuda:0")
    for args, what in (((idx.int(), td), "int64"), ((idx, td.double()), "float32"), ((idx, td[:3]), "shape"), ((idx.cpu(), td), "device tensor"),
                       ((idx.view(2, 2), td), "shape \\[B\\]"), (([0, 1], td), "tensor")):
        with pytest.raises(ValueError, match=what):
            buf.update_priorities(*args)
