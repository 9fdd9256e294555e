"""gym_amd.policy on the device against tests/policy_host.py, bit for bit — actions, the bits of log_prob and the bits of entropy:
every shape class and both instantiation kinds, 2048 * 256 + 257 rows (the tile loop strides), strided views with guarded outputs,
non-finite and extreme rows, the device step counter under graph replay, checkpoints, and the samplers of the three rollout front
ends end to end."""
import numpy as np
import pytest

import policy_host as ph
from policy_host import bits

pytestmark = pytest.mark.gpu

GUARD_F32 = 0x7FABCDEF      # a NaN pattern no computation produces (NaN results are written as 0x7FC00000)
GUARD_INT = -0x5A5A5A5B
SIZES = (1, 3, 63, 64, 65, 255, 257, 4099)
ACTIONS = (1, 2, 3, 4, 6, 7, 64)
OFFSETS = (0, 1, 6)
STEPS = (0, 5, 2 ** 32 + 1)


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host_bits(torch, x):
    return x.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _logits(rng, N, A):
    """Rows of every scale the accuracy test uses, some with a masked action."""
    x = (rng.standard_normal((N, A)) * rng.choice([0.1, 1.0, 5.0, 30.0], size=(N, 1))).astype(np.float32)
    if A > 1:
        rows = rng.random(N) < 0.2
        x[rows, rng.integers(0, A, N)[rows]] = -np.inf
    return x


def _assert_equal(torch, got, want, what):
    a, lp, en = got
    wa, wlp, wen = want
    assert np.array_equal(a.cpu().numpy().astype(np.int64), wa), what
    if lp is not None:
        assert np.array_equal(host_bits(torch, lp), bits(wlp)), what
    if en is not None:
        assert np.array_equal(host_bits(torch, en), bits(wen)), what


def _expected_launch(N, A):
    from gym_amd.policy import STRAIGHT_LINE_ACTIONS

    return (1, A if A in STRAIGHT_LINE_ACTIONS else 0, min((N + 255) // 256, 2048))


@pytest.mark.parametrize("A", ACTIONS)
def test_every_shape_offset_and_step_matches_the_twin(torch, A):
    from gym_amd import policy

    rng = np.random.default_rng(7 + A)
    case = 0
    for N in SIZES:
        x = _logits(rng, N, A)
        xd = dev(torch, x)
        for off in OFFSETS:
            for step in STEPS:
                dtype = (torch.int64, torch.int32)[case % 2]
                case += 1
                got = policy.sample_categorical(xd, seed=11 + A, step=step, env_offset=off, action_dtype=dtype)
                assert got[0].dtype == dtype and policy.last_launch() == _expected_launch(N, A)
                _assert_equal(torch, got, ph.sample_categorical(x, seed=11 + A, step=step, env_offset=off), (N, A, off, step, dtype))


@pytest.mark.parametrize("dtype_name", ["int64", "int32"])
def test_both_action_dtypes_at_every_offset_and_step(torch, dtype_name):
    from gym_amd import policy

    dtype = getattr(torch, dtype_name)
    rng = np.random.default_rng(3)
    for A in (3, 7):
        x = _logits(rng, 257, A)
        xd = dev(torch, x)
        for off in OFFSETS:
            for step in STEPS:
                got = policy.sample_categorical(xd, seed=2 ** 63 + 5, step=step, env_offset=off, action_dtype=dtype)
                _assert_equal(torch, got, ph.sample_categorical(x, seed=2 ** 63 + 5, step=step, env_offset=off), (A, off, step))


def _guarded(torch, N, dtype, lead):
    """A [N] view `lead` elements into a guard-filled parent; -> (view, parent)."""
    parent = torch.full((N + lead + 5,), GUARD_INT if dtype in (torch.int32, torch.int64) else 0, dtype=dtype, device="cuda:0")
    if dtype == torch.float32:
        parent.view(torch.int32).fill_(GUARD_F32)
    return parent[lead:lead + N], parent


def _assert_guard_intact(torch, parent, lead, N, what):
    p = parent.view(torch.int32) if parent.dtype == torch.float32 else parent
    guard = GUARD_F32 if parent.dtype == torch.float32 else GUARD_INT
    rest = torch.cat((p[:lead], p[lead + N:])).cpu().numpy()
    assert np.all(rest == guard), what


@pytest.mark.parametrize("A", (2, 3, 4, 6, 7))
def test_views_of_wider_buffers_and_guarded_outputs(torch, A):
    from gym_amd import policy

    rng = np.random.default_rng(40 + A)
    N = 259
    for k, off in enumerate((1, 2, 4)):
        ld = A + 5 + off
        wide = rng.standard_normal((N, ld)).astype(np.float32)
        wd = dev(torch, wide)
        xd = wd[:, off:off + A]
        assert xd.stride(0) == ld and xd.data_ptr() == wd.data_ptr() + 4 * off
        x = wide[:, off:off + A]
        dtype = (torch.int64, torch.int32)[k % 2]
        (a, pa), (lp, plp), (en, pen) = _guarded(torch, N, dtype, 3), _guarded(torch, N, torch.float32, 1), _guarded(torch, N, torch.float32, 2)
        want = ph.sample_categorical(x, seed=5, step=9, env_offset=off)
        for omit in (None, 1, 2):
            out = [a, lp, en]
            if omit is not None:
                out[omit] = None
                (plp if omit == 1 else pen).view(torch.int32).fill_(GUARD_F32)
            got = policy.sample_categorical(xd, seed=5, step=9, env_offset=off, out=tuple(out))
            assert got[0] is a and got[1] is out[1] and got[2] is out[2]
            _assert_equal(torch, got, want, (A, off, omit))
            if omit is not None:                                   # an omitted output is not written at all
                assert np.all((plp if omit == 1 else pen).view(torch.int32).cpu().numpy() == GUARD_F32)
            for parent, lead, name in ((pa, 3, "actions"), (plp, 1, "log_prob"), (pen, 2, "entropy")):
                _assert_guard_intact(torch, parent, lead, N, (A, off, omit, name))
        assert torch.equal(wd.cpu(), torch.from_numpy(wide))       # the logits are read only
    with pytest.raises(ValueError, match="overlaps the logits"):
        policy.sample_categorical(xd, seed=0, step=0, out=(torch.zeros(N, dtype=torch.int64, device="cuda:0"), wd.view(-1)[3:3 + N], None))


# kMaxBlocks * kThreads + 257 rows: the tile loop of categorical_kernel strides (every smaller N above gives each workgroup one tile);
# workgroup 0 takes a second, full tile (rows 524 288 ..) and workgroup 1 a second tile of one row
STRIDING = 2048 * 256 + 257


@pytest.mark.parametrize("A,off,step", ((3, 6, 5), (7, 0, 2 ** 32 + 1)))      # the straight-line kernel and the loop over A
def test_above_2048_tiles_every_workgroup_takes_a_second_tile(torch, A, off, step):
    from gym_amd import policy

    N = STRIDING
    x = _logits(np.random.default_rng(1300 + A), N, A)
    xd = dev(torch, x)
    (a, pa), (lp, plp), (en, pen) = _guarded(torch, N, torch.int64, 3), _guarded(torch, N, torch.float32, 1), _guarded(torch, N, torch.float32, 2)
    got = policy.sample_categorical(xd, seed=11 + A, step=step, env_offset=off, out=(a, lp, en))
    assert policy.last_launch() == (1, A if A == 3 else 0, 2048)
    _assert_equal(torch, got, ph.sample_categorical(x, seed=11 + A, step=step, env_offset=off), (N, A, off, step))
    for parent, lead, name in ((pa, 3, "actions"), (plp, 1, "log_prob"), (pen, 2, "entropy")):
        _assert_guard_intact(torch, parent, lead, N, (A, name))                # behind row N - 1 too


@pytest.mark.parametrize("A", (3, 4, 7))
def test_non_finite_and_extreme_rows(torch, A):
    from gym_amd import policy

    inf, nan = np.inf, np.nan
    rng = np.random.default_rng(60 + A)
    special = []
    for a in range(A):
        for v in (nan, inf):
            row = rng.standard_normal(A)
            row[a] = v
            special.append(row)
    special += [np.full(A, -inf), np.full(A, nan), np.full(A, inf), np.full(A, 3e38), np.full(A, -3e38), np.zeros(A), np.full(A, 1.25)]
    alt = np.where(np.arange(A) % 2 == 0, 3e38, -3e38)
    special += [alt, -alt, np.arange(A) * -709.0, np.arange(A)[::-1] * -709.0, np.arange(A) * -707.9, np.where(np.arange(A) == A - 1, 0.0, -inf),
                np.where(np.arange(A) == 0, nan, -inf), np.concatenate(([-inf], np.zeros(A - 1))), np.full(A, 1e-45), np.full(A, -1e-45)]
    x = np.asarray(special, np.float32)
    got = policy.sample_categorical(dev(torch, x), seed=8, step=2, env_offset=3)
    want = ph.sample_categorical(x, seed=8, step=2, env_offset=3)
    _assert_equal(torch, got, want, A)
    degenerate = np.isnan(x).any(1) | (x == inf).any(1) | (x == -inf).all(1)
    assert degenerate.sum() >= 2 * A + 4
    assert np.all(got[0].cpu().numpy()[degenerate] == 0)
    assert np.all(host_bits(torch, got[1])[degenerate] == 0x7FC00000) and np.all(host_bits(torch, got[2])[degenerate] == 0x7FC00000)
    assert np.all(np.isfinite(got[1].cpu().numpy()[~degenerate])) and np.all(np.isfinite(got[2].cpu().numpy()[~degenerate]))
    # one -inf logit is never selected over 4 096 envs, at any position
    for masked in range(A):
        row = rng.standard_normal(A).astype(np.float32)
        row[masked] = -inf
        rows = np.broadcast_to(row, (4096, A)).copy()
        a, lp, en = policy.sample_categorical(dev(torch, rows), seed=21, step=masked)
        _assert_equal(torch, (a, lp, en), ph.sample_categorical(rows, seed=21, step=masked), (A, masked))
        counts = np.bincount(a.cpu().numpy(), minlength=A)
        assert counts[masked] == 0 and counts.sum() == 4096


def test_device_step_counter_under_graph_replay(torch):
    from gym_amd import policy

    N, A, calls, replays = 300, 3, 8, 3
    x = _logits(np.random.default_rng(77), N, A)
    xd = dev(torch, x)
    s = policy.PolicySampler(A, seed=31, env_offset=2, device=0)
    rows = [torch.zeros((calls, N), dtype=dt, device="cuda:0") for dt in (torch.int64, torch.float32, torch.float32)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.sample(xd, out=(rows[0][0], rows[1][0], rows[2][0]))                # warm-up outside the capture
        assert s.step_index() == 1 and policy.last_launch() == _expected_launch(N, A)
        s.load_state_dict(dict(s.state_dict(), step=0))
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for k in range(calls):
                s.sample(xd, out=(rows[0][k], rows[1][k], rows[2][k]))
        got = []
        for _ in range(replays):
            g.replay()
            side.synchronize()
            got.append([r.clone() for r in rows])
    assert s.step_index() == calls * replays
    for i in range(calls * replays):
        host_stepped = policy.sample_categorical(xd, seed=31, step=i, env_offset=2)
        graphed = tuple(r[i % calls] for r in got[i // calls])
        assert torch.equal(graphed[0], host_stepped[0])
        assert np.array_equal(host_bits(torch, graphed[1]), host_bits(torch, host_stepped[1]))
        assert np.array_equal(host_bits(torch, graphed[2]), host_bits(torch, host_stepped[2]))
        if i % 5 == 0:
            _assert_equal(torch, host_stepped, ph.sample_categorical(x, seed=31, step=i, env_offset=2), i)
    assert len({tuple(got[r][0][k].cpu().tolist()) for r in range(replays) for k in range(calls)}) == calls * replays


def test_a_restored_sampler_continues_with_the_same_bits(torch):
    from gym_amd import policy

    x = _logits(np.random.default_rng(78), 130, 6)
    xd = dev(torch, x)
    s = policy.PolicySampler(6, seed=2 ** 64 - 3, env_offset=2 ** 40 + 1, action_dtype=torch.int32)
    for _ in range(5):
        s.sample(xd)
    state = s.state_dict()
    assert state["step"] == 5 and state["seed"] == 2 ** 64 - 3 and state["env_offset"] == 2 ** 40 + 1
    fresh = policy.PolicySampler(6, action_dtype=torch.int32)
    fresh.load_state_dict(state)
    for i in range(3):
        a, b = s.sample(xd), fresh.sample(xd)
        _assert_equal(torch, a, ph.sample_categorical(x, seed=2 ** 64 - 3, step=5 + i, env_offset=2 ** 40 + 1), i)
        assert torch.equal(a[0], b[0]) and np.array_equal(host_bits(torch, a[1]), host_bits(torch, b[1]))
        assert np.array_equal(host_bits(torch, a[2]), host_bits(torch, b[2]))
    assert s.step_index() == fresh.step_index() == 8
    with pytest.raises(ValueError, match="columns"):
        s.sample(xd[:, :3])
    with pytest.raises(ValueError, match="actions"):
        policy.PolicySampler(3).load_state_dict(state)


def _head(torch, O, NA, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((O, NA)).astype(np.float32)).to("cuda:0")


@pytest.mark.parametrize("env_id", ["CartPole-v1", "Acrobot-v1"])
def test_device_rollout_eager_graphed_and_sharded(torch, env_id):
    from gym_amd.rollout import DeviceRollout

    n, K, warm = 256, 16, 3

    def make(num, off=0):
        r = DeviceRollout(env_id, num, seed=4, action_seed=9, env_offset=off)
        r.reset(seed=4)
        return r, r.policy_sampler()

    def eager(r, s, W, steps):
        acts, obs, lps = [], [], []
        with torch.cuda.stream(r.stream):
            for _ in range(steps):
                logits = r.obs @ W
                a, lp, _ = s.sample(logits)
                lps.append((logits.clone(), lp))
                r.step(a)
                acts.append(a.clone())
                obs.append(r.obs.clone())
        r.synchronize()
        return torch.stack(acts), torch.stack(obs), lps

    r, s = make(n)
    assert s.num_actions == r.NA and s.action_dtype == r.action_dtype and s.seed == 9 and s.env_offset == 0
    W = _head(torch, r.O, r.NA, 1)
    acts, obs, lps = eager(r, s, W, warm + K)
    assert s.step_index() == warm + K
    for t in (0, warm + K - 1):                                  # the draws are the twin's for the logits the device computed
        want = ph.sample_categorical(lps[t][0].cpu().numpy(), seed=9, step=t)
        assert np.array_equal(acts[t].cpu().numpy(), want[0]) and np.array_equal(host_bits(torch, lps[t][1]), bits(want[1]))
    r.close()

    r, s = make(n)
    g_acts = torch.zeros((K, n), dtype=r.action_dtype, device=r.device)
    g_obs = torch.zeros((K, n, r.O), device=r.device)
    torch.cuda.synchronize()                                     # the buffers are filled on the default stream, used on the engine's
    pending = {}

    def policy(o):
        pending["a"] = s.sample(o @ W)[0]
        return pending["a"]

    def record(k):
        g_acts[k].copy_(pending["a"])
        g_obs[k].copy_(r.obs)

    graph = r.graphed_loop(policy, K, warmup=warm, on_step=record)
    graph.replay()
    r.synchronize()
    assert s.step_index() == warm + K
    assert torch.equal(g_acts, acts[warm:]) and torch.equal(g_obs, obs[warm:])
    r.close()

    parts = []
    for off in (0, n // 2):
        r, s = make(n // 2, off)
        assert s.env_offset == off
        parts.append(eager(r, s, W, warm + K)[:2])
        r.close()
    assert torch.equal(torch.cat((parts[0][0], parts[1][0]), dim=1), acts)
    assert torch.equal(torch.cat((parts[0][1], parts[1][1]), dim=1), obs)


def test_box_envs_name_the_follow_up(torch):
    from gym_amd.rollout import DeviceRollout

    r = DeviceRollout("Pendulum-v1", 8)
    with pytest.raises(ValueError, match="Gaussian"):
        r.policy_sampler()
    r.close()


def test_one_tape_step_through_the_tabular_and_blackjack_rollouts(torch):
    from gym_amd.toy_text import BlackjackRollout, TabularRollout

    r = TabularRollout("FrozenLake-v1", 64, seed=2, action_seed=6, env_offset=8)      # the engines take offsets in whole Philox groups
    obs = r.reset(seed=2)
    s = r.policy_sampler()
    assert (s.num_actions, s.action_dtype, s.seed, s.env_offset) == (4, torch.int64, 6, 8)
    table = _head(torch, 16, 4, 2)
    logits = table[obs]
    a, lp, en = s.sample(logits)
    out = r.rollout_tape(a[None])
    r.synchronize()
    want = ph.sample_categorical(logits.cpu().numpy(), seed=6, step=0, env_offset=8)
    _assert_equal(torch, (a, lp, en), want, "FrozenLake-v1")
    assert torch.equal(out["actions"][0], a) and int(out["obs"].min()) >= 0 and int(out["obs"].max()) < 16
    r.close()

    r = BlackjackRollout(64, seed=2, action_seed=6)
    obs = r.reset(seed=2)
    s = r.policy_sampler(seed=12)
    assert (s.num_actions, s.action_dtype, s.seed, s.env_offset) == (2, torch.int64, 12, 0)
    logits = _head(torch, 32, 2, 3)[obs[0]]
    a, lp, en = s.sample(logits)
    out = r.rollout_tape(a[None])
    r.synchronize()
    _assert_equal(torch, (a, lp, en), ph.sample_categorical(logits.cpu().numpy(), seed=12, step=0), "Blackjack-v1")
    assert torch.equal(out["actions"][0], a) and set(out["terminated"].unique().tolist()) <= {0, 1}
    r.close()


def test_the_example_prints_the_same_history_twice(torch, capsys):
    import os
    import sys

    from conftest import ROOT

    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import actor_critic_sampled
    finally:
        sys.path.pop(0)
    printed = []
    for _ in range(2):
        h = actor_critic_sampled.train(256, 2, K=16)
        printed.append(capsys.readouterr().out)
        assert len(h) == 2 and all(np.isfinite(list(row.values())).all() for row in h)
        assert 0 < h[0]["mean_entropy"] <= np.log(2.0) + 1e-6 and h[0]["mean_log_prob"] < 0
    assert printed[0] == printed[1] and "iteration   1" in printed[0] and f"{3 + 2 * 16} policy steps drawn" in printed[0]
