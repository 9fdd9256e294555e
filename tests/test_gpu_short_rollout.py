"""Short fused launches against one launch per step, bit for bit.

rollout_kernel_v3 keeps a ready-made reset entry per env slot in LDS and refills empty slots on a periodic look-ahead pass, or at once
when an env finishes and finds its slot empty.  An entry is a pure function of (seed, reset ordinal), so no schedule of
fills may change a bit.  Held here where the schedule matters most: launches shorter than one pass period, TimeLimits of 1-3 steps (every
slot is empty again before any pass comes round), one launch continuing from the state another left, sub-tile / ragged / two-envs-per-lane
shards, tapes, the STATS instantiation, and the oracle."""
import numpy as np
import pytest

from helpers import ENV_IDS, ENV_NAMES, GYM_IDS, MAX_OBS_ULPS, ulps32

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5, 8, 9, 20)                      # below, at and across the 8-step pass period; 20 = the driver's launch
TWO_PER_LANE = (1 << 17) + 128                      # the smallest shard of a two-envs-per-lane kind that takes two
ROLLOUT_ENVS_PER_LANE = {"CartPole": 2, "Pendulum": 1, "Acrobot": 1, "MountainCar": 2, "MountainCarContinuous": 2}
KEYS = ("obs", "reward", "terminated", "truncated", "actions")


def _bits(t):
    import torch

    return t.contiguous().view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def _same(a, b):
    import torch

    return torch.equal(_bits(a), _bits(b))


def _same_state(a, b):
    """final fp64 state, TimeLimit counters, reset ordinals, step / reset counters — bit for bit"""
    sa, ea = a.handle.get_state()
    sb, eb = b.handle.get_state()
    assert np.array_equal(sa.view(np.uint64), sb.view(np.uint64)) and np.array_equal(ea, eb)
    assert np.array_equal(a.handle.get_episodes(), b.handle.get_episodes())
    assert a.handle.get_counters() == b.handle.get_counters()


def _pair(name, n, limit, **kw):
    from gym_amd.rollout import DeviceRollout

    kw = dict(kw, seed=21, action_seed=22)
    if limit is not None:
        kw["max_episode_steps"] = limit
    a, b = DeviceRollout(GYM_IDS[name], n, **kw), DeviceRollout(GYM_IDS[name], n, **kw)
    a.reset(seed=21), b.reset(seed=21)
    return a, b


@pytest.mark.parametrize("limit", [1, 2, 3, None])
@pytest.mark.parametrize("n", [64, 1000, TWO_PER_LANE])
@pytest.mark.parametrize("name", ENV_NAMES)
def test_fused_launches_of_every_short_length_equal_single_steps(name, n, limit):
    """Every K of KS in turn on one pair of engines, so each launch but the first starts from the state a launch of another length left."""
    a, b = _pair(name, n, limit)
    fused, eager = a.trajectory_buffers(max(KS), layout="separate"), b.trajectory_buffers(max(KS), layout="separate")
    ended = 0
    for K in KS:
        a.rollout_per_step(K, mode="fused", out=fused)
        li = a.handle.last_launch()
        b.rollout_per_step(K, mode="eager", out=eager)
        a.synchronize(), b.synchronize()
        assert li["steps"] == K and li["kernel"] == (1 if K > 1 else 0), li
        if K > 1:
            assert li["envs_per_lane"] == (ROLLOUT_ENVS_PER_LANE[name] if n == TWO_PER_LANE else 1), li
        for key in KEYS:
            assert _same(fused[key][:K], eager[key][:K]), (name, n, limit, K, key)
        ended += int(((fused["terminated"][:K] | fused["truncated"][:K]) != 0).sum())
    _same_state(a, b)
    if limit is not None:
        assert ended >= (sum(KS) // limit - 1) * n          # every env ran out of its TimeLimit again and again
    a.close(), b.close()


@pytest.mark.parametrize("name", ENV_NAMES)
def test_two_launches_back_to_back_without_a_synchronise_between_them(name):
    a, b = _pair(name, 1000, 2)
    fa = [a.trajectory_buffers(5, layout="separate"), a.trajectory_buffers(3, layout="separate")]
    fb = [b.trajectory_buffers(5, layout="separate"), b.trajectory_buffers(3, layout="separate")]
    for K, oa, ob in ((5, fa[0], fb[0]), (3, fa[1], fb[1])):
        a.rollout_per_step(K, mode="fused", out=oa)
        b.rollout_per_step(K, mode="eager", out=ob)
    a.synchronize(), b.synchronize()
    for oa, ob in zip(fa, fb):
        for key in KEYS:
            assert _same(oa[key], ob[key]), (name, key)
    _same_state(a, b)
    a.close(), b.close()


@pytest.mark.parametrize("name", ENV_NAMES)
def test_a_tape_driven_short_launch_equals_stepping_the_same_rows(name):
    """K = 5 and then K = 3 with the caller's actions, TimeLimit 2, a ragged and a two-envs-per-lane shard."""
    import torch

    for n in (1000, TWO_PER_LANE):
        a, b = _pair(name, n, 2)
        src, spare = _pair(name, n, 2)
        spare.close()
        for K in (5, 3):
            sampled = src.rollout_per_step(K, mode="fused")
            src.synchronize()
            rows = sampled["actions"].clone()
            torch.cuda.synchronize()
            out = a.rollout_tape(rows)
            li = a.handle.last_launch()
            assert li["kernel"] == 1 and li["tape"] == 1 and li["envs_per_lane"] == (ROLLOUT_ENVS_PER_LANE[name] if n == TWO_PER_LANE else 1), li
            a.synchronize()
            for k in range(K):
                b.step(rows[k], want_final=False)
                b.synchronize()
                for key, got in (("obs", b.obs), ("reward", b.reward), ("terminated", b.terminated), ("truncated", b.truncated)):
                    assert _same(out[key][k], got.reshape(out[key][k].shape)), (name, n, K, k, key)
        _same_state(a, b)
        a.close(), b.close(), src.close()


def test_stats_partials_of_a_short_launch_follow_the_kernels_rule():
    """STATS = 1 at K = 5, TimeLimit 2, a ragged shard: the outputs equal the plain launch's, and every tile's column sums and sums of
    squares equal the kernel's rule restated on the host (a lane's two envs in order, then tests/test_wave_sums_tree.py's tree), bit for bit."""
    from test_wave_sums_tree import wave_sums

    n, K = 1000, 5
    a, b = _pair("CartPole", n, 2)
    out = a.trajectory_buffers(K, layout="separate", obs_partials=True)
    ref = b.trajectory_buffers(K, layout="separate")
    leaves, per, vals = a.handle.obs_partials_layout()
    assert per == 128 and vals == 8 and leaves == -(-n // per)
    for _ in range(2):
        a.rollout_per_step(K, out=out)
        b.rollout_per_step(K, mode="eager", out=ref)
        a.synchronize(), b.synchronize()
        for key in KEYS:
            assert _same(out[key], ref[key]), key
        x = out["obs"].cpu().numpy().astype(np.float64)
        xp = np.concatenate([x, np.zeros((K, leaves * per - n, 4))], axis=1).reshape(K, leaves, 2, 64, 4)    # [K][tile][j][lane][O]
        sm = (0.0 + xp[:, :, 0]) + xp[:, :, 1]
        sq = (0.0 + xp[:, :, 0] * xp[:, :, 0]) + xp[:, :, 1] * xp[:, :, 1]                                 # x * x is exact in fp64
        v = np.concatenate([sm, sq], axis=-1)                                                                # [K][tile][lane][8]
        lane = np.arange(64)
        idx = (lane & 3) | ((lane >> 1) & 4)
        holder = (lane & 0x34) == 0
        want = np.empty((K, leaves, 8))
        for k in range(K):
            for t in range(leaves):
                tot = wave_sums(v[k, t])
                want[k, t, idx[holder]] = tot[holder]
        got = out["obs_partials"].cpu().numpy()
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    _same_state(a, b)
    a.close(), b.close()


def test_first_envs_of_a_short_cartpole_launch_against_the_oracle():
    """K = 20 then K = 3 at TimeLimit 3: the first 4096 envs of a two-envs-per-lane shard against the oracle twin — flags and actions exactly,
    observations within the engine's float32 bar."""
    from gym_amd.rollout import DeviceRollout
    from oracle.oracle import OracleVecEnv

    n, c = TWO_PER_LANE, 4096
    r = DeviceRollout("CartPole-v1", n, seed=21, action_seed=22, max_episode_steps=3)
    obs0 = r.reset(seed=21)[:c].cpu().numpy()
    o = OracleVecEnv(ENV_IDS["CartPole"], c, 3, seed=21, action_seed=22)
    np.testing.assert_array_equal(o.reset(seed=21), obs0)
    for K in (20, 3):
        out = r.rollout_per_step(K, mode="fused")
        r.synchronize()
        assert r.handle.last_launch()["envs_per_lane"] == 2
        got = {k: out[k][:, :c].cpu().numpy() for k in KEYS}
        for k in range(K):
            act = o.sample_actions()
            ob, rw, te, tr, _, _ = o.step(act)
            assert np.array_equal(got["actions"][k], act) and np.array_equal(got["terminated"][k].astype(bool), te), (K, k)
            assert np.array_equal(got["truncated"][k].astype(bool), tr) and np.array_equal(got["reward"][k], rw), (K, k)
            assert ulps32(got["obs"][k], ob).max() <= MAX_OBS_ULPS, (K, k)
    r.close()
