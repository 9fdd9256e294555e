"""Host-side mirror of the reference interface (no GPU): spaces, batch_space, registry, seeding rules, LazyInfos.
When /root/reference is present (build container) the same checks also run against the live reference."""
import os
import sys

import numpy as np
from helpers import reference_wrapper_stub
import pytest

from gym_amd import error
from gym_amd.registration import PARAM_NAMES, registry, single_spaces, spec
from gym_amd.spaces import Box, Discrete, MultiDiscrete, batch_space, np_random

REF = "/root/reference"


def _ref_gym():
    if not os.path.isdir(os.path.join(REF, "gym")):
        pytest.skip("live reference not available")
    for name, val in (("bool8", np.bool_), ("float_", np.float64), ("alltrue", np.all)):
        if not hasattr(np, name):
            setattr(np, name, val)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import gym

    gym.logger.set_level(gym.logger.ERROR)
    return gym


def test_registry_matches_reference_ids_and_limits():
    want = {"CartPole-v0": 200, "CartPole-v1": 500, "MountainCar-v0": 200, "MountainCarContinuous-v0": 999,
            "Pendulum-v1": 200, "Acrobot-v1": 500}  # gym/envs/__init__.py:11-50
    assert {k: v.max_episode_steps for k, v in registry.items()} == want
    with pytest.raises(error.UnregisteredEnv):
        spec("LunarLander-v2")


def test_registry_against_live_reference():
    gym = _ref_gym()
    for env_id, s in registry.items():
        rs = gym.spec(env_id)
        assert rs.max_episode_steps == s.max_episode_steps and rs.reward_threshold == s.reward_threshold
        env = gym.make(env_id, disable_env_checker=True)
        obs_space, act_space = single_spaces(s.kind)
        assert obs_space.shape == env.observation_space.shape and obs_space.dtype == env.observation_space.dtype
        assert np.array_equal(obs_space.low, env.observation_space.low)
        assert np.array_equal(obs_space.high, env.observation_space.high)
        if isinstance(act_space, Discrete):
            assert act_space.n == env.action_space.n
        else:
            assert np.array_equal(act_space.low, env.action_space.low) and act_space.shape == env.action_space.shape
        for name in PARAM_NAMES[s.kind]:  # every attribute the engine exposes exists on the reference env object
            assert hasattr(env.unwrapped, name), (env_id, name)


def test_spaces_sample_like_the_reference():
    gym = _ref_gym()
    from gym import spaces as rs
    from gym.vector.utils import batch_space as ref_batch

    for mine, ref in ((Discrete(3), rs.Discrete(3)), (Box(-2.0, 2.0, (1,), np.float32), rs.Box(-2.0, 2.0, (1,), np.float32)),
                      (MultiDiscrete([2] * 5), rs.MultiDiscrete([2] * 5))):
        mine.seed(123), ref.seed(123)
        for _ in range(5):
            assert np.array_equal(np.asarray(mine.sample()), np.asarray(ref.sample()))
    # batch_space: same class, bounds, dtype and the same RNG stream (deepcopy of the single space's generator)
    for mine, ref in ((Discrete(2), rs.Discrete(2)), (Box(-1.0, 1.0, (1,), np.float32), rs.Box(-1.0, 1.0, (1,), np.float32))):
        mine.seed(7), ref.seed(7)
        bm, br = batch_space(mine, 6), ref_batch(ref, 6)
        assert type(bm).__name__ == type(br).__name__ and bm.shape == br.shape and bm.dtype == br.dtype
        assert np.array_equal(bm.sample(), br.sample())


def test_batch_space_shapes_and_dtypes():
    b = batch_space(Discrete(3), 8)
    assert isinstance(b, MultiDiscrete) and b.shape == (8,) and b.dtype == np.int64 and np.all(b.nvec == 3)
    bb = batch_space(Box(-2.0, 2.0, (1,), np.float32), 8)
    assert isinstance(bb, Box) and bb.shape == (8, 1) and bb.dtype == np.float32
    obs, _ = single_spaces(spec("CartPole-v1").kind)
    bo = batch_space(obs, 4)
    assert bo.shape == (4, 4) and np.array_equal(bo.high[2], obs.high)
    assert b.contains(np.array([0, 1, 2, 0, 1, 2, 0, 1])) and not b.contains(np.array([0, 1, 3, 0, 1, 2, 0, 1]))
    assert Discrete(2).contains(1) and not Discrete(2).contains(2) and not Discrete(2).contains(1.0)


def test_seeding_rules():
    rng, s = np_random(5)
    assert s == 5 and rng.integers(10) == np.random.Generator(np.random.PCG64(np.random.SeedSequence(5))).integers(10)
    for bad in (-1, 1.5, "x"):
        with pytest.raises(error.Error):  # gym/utils/seeding.py:21-22
            np_random(bad)


def test_lazy_infos_materialise_on_access():
    from gym_amd.vector_env import LazyInfos, _Pending

    calls = []

    def build():
        calls.append(1)
        return np.array([None, 3], dtype=object)

    d = LazyInfos()
    dict.__setitem__(d, "final_observation", _Pending(build))
    dict.__setitem__(d, "_final_observation", np.array([False, True]))
    assert "final_observation" in d and not calls
    assert d["final_observation"][1] == 3 and d.get("final_observation")[0] is None and len(calls) == 1
    assert d.get("missing", 9) == 9
    assert dict(d.items())["_final_observation"][1]


def test_vector_env_base_surface():
    """Names of gym.vector.VectorEnv (vector_env.py:25-206) exist with the same call shapes."""
    from gym_amd.vector_env import HipVectorEnv, VectorEnv

    for name in ("reset_async", "reset_wait", "reset", "step_async", "step_wait", "step", "call_async", "call_wait",
                 "call", "get_attr", "set_attr", "close_extras", "close"):
        assert callable(getattr(VectorEnv, name)) and callable(getattr(HipVectorEnv, name))
    obs, act = single_spaces(spec("Pendulum-v1").kind)
    v = VectorEnv(5, obs, act)
    assert v.num_envs == 5 and v.is_vector_env and v.observation_space.shape == (5, 3) and v.action_space.shape == (5, 1)
    assert v.single_observation_space is obs and not v.closed
    v.close()
    assert v.closed


def test_vector_env_wrapper_forwards_like_the_reference():
    """gym.vector.VectorEnvWrapper (vector_env.py:277-332): explicit forwarding of the VectorEnv methods, implicit of
    public attributes, private ones refused; a subclass hooks reset_async like tests/vector/test_vector_env_wrapper.py."""
    from gym_amd.vector_env import VectorEnv, VectorEnvWrapper

    calls = []

    class Fake(VectorEnv):
        gravity = 9.8

        def reset_async(self, seed=None, options=None):
            calls.append(("reset_async", seed))

        def reset_wait(self, seed=None, options=None):
            return "obs", {}

        def step_async(self, actions):
            calls.append(("step_async", actions))

        def step_wait(self):
            return "step"

        def call(self, name, *a, **k):
            return (getattr(self, name),) * self.num_envs

        def set_attr(self, name, values):
            setattr(self, name, values)

    class Counting(VectorEnvWrapper):
        def __init__(self, env):
            self.env = env
            self.counter = 0

        def reset_async(self, **kwargs):
            super().reset_async(**kwargs)
            self.counter += 1

    obs, act = single_spaces(spec("CartPole-v1").kind)
    base = Fake(3, obs, act)
    w = Counting(base)
    assert w.reset(seed=7) == ("obs", {}) and w.counter == 1 and calls[-1] == ("reset_async", 7)
    assert w.step([0, 1, 0]) == "step" and calls[-1] == ("step_async", [0, 1, 0])
    assert w.num_envs == 3 and w.single_action_space is act and w.unwrapped is base
    assert w.call("gravity") == (9.8, 9.8, 9.8) and w.get_attr("gravity") == (9.8, 9.8, 9.8)
    w.set_attr("gravity", 20.0)
    assert base.gravity == 20.0
    with pytest.raises(AttributeError):
        w._private
    assert repr(w).startswith("<Counting, ")
    with pytest.raises(AssertionError):
        VectorEnvWrapper(object())
    w.close()
    assert base.closed


def test_gym_shaped_namespaces():
    """`import gym_amd as gym`: gym.vector.make / gym.vector.VectorEnv(Wrapper) / gym.wrappers.* / gym.spaces / gym.error."""
    import gym_amd as gym
    import gym_amd.vector

    assert gym.vector.make is gym.make and gym.vector.VectorEnv is gym.VectorEnv
    assert issubclass(gym.vector.VectorEnvWrapper, gym.vector.VectorEnv)
    import gym_amd.spaces as spaces
    import gym_amd.wrappers as wrappers

    for name in ("RecordEpisodeStatistics", "VectorListInfo", "NormalizeObservation", "NormalizeReward"):
        assert getattr(wrappers, name) is getattr(gym, name)
    for name in ("Box", "Discrete", "MultiDiscrete", "Tuple"):
        assert hasattr(spaces, name)
    for name in ("Error", "ResetNeeded", "AlreadyPendingCallError", "NoAsyncCallError", "ClosedEnvironmentError", "UnregisteredEnv"):
        assert issubclass(getattr(gym.error, name), Exception)


def test_make_refuses_per_sub_env_wrappers_loudly():
    """gym.vector.make(wrappers=...) wraps every Python sub-env (gym/vector/__init__.py:56-65); the engine has none and must
    not silently drop them."""
    import gym_amd

    with pytest.raises(NotImplementedError):
        gym_amd.make("CartPole-v1", num_envs=4, wrappers=[lambda e: e])


def test_plugin_registers_with_the_live_reference_registry():
    """gym.register / import hook route gym.make to the engine's entry point."""
    gym = _ref_gym()
    from conftest import HAS_GPU
    import gym_amd.plugin as plugin

    ids = plugin.register_envs(gym)
    assert "hip/CartPole-v1" in ids and "hip/Taxi-v3" in ids and "hip/Blackjack-v1" in ids and len(ids) == len(registry) + 5
    s = gym.spec("hip/Pendulum-v1")
    assert s.max_episode_steps is None and s.order_enforce is False and s.disable_env_checker is True
    assert s.kwargs == {"id": "Pendulum-v1"} and s.namespace == "hip"
    assert plugin.register_envs(gym) == ids  # idempotent
    if not HAS_GPU:
        from gym_amd import _native
        for env_id in ("hip/CartPole-v1", "gym_amd.plugin:hip/Acrobot-v1"):  # plain id and module:id import hook
            with pytest.raises(_native.MxvError) as ei:   # reached mxv_create: no device here, and no CPU fallback
                gym.make(env_id, num_envs=8)
            assert "no HIP device" in str(ei.value) or ei.value.code == _native.ERR_HIP


def test_bench_accounting_is_a_pure_function_of_the_arguments():
    """bench.py: algorithmic bytes per env-step and the repeat count of a short timed region — the driver runs
    `--steps 20 --warmup 5`, every rank must derive the same launches from the arguments alone."""
    import bench

    assert bench.algorithmic_bytes_per_env_step("fused", 256) == pytest.approx(4 * 4 + 4 + 4 + 2 + 16 * 4 / 256) == pytest.approx(26.25)
    assert bench.algorithmic_bytes_per_env_step("fused", 20) == pytest.approx(29.2)
    assert bench.algorithmic_bytes_per_env_step("eager", 1) == 66
    r = bench.timed_repeats(20, 256, 1 << 20, 60.0)
    assert r == 512 and (r * 20) % 256 == 0 and r * 20 * 6e-3 >= 60.0          # 40 whole launches of 256 steps, >= 60 ms nominal
    assert bench.timed_repeats(20480, 256, 1 << 20, 60.0) == 1                  # the default run is long enough as it is
    r8 = bench.timed_repeats(20, 256, 1 << 17, 60.0)                            # an 8-GPU strong-scaling shard: 8x shorter steps
    assert r8 >= 8 * 500 and (r8 * 20) % 256 == 0
    assert bench.timed_repeats(20, 256, 1 << 20, 60.0, mode="eager") == 500


def test_array_pool_recycles_only_what_nobody_references():
    """_ArrayPool (gym_amd/_native.py): a buffer goes out again only when the caller dropped the array it got AND every view of it."""
    from gym_amd._native import _ArrayPool

    pool = _ArrayPool(limit=2)
    a = pool.take((1000, 4), np.float32)
    b = pool.take((1000, 4), np.float32)
    assert a.ctypes.data != b.ctypes.data and a.shape == (1000, 4) and a.dtype == np.float32 and a.flags.c_contiguous and a.flags.writeable
    pa, pb = a.ctypes.data, b.ctypes.data
    view = a[10:20]
    del a
    c = pool.take((1000, 4), np.float32)          # a's memory is still visible through `view`; b is held: a third array (unpooled: limit 2)
    assert c.ctypes.data not in (pa, pb)
    del view, c
    d = pool.take((1000, 4), np.float32)
    assert d.ctypes.data == pa                    # now a's buffer is free again
    e = pool.take((1000,), np.float32)            # another shape: its own list
    assert e.shape == (1000,)
    del b
    f = pool.take((1000, 4), np.float32)
    assert f.ctypes.data == pb


def test_pools_do_not_depend_on_reference_counts():
    """Round 3's pools asked sys.getrefcount whether "nobody holds this array"; a tracer, a debugger holding a frame or an interpreter
    with different borrowed-reference rules changes that number silently, and a step would have overwritten an array the caller kept
    (engineering #9).  Ownership is explicit now (a lease object that is the base of the array and of every view, returned
    by its finalizer): 100 hand-outs kept in a list under sys.settrace, with extra references to each array parked in frames,
    containers and views, never alias each other or a later hand-out."""
    import gc
    import sys

    from gym_amd._native import _ArrayPool

    pool = _ArrayPool(limit=4)
    kept, events = [], []

    def tracer(frame, event, arg):          # holds frames (and through them locals) alive, as a debugger or coverage tool does
        events.append(frame)
        return tracer

    def step(i):
        arr = pool.take((257, 3), np.float32)
        arr[:] = i
        extra = {"alias": arr, "slice": arr[5:7], "T": arr.T}        # more references of every kind
        return arr, extra

    sys.settrace(tracer)
    try:
        for i in range(100):
            arr, extra = step(i)
            kept.append(arr if i % 2 else extra["slice"])            # sometimes only a VIEW survives
            scratch = pool.take((257, 3), np.float32)                # taken and dropped at once: the buffers that do get recycled
            scratch[:] = -1.0
            del scratch, arr, extra
    finally:
        sys.settrace(None)
    for i, k in enumerate(kept):
        assert np.all(k == i), f"hand-out {i} was overwritten while the caller still held it"
    ptrs = {k.ctypes.data - (0 if i % 2 else 5 * 3 * 4) for i, k in enumerate(kept)}
    assert len(ptrs) == 100
    del kept, events
    gc.collect()
    again = [pool.take((257, 3), np.float32) for _ in range(4)]       # everything came back: the pool hands out pooled buffers again
    assert all(type(a.base).__name__ == "_Lease" for a in again)


def test_large_env_adapter_paths_on_a_packed_stand_in(monkeypatch):
    """HipVectorEnv + RecordEpisodeStatistics + VectorListInfo over a handle that reports packed final records (what a large
    vector env does on the device): infos built from the packed rows equal what the dense path builds, step for step."""
    from oracle_engine import FakeHandle, PackedFakeHandle

    import gym_amd
    from gym_amd import _native

    n = 64
    monkeypatch.setattr(_native, "Handle", PackedFakeHandle)
    packed = gym_amd.RecordEpisodeStatistics(gym_amd.make("CartPole-v1", num_envs=n, max_episode_steps=7), deque_size=5)
    assert packed.unwrapped._packed
    monkeypatch.setattr(_native, "Handle", FakeHandle)
    dense = gym_amd.make("CartPole-v1", num_envs=n, max_episode_steps=7)
    assert not dense._packed
    packed.reset(seed=3), dense.reset(seed=3)
    dense.action_space.seed(4)
    from oracle.oracle import EpisodeStats

    stats = EpisodeStats(n)
    want_r, want_l, count = [], [], 0
    for t in range(40):
        a = dense.action_space.sample()
        o1, r1, te1, tr1, i1 = packed.step(a)
        o2, r2, te2, tr2, i2 = dense.step(a)
        assert np.array_equal(o1, o2) and np.array_equal(r1, r2) and np.array_equal(te1, te2) and np.array_equal(tr1, tr2)
        er, el, done = stats.step(r2, te2, tr2)
        if not done.any():
            assert "episode" not in i1 and "final_observation" not in i1
            continue
        assert set(i1) == set(i2) | {"episode", "_episode"}
        f1, f2 = i1["final_observation"], i2["final_observation"]
        for i in range(n):
            assert (f1[i] is None) == (f2[i] is None) == (not done[i])
            if done[i]:
                assert np.array_equal(f1[i], f2[i])
        assert np.array_equal(i1["_final_observation"], done) and np.array_equal(i1["_final_info"], done)
        ep = i1["episode"]
        assert np.array_equal(ep["r"], er.astype(np.float64)) and np.array_equal(ep["l"], el.astype(np.float64))
        assert np.array_equal(i1["_episode"], done) and np.array_equal(ep["t"] > 0, done)
        idx = np.flatnonzero(done)
        want_r += er[idx].tolist()
        want_l += el[idx].tolist()
        count += idx.size
        assert packed.episode_count == count
        assert list(packed.return_queue) == want_r[-5:] and list(packed.length_queue) == want_l[-5:]
        assert dict(i1).keys() == i1.keys() and isinstance(dict(i1)["episode"], dict)   # placeholders resolve on every way out
    assert count > n
    # VectorListInfo over the packed path
    monkeypatch.setattr(_native, "Handle", PackedFakeHandle)
    env = gym_amd.VectorListInfo(gym_amd.RecordEpisodeStatistics(gym_amd.make("CartPole-v1", num_envs=8, max_episode_steps=2)))
    env.reset(seed=1)
    env.step(np.zeros(8, dtype=np.int64))
    infos = env.step(np.zeros(8, dtype=np.int64))[4]
    assert isinstance(infos, list) and all(d["episode"]["l"] == 2.0 and d["final_observation"].shape == (4,) for d in infos)


@pytest.mark.parametrize("env_name", ["Acrobot-v1", "CartPole-v1", "MountainCar-v0", "MountainCarContinuous-v0"])
def test_customizable_resets_like_the_reference_tests(env_name, monkeypatch):
    """tests/envs/test_env_implementation.py:150-215 restated for the vector adapter (oracle-backed stand-in handle): reset
    options low/high as floats or 0-d arrays bound every state component; strings, low > high, lists and 1-d arrays raise
    ValueError (classic_control/utils.py:8-46); Pendulum takes x_init / y_init instead (pendulum.py:141-159)."""
    from oracle_engine import FakeHandle

    import gym_amd
    from gym_amd import _native

    monkeypatch.setattr(_native, "Handle", FakeHandle)
    for low_high in (None, (-0.4, 0.4), (np.array(-0.4), np.array(0.4))):
        env = gym_amd.make(env_name, num_envs=16)
        env.action_space.seed(0)
        if low_high is None:
            env.reset()
        else:
            low, high = low_high
            env.reset(options={"low": low, "high": high})
            st = env.handle.o.state
            assert np.all((st >= low) & (st <= high))
        env.step(env.action_space.sample())
        env.close()
    for low_high in (("x", "y"), (10.0, 8.0), ([-1.0, -1.0], [1.0, 1.0]), (np.array([-1.0, -1.0]), np.array([1.0, 1.0]))):
        env = gym_amd.make(env_name, num_envs=4)
        with pytest.raises(ValueError):
            env.reset(options={"low": low_high[0], "high": low_high[1]})
        env.close()


def test_customizable_pendulum_resets_like_the_reference_test(monkeypatch):
    from oracle_engine import FakeHandle

    import gym_amd
    from gym_amd import _native

    monkeypatch.setattr(_native, "Handle", FakeHandle)
    for low_high in (None, (1.2, 1.0), (np.array(1.2), np.array(1.0))):
        env = gym_amd.make("Pendulum-v1", num_envs=32)
        env.action_space.seed(0)
        if low_high is None:
            env.reset()
            st = env.handle.o.state
            assert np.all(np.abs(st[0]) <= np.pi) and np.all(np.abs(st[1]) <= 1.0)
        else:
            x, y = low_high
            env.reset(options={"x_init": x, "y_init": y})
            st = env.handle.o.state
            assert np.all(np.abs(st[0]) <= 1.2) and np.all(np.abs(st[1]) <= 1.0)
        env.step(env.action_space.sample())
        env.close()


@pytest.mark.parametrize("env_name", ["Pendulum-v1", "MountainCarContinuous-v0"])
def test_box_actions_out_of_bound_like_the_reference_test(env_name, monkeypatch):
    """tests/envs/test_action_dim_check.py:90-136: a Box action beyond a bound has the effect of the action AT the bound (the envs
    clip inside step); discrete envs reject out-of-range actions (:62-78)."""
    from oracle_engine import FakeHandle

    import gym_amd
    from gym_amd import _native

    monkeypatch.setattr(_native, "Handle", FakeHandle)
    n = 8
    env, oob_env = gym_amd.make(env_name, num_envs=n), gym_amd.make(env_name, num_envs=n)
    env.reset(seed=42), oob_env.reset(seed=42)
    hi, lo = env.single_action_space.high, env.single_action_space.low
    for bound, sign in ((hi, +1), (lo, -1)):
        a = np.tile(bound, (n, 1)).astype(np.float32)
        obs = env.step(a)[0]
        oob_obs = oob_env.step(a + np.float32(sign * 100))[0]
        if env_name == "Pendulum-v1":
            assert np.all(obs == oob_obs)
        else:
            # MountainCarContinuous under NumPy 2 (NEP 50): `min(max(action[0], min_action), max_action)` hands back the float32
            # action itself AT the bound but the Python-float bound beyond it, so `force * self.power` is a float32 product in one
            # case and a float64 product in the other (continuous_mountain_car.py:146-148): the reference — and
            # therefore the oracle and the engine — may differ in the last float32 bit of the velocity between the two
            np.testing.assert_allclose(obs, oob_obs, rtol=3e-7, atol=1e-9)
    env.close(), oob_env.close()
    disc = gym_amd.make("CartPole-v1", num_envs=4)
    disc.reset(seed=0)
    with pytest.raises(Exception):
        disc.step(np.full(4, disc.single_action_space.n))
    disc.close()


@pytest.mark.parametrize("packed", [False, True])
def test_adapter_error_and_time_limit_contract_on_the_stand_in(packed, monkeypatch):
    """The ordering / error / TimeLimit contract of the NumPy adapter without a device (the same checks run against the HIP
    engine in tests/test_gpu_vector_env.py): order_enforcing.py:33-37, seeding.py:21-22, cartpole.py:131-132,
    async_vector_env.py's pending-call errors, time_limit.py:50-54 and tests/wrappers/test_time_limit.py:38-57."""
    from oracle_engine import FakeHandle, PackedFakeHandle

    import gym_amd
    from gym_amd import _native, error

    monkeypatch.setattr(_native, "Handle", PackedFakeHandle if packed else FakeHandle)
    env = gym_amd.make("CartPole-v1", num_envs=8)
    with pytest.raises(error.ResetNeeded):
        env.step(np.zeros(8, dtype=np.int64))
    with pytest.raises(error.Error):
        env.reset(seed=-1)
    obs, info = env.reset(seed=0)
    assert info == {} and obs.shape == (8, 4)
    with pytest.raises(AssertionError):
        env.step(np.full(8, 2, dtype=np.int64))
    with pytest.raises(AssertionError):
        env.step(np.zeros(8, dtype=np.float32))
    with pytest.raises(error.NoAsyncCallError):
        env.step_wait()
    env.step_async(np.zeros(8, dtype=np.int64))
    with pytest.raises(error.AlreadyPendingCallError):
        env.step_async(np.zeros(8, dtype=np.int64))
    env.step_wait()
    env.step(np.ones(8, dtype=np.int64))
    env.close()
    with pytest.raises(error.ClosedEnvironmentError):
        env.step(np.ones(8, dtype=np.int64))
    with pytest.raises(error.UnregisteredEnv):
        gym_amd.make("LunarLander-v2", num_envs=8)
    with pytest.raises(TypeError):
        gym_amd.make("CartPole-v1", num_envs=8, g=1.0)
    # TimeLimit: truncation every third step; termination and truncation can coincide
    env = gym_amd.make("CartPole-v1", num_envs=16, max_episode_steps=3)
    env.reset(seed=0)
    for k in range(1, 7):
        _, _, term, trunc, infos = env.step(np.zeros(16, dtype=np.int64))
        assert np.all(trunc == (k % 3 == 0))
        if k % 3 == 0:
            assert infos["_final_observation"].all() and all(o.shape == (4,) for o in infos["final_observation"])
    st, el = env.handle.get_state()
    st[0, :], st[1, :], el[:] = 2.399, 5.0, 2
    env.handle.set_state(st, el)
    _, _, term, trunc, infos = env.step(np.ones(16, dtype=np.int64))
    assert term.all() and trunc.all() and infos["_final_observation"].all()
    assert all(abs(o[0]) > 2.4 for o in infos["final_observation"])      # the terminal observation, not the reset one
    env.close()


def _space_pairs(rs):
    from gym_amd.spaces import Tuple

    box_m, box_r = Box(-1.0, 1.0, (3,), np.float32), rs.Box(-1.0, 1.0, (3,), np.float32)
    md_m, md_r = MultiDiscrete([3, 4]), rs.MultiDiscrete([3, 4])
    return [("box", box_m, box_r), ("discrete", Discrete(5), rs.Discrete(5)), ("multidiscrete", md_m, md_r),
            ("tuple", Tuple((box_m, md_m)), rs.Tuple((box_r, md_r)))]


def test_vector_utils_against_the_reference():
    """gym_amd.vector.utils.{batch_space, create_empty_array, concatenate, iterate} do what gym.vector.utils does for the spaces this engine
    has (gym/vector/utils/numpy_utils.py:14-150, spaces.py:17-212; the reference's own tests: tests/vector/test_numpy_utils.py,
    tests/vector/test_spaces.py)."""
    gym = _ref_gym()
    from gym import spaces as rs
    from gym.vector import utils as ru

    from gym_amd.vector import utils as mu

    def same(a, b):
        if isinstance(a, tuple):
            assert isinstance(b, tuple) and len(a) == len(b)
            for x, y in zip(a, b):
                same(x, y)
        else:
            a, b = np.asarray(a), np.asarray(b)
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)

    n = 4
    for name, mine, ref in _space_pairs(rs):
        mine.seed(11), ref.seed(11)
        # batch_space: class, shape, dtype, bounds, and the same sample stream
        bm, br = mu.batch_space(mine, n), ru.batch_space(ref, n)
        assert type(bm).__name__ == type(br).__name__, name
        if name != "tuple":
            assert bm.shape == br.shape and bm.dtype == br.dtype, name
            if isinstance(bm, Box):
                assert np.array_equal(bm.low, br.low) and np.array_equal(bm.high, br.high)
        same(bm.sample(), br.sample())
        # create_empty_array: n elements, one element (n=None), another constructor
        same(mu.create_empty_array(mine, n), ru.create_empty_array(ref, n))
        same(mu.create_empty_array(mine, None), ru.create_empty_array(ref, None))
        same(mu.create_empty_array(mine, 2, fn=np.ones), ru.create_empty_array(ref, 2, fn=np.ones))
        # concatenate: stack n samples into the preallocated batch; the result IS `out` for array spaces
        items_m = [mine.sample() for _ in range(n)]
        items_r = [ref.sample() for _ in range(n)]
        out_m, out_r = mu.create_empty_array(mine, n), ru.create_empty_array(ref, n)
        cm, cr = mu.concatenate(mine, items_m, out_m), ru.concatenate(ref, items_r, out_r)
        same(cm, cr)
        if name != "tuple":
            assert cm is out_m
        # iterate: the batch taken apart again (Discrete: TypeError, in both)
        if name == "discrete":
            with pytest.raises(TypeError):
                mu.iterate(mine, cm)
            with pytest.raises(TypeError):
                ru.iterate(ref, cr)
        else:
            back_m, back_r = list(mu.iterate(mine, cm)), list(ru.iterate(ref, cr))
            assert len(back_m) == len(back_r) == n
            for x, y, item in zip(back_m, back_r, items_m):
                same(x, y)
                same(x, item)
    with pytest.raises(TypeError):
        mu.iterate(Box(-1.0, 1.0, (3,), np.float32), 5)           # not iterable (spaces.py:171-175)


def test_vector_utils_without_the_reference():
    from gym_amd.error import CustomSpaceError
    from gym_amd.spaces import Space, Tuple
    from gym_amd.vector import utils as mu

    class Odd(Space):
        pass

    odd = Odd((), np.float32)
    assert mu.create_empty_array(odd, 3) is None and mu.concatenate(odd, [1, 2], None) == (1, 2)
    with pytest.raises(CustomSpaceError):
        mu.iterate(odd, [1, 2])
    for f in (lambda: mu.create_empty_array("no space"), lambda: mu.concatenate(3, [], None), lambda: mu.iterate(None, [])):
        with pytest.raises(ValueError):
            f()
    t = Tuple((Box(0.0, 1.0, (2,), np.float32), MultiDiscrete([2, 2])))
    out = mu.create_empty_array(t, 3)
    assert isinstance(out, tuple) and out[0].shape == (3, 2) and out[0].dtype == np.float32 and out[1].shape == (3, 2) and out[1].dtype == np.int64
    rows = list(mu.iterate(t, out))
    assert len(rows) == 3 and rows[0][0].shape == (2,) and rows[0][1].shape == (2,)
    b = mu.batch_space(MultiDiscrete([3, 4]), 5)
    assert isinstance(b, Box) and b.shape == (5, 2) and b.dtype == np.int64 and np.array_equal(b.high[0], [2, 3]) and np.all(b.low == 0)
    import gym_amd
    assert gym_amd.vector.utils is mu and gym_amd.vector.make is gym_amd.make


@pytest.mark.parametrize("gid", ["CartPole-v1", "Pendulum-v1", "Acrobot-v1", "MountainCar-v0", "MountainCarContinuous-v0"])
def test_call_state_has_the_references_container_types(gid, monkeypatch):
    """VectorEnv.call("state") against the reference's answers (tests/golden/live_call_state.json, make_golden_live.py: a SyncVectorEnv of 3
    envs after reset(seed=1) and after a step of the recorded actions): the reference's sub-envs hold their state in different
    containers (ndarray of the generator's dtype vs tuple / float32 array); the adapter reproduces container, dtype and shape — and
    `_elapsed_steps`, `_max_episode_steps`, `render_mode` — value for value."""
    import json
    import os

    from oracle_engine import FakeHandle

    import gym_amd
    from gym_amd import _native

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live_call_state.json")) as f:
        phases = json.load(f)[gid]
    monkeypatch.setattr(_native, "Handle", FakeHandle)
    env = gym_amd.make(gid, num_envs=3)
    env.reset(seed=1)

    def same_kind(a, want):
        if want["type"] == "ndarray":
            assert isinstance(a, np.ndarray), (type(a), want)
            assert str(a.dtype) == want["dtype"] and list(a.shape) == want["shape"], (a.dtype, a.shape, want)
        else:
            assert type(a).__name__ == want["type"] and len(a) == want["len"], (type(a), want)
            assert want["all_float"] and all(isinstance(x, float) for x in a)

    for ph in phases:        # after reset, after a step
        ea = env.call("state")
        assert isinstance(ea, tuple) and len(ea) == 3
        for a, want in zip(ea, ph["state"]):
            same_kind(a, want)
        assert list(env.call("_elapsed_steps")) == ph["_elapsed_steps"] and list(env.call("_max_episode_steps")) == ph["_max_episode_steps"]
        assert list(env.call("render_mode")) == ph["render_mode"]
        env.step(np.asarray(ph["action"], dtype=ph["action_dtype"]))
    env.close()


def test_partials_are_attached_and_detached_by_call_shape():
    """DeviceRollout's bookkeeping of the fused-moment buffers (mxv_set_obs_partials / mxv_set_return_partials) on a stand-in handle:
    attached when a trajectory call brings them, detached before every call shape that does not fill them (the C ABI would refuse),
    re-attached when the normaliser behind the returns changes, refused without one."""
    from gym_amd.rollout import DeviceRollout

    calls = []

    class H:
        def set_obs_partials(self, p):
            calls.append(("obs", p))

        def set_return_partials(self, ptr, gamma, p):
            calls.append(("ret", ptr, gamma, p))

    r = object.__new__(DeviceRollout)
    r.handle = H()
    P, Q = object(), object()
    r._attach_partials(None, None)
    assert calls == []                                            # nothing attached, nothing to do
    r._attach_partials(P, None)
    r._attach_partials(P, None)
    assert calls == [("obs", P)]                                  # once per change
    with pytest.raises(RuntimeError):
        r._attach_partials(P, Q)                                  # returns need a normaliser first

    class Backend:
        def __init__(self, ptr):
            self.ptr = ptr

        def returns_ptr(self):
            return self.ptr

    class Nz:
        def __init__(self, ptr, gamma):
            self.backend, self.gamma = Backend(ptr), gamma

    a = Nz(0x1000, 0.9)
    r.fuse_reward_normalizer(a)
    r._attach_partials(P, Q)
    assert calls[-1] == ("ret", 0x1000, 0.9, Q) and r._fused_normalizer is a
    b = Nz(0x2000, 0.5)
    r.fuse_reward_normalizer(b)                                   # another normaliser: detach now, attach its array at the next rollout
    assert calls[-1] == ("ret", None, 0.0, None)
    r._attach_partials(P, Q)
    assert calls[-1] == ("ret", 0x2000, 0.5, Q)
    n = len(calls)
    r._attach_partials(None, None)                                # what step() / rollout() / rollout_tape() do first
    assert calls[n:] == [("obs", None), ("ret", None, 0.0, None)]


def test_normaliser_folds_partials_instead_of_reading_the_batch_again():
    """RunningNormalizer.normalize_obs / normalize_rewards with `partials=`: the backend's *_sums_partials is called with the leaf count of
    the buffer, the pass over the batch is not."""
    import torch

    from gym_amd.normalize import RunningNormalizer

    log = []

    class B:
        stream, torch_device = None, torch.device("cpu")

        def obs_sums(self, K, x, sums):
            log.append("obs_sums")

        def obs_sums_partials(self, K, partials, sums):
            log.append(("obs_partials", K, partials.shape[-2]))

        def obs_apply(self, K, x, y, eps, all_sums, world, total):
            log.append(("obs_apply", tuple(all_sums.shape)))

        def reward_sums(self, K, r, te, tr, gamma, sums):
            log.append("reward_sums")

        def reward_sums_partials(self, K, partials, sums):
            log.append(("ret_partials", K, partials.shape[-2]))

        def reward_apply(self, K, r, out, eps, all_sums, world, total):
            log.append(("reward_apply", tuple(all_sums.shape)))

    n, K, O, leaves = 256, 3, 4, 2
    nz = RunningNormalizer(n, O, backend=B())
    x = torch.zeros((K, n, O), dtype=torch.float32)
    nz.normalize_obs(x, partials=torch.zeros((K, leaves, 2 * O), dtype=torch.float64))
    nz.normalize_obs(x)
    r, f = torch.zeros((K, n), dtype=torch.float64), torch.zeros((K, n), dtype=torch.uint8)
    nz.normalize_rewards(r, f, f, partials=torch.zeros((K, leaves, 2), dtype=torch.float64))
    nz.normalize_rewards(r, f, f)
    assert log == [("obs_partials", K, leaves), ("obs_apply", (1, K, 2 * O)), "obs_sums", ("obs_apply", (1, K, 2 * O)),
                   ("ret_partials", K, leaves), ("reward_apply", (1, K, 2)), "reward_sums", ("reward_apply", (1, K, 2))]
    with pytest.raises(AssertionError):
        nz.normalize_obs(x, partials=torch.zeros((K, leaves, 2 * O + 1), dtype=torch.float64))


def test_vector_make_recognises_the_sub_env_wrappers_it_can_map():
    """gym.vector.make(..., wrappers=...) (gym/vector/__init__.py:56-65): TimeLimit / RecordEpisodeStatistics / OrderEnforcing /
    PassiveEnvChecker as classes or functools.partial — the reference's classes where the reference is importable, this package's, or any
    class of that name — are mapped; Normalize* (per-sub-env statistics are a different normalisation) and everything else say why not."""
    import functools

    from gym_amd.vector_env import _sub_env_wrappers
    from gym_amd.wrappers import NormalizeObservation, RecordEpisodeStatistics

    TimeLimit = reference_wrapper_stub("TimeLimit")

    OrderEnforcing = reference_wrapper_stub("OrderEnforcing")

    assert _sub_env_wrappers(None) == (None, [])
    assert _sub_env_wrappers(TimeLimit) == (None, [])                                      # max_episode_steps=None: the spec's own limit
    assert _sub_env_wrappers(functools.partial(TimeLimit, max_episode_steps=25)) == (25, [])
    assert _sub_env_wrappers([functools.partial(TimeLimit, max_episode_steps=25), OrderEnforcing,
                              functools.partial(TimeLimit, max_episode_steps=9)]) == (9, [])
    ClipAction = reference_wrapper_stub("ClipAction")

    assert _sub_env_wrappers([ClipAction]) == (None, [("identity_for_classic_control", {"wrapper": "ClipAction"})])
    assert _sub_env_wrappers((RecordEpisodeStatistics,)) == (None, [("episode_statistics", {})])
    assert _sub_env_wrappers([functools.partial(RecordEpisodeStatistics, deque_size=5)]) == (None, [("episode_statistics", {"deque_size": 5})])
    assert _sub_env_wrappers([NormalizeObservation]) == (None, [("normalize_observation", {})])
    assert _sub_env_wrappers([functools.partial(NormalizeObservation, epsilon=1e-6)]) == (None, [("normalize_observation", {"epsilon": 1e-6})])
    for bad, needle in ((lambda e: e, "cannot run inside the device engine"), (functools.partial(NormalizeObservation, foo=1), "cannot run"),
                        (functools.partial(TimeLimit, new_step_api=True), "not supported"), (functools.partial(TimeLimit, 5), "cannot run"),
                        ([3], "cannot run"), (7, "callable or an iterable")):
        with pytest.raises(NotImplementedError) as e:
            _sub_env_wrappers(bad)
        assert needle in str(e.value), (bad, str(e.value))
    # classes with the reference's own names and home modules (tests/golden/live_reference_facts.json, make_golden_live.py)
    import json

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live_reference_facts.json")) as f:
        homes = json.load(f)["wrappers"]
    RefLimit, RefStats = (type(n, (), {"__module__": homes[n]}) for n in ("TimeLimit", "RecordEpisodeStatistics"))
    assert _sub_env_wrappers([functools.partial(RefLimit, max_episode_steps=30), RefStats]) == (30, [("episode_statistics", {})])


def test_vector_make_wrappers_replay_the_reference_on_the_host_adapter(monkeypatch):
    """The host side of make(wrappers=[partial(TimeLimit, max_episode_steps=12), RecordEpisodeStatistics]) without a device: the adapter over
    an oracle-backed handle (tests/oracle_engine.py) replays tests/golden/vector_make_wrappers_CartPole.npz — what the REFERENCE's
    per-sub-env wrappers produced — mask for mask, with `final_info[i]["episode"]` where the reference puts it (the GPU twin of this
    test, through the HIP engine: tests/test_gpu_vector_env.py)."""
    import functools

    import gym_amd
    from gym_amd import _native
    from gym_amd.wrappers import RecordEpisodeStatistics, SubEnvEpisodeStatistics
    from oracle_engine import PackedFakeHandle

    TimeLimit = reference_wrapper_stub("TimeLimit")

    monkeypatch.setattr(_native, "Handle", PackedFakeHandle)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vector_make_wrappers_CartPole.npz"))
    T, N = g["action"].shape
    env = gym_amd.make("CartPole-v1", num_envs=N, wrappers=[functools.partial(TimeLimit, max_episode_steps=int(g["max_episode_steps"])),
                                                             functools.partial(RecordEpisodeStatistics, deque_size=7)])
    assert isinstance(env, SubEnvEpisodeStatistics) and env.return_queue.maxlen == 7
    env.reset(seed=1)
    handle = env.unwrapped.handle
    episodes = 0
    for t in range(T):
        handle.set_state(np.ascontiguousarray(g["state_pre"][t].T), g["elapsed_pre"][t])
        obs, rew, term, trunc, infos = env.step(g["action"][t])
        assert np.array_equal(term, g["terminated"][t]) and np.array_equal(trunc, g["truncated"][t]) and np.array_equal(rew, g["reward"][t]), t
        assert "episode" not in infos and "_episode" not in infos
        done = g["ep_mask"][t]
        assert np.array_equal(obs[~done], g["obs"][t][~done])            # the oracle is bit-exact against the reference
        for i in np.flatnonzero(done):
            ep = infos["final_info"][i]["episode"]
            assert isinstance(ep["r"], np.float32) and isinstance(ep["l"], np.int32) and isinstance(ep["t"], float)
            assert ep["r"] == g["ep_r"][t][i] and ep["l"] == g["ep_l"][t][i], (t, i, ep)
            episodes += 1
    assert episodes == int(g["ep_mask"].sum()) and env.episode_count == episodes and len(env.return_queue) == 7
    env.close()


def test_vector_make_identity_wrappers(monkeypatch):
    """ClipAction around a Box-action sub-env clips to the bounds the env's own step clips to first (pendulum.py:126,
    continuous_mountain_car.py:148-149), FlattenObservation flattens what is flat: accepted as identities for the classic-control ids,
    refused elsewhere (ClipAction asserts a Box action space, clip_action.py:28)."""
    import gym_amd
    from gym_amd import _native
    from oracle_engine import FakeHandle

    ClipAction = reference_wrapper_stub("ClipAction")

    FlattenObservation = reference_wrapper_stub("FlattenObservation")

    monkeypatch.setattr(_native, "Handle", FakeHandle)
    env = gym_amd.make("Pendulum-v1", num_envs=3, wrappers=[ClipAction, FlattenObservation])
    plain = gym_amd.make("Pendulum-v1", num_envs=3)
    env.reset(seed=4), plain.reset(seed=4)
    a = np.array([[5.0], [-7.0], [0.3]], dtype=np.float32)                  # beyond the bounds: the env's own clip handles it
    for x, y in zip(env.step(a)[:4], plain.step(a)[:4]):
        assert np.array_equal(x, y)
    env.close(), plain.close()
    with pytest.raises(NotImplementedError):
        gym_amd.make("CartPole-v1", num_envs=3, wrappers=ClipAction)
    gym_amd.make("CartPole-v1", num_envs=3, wrappers=FlattenObservation).close()


def test_vector_make_clipaction_is_applied_where_it_is_not_an_identity(monkeypatch):
    """MountainCarContinuous-v0 charges its action penalty on the action AS GIVEN (continuous_mountain_car.py:169): under the reference's
    per-sub-env ClipAction that is the clipped action.  The reference's own run (golden), bit for bit over the oracle-backed handle."""
    from gym_amd import _native
    from helpers import replay_vector_make_clipaction
    from oracle_engine import FakeHandle

    monkeypatch.setattr(_native, "Handle", FakeHandle)
    assert replay_vector_make_clipaction(exact=True) == 60


@pytest.mark.parametrize("name", ["Pendulum", "MountainCarContinuous"])
def test_vector_make_rescaleaction_matches_the_reference_bit_for_bit(monkeypatch, name):
    """wrappers=partial(RescaleAction, min_action=, max_action=): the reference's own run (golden) over the oracle-backed handle; the action
    space is the rescaled one; Discrete-action ids are refused like the reference refuses them (rescale_action.py:45-47)."""
    import functools

    import gym_amd
    from gym_amd import _native
    from helpers import replay_vector_make_rescaleaction
    from oracle_engine import FakeHandle

    monkeypatch.setattr(_native, "Handle", FakeHandle)
    assert replay_vector_make_rescaleaction(name, exact=True) == 60
    with pytest.raises(NotImplementedError):
        gym_amd.make("CartPole-v1", num_envs=3, wrappers=functools.partial(reference_wrapper_stub("RescaleAction"), min_action=-1.0, max_action=1.0))


def test_vector_make_transform_wrappers_replay_the_reference_bit_for_bit(monkeypatch):
    """wrappers=[TimeLimit, ClipAction, NormalizeObservation, TransformObservation(clip), NormalizeReward, TransformReward(clip)] — the
    continuous-control PPO recipe — as the reference ran it (golden), over the oracle-backed handle: the observation transform sees the
    float64 rows, the batch rounds to float32 afterwards, final observations stay float64; f is applied to whole batches once checked."""
    from gym_amd import _native
    from gym_amd.wrappers import _RowMap
    from helpers import replay_vector_make_transform
    from oracle_engine import FakeHandle

    monkeypatch.setattr(_native, "Handle", FakeHandle)
    assert replay_vector_make_transform(exact=True) > 40
    # a function that is NOT elementwise over the batch axis stays row by row, with the reference's per-sub-env result
    m = _RowMap(lambda o: o - o.mean())
    x = np.arange(12, dtype=np.float64).reshape(4, 3)
    assert np.array_equal(m(x), x - x.mean(axis=1, keepdims=True)) and m.batched is False and np.array_equal(m(x + 1), x - x.mean(axis=1, keepdims=True))
    m = _RowMap(lambda r: 0.01 * r)
    assert np.array_equal(m(np.array([1.0, -2.0])), np.array([0.01, -0.02])) and m.batched is True


def test_vector_make_recognises_wrappers_by_name_and_home(monkeypatch):
    """A user class that merely shares a name with a known wrapper keeps its own semantics: it must reach the explicit error, not be
    replaced by the engine's mapping."""
    from gym_amd.vector_env import _sub_env_wrappers

    class TimeLimit:                       # home module: this test file
        def __init__(self, env, max_episode_steps=None):
            self.env = env

    with pytest.raises(NotImplementedError):
        _sub_env_wrappers([TimeLimit])
    assert _sub_env_wrappers([reference_wrapper_stub("TimeLimit")]) == (None, [])


@pytest.mark.parametrize("name", ["CartPole", "Pendulum"])
def test_vector_make_normalize_wrappers_replay_the_reference_bit_for_bit(name, monkeypatch):
    """wrappers=[TimeLimit, NormalizeObservation, NormalizeReward, RecordEpisodeStatistics] around every sub-env, as the reference runs them
    (gym/vector/__init__.py:56-65 + gym/wrappers/normalize.py:50-145): per-sub-env running statistics with batches of one, the terminal and
    the reset observation of a finished sub-env as two updates, float32 batched / float64 final observations, episode returns of normalised
    rewards — gym_amd's per-sub-env wrappers over the oracle-backed handle reproduce the reference's own run BIT FOR BIT."""
    from gym_amd import _native
    from helpers import replay_vector_make_normalize
    from oracle_engine import PackedFakeHandle

    monkeypatch.setattr(_native, "Handle", PackedFakeHandle)
    assert replay_vector_make_normalize(name, exact=True) > 50
