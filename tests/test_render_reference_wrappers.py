"""render_mode through gym.make and the reference's own wrappers, on the CPU: the engine's single env over the oracle-backed handle
(tests/oracle_engine.FakeHandle) with the frame drawn by the host restatement (tests/render_host.py) in place of the device launch —
what is checked here is the plumbing the GPU box cannot import the reference for: gym.make("hip/<id>", render_mode=...), the reference's
env checker WITHOUT skip_render_check, PixelObservationWrapper, RenderCollection (rgb_array_list).  tests/test_gpu_render.py holds the
device's frames to the same restatement bit for bit."""
import os
import sys
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import render_host as rh  # noqa: E402


@pytest.fixture
def ref_gym(monkeypatch):
    from test_host_logic import _ref_gym

    gym = _ref_gym()
    from gym_amd import _native, _render, plugin
    from oracle_engine import FakeHandle

    def host_frames(handle, indices=None):
        st, p = handle.get_state()[0], handle.get_params()
        idx = range(handle.num_envs) if indices is None else indices
        return np.stack([rh.render(rh.KIND_NAME[handle.env_id], st[:, i], p) for i in idx])

    monkeypatch.setattr(_native, "Handle", FakeHandle)
    monkeypatch.setattr(_render, "render_host", host_frames)
    plugin.register_envs(gym)
    return gym


@pytest.mark.parametrize("gid", ["CartPole-v1", "Acrobot-v1", "MountainCar-v0", "MountainCarContinuous-v0"])
def test_env_checker_with_the_render_check(ref_gym, gid):
    from gym.utils.env_checker import check_env

    env = ref_gym.make("hip/" + gid, render_mode="rgb_array", disable_env_checker=True)
    assert env.unwrapped.metadata["render_modes"] == ["rgb_array"] and env.unwrapped.render_mode == "rgb_array"
    assert env.unwrapped.render() is None                      # before reset
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        check_env(env.unwrapped)
    msgs = [str(x.message) for x in w]
    assert not msgs, msgs
    env.reset(seed=0)
    f = env.render()
    assert f.dtype == np.uint8 and f.shape == rh.DIMS[rh.KIND_NAME[env.unwrapped._vec.kind]] + (3,)
    env.close()


def test_pixel_observation_wrapper_and_render_collection(ref_gym):
    from gym.wrappers.pixel_observation import PixelObservationWrapper

    env = PixelObservationWrapper(ref_gym.make("hip/CartPole-v1", render_mode="rgb_array"), pixels_only=True)
    obs, _ = env.reset(seed=1)
    assert obs["pixels"].shape == (400, 600, 3) and obs["pixels"].dtype == np.uint8
    st = np.asarray(env.unwrapped.state, np.float64)
    assert np.array_equal(obs["pixels"], rh.render("CartPole", st, env.unwrapped._vec.handle.get_params()))
    obs, *_ = env.step(1)
    assert env.observation_space["pixels"].contains(obs["pixels"])
    env.close()
    rc = ref_gym.make("hip/Acrobot-v1", render_mode="rgb_array_list")
    assert type(rc).__name__ == "RenderCollection"
    rc.reset(seed=0)
    for _ in range(3):
        rc.step(1)
    frames = rc.render()
    assert len(frames) == 4 and all(f.shape == (500, 500, 3) for f in frames) and rc.render() == []
    rc.close()
    with pytest.raises(ValueError, match="rgb_array"):
        ref_gym.make("hip/CartPole-v1", render_mode="human")


def test_vector_env_render_through_gym_vector_surface(ref_gym):
    import gym_amd

    env = gym_amd.make("MountainCar-v0", 3, render_mode="rgb_array")
    env.reset(seed=2)
    assert env.get_attr("render_mode") == ("rgb_array",) * 3
    frames = env.call("render")
    st = env.call("state")
    assert len(frames) == 3 and all(np.array_equal(frames[i], rh.render("MountainCar", np.asarray(st[i], np.float64),
                                                                        env.handle.get_params())) for i in range(3))
    env.close()
