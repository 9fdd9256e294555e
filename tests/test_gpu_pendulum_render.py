"""Pendulum-v1 frames and pixel observations on the device (include/mxv_render.h): the integer scenes against the
reference's recorded draw lists, frames and observations against the NumPy twin (tests/pendulum_render_host.py) bit for bit, and the
handle's last_u on every stepping and resetting surface."""
import os
import pickle

import numpy as np
import pytest

import pendulum_render_host as prh
import pixels_host as ph

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MT = 1   # max_torque's index in Pendulum's parameter vector


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "render_pendulum.npz"))


@pytest.fixture(scope="module")
def arrow():
    return prh.arrow()


def _handle(n, arrow, flags=0, limit=200):
    from gym_amd import _native, _render

    h = _native.Handle(_native.PENDULUM, n, limit, device=0, seed=11, action_seed=12, flags=flags)
    if arrow is not None:
        _render.attach_image(h, arrow)
    return h


def _put(h, states, last_u):
    """States and last_u set directly (set_state leaves last_u alone)."""
    from gym_amd import _render

    n = h.num_envs
    h.reset_host()
    h.set_state(np.ascontiguousarray(np.asarray(states, np.float64).T), np.zeros(n, np.int32))
    _render.set_torques(h, np.asarray(last_u, np.float32))


def _same_f32(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _expect_u(actions, max_torque, elapsed):
    u = np.array([prh.clip(a, m) for a, m in zip(np.asarray(actions, np.float32).reshape(-1), np.broadcast_to(max_torque, len(elapsed)))],
                 np.float32)
    u[np.asarray(elapsed) == 0] = np.nan
    return u


def test_scenes_equal_the_golden(golden, arrow):
    from gym_amd import _render

    g = golden
    m = len(g["states"])
    h = _handle(m, arrow)
    _put(h, g["states"], g["last_u"])
    recs = _render.scene_host(h)
    assert (recs[:, prh.RECORDS:] == 0).all()
    for i in range(m):
        assert np.array_equal(recs[i, :prh.RECORDS], prh.golden_records(g, i)), i
    h.close()


def test_frames_equal_the_twin_on_every_golden_case(golden, arrow):
    from gym_amd import _render

    g = golden
    m = len(g["states"])
    h = _handle(m, arrow)
    _put(h, g["states"], g["last_u"])
    frames = _render.render_host(h)
    assert frames.shape == (m, 500, 500, 3)
    for i in range(m):
        want = prh.render(g["states"][i], g["last_u"][i], arrow)
        assert np.array_equal(frames[i], want), (i, np.argwhere((frames[i] != want).any(-1))[:5])
    h.close()


@pytest.mark.parametrize("per_env", [False, True])
def test_clipped_torques_through_the_step_equal_the_reference(golden, arrow, per_env):
    """The golden cases driven through the reference's own step(): raw actions beyond +-max_torque, max_torque 2 and 0.7, common
    (set_params, one handle per value) or per env (set_params_per_env)."""
    from gym_amd import _render

    g = golden
    idx = np.flatnonzero(~np.isnan(g["pre_state"][:, 0]))
    groups = [idx] if per_env else [idx[g["max_torque"][idx] == v] for v in (2.0, 0.7)]
    for sel in groups:
        n = len(sel)
        h = _handle(n, arrow)
        h.reset_host()
        p = h.get_params()
        if per_env:
            pe = np.repeat(p[:, None], n, axis=1)
            pe[MT] = g["max_torque"][sel]
            h.set_params_per_env(np.ascontiguousarray(pe))
        else:
            p[MT] = g["max_torque"][sel[0]]
            h.set_params(p)
        h.set_state(np.ascontiguousarray(g["pre_state"][sel].T), np.zeros(n, np.int32))
        h.step_host(g["action"][sel].reshape(n, 1))
        assert _same_f32(_render.get_torques(h), g["last_u"][sel])
        np.testing.assert_allclose(h.get_state()[0].T, g["states"][sel], rtol=1e-12, atol=1e-12)
        h.set_state(np.ascontiguousarray(g["states"][sel].T), np.ones(n, np.int32))    # the reference's state bit for bit
        assert _same_f32(_render.get_torques(h), g["last_u"][sel])                       # set_state leaves last_u alone
        recs = _render.scene_host(h)
        frames = _render.render_host(h)
        for k, i in enumerate(sel):
            assert np.array_equal(recs[k, :prh.RECORDS], prh.golden_records(g, i)), i
            assert np.array_equal(frames[k], prh.render(g["states"][i], g["last_u"][i], arrow)), i
        h.close()


@pytest.mark.parametrize("hw", [(84, 84), (64, 64), (1, 1), (500, 500)])
@pytest.mark.parametrize("gray", [True, False])
def test_pixels_equal_the_twin_reduction(golden, arrow, hw, gray):
    from gym_amd import _render

    g = golden
    sel = np.r_[0:6, 41:53, 150:160, len(g["states"]) - 12:len(g["states"])]
    h = _handle(len(sel), arrow)
    _put(h, g["states"][sel], g["last_u"][sel])
    obs = _render.pixels_host(h, hw[0], hw[1], gray)
    for k, i in enumerate(sel):
        want = ph.reduce(prh.render(g["states"][i], g["last_u"][i], arrow), hw[0], hw[1], gray)
        assert np.array_equal(obs[k], want), (hw, gray, i)
    h.close()


def test_handles_without_an_image_stay_unsupported(arrow):
    import ctypes

    import torch

    from gym_amd import _native, _render

    lib = _native.lib
    h = _handle(4, None)
    buf = torch.zeros(4 * 500 * 500 * 3, dtype=torch.uint8, device="cuda")
    P = buf.data_ptr()
    assert lib.mxv_render(h._h, None, 4, P) == _native.ERR_UNSUPPORTED
    assert lib.mxv_pixels(h._h, None, 4, 84, 84, 1, P) == _native.ERR_UNSUPPORTED
    assert lib.mxv_pixels_strided(h._h, None, 84, 84, 1, 1, P, 7056, 0) == _native.ERR_UNSUPPORTED
    host = np.zeros(4 * 500 * 500 * 3, np.uint8)
    assert lib.mxv_render_host(h._h, None, 4, host.ctypes.data) == _native.ERR_UNSUPPORTED
    assert lib.mxv_render_scene_host(h._h, None, 4, host.ctypes.data) == _native.ERR_UNSUPPORTED
    assert lib.mxv_pixels_host(h._h, None, 4, 84, 84, 1, host.ctypes.data) == _native.ERR_UNSUPPORTED
    hh, ww = ctypes.c_int32(), ctypes.c_int32()
    assert lib.mxv_render_frame_dims(h._h, ctypes.byref(hh), ctypes.byref(ww)) == _native.ERR_UNSUPPORTED
    assert lib.mxv_render_get_torques_host(h._h, host.ctypes.data) == _native.ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="clockwise.png"):
        _render.render_host(h)
    c = _native.Handle(_native.CARTPOLE, 4, 500, device=0)
    assert lib.mxv_render_attach_image(c._h, arrow.ctypes.data, 312, 329) == _native.ERR_UNSUPPORTED
    assert lib.mxv_render_attach_image(h._h, arrow.ctypes.data, 0, 329) == _native.ERR_INVALID_ARG
    assert lib.mxv_render_attach_image(h._h, arrow.ctypes.data, 312, 1025) == _native.ERR_INVALID_ARG
    _render.attach_image(h, arrow)
    assert lib.mxv_render_frame_dims(h._h, ctypes.byref(hh), ctypes.byref(ww)) == _native.OK and (hh.value, ww.value) == (500, 500)
    assert np.isnan(_render.get_torques(h)).all()
    h.close()
    c.close()


def test_step_outputs_do_not_depend_on_the_image(arrow):
    import torch

    from gym_amd import DeviceRollout

    outs = []
    for img in (None, arrow):
        r = DeviceRollout("Pendulum-v1", 4096, seed=5, action_seed=6, max_episode_steps=7, arrow_image=img)
        r.reset()
        acc = []
        for k in range(9):
            if k % 3 == 0:
                a = torch.linspace(-3, 3, 4096, device=r.device, dtype=torch.float32)
                r.step(a)
            else:
                r.step_sampled()
            r.synchronize()
            acc += [t.cpu().numpy().copy() for t in (r.obs, r.reward, r.terminated, r.truncated)]
        out = r.rollout_per_step(5)
        r.synchronize()
        acc += [out[k].cpu().numpy().copy() for k in ("obs", "reward", "terminated", "truncated", "actions")]
        r.rollout(4)
        r.synchronize()
        acc += [r.obs.cpu().numpy().copy()]
        outs.append(acc)
        r.close()
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_last_u_on_the_vector_env_and_single_env_surfaces(arrow):
    import gym_amd
    from gym_amd import _render
    from gym_amd.single_env import HipEnv

    n = 8
    env = gym_amd.make("Pendulum-v1", n, max_episode_steps=3, render_mode="rgb_array", arrow_image=arrow)
    assert env.metadata["render_fps"] == 30
    h = env.handle
    env.reset(seed=3)
    assert np.isnan(_render.get_torques(h)).all()
    rng = np.random.default_rng(1)
    for k in range(7):
        a = rng.uniform(-3, 3, (n, 1)).astype(np.float32)
        a[0, 0] = np.float32(np.nan) if k == 1 else a[0, 0]
        env.step(a)
        el = h.get_state()[1]
        u = _render.get_torques(h)
        assert _same_f32(u, _expect_u(a, 2.0, el)), k
        frames = np.stack(env.call("render"))
        st = h.get_state()[0].T
        for i in (0, 3):
            assert np.array_equal(frames[i], prh.render(st[i], u[i], arrow))
        assert np.array_equal(env.render_frames([5])[0], prh.render(st[5], u[5], arrow))
    mask = np.zeros(n, np.uint8)
    mask[[1, 4]] = 1
    before = _render.get_torques(h)
    h.reset_host(mask)
    after = _render.get_torques(h)
    assert np.isnan(after[[1, 4]]).all() and _same_f32(np.delete(after, [1, 4]), np.delete(before, [1, 4]))
    blob = pickle.dumps(env)
    env2 = pickle.loads(blob)
    assert _same_f32(_render.get_torques(env2.handle), after)
    assert np.array_equal(env2.render_frames(), env.render_frames())
    a = rng.uniform(-2, 2, (n, 1)).astype(np.float32)
    env.step(a)
    env2.step(a)
    assert np.array_equal(env2.render_frames(), env.render_frames())
    env.close()
    env2.close()
    # the single env: no arrow after reset, the clipped torque after a step
    e = HipEnv("Pendulum-v1", render_mode="rgb_array", arrow_image=arrow)
    e.reset(seed=1)
    f0 = e.render()
    assert f0.shape == (500, 500, 3) and f0.dtype == np.uint8
    assert np.array_equal(f0, prh.render(e.state, np.nan, arrow))
    e.step(np.array([5.0], np.float32))
    assert np.array_equal(e.render(), prh.render(e.state, np.float32(2.0), arrow))
    e2 = pickle.loads(pickle.dumps(e))
    assert np.array_equal(e2.render(), e.render())
    e.close()
    e2.close()


def test_last_u_on_the_device_rollout_surfaces(arrow):
    import torch

    from gym_amd import DeviceRollout, _render

    n = 4096
    r = DeviceRollout("Pendulum-v1", n, seed=7, action_seed=8, max_episode_steps=5, arrow_image=arrow)
    h = r.handle
    r.reset()
    assert np.isnan(_render.get_torques(h)).all()
    per_env = h.get_params()
    pe = np.repeat(per_env[:, None], n, axis=1)
    pe[MT] = np.linspace(0.1, 3.0, n)
    mts = [2.0, 2.0, 2.0, pe[MT]]
    for phase, mt in enumerate(mts):
        if phase == 3:
            h.set_params_per_env(np.ascontiguousarray(pe))
        # caller's actions
        a = torch.linspace(-4, 4, n, device=r.device, dtype=torch.float32)
        r.step(a)
        r.synchronize()
        assert _same_f32(_render.get_torques(h), _expect_u(a.cpu().numpy(), mt, h.get_state()[1]))
        # sampled, recorded and not
        r.step_sampled(record_actions=True)
        r.synchronize()
        assert _same_f32(_render.get_torques(h), _expect_u(r.actions.cpu().numpy(), mt, h.get_state()[1]))
        snap = r.state_dict()
        r.step_sampled(record_actions=False)
        u_plain = _render.get_torques(h)
        r.load_state_dict(snap)
        r.step_sampled(record_actions=True)
        r.synchronize()
        assert _same_f32(u_plain, _render.get_torques(h))
        assert _same_f32(u_plain, _expect_u(r.actions.cpu().numpy(), mt, h.get_state()[1]))
        # K-step launches: per step (fused / eager / graph) with the actions recorded, and the fused one without
        for mode in ("fused", "eager", "graph"):
            out = r.rollout_per_step(7, mode=mode)
            r.synchronize()
            assert _same_f32(_render.get_torques(h), _expect_u(out["actions"][6].cpu().numpy(), mt, h.get_state()[1])), mode
        snap = r.state_dict()
        out = r.rollout_per_step(6, mode="fused")
        r.synchronize()
        want = _expect_u(out["actions"][5].cpu().numpy(), mt, h.get_state()[1])
        r.load_state_dict(snap)
        r.rollout(6, mode="fused", record_actions=False)
        assert _same_f32(_render.get_torques(h), want)
        r.load_state_dict(snap)
        r.rollout_per_step(6, mode="fused", record_actions=False)
        assert _same_f32(_render.get_torques(h), want)
        # an action tape
        tape = (torch.rand((4, n), device=r.device) * 8 - 4).contiguous()
        r.rollout_tape(tape)
        r.synchronize()
        assert _same_f32(_render.get_torques(h), _expect_u(tape[3].cpu().numpy(), mt, h.get_state()[1]))
        # masked reset
        before = _render.get_torques(h)
        mask = (torch.arange(n, device=r.device) % 3 == 0).to(torch.uint8)
        r.reset(mask=mask)
        r.synchronize()
        after = _render.get_torques(h)
        m = mask.cpu().numpy().astype(bool)
        assert np.isnan(after[m]).all() and _same_f32(after[~m], before[~m])
    # device frames of the tracked state: autoreset envs show no arrow
    idx = torch.tensor([0, 1, 2, 3, n - 1], dtype=torch.int32, device=r.device)
    frames = r.render(idx)
    r.synchronize()
    frames = frames.cpu().numpy()
    st, u = h.get_state()[0].T, _render.get_torques(h)
    for k, i in enumerate([0, 1, 2, 3, n - 1]):
        assert np.array_equal(frames[k], prh.render(st[i], u[i], arrow))
    pix = r.pixels(idx, height=84, width=84)
    r.synchronize()
    pix = pix.cpu().numpy()
    for k, i in enumerate([0, 1, 2, 3, n - 1]):
        assert np.array_equal(pix[k], ph.reduce(prh.render(st[i], u[i], arrow), 84, 84))
    r.close()


def test_checkpoint_round_trips_give_identical_next_frames(arrow):
    import torch

    from gym_amd import DeviceRollout, PixelRollout, _render

    r = DeviceRollout("Pendulum-v1", 64, seed=1, action_seed=2, arrow_image=arrow)
    r.reset()
    for _ in range(3):
        r.step_sampled()
    snap = pickle.loads(pickle.dumps(r.state_dict()))
    assert "last_u" in snap
    r.step_sampled()
    f1 = r.render()
    r.synchronize()
    f1 = f1.cpu().numpy()
    r2 = DeviceRollout("Pendulum-v1", 64, arrow_image=arrow)
    r2.load_state_dict(snap)
    r2.step_sampled()
    f2 = r2.render()
    r2.synchronize()
    assert np.array_equal(f2.cpu().numpy(), f1)
    r3 = DeviceRollout("Pendulum-v1", 64)
    with pytest.raises(ValueError, match="arrow"):
        r3.load_state_dict(snap)
    # a snapshot taken without an image leaves no stale torque on a handle with one
    r3.reset()
    r3.step_sampled()
    plain = r3.state_dict()
    assert "last_u" not in plain
    r2.load_state_dict(plain)
    assert np.isnan(_render.get_torques(r2.handle)).all()
    for x in (r, r2, r3):
        x.close()
    p = PixelRollout("Pendulum-v1", 64, arrow_image=arrow, max_episode_steps=4)
    p.reset()
    for _ in range(2):
        p.step()
    snap = pickle.loads(pickle.dumps(p.state_dict()))
    nxt = p.step()[0]
    p.synchronize()
    nxt = nxt.cpu().numpy()
    q = PixelRollout("Pendulum-v1", 64, arrow_image=arrow, max_episode_steps=4)
    q.load_state_dict(snap)
    got = q.step()[0]
    q.synchronize()
    assert np.array_equal(got.cpu().numpy(), nxt)
    assert _same_f32(_render.get_torques(q.engine.handle), _render.get_torques(p.engine.handle))
    p.close()
    q.close()


@pytest.mark.parametrize("sampled", [True, False])
def test_pixel_rollout_follows_the_autoreset_engine(arrow, sampled):
    import torch

    from gym_amd import DeviceRollout, PixelRollout, _render

    n, limit = 4096, 6
    p = PixelRollout("Pendulum-v1", n, arrow_image=arrow, seed=3, action_seed=4, max_episode_steps=limit)
    d = DeviceRollout("Pendulum-v1", n, arrow_image=arrow, seed=3, action_seed=4, max_episode_steps=limit, autoreset=True)
    # the same envs without any reset: through the first episode end (every env truncates at step `limit`) its states and last_u are the
    # terminal ones
    q = DeviceRollout("Pendulum-v1", n, arrow_image=arrow, seed=3, action_seed=4, max_episode_steps=limit, autoreset=False)
    p.reset()
    d.reset()
    q.reset()
    check = torch.tensor([0, 17, n - 1], dtype=torch.int32, device=d.device)
    for k in range(14):
        if sampled:
            px = p.step()[0]
            d.step_sampled()
            if k < limit:
                q.step_sampled()
        else:
            a = (torch.rand(n, device=d.device) * 6 - 3).contiguous()
            px = p.step(a)[0]
            d.step(a)
            if k < limit:
                q.step(a)
        p.synchronize()
        d.synchronize()
        q.synchronize()
        assert torch.equal(p.obs, d.obs)
        assert _same_f32(_render.get_torques(p.engine.handle), _render.get_torques(d.handle)), k
        newest = px[:, -1]
        dpx = d.pixels(height=84, width=84)
        d.synchronize()
        assert torch.equal(newest, dpx)
        done = (d.truncated | d.terminated).bool()
        if done.any():
            # the terminal frame shows the terminal step's arrow, the reset frames none
            i = int(torch.nonzero(done)[0])
            assert np.isnan(_render.get_torques(d.handle)[i]) and np.isnan(_render.get_torques(p.engine.handle)[i])
            assert not np.array_equal(p.final_pixels[i, -1].cpu().numpy(), newest[i].cpu().numpy())
        if k == limit - 1:
            assert done.all()
            qs, qu = q.handle.get_state()[0].T, _render.get_torques(q.handle)
            assert not np.isnan(qu).any()
            fin = p.final_pixels[:, -1].cpu().numpy()
            for i in (0, 17, 1000, n - 1):
                assert np.array_equal(fin[i], ph.reduce(prh.render(qs[i], qu[i], arrow), 84, 84)), i
        st, u = d.handle.get_state()[0].T, _render.get_torques(d.handle)
        frames = d.render(check)
        d.synchronize()
        frames = frames.cpu().numpy()
        for kk, i in enumerate(check.tolist()):
            assert np.array_equal(frames[kk], prh.render(st[i], u[i], arrow))
    p.close()
    d.close()
    q.close()


def test_graph_replay_of_step_and_pixels_equals_eager(arrow):
    import torch

    from gym_amd import DeviceRollout, _render

    n = 1024
    outs = []
    for graphed in (False, True):
        r = DeviceRollout("Pendulum-v1", n, seed=9, action_seed=10, max_episode_steps=4, arrow_image=arrow)
        r.reset()
        r.enable_graph_capture()
        pix = torch.zeros((n, 64, 64), dtype=torch.uint8, device=r.device)
        acc = []
        if graphed:
            with torch.cuda.stream(r.stream):
                r.step_sampled()
                r.pixels(height=64, width=64, out=pix)
                r.stream.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=r.stream):
                    r.step_sampled()
                    r.pixels(height=64, width=64, out=pix)
            for _ in range(6):
                g.replay()
                r.synchronize()
                acc += [pix.cpu().numpy().copy(), _render.get_torques(r.handle)]
        else:
            with torch.cuda.stream(r.stream):
                r.step_sampled()
                r.pixels(height=64, width=64, out=pix)
            for _ in range(6):
                with torch.cuda.stream(r.stream):
                    r.step_sampled()
                    r.pixels(height=64, width=64, out=pix)
                r.synchronize()
                acc += [pix.cpu().numpy().copy(), _render.get_torques(r.handle)]
        outs.append(acc)
        r.close()
    for a, b in zip(*outs):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
