"""The classic-control step kernels at every comparison and guard edge.

Part 1 — tests/golden/<env>_p1_edges.npz (make_golden_edges.py: the reference stepped from states whose decisive post-step quantity is a sum of
two doubles or saturated by a clip, ON each bound, one ulp inside and one ulp outside it) through every kernel form that inlines Env<>::step,
the form asserted through last_launch().  Bars: terminated / truncated / elapsed equal on every row; the state components the fixture marks
exact (and, where the observation is float32(state), those observation columns) bit for bit; CartPole, MountainCar and
MountainCarContinuous rewards bit for bit; everything else at helpers.py's bars.  A fused launch shows no state between its steps: there
the first step is held through its outputs (masks, rewards, observations / final observations) and the state after the second step
against the oracle stepping the same tape.

Part 2 — the host logic that picks the guarded or the unguarded trigonometry (mxv_set_state / mxv_reset, last_launch()["safe"]): states and
reset bounds ON each range bound and one ulp beyond it, the persistence rules, NaN; outputs against the oracle stepping the same sampled
actions, NaN / Inf patterns and the sign of every infinity equal."""
import functools

import numpy as np
import pytest

from helpers import (EDGE_ENVS, ENV_IDS, GYM_IDS, LIMITS, MAX_OBS_ULPS, REWARD_ATOL, REWARD_ATOL_DEFAULT, REWARD_RTOL, STATE_ATOL, STATE_RTOL,
                     edge_groups, load_golden, same_bits, ulps32)

pytestmark = pytest.mark.gpu

PM_BROADCAST, PM_DEFAULT, PM_PER_ENV = 0, 1, 2                          # mxv_device.hpp
EXACT_REWARD = ("CartPole", "MountainCar", "MountainCarContinuous")
OBS_IS_STATE = ("CartPole", "MountainCar", "MountainCarContinuous")     # observation k = float32(state k)
ROLLOUT_ENVS_PER_LANE = {"CartPole": 2, "Pendulum": 1, "MountainCar": 2, "MountainCarContinuous": 2}   # of a shard that fills the chip
TILED = 1024 * 2 * 64 + 129                                             # just above one two-envs-per-lane wave per SIMD
HILO = ("CartPole", "MountainCar", "MountainCarContinuous")
PI_4 = 0.78539816339744830962


@functools.lru_cache(maxsize=None)
def groups(name):
    return edge_groups(name)


@functools.lru_cache(maxsize=None)
def whole(name):
    g = load_golden(name, "p1_edges")
    return {k: g[k] for k in g.files}


def default_rows(name):
    return groups(name)[0][1]


def tiled(g, n):
    idx = np.arange(n) % len(g["action"])
    return {k: v[idx] for k, v in g.items()}


def select(g, pred):
    rows = np.array([bool(pred(str(k))) for k in g["klass"]])
    return {k: v[rows] for k, v in g.items()}


def elapsed0(g):
    return np.where(g["fresh"] == 1, 0, 5).astype(np.int32)


def rows_of(bad, g):
    i = np.flatnonzero(bad)[:6]
    return f"rows {i.tolist()} ({[str(k) for k in g['klass'][i]]})"


def check(tag, name, g, term, trunc, reward, obs=None, state=None, elapsed=None, rows=None, want_trunc=False, start=None):
    """One step's results against the fixture rows g.  rows: the rows whose obs / state / elapsed are this step's (not an autoreset's)."""
    n = len(g["action"])
    rows = np.ones(n, bool) if rows is None else rows
    ex = g["exact"].astype(bool)
    bad = np.asarray(term).astype(bool) != g["terminated"].astype(bool)
    assert not bad.any(), f"{tag}: terminated differs in {rows_of(bad, g)}"
    bad = np.asarray(trunc).astype(bool) != np.broadcast_to(want_trunc, n)
    assert not bad.any(), f"{tag}: truncated differs in {rows_of(bad, g)}"
    if elapsed is not None:
        assert np.array_equal(elapsed[rows], ((elapsed0(g) if start is None else start) + 1)[rows]), f"{tag}: elapsed"
    if name in EXACT_REWARD:
        bad = ~same_bits(np.asarray(reward, np.float64), g["reward"])
        assert not bad.any(), f"{tag}: reward not bit-exact in {rows_of(bad, g)}"
    else:
        np.testing.assert_allclose(reward, g["reward"], rtol=REWARD_RTOL, atol=REWARD_ATOL.get(name, REWARD_ATOL_DEFAULT), err_msg=f"{tag}: reward")
    if obs is not None:
        o, ro = obs[rows], g["obs"][rows]
        u = ulps32(o, ro)
        assert u.size == 0 or u.max() <= MAX_OBS_ULPS, f"{tag}: obs off by {u.max()} float32 ulps"
        if name in OBS_IS_STATE:
            bad = (~same_bits(o, ro) & ex[rows]).any(axis=1)
            assert not bad.any(), f"{tag}: exact observation columns differ in {rows_of(bad, {'klass': g['klass'][rows]})}"
    if state is not None:
        s, rs, m = np.ascontiguousarray(state[rows]), np.ascontiguousarray(g["state1"][rows]), ex[rows]
        bad = (~same_bits(s, rs) & m).any(axis=1)
        assert not bad.any(), f"{tag}: exact state components differ in {rows_of(bad, {'klass': g['klass'][rows]})}: {s[bad][:2]} vs {rs[bad][:2]}"
        np.testing.assert_allclose(s[~m], rs[~m], rtol=STATE_RTOL, atol=STATE_ATOL, err_msg=f"{tag}: state")


# ---- part 1: single-step forms --------------------------------------------------------------------------------------------------------------
def step_handle(name, g, *, params=None, per_env=None, max_steps=0, elapsed=None):
    """One step_kernel launch (no autoreset) from the fixture's states -> results, last_launch()."""
    from gym_amd import _native

    h = _native.Handle(ENV_IDS[name], len(g["action"]), max_steps, flags=_native.FLAG_NO_AUTORESET)
    if params is not None:
        h.set_params(params)
    if per_env is not None:
        h.set_params_per_env(per_env)
    h.set_state(np.ascontiguousarray(g["state0"].T), elapsed0(g) if elapsed is None else elapsed)
    obs, rew, term, trunc, _ = h.step_host(g["action"])
    st, el = h.get_state()
    ll = h.last_launch()
    h.close()
    return dict(obs=obs, reward=rew, term=term, trunc=trunc, state=st.T, elapsed=el), ll


@pytest.mark.parametrize("mode", ["default", "broadcast", "per_env"])
@pytest.mark.parametrize("name", EDGE_ENVS)
def test_single_step_default_parameter_rows(name, mode):
    """The default-parameter rows through step_kernel's three parameter modes: the default vector handed over by set_params / as a table.
    (mxv_set_params recognises the exact default vector and keeps the compile-time-constant kernel, so the broadcast launch gets the
    default physics with a mark in slot 11, which none of these four kinds reads.)"""
    from oracle import oracle

    g = default_rows(name)
    P = oracle.default_params(ENV_IDS[name])
    marked = P.copy()
    assert marked[11] == 0.0
    marked[11] = 1.0
    kw = {"default": {}, "broadcast": dict(params=marked), "per_env": dict(per_env=np.repeat(P[:, None], len(g["action"]), axis=1))}[mode]
    got, ll = step_handle(name, g, **kw)
    assert ll["kernel"] == 0 and ll["param_mode"] == {"default": PM_DEFAULT, "broadcast": PM_BROADCAST, "per_env": PM_PER_ENV}[mode], ll
    check(f"{name} {mode}", name, g, got["term"], got["trunc"], got["reward"], got["obs"], got["state"], got["elapsed"])


@pytest.mark.parametrize("name", ["CartPole", "MountainCar", "MountainCarContinuous"])
def test_single_step_parameter_rows(name):
    """The rows with moved thresholds, a smaller max_speed, a goal_velocity on / one ulp above the saturated velocity ...: each parameter
    set broadcast, and the whole fixture — every set side by side — through one per-env table."""
    sets = groups(name)[1:]
    assert len(sets) >= 1
    for params, g in sets:
        got, ll = step_handle(name, g, params=params)
        assert ll["kernel"] == 0 and ll["param_mode"] == PM_BROADCAST, ll
        check(f"{name} broadcast {params[:10]}", name, g, got["term"], got["trunc"], got["reward"], got["obs"], got["state"], got["elapsed"])
    g = whole(name)
    got, ll = step_handle(name, g, per_env=np.ascontiguousarray(g["params"].T))
    assert ll["kernel"] == 0 and ll["param_mode"] == PM_PER_ENV, ll
    check(f"{name} per-env", name, g, got["term"], got["trunc"], got["reward"], got["obs"], got["state"], got["elapsed"])


def test_single_step_cartpole_one_env_per_lane():
    """From 2^19 envs a default-parameter CartPole step runs one env per lane: the fixture tiled to that size."""
    g = tiled(default_rows("CartPole"), 1 << 19)
    got, ll = step_handle("CartPole", g)
    assert ll["kernel"] == 0 and ll["envs_per_lane"] == 1 and ll["param_mode"] == PM_DEFAULT, ll
    check("CartPole 2^19", "CartPole", g, got["term"], got["trunc"], got["reward"], got["obs"], got["state"], got["elapsed"])


@pytest.mark.parametrize("name", HILO)
def test_adopted_observation_form(name):
    """obs_carries_state: the float32 observation + int32 residual pair must reproduce a state one ulp off a bound, and the step from it."""
    import torch

    from gym_amd.rollout import DeviceRollout

    g = default_rows(name)
    n = len(g["action"])
    r = DeviceRollout(GYM_IDS[name], n, obs_carries_state=True, autoreset=False)
    r.handle.set_state(np.ascontiguousarray(g["state0"].T), elapsed0(g))
    act = torch.from_numpy(g["action"]).cuda()
    torch.cuda.synchronize()
    obs, rew, term, trunc = r.step(act)
    r.synchronize()
    ll = r.handle.last_launch()
    assert ll["kernel"] == 0 and ll["out_mode"] == 3 and ll["param_mode"] == PM_DEFAULT, ll
    got = [x.cpu().numpy() for x in (term, trunc, rew, obs)]
    st, el = r.handle.get_state()              # joins the pairs back into fp64
    r.close()
    check(f"{name} adopted", name, g, *got, st.T, el)


# ---- part 1: fused tape-driven launches ---------------------------------------------------------------------------------------------------
def tape_launch(name, g, *, want_final, extra_state=None, max_steps=None, elapsed=None):
    """A two-step rollout_tape launch whose first step is the fixture's (the second takes action 0) -> step-0 outputs, last_launch(), and the
    comparison of both steps' masks and of the final state with the oracle stepping the same tape.  extra_state: one more env, appended."""
    import torch

    from gym_amd.rollout import DeviceRollout
    from oracle.oracle import OracleVecEnv

    n = len(g["action"])
    N = n + (extra_state is not None)
    limit = LIMITS[name] if max_steps is None else max_steps
    r = DeviceRollout(GYM_IDS[name], N, seed=11, action_seed=12, max_episode_steps=limit)
    ref = OracleVecEnv(ENV_IDS[name], N, limit, seed=11, action_seed=12)
    r.reset(seed=11), ref.reset(seed=11)
    st, el = np.zeros((g["state0"].shape[1], N)), np.zeros(N, np.int32)
    st[:, :n], el[:n] = g["state0"].T, elapsed0(g) if elapsed is None else elapsed
    if extra_state is not None:
        st[:, n] = extra_state
    r.handle.set_state(st, el)
    ref.state[:], ref.elapsed[:] = st, el
    tape = np.zeros((2, N), g["action"].dtype)
    tape[0, :n] = g["action"]
    dev = torch.from_numpy(tape).cuda()
    torch.cuda.synchronize()
    out = r.trajectory_buffers(2, want_final=want_final, layout="separate")
    r.rollout_tape(dev, out=out)
    r.synchronize()
    ll = r.handle.last_launch()
    res = {k: out[k].cpu().numpy() for k in ("obs", "reward", "terminated", "truncated") + (("final_obs",) if want_final else ())}
    st2, el2 = r.handle.get_state()
    r.close()
    alive = np.ones(N, bool)
    with np.errstate(all="ignore"):
        for k in range(2):
            _, _, te, tr, _, _ = ref.step(tape[k])
            assert np.array_equal(res["terminated"][k].astype(bool), te) and np.array_equal(res["truncated"][k].astype(bool), tr), (name, k)
            alive &= ~(te | tr)
    alive[n:] = False
    assert np.array_equal(el2[alive], ref.elapsed[alive])
    np.testing.assert_allclose(st2[:, alive], ref.state[:, alive], rtol=STATE_RTOL, atol=STATE_ATOL, err_msg=f"{name}: state after the second step")
    return {k: v[0][:n] for k, v in res.items()}, ll


def check_tape(tag, name, g, got, want_trunc=False):
    done = g["terminated"].astype(bool) | np.broadcast_to(want_trunc, len(g["action"]))
    check(tag, name, g, got["terminated"], got["truncated"], got["reward"], got["obs"], rows=~done, want_trunc=want_trunc)
    if "final_obs" in got and done.any():
        check(tag + " final_obs", name, g, got["terminated"], got["truncated"], got["reward"], got["final_obs"], rows=done, want_trunc=want_trunc)


@pytest.mark.parametrize("want_final", [False, True])
@pytest.mark.parametrize("name", EDGE_ENVS)
def test_fused_tape_first_step_unguarded_and_guarded(name, want_final):
    """The first step of a tape-driven fused launch: on the unguarded path (every fixture state is inside the range), and the same launch
    made guarded by one more env whose state is outside it.  With and without final observations: the generic and the trajectory body."""
    g = default_rows(name)
    got, ll = tape_launch(name, g, want_final=want_final)
    assert ll["kernel"] == 1 and ll["tape"] == 1 and ll["steps"] == 2 and ll["safe"] == 0 and ll["param_mode"] == PM_DEFAULT, ll
    assert ll["envs_per_lane"] == 1 and ll["out_mode"] == (0 if want_final else 1), ll
    check_tape(f"{name} tape unguarded", name, g, got)
    outside = {"CartPole": [0.0, 0.0, 1.0, 0.0], "Pendulum": [1e6, 0.0], "MountainCar": [1e6, 0.0], "MountainCarContinuous": [1e6, 0.0]}[name]
    got, ll = tape_launch(name, g, want_final=want_final, extra_state=outside)
    assert ll["kernel"] == 1 and ll["tape"] == 1 and ll["safe"] == 1 and ll["out_mode"] == (0 if want_final else 1), ll
    check_tape(f"{name} tape guarded", name, g, got)


@pytest.mark.parametrize("name", EDGE_ENVS)
def test_fused_tape_two_envs_per_lane(name):
    """The fixture tiled to just above one two-envs-per-lane wave per SIMD: the rollout instantiation of a shard that fills the chip."""
    g = tiled(default_rows(name), TILED)
    got, ll = tape_launch(name, g, want_final=True)
    assert ll["kernel"] == 1 and ll["tape"] == 1 and ll["safe"] == 0 and ll["envs_per_lane"] == ROLLOUT_ENVS_PER_LANE[name], ll
    check_tape(f"{name} tape tiled", name, g, got)


@pytest.mark.parametrize("max_steps", [500, 1])
def test_cartpole_time_limit_on_the_bound(max_steps):
    """A row on the bound and its one-ulp-outside sibling in the step that reaches the time limit: (terminated, truncated) = (False, True) and
    (True, True) — with elapsed = max_steps - 1, and with max_steps = 1; single step and fused."""
    g = select(default_rows("CartPole"), lambda k: ":on" in k or ":out" in k)
    on = np.array([":on" in str(k) for k in g["klass"]])
    assert on.sum() >= 4 * 64 and (~on).sum() >= 4 * 64
    assert not g["terminated"][on].any() and g["terminated"][~on].all()
    start = np.full(len(on), max_steps - 1, np.int32)
    got, ll = step_handle("CartPole", g, max_steps=max_steps, elapsed=start)
    assert ll["kernel"] == 0, ll
    assert not got["term"][on].any() and got["term"][~on].all() and got["trunc"].all()
    check("CartPole limit", "CartPole", g, got["term"], got["trunc"], got["reward"], got["obs"], got["state"], got["elapsed"], want_trunc=True, start=start)
    got, ll = tape_launch("CartPole", g, want_final=True, max_steps=max_steps, elapsed=start)
    assert ll["kernel"] == 1 and ll["safe"] == 0, ll
    assert not got["terminated"][on].any() and got["terminated"][~on].all() and got["truncated"].all()
    check_tape("CartPole limit fused", "CartPole", g, got, want_trunc=True)


# ---- part 2: the edge of the unguarded path ---------------------------------------------------------------------------------------------
N2 = 256


def up(x):
    """One ulp further from zero."""
    return float(np.nextafter(x, np.copysign(np.inf, x)))


def same_pattern(tag, got, ref, atol=None, rtol=None):
    """NaN for NaN, Inf for Inf with its sign; finite values within MAX_OBS_ULPS float32 ulps (or rtol / atol when given)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{tag}: NaN pattern"
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), f"{tag}: Inf pattern / signs"
    ok = np.isfinite(ref)
    if not ok.any():
        return
    if rtol is None:
        assert ulps32(got[ok], ref[ok]).max() <= MAX_OBS_ULPS, f"{tag}: {ulps32(got[ok], ref[ok]).max()} float32 ulps"
    else:
        np.testing.assert_allclose(got[ok], ref[ok], rtol=rtol, atol=atol, err_msg=tag)


class Pair:
    """A DeviceRollout and its oracle twin, reset from one seed; launch() = one fused K-step launch with sampled actions, every step's
    outputs compared with the twin stepping the same actions; -> last_launch()."""

    def __init__(self, name, n=N2, max_steps=None):
        from gym_amd.rollout import DeviceRollout
        from oracle.oracle import OracleVecEnv

        limit = LIMITS[name] if max_steps is None else max_steps
        self.name = name
        self.r = DeviceRollout(GYM_IDS[name], n, seed=31, action_seed=32, max_episode_steps=limit)
        self.ref = OracleVecEnv(ENV_IDS[name], n, limit, seed=31, action_seed=32)
        self.reset(seed=31)

    def reset(self, seed=None, mask=None, bounds=None):
        import torch

        m = None
        if mask is not None:
            m = torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).cuda()
            torch.cuda.synchronize()
        obs = self.r.reset(seed=seed, mask=m, bounds=bounds)
        self.r.synchronize()
        want = self.ref.reset(seed=seed, mask=mask, bounds=bounds)
        rows = slice(None) if mask is None else np.asarray(mask, bool)
        same_pattern(f"{self.name} reset", obs.cpu().numpy()[rows], want[rows])

    def inject(self, edits):
        """edits: [(component, env, value)] written over the current state, through mxv_set_state."""
        st, el = self.r.handle.get_state()
        st = st.copy()
        for k, i, v in edits:
            st[k, i] = v
        self.r.handle.set_state(st, el)
        self.ref.state[:], self.ref.elapsed[:] = st, el

    def launch(self, K=2):
        r, ref, name = self.r, self.ref, self.name
        out = r.trajectory_buffers(K, want_final=True, layout="separate")
        r.rollout_per_step(K, out=out)
        r.synchronize()
        ll = r.handle.last_launch()
        assert ll["kernel"] == 1 and ll["tape"] == 0 and ll["steps"] == K, ll
        ratol = REWARD_ATOL.get(name, REWARD_ATOL_DEFAULT)
        self.terminated = []
        with np.errstate(all="ignore"):
            for k in range(K):
                a = ref.sample_actions()
                assert np.array_equal(a, out["actions"][k].cpu().numpy()), (name, k)
                o, rw, te, tr, fin, fm = ref.step(a)
                tag = f"{name} step {k}"
                assert np.array_equal(out["terminated"][k].cpu().numpy().astype(bool), te), f"{tag}: terminated"
                assert np.array_equal(out["truncated"][k].cpu().numpy().astype(bool), tr), f"{tag}: truncated"
                same_pattern(tag + " obs", out["obs"][k].cpu().numpy(), o)
                same_pattern(tag + " final_obs", out["final_obs"][k].cpu().numpy()[fm], fin[fm])
                same_pattern(tag + " reward", out["reward"][k].cpu().numpy(), rw, rtol=REWARD_RTOL, atol=ratol)
                self.terminated.append(te)
        st, el = r.handle.get_state()            # the twin goes on from the device's state: last-bit differences must not pile up
        assert np.array_equal(el, ref.elapsed)
        same_pattern(f"{name} state", st, ref.state, rtol=1e-9, atol=1e-9)
        ref.state[:] = st
        return ll

    def close(self):
        self.r.close()


@pytest.mark.parametrize("beyond", [False, True])
def test_cartpole_theta_on_and_beyond_the_unguarded_bound(beyond):
    """|theta| = fl(pi/4) injected keeps the unguarded launch, one ulp beyond takes the guarded one; two steps against the oracle, and the
    launch after is unguarded.  Thetas in (theta_threshold, pi/4] whose theta_dot brings them back inside continue, unterminated."""
    q = up(PI_4) if beyond else PI_4
    p = Pair("CartPole")
    edits = [(2, 0, q), (2, 1, -q), (2, 2, q), (3, 2, -30.0), (2, 3, -q), (3, 3, 30.0)]
    back = range(8, 40)
    rng = np.random.default_rng(5)
    if not beyond:
        for i in back:
            th = float(rng.uniform(0.215, PI_4)) * (1 if i % 2 else -1)
            edits += [(2, i, th), (3, i, -(th - np.sign(th) * 0.15) / 0.02)]
    p.inject(edits)
    assert p.launch()["safe"] == (1 if beyond else 0)
    assert p.terminated[0][:2].all() and not p.terminated[0][2:4].any()
    if not beyond:
        assert not p.terminated[0][list(back)].any()
    assert p.launch()["safe"] == 0
    p.close()


@pytest.mark.parametrize("beyond", [False, True])
def test_cartpole_velocity_on_and_beyond_the_unguarded_bound(beyond):
    """x_dot / theta_dot at exactly +-1e150 keep the unguarded launch, one ulp beyond takes the guarded one; both against the oracle."""
    v = up(1e150) if beyond else 1e150
    p = Pair("CartPole")
    p.inject([(1, 0, v), (1, 1, -v), (3, 2, v), (3, 3, -v)])
    assert p.launch()["safe"] == (1 if beyond else 0)
    assert p.terminated[0][:4].all()
    assert p.launch()["safe"] == 0
    p.close()


@pytest.mark.parametrize("beyond", [False, True])
@pytest.mark.parametrize("name", ["Pendulum", "Acrobot", "MountainCar", "MountainCarContinuous"])
def test_other_kinds_on_and_beyond_the_unguarded_bound(name, beyond):
    """A component at exactly +-65536 keeps the unguarded launch, one ulp beyond takes the guarded one.  The next launch is unguarded again
    (the clamps / wraps restored the range) — except Pendulum's, whose angle is never wrapped."""
    v = up(65536.0) if beyond else 65536.0
    p = Pair(name)
    comps = (0, 1)          # (Acrobot: the two angles; its injected velocities are clamped like MountainCar's)
    p.inject([(k, 2 * k + j, s * v) for k in comps for j, s in enumerate((1, -1))])
    assert p.launch()["safe"] == (1 if beyond else 0)
    assert p.launch()["safe"] == (1 if beyond and name == "Pendulum" else 0)
    p.close()


def test_pendulum_out_of_range_angle_is_sticky_until_a_full_reset():
    p = Pair("Pendulum")
    p.inject([(0, 0, 1e6), (0, 1, -up(65536.0))])
    for _ in range(3):
        assert p.launch()["safe"] == 1
    mask = np.arange(N2) % 2 == 1                 # a partial reset (it even re-draws one of the two): still guarded
    p.reset(mask=mask)
    assert p.launch()["safe"] == 1
    p.reset()
    assert p.launch()["safe"] == 0
    p.close()


@pytest.mark.parametrize("max_steps,safe", [(0, 1), (1000000, 1), (999999, 0)])
def test_pendulum_time_limit_decides_the_unguarded_path(max_steps, safe):
    """Without a time limit below 1 000 000 steps the angle can turn without bound: such a handle never takes the unguarded launch."""
    p = Pair("Pendulum", max_steps=max_steps)
    for _ in range(2):
        assert p.launch()["safe"] == safe
    p.close()


@pytest.mark.parametrize("width,first", [(PI_4, 0), (up(PI_4), 1), (0.9, 1)])
def test_cartpole_reset_bounds_on_and_beyond_pi_4(width, first):
    """reset(options={"low", "high"}): bounds beyond pi/4 give one guarded launch (every such env ends in its first step), then unguarded."""
    p = Pair("CartPole")
    p.reset(seed=31, bounds=(-width, width))
    assert p.launch()["safe"] == first
    assert p.launch()["safe"] == 0
    p.close()


@pytest.mark.parametrize("x_init,safe", [(65536.0, 0), (up(65536.0), 1), (70000.0, 1)])
def test_pendulum_reset_bounds_on_and_beyond_the_range(x_init, safe):
    """Pendulum x_init beyond 65536: guarded launches until a full reset with the default bounds."""
    p = Pair("Pendulum")
    p.reset(seed=31, bounds=(x_init, 1.0))
    for _ in range(2):
        assert p.launch()["safe"] == safe
    p.reset(mask=np.arange(N2) % 2 == 0)
    assert p.launch()["safe"] == safe
    p.reset()
    assert p.launch()["safe"] == 0
    p.close()


@pytest.mark.parametrize("name", ["CartPole", "Pendulum", "Acrobot", "MountainCar", "MountainCarContinuous"])
def test_nan_in_any_component_takes_the_guarded_launch(name):
    """Non-finite counts as outside the range: a NaN in any one component gives the guarded launch, with the oracle's NaN pattern."""
    S = {"CartPole": 4, "Acrobot": 4}.get(name, 2)
    for k in range(S):
        p = Pair(name, n=64)
        p.inject([(k, 3 + k, np.nan)])
        assert p.launch()["safe"] == 1, (name, k)
        p.close()
