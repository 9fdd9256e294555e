"""Non-finite, huge and limit-straddling states through scene_kernel, render_kernel and pixels_kernel (-m gpu).

The engine propagates NaN and Inf states like the reference, so they are legal inputs to render() and pixels().  The NumPy twins
(tests/render_host.py, tests/pendulum_render_host.py) define what their frames are: a primitive with a non-finite coordinate, or one
beyond +-2^20 px, is skipped.  The golden scenes hold finite states only, and the device's float -> int conversions saturate where
NumPy's do not, so the two agree only if every guard fires before a conversion.  Here each state slot in turn, and all at once, takes
nan, +-inf, +-1e300, +-1e7 and, where the slot is a position with a world-to-pixel scale, the adjacent doubles on either side of the
+-2^20 px limit (and 64 px inside / outside it, where every vertex of the primitive is on one side).  Acrobot's and Pendulum's state
slots are angles and velocities: no value of them moves a coordinate out of the frame's neighbourhood, so they have no such pair;
Pendulum's arrow has one in last_u (float32), and takes NaN and Inf there too.  At that pair the arrow is 2^20 px wide: the NumPy
twin cannot scale the image that far, so the frame of that env is held to its records and its observations, not to the raster twin.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pendulum_render_host as prh  # noqa: E402
import pixels_host as ph  # noqa: E402
import render_host as rh  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")
IDS = {"CartPole": "CartPole-v1", "Acrobot": "Acrobot-v1", "MountainCar": "MountainCar-v0",
       "MountainCarContinuous": "MountainCarContinuous-v0"}
KINDS = list(IDS) + ["Pendulum"]
SLOTS = {"CartPole": 4, "Acrobot": 4, "MountainCar": 2, "MountainCarContinuous": 2, "Pendulum": 2}
VALUES = [np.nan, np.inf, -np.inf, 1e300, -1e300, 1e7, -1e7]
NAN_PARAM = {"CartPole": 9, "Acrobot": 1, "MountainCar": 0, "MountainCarContinuous": 2}   # x_threshold, LINK_LENGTH_1, min_position
BLIT_TWIN_MAX = 4096   # px: the twin scales the whole arrow image before it clips (2^20 x 2^20 x 4 at the limit); wider arrows are held
#                        to the scene and to the agreement of frames and observations only
BASE = {"CartPole": [0.3, 0.1, -0.07, 0.2], "Acrobot": [0.4, -0.9, 0.1, 0.2], "MountainCar": [-0.6, 0.01],
        "MountainCarContinuous": [-0.3, -0.02], "Pendulum": [0.8, 0.5]}


def _straddle(term, target, lo, hi):
    """Adjacent doubles (a, b), a on lo's side, with term(a) <= target < term(b) (term increasing on [lo, hi]) or, for a decreasing
    side, term(a) >= target > term(b): bisection on the doubles themselves."""
    inside = (lambda v: term(v) <= target) if target > 0 else (lambda v: term(v) >= target)
    assert inside(lo) and not inside(hi)
    while True:
        mid = lo + (hi - lo) / 2
        if mid == lo or mid == hi:
            return lo, hi
        lo, hi = (mid, hi) if inside(mid) else (lo, mid)


def limit_positions(name, params):
    """Positions whose world-to-pixel term (the translation every vertex of the cart / car shares: render_host.scene) lies 64 px inside,
    just inside, just outside and 64 px outside +-2^20."""
    P = [float(v) for v in params]
    if name == "CartPole":
        scale = rh._div(600, P[9] * 2)
        term = lambda x: x * scale + 600 / 2.0                       # noqa: E731  cartx
    else:
        lo = P[0] if name == "MountainCar" else P[2]
        hi = P[1] if name == "MountainCar" else P[3]
        scale = rh._div(600, hi - lo)
        term = lambda x: (x - lo) * scale                            # noqa: E731
    out = []
    for sign in (1.0, -1.0):
        reach = sign * 4 * rh.LIMIT_PX / scale
        for target in (sign * (rh.LIMIT_PX - 64), sign * rh.LIMIT_PX, sign * (rh.LIMIT_PX + 64)):
            a, b = _straddle(term, target, 0.0, reach)
            out += [a, b] if abs(target) == rh.LIMIT_PX else [a]
    return out


def limit_torques():
    """float32 last_u whose arrow size float32(scale) * |u| / 2 is the last <= 2^20 and the first beyond it, both signs."""
    a = np.float32(2 * rh.LIMIT_PX / prh.SCALE)
    while prh.blit_size(a) >= 0:
        a = np.nextafter(a, np.float32(np.inf))
    while prh.blit_size(a) < 0:
        a = np.nextafter(a, np.float32(0))
    b = np.nextafter(a, np.float32(np.inf))
    assert prh.blit_size(a) >= (1 << 20) - 1 and prh.blit_size(b) < 0
    return [a, b, -a, -b]


def edge_states(name, params):
    """(states [n, S], near [n], last_u [n] or None): the base state with one slot replaced, then every slot replaced, per value."""
    S = SLOTS[name]
    base = np.array(BASE[name], np.float64)
    states, near = [base.copy()], [False]
    for v in VALUES:
        for slot in range(S):
            s = base.copy()
            s[slot] = v
            states.append(s)
        states.append(np.full(S, v))
        near += [False] * (S + 1)
    if name in ("CartPole", "MountainCar", "MountainCarContinuous"):
        for v in limit_positions(name, params):
            s = base.copy()
            s[0] = v
            states += [s, np.full(S, v)]
            near += [True, True]
    states = np.array(states)
    if name != "Pendulum":
        return states, np.array(near), None
    u = [np.float32(1.5)] * len(states)                              # an ordinary arrow under every edge state ...
    extra = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)] + limit_torques()
    states = np.concatenate([states, np.tile(base, (len(extra), 1)), np.full((2, S), np.nan)])
    u += extra + [np.float32(np.inf), np.float32(np.nan)]           # ... every edge torque under an ordinary state, and both at once
    return states, np.zeros(len(states), bool), np.array(u, np.float32)


def _make(name, n):
    from gym_amd import _native, _render
    from gym_amd.registration import spec

    if name == "Pendulum":
        h = _native.Handle(_native.PENDULUM, n, 200, device=0, seed=11, action_seed=12)
        _render.attach_image(h, prh.arrow())
    else:
        h = _native.Handle(spec(IDS[name]).kind, n, 500, device=0, seed=1, action_seed=2)
    h.reset_host()
    return h


def _put(h, states, last_u=None):
    from gym_amd import _render

    h.set_state(np.ascontiguousarray(np.asarray(states, np.float64).T), np.zeros(len(states), np.int32))
    if last_u is not None:
        _render.set_torques(h, np.asarray(last_u, np.float32))


class Twin:
    """The kind's NumPy scene and raster rule; frames of equal record lists are drawn once."""

    def __init__(self, name):
        self.name = name
        self.H, self.W = (prh.H, prh.W) if name == "Pendulum" else rh.DIMS[name]
        self.nrec = prh.RECORDS if name == "Pendulum" else rh.RECORDS[name]
        self.arrow = prh.arrow() if name == "Pendulum" else None
        self._drawn = {}

    def scene(self, state, params, u=None):
        with np.errstate(all="ignore"):
            return prh.scene(state, u) if self.name == "Pendulum" else rh.scene(self.name, state, params)

    def rasterize(self, recs):
        key = np.ascontiguousarray(recs, np.int64).tobytes()
        if key not in self._drawn:
            self._drawn[key] = prh.rasterize(recs, self.arrow) if self.name == "Pendulum" else rh.rasterize(recs, self.H, self.W)
        return self._drawn[key]


def _check(h, twin, states, params_of, near, last_u=None):
    """Everything the issue of non-finite states asks of one handle: records, frames of the device's own records, observations of those
    frames, no latched error."""
    from gym_amd import _render

    n = len(states)
    recs = _render.scene_host(h)
    frames = _render.render_host(h)
    gray = _render.pixels_host(h, 84, 84, True)
    rgb = _render.pixels_host(h, 7, 13, False)
    h.sync()
    assert (recs[:, twin.nrec:] == 0).all()
    for i in range(n):
        what = (twin.name, i, states[i].tolist(), None if last_u is None else float(last_u[i]))
        want = twin.scene(states[i], params_of(i), None if last_u is None else last_u[i])
        got = recs[i, :twin.nrec].astype(np.int64)
        if near[i]:
            assert np.array_equal(got[:, :4], want[:, :4]) and np.all(np.abs(got[:, 4:] - want[:, 4:]) <= 8), what
        else:
            assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4].tolist())
        if not (twin.name == "Pendulum" and got[6, 6] > BLIT_TWIN_MAX):
            frame = twin.rasterize(got)                              # the raster rule on the device's own records
            assert np.array_equal(frames[i], frame), (what, np.argwhere((frames[i] != frame).any(-1))[:4].tolist())
        assert np.array_equal(gray[i], ph.reduce(frames[i], 84, 84, True)), what
        assert np.array_equal(rgb[i], ph.reduce(frames[i], 7, 13, False)), what


def _ordinary(name):
    """A few golden states (default attributes) and their last_u: what the handle must still draw correctly afterwards."""
    if name == "Pendulum":
        g = np.load(os.path.join(GOLDEN, "render_pendulum.npz"))
        pick = np.flatnonzero(~g["raised"])[[0, 50, -1]]
        return g["states"][pick], g["last_u"][pick]
    g = np.load(os.path.join(GOLDEN, "render_scenes.npz"))
    pr = g[f"{name}_params"]
    same = np.flatnonzero((pr == pr[0]).all(1))
    return g[f"{name}_states"][same[[0, len(same) // 2, -1]]], None


@pytest.mark.parametrize("name", KINDS)
def test_edge_states_give_the_twins_frames(name):
    """nan, +-inf, +-1e300, +-1e7 and the +-2^20 px pairs in each state slot and in all of them (Pendulum: in last_u too): the device's
    records equal the twin's scene (the pairs at the limit within the golden scenes' `near` tolerance of 1 px, same primitives drawn),
    its frames equal the raster rule on those records, its observations the reduction of those frames; no error is latched; an
    ordinary state on the same handle is then drawn correctly."""
    from gym_amd import _render

    params = None
    if name != "Pendulum":
        g = np.load(os.path.join(GOLDEN, "render_scenes.npz"))
        params = g[f"{name}_params"][0]
    states, near, last_u = edge_states(name, params)
    twin = Twin(name)
    n = len(states)
    h = _make(name, n)
    if params is not None:
        h.set_params(np.asarray(params, np.float64))
    _put(h, states, last_u)
    _check(h, twin, states, lambda i: params, near, last_u)
    if name in ("CartPole", "MountainCar", "MountainCarContinuous"):
        recs = _render.scene_host(h)                                 # the pairs do straddle: the car is drawn on one side only
        drawn = (recs[:, :twin.nrec, 0] != 0).sum(1)
        assert len({int(d) for d in drawn[near]}) > 1
    ordinary, u = _ordinary(name)
    fill = np.tile(ordinary, (n // len(ordinary) + 1, 1))[:n]
    fill_u = None if u is None else np.tile(u, n // len(u) + 1)[:n]
    _put(h, fill, fill_u)
    frames = _render.render_host(h, [0, 1, 2])
    for i in range(3):
        want = prh.render(fill[i], fill_u[i], twin.arrow) if name == "Pendulum" else rh.render(name, fill[i], params)
        assert np.array_equal(frames[i], want), (name, i)
    h.sync()
    h.close()


@pytest.mark.parametrize("name", list(IDS))
def test_edge_parameters_give_the_twins_frames(name):
    """A NaN render attribute per env, and CartPole's x_threshold = 0 (600 / 0: the frame keeps the track line only), next to an env with
    the default attributes."""
    g = np.load(os.path.join(GOLDEN, "render_scenes.npz"))
    p = g[f"{name}_params"][0].astype(np.float64)
    per_env = [p.copy(), p.copy()]
    per_env[1][NAN_PARAM[name]] = np.nan
    if name == "CartPole":
        per_env += [p.copy(), p.copy()]
        per_env[2][9] = 0.0
        per_env[3][4] = np.inf                                       # the pole's length
    per_env = np.array(per_env)
    n = len(per_env)
    states = np.tile(np.array(BASE[name], np.float64), (n, 1))
    twin = Twin(name)
    h = _make(name, n)
    h.set_params_per_env(np.ascontiguousarray(per_env.T))
    _put(h, states)
    _check(h, twin, states, lambda i: per_env[i], np.zeros(n, bool))
    if name == "CartPole":
        from gym_amd import _render

        f = _render.render_host(h, [2])[0]
        assert (f[299] == 0).all() and (np.delete(f, 299, axis=0) == 255).all()
    h.close()
