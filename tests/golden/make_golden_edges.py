#!/usr/bin/env python3
"""Golden single steps of the reference envs from EXACTLY-DETERMINED EDGE STATES: states found by search on the CPU whose decisive
post-step quantity (the value a threshold comparison or a clamp looks at) is a sum of two doubles or saturated by a clip, so that it
does not depend on the last bit of any sine or cosine — and which sit ON a bound, one ulp inside it or one ulp outside it.

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_edges.py

Like make_golden.py / make_golden_variants.py the script sets states (and attributes) on the reference's raw envs, steps once and records
what the reference returned.  <env>_p1_edges.npz holds per row: state0, action, fresh, params (the engine's parameter vector of the
row's attribute set), obs, reward, terminated, state1, klass (a label, see below) and exact (uint8 [n, S]: 1 where that component of
state1 is exactly determined — a device must reproduce it bit for bit).  The script asserts every row's intended post-step value against the
reference's own state1 and every class's minimum count before it writes.

Classes (klass):
  CartPole (Euler)   "<set>|<bound>:<on|in|out>[:split|:v0]"   set = default | moved (x_threshold 1.7, theta_threshold_radians 0.3);
                     bound = x+ x- th+ th-;  on / in / out = post-step x (theta) equals the bound / is one ulp inside / one ulp outside;
                     :split = fma(tau, v, x), rounded once (fractions), lands on the other side of the bound than fl(x + fl(tau * v));
                     :v0 = zero velocity, the state itself sits there.
  MountainCar        "goal:on|below|above", "max:on|clamped", "min:on|above|clamped" (default and max_speed = 0.05), "gv:eq|above"
                     (goal_velocity = the saturated velocity / one ulp above it); the velocity is saturated at +-max_speed by the clip.
  MountainCarCont.   the same with a "f64|" (fresh = 1) or "f32|" (fresh = 0: float32 state, bounds and goal as float32 values, one
                     float32 ulp) prefix, "gv:above32" (goal_velocity one FLOAT32 ulp above), "act:max|max+1|max+far|min|min-1|min-far"
                     (action on the bound, one float32 ulp beyond, far beyond: the `clipped` branches) and "term:reward" (100 - 0.1 a^2).
  Pendulum           "speed+|speed-" (thdot = +-max_speed pushed outward), "torque:<max|max+1|max+far|min|min-1|min-far|+0|-0>[:th0]"
                     (:th0 = th = +-0, where sin is exactly 0 and the step is exact), "kpi:<k>:<at|lo|hi|far>" (th = k * fl(pi), the doubles
                     next to it, and + 1.0), "mag" (|th| from 1e-300 to 65536).
"""
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402  (NumPy-2 shim + reference import + state helpers)
import make_golden_variants as mv  # noqa: E402  (param_vector)

gym = mg.gym
F32 = np.float32
INF = np.inf


def up(x, k=1):
    """k ulps up (k < 0: down), in x's own dtype."""
    x = np.asarray(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, x.dtype.type(INF if k > 0 else -INF))
    return x


class Rows:
    def __init__(self, name):
        self.name, self.S = name, mg.ENVS[name][1]
        self.r = []

    def add(self, klass, s0, action, fresh=0, attrs=None, exact=None, want=None, term=None):
        """want: {component: exact post-step value}; term: the intended terminated flag — both asserted against the reference."""
        self.r.append(dict(klass=klass, s0=np.asarray(s0, np.float64), action=action, fresh=int(fresh), attrs=dict(attrs or {}),
                           exact=np.ones(self.S, np.uint8) if exact is None else np.asarray(exact, np.uint8), want=want or {}, term=term))

    def run(self):
        """Step the reference from every row (one raw env per attribute set) and assemble the fixture."""
        name, rows = self.name, self.r
        gid, S, O, nd, _ = mg.ENVS[name]
        n = len(rows)
        assert 0 < n <= 4096, n
        rec = dict(state0=np.stack([r["s0"] for r in rows]), action=np.array([r["action"] for r in rows], np.int64 if nd else F32),
                   fresh=np.array([r["fresh"] for r in rows], np.uint8), params=np.zeros((n, 12)), obs=np.zeros((n, O), F32),
                   reward=np.zeros(n), terminated=np.zeros(n, np.uint8), state1=np.zeros((n, S)),
                   klass=np.array([r["klass"] for r in rows]), exact=np.stack([r["exact"] for r in rows]))
        envs = {}
        for i, r in enumerate(rows):
            key = tuple(sorted(r["attrs"].items()))
            if key not in envs:
                raw = gym.make(gid, disable_env_checker=True).unwrapped
                raw.reset(seed=0)
                for k, v in r["attrs"].items():
                    assert hasattr(raw, k), (name, k)
                    setattr(raw, k, v)
                envs[key] = (raw, mv.param_vector(name, raw, r["attrs"]))
            raw, pv = envs[key]
            mg.set_state(raw, name, r["s0"], bool(r["fresh"]))
            a = rec["action"][i] if nd else np.array([rec["action"][i]], dtype=F32)
            o, rew, te, tr, info = raw.step(a)
            assert tr is False
            s1 = mg.get_state(raw)
            for k, v in r["want"].items():
                assert s1[k] == v and np.signbit(s1[k]) == np.signbit(v), (name, r["klass"], k, s1[k].hex(), float(v).hex())
            if r["term"] is not None:
                assert bool(te) == r["term"], (name, r["klass"], r["s0"], te)
            rec["params"][i], rec["obs"][i], rec["reward"][i], rec["terminated"][i], rec["state1"][i] = pv, o, rew, te, s1
        return rec


def count(klass, pred):
    return int(sum(1 for k in klass if pred(k)))


# ---- CartPole ---------------------------------------------------------------------------------------------------------------------------
CP_SETS = {"default": {}, "moved": dict(x_threshold=1.7, theta_threshold_radians=0.3)}
CP_MIN = 64


def fma_once(tau, v, x):
    """fma(tau, v, x): the exact sum rounded once (int / int division of a Fraction is correctly rounded)."""
    return float(Fraction(float(x)) + Fraction(float(tau)) * Fraction(float(v)))


def cartpole_search(rng, target, tau, n):
    """(x0, v) with fl(x0 + fl(tau * v)) == target exactly, v of either sign in 0.8 .. 3."""
    v = rng.uniform(0.8, 3.0, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    p = tau * v
    x = target - p
    for d in (0, 1, -1):
        xx = up(x, d) if d else x
        hit = (xx + p == target) & ~(x + p == target)
        x = np.where(hit, xx, x)
    ok = x + p == target
    return x[ok], v[ok]


def cartpole_rows(seed=20261021):
    rng = np.random.default_rng(seed)
    R = Rows("CartPole")
    tau = 0.02
    for sname, attrs in CP_SETS.items():
        x_thr = attrs.get("x_threshold", 2.4)
        th_thr = attrs.get("theta_threshold_radians", 12 * 2 * np.pi / 360)
        for bname, comp, B in (("x+", 0, x_thr), ("x-", 0, -x_thr), ("th+", 2, th_thr), ("th-", 2, -th_thr)):
            B = np.float64(B)
            out_dir = 1 if B > 0 else -1
            targets = {"on": B, "in": up(B, -out_dir), "out": up(B, out_dir)}

            def outside(val):
                return bool(val > B) if B > 0 else bool(val < B)

            def state(x0, v):
                s = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.05, 0.05), rng.uniform(-0.5, 0.5)])
                s[comp], s[comp + 1] = x0, v
                return s

            nsplit = 0
            for pos, T in targets.items():
                xs, vs = cartpole_search(rng, T, tau, 400000)
                assert len(xs) > 10000, (sname, bname, pos, len(xs))
                # candidates for a split: the rounding error of x + p within one ulp(p) of half an ulp of the target (TwoSum)
                p = tau * vs
                s = xs + p
                bb = s - xs
                err = (xs - (s - bb)) + (p - bb)
                near = np.flatnonzero(np.abs(err) >= 0.5 * np.spacing(np.abs(T)) - 2 * np.spacing(np.abs(p)))
                split = [i for i in near if outside(fma_once(tau, vs[i], xs[i])) != outside(T)]
                plain = [i for i in range(400) if outside(fma_once(tau, vs[i], xs[i])) == outside(T)]
                # (a split needs x + p to be an exact tie that rounds to an EVEN target: for an odd bound only "out" rows can split)
                take_split = split[:80] if pos != "in" else []
                nsplit += len(take_split)
                for i in take_split:
                    R.add(f"{sname}|{bname}:{pos}:split", state(xs[i], vs[i]), int(rng.integers(0, 2)), attrs=attrs, exact=[1, 0, 1, 0],
                          want={comp: T}, term=outside(T))
                for i in plain[:64]:
                    R.add(f"{sname}|{bname}:{pos}", state(xs[i], vs[i]), int(rng.integers(0, 2)), attrs=attrs, exact=[1, 0, 1, 0],
                          want={comp: T}, term=outside(T))
                for z in (0.0, -0.0, 0.0, -0.0):
                    R.add(f"{sname}|{bname}:{pos}:v0", state(T, z), int(rng.integers(0, 2)), attrs=attrs, exact=[1, 0, 1, 0],
                          want={comp: T}, term=outside(T))
            assert nsplit >= CP_MIN
    return R


def cartpole_check(klass):
    for s in CP_SETS:
        for b in ("x+", "x-", "th+", "th-"):
            for pos in ("on", "in", "out"):
                moving = count(klass, lambda k: k in (f"{s}|{b}:{pos}", f"{s}|{b}:{pos}:split"))
                assert moving >= CP_MIN, (s, b, pos, moving)
                assert count(klass, lambda k: k == f"{s}|{b}:{pos}:v0") >= 4
            assert count(klass, lambda k: k.startswith(f"{s}|{b}:") and k.endswith(":split")) >= CP_MIN, (s, b)


# ---- MountainCar / MountainCarContinuous -------------------------------------------------------------------------------------------------
MC_MIN = 32


def solve_add(T, q):
    """Every p (of T's dtype) among the neighbours of T - q with fl(p + q) == T."""
    dt = np.asarray(T).dtype.type
    T, q = dt(T), dt(q)
    base = dt(T - q)
    return [dt(p) for p in (up(base, d) for d in range(-3, 4)) if dt(p + q) == T]


def car_rows(name, seed=20261022):
    """MountainCar (fresh ignored, float64) and MountainCarContinuous (f64: fresh = 1; f32: fresh = 0, float32 state and bounds)."""
    rng = np.random.default_rng(seed + len(name))
    cont = name == "MountainCarContinuous"
    R = Rows(name)
    goal_default = 0.45 if cont else 0.5
    n = MC_MIN

    def emit(prefix, dt, fresh):
        def c(v):
            return dt(v)                       # a bound as the path under test sees it

        def margin_ok(p, v0, a, max_speed, sign):
            """The pre-clip velocity is beyond the bound by more than 1e-6: the cosine's last bits cannot matter."""
            if cont:
                pre = v0 + (min(max(a, -1.0), 1.0) * 0.0015 - 0.0025 * np.cos(3 * p))
            else:
                pre = v0 + ((a - 1) * 0.001 + np.cos(3 * p) * (-0.0025))
            return pre > max_speed + 1e-6 if sign > 0 else pre < -max_speed - 1e-6

        def action():
            return float(F32(rng.uniform(-1, 1))) if cont else int(rng.integers(0, 3))

        def sat(klass, ps, sign, attrs, want_pos, want_vel, term, count_=n):
            """count_ rows from positions ps with the velocity saturated at sign * max_speed."""
            ms = attrs.get("max_speed", 0.07)
            for j in range(count_):
                p = ps[j % len(ps)]
                a = action()
                v0 = dt(sign * rng.uniform(ms + 0.005, ms + 0.02))
                if j % 2 == 0 and margin_ok(float(p), sign * ms, a, ms, sign):
                    v0 = c(sign * ms)          # from the bound itself, where the dynamics alone push beyond it
                assert margin_ok(float(p), float(v0), a, ms, sign), (klass, p, v0, a)
                want = {1: want_vel} if want_pos is None else {0: want_pos, 1: want_vel}   # (the continuous env stores float32)
                R.add(prefix + klass, [p, v0], a, fresh=fresh, attrs=attrs, want={k: float(F32(v)) if cont else float(v) for k, v in want.items()},
                      term=term)

        V = c(0.07)
        goal, pmax, pmin = c(goal_default), c(0.6), c(-1.2)
        # goal_position: exactly, one ulp below, one ulp above (velocity +max_speed >= goal_velocity = 0)
        sat("goal:on", solve_add(goal, V), +1, {}, goal, V, True)
        sat("goal:below", solve_add(up(goal, -1), V), +1, {}, up(goal, -1), V, False)
        sat("goal:above", solve_add(up(goal, 1), V), +1, {}, up(goal, 1), V, True)
        # max_position: reached exactly, and by the clamp
        # (0.6 - 0.07 is an exact tie that rounds away from the odd 0.6: no position reaches it at the default max_speed)
        for attrs in ({}, dict(max_speed=0.05), dict(max_speed=0.06)):
            ms = c(attrs.get("max_speed", 0.07))
            if solve_add(pmax, ms):
                sat("max:on", solve_add(pmax, ms), +1, attrs, pmax, ms, True)
                break
        sat("max:clamped", [dt(pmax - V + dt(x)) for x in rng.uniform(1e-4, 0.06, 8)], +1, {}, pmax, V, True)
        # min_position: exactly without the clamp (velocity zeroed), one ulp above (velocity kept), clamped onto it (zeroed)
        for attrs in ({}, dict(max_speed=0.05)):
            ms = c(attrs.get("max_speed", 0.07))
            sat("min:on", solve_add(pmin, -ms), -1, attrs, pmin, 0.0, False)
            sat("min:above", solve_add(up(pmin, 1), -ms), -1, attrs, up(pmin, 1), -ms, False)
            sat("min:clamped", [dt(pmin + ms - dt(x)) for x in rng.uniform(1e-4, 0.04, 8)], -1, attrs, pmin, 0.0, False)
        # goal_velocity: equal to the saturated velocity, one (float64) ulp above it, one float32 ulp above it
        at_goal = solve_add(goal, V) + solve_add(up(goal, 1), V)
        sat("gv:eq", at_goal, +1, dict(goal_velocity=0.07), None, V, True)
        gv64 = float(up(np.float64(0.07), 1))
        # (float32 path too: the clip leaves `velocity = self.max_speed`, a Python float, so this comparison is made in float64 even there)
        sat("gv:above", at_goal, +1, dict(goal_velocity=gv64), None, V, False)
        if cont:
            gv32 = float(up(F32(0.07), 1))
            sat("gv:above32", at_goal, +1, dict(goal_velocity=gv32), None, V, False)
            # a variable a clamp assigned is a Python float (:150, :155) or the int 0 (:159) and compares in float64 on the float32 path too:
            # 0 >= 1e-50 is false although float32(1e-50) is 0; a max_position one float64 ulp below the goal is below it although both
            # round to one float32
            sat("zero:gv", solve_add(pmin, -V), -1, dict(goal_position=-1.2, goal_velocity=1e-50), pmin, 0.0, False)
            below = float(up(np.float64(0.45), -1))
            sat("clamp:goal", [dt(c(below) - V + dt(x)) for x in rng.uniform(1e-4, 0.06, 8)], +1, dict(max_position=below), c(below), V, False)
            for j in range(n):                 # a terminating step's reward with actions inside and far outside the Box
                p = at_goal[j % len(at_goal)]
                a = float(F32(rng.uniform(-3, 3)))
                v0 = dt(rng.uniform(0.075, 0.09))
                assert margin_ok(float(p), float(v0), a, 0.07, +1)
                R.add(prefix + "term:reward", [p, v0], a, fresh=fresh, want={1: float(F32(V))}, term=True)

    if not cont:
        emit("", np.float64, 0)
    else:
        emit("f64|", np.float64, 1)
        emit("f32|", F32, 0)
        one, far = F32(1.0), F32(3.5)
        acts = {"act:max": one, "act:max+1": up(one, 1), "act:max+far": far, "act:min": -one, "act:min-1": -up(one, 1), "act:min-far": -far}
        for prefix, fresh, dt in (("f64|", 1, np.float64), ("f32|", 0, F32)):
            for klass, a in acts.items():
                for _ in range(n):
                    R.add(prefix + klass, [dt(rng.uniform(-1.0, 0.3)), dt(rng.uniform(-0.03, 0.03))], float(a), fresh=fresh, exact=[0, 0])
    return R


def car_check(name, klass):
    base = ["goal:on", "goal:below", "goal:above", "max:on", "max:clamped", "min:on", "min:above", "min:clamped", "gv:eq", "gv:above"]
    if name == "MountainCar":
        want = base
    else:
        extra = ["gv:above32", "zero:gv", "clamp:goal", "term:reward", "act:max", "act:max+1", "act:max+far", "act:min", "act:min-1", "act:min-far"]
        want = [p + k for p in ("f64|", "f32|") for k in base + extra]
    for k in want:
        assert count(klass, lambda x: x == k) >= MC_MIN, (name, k)


# ---- Pendulum ---------------------------------------------------------------------------------------------------------------------------
def pendulum_rows(seed=20261023):
    rng = np.random.default_rng(seed)
    R = Rows("Pendulum")
    ms, mt, dt, A, B = 8.0, 2.0, 0.05, 15.0, 3.0
    PI = float(np.pi)

    def outward(th, u, sign):
        """thdot = sign * max_speed: the push (A sin(th) + B clip(u)) dt is outward by more than 1e-6 whatever sin's last bits."""
        push = (A * np.sin(th) + B * min(max(u, -mt), mt)) * dt
        return sign * push > 1e-6

    def saturated(klass, th, u=None):
        """One row per direction in which `th` can be pushed outward at the speed bound; newthdot and newth are then exact."""
        k = 0
        for sign in (+1, -1):
            uu = float(F32(sign * rng.uniform(0.5, 2.5))) if u is None else sign * u
            if outward(th, uu, sign):
                R.add(klass, [th, sign * ms], uu, want={0: th + (sign * ms) * dt, 1: sign * ms})
                k += 1
        assert k > 0, (klass, th)

    for _ in range(96):
        saturated("speed", float(rng.uniform(-3.1, 3.1)))
    for r in R.r:
        r["klass"] = "speed+" if r["s0"][1] > 0 else "speed-"
    two = F32(2.0)
    torques = {"max": two, "max+1": up(two, 1), "max+far": F32(7.5), "min": -two, "min-1": -up(two, 1), "min-far": F32(-7.5),
               "+0": F32(0.0), "-0": F32(-0.0)}
    for tname, u in torques.items():
        for j in range(32):                    # th = +-0: sin is exactly +-0, so the whole step is exact arithmetic on thdot and u
            th = 0.0 if j % 2 == 0 else -0.0
            thdot = float(rng.uniform(-5, 5))
            uc = float(min(max(u, -two), two))
            nv = thdot + (A * float(np.sin(th)) + float(F32(F32(B) * F32(uc)))) * dt
            R.add(f"torque:{tname}:th0", [th, thdot], float(u), want={0: th + nv * dt, 1: nv})
        for j in range(32):
            R.add(f"torque:{tname}", [float(rng.uniform(-3.1, 3.1)), float(rng.uniform(-5, 5))], float(u), exact=[0, 0])
    for k in range(-9, 10):
        at = k * PI
        for tag, th in (("at", at), ("lo", float(up(np.float64(at), -1))), ("hi", float(up(np.float64(at), 1))), ("far", at + 1.0)):
            saturated(f"kpi:{k}:{tag}", th, u=2.0)
    mags = [65536.0, float(up(np.float64(65536.0), -1)), 65535.5, 40000.25, 4096.125, 1000.0, 100.0, 10.0, 1e-5, 1e-10, 1e-100, 1e-300,
            5e-324]
    for m in mags:
        for th in (m, -m):
            saturated("mag", th, u=2.0)
    for _ in range(64):                        # large angles off the speed bound: the medium-range sine itself (held to the state bars)
        R.add("mag:free", [float(rng.uniform(-65536, 65536)), float(rng.uniform(-5, 5))], float(F32(rng.uniform(-2, 2))), exact=[0, 0])
    return R


def pendulum_check(klass):
    assert count(klass, lambda k: k == "speed+") >= 32 and count(klass, lambda k: k == "speed-") >= 32
    for t in ("max", "max+1", "max+far", "min", "min-1", "min-far", "+0", "-0"):
        assert count(klass, lambda k: k == f"torque:{t}:th0") >= 32 and count(klass, lambda k: k == f"torque:{t}") >= 32, t
    for k in range(-9, 10):
        for tag in ("at", "lo", "hi", "far"):
            assert count(klass, lambda x: x == f"kpi:{k}:{tag}") >= 1, (k, tag)
    assert count(klass, lambda k: k == "mag") >= 26 and count(klass, lambda k: k == "mag:free") >= 64


BUILDERS = {"CartPole": cartpole_rows, "MountainCar": lambda: car_rows("MountainCar"),
            "MountainCarContinuous": lambda: car_rows("MountainCarContinuous"), "Pendulum": pendulum_rows}
CHECKS = {"CartPole": cartpole_check, "MountainCar": lambda k: car_check("MountainCar", k),
          "MountainCarContinuous": lambda k: car_check("MountainCarContinuous", k), "Pendulum": pendulum_check}


def class_counts(klass):
    names, counts = np.unique(klass, return_counts=True)
    return dict(zip((str(x) for x in names), (int(c) for c in counts)))


if __name__ == "__main__":
    for name in sys.argv[1:] or list(BUILDERS):
        rec = BUILDERS[name]().run()
        CHECKS[name](rec["klass"])
        np.savez_compressed(os.path.join(HERE, f"{name}_p1_edges.npz"), **rec)
        print(f"{name:24s} edges: {len(rec['klass'])} rows, {int(rec['terminated'].sum())} terminations")
        for k, c in class_counts(rec["klass"]).items():
            print(f"    {k:32s} {c}")
