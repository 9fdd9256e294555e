#!/usr/bin/env python3
"""<env>_p1_signed_zero.npz — the reference's single step from states and actions built out of +-0 components: every sign pattern of
the state, every discrete action resp. the Box actions +0.0 and -0.0 (MountainCarContinuous also right after reset, with its float64
state).  The sign of a zero survives the reference's arithmetic in places (Pendulum at theta = -0, theta_dot = -0 and u = -0 returns
obs [1, -0, -0] and state (-0, -0)); an engine whose sin(-0) or division turns -0 into +0 differs there, which float32-ulp comparisons
that ignore the sign of zero cannot see.  Same layout and replay as make_golden_nonfinite.py (helpers.run_p1_signed_zero).

Run in the build container only (needs /root/reference):   python tests/golden/make_golden_signed_zero.py"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

gym = mg.gym


def cases(name):
    gid, S, O, nd, _ = mg.ENVS[name]
    states = np.array(list(itertools.product([0.0, -0.0], repeat=S)), dtype=np.float64)
    acts = list(range(nd)) if nd else [0.0, -0.0]
    fresh_opts = [0, 1] if name == "MountainCarContinuous" else [0]
    rows = [(s, a, f) for s in states for a in acts for f in fresh_opts]
    s0 = np.stack([r[0] for r in rows])
    act = np.array([r[1] for r in rows], dtype=np.int64 if nd else np.float32)
    fresh = np.array([r[2] for r in rows], np.uint8)
    return s0, act, fresh


def make(name):
    gid, S, O, nd, _ = mg.ENVS[name]
    raw = gym.make(gid, disable_env_checker=True).unwrapped
    raw.reset(seed=0)
    s0, act, fresh = cases(name)
    n = len(act)
    obs = np.zeros((n, O), np.float32)
    rew = np.zeros(n)
    term = np.zeros(n, np.uint8)
    s1 = np.zeros((n, S))
    for i in range(n):
        mg.set_state(raw, name, s0[i], bool(fresh[i]))
        a = int(act[i]) if nd else np.array([act[i]], dtype=np.float32)
        o, r, te, tr, info = raw.step(a)
        obs[i], rew[i], term[i], s1[i] = o, r, te, mg.get_state(raw)
    np.savez_compressed(os.path.join(HERE, f"{name}_p1_signed_zero.npz"), state0=s0, action=act, fresh=fresh, obs=obs, reward=rew,
                        terminated=term, state1=s1)
    nz = int(((obs == 0) & np.signbit(obs)).sum() + ((s1 == 0) & np.signbit(s1)).sum())
    print(f"{name:24s} P1[signed_zero]: {n} steps, {nz} negative zeros among the outputs")


if __name__ == "__main__":
    for name in mg.ENVS:
        make(name)
