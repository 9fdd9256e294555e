"""The oracle against the reference on vectors no other fixture uses (CPU).  tests/test_oracle_golden.py pins the oracle to the committed
fixtures of tests/golden/make_golden.py; this file holds it to the same bar — BIT-EXACT observations, rewards, masks, fp64 post-step
states, final observations — on what the same generators made, from the reference itself, at a seed of this file's own, 777000123
(tests/golden/make_golden_live.py: live_<env>_*.npz):

  * 12 000 single raw-env steps per env kind from states sampled broadly and next to every threshold, in- and out-of-range actions;
  * a 32-env SyncVectorEnv trajectory per env kind (TimeLimit + autoreset + final_observation, RecordEpisodeStatistics riding along),
    once with the registered TimeLimit and once with a short one.

Exploring other seeds where the reference tree is importable: MXV_LIVE_SEED=<int> runs make_golden.py's generators live with that seed
instead of reading the fixtures, MXV_LIVE_SEED=clock with a new one per run; a failure prints the seed, which reproduces it."""
import importlib.util
import os
import time

import numpy as np
import pytest

from helpers import ENV_NAMES, OracleEngine, run_p1, run_p2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_s = os.environ.get("MXV_LIVE_SEED", "")
LIVE_SEED = (int(time.time()) % 1_000_000_007 if _s == "clock" else int(_s)) if _s else None


@pytest.fixture(scope="module")
def vectors():
    """name, kind -> the vectors: the committed fixtures, or (MXV_LIVE_SEED set) make_golden.py's generators run on the spot."""
    if LIVE_SEED is None:
        def get(name, kind):
            with np.load(os.path.join(GOLDEN, f"live_{name}_{kind}.npz")) as z:
                return {k: z[k] for k in z.files}
        return get
    spec = importlib.util.spec_from_file_location("make_golden_live_seed", os.path.join(GOLDEN, "make_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)      # imports the reference's gym (read-only): only on request

    def make(name, kind):
        if kind == "p1":
            return gen.make_p1(name, n=12000, seed=LIVE_SEED, save=False)
        kw = {"max_episode_steps": gen.ENVS[name][4]} if kind == "p2_short" else {}
        return gen.make_p2(name, kind[3:], T=240, num_envs=32, seed=LIVE_SEED + 17, save=False, **kw)
    return make


def _seed_note():
    return f" (MXV_LIVE_SEED={LIVE_SEED} reproduces this)" if LIVE_SEED is not None else ""


@pytest.mark.parametrize("name", ENV_NAMES)
def test_fresh_single_steps_bit_exact(vectors, name):
    g = vectors(name, "p1")
    assert len(g["action"]) == 12000
    try:
        run_p1(OracleEngine, name, strict=True, golden=g)
    except AssertionError as e:
        raise AssertionError(f"{e}{_seed_note()}") from e
    if name in ("CartPole", "Acrobot", "MountainCar", "MountainCarContinuous"):
        assert int(g["terminated"].sum()) > 0          # the sampler reaches the thresholds


@pytest.mark.parametrize("name", ENV_NAMES)
def test_fresh_vector_trajectories_bit_exact(vectors, name):
    limits = {}
    for tag in ("default", "short"):
        g = vectors(name, f"p2_{tag}")
        assert g["obs"].shape[:2] == (240, 32)
        limits[tag] = int(g["max_episode_steps"])
        try:
            ndone = run_p2(OracleEngine, name, tag, strict=True, golden=g)
        except AssertionError as e:
            raise AssertionError(f"{e}{_seed_note()}") from e
        if tag == "short":
            assert ndone > 32                           # truncations + autoresets were exercised
    assert limits["short"] < limits["default"]          # the short run really ran under its own, shorter TimeLimit
