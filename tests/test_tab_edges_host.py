"""The CPU twin of the tabular engine (oracle/tabular.c through OracleTabEnv) held to the exact model of tests/tab_edges.py, on every case
tests/test_gpu_toytext_edges.py runs: the GPU file compares the device with the twin, so the twin has to be right there first — at every
pinned threshold, at every counter carry, with keys that wrap inside the batch, and under a TimeLimit of 1.  No device needed."""
import numpy as np
import pytest

import tab_edges as te


def _same(ref, got, what):
    for k in ("actions", "obs", "reward", "prob", "terminated", "truncated", "final_mask"):
        assert np.array_equal(ref[k], got[k]), (what, k)
    m = ref["final_mask"]
    assert np.array_equal(ref["final_obs"][m], got["final_obs"][m]) and np.array_equal(ref["final_prob"][m], got["final_prob"][m]), what


@pytest.mark.parametrize("t0", [0, 1])
def test_pinned_transition_tables_oracle_equals_exact_model(t0):
    case = te.transition_case(t0)
    assert case["S"] * case["A"] == 32 and len({(e, k) for e, k, _, _ in case["pins"]}) == 32       # all 32 pairs are pinned
    assert te.transition_coverage([case])
    assert all(te.packable(case["cum"][s, a]) for s in range(case["S"]) for a in range(case["A"]))
    orc = te.oracle_of(case)
    assert np.array_equal(te.prepare(case, orc), case["s0"])
    out = te.oracle_rollout(orc, case["K"])
    assert np.array_equal(out["actions"], case["actions"])
    assert te.check_pins(case, out) == len(case["pins"]) >= 32
    # the same thresholds from the other side: at a pin "on" the word the index moved past the pinned entry, "above" it stayed on it
    for (e, k, q, side), want in zip(case["pins"], case["expect"]):
        lst = case["cum"][(int(case["s0"][e]) + k) % case["S"], case["actions"][k, e]]
        if lst[0] == lst[1]:
            assert want == 2
        else:
            assert want == {("c0", "on"): 1, ("c0", "above"): 0, ("c1", "on"): 2, ("c1", "above"): 1}[(q, side)]
    for k in range(case["K"]):                                      # off the pins: every draw of the run
        for e in range(case["n"]):
            assert te.index_at(case, out, e, k) == te.transition_expect(case, e, k), (e, k)
    assert not out["terminated"].any() and not out["truncated"].any()


@pytest.mark.parametrize("S1", te.S1_VALUES)
def test_pinned_initial_tables_oracle_equals_exact_model(S1):
    for M in (1, 3):
        for t0 in (6, 7):
            family = [te.initial_case(S1, M, t0, flip) for flip in (0, 1)]
            assert te.initial_coverage(family), (S1, M, t0)
            for case in family:
                assert te.packed_S1(case["init_cum"]) == S1
                assert all(case["init_cum"][i] == 0.0 for i in range(0 if S1 == 1 else 1))
                orc = te.oracle_of(case)
                te.prepare(case, orc)
                out = te.oracle_rollout(orc, case["K"])
                assert te.check_pins(case, out) == len(case["pins"]) == S1 - (0 if S1 == 1 else 1)
                ev = np.zeros((case["K"], case["n"]), bool)
                for e, k in case["events"]:
                    ev[k, e] = True
                    assert int(out["obs"][k, e]) == te.initial_expect(case, e, k), (S1, M, t0, e, k)
                assert np.array_equal(out["truncated"], ev)
                assert {k & 1 for _, k in case["events"]} == {0, 1}       # resets inside even and inside odd steps
                # a state behind an equal pair, and state 0, are never drawn
                if S1 >= 3:
                    assert not (out["obs"][ev] == 2).any()
                if S1 >= 2:
                    assert not (out["obs"][ev] == 0).any()


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("name,n,K,t0,env_offset,seed,per_env", te.CARRY_CASES, ids=[c[0] for c in te.CARRY_CASES])
def test_oracle_equals_exact_model_across_every_carry(name, n, K, t0, env_offset, seed, per_env, M):
    from oracle.oracle import OracleTabEnv

    tbl = te.synthetic_table(M)
    seeds = te.scattered_seeds(n) if per_env else None
    orc = OracleTabEnv(tbl["cum"], tbl["prob"], tbl["next"], tbl["reward"], tbl["term"], tbl["init_cum"], n, te.CARRY_LIMIT, seed=seed,
                       action_seed=77, env_offset=env_offset)
    orc.seeds = seeds
    orc.t = t0
    obs0 = orc.reset()
    assert np.array_equal(obs0, te.model_reset(tbl, n, seed=seed, t=t0, r=1, env_offset=env_offset, per_env=seeds))
    ref, (st, el) = te.model_rollout(tbl, obs0, np.zeros(n, np.int32), K, seed=seed, action_seed=77, t0=t0, limit=te.CARRY_LIMIT,
                                     env_offset=env_offset, per_env=seeds)
    _same(ref, te.oracle_rollout(orc, K), name)
    assert np.array_equal(orc.state, st) and np.array_equal(orc.elapsed, el)
    assert ref["truncated"].any() and (M == 1 or len(np.unique(ref["prob"])) > 2)


def test_carry_cases_cross_what_they_claim():
    by = {c[0]: c for c in te.CARRY_CASES}
    assert {by[f"phase{p}"][3] & 3 for p in range(4)} == {0, 1, 2, 3}
    _, _, K, t0, *_ = by["t-2^32"]
    assert t0 < 1 << 32 <= t0 + K - 1 and (t0 >> 2) != ((t0 + K - 1) >> 2)
    _, _, K, t0, *_ = by["b-2^32"]
    assert (t0 >> 1) < 1 << 32 <= ((t0 + K - 1) >> 1)
    _, n, _, _, off, *_ = by["env-2^34"]
    assert off % 4 == 0 and (off >> 2) >> 32 == 1 and ((off + n - 1) >> 2) - (off >> 2) >= 64
    for nm, bits in (("seed-2^32", 32), ("seed-2^64", 64)):
        _, n, _, _, _, seed, _ = by[nm]
        assert seed < 1 << bits <= seed + n - 1


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("spread", [False, True])
def test_oracle_under_a_time_limit_of_one_and_two(M, spread):
    from oracle.oracle import OracleTabEnv

    tbl = te.synthetic_table(M)
    if not spread:
        tbl["init_cum"] = np.array([0.0, 0.0, 1.0, 1.0, 1.0, 1.0])
    for limit in (1, 2):
        n, K = 33, 5
        orc = OracleTabEnv(tbl["cum"], tbl["prob"], tbl["next"], tbl["reward"], tbl["term"], tbl["init_cum"], n, limit, seed=8, action_seed=9)
        obs0 = orc.reset()
        ref, (st, el) = te.model_rollout(tbl, obs0, np.zeros(n, np.int32), K, seed=8, action_seed=9, t0=0, limit=limit)
        _same(ref, te.oracle_rollout(orc, K), (M, spread, limit))
        if limit == 1:
            assert ref["truncated"].all() and not el.any()
        assert np.array_equal(orc.state, st) and np.array_equal(orc.elapsed, el)


def test_oracle_explicit_reset_words():
    from oracle.oracle import OracleTabEnv

    tbl = te.synthetic_table(1)
    n = 67
    for t, r in te.RESET_POINTS:
        for seeds in (None, te.scattered_seeds(n)):
            orc = OracleTabEnv(tbl["cum"], tbl["prob"], tbl["next"], tbl["reward"], tbl["term"], tbl["init_cum"], n, -1, seed=(1 << 32) - 30)
            orc.seeds, orc.t, orc.r = seeds, t, (r - 1) & 0xFFFFFFFF
            got = orc.reset()
            assert np.array_equal(got, te.model_reset(tbl, n, seed=(1 << 32) - 30, t=t, r=r, per_env=seeds)), (t, r)
            assert set(np.unique(got)) <= {1, 2, 4}
