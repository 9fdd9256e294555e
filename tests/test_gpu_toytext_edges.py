"""tab_traj_kernel / tab_step_kernel / tab_reset_kernel (gym_amd/csrc/mxv_tab.hip) held at every threshold, carry, limit and size.

Thresholds: tables whose cumulative probabilities sit exactly on (or one float64 above) Philox words the run WILL draw (tests/tab_edges.py),
through the trajectory kernel (wide and compact), the general kernel (fused, single steps) and a tape replay — against the C twin everywhere
and against the exact Fraction model at every pin; injected uniforms at, below and above every cumulative value.  Carries: every word of
the action, transition and reset counters and of the key across its 2^32 (2^64) boundary inside a launch.  TimeLimit 1 and 2, counters set
at and beyond the limit, terminated-and-truncated steps.  Sizes below a wave and a workgroup, tile counts of every remainder mod 8, guarded
and absent outputs, the host path on both sides of its staging threshold, the masked reset.  Tables on both sides of the two 64-KiB limits.

tests/test_tab_edges_host.py holds the twin to the exact model on the same cases.  Every comparison is exact equality."""
import numpy as np
import pytest

import tab_edges as te

pytestmark = pytest.mark.gpu

I_SENT, F_SENT, U8_SENT = -77, -77.0, 0xA5
GUARD = 2
REAL, INTS, FLAGS = ("reward", "prob", "final_prob"), ("obs", "actions", "final_obs"), ("terminated", "truncated")
FORMS = ("traj", "traj-compact", "fused", "single", "tape")


def _dev():
    import torch

    return torch.device("cuda")


def _native():
    from gym_amd import _native

    return _native


def _tab(tbl, n, limit, **kw):
    return _native().Tab(tbl["S"], tbl["A"], tbl["cum"], tbl["prob"], tbl["next"], tbl["reward"], tbl["term"], tbl["init_cum"], n,
                         -1 if limit is None else limit, **kw)


def _orc(tbl, n, limit, **kw):
    from oracle.oracle import OracleTabEnv

    return OracleTabEnv(tbl["cum"], tbl["prob"], tbl["next"], tbl["reward"], tbl["term"], tbl["init_cum"], n, limit, **kw)


def _pair(tbl, n, limit, *, seed=3, action_seed=4, env_offset=0, t0=0, per_env=None, elapsed0=None, compact=False, general=False):
    """A device handle and its twin after the same explicit reset (r = 1) at step t0 — the reset itself is compared."""
    h = _tab(tbl, n, limit, seed=seed, action_seed=action_seed, env_offset=env_offset, compact=compact, general_kernel=general)
    orc = _orc(tbl, n, limit, seed=seed, action_seed=action_seed, env_offset=env_offset)
    if per_env is not None:
        h.seed(seed, per_env)
        orc.seeds = np.ascontiguousarray(per_env, np.uint64)
    h.set_counters(t0, 0)
    orc.t, orc.r = t0, 0
    assert np.array_equal(h.reset_host(), orc.reset()), "reset"
    if elapsed0 is not None:
        h.set_state(None, elapsed0)
        orc.elapsed[:] = elapsed0
    return h, orc


def _bufs(n, K, compact):
    """Parents [GUARD + K + GUARD][n] filled with sentinels; the launch sees rows GUARD .. GUARD + K - 1."""
    import torch

    it, ft = (torch.int32, torch.float32) if compact else (torch.int64, torch.float64)
    rows = K + 2 * GUARD
    par = {k: torch.full((rows, n), I_SENT, dtype=it, device=_dev()) for k in INTS}
    par.update({k: torch.full((rows, n), F_SENT, dtype=ft, device=_dev()) for k in REAL})
    par.update({k: torch.full((rows, n), U8_SENT, dtype=torch.uint8, device=_dev()) for k in FLAGS})
    return par, {k: v[GUARD:GUARD + K] for k, v in par.items()}


def _run(h, n, K, form, *, compact=False, tape=None, absent=()):
    """One launch form into guarded buffers -> numpy outputs [K][n] (an absent output keeps its sentinel).  traj*: every per-step output, no
    final_* (what selects the trajectory kernel); fused / single / tape: final_obs and final_prob too."""
    import torch

    par, b = _bufs(n, K, compact)
    want_final = not form.startswith("traj")
    arg = lambda name, k=None: None if name in absent or (name.startswith("final") and not want_final) else (b[name] if k is None else b[name][k])
    tape_dev = None
    if form == "tape":
        tape_dev = torch.from_numpy(np.ascontiguousarray(tape, np.int32 if compact else np.int64)).to(_dev())
    torch.cuda.synchronize()
    if form == "single":
        for k in range(K):
            h.rollout(1, b["obs"][k], arg("reward", k), arg("terminated", k), arg("truncated", k), arg("prob", k), arg("final_obs", k),
                      arg("final_prob", k), actions_out_dev=arg("actions", k), per_step=False)
    elif form == "tape":
        h.rollout_tape(K, tape_dev, b["obs"], arg("reward"), arg("terminated"), arg("truncated"), arg("prob"), arg("final_obs"),
                       arg("final_prob"), per_step=True)
    else:
        h.rollout(K, b["obs"], arg("reward"), arg("terminated"), arg("truncated"), arg("prob"), arg("final_obs"), arg("final_prob"),
                  actions_out_dev=arg("actions"), per_step=True)
    h.sync()
    got = {k: v.cpu().numpy() for k, v in par.items()}
    for k, v in got.items():                                        # nothing outside [K][n] changed
        sent = U8_SENT if k in FLAGS else I_SENT
        assert (v[:GUARD] == sent).all() and (v[GUARD + K:] == sent).all(), (form, k, "guard rows")
    return {k: v[GUARD:GUARD + K] for k, v in got.items()}


def _same(got, ref, what, *, sampled=True, compact=False, absent=(), final=True):
    """Every output of every step against the twin's; final_* keep the sentinel where no episode ended, an absent output everywhere."""
    f = (lambda x: x.astype(np.float32)) if compact else (lambda x: x)
    m = ref["final_mask"]
    want = dict(obs=ref["obs"], actions=ref["actions"] if sampled else None, reward=f(ref["reward"]), prob=f(ref["prob"]),
                terminated=ref["terminated"].astype(np.uint8), truncated=ref["truncated"].astype(np.uint8),
                final_obs=np.where(m, ref["final_obs"], I_SENT) if final else None,
                final_prob=np.where(m, f(ref["final_prob"]), f(np.float64(F_SENT))) if final else None)
    for k, w in want.items():
        if k in absent or w is None:
            sent = U8_SENT if k in FLAGS else I_SENT
            assert (got[k] == sent).all(), (what, k, "absent output written")
        else:
            assert np.array_equal(got[k], w), (what, k)


def _state_same(h, orc, what):
    st, el = h.get_state()
    assert np.array_equal(st, orc.state) and np.array_equal(el, orc.elapsed), what
    assert h.get_counters()[0] == orc.t, what


def _kernel(h, form):
    nat = _native()
    return h.last_kernel() == (nat.TAB_KERNEL_TRAJECTORY if form.startswith("traj") else nat.TAB_KERNEL_GENERAL)


def _case_forms(case):
    """A pinned case through the five launch forms -> {form: pins checked}."""
    checked = {}
    for form in FORMS:
        compact = form == "traj-compact"
        h, orc = _pair(case, case["n"], case["limit"], seed=case["seed"], action_seed=case["action_seed"], t0=case["t0"],
                       elapsed0=case["elapsed0"], compact=compact, general=form in ("fused", "single"))
        ref = te.oracle_rollout(orc, case["K"])
        got = _run(h, case["n"], case["K"], form, compact=compact, tape=ref["actions"])
        assert _kernel(h, form), (form, "kernel")
        _same(got, ref, (case["kind"], case.get("S1"), case["M"], case["t0"], form), sampled=form != "tape", compact=compact,
              final=not form.startswith("traj"))
        checked[form] = te.check_pins(case, got)
        _state_same(h, orc, form)
        h.close()
    return checked


# ---- thresholds --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t0", [0, 1])
def test_pinned_transition_thresholds_in_every_form(t0):
    case = te.transition_case(t0)
    assert te.transition_coverage([case])
    checked = _case_forms(case)
    print(f"pinned transition table, t0 = {t0}: pins checked per form {checked}")
    assert set(checked) == set(FORMS) and all(v == len(case["pins"]) >= 32 for v in checked.values())


@pytest.mark.parametrize("S1", te.S1_VALUES)
def test_pinned_initial_thresholds_in_every_form(S1):
    total = {f: 0 for f in FORMS}
    for M in (1, 3):
        for t0 in (6, 7):
            family = [te.initial_case(S1, M, t0, flip) for flip in (0, 1)]
            assert te.initial_coverage(family)
            for case in family:
                for f, c in _case_forms(case).items():
                    assert c == len(case["pins"])
                    total[f] += c
    print(f"pinned initial tables, S1 = {S1}: pins checked per form {total}")
    assert all(v == 8 * (S1 - (0 if S1 == 1 else 1)) for v in total.values())


def _injected_table(last):
    """S = 4, A = 2, M = 3: lists of three, two and one entries (padding -1, whose entries carry a reward and a state nothing else has)."""
    S, A = 4, 2
    lists = [[0.25, 0.5, last], [0.125, last, -1.0], [last, -1.0, -1.0], [1.0 / 3.0, 2.0 / 3.0, last], [0.5, 0.5, last], [2.0 ** -33, 0.75, last],
             [0.1, last, -1.0], [0.7, 0.9, last]]
    cum = np.array(lists).reshape(S, A, 3)
    pad = cum < 0
    rew = np.where(pad, 99.0, np.broadcast_to(np.arange(3.0), (S, A, 3)))
    nxt = np.where(pad, 3, np.broadcast_to(np.arange(3), (S, A, 3))).astype(np.int32)       # index i leads to state i; state 3 only from padding
    prob = np.where(pad, 0.0, np.broadcast_to(np.array(te.PROBS3), (S, A, 3)))
    init = np.array([0.0, 0.25, 0.75, 0.75])
    init[3] = last
    return dict(S=S, A=A, M=3, cum=cum, prob=prob, next=nxt, reward=rew, term=np.zeros((S, A, 3), np.uint8), init_cum=init)


@pytest.mark.parametrize("last", [1.0, 1.0 - 2.0 ** -34, 1.0 - 2.0 ** -33])
def test_injected_uniforms_at_below_and_above_every_cumulative_value(last):
    """step_host(actions, uniforms) on the general kernel: u equal to each cumulative value of each list and of the initial distribution, one
    float64 below and one above (kept inside [0, 1), the range of a uniform)."""
    from fractions import Fraction

    tbl = _injected_table(last)
    S, A = tbl["S"], tbl["A"]
    lanes = []                                                       # (state, action, u_step, u_reset)
    for s in range(S - 1):                                           # state 3 is never entered
        for a in range(A):
            for c in tbl["cum"][s, a]:
                if c >= 0:
                    lanes += [(s, a, u, 0.5) for u in (te.below(c), c, te.above(c)) if 0.0 <= u < 1.0]
    for c in tbl["init_cum"]:
        lanes += [(0, 0, 0.3, u) for u in (te.below(c), c, te.above(c)) if 0.0 <= u < 1.0]
    lanes.append((0, 0, 1.0 - 2.0 ** -33, 1.0 - 2.0 ** -33))         # the largest uniform a word yields
    n = len(lanes)
    st = np.array([l[0] for l in lanes], np.int32)
    act = np.array([l[1] for l in lanes], np.int64)
    uni = np.array([[l[2] for l in lanes], [l[3] for l in lanes]])
    for limit in (-1, 1):                                            # limit 1: every step ends in a reset drawn with u_reset
        h, orc = _tab(tbl, n, limit, seed=1, action_seed=2), _orc(tbl, n, limit, seed=1, action_seed=2)
        h.reset_host(), orc.reset()
        h.set_state(st, np.zeros(n, np.int32))
        orc.state[:] = st
        obs, rew, term, trunc, prob, fin, fprob = h.step_host(act, uni)
        assert h.last_kernel() == _native().TAB_KERNEL_GENERAL
        o = orc.step(act, uni)
        for got, key in ((obs, "obs"), (rew, "reward"), (term, "terminated"), (trunc, "truncated"), (prob, "prob")):
            assert np.array_equal(got, o[key]), (last, limit, key)
        assert not (rew == 99.0).any() and not (fin == 3).any() and (limit == 1 or not (obs == 3).any())    # padding is never selected
        for i, (s, a, us, ur) in enumerate(lanes):
            idx = te.sample_exact(tbl["cum"][s, a], Fraction(us))
            assert rew[i] == idx, (last, limit, i)
            if limit == 1:
                assert trunc[i] and fin[i] == idx and fprob[i] == te.PROBS3[idx] and prob[i] == 1.0
                assert obs[i] == te.sample_exact(tbl["init_cum"], Fraction(ur)), (last, i)
            else:
                assert not trunc[i] and obs[i] == idx and prob[i] == te.PROBS3[idx]
        h.close()


@pytest.mark.parametrize("last,packs", [(1.0 - 2.0 ** -34, True), (1.0 - 2.0 ** -33, False)])
def test_a_last_value_just_below_one(last, packs):
    """1 - 2^-34 exceeds every uniform a word yields: accepted by the packing, behaves as 1.  1 - 2^-33 IS the largest uniform: such a list keeps
    the general kernel."""
    tbl = te.synthetic_table(3)
    tbl["cum"] = np.where(tbl["cum"] == 1.0, last, tbl["cum"])
    n, K = 513, 9
    h, orc = _pair(tbl, n, 4)
    got = _run(h, n, K, "traj")
    assert _kernel(h, "traj" if packs else "fused")
    ref = te.oracle_rollout(orc, K)
    _same(got, ref, last, final=False)
    if packs:
        one = te.synthetic_table(3)
        h1, orc1 = _pair(one, n, 4)
        _same(_run(h1, n, K, "traj"), ref, "as 1.0", final=False)
        h1.close()
    h.close()


# ---- carries -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("name,n,K,t0,env_offset,seed,per_env", te.CARRY_CASES, ids=[c[0] for c in te.CARRY_CASES])
def test_counter_and_key_carries_inside_a_launch(name, n, K, t0, env_offset, seed, per_env, M):
    tbl = te.synthetic_table(M)
    seeds = te.scattered_seeds(n) if per_env else None
    for form in ("traj", "traj-compact", "fused", "single"):
        compact = form == "traj-compact"
        h, orc = _pair(tbl, n, te.CARRY_LIMIT, seed=seed, action_seed=77, env_offset=env_offset, t0=t0, per_env=seeds, compact=compact,
                       general=form in ("fused", "single"))
        ref = te.oracle_rollout(orc, K)
        got = _run(h, n, K, form, compact=compact)
        assert _kernel(h, form)
        _same(got, ref, (name, M, form), compact=compact, final=not form.startswith("traj"))
        assert h.get_counters() == (t0 + K, 1)
        h.close()
    assert ref["truncated"].any()


def test_point_mass_start_across_the_carries():
    """FrozenLake-v1 (M = 3, a point-mass start: the kernel variant without a reset search) over the same launches."""
    from gym_amd.toy_text import frozen_lake_mdp

    m = frozen_lake_mdp(map_name="4x4")
    tbl = dict(S=m.num_states, A=m.num_actions, M=3, cum=m.cum_prob, prob=m.prob, next=m.next_state, reward=m.reward, term=m.terminated,
               init_cum=m.initial_cum)
    for name, n, K, t0, env_offset, seed, per_env in te.CARRY_CASES[3:]:
        seeds = te.scattered_seeds(n) if per_env else None
        for form in ("traj", "fused"):
            h, orc = _pair(tbl, n, 5, seed=seed, action_seed=78, env_offset=env_offset, t0=t0, per_env=seeds, general=form == "fused")
            ref = te.oracle_rollout(orc, K)
            _same(_run(h, n, K, form), ref, (name, form), final=form == "fused")
            assert _kernel(h, form)
            h.close()


def test_explicit_reset_above_2_32_and_at_several_ordinals():
    tbl = te.synthetic_table(1)
    n = 321
    for per_env in (None, te.scattered_seeds(n)):
        h, orc = _tab(tbl, n, -1, seed=(1 << 32) - 30), _orc(tbl, n, -1, seed=(1 << 32) - 30)
        if per_env is not None:
            h.seed((1 << 32) - 30, per_env)
            orc.seeds = per_env
        for t, r in te.RESET_POINTS:
            h.set_counters(t, (r - 1) & 0xFFFFFFFF)
            orc.t, orc.r = t, (r - 1) & 0xFFFFFFFF
            got = h.reset_host()
            assert np.array_equal(got, orc.reset()), (t, r)
            assert h.get_counters() == (t, r)
            assert np.array_equal(got[:16], te.model_reset(tbl, 16, seed=(1 << 32) - 30, t=t, r=r, per_env=per_env))
        h.close()


# ---- time limits -------------------------------------------------------------------------------------------------------------------
def _point(tbl, s=2):
    t = dict(tbl)
    t["init_cum"] = (np.arange(tbl["S"]) >= s).astype(np.float64)
    return t


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("spread", [False, True])
@pytest.mark.parametrize("limit", [1, 2, -1, 0])
def test_time_limits_of_one_two_and_none(limit, spread, M):
    tbl = te.synthetic_table(M) if spread else _point(te.synthetic_table(M))
    n, K = 300, 7
    for form in ("traj", "traj-compact", "fused", "single"):
        compact = form == "traj-compact"
        h, orc = _pair(tbl, n, limit, t0=1, compact=compact, general=form in ("fused", "single"))
        ref = te.oracle_rollout(orc, K)
        _same(_run(h, n, K, form, compact=compact), ref, (limit, spread, M, form), compact=compact, final=not form.startswith("traj"))
        assert _kernel(h, form)
        _state_same(h, orc, (limit, spread, M, form))
        h.close()
    if limit == 1:
        assert ref["truncated"].all()
    elif limit == 2:
        assert ref["truncated"].any() and not ref["truncated"].all()
    else:
        assert not ref["truncated"].any() and ref["terminated"].any()


@pytest.mark.parametrize("M", [1, 3])
def test_elapsed_set_at_and_beyond_the_limit_and_terminal_truncated_steps(M):
    tbl = te.synthetic_table(M)
    n, K, limit = 600, 3, 6
    el0 = np.array([limit - 1, limit, limit + 5, 0, limit - 2], np.int32)[np.arange(n) % 5]
    for form in ("traj", "fused", "single"):
        h, orc = _pair(tbl, n, limit, elapsed0=el0, general=form != "traj")
        ref = te.oracle_rollout(orc, K)
        got = _run(h, n, K, form)
        _same(got, ref, (M, form), final=form != "traj")
        _state_same(h, orc, (M, form))
        h.close()
        if form == "fused":
            both = got["terminated"][0].astype(bool) & got["truncated"][0].astype(bool)
            assert both.any()                                     # terminated and truncated in one step: final_* are the terminal transition's
            assert np.array_equal(got["final_obs"][0][both], ref["final_obs"][0][both])
            assert np.array_equal(got["final_prob"][0][both], ref["final_prob"][0][both]) and (got["prob"][0][both] == 1.0).all()
            if M == 3:
                assert len(np.unique(got["final_prob"][0][both])) > 1
    first = ref["truncated"][0]
    assert first[el0 >= limit - 1].all() and not first[el0 < limit - 1].any()            # the next step truncates, at or beyond the limit


# ---- sizes, outputs, the host path ---------------------------------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 255, 256, 257] + [256 * k + 1 for k in range(7, 16)]


@pytest.mark.parametrize("n", SIZES)
def test_every_size_and_tile_count_into_guarded_buffers(n):
    K = 5
    for M in (1, 3):
        tbl = te.synthetic_table(M)
        for form in ("traj", "traj-compact", "fused"):
            compact = form == "traj-compact"
            h, orc = _pair(tbl, n, 3, seed=13, action_seed=14, t0=2, compact=compact, general=form == "fused")
            ref = te.oracle_rollout(orc, K)
            _same(_run(h, n, K, form, compact=compact), ref, (n, M, form), compact=compact, final=form == "fused")
            assert _kernel(h, form)
            _state_same(h, orc, (n, M, form))
            h.close()


def test_tile_counts_cover_every_remainder_mod_8():
    assert {(n + 255) // 256 % 8 for n in SIZES if n > 257} == set(range(8)) and max(SIZES) <= 4353


@pytest.mark.parametrize("n", [257, 2049])
def test_each_optional_output_absent_in_turn(n):
    tbl = te.synthetic_table(3)
    K = 4
    for name in ("reward", "terminated", "truncated", "prob", "final_obs", "final_prob", "actions"):
        for form in ("fused", "single"):
            h, orc = _pair(tbl, n, 3, general=True)
            ref = te.oracle_rollout(orc, K)
            _same(_run(h, n, K, form, absent=(name,)), ref, (name, form), absent=(name,))
            assert _kernel(h, form)
            _state_same(h, orc, (name, form))
            h.close()


def _staging_total(n):
    """The byte count tab_ensure_staging compares with 2 MiB: six 8-byte arrays, the [2][n] uniforms, three byte arrays, the error word."""
    up = lambda b: (b + 255) // 256 * 256
    return 6 * up(n * 8) + up(2 * n * 8) + 3 * up(n) + 256


def test_host_path_on_both_sides_of_the_staging_threshold():
    lim = 2 << 20
    n_lo = max(n for n in range(30000, 33000) if _staging_total(n) <= lim)
    assert _staging_total(n_lo) <= lim < _staging_total(n_lo + 1) and all(_staging_total(n) <= lim for n in range(1, n_lo, 97))
    tbl = te.synthetic_table(3)
    rng = np.random.default_rng(5)
    for n in (n_lo, n_lo + 1):
        h, orc = _pair(tbl, n, 3, seed=(1 << 32) - 7)
        for step in range(4):
            a = rng.integers(0, tbl["A"], n)
            obs, rew, term, trunc, prob, fin, fprob = h.step_host(a)
            o = orc.step(a)
            for got, key in ((obs, "obs"), (rew, "reward"), (term, "terminated"), (trunc, "truncated"), (prob, "prob")):
                assert np.array_equal(got, o[key]), (n, step, key)
            m = o["final_mask"]
            assert np.array_equal(fin[m], o["final_obs"][m]) and np.array_equal(fprob[m], o["final_prob"][m])
            if step == 1:
                mask = rng.random(n) < 0.5
                assert np.array_equal(h.reset_host(mask), orc.reset(mask=mask)), (n, "masked reset")
        _state_same(h, orc, n)
        h.close()


@pytest.mark.parametrize("n", [1, 255, 1025])
def test_masked_reset_redraws_the_masked_and_keeps_the_rest(n):
    import torch

    tbl = te.synthetic_table(1)
    h, orc = _pair(tbl, n, 50, t0=(1 << 32) - 2)
    a = np.arange(n) % tbl["A"]
    for _ in range(3):
        h.step_host(a), orc.step(a)
    st0, el0 = h.get_state()
    assert el0.any() or n == 1
    for mask in (np.arange(n) % 3 == 0, np.zeros(n, bool), np.ones(n, bool)):
        before = h.get_state()
        obs_dev = torch.full((n,), I_SENT, dtype=torch.int64, device=_dev())
        mask_dev = torch.from_numpy(mask.astype(np.uint8)).to(_dev())
        torch.cuda.synchronize()
        h.reset(obs_dev, mask_dev)
        h.sync()
        want = orc.reset(mask=mask)
        st, el = h.get_state()
        assert np.array_equal(obs_dev.cpu().numpy(), want) and np.array_equal(st, orc.state) and np.array_equal(el, orc.elapsed)
        assert np.array_equal(st[~mask], before[0][~mask]) and np.array_equal(el[~mask], before[1][~mask]) and not el[mask].any()
        assert np.array_equal(want, st)                              # masked: the new state; unmasked: the current one
        h.step_host(a), orc.step(a)
    _state_same(h, orc, n)
    h.close()


# ---- table placement ---------------------------------------------------------------------------------------------------------------
LDS_LIMIT = 64 * 1024


def _general_lds_bytes(S, A, M, all_one):
    """lds_bytes of mxv_tab_create: reward + (cum when M > 1) + (prob unless every probability is 1) as float64, next|terminated as int32,
    the initial distribution."""
    return S * A * M * (8 * (1 + (1 if M > 1 else 0) + (0 if all_one else 1)) + 4) + S * 8


def _packed_bytes(S, A, M, init_words):
    """The table of pack_fast_table: two thresholds per (s, a) when M == 3, padded to 16 bytes; entries of 8 (M == 1) or 3 x 16 bytes; the
    initial thresholds (S1 + 1 words, none for a point mass), padded to 16 bytes."""
    up4 = lambda w: (w + 3) // 4 * 4
    return 4 * up4(up4(S * A * 2 if M == 3 else 0) + S * A * (2 if M == 1 else 12) + init_words)


def _lake(size):
    from gym_amd.toy_text import frozen_lake_mdp

    rng = np.random.default_rng(size)
    rows = [["F"] * size for _ in range(size)]
    for _ in range(size * size // 10):
        rows[rng.integers(size)][rng.integers(size)] = "H"
    rows[0][0], rows[size - 1][size - 1] = "S", "G"
    m = frozen_lake_mdp(desc=["".join(r) for r in rows])
    return dict(S=m.num_states, A=m.num_actions, M=m.max_transitions, cum=m.cum_prob, prob=m.prob, next=m.next_state, reward=m.reward,
                term=m.terminated, init_cum=m.initial_cum)


def _placement_run(tbl, n, K, limit, traj_packs, what):
    """Sampled fused rollouts (wide and compact), a tape: the twin everywhere, the trajectory kernel against the general one where both exist."""
    runs = {}
    for form in ("traj", "traj-compact", "fused", "fused-compact", "tape"):
        compact = form.endswith("compact")
        base = form.split("-")[0]
        h, orc = _pair(tbl, n, limit, seed=17, action_seed=18, compact=compact, general=base == "fused")
        ref = te.oracle_rollout(orc, K)
        got = _run(h, n, K, base, compact=compact, tape=ref["actions"])
        assert _kernel(h, base if (traj_packs or base != "traj") else "fused"), (what, form)
        _same(got, ref, (what, form), sampled=base != "tape", compact=compact, final=base != "traj")
        _state_same(h, orc, (what, form))
        h.close()
        runs[form] = got
    for fast, gen in (("traj", "fused"), ("traj-compact", "fused-compact")):        # the two kernels directly, output by output
        for key in ("obs", "actions", "reward", "prob", "terminated", "truncated"):
            assert runs[fast][key].dtype == runs[gen][key].dtype and np.array_equal(runs[fast][key], runs[gen][key]), (what, fast, key)
    assert ref["terminated"].any() and ref["truncated"].any()


@pytest.mark.parametrize("size,general_in_lds,traj_packs", [(13, True, True), (14, False, True), (17, False, True), (18, False, False)])
def test_custom_maps_on_either_side_of_the_two_64_kib_limits(size, general_in_lds, traj_packs):
    tbl = _lake(size)
    S = size * size
    assert (tbl["S"], tbl["A"], tbl["M"]) == (S, 4, 3)
    assert (_general_lds_bytes(S, 4, 3, False) <= LDS_LIMIT) == general_in_lds
    assert (_packed_bytes(S, 4, 3, 0) <= LDS_LIMIT) == traj_packs
    _placement_run(tbl, 2049, 24, 11, traj_packs, size)


def _flat_table(S, A, S1):
    """M = 1 (every probability 1): next state and reward from a fixed rule, a few terminal entries, S1 states below 2^32 at the start."""
    sa = np.arange(S * A).reshape(S, A, 1)
    init = np.ones(S)
    init[:S1] = (np.arange(S1) + 1.0) / (S1 + 1)
    return dict(S=S, A=A, M=1, cum=np.ones((S, A, 1)), prob=np.ones((S, A, 1)), next=((sa * 7 + 3) % S).astype(np.int32),
                reward=((sa % 5) - 2) * 0.5, term=(sa % 11 == 0).astype(np.uint8), init_cum=init)


@pytest.mark.parametrize("S,A,S1,general_in_lds,traj_packs", [(128, 42, 3, True, True), (128, 43, 3, False, True), (90, 91, 3, False, True),
                                                              (90, 91, 4, False, False)])
def test_tables_of_exactly_64_kib_and_just_above(S, A, S1, general_in_lds, traj_packs):
    """128 x 42: the general table is 65 536 B exactly, 128 x 43 is above; 90 x 91 with four initial words: the packed table is 65 536 B exactly,
    with eight it is above and a trajectory launch takes the general kernel."""
    tbl = _flat_table(S, A, S1)
    g, p = _general_lds_bytes(S, A, 1, True), _packed_bytes(S, A, 1, S1 + 1)
    assert (g <= LDS_LIMIT) == general_in_lds and (p <= LDS_LIMIT) == traj_packs
    assert (S, A) != (128, 42) or g == LDS_LIMIT
    assert (S, A, S1) != (90, 91, 3) or p == LDS_LIMIT
    assert te.packed_S1(tbl["init_cum"]) == S1
    _placement_run(tbl, 2049, 24, 9, traj_packs, (S, A, S1))
