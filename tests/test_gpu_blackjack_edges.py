"""bj_kernel / bj_reset_kernel (gym_amd/csrc/mxv_bj.hip) held at every hand, size and launch form.

Injected cards against the literal model of tests/bj_host.py: every reachable player state against every dealer completion under all four
rule settings, every hit, every deal, TimeLimit.  Philox mode against the C oracle (OracleBlackjack): all rule settings, sizes below one
wave and one workgroup, tile counts of every remainder mod 8, forced fifth-and-later dealer draws, the step counter across 2^32, the high
word of the action counter, the action-block boundary inside a launch, per-env seeds, compact outputs, absent outputs, guarded buffers, the
host path on both sides of its staging threshold, and the reset kernel in its Philox, injected and masked forms.

Every value is an integer or one of -1, 0, 1, 1.5: every comparison is exact equality."""
import numpy as np
import pytest

import bj_host as bj

pytestmark = pytest.mark.gpu

I_SENT, U8_SENT = -77, 0xA5
BIG_OFFSET = (1 << 34) + 4092          # the high word of the action counter (env >> 2 >= 2^32), all four words of a group in 257 lanes
T_WRAP = (1 << 32) - 3                 # == 29 (mod 32): K = 7 crosses both the action block and the low word of the step counter


def _dev():
    import torch

    return torch.device("cuda")


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _bufs(n, K=None, compact=False, ints=I_SENT):
    """Output tensors [K][(3)][n] (no K axis for K=None), integer observations prefilled with a sentinel."""
    import torch

    it, ft = (torch.int32, torch.float32) if compact else (torch.int64, torch.float64)
    lead = () if K is None else (K,)
    d = _dev()
    return dict(obs=torch.full(lead + (3, n), ints, dtype=it, device=d), reward=torch.full(lead + (n,), float(I_SENT), dtype=ft, device=d),
                terminated=torch.full(lead + (n,), U8_SENT, dtype=torch.uint8, device=d),
                truncated=torch.full(lead + (n,), U8_SENT, dtype=torch.uint8, device=d),
                final_obs=torch.full(lead + (3, n), ints, dtype=it, device=d), actions=torch.full(lead + (n,), ints, dtype=it, device=d))


def _np(b):
    return {k: v.cpu().numpy() for k, v in b.items()}


def _oracle_words(orc):
    """The device's state word of every oracle table, from its card lists (rows of int[33]: 32 cards, then the count)."""
    def fields(a):
        cnt = a[:, 32].astype(np.int64)
        c = np.where(np.arange(32)[None, :] < cnt[:, None], a[:, :32], 0).astype(np.int64)
        return c.sum(1), (c == 1).any(1).astype(np.int64), (cnt == 2).astype(np.int64), c[:, 0]

    ps, pa, pt, _ = fields(orc.player)
    ds, da, dt, df = fields(orc.dealer)
    return bj.pack(ps, pa, pt, df, ds, da, dt).astype(np.int32)


def _set_oracle_hands(orc, player, dealer):
    for arr, hand in ((orc.player, player), (orc.dealer, dealer)):
        arr[:] = 0
        arr[:, :len(hand)] = hand
        arr[:, 32] = len(hand)


def _oracle_rollout(orc, K, tape=None):
    outs = [orc.step(None if tape is None else tape[k]) for k in range(K)]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def _device_rollout(h, n, K, *, compact=False, tape=None, single=False, absent=()):
    """One fused launch (or K launches of one step) into sentinel-filled buffers -> (numpy outputs, (state, elapsed), counters)."""
    import torch

    b = _bufs(n, K, compact)
    tape_dev = None if tape is None else _t(np.asarray(tape, np.int64))
    torch.cuda.synchronize()
    arg = lambda name, k=None: None if name in absent else (b[name] if k is None else b[name][k])
    if single:
        for k in range(K):
            h.rollout(1, b["obs"][k], arg("reward", k), arg("terminated", k), arg("truncated", k), arg("final_obs", k),
                      None if tape is not None else arg("actions", k), actions_tape_dev=None if tape is None else tape_dev[k], compact=compact)
    else:
        h.rollout(K, b["obs"], arg("reward"), arg("terminated"), arg("truncated"), arg("final_obs"), None if tape is not None else arg("actions"),
                  actions_tape_dev=tape_dev, per_step=True, compact=compact)
    h.sync()
    return _np(b), h.get_state(), h.get_counters()


def _assert_equals_oracle(got, ref, *, sampled=True, what=""):
    """Every output of every step; final_obs columns of tables that did not finish keep the sentinel."""
    if sampled:
        assert np.array_equal(got["actions"], ref["actions"]), (what, "actions")
    assert np.array_equal(got["obs"], ref["obs"]), (what, "obs")
    assert np.array_equal(got["reward"], ref["reward"]), (what, "reward")
    assert np.array_equal(got["terminated"], ref["terminated"].astype(np.uint8)), (what, "terminated")
    assert np.array_equal(got["truncated"], ref["truncated"].astype(np.uint8)), (what, "truncated")
    m = np.broadcast_to(ref["final_mask"][:, None, :], ref["final_obs"].shape)
    assert np.array_equal(got["final_obs"], np.where(m, ref["final_obs"], I_SENT)), (what, "final_obs")


def _pair(n, *, natural, sab, seed=3, action_seed=4, env_offset=0, t0=0, per_env_seeds=None, max_episode_steps=-1):
    """A device handle and its oracle twin after the same Philox reset, both at step t0.  The reset itself is compared."""
    from gym_amd import _native
    from oracle.oracle import OracleBlackjack

    h = _native.Blackjack(n, natural=natural, sab=sab, max_episode_steps=max_episode_steps, env_offset=env_offset, seed=seed, action_seed=action_seed)
    orc = OracleBlackjack(n, natural=natural, sab=sab, max_episode_steps=max_episode_steps, seed=seed, action_seed=action_seed, env_offset=env_offset)
    if per_env_seeds is not None:
        h.seed(seed, per_env_seeds, action_seed)
        orc.seeds = np.ascontiguousarray(per_env_seeds, dtype=np.uint64)
    assert np.array_equal(h.reset_host(), orc.reset()), "reset"
    if t0:
        h.set_state(None, None, t=t0, r=1)
        orc.t = t0
    st, el = h.get_state()
    assert np.array_equal(st, _oracle_words(orc)) and not el.any()
    return h, orc


def _seeds(n):
    """Per-env seeds in no arithmetic progression, every third one >= 2^63."""
    s = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0x0123456789ABCDEF)
    s[::3] |= np.uint64(1 << 63)
    assert (s >= np.uint64(1 << 63)).sum() >= n // 3 and len(set(s.tolist())) == n
    return s


# ---- injected cards against the model ------------------------------------------------------------------------------------------------------
_STICK = {}


def _stick_product():
    """Inputs and the rule-independent expectations of the stick product, built once: lane = player state j * 54 433 + completion c."""
    if not _STICK:
        ct, reps = bj.completion_table(), bj.player_representatives()
        C, P = len(ct["ndraws"]), len(reps)
        assert (C, P) == (54_433, 62)
        ps = bj.summarise(reps.values())
        n = P * C
        lane_p, lane_c = np.repeat(np.arange(P), C), np.tile(np.arange(C), P)
        deal = bj.deals_of(np.arange(n) * 7 + 13)
        rows = np.tile(bj.stick_rows(np.zeros((C, 4), np.int8)), (P, 1))
        col = ct["ndraws"][lane_c][:, None] + np.arange(4)[None, :]
        rows[np.arange(n)[:, None], col] = deal
        state = bj.pack(ps["raw"][lane_p], ps["ace"][lane_p], ps["two"][lane_p], ct["first"][lane_c], ct["start_raw"][lane_c],
                        ct["start_ace"][lane_c], 1).astype(np.int32)
        _STICK.update(n=n, lane_p=lane_p, lane_c=lane_c, deal=deal, rows=rows, state=state, ps=ps, ct=ct,
                      final_obs=np.stack([ps["total"][lane_p], ct["first"][lane_c], ps["usable"][lane_p]]), obs=bj.obs_of_deal(deal),
                      new_state=bj.pack_deal(deal))
    return _STICK


@pytest.mark.parametrize("natural,sab", bj.RULES)
def test_injected_stick_product_equals_model(natural, sab):
    """62 player states x 54 433 dealer completions = 3 374 846 lanes in one launch, the four dealt cards varying per lane."""
    import torch
    from gym_amd import _native

    s = _stick_product()
    n, ps, ct, lp, lc = s["n"], s["ps"], s["ct"], s["lane_p"], s["lane_c"]
    assert n == 62 * 54_433 == 3_374_846
    pn, dn, dsc = ps["natural"][lp], ct["natural"][lc], ct["score"][lc]
    assert (pn & dn).any(), "a natural against a natural"
    assert (pn & (dsc == 21) & (ct["ncards"][lc] == 3)).any(), "a natural against a 21 of three cards"
    assert (dsc == 0).any() and (ct["ndraws"][lc] == 10).any(), "a dealer bust, a completion of ten draws"
    want_reward = bj.reward_table(natural, sab)[ps["score"][lp], pn, dsc, dn]
    assert (1.5 in want_reward) == (natural and not sab) and {-1.0, 0.0, 1.0} <= set(np.unique(want_reward))
    h = _native.Blackjack(n, natural=natural, sab=sab)
    h.set_state(s["state"], np.zeros(n, np.int32), t=0, r=1)
    b = _bufs(n)
    cards, actions = _t(s["rows"]), torch.zeros(n, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    h.step(actions, b["obs"], b["reward"], b["terminated"], b["truncated"], b["final_obs"], cards_dev=cards)
    h.sync()
    got = _np(b)
    st, el = h.get_state()
    h.close()
    bad = np.flatnonzero(got["reward"] != want_reward)
    assert bad.size == 0, (bad.size, [(list(bj.player_representatives())[lp[i]], bj.dealer_completions()[lc[i]], got["reward"][i], want_reward[i]) for i in bad[:4]])
    assert np.all(got["terminated"] == 1) and np.all(got["truncated"] == 0)
    for name in ("final_obs", "obs"):
        assert np.array_equal(got[name], s[name]), name
    assert np.array_equal(st, s["new_state"]) and not el.any()


def test_injected_hit_product_equals_model():
    """62 player states x 10 hit cards x 16 deals (and 16 dealer hands): bust or not, the new (sum, ace, two = 0) state, the dealer's hand
    untouched where nobody finished."""
    import torch
    from gym_amd import _native

    reps = list(bj.player_representatives().values())
    lanes = [(hand, c, k) for hand in reps for c in bj.CARDS for k in range(16)]
    n = len(lanes)
    assert n == 62 * 10 * 16
    deal = bj.deals_of(np.arange(n) * 619 + 7)
    assert len({tuple(r) for r in deal.tolist()}) == n            # 16 distinct deals per (state, card), none used twice
    dealers = [[1 + (i * 3) % 10, 1 + (i // 16 + i) % 10] for i in range(n)]
    rows = bj.injected_rows([[c] for _, c, _ in lanes], deal)
    state0 = np.array([bj.pack_hands(hand, d) for (hand, _, _), d in zip(lanes, dealers)], np.int32)
    want = dict(obs=np.zeros((3, n), np.int64), reward=np.zeros(n), terminated=np.zeros(n, np.uint8), final_obs=np.full((3, n), I_SENT, np.int64))
    want_state, want_el = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i, ((hand, c, _), d) in enumerate(zip(lanes, dealers)):
        t = bj.Table(True, False)
        t.player, t.dealer, t.elapsed = list(hand), list(d), 4
        o = t.step(1, rows[i])
        want["obs"][:, i], want["reward"][i], want["terminated"][i] = o["obs"], o["reward"], o["terminated"]
        if o["final_obs"] is not None:
            want["final_obs"][:, i] = o["final_obs"]
        else:
            assert t.dealer == d and len(t.player) == len(hand) + 1
        want_state[i], want_el[i] = bj.pack_hands(t.player, t.dealer), t.elapsed
    nbust = int(want["terminated"].sum())
    assert 0 < nbust < n and np.all(want["reward"] == -1.0 * want["terminated"])
    h = _native.Blackjack(n, natural=True, sab=False)
    h.set_state(state0, np.full(n, 4, np.int32), t=0, r=1)
    b = _bufs(n)
    cards, actions = _t(rows), torch.ones(n, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    h.step(actions, b["obs"], b["reward"], b["terminated"], b["truncated"], b["final_obs"], cards_dev=cards)
    h.sync()
    got = _np(b)
    st, el = h.get_state()
    h.close()
    for name in want:
        assert np.array_equal(got[name], want[name]), name
    assert not got["truncated"].any()
    assert np.array_equal(st, want_state), np.flatnonzero(st != want_state)[:8]
    alive = want["terminated"] == 0
    u = bj.unpack(st[alive])
    assert not u["p_two"].any() and np.array_equal(st[alive] >> 8, state0[alive] >> 8)
    assert np.array_equal(el, want_el) and np.array_equal(el, np.where(alive, 5, 0))


def test_injected_deal_product_equals_model():
    """All 10^4 deals after a bust (lanes 0..9999) and after a stick (10 000..19 999): obs and every field of the new state word."""
    import torch
    from gym_amd import _native

    n = 20_000
    deal = bj.deals_of(np.arange(n))
    bust = np.arange(n) < 10_000
    rows = bj.injected_rows([[10] if x else [] for x in bust], deal)
    h = _native.Blackjack(n, natural=False, sab=True)
    h.set_state(np.full(n, bj.pack_hands([10, 6, 4], [10, 10]), np.int32), np.full(n, 2, np.int32), t=0, r=1)
    b = _bufs(n)
    cards, actions = _t(rows), _t(bust.astype(np.int64))
    torch.cuda.synchronize()
    h.step(actions, b["obs"], b["reward"], b["terminated"], b["truncated"], b["final_obs"], cards_dev=cards)
    h.sync()
    got = _np(b)
    st, el = h.get_state()
    h.close()
    assert np.all(got["terminated"] == 1) and np.array_equal(got["reward"], np.where(bust, -1.0, 0.0))
    assert np.array_equal(got["final_obs"], np.stack([np.where(bust, 30, 20), np.full(n, 10), np.zeros(n, np.int64)]))
    assert np.array_equal(got["obs"], bj.obs_of_deal(deal))
    u, d = bj.unpack(st), deal.astype(np.int64)
    assert np.array_equal(u["p_sum"], d[:, 2] + d[:, 3]) and np.array_equal(u["p_ace"], ((d[:, 2] == 1) | (d[:, 3] == 1)).astype(np.int64))
    assert np.array_equal(u["dfirst"], d[:, 0]) and np.array_equal(u["d_sum"], d[:, 0] + d[:, 1])
    assert np.array_equal(u["d_ace"], ((d[:, 0] == 1) | (d[:, 1] == 1)).astype(np.int64))
    assert u["p_two"].all() and u["d_two"].all() and np.array_equal(st, bj.pack_deal(deal)) and not (st >> 20).any() and not el.any()


@pytest.mark.parametrize("limit", [1, 2, 3, -1])
def test_injected_time_limit_equals_model(limit):
    """elapsed in {0, 1, 2} (through set_state) x {non-busting hit, busting hit, stick}: truncated alone, both flags, neither; final_obs is
    the hand after the hit; the counter is 0 after a finish and +1 otherwise; max_episode_steps = -1 never truncates."""
    from gym_amd import _native

    cases = [(e, kind) for e in (0, 1, 2) for kind in ("hit", "bust", "stick")]
    n = len(cases)
    rows = bj.injected_rows([{"hit": [2], "bust": [10], "stick": []}[k] for _, k in cases], [[2, 3, 1, 5]] * n)
    acts = np.array([k != "stick" for _, k in cases], np.int64)
    h = _native.Blackjack(n, natural=False, sab=True, max_episode_steps=limit)
    h.set_state(np.full(n, bj.pack_hands([5, 4, 3], [10, 9]), np.int32), np.array([e for e, _ in cases], np.int32), t=0, r=1)
    import torch

    b = _bufs(n)
    cards, actions = _t(rows), _t(acts)
    torch.cuda.synchronize()
    h.step(actions, b["obs"], b["reward"], b["terminated"], b["truncated"], b["final_obs"], cards_dev=cards)
    h.sync()
    got = _np(b)
    st, el = h.get_state()
    h.close()
    seen = set()
    for i, (e, kind) in enumerate(cases):
        t = bj.Table(False, True, limit)
        t.player, t.dealer, t.elapsed = [5, 4, 3], [10, 9], e
        o = t.step(int(acts[i]), rows[i])
        assert o["truncated"] == (limit > 0 and e + 1 >= limit) and o["terminated"] == (kind != "hit")
        assert (got["terminated"][i], got["truncated"][i], got["reward"][i]) == (o["terminated"], o["truncated"], o["reward"]), (limit, e, kind)
        done = o["terminated"] or o["truncated"]
        assert el[i] == t.elapsed == (0 if done else e + 1), (limit, e, kind)
        assert tuple(got["obs"][:, i]) == o["obs"] and st[i] == bj.pack_hands(t.player, t.dealer)
        if done:
            assert tuple(got["final_obs"][:, i]) == o["final_obs"] == ({"hit": 14, "bust": 22, "stick": 12}[kind], 10, 0), (limit, e, kind)
            assert o["obs"] == (16, 2, 1)
        else:
            assert tuple(got["final_obs"][:, i]) == (I_SENT,) * 3 and o["obs"] == (14, 10, 0)
        seen.add((bool(o["terminated"]), bool(o["truncated"])))
    if limit == -1:
        assert not got["truncated"].any() and seen == {(True, False), (False, False)}
    elif limit == 1:
        assert got["truncated"].all() and seen == {(True, True), (False, True)}
    elif limit == 3:
        assert seen == {(False, True), (True, True), (True, False), (False, False)}


# ---- Philox mode against the oracle ----------------------------------------------------------------------------------------------------------
SMALL = [1, 63, 64, 65, 255, 256, 257]
SWEEP = [256 * k + 1 for k in range(1, 17)]          # 2 .. 17 tiles: every remainder of the tile count mod 8 with base 0, 1 and 2


def _rollout_against_oracle(n, natural, sab, K=9):
    h, orc = _pair(n, natural=natural, sab=sab, seed=11, action_seed=12)
    got, (st, el), (t, r) = _device_rollout(h, n, K)
    h.close()
    ref = _oracle_rollout(orc, K)
    _assert_equals_oracle(got, ref, what=(n, natural, sab))
    assert np.array_equal(st, _oracle_words(orc)) and np.array_equal(el, orc.elapsed) and (t, r) == (K, 1)
    return ref


def test_tile_sweep_covers_every_remainder():
    tiles = sorted({(n + 255) // 256 for n in SWEEP})
    assert tiles == list(range(2, 18)) and {(x % 8, x // 8) for x in tiles} >= {(m, b) for m in range(8) for b in (1,)} | {(0, 2), (1, 2), (2, 0), (7, 0)}


@pytest.mark.parametrize("n", SMALL + SWEEP[1:])
def test_philox_sizes_equal_oracle(n):
    ref = _rollout_against_oracle(n, True, False)
    if n >= 63:
        assert ref["final_mask"].any() and not ref["final_mask"].all()


@pytest.mark.parametrize("natural,sab", bj.RULES)
@pytest.mark.parametrize("n", [257, 2049])
def test_philox_all_rule_settings_equal_oracle(n, natural, sab):
    ref = _rollout_against_oracle(n, natural, sab)
    assert {-1.0, 0.0, 1.0} <= set(np.unique(ref["reward"])) and ref["actions"].min() == 0 and ref["actions"].max() == 1
    if n == 2049:
        assert (1.5 in ref["reward"]) == (natural and not sab)


def _count_late_draws(n, base_seed, t, start):
    """Dealer draws per table by the model's rule over the step's card stream (draw j < 4 is stream card j, draw j >= 4 stream card j + 4)."""
    from oracle.oracle import _p, lib

    cards = np.zeros((n, 24), np.int8)
    lib().orc_bj_stream_cards(n, base_seed, t, 24, _p(cards))
    draws = np.zeros(n, np.int64)
    for i in range(n):
        hand, j = list(start), 0
        while bj.sum_hand(hand) < 17:
            hand.append(int(cards[i, j if j < 4 else j + 4]))
            j += 1
        draws[i] = j
    return draws


@pytest.mark.parametrize("start", [(1, 1), (2, 2)])
def test_forced_late_draws_equal_oracle(start):
    """Every dealer at (A, A) resp. (2, 2), every table sticks: hundreds of dealers draw a fifth card and dozens a sixth, through the
    out-of-line late_draw, at steps 2^32 - 2 .. 2^32 + 1 and env_offset 2^34 (both words of the draw counter, seeds past 2^34)."""
    import torch
    from gym_amd import _native
    from oracle.oracle import OracleBlackjack

    n, seed, off = 20_000, 3, 1 << 34
    player = [10, 9]
    h = _native.Blackjack(n, natural=True, sab=False, seed=seed, action_seed=5, env_offset=off)
    orc = OracleBlackjack(n, natural=True, sab=False, seed=seed, action_seed=5, env_offset=off)
    state0 = np.full(n, bj.pack_hands(player, list(start)), np.int32)
    actions = torch.zeros(n, dtype=torch.int64, device=_dev())
    five = six = 0
    for t in range((1 << 32) - 2, (1 << 32) + 2):
        draws = _count_late_draws(n, seed + off, t, start)
        five, six = five + int((draws >= 5).sum()), six + int((draws >= 6).sum())
        h.set_state(state0, np.zeros(n, np.int32), t=t, r=1)
        _set_oracle_hands(orc, player, list(start))
        orc.elapsed[:] = 0
        orc.t = t
        b = _bufs(n)
        torch.cuda.synchronize()
        h.step(actions, b["obs"], b["reward"], b["terminated"], b["truncated"], b["final_obs"])
        h.sync()
        got = _np(b)
        ref = {k: v[None] for k, v in orc.step(np.zeros(n, np.int64)).items()}
        _assert_equals_oracle({k: v[None] for k, v in got.items()}, ref, sampled=False, what=(start, t))
        late = draws >= 5
        assert np.array_equal(got["reward"][late], ref["reward"][0][late]) and len(set(ref["reward"][0][late])) == 3
        st, el = h.get_state()
        assert np.array_equal(st, _oracle_words(orc)) and not el.any() and h.get_counters() == (t + 1, 1)
    h.close()
    assert five >= 100 and six >= 5, (five, six)          # over the four steps: 463 and 26 from (A, A), 561 and 37 from (2, 2)


@pytest.mark.parametrize("per_env", [False, True])
@pytest.mark.parametrize("t0", [61, T_WRAP])
def test_counters_one_launch_seven_launches_and_tape(t0, per_env):
    """K = 7 sampled from t == 29 (mod 32): the action word changes inside the launch (and, from 2^32 - 3, the step counter's low word wraps),
    at env_offset 2^34 + 4092 (the high word of the action counter; 2^34 + 4093 is no multiple of MXV_ENV_ALIGN and must be refused), with
    the draw streams keyed by base seed + env or by per-env seeds."""
    from gym_amd import _native

    n, K = 257, 7
    assert t0 % 32 == 29 and BIG_OFFSET % 4 == 0
    with pytest.raises(Exception):           # the one env_offset rule: multiples of MXV_ENV_ALIGN = 4 (Philox action groups of four tables)
        _native.Blackjack(n, env_offset=BIG_OFFSET + 1)
    kw = dict(natural=True, sab=False, seed=21, action_seed=22, env_offset=BIG_OFFSET, t0=t0, per_env_seeds=_seeds(n) if per_env else None,
              max_episode_steps=4)
    h, orc = _pair(n, **kw)
    fused, (st, el), ctr = _device_rollout(h, n, K)
    h.close()
    ref = _oracle_rollout(orc, K)
    _assert_equals_oracle(fused, ref, what=("fused", t0, per_env))
    assert np.array_equal(st, _oracle_words(orc)) and np.array_equal(el, orc.elapsed) and ctr == (t0 + K, 1)
    assert ref["truncated"].any() and ref["terminated"].any() and 0 < ref["actions"].mean() < 1
    if per_env:                              # the per-env seeds key the draws: the same run under base seed + env deals other cards
        h2, _ = _pair(n, **dict(kw, per_env_seeds=None))
        other, _, _ = _device_rollout(h2, n, K)
        h2.close()
        assert np.array_equal(other["actions"], fused["actions"]) and not np.array_equal(other["obs"], fused["obs"])
    for mode in ("single", "tape"):
        h, _ = _pair(n, **kw)
        got, (st2, el2), ctr2 = _device_rollout(h, n, K, single=mode == "single", tape=fused["actions"] if mode == "tape" else None)
        h.close()
        for k in fused:
            if not (mode == "tape" and k == "actions"):
                assert np.array_equal(got[k], fused[k]), (mode, k)
        assert np.array_equal(st2, st) and np.array_equal(el2, el) and ctr2 == ctr


@pytest.mark.parametrize("tape", [False, True])
@pytest.mark.parametrize("n", [257, 4099])
def test_compact_outputs_equal_oracle(n, tape):
    """mxv_bj_rollout_compact against the oracle itself: int32 / float32 outputs, the natural rule's 1.5, TimeLimit 3."""
    K = 12
    h, orc = _pair(n, natural=True, sab=False, seed=8, action_seed=9, max_episode_steps=3)
    tp = np.random.default_rng(3).integers(0, 2, (K, n)).astype(np.int64) if tape else None
    got, (st, el), ctr = _device_rollout(h, n, K, compact=True, tape=tp)
    h.close()
    assert got["obs"].dtype == got["final_obs"].dtype == got["actions"].dtype == np.int32 and got["reward"].dtype == np.float32
    ref = _oracle_rollout(orc, K, tp)
    _assert_equals_oracle(got, ref, sampled=not tape, what=(n, tape))
    if tape:
        assert np.all(got["actions"] == I_SENT)
    assert np.array_equal(st, _oracle_words(orc)) and np.array_equal(el, orc.elapsed) and ctr == (K, 1)
    assert 1.5 in got["reward"] and got["truncated"].any() and got["terminated"].any()


@pytest.mark.parametrize("compact", [False, True])
def test_absent_outputs_leave_the_rest_unchanged(compact):
    n, K = 257, 5
    kw = dict(natural=True, sab=False, seed=31, action_seed=32, max_episode_steps=3)
    h, orc = _pair(n, **kw)
    full, (st, el), ctr = _device_rollout(h, n, K, compact=compact)
    h.close()
    _assert_equals_oracle(full, _oracle_rollout(orc, K), what="all outputs")
    for gone in ("reward", "terminated", "truncated", "final_obs", "actions"):
        h, _ = _pair(n, **kw)
        got, (st2, el2), ctr2 = _device_rollout(h, n, K, compact=compact, absent=(gone,))
        h.close()
        for k in full:
            if k == gone:
                sent = U8_SENT if got[k].dtype == np.uint8 else I_SENT
                assert np.all(got[k] == sent), (gone, "written though absent")
            else:
                assert np.array_equal(got[k], full[k]), (gone, k)
        assert np.array_equal(st2, st) and np.array_equal(el2, el) and ctr2 == ctr


@pytest.mark.parametrize("compact", [False, True])
def test_nothing_is_written_outside_the_output_views(compact):
    """Every output a [K, (3,) n] view into a larger sentinel-filled buffer, 1024 guard elements (1021 for the byte flags) on either side."""
    import torch

    n, K = 257, 5
    kw = dict(natural=True, sab=False, seed=31, action_seed=32, max_episode_steps=3)
    h, orc = _pair(n, **kw)
    it, ft = (torch.int32, torch.float32) if compact else (torch.int64, torch.float64)
    spec = dict(obs=(it, (K, 3, n), 1024, I_SENT), final_obs=(it, (K, 3, n), 1024, I_SENT), actions=(it, (K, n), 1024, I_SENT),
                reward=(ft, (K, n), 1024, I_SENT), terminated=(torch.uint8, (K, n), 1021, U8_SENT), truncated=(torch.uint8, (K, n), 1021, U8_SENT))
    whole, view = {}, {}
    for k, (dt, shape, pad, sent) in spec.items():
        size = int(np.prod(shape))
        whole[k] = torch.full((size + 2 * pad,), sent, dtype=dt, device=_dev())
        view[k] = whole[k][pad:pad + size].view(shape)
    torch.cuda.synchronize()
    h.rollout(K, view["obs"], view["reward"], view["terminated"], view["truncated"], view["final_obs"], view["actions"], per_step=True, compact=compact)
    h.sync()
    h.close()
    ref = _oracle_rollout(orc, K)
    _assert_equals_oracle(_np(view), ref, what="views")
    assert not ref["final_mask"].all() and ref["final_mask"].any()
    for k, (dt, shape, pad, sent) in spec.items():
        w = whole[k].cpu().numpy()
        assert np.all(w[:pad] == sent) and np.all(w[-pad:] == sent), (k, "guard overwritten")


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("n", [3001, 30_001])
def test_host_path_both_sides_of_the_staging_threshold(n, stats):
    """reset_host / step_host: the pinned, device-mapped block (it fits 2 MiB up to about 23 000 tables) and the staged copies, six steps of
    given actions against the oracle, with the fused episode statistics off and on."""
    from gym_amd import _native
    from oracle.oracle import OracleBlackjack

    assert 90 * 3001 + 256 < (2 << 20) < 90 * 30_001
    h = _native.Blackjack(n, natural=True, sab=False, max_episode_steps=3, seed=41, action_seed=42)
    orc = OracleBlackjack(n, natural=True, sab=False, max_episode_steps=3, seed=41, action_seed=42)
    if stats:
        h.episode_stats(True)
    assert np.array_equal(h.reset_host(), orc.reset())
    rng = np.random.default_rng(6)
    acc, length, episodes = np.zeros(n, np.float32), np.zeros(n, np.int32), 0
    for k in range(6):
        a = rng.integers(0, 2, n).astype(np.int64)
        obs, rew, term, trunc, fin = h.step_host(a)
        o = orc.step(a)
        assert np.array_equal(obs, o["obs"]) and np.array_equal(rew, o["reward"]), k
        assert np.array_equal(term, o["terminated"]) and np.array_equal(trunc, o["truncated"]), k
        m = o["final_mask"]
        assert np.array_equal(fin[:, m], o["final_obs"][:, m]), k
        acc, length = (acc + o["reward"]).astype(np.float32), length + 1
        if stats:
            er, el_, run = h.episode_stats_host(want_running=True)
            assert np.array_equal(er[m], acc[m]) and np.array_equal(el_[m], length[m]), k
            acc, length = np.where(m, np.float32(0), acc), np.where(m, 0, length).astype(np.int32)
            assert np.array_equal(run, acc), k
        else:
            acc, length = np.where(m, np.float32(0), acc), np.where(m, 0, length).astype(np.int32)
        episodes += int(m.sum())
    st, el = h.get_state()
    assert np.array_equal(st, _oracle_words(orc)) and np.array_equal(el, orc.elapsed) and np.array_equal(el, length) and h.get_counters() == (6, 1)
    assert episodes > n
    if not stats:
        with pytest.raises(Exception):
            h.episode_stats_host()
    h.close()


# ---- bj_reset_kernel --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_env", [False, True])
@pytest.mark.parametrize("n", SMALL + [2049, 4097])
def test_philox_reset_equals_oracle(n, per_env):
    """Three resets in a row (r = 1, 2, 3) at a nonzero step index, through the device-pointer call."""
    import torch
    from gym_amd import _native
    from oracle.oracle import OracleBlackjack

    t0 = (1 << 32) + 5
    h = _native.Blackjack(n, sab=True, seed=51, action_seed=52, env_offset=BIG_OFFSET)
    orc = OracleBlackjack(n, sab=True, seed=51, action_seed=52, env_offset=BIG_OFFSET)
    if per_env:
        h.seed(51, _seeds(n), 52)
        orc.seeds = _seeds(n)
    h.set_state(np.zeros(n, np.int32), np.full(n, 9, np.int32), t=t0, r=0)
    orc.t = t0
    seen = []
    for r in (1, 2, 3):
        obs = torch.full((3, n), I_SENT, dtype=torch.int64, device=_dev())
        torch.cuda.synchronize()
        h.reset(obs)
        h.sync()
        want = orc.reset()
        assert orc.r == r and h.get_counters() == (t0, r)
        assert np.array_equal(obs.cpu().numpy(), want), r
        st, el = h.get_state()
        assert np.array_equal(st, _oracle_words(orc)) and not el.any(), r
        seen.append(st)
    if n >= 63:
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    h.close()


def test_injected_reset_over_every_deal():
    import torch
    from gym_amd import _native

    n = 10_000
    deal = bj.deals_of(np.arange(n))
    h = _native.Blackjack(n, sab=True)
    obs = torch.full((3, n), I_SENT, dtype=torch.int64, device=_dev())
    cards = _t(deal)
    torch.cuda.synchronize()
    h.reset(obs, cards_dev=cards)
    h.sync()
    st, el = h.get_state()
    assert np.array_equal(obs.cpu().numpy(), bj.obs_of_deal(deal)) and np.array_equal(st, bj.pack_deal(deal)) and not el.any()
    assert np.array_equal(h.reset_host(deal), bj.obs_of_deal(deal)) and h.get_counters() == (0, 2)
    h.close()


@pytest.mark.parametrize("which", ["third", "none", "all"])
def test_masked_reset_equals_oracle_merged_by_the_mask(which):
    """Masked-out tables keep state, counter and running return, and their obs row is their current hand; masked-in tables are the oracle's
    reset; ep_acc is zeroed only where masked in."""
    import torch

    n, K = 1031, 3
    h, orc = _pair(n, natural=False, sab=True, seed=61, action_seed=62)
    h.episode_stats(True)
    got, (st0, el0), _ = _device_rollout(h, n, K)
    ref = _oracle_rollout(orc, K)
    _assert_equals_oracle(got, ref, what="before the reset")
    assert np.array_equal(st0, _oracle_words(orc)) and np.array_equal(el0, orc.elapsed) and el0.any()
    running = (np.arange(n) % 7 - 3).astype(np.float32) * np.float32(0.5) + np.float32(8)
    h.set_running_returns(running)
    cur_obs = ref["obs"][-1]
    mask = dict(third=np.arange(n) % 3 == 0, none=np.zeros(n, bool), all=np.ones(n, bool))[which]
    obs = torch.full((3, n), I_SENT, dtype=torch.int64, device=_dev())
    mask_dev = _t(mask.astype(np.uint8))
    torch.cuda.synchronize()
    h.reset(obs, mask_dev=mask_dev)
    h.sync()
    fresh = orc.reset()                      # the oracle resets every table: merge by the mask
    assert orc.r == 2 and h.get_counters() == (K, 2)
    st, el = h.get_state()
    assert np.array_equal(obs.cpu().numpy(), np.where(mask[None, :], fresh, cur_obs))
    assert np.array_equal(st, np.where(mask, _oracle_words(orc), st0)) and np.array_equal(el, np.where(mask, 0, el0))
    assert np.array_equal(h.episode_stats_host(want_running=True)[2], np.where(mask, np.float32(0), running))
    h.close()
