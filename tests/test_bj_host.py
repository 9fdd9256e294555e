"""The literal Blackjack model of tests/bj_host.py against the two independent witnesses the suite has: the C oracle (oracle/tabular.c)
on the exhaustive products the GPU tests use, and the reference's own recorded games (tests/golden/blackjack_*.npz).  Everything is an
integer or one of -1, 0, 1, 1.5: every comparison is exact."""
import numpy as np
import pytest

import bj_host as bj
from helpers import BLACKJACK_CASES, replay_blackjack
from oracle.oracle import OracleBlackjack


def set_hands(arr, hands):
    """Write card lists into an OracleBlackjack hand array: each row is int[33] = 32 cards, then the count."""
    arr[:] = 0
    for i, h in enumerate(hands):
        arr[i, :len(h)] = h
        arr[i, 32] = len(h)


def set_hand_all(arr, hand):
    arr[:] = 0
    arr[:, :len(hand)] = hand
    arr[:, 32] = len(hand)


def hands_of(arr):
    return [list(map(int, r[:r[32]])) for r in arr]


def test_enumeration_counts():
    comp = bj.dealer_completions()
    assert len(comp) == 54_433 and len(set(comp)) == 54_433
    assert max(len(c) for c in comp) == 12 and min(len(c) for c in comp) == 2
    assert all(bj.sum_hand(c) >= 17 and (len(c) == 2 or bj.sum_hand(c[:-1]) < 17) for c in comp)
    assert len({c[:2] for c in comp}) == 100
    reps = bj.player_representatives()
    assert len(reps) == 62 and all(bj.player_key(h) == k and not bj.is_bust(h) for k, h in reps.items())
    assert sum(k[2] for k in reps) == 27            # two-card states: 17 without an ace, 10 with one
    ct = bj.completion_table()
    assert int(ct["ndraws"].max()) == 10 and np.array_equal(ct["ndraws"], [len(c) - 2 for c in comp])


def test_packing_round_trips():
    for k, h in bj.player_representatives().items():
        for d in ([1, 1], [10, 1], [5, 6], [10, 10]):
            u = bj.unpack(bj.pack_hands(h, d))
            assert (int(u["p_sum"]), int(u["p_ace"]), int(u["p_two"])) == k
            assert (int(u["d_sum"]), int(u["d_ace"]), int(u["d_two"]), int(u["dfirst"])) == (*bj.player_key(d), d[0])
    deal = bj.deals_of(np.arange(10000))
    assert len({tuple(r) for r in deal}) == 10000 and deal.min() == 1 and deal.max() == 10
    assert np.array_equal(bj.pack_deal(deal), [bj.pack_hands([c, d], [a, b]) for a, b, c, d in deal.tolist()])
    t = bj.Table()
    assert np.array_equal(bj.obs_of_deal(deal[:300]).T, [t.deal(r) for r in deal[:300]])
    rows = bj.injected_rows([[], [3], [1, 2, 3]], [[1, 2, 3, 4]] * 3)
    assert rows.shape == (3, 24) and rows[0, :5].tolist() == [1, 2, 3, 4, 0] and rows[2, :8].tolist() == [1, 2, 3, 1, 2, 3, 4, 0]


class _ModelAdapter:
    def __init__(self, n, natural, sab):
        self.tables = [bj.Table(natural, sab) for _ in range(n)]

    def reset(self, cards):
        return np.array([t.deal(c) for t, c in zip(self.tables, cards)], np.int64).T

    def step(self, actions, cards):
        outs = [t.step(int(a), c) for t, a, c in zip(self.tables, actions, cards)]
        n = len(outs)
        fin = np.zeros((3, n), np.int64)
        for i, o in enumerate(outs):
            if o["final_obs"] is not None:
                fin[:, i] = o["final_obs"]
        self.used = np.array([o["used"] for o in outs])
        return dict(obs=np.array([o["obs"] for o in outs], np.int64).T, reward=np.array([o["reward"] for o in outs]),
                    terminated=np.array([o["terminated"] for o in outs]), truncated=np.array([o["truncated"] for o in outs]), final_obs=fin)


@pytest.mark.parametrize("tag", BLACKJACK_CASES)
def test_model_replays_reference_games_exactly(tag):
    ndone, g = replay_blackjack(tag, _ModelAdapter)
    assert ndone == int(g["final_mask"].sum()) > 1000


def test_model_consumes_the_cards_the_reference_consumed():
    g = np.load(f"{__import__('helpers').GOLDEN}/blackjack_natural.npz")
    eng = _ModelAdapter(g["actions"].shape[1], True, False)
    eng.reset(g["cards0"])
    for t in range(g["actions"].shape[0]):
        eng.step(g["actions"][t], g["cards"][t])
        assert np.array_equal(eng.used, g["ncards"][t]), t


@pytest.mark.parametrize("natural,sab", bj.RULES)
def test_model_equals_oracle_on_the_stick_product(natural, sab):
    """62 player states x 54 433 dealer completions, one oracle call per player state."""
    comp, ct, reps = bj.dealer_completions(), bj.completion_table(), bj.player_representatives()
    C = len(comp)
    table = bj.reward_table(natural, sab)
    ps = bj.summarise(reps.values())
    orc = OracleBlackjack(C, natural=natural, sab=sab)
    starts = [c[:2] for c in comp]
    lanes = seen_15 = 0
    for j, hand in enumerate(reps.values()):
        deal = bj.deals_of(np.arange(C) * 7 + j * 1009)
        set_hands(orc.dealer, starts)
        set_hand_all(orc.player, hand)
        orc.elapsed[:] = 0
        out = orc.step(np.zeros(C, np.int64), bj.stick_rows(deal))
        want = table[ps["score"][j], ps["natural"][j], ct["score"], ct["natural"]]
        assert np.array_equal(out["reward"], want), hand
        assert out["terminated"].all() and not out["truncated"].any() and out["final_mask"].all()
        assert np.array_equal(out["final_obs"], np.stack([np.full(C, ps["total"][j]), ct["first"], np.full(C, ps["usable"][j])]))
        assert np.array_equal(out["obs"], bj.obs_of_deal(deal))
        assert np.array_equal(orc.dealer[:, [0, 1, 32]], np.c_[deal[:, :2], np.full(C, 2)])
        assert np.array_equal(orc.player[:, [0, 1, 32]], np.c_[deal[:, 2:], np.full(C, 2)])
        lanes += C
        seen_15 += int((want == 1.5).sum())
    assert lanes == 62 * 54_433
    assert (seen_15 > 0) == (natural and not sab)
    # the broadcast is the per-table model: spot lanes through Table.step itself
    rng = np.random.default_rng(5)
    hands = list(reps.values())
    for j, i in zip(rng.integers(0, 62, 400), rng.integers(0, C, 400)):
        t = bj.Table(natural, sab)
        t.player, t.dealer = list(hands[j]), list(comp[i][:2])
        o = t.step(0, list(comp[i][2:]) + [1, 2, 3, 4])
        assert o["reward"] == table[ps["score"][j], ps["natural"][j], ct["score"][i], ct["natural"][i]] and o["used"] == ct["ndraws"][i] + 4
        assert o["final_obs"] == (ps["total"][j], comp[i][0], ps["usable"][j]) and t.dealer == [1, 2] and t.player == [3, 4]


@pytest.mark.parametrize("natural,sab", bj.RULES)
def test_model_equals_oracle_on_the_hit_product(natural, sab):
    reps = bj.player_representatives()
    hands = [h for h in reps.values() for _ in bj.CARDS]
    cards = [c for _ in reps for c in bj.CARDS]
    n = len(hands)
    assert n == 620
    dealers = [[1 + i % 10, 1 + (i // 10) % 10] for i in range(n)]
    deal = bj.deals_of(np.arange(n) * 17 + 3)
    orc = OracleBlackjack(n, natural=natural, sab=sab)
    set_hands(orc.player, hands)
    set_hands(orc.dealer, dealers)
    out = orc.step(np.ones(n, np.int64), bj.injected_rows([[c] for c in cards], deal))
    nbust = 0
    for i in range(n):
        t = bj.Table(natural, sab)
        t.player, t.dealer = list(hands[i]), list(dealers[i])
        o = t.step(1, [cards[i]] + deal[i].tolist())
        assert (o["reward"], o["terminated"], o["truncated"]) == (out["reward"][i], out["terminated"][i], out["truncated"][i])
        assert o["obs"] == tuple(out["obs"][:, i]) and (o["final_obs"] is not None) == out["final_mask"][i]
        if o["terminated"]:
            assert o["final_obs"] == tuple(out["final_obs"][:, i]) and o["reward"] == -1.0
            nbust += 1
        assert [t.player, t.dealer] == [hands_of(orc.player[i:i + 1])[0], hands_of(orc.dealer[i:i + 1])[0]]
        assert t.elapsed == orc.elapsed[i]
    assert 100 < nbust < 400


@pytest.mark.parametrize("action", [0, 1])
def test_model_equals_oracle_on_every_deal(action):
    """All 10^4 four-card deals after a terminating step: a bust (hard 20 draws a ten) and a stick (dealer stands on 20)."""
    n = 10_000
    deal = bj.deals_of(np.arange(n))
    orc = OracleBlackjack(n, natural=True, sab=False)
    set_hand_all(orc.player, [10, 6, 4])
    set_hand_all(orc.dealer, [10, 10])
    out = orc.step(np.full(n, action, np.int64), bj.injected_rows([[10]] * n if action else [[]] * n, deal))
    assert out["terminated"].all() and np.all(out["reward"] == (-1.0 if action else 0.0))
    assert np.array_equal(out["obs"], bj.obs_of_deal(deal))
    t = bj.Table(True, False)
    for i in range(0, n, 7):
        t.player, t.dealer = [10, 6, 4], [10, 10]
        o = t.step(action, ([10] if action else []) + deal[i].tolist())
        assert o["obs"] == tuple(out["obs"][:, i]) and o["final_obs"] == tuple(out["final_obs"][:, i]) == ((30 if action else 20), 10, 0)
    got = np.array([bj.pack_hands(p, d) for p, d in zip(hands_of(orc.player), hands_of(orc.dealer))], np.int32)
    assert np.array_equal(got, bj.pack_deal(deal)) and not orc.elapsed.any()


@pytest.mark.parametrize("limit", [1, 2, 3, -1])
def test_model_time_limit_equals_oracle(limit):
    cases = [(el, kind) for el in (0, 1, 2) for kind in ("hit", "bust", "stick")]
    n = len(cases)
    orc = OracleBlackjack(n, sab=True, max_episode_steps=limit)
    set_hand_all(orc.player, [5, 4, 3])
    set_hand_all(orc.dealer, [10, 9])
    orc.elapsed[:] = [el for el, _ in cases]
    rows = bj.injected_rows([{"hit": [2], "bust": [10], "stick": []}[k] for _, k in cases], [[2, 3, 4, 5]] * n)
    out = orc.step(np.array([k != "stick" for _, k in cases], np.int64), rows)
    for i, (el, kind) in enumerate(cases):
        t = bj.Table(False, True, limit)
        t.player, t.dealer, t.elapsed = [5, 4, 3], [10, 9], el
        o = t.step(int(kind != "stick"), rows[i])
        assert (o["terminated"], o["truncated"], o["reward"]) == (out["terminated"][i], out["truncated"][i], out["reward"][i])
        assert o["truncated"] == (limit > 0 and el + 1 >= limit) and o["terminated"] == (kind != "hit")
        assert t.elapsed == orc.elapsed[i] == (0 if o["terminated"] or o["truncated"] else el + 1)
        if o["final_obs"] is not None:
            assert o["final_obs"] == tuple(out["final_obs"][:, i]) == ({"hit": 14, "bust": 22, "stick": 12}[kind], 10, 0)
