"""A literal model of Blackjack-v1 (gym/envs/toy_text/blackjack.py under TimeLimit and SyncVectorEnv's autoreset) on card lists, and the
enumerations the exhaustive tests are built from.  Host-only, plain Python / NumPy; it takes nothing from the oracle (oracle/tabular.c)
and nothing from the kernel (gym_amd/csrc/mxv_bj.hip) except the bit layout of the packed state word, which the tests need to set and
read device state.

The per-table model (`Table`) is what the reference does, line for line.  The big products (62 player states x 54 433 dealer completions)
are not run through it lane by lane: the model is evaluated once per dealer completion and once per player hand (`summarise`), and the
outcome of a lane is looked up in a small table over (player score, player natural, dealer score, dealer natural) that `reward_table`
fills by calling the very rule function `Table.step` uses."""
import numpy as np

MAX_DRAWS = 24          # width of an injected-card row (OracleBlackjack.MAX_DRAWS, MXV_BJ_MAX_DRAWS)
CARDS = tuple(range(1, 11))
RULES = ((False, False), (False, True), (True, False), (True, True))     # (natural, sab)


# ---- blackjack.py:11-46, on card lists ---------------------------------------------------------------------------------------------------
def cmp(a, b):
    return float(a > b) - float(a < b)


def usable_ace(hand):
    return 1 in hand and sum(hand) + 10 <= 21


def sum_hand(hand):
    if usable_ace(hand):
        return sum(hand) + 10
    return sum(hand)


def is_bust(hand):
    return sum_hand(hand) > 21


def score(hand):
    return 0 if is_bust(hand) else sum_hand(hand)


def is_natural(hand):
    return sorted(hand) == [1, 10]


def settle(player_score, player_natural, dealer_score, dealer_natural, natural, sab):
    """The reward of a stick once the dealer has drawn (blackjack.py:147-158): cmp of the scores, then the Sutton-Barto rule, which takes
    precedence over the casino rule."""
    reward = cmp(player_score, dealer_score)
    if sab and player_natural and not dealer_natural:
        reward = 1.0
    elif not sab and natural and player_natural and reward == 1.0:
        reward = 1.5
    return reward


class Table:
    """One sub-env: BlackjackEnv.step (:133-162) under TimeLimit (time_limit.py:50-53) and the vector env's autoreset
    (sync_vector_env.py:152-156), dealt from a list of cards in the order the reference consumes them."""

    def __init__(self, natural=False, sab=False, max_episode_steps=-1):
        self.natural, self.sab, self.max_episode_steps = bool(natural), bool(sab), int(max_episode_steps)
        self.player, self.dealer, self.elapsed = [], [], 0

    def obs(self):
        return (sum_hand(self.player), self.dealer[0], int(usable_ace(self.player)))

    def deal(self, cards):
        """reset (:167-176): the dealer's two cards, then the player's two."""
        self.dealer = [int(cards[0]), int(cards[1])]
        self.player = [int(cards[2]), int(cards[3])]
        self.elapsed = 0
        return self.obs()

    def step(self, action, cards):
        """-> dict(obs, reward, terminated, truncated, final_obs (None unless the episode ended), used = cards consumed)."""
        cards = [int(c) for c in cards]
        used = 0
        assert action in (0, 1)
        if action:
            self.player.append(cards[used]); used += 1
            if is_bust(self.player):
                terminated, reward = True, -1.0
            else:
                terminated, reward = False, 0.0
        else:
            terminated = True
            while sum_hand(self.dealer) < 17:
                self.dealer.append(cards[used]); used += 1
            reward = settle(score(self.player), is_natural(self.player), score(self.dealer), is_natural(self.dealer), self.natural, self.sab)
        self.elapsed += 1
        truncated = self.max_episode_steps > 0 and self.elapsed >= self.max_episode_steps
        final_obs = None
        if terminated or truncated:
            final_obs = self.obs()
            self.deal(cards[used:used + 4])
            used += 4
        return dict(obs=self.obs(), reward=reward, terminated=terminated, truncated=truncated, final_obs=final_obs, used=used)


# ---- enumerations ------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def dealer_completions():
    """Every ordered two-card start extended card by card until sum_hand >= 17 (:145-146): a list of card tuples, the first two being the
    start.  54 433 of them; the longest holds 12 cards."""
    if "completions" not in _CACHE:
        out = []

        def grow(hand):
            if sum_hand(hand) >= 17:
                out.append(tuple(hand))
                return
            for c in CARDS:
                hand.append(c)
                grow(hand)
                hand.pop()

        for a in CARDS:
            for b in CARDS:
                grow([a, b])
        _CACHE["completions"] = out
    return _CACHE["completions"]


def player_key(hand):
    """What the dynamics can see of a player's hand: (raw sum with aces as 1, holds an ace, is still the two dealt cards)."""
    return (sum(hand), int(1 in hand), int(len(hand) == 2))


def player_representatives():
    """One hand per reachable packed player state, in the order of discovery: every two-card deal, then every hit from a hand that is not
    bust.  dict key -> card list; 62 keys."""
    if "players" not in _CACHE:
        reps, frontier = {}, [[a, b] for a in CARDS for b in CARDS]
        while frontier:
            nxt = []
            for hand in frontier:
                k = player_key(hand)
                if k in reps:
                    continue
                reps[k] = list(hand)
                nxt.extend(hand + [c] for c in CARDS if not is_bust(hand + [c]))
            frontier = nxt
        _CACHE["players"] = reps
    return _CACHE["players"]


def dealer_representative(raw_sum, ace, two):
    """A dealer hand with the given packed fields (for seeding the card-list oracle from a device state word)."""
    for a in CARDS:
        for b in CARDS:
            if two and player_key([a, b]) == (raw_sum, ace, 1):
                return [a, b]
            if not two:
                for c in CARDS:
                    if player_key([a, b, c]) == (raw_sum, ace, 0):
                        return [a, b, c]
    raise ValueError((raw_sum, ace, two))


# ---- the device's state word (bit layout at the top of gym_amd/csrc/mxv_bj.hip) --------------------------------------------------------------
def pack(p_sum, p_ace, p_two, dfirst, d_sum, d_ace, d_two):
    """bits 0-5 player sum | 6 player ace | 7 player has two cards | 8-11 dealer's first card | 12-17 dealer sum | 18 dealer ace |
    19 dealer has two cards.  Scalars or arrays."""
    return p_sum | (p_ace << 6) | (p_two << 7) | (dfirst << 8) | (d_sum << 12) | (d_ace << 18) | (d_two << 19)


def unpack(word):
    w = np.asarray(word).astype(np.int64)
    return dict(p_sum=w & 63, p_ace=(w >> 6) & 1, p_two=(w >> 7) & 1, dfirst=(w >> 8) & 15, d_sum=(w >> 12) & 63, d_ace=(w >> 18) & 1,
                d_two=(w >> 19) & 1)


def pack_hands(player, dealer):
    ps, pa, pt = player_key(player)
    ds, da, dt = player_key(dealer)
    return pack(ps, pa, pt, dealer[0], ds, da, dt)


def pack_deal(deal):
    """State words after a deal: deal int [n][4] = the dealer's two cards, then the player's two."""
    d = np.asarray(deal).astype(np.int64)
    ace = lambda a, b: ((a == 1) | (b == 1)).astype(np.int64)
    return pack(d[:, 2] + d[:, 3], ace(d[:, 2], d[:, 3]), 1, d[:, 0], d[:, 0] + d[:, 1], ace(d[:, 0], d[:, 1]), 1).astype(np.int32)


def obs_of_deal(deal):
    """Observations [3][n] after a deal, through the model's own sum_hand / usable_ace of every distinct player hand."""
    d = np.asarray(deal).astype(np.int64)
    tot, use = np.zeros((11, 11), np.int64), np.zeros((11, 11), np.int64)
    for a in CARDS:
        for b in CARDS:
            tot[a, b], use[a, b] = sum_hand([a, b]), usable_ace([a, b])
    return np.stack([tot[d[:, 2], d[:, 3]], d[:, 0], use[d[:, 2], d[:, 3]]])


def deals_of(index):
    """Four cards from a number: the base-10 digits of index mod 10^4, each + 1.  int8 [n][4]; 0..9999 covers all 10^4 deals."""
    i = np.asarray(index).astype(np.int64) % 10000
    return np.stack([i // 1000 % 10, i // 100 % 10, i // 10 % 10, i % 10], axis=1).astype(np.int8) + 1


def injected_rows(draws, deal):
    """Injected-card rows in the reference's consumption order: the step's draws (list of card sequences, one per lane), then the four
    dealt cards, zero-padded to MAX_DRAWS.  int8 [n][MAX_DRAWS]."""
    n = len(draws)
    rows = np.zeros((n, MAX_DRAWS), np.int8)
    deal = np.asarray(deal, dtype=np.int8).reshape(n, 4)
    for i, d in enumerate(draws):
        k = len(d)
        assert k + 4 <= MAX_DRAWS
        rows[i, :k] = d
        rows[i, k:k + 4] = deal[i]
    return rows


# ---- the model evaluated once per hand, broadcast over lanes -----------------------------------------------------------------------------------
def summarise(hands):
    """Per hand: the model's score, is_natural, sum_hand, usable_ace, first card, number of cards and the packed fields — int64 arrays."""
    f = dict(score=[], natural=[], total=[], usable=[], first=[], ncards=[], raw=[], ace=[], two=[])
    for h in hands:
        h = list(h)
        k = player_key(h)
        for name, v in (("score", score(h)), ("natural", is_natural(h)), ("total", sum_hand(h)), ("usable", usable_ace(h)), ("first", h[0]),
                        ("ncards", len(h)), ("raw", k[0]), ("ace", k[1]), ("two", k[2])):
            f[name].append(int(v))
    return {k: np.array(v, np.int64) for k, v in f.items()}


def reward_table(natural, sab):
    """settle() over every (player score 0..21, player natural, dealer score 0..21, dealer natural): float64 [22][2][22][2]."""
    t = np.zeros((22, 2, 22, 2))
    for ps in range(22):
        for pn in (0, 1):
            for ds in range(22):
                for dn in (0, 1):
                    t[ps, pn, ds, dn] = settle(ps, bool(pn), ds, bool(dn), natural, sab)
    return t


def completion_table():
    """The dealer completions as arrays: summarise() of the finished hands, `start` = packed (sum, ace) of the two-card start as a dealer
    state needs them, and `draws` int8 [C][10] (zero-padded) with `ndraws`."""
    if "ctable" not in _CACHE:
        comp = dealer_completions()
        s = summarise(comp)
        st = summarise([c[:2] for c in comp])
        draws = np.zeros((len(comp), 10), np.int8)
        for i, c in enumerate(comp):
            draws[i, :len(c) - 2] = c[2:]
        s.update(start_raw=st["raw"], start_ace=st["ace"], draws=draws, ndraws=s["ncards"] - 2)
        _CACHE["ctable"] = s
    return _CACHE["ctable"]


def stick_rows(deal):
    """Injected rows of a stick against every completion: the completion's draws, then deal [C][4]."""
    ct = completion_table()
    C = len(ct["ndraws"])
    rows = np.zeros((C, MAX_DRAWS), np.int8)
    rows[:, :10] = ct["draws"]
    deal = np.asarray(deal, dtype=np.int8).reshape(C, 4)
    col = ct["ndraws"][:, None] + np.arange(4)[None, :]
    rows[np.arange(C)[:, None], col] = deal
    return rows
