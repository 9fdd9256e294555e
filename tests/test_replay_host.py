"""tests/replay_host.py, the NumPy twin of include/mxv_replay.h, held on the CPU: against a literal buffer written row by row from the
prose of the rule, against Random123's known answers for the Philox under tag 9, and — the draw's uniformity — against a chi-square
bar.  The device is held to the twin bit for bit (tests/test_gpu_replay.py), so no large draw runs on the GPU."""
import numpy as np
import pytest

import replay_host as rh
from oracle import oracle
from test_philox import KATS


class LiteralBuffer:
    """A ring written one row at a time with Python integers: no vector operation, no np.roll."""

    def __init__(self, C, W):
        self.C, self.W = C, W
        self.obs = [[0] * W for _ in range(C)]
        self.next = [[0] * W for _ in range(C)]
        self.action, self.reward, self.term = [0] * C, [0] * C, [0] * C

    def insert(self, count, first_obs, obs, actions, reward, terminated, truncated=None, final_obs=None):
        K, N = len(obs), len(first_obs)
        for t in range(K):
            for i in range(N):
                r = t * N + i
                s = (count + r) % self.C                  # Python integers: exact at any count
                pre = first_obs[i] if t == 0 else obs[t - 1][i]
                done = terminated[t][i] != 0 or (truncated is not None and truncated[t][i] != 0)
                nxt = final_obs[t][i] if (done and final_obs is not None) else obs[t][i]
                self.obs[s] = [int(x) for x in np.asarray(pre).reshape(-1).view(np.uint32)]
                self.next[s] = [int(x) for x in np.asarray(nxt).reshape(-1).view(np.uint32)]
                self.action[s] = int(actions[t][i]) & 0xFFFFFFFF
                rew = reward[t][i]
                if isinstance(rew, np.float32):
                    self.reward[s] = int(np.array(rew, np.float32).view(np.uint32))
                else:
                    f = np.float32(rew)
                    self.reward[s] = 0x7FC00000 if np.isnan(f) else int(np.array(f, np.float32).view(np.uint32))
                self.term[s] = 1 if terminated[t][i] != 0 else 0
        return count + K * N


def _chunk(rng, K, N, W, reward_dtype, action_dtype, with_final):
    obs = rng.integers(0, 1 << 32, size=(K, N, W), dtype=np.uint64).astype(np.uint32)
    first = rng.integers(0, 1 << 32, size=(N, W), dtype=np.uint64).astype(np.uint32)
    final = rng.integers(0, 1 << 32, size=(K, N, W), dtype=np.uint64).astype(np.uint32) if with_final else None
    actions = rng.integers(-5, 5, size=(K, N)).astype(action_dtype)
    reward = (rng.standard_normal((K, N)) * 1e3).astype(reward_dtype)
    reward.reshape(-1)[::7] = np.nan
    reward.reshape(-1)[3::11] = np.inf
    if reward_dtype == np.float64:
        reward.reshape(-1)[5::13] = 1.0 + 2.0 ** -24           # a tie: rounds to even
        reward.reshape(-1)[6::13] = 1.0 + 3 * 2.0 ** -24
    term = (rng.random((K, N)) < 0.2).astype(np.uint8) * rng.integers(1, 255, size=(K, N)).astype(np.uint8)
    trunc = (rng.random((K, N)) < 0.2).astype(np.uint8) if with_final else None
    return first, obs, actions, reward, term, trunc, final


@pytest.mark.parametrize("start", [0, (1 << 32) - 3, None])
@pytest.mark.parametrize("C,W,K,N", [(5, 1, 1, 1), (5, 3, 1, 5), (64, 4, 3, 5), (257, 2, 4, 64), (257, 9, 1, 257), (1025, 6, 2, 257)])
def test_the_twin_equals_a_literal_buffer_over_inserts_that_wrap_the_ring(C, W, K, N, start):
    """Sequences of inserts that wrap the ring several times; count starting at 0, at 2^32 - 3 and at 2^63 - R (the last insert ends at
    2^63 exactly: the 64-bit mod)."""
    rng = np.random.default_rng(C * 1000 + W)
    R = K * N
    rounds = max(3, (3 * C) // R + 1) if R * 40 >= C else 5
    count = (1 << 63) - R * rounds if start is None else start
    twin, lit = rh.Ring(C, W), LiteralBuffer(C, W)
    c_twin = c_lit = count
    for n in range(rounds):
        with_final = n % 2 == 0
        first, obs, actions, reward, term, trunc, final = _chunk(rng, K, N, W, (np.float64, np.float32)[n % 2], (np.int64, np.int32)[n % 2], with_final)
        c_twin = rh.insert(twin, c_twin, first, obs, actions, reward, term, trunc, final)
        c_lit = lit.insert(c_lit, first, obs, actions, reward, term, trunc, final)
    assert c_twin == c_lit == count + rounds * R
    assert np.array_equal(twin.obs, np.array(lit.obs, np.uint32)) and np.array_equal(twin.next, np.array(lit.next, np.uint32))
    assert np.array_equal(twin.action, np.array(lit.action, np.uint32)) and np.array_equal(twin.reward, np.array(lit.reward, np.uint32))
    assert np.array_equal(twin.term, np.array(lit.term, np.uint8))


def test_the_slots_at_the_edges_of_the_64_bit_count():
    assert rh.slots((1 << 32) - 3, 5, 7).tolist() == [((1 << 32) - 3 + r) % 7 for r in range(5)]
    assert rh.slots((1 << 63) - 4, 4, 1 << 31).tolist() == [((1 << 63) - 4 + r) % (1 << 31) for r in range(4)]
    assert rh.slots(1 << 63, 3, 5).tolist() == [((1 << 63) + r) % 5 for r in range(3)]


def test_flat_add_is_the_same_insert_with_one_step():
    rng = np.random.default_rng(3)
    obs, nxt = rng.standard_normal((6, 4)).astype(np.float32), rng.standard_normal((1, 6, 4)).astype(np.float32)
    ring = rh.Ring(8, 4)
    assert rh.insert(ring, 5, obs, nxt, np.arange(6, dtype=np.int32)[None], np.ones((1, 6), np.float32), np.zeros((1, 6), np.uint8)) == 11
    s = [(5 + r) % 8 for r in range(6)]
    assert np.array_equal(ring.obs[s], obs.view(np.uint32)) and np.array_equal(ring.next[s], nxt[0].view(np.uint32))
    assert ring.action[s].tolist() == list(range(6)) and not ring.obs[[3, 4]].any()


def test_multiply_high_stays_below_n_at_the_largest_word():
    for n in (1, 5, 1 << 31):
        k = rh.multiply_high(np.array([0, 1, (1 << 31), (1 << 32) - 1], np.uint32), n)
        assert k.min() >= 0 and k.max() < n and int(k[-1]) == ((((1 << 32) - 1) * n) >> 32)
    assert rh.multiply_high(np.array([(1 << 32) - 1], np.uint32), 1 << 31)[0] == (1 << 31) - 1


def test_a_rows_draw_does_not_depend_on_the_batch_size():
    full = rh.draw(11, 4, 1000, 1025)
    for B in (1, 3, 63, 64, 65, 257):
        assert np.array_equal(rh.draw(11, 4, 1000, B), full[:B])
    assert not np.array_equal(rh.draw(11, 5, 1000, 64), full[:64]) and not np.array_equal(rh.draw(12, 4, 1000, 64), full[:64])
    assert (rh.draw(11, 4, 0, 7) == -1).all()


def test_philox_known_answers_and_the_tag_9_counter():
    for ctr, key, want in KATS:      # Random123's kat_vectors
        got = rh.philox4x32_10(*[np.array([c], np.uint32) for c in ctr], *key)
        assert tuple(int(x[0]) for x in got) == want
    # the counter of the rule: g = j >> 2 in words 0, 1; t in word 2 and the low 28 bits of word 3; 9 in its top four bits
    seed, t = 0x0123456789ABCDEF, (0xABCDEF12 << 32) | 0x3456789A
    J = np.array([0, 1, 2, 3, 4, 7, (1 << 34) + 5, (5 << 34) + 2], np.uint64)
    got = rh.words(seed, t, J)
    for j, w in zip(J.tolist(), got.tolist()):
        g = j >> 2
        ctr = (g & 0xFFFFFFFF, g >> 32, t & 0xFFFFFFFF, ((t >> 32) & 0x0FFFFFFF) | (9 << 28))
        assert ctr[3] >> 28 == rh.STREAM_REPLAY == 9
        assert w == int(oracle.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[j & 3])
    # a known answer of the whole draw, fixed when the rule was written: seed 0, step 0, the first eight words
    assert rh.words(0, 0, np.arange(8)).tolist() == [int(x) for x in oracle.philox4x32_10((0, 0, 0, 9 << 28), (0, 0))] + \
        [int(x) for x in oracle.philox4x32_10((1, 0, 0, 9 << 28), (0, 0))]
    assert rh.words(0, 0, np.arange(4)).tolist() == KNOWN_TAG_9


# Philox4x32-10(key = (0, 0), ctr = (0, 0, 0, 0x90000000)), computed with the oracle's and the twin's Philox, which both reproduce
# Random123's vectors above
KNOWN_TAG_9 = [0xD35B569A, 0x2F334C40, 0x7174516B, 0x9923E6AC]


@pytest.mark.parametrize("seed,t,n", [(0, 0, 1000), (1, 5, 1000), (12345, (1 << 33) + 7, 257), (7, 1, 4099), (3, 0, 5)])
def test_the_draw_is_uniform_over_the_live_slots(seed, t, n):
    """Pearson's chi-square over the n slots at B = 2^18 as a Wilson-Hilferty z-score stays below 4.75: a one-sided false alarm of about
    1e-6.  Measured when the rule was written: z = 0.37, 1.55, -0.90, -0.45, -0.76."""
    k = rh.draw(seed, t, n, 1 << 18)
    assert k.min() >= 0 and k.max() < n
    z = rh.chi_square_z(k, n)
    print(f"seed {seed} t {t} n {n}: z = {z:.2f}")
    assert z < 4.75


def test_sample_gathers_what_insert_stored_and_zeros_from_an_empty_ring():
    rng = np.random.default_rng(0)
    ring = rh.Ring(16, 3)
    first, obs, actions, reward, term, trunc, final = _chunk(rng, 2, 5, 3, np.float64, np.int64, True)
    count = rh.insert(ring, 0, first, obs, actions, reward, term, trunc, final)
    out = rh.sample(ring, count, 9, 2, 33, action_bytes=8)
    k = out["indices"]
    assert k.min() >= 0 and k.max() < 10 and np.array_equal(out["obs"], ring.obs[k]) and np.array_equal(out["next_obs"], ring.next[k])
    assert np.array_equal(out["actions"], actions.reshape(-1)[k]) and out["actions"].dtype == np.int64      # sign-extended back
    assert np.array_equal(out["reward"], ring.reward[k]) and np.array_equal(out["terminated"], ring.term[k])
    done = (term.reshape(-1) != 0) | (trunc.reshape(-1) != 0)
    want_next = np.where(done[:, None], final.reshape(10, 3), obs.reshape(10, 3))
    assert np.array_equal(ring.next[:10], want_next) and np.array_equal(ring.obs[:5], first) and np.array_equal(ring.obs[5:10], obs[0])
    empty = rh.sample(rh.Ring(4, 2, fill=0xAB), 0, 1, 0, 6)
    assert (empty["indices"] == -1).all() and not empty["obs"].any() and not empty["next_obs"].any() and not empty["actions"].any()
    assert not empty["reward"].any() and not empty["terminated"].any()
