"""tests/nstep_host.py, the NumPy twin of include/mxv_nstep.h, held to references that share none of its code: a per-env, per-episode
Python model of the n-step return on random chunks, the one-step twin tests/replay_host.py at n = 1, every one of the 3^4 flag patterns
of a four-step chunk at n = 1..5, non-finite rewards behind an episode end, and gamma = 0 and 1.  No device needed."""
import itertools

import numpy as np
import pytest

import nstep_host as nh
import replay_host as rh


def chunk(rng, K, N, W, reward_dtype=np.float64, p_term=0.15, p_trunc=0.15, with_final=True):
    first = rng.integers(0, 1 << 32, size=(N, W), dtype=np.int64).astype(np.uint32)
    obs = rng.integers(0, 1 << 32, size=(K, N, W), dtype=np.int64).astype(np.uint32)
    final = rng.integers(0, 1 << 32, size=(K, N, W), dtype=np.int64).astype(np.uint32) if with_final else None
    actions = rng.integers(-3, 4, size=(K, N)).astype(np.int64)
    reward = (rng.standard_normal((K, N)) * 10).astype(reward_dtype)
    term = ((rng.random((K, N)) < p_term) * rng.integers(1, 256, size=(K, N))).astype(np.uint8)
    trunc = ((rng.random((K, N)) < p_trunc) * rng.integers(1, 256, size=(K, N))).astype(np.uint8) if with_final else None
    return first, obs, actions, reward, term, trunc, final


def episode_model(n, gamma, reward, term, trunc):
    """Per env, per episode: the column is cut into segments that end at a done step or at the chunk's end; inside a segment [a, b] the
    window of step t ends at min(t + n - 1, b) and its return is summed left to right in Python floats.  -> e, G, discount (float64)."""
    K, N = reward.shape
    e_out, G_out, d_out = np.zeros((K, N), np.int64), np.zeros((K, N)), np.zeros((K, N))
    for i in range(N):
        a = 0
        while a < K:
            b = a
            while b < K - 1 and not (term[b, i] or (trunc is not None and trunc[b, i])):
                b += 1
            for t in range(a, b + 1):
                e = min(t + n - 1, b)
                G, g = float(reward[t, i]), 1.0
                for k in range(t + 1, e + 1):
                    g = g * gamma
                    G = G + g * float(reward[k, i])
                e_out[t, i], G_out[t, i], d_out[t, i] = e, G, g * gamma
            a = b + 1
    return e_out, G_out, d_out


@pytest.mark.parametrize("n", (1, 2, 3, 5, 8, 64))
def test_the_twin_equals_a_per_episode_model_on_random_chunks(n):
    rng = np.random.default_rng(n)
    for K, N, gamma, dtype in ((1, 3, 0.99, np.float64), (7, 5, 0.9, np.float32), (12, 4, 0.997, np.float64), (70, 2, 0.5, np.float32)):
        first, obs, actions, reward, term, trunc, final = chunk(rng, K, N, 2, dtype)
        w = nh.windows(n, gamma, reward, term, trunc)
        e, G, d = episode_model(n, gamma, reward, term, trunc)
        assert np.array_equal(w["e"], e), (n, K)
        assert np.array_equal(w["G"].view(np.uint64), G.view(np.uint64)), (n, K)
        assert np.array_equal((w["g"] * gamma).view(np.uint64), d.view(np.uint64)), (n, K)
        ring = nh.Ring(K * N + 3, 2, fill=0xCACACACA)
        assert nh.insert(ring, 5, n, gamma, first, obs, actions, reward, term, trunc, final) == 5 + K * N
        s = rh.slots(5, K * N, ring.C)
        r = np.arange(K * N)
        t, i = r // N, r % N
        re = e.reshape(-1) * N + i
        done = (term.reshape(-1)[re] != 0) | (trunc.reshape(-1)[re] != 0)
        assert np.array_equal(ring.next[s], np.where(done[:, None], final.reshape(K * N, 2)[re], obs.reshape(K * N, 2)[re]))
        assert np.array_equal(ring.obs[s], np.where((t == 0)[:, None], first[i], obs.reshape(K * N, 2)[np.maximum(r - N, 0)]))
        assert np.array_equal(ring.reward[s].view(np.float32), G.reshape(-1).astype(np.float32))
        assert np.array_equal(ring.discount[s].view(np.float32), d.reshape(-1).astype(np.float32))
        assert np.array_equal(ring.term[s], (term.reshape(-1)[re] != 0).astype(np.uint8))
        assert np.array_equal(ring.action[s], rh.action_bits(actions))
        untouched = np.setdiff1d(np.arange(ring.C), s)
        assert (ring.discount[untouched] == 0xCACACACA).all() and (ring.term[untouched] == 0xCA).all()
        # the discount is gamma to the number of steps, by repeated multiplication
        steps = e - np.arange(K)[:, None] + 1
        assert steps.min() >= 1 and steps.max() <= min(n, K)
        assert np.allclose(d, gamma ** steps, rtol=1e-13)


@pytest.mark.parametrize("reward_dtype", (np.float32, np.float64))
def test_one_step_is_the_replay_twin_on_every_ring(reward_dtype):
    rng = np.random.default_rng(3)
    for with_final in (True, False):
        a, b = nh.Ring(50, 3, fill=7), rh.Ring(50, 3, fill=7)
        ca = cb = (1 << 32) - 9
        for _ in range(4):
            c = chunk(rng, 3, 7, 3, reward_dtype, with_final=with_final)
            flat = c[3].reshape(-1)
            flat[::5] = np.nan
            flat[1::7] = np.inf
            flat[2::11] = -np.inf
            flat[3::13] = -0.0
            ca = nh.insert(a, ca, 1, 0.97, *c)
            cb = rh.insert(b, cb, *c)
        assert ca == cb
        for x, y in zip(a.arrays()[:5], b.arrays()):
            assert np.array_equal(x, y)
        written = a.discount != 7
        assert written.sum() == 50 and (a.discount.view(np.float32) == np.float32(0.97)).all()


def test_every_flag_pattern_of_a_four_step_chunk():
    """K = 4, N = 1: 0 = running, 1 = terminated, 2 = truncated at each step; n = 1..5."""
    K, gamma = 4, 0.75      # powers of 0.75 and the sums below are exact in float64
    reward = np.array([[1.0], [2.0], [4.0], [8.0]])
    first = np.array([[100]], np.uint32)
    obs = np.array([[[10]], [[11]], [[12]], [[13]]], np.uint32)
    final = np.array([[[20]], [[21]], [[22]], [[23]]], np.uint32)
    cases = 0
    for pattern in itertools.product((0, 1, 2), repeat=K):
        term = np.array([[p == 1] for p in pattern], np.uint8)
        trunc = np.array([[p == 2] for p in pattern], np.uint8)
        for n in range(1, 6):
            ring = nh.Ring(K, 1)
            nh.insert(ring, 0, n, gamma, first, obs, np.zeros((K, 1), np.int32), reward, term, trunc, final)
            w = nh.windows(n, gamma, reward, term, trunc)
            for t in range(K):
                ends = [u for u in range(t, K) if pattern[u] != 0]
                e = min(t + n - 1, K - 1, ends[0] if ends else K)
                G = sum(0.75 ** (u - t) * float(reward[u, 0]) for u in range(t, e + 1))
                assert w["e"][t, 0] == e and w["G"][t, 0] == G, (pattern, n, t)
                assert ring.reward[t].view(np.float32) == np.float32(G) and ring.discount[t].view(np.float32) == np.float32(0.75 ** (e - t + 1))
                assert ring.term[t] == (1 if pattern[e] == 1 else 0), (pattern, n, t)
                assert ring.next[t, 0] == (20 + e if pattern[e] != 0 else 10 + e), (pattern, n, t)
                assert ring.obs[t, 0] == (100 if t == 0 else 9 + t)
                cases += 1
    assert cases == 81 * 5 * 4


def test_a_non_finite_reward_behind_an_episode_end_changes_no_earlier_row():
    rng = np.random.default_rng(5)
    K, N, n = 9, 6, 4
    first, obs, actions, reward, term, trunc, final = chunk(rng, K, N, 1, p_term=0.0, p_trunc=0.0)
    term[3, :3] = 1
    trunc[3, 3:] = 9
    clean = nh.Ring(K * N, 1)
    nh.insert(clean, 0, n, 0.9, first, obs, actions, reward, term, trunc, final)
    for poison in (np.nan, np.inf, -np.inf):
        dirty_reward = reward.copy()
        dirty_reward[4] = poison      # the first step of every env's next episode
        dirty = nh.Ring(K * N, 1)
        nh.insert(dirty, 0, n, 0.9, first, obs, actions, dirty_reward, term, trunc, final)
        rows = np.arange(4 * N)       # steps 0..3: their windows end at step 3 at the latest
        for x, y in zip(clean.arrays(), dirty.arrays()):
            assert np.array_equal(x[rows], y[rows])
        # inside a window the value propagates: rows of steps 1..4 of the second episode hold it or what it turns into
        later = dirty.reward[4 * N:5 * N].view(np.float32)
        assert (~np.isfinite(later)).all()
        if np.isnan(poison):
            assert (dirty.reward[4 * N:5 * N] == 0x7FC00000).all()
    # with a multiply in place of the branch, 0 * inf would have made those rows NaN: the twin's select keeps them finite
    assert np.isfinite(clean.reward.view(np.float32)).all()


def test_gamma_zero_and_one():
    rng = np.random.default_rng(8)
    K, N, n = 6, 4, 3
    first, obs, actions, reward, term, trunc, final = chunk(rng, K, N, 1, np.float32)
    w0, w1 = nh.windows(n, 0.0, reward, term, trunc), nh.windows(n, 1.0, reward, term, trunc)
    assert np.array_equal(w0["e"], w1["e"])
    assert np.array_equal(w0["G"], reward.astype(np.float64))      # 0 * finite = 0 adds nothing
    steps = w1["e"] - np.arange(K)[:, None] + 1
    for t in range(K):
        for i in range(N):
            G = float(reward[t, i])
            for u in range(t + 1, w1["e"][t, i] + 1):
                G = G + float(reward[u, i])
            assert w1["G"][t, i] == G
    a, b = nh.Ring(K * N, 1), nh.Ring(K * N, 1)
    nh.insert(a, 0, n, 0.0, first, obs, actions, reward, term, trunc, final)
    nh.insert(b, 0, n, 1.0, first, obs, actions, reward, term, trunc, final)
    assert (a.discount == 0).all() and (b.discount.view(np.float32) == 1.0).all()
    assert np.array_equal(a.next, b.next) and np.array_equal(a.term, b.term) and (steps > 1).any()


def test_gather_rule_and_classes():
    d = np.arange(10, 15, dtype=np.uint32)
    got = nh.gather(d, [0, 4, -1, 5, -2, 1 << 40, -(1 << 62)])
    assert got.dtype == np.uint32 and list(got) == [10, 14, 0, 0x7FC00000, 0x7FC00000, 0x7FC00000, 0x7FC00000]
    term = np.array([[0, 0], [1, 0], [0, 0], [0, 0]], np.uint8)
    trunc = np.array([[0, 0], [0, 0], [0, 2], [0, 0]], np.uint8)
    c = nh.classes(2, np.zeros((4, 2)), term, trunc)
    assert c["full"].tolist() == [[False, True], [False, False], [True, False], [False, False]]
    assert c["last"].tolist() == [[True, False], [False, True], [False, False], [False, False]]
    assert c["first"].tolist() == [[False, False], [True, False], [False, True], [False, False]]
    assert c["chunk"].tolist() == [[False, False], [False, False], [False, False], [True, True]]
    assert c["terminated"].tolist() == [[False, False], [True, False], [False, False], [False, False]]
    assert c["truncated"].tolist() == [[False, False], [False, False], [False, True], [False, False]]
