"""tests/norm_tree_host.py, the NumPy statement of the normalisation sum trees (gym_amd/csrc/mxv_norm.hip), checked on its own: integers sum
exactly whatever the order, the order is fixed and matters (a wide dynamic range separates it from np.sum), power-of-two shards of whole
leaves are complete subtrees (shard sums combined by the rank tree == the unsharded tree, the README's sharding claim), and the tree stays
within the bound its depth implies against the exact sum.  No device needed; tests/test_gpu_norm_trees.py holds the kernels to this twin."""
from fractions import Fraction

import numpy as np
import pytest

import norm_tree_host as nt


def _wide(rng, shape):
    """wide dynamic range: the order of additions decides the last bits"""
    return rng.standard_normal(shape) * np.exp(rng.uniform(-20, 20, shape))


def test_butterfly_leaves_the_same_pairwise_tree_in_every_lane():
    rng = np.random.default_rng(0)
    v = _wide(rng, (5, 64))
    b = nt.wave_butterfly(v)
    assert np.all(b == b[:, :1])
    # the pairwise tree over lane index, written as a recursion
    def pairwise(a):
        return a[0] if len(a) == 1 else pairwise(a[0::2] + a[1::2])
    for row, got in zip(v, nt.wave_tree_sum(v)):
        assert got == pairwise(row)
    assert not np.array_equal(nt.wave_tree_sum(v), v.sum(axis=1))          # not NumPy's order
    assert nt.wave_tree_sum(np.arange(64.0)) == 2016.0


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097, 9000])
@pytest.mark.parametrize("O", [1, 3, 6])
def test_integer_observations_sum_exactly(n, O):
    rng = np.random.default_rng(n * 7 + O)
    x = rng.integers(-1000, 1000, (2, n, O))
    assert n * 1000 ** 2 < 2 ** 53
    got = nt.obs_sums(x.astype(np.float32))
    want = np.concatenate([x.sum(axis=1), (x * x).sum(axis=1)], axis=1)
    assert np.array_equal(got, want.astype(np.float64))


@pytest.mark.parametrize("n", [1, 3, 4, 255, 256, 257, 1022, 2049, 262_149])
@pytest.mark.parametrize("gamma", [1.0, 0.5])
def test_integer_returns_sum_exactly_and_finished_envs_restart(n, gamma):
    rng = np.random.default_rng(n)
    K = 5
    rew = rng.integers(-100, 100, (K, n))
    done = rng.random((K, n)) < 0.2
    ret0 = rng.integers(-100, 100, n)
    sums, final = nt.reward_sums(ret0, rew, done, gamma)
    # exact integers at scale 2^K: returns are multiples of 2^-k after step k
    scale = 1 << K
    r = ret0.astype(np.int64) * scale
    for k in range(K):
        r = (r if gamma == 1.0 else r // 2) + rew[k] * scale
        assert n * int(np.abs(r).max()) ** 2 < 2 ** 53
        assert sums[k, 0] == r.sum() / scale and sums[k, 1] == (r * r).sum() / scale ** 2
        r[done[k]] = 0
    assert np.array_equal(final, r / scale) and np.all(final[done[-1]] == 0)


def test_order_matters_and_is_fixed():
    rng = np.random.default_rng(1)
    x = _wide(rng, (1, 12_289, 4)).astype(np.float32)
    s = nt.obs_sums(x)
    assert np.array_equal(s, nt.obs_sums(x.copy()))
    plain = np.concatenate([x.astype(np.float64).sum(axis=1), (x.astype(np.float64) ** 2).sum(axis=1)], axis=1)
    assert not np.array_equal(s, plain)
    np.testing.assert_allclose(s, plain, rtol=1e-11)
    perm = rng.permutation(x.shape[1])
    assert not np.array_equal(s, nt.obs_sums(x[:, perm]))                  # WHERE a row sits decides the rounding
    p = _wide(rng, (2049, 2))
    assert np.array_equal(nt.tree(p), nt.tree(p.copy())) and not np.array_equal(nt.tree(p), p.sum(axis=0))


@pytest.mark.parametrize("leaves", [1, 2, 3, 4, 5, 1023, 1024, 1025, 2049])
def test_tree_levels_missing_leaves_and_pass_through(leaves):
    rng = np.random.default_rng(leaves)
    p = _wide(rng, (leaves, 2))
    lvl = nt.tree_level(p)
    assert lvl.shape == (-(-leaves // 1024), 2)
    assert nt.tree_levels(leaves) == (1 if leaves <= 1024 else 2)
    if leaves % 1024 == 1:
        assert np.array_equal(lvl[-1], p[-1])                              # a single leftover leaf passes through unchanged
    k = rng.integers(-1000, 1000, (leaves, 2)).astype(np.float64)
    assert np.array_equal(nt.tree(k), k.sum(axis=0))
    if leaves <= 4:                                                        # (a0 + a1) + (a2 + a3), missing = +0.0
        a = np.zeros((4, 2))
        a[:leaves] = p
        assert np.array_equal(nt.tree(p), (a[0] + a[1]) + (a[2] + a[3]))


def test_third_level_with_two_pass_throughs():
    leaves = 1024 * 1024 + 1
    rng = np.random.default_rng(2)
    p = _wide(rng, (leaves, 2))
    assert nt.tree_levels(leaves) == 3
    l1 = nt.tree_level(p)
    l2 = nt.tree_level(l1)
    assert l1.shape[0] == 1025 and l2.shape[0] == 2
    assert np.array_equal(l1[-1], p[-1]) and np.array_equal(l2[-1], p[-1])
    assert np.array_equal(nt.tree(p), l2[0] + l2[1])


@pytest.mark.parametrize("W", [1, 2, 3, 5, 8, 63, 64])
def test_rank_tree_is_the_pairwise_tree_with_odd_leftovers(W):
    rng = np.random.default_rng(W)
    a = _wide(rng, (W, 3, 4))

    def pairwise(v):                                                       # oracle/normalize.c tree_over_ranks as a recursion
        if len(v) == 1:
            return v[0]
        nxt = [v[i] + v[i + 1] for i in range(0, len(v) - 1, 2)] + ([v[-1]] if len(v) % 2 else [])
        return pairwise(nxt)

    assert np.array_equal(nt.rank_tree(a), pairwise(list(a)))
    k = rng.integers(-1000, 1000, (W, 3, 4)).astype(np.float64)
    assert np.array_equal(nt.rank_tree(k), k.sum(axis=0))


@pytest.mark.parametrize("world", [2, 4, 8])
def test_power_of_two_shards_are_complete_subtrees(world):
    """n = 32768 rows = 8 observation leaves = 128 return leaves; every shard is at least one leaf of either kind."""
    rng = np.random.default_rng(world)
    n = 32_768
    x = _wide(rng, (2, n, 3)).astype(np.float32)
    nl = n // world
    shards = np.stack([nt.obs_sums(x[:, w * nl:(w + 1) * nl]) for w in range(world)])
    assert np.array_equal(nt.rank_tree(shards), nt.obs_sums(x))
    ret = _wide(rng, n).astype(np.float32).astype(np.float64)               # 24 significant bits: squares are exact
    assert nt.significant_bits_at_most(ret, 26)
    whole = nt.tree(nt.returns_leaves(ret))
    parts = np.stack([nt.tree(nt.returns_leaves(ret[w * nl:(w + 1) * nl])) for w in range(world)])
    assert np.array_equal(nt.rank_tree(parts), whole)
    assert not np.array_equal(whole, nt.tree(nt.returns_leaves(rng.permutation(ret))))   # order-sensitive input: the check above is not vacuous


def test_shards_of_three_leaves_are_not_subtrees():
    """the claim is about shards that are complete subtrees: power-of-two counts of whole leaves.  Two shards of three leaves each pair
    their leaves as ((a0 + a1) + a2) + ((a3 + a4) + a5), the unsharded tree as ((a0 + a1) + (a2 + a3)) + (a4 + a5): both are sums,
    the bits differ.  (Three shards of ONE leaf each are still the unsharded tree: an odd leftover passes through both alike.)"""
    rng = np.random.default_rng(5)
    x = _wide(rng, (1, 6 * 4096, 2)).astype(np.float32)
    whole = nt.obs_sums(x)
    halves = np.stack([nt.obs_sums(x[:, w * 3 * 4096:(w + 1) * 3 * 4096]) for w in range(2)])
    np.testing.assert_allclose(nt.rank_tree(halves), whole, rtol=1e-11)
    assert not np.array_equal(nt.rank_tree(halves), whole)
    thirds = np.stack([nt.obs_sums(x[:, w * 4096:(w + 1) * 4096]) for w in range(3)])
    assert np.array_equal(nt.rank_tree(thirds), nt.obs_sums(x[:, :3 * 4096]))


def test_single_leaf_forms_are_the_first_leaf_of_the_batched_ones():
    rng = np.random.default_rng(8)
    x = _wide(rng, (5000, 3)).astype(np.float32)
    assert np.array_equal(nt.obs_leaf(x[:4096]), nt.obs_leaves(x)[0]) and np.array_equal(nt.obs_leaf(x[4096:]), nt.obs_leaves(x)[1])
    ret = _wide(rng, 300).astype(np.float32).astype(np.float64)
    assert np.array_equal(nt.returns_leaf(ret[:256]), nt.returns_leaves(ret)[0])
    assert np.array_equal(nt.returns_leaf(ret[256:]), nt.returns_leaves(ret)[1])
    with pytest.raises(AssertionError):
        nt.obs_leaf(x[:4097])
    with pytest.raises(AssertionError):
        nt.returns_leaf(ret[:257])


def test_two_square_is_error_free():
    rng = np.random.default_rng(6)
    a = np.concatenate([_wide(rng, 200), rng.standard_normal(200), [0.0, 1.0, -3.5, 2.0 ** -30 + 1.0]])
    p, e = nt.two_square(a)
    for ai, pi, ei in zip(a, p, e):
        assert Fraction(ai) ** 2 == Fraction(pi) + Fraction(ei)
    assert np.any(e != 0)
    small = np.ldexp(rng.integers(-2 ** 26 + 1, 2 ** 26, 100).astype(np.float64), rng.integers(-30, 30, 100))
    assert nt.significant_bits_at_most(small, 26) and np.all(nt.two_square(small)[1] == 0)
    assert not nt.significant_bits_at_most(np.array([2.0 ** 27 + 1.0]), 26)


@pytest.mark.parametrize("n", [1022, 70_003])
def test_twin_within_the_depth_bound_of_the_exact_sum(n):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((1, n, 4)) * [2.4, 3.0, 0.2, 3.0] + [0.5, -1.0, 0.0, 2.0]).astype(np.float32)
    got = nt.obs_sums(x)[0]
    d = nt.depth_obs(n)
    assert d == (4 if n == 1022 else 16) + 6 + 2 + 10
    x64 = x[0].astype(np.float64)
    for j in range(4):
        for col, terms in ((j, x64[:, j]), (4 + j, x64[:, j] * x64[:, j])):   # squares of float32 are exact in float64
            err = abs(nt.exact_sum(terms, [-got[col]]))
            assert err <= nt.sum_error_bound(d, nt.exact_sum(np.abs(terms))), (n, col)
    # returns whose squares are exact
    ret = np.ldexp(rng.integers(-2 ** 25, 2 ** 25, n).astype(np.float64), rng.integers(-8, 8, n))
    assert nt.significant_bits_at_most(ret, 26)
    s, q = nt.tree(nt.returns_leaves(ret))
    d = nt.depth_returns(n)
    assert d == 4 + 6 + 10
    assert abs(nt.exact_sum(ret, [-s])) <= nt.sum_error_bound(d, nt.exact_sum(np.abs(ret)))
    assert abs(nt.exact_sum(ret * ret, [-q])) <= nt.sum_error_bound(d, nt.exact_sum(ret * ret))


def test_depths_follow_the_shapes():
    assert nt.depth_obs(1) == 1 + 8 + 10 and nt.depth_obs(257) == 2 + 8 + 10 and nt.depth_obs(4097) == 16 + 8 + 10
    assert nt.depth_obs(4096 * 1024 + 1) == 16 + 8 + 20
    assert nt.depth_returns(262_144) == 20 and nt.depth_returns(262_145) == 30
