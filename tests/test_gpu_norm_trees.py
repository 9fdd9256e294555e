"""The sums kernels of the vector-level NormalizeObservation / NormalizeReward (gym_amd/csrc/mxv_norm.hip: obs_sums_kernel,
returns_sums_kernel, tree_kernel) on the MI355X, held to references that fail on one wrong bit:

  (a) small signed integers sum exactly in any order: the device sums of x and x^2 equal int64 sums — a dropped, doubled or misplaced row,
      env, leaf or flag byte is a wrong integer.  Every size at which a kernel takes another path: one lane, one wave, four waves, the
      r += 256 row loop, whole and ragged leaves, every residue of the return leaves mod 8 (the XCD remap) and of n mod 4 (vector or
      element loads), K below, at and above the 4-deep register ring (results only: a look-ahead that read behind the tape could not show in
      them), a second tree level with a single leftover group;
  (b) inputs of a wide dynamic range, where the order of additions decides the last bits, equal tests/norm_tree_host.py bit for bit —
      the kernels, the tree alone on synthetic partials (up to a third level), and shards combined by the rank tree;
  (c) general inputs (gamma = 0.99, random doubles) stay within d * 2^-53 * sum|term| * (1 + 2^-40) of the exact sum, d counted from the
      tree for the shape at hand.

Each integer test asserts its own bit budget (n * max^2 in units of the smallest lsb < 2^53); each bit-exact return test asserts that its
returns have at most 26 significant bits, so that the twin's q + ret * ret is the device's fma(ret, ret, q).
"""
import numpy as np
import pytest

import norm_tree_host as nt

pytestmark = pytest.mark.gpu

DIMS = (1, 2, 3, 4, 6)
K_MAX = 9
RING_KS = (1, 2, 3, 4, 5, 7, 8, 9)
FLAG_PATTERNS = ("byte0", "byte1", "byte2", "byte3", "terminated", "truncated", "both", "none")
REWARD_NS = [256 * L + r for L in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 23) for r in (0, 1, 3, 4, 255) if 256 * L + r > 0]
REWARD_NS += [262_144, 262_148, 262_149]


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _wide(rng, shape):
    return rng.standard_normal(shape) * np.exp(rng.uniform(-20, 20, shape))


def _flags(pattern, rng, K, n):
    """-> (terminated, truncated) uint8 [K][n]"""
    te, tr = np.zeros((K, n), np.uint8), np.zeros((K, n), np.uint8)
    if pattern.startswith("byte"):                       # exactly the envs with e % 4 == j finish, at step 0
        te[0, np.arange(n) % 4 == int(pattern[4])] = 1
    if pattern in ("terminated", "both"):
        te[:] = rng.random((K, n)) < 0.2
    if pattern in ("truncated", "both"):
        tr[:] = rng.random((K, n)) < 0.2
    return te, tr


# ---- (a) integers ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8193, 70_003])
@pytest.mark.parametrize("O", DIMS)
def test_obs_sums_of_integers_are_exact(O, n):
    import torch
    from gym_amd import _native

    rng = np.random.default_rng(1000 * O + n)
    for K in (1, 3):
        xi = rng.integers(-1000, 1000, (K, n, O))
        assert n * int(np.abs(xi).max()) ** 2 < 2 ** 53                    # bit budget: every partial sum is an exact integer
        want = np.concatenate([xi.sum(axis=1), (xi * xi).sum(axis=1)], axis=1)
        nm = _native.Norm(O, n)
        sums = torch.full((K, 2 * O), np.nan, dtype=torch.float64, device="cuda")
        nm.obs_sums(K, _dev(xi.astype(np.float32)), sums)
        torch.cuda.synchronize()
        got = sums.cpu().numpy()
        nm.close()
        assert np.array_equal(got, want.astype(np.float64)), (K, np.argwhere(got != want)[:4])
        if K == 1:
            assert np.array_equal(nt.obs_sums(xi.astype(np.float32)), got)  # and so does the twin


@pytest.mark.parametrize("n", REWARD_NS)
def test_reward_sums_of_integers_are_exact(n):
    """Every K of RING_KS x every flag pattern x gamma in {1, 0.5} x float32 / float64 rewards, from non-zero initial returns; the sums of
    every step and the accumulators left behind (get_state) against int64 arithmetic (at scale 2^K_MAX for gamma = 0.5, which then halves exactly)."""
    import torch
    from gym_amd import _native

    rng = np.random.default_rng(n)
    rew = rng.integers(-100, 100, (K_MAX, n))
    ret0 = rng.integers(-100, 100, n)
    rew_dev = {False: _dev(rew.astype(np.float64)), True: _dev(rew.astype(np.float32))}
    nm = _native.Norm(1, n)
    sums = torch.empty((K_MAX, 2), dtype=torch.float64, device="cuda")
    for pattern in FLAG_PATTERNS:
        te, tr = _flags(pattern, rng, K_MAX, n)
        done = (te | tr).astype(bool)
        ted, trd = _dev(te), _dev(tr)
        for gamma in (1.0, 0.5):
            scale = 1 if gamma == 1.0 else 1 << K_MAX                      # the returns' smallest lsb is 1 resp. 2^-(K_MAX - 1)
            r = ret0.astype(np.int64) * scale
            want, finals = np.zeros((K_MAX, 2)), []
            for k in range(K_MAX):
                r = (r if gamma == 1.0 else r // 2) + rew[k] * scale
                assert n * int(np.abs(r).max()) ** 2 < 2 ** 53             # bit budget, in units of 1 / scale (squares: 1 / scale^2)
                want[k] = r.sum() / scale, (r * r).sum() / scale ** 2
                r = np.where(done[k], 0, r)
                finals.append(r / scale)
            for K in RING_KS:
                # tensors of exactly K steps: nothing valid lies behind the tape for the ring's look-ahead to read
                tek, trk = ted[:K].clone(), trd[:K].clone()
                for f32 in (False, True):
                    rk = rew_dev[f32][:K].clone()
                    assert rk.data_ptr() % 32 == 0 and tek.data_ptr() % 4 == 0 and trk.data_ptr() % 4 == 0    # whole allocations
                    nm.set_state([0.0], [1.0], 1e-4, returns=ret0.astype(np.float64))
                    sums.fill_(float("nan"))
                    nm.reward_sums(K, rk, f32, tek, trk, gamma, sums)
                    torch.cuda.synchronize()
                    got = sums.cpu().numpy()[:K]
                    returns = nm.get_state(want_returns=True)[3]
                    where = (pattern, gamma, K, f32)
                    assert np.array_equal(got, want[:K]), (where, got - want[:K])
                    assert np.array_equal(returns, finals[K - 1]), (where, np.flatnonzero(returns != finals[K - 1])[:8])
    nm.close()


# ---- (b) the order of additions, bit for bit against the twin -------------------------------------------------------------------------

@pytest.mark.parametrize("n", [300, 4097, 12_289])
@pytest.mark.parametrize("O", [3, 4, 6])
def test_obs_sums_equal_the_twin_bit_for_bit(O, n):
    import torch
    from gym_amd import _native

    rng = np.random.default_rng(100 * O + n)
    K = 2
    x = _wide(rng, (K, n, O)).astype(np.float32)
    nm = _native.Norm(O, n)
    sums = torch.full((K, 2 * O), np.nan, dtype=torch.float64, device="cuda")
    nm.obs_sums(K, _dev(x), sums)
    torch.cuda.synchronize()
    got = sums.cpu().numpy()
    nm.close()
    want = nt.obs_sums(x)
    plain = np.concatenate([x.astype(np.float64).sum(axis=1), (x.astype(np.float64) ** 2).sum(axis=1)], axis=1)
    assert not np.array_equal(want, plain)                                  # the order matters on these inputs
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


def _narrow_returns_case(rng, n, K):
    """rewards integer x 2^e with one exponent per env, flags on, gamma = 0.5: every return keeps at most 26 significant bits"""
    e = rng.integers(-40, 41, n)                                            # 2^80 between envs: sums round, in an order-dependent way
    rew = np.ldexp(rng.integers(-1000, 1000, (K, n)).astype(np.float64), e[None, :])
    ret0 = np.ldexp(rng.integers(-1000, 1000, n).astype(np.float64), e)
    te = (rng.random((K, n)) < 0.1).astype(np.uint8)
    tr = (rng.random((K, n)) < 0.1).astype(np.uint8)
    return rew, ret0, te, tr


@pytest.mark.parametrize("n", [1022, 4100, 70_003])
@pytest.mark.parametrize("gamma", [1.0, 0.5])
def test_reward_sums_equal_the_twin_bit_for_bit(gamma, n):
    import torch
    from gym_amd import _native

    rng = np.random.default_rng(n)
    K = 3
    rew, ret0, te, tr = _narrow_returns_case(rng, n, K)
    rets, final = nt.returns_trajectory(ret0, rew, te | tr, gamma)
    assert nt.significant_bits_at_most(rets, 26)                            # ret * ret is exact: fma(ret, ret, q) == q + ret * ret
    assert np.all(nt.two_square(rets)[1] == 0)
    want = np.stack([nt.tree(nt.returns_leaves(r)) for r in rets])
    assert not np.array_equal(want[:, 0], rets.sum(axis=1))                 # the order matters on these inputs
    nm = _native.Norm(1, n)
    nm.set_state([0.0], [1.0], 1e-4, returns=ret0)
    sums = torch.full((K, 2), np.nan, dtype=torch.float64, device="cuda")
    nm.reward_sums(K, _dev(rew), False, _dev(te), _dev(tr), gamma, sums)
    torch.cuda.synchronize()
    got = sums.cpu().numpy()
    returns = nm.get_state(want_returns=True)[3]
    nm.close()
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(returns, final)


TREE_LEAVES = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049]


# the third level (two pass-throughs) is driven at V = 2 only: 16 MB of partials per step
@pytest.mark.parametrize("V,leaves", [(V, l) for V in (2, 12) for l in TREE_LEAVES] + [(2, 1024 * 1024 + 1)])
def test_tree_alone_on_synthetic_partials(V, leaves):
    """mxv_norm_reward_sums_partials (V = 2) / mxv_norm_obs_sums_partials (V = 2 dim, also at dim 1): one, two and three levels, missing
    leaves, single leftover groups passing through."""
    import torch
    from gym_amd import _native

    rng = np.random.default_rng(leaves + V)
    handles = [("obs", _native.Norm(V // 2, 1))] + ([("reward", _native.Norm(1, 1))] if V == 2 else [])
    for K in (1, 2):
        p = _wide(rng, (K, leaves, V))
        want = np.stack([nt.tree(pk) for pk in p])
        pd = _dev(p)
        for kind, nm in handles:
            sums = torch.full((K, V), np.nan, dtype=torch.float64, device="cuda")
            (nm.obs_sums_partials if kind == "obs" else nm.reward_sums_partials)(K, pd, leaves, sums)
            torch.cuda.synchronize()
            got = sums.cpu().numpy()
            assert np.array_equal(got, want), (kind, K, np.argwhere(got != want)[:4])
        if leaves >= 255:                                                   # the order matters on these inputs
            assert not np.array_equal(want, p.sum(axis=1))
    for _, nm in handles:
        nm.close()


@pytest.mark.parametrize("world", [2, 4])
def test_shard_sums_combined_by_the_rank_tree_equal_the_unsharded_sums(world):
    import torch
    from gym_amd import _native

    n, K, O = 16_384, 2, 4
    rng = np.random.default_rng(world)
    x = _wide(rng, (K, n, O)).astype(np.float32)
    rew, ret0, te, tr = _narrow_returns_case(rng, n, K)

    def device_sums(lo, hi):
        m = hi - lo
        a, b = _native.Norm(O, m), _native.Norm(1, m)
        so = torch.full((K, 2 * O), np.nan, dtype=torch.float64, device="cuda")
        sr = torch.full((K, 2), np.nan, dtype=torch.float64, device="cuda")
        a.obs_sums(K, _dev(x[:, lo:hi]), so)
        b.set_state([0.0], [1.0], 1e-4, returns=ret0[lo:hi])
        b.reward_sums(K, _dev(rew[:, lo:hi]), False, _dev(te[:, lo:hi]), _dev(tr[:, lo:hi]), 0.5, sr)
        torch.cuda.synchronize()
        out = so.cpu().numpy(), sr.cpu().numpy()
        a.close(), b.close()
        return out

    whole_o, whole_r = device_sums(0, n)
    nl = n // world
    parts = [device_sums(w * nl, (w + 1) * nl) for w in range(world)]
    assert np.array_equal(nt.rank_tree(np.stack([p[0] for p in parts])), whole_o)
    assert np.array_equal(nt.rank_tree(np.stack([p[1] for p in parts])), whole_r)
    assert np.array_equal(whole_o, nt.obs_sums(x))
    assert not np.array_equal(whole_r[:, 0], nt.returns_trajectory(ret0, rew, te | tr, 0.5)[0].sum(axis=1))


# ---- (c) general inputs against exact sums under the bound of the tree's depth --------------------------------------------------------

@pytest.mark.parametrize("n", [1022, 70_003])
def test_general_inputs_within_the_depth_bound_of_the_exact_sums(n):
    """|device - exact| <= d * 2^-53 * sum|term| * (1 + 2^-40): every term passes through at most d additions, each rounding to nearest
    (relative error <= 2^-53), and (1 + u)^d - 1 <= d u (1 + 2^-40) while d u < 2^-46.  d = depth_obs / depth_returns of the shape: the row
    loop (4 and 16 rows a lane here) or a lane's four envs, six butterfly stages, two for the four waves, ten per tree level.  Exact terms:
    squares of float32 are exact doubles; squares of returns are split error-free (two_square); math.fsum sums them exactly and rounds
    once — the device's value goes into the same fsum, so the error itself is what is rounded (relative 2^-53, inside the 2^-40 slack)."""
    import torch
    from gym_amd import _native

    rng = np.random.default_rng(n)
    K, O, gamma = 3, 4, 0.99
    x = (rng.standard_normal((K, n, O)) * [2.4, 3.0, 0.2, 3.0] + [0.5, -1.0, 0.0, 2.0]).astype(np.float32)   # CartPole-like columns
    rew = rng.standard_normal((K, n)) * 3.0 + 1.0
    te = (rng.random((K, n)) < 0.1).astype(np.uint8)
    tr = (rng.random((K, n)) < 0.05).astype(np.uint8)
    a, b = _native.Norm(O, n), _native.Norm(1, n)
    so = torch.full((K, 2 * O), np.nan, dtype=torch.float64, device="cuda")
    sr = torch.full((K, 2), np.nan, dtype=torch.float64, device="cuda")
    a.obs_sums(K, _dev(x), so)
    b.reward_sums(K, _dev(rew), False, _dev(te), _dev(tr), gamma, sr)
    torch.cuda.synchronize()
    so, sr = so.cpu().numpy(), sr.cpu().numpy()
    returns = b.get_state(want_returns=True)[3]
    a.close(), b.close()

    d_obs, d_ret = nt.depth_obs(n), nt.depth_returns(n)
    assert d_obs == -(-min(n, 4096) // 256) + 6 + 2 + 10 and d_ret == 4 + 6 + 10
    worst = 0.0
    x64 = x.astype(np.float64)
    for k in range(K):
        for j in range(O):
            for col, terms in ((j, x64[k, :, j]), (O + j, x64[k, :, j] * x64[k, :, j])):
                err, bound = abs(nt.exact_sum(terms, [-so[k, col]])), nt.sum_error_bound(d_obs, nt.exact_sum(np.abs(terms)))
                worst = max(worst, err / bound)
                assert err <= bound, ("obs", k, col, err, bound)
    rets, final = nt.returns_trajectory(np.zeros(n), rew, te | tr, gamma)       # the recurrence itself is IEEE-exact
    assert np.array_equal(returns, final)
    for k in range(K):
        p, e = nt.two_square(rets[k])
        for col, terms in ((0, (rets[k],)), (1, (p, e))):
            err = abs(nt.exact_sum(*terms, [-sr[k, col]]))
            bound = nt.sum_error_bound(d_ret, nt.exact_sum(np.abs(rets[k])) if col == 0 else nt.exact_sum(p, e))
            worst = max(worst, err / bound)
            assert err <= bound, ("returns", k, col, err, bound)
    print(f"n={n}: worst |error| / bound = {worst:.3f} (d = {d_obs} observations, {d_ret} returns)")
