"""Host statement of the ORDER OF ADDITIONS of the vector-level normalisation sums (gym_amd/csrc/mxv_norm.hip), in NumPy float64.

Not a test module: tests/test_norm_tree_host.py (CPU) and tests/test_gpu_norm_trees.py (device) import it.  Nothing under gym_amd/ does.

The device forms every per-step column sum as a fixed binary tree, so a sum is a pure function of its inputs and their positions:
  * wave_tree_sum   the xor butterfly over lane bits 0..5 = the pairwise tree over the lane index of a wave64;
  * obs_leaves      a leaf = 4096 rows, lane t of 256 accumulates rows t, t + 256, ... from 0.0 (s += v; q = q + v * v), the butterfly per
                    wave, then (w0 + w1) + (w2 + w3);
  * returns_leaves  a leaf = 256 envs = one wave, lane L accumulates envs 4 L + j, j = 0..3, from 0.0, then the butterfly;
  * tree_level      groups of 1024 leaves, lane t takes leaves 4 t .. 4 t + 3 as (a0 + a1) + (a2 + a3), missing leaves +0.0, the butterfly,
                    the four-wave combine; `tree` repeats it until one group is left (at least once, as the device does);
  * rank_tree       the stride-doubling tree over the shards' sums (scan_kernel; tree_over_ranks in oracle/normalize.c);
  * returns_update / reward_sums   NormalizeReward's recurrence ret = ret * gamma + r (two roundings), zeroed AFTER the sums where an env
                    finished.

Two places use an identity instead of the device's literal instruction, both exact:
  * rows / envs past the end are padded with +0.0 where the device skips them: an accumulator that starts at +0.0 is never -0.0, and
    x + 0.0 == x for every other x (NaN included), so the padded additions change nothing;
  * q = q + v * v stands for __fma_rn(v, v, q).  They agree when v * v is exact in float64: always for a float32 v (24-bit significand),
    and for a return of at most 26 significant bits (`significant_bits_at_most`).  For general returns the square is rounded once more
    here than on the device; tests of such inputs use the exact references below, not this twin, for q.

Exact references (no tree): `two_square` (Dekker's error-free product), `exact_sum` (math.fsum of exactly representable terms) and
`depth_obs` / `depth_returns`, the largest number of additions any one term passes through, for the bound
|sum - exact| <= d * 2^-53 * sum|term| * (1 + 2^-40).
"""
from __future__ import annotations

import math

import numpy as np

LANES = 64
THREADS = 256            # lanes per workgroup of the observation leaves and of a tree level
OBS_LEAF_ROWS = 4096
REW_LEAF_ENVS = 256
TREE_FAN = 1024
_LANE = np.arange(LANES)


def wave_butterfly(v: np.ndarray) -> np.ndarray:
    """[..., 64] -> [..., 64]: every lane's value after the six xor stages (lane ^ 1, ^ 2, ^ 4, ^ 8, ^ 16, ^ 32)."""
    v = np.asarray(v, np.float64)
    assert v.shape[-1] == LANES
    for bit in range(6):
        v = v + v[..., _LANE ^ (1 << bit)]
    return v


def wave_tree_sum(v: np.ndarray) -> np.ndarray:
    """[..., 64] -> [...]: the wave's total (what lane 0 holds; every lane holds the same)."""
    return wave_butterfly(v)[..., 0]


def _four_waves(w: np.ndarray) -> np.ndarray:
    """[..., 4, V] -> [..., V]: (w0 + w1) + (w2 + w3)."""
    return (w[..., 0, :] + w[..., 1, :]) + (w[..., 2, :] + w[..., 3, :])


def _pad_rows(a: np.ndarray, rows: int) -> np.ndarray:
    if a.shape[0] == rows:
        return a
    out = np.zeros((rows,) + a.shape[1:], np.float64)
    out[:a.shape[0]] = a
    return out


def obs_leaves(x: np.ndarray) -> np.ndarray:
    """x [n][O] (float32 values) -> partials [ceil(n / 4096)][2 O] = (sum_0.., sumsq_0..) per leaf."""
    x = np.asarray(x, np.float64)
    n, O = x.shape
    leaves = -(-n // OBS_LEAF_ROWS)
    v = _pad_rows(x, leaves * OBS_LEAF_ROWS).reshape(leaves, OBS_LEAF_ROWS // THREADS, THREADS, O)
    s = np.zeros((leaves, THREADS, O))
    q = np.zeros((leaves, THREADS, O))
    for i in range(v.shape[1]):                      # a lane's rows t, t + 256, ... in order
        s = s + v[:, i]
        q = q + v[:, i] * v[:, i]
    sq = np.concatenate([s, q], axis=-1).reshape(leaves, THREADS // LANES, LANES, 2 * O)
    return _four_waves(wave_tree_sum(np.moveaxis(sq, 2, -1)))


def obs_leaf(x: np.ndarray) -> np.ndarray:
    """x [rows <= 4096][O] -> [2 O]."""
    assert x.shape[0] <= OBS_LEAF_ROWS
    return obs_leaves(x)[0]


def returns_leaves(ret: np.ndarray) -> np.ndarray:
    """ret [n] (the returns after a step's update) -> partials [ceil(n / 256)][2] = (sum, sumsq) per leaf."""
    ret = np.asarray(ret, np.float64)
    leaves = -(-ret.shape[0] // REW_LEAF_ENVS)
    v = _pad_rows(ret, leaves * REW_LEAF_ENVS).reshape(leaves, LANES, 4)
    s = np.zeros((leaves, LANES))
    q = np.zeros((leaves, LANES))
    for j in range(4):
        s = s + v[:, :, j]
        q = q + v[:, :, j] * v[:, :, j]
    return np.stack([wave_tree_sum(s), wave_tree_sum(q)], axis=-1)


def returns_leaf(ret: np.ndarray) -> np.ndarray:
    """ret [<= 256] -> [2]."""
    assert ret.shape[0] <= REW_LEAF_ENVS
    return returns_leaves(ret)[0]


def tree_level(partials: np.ndarray) -> np.ndarray:
    """partials [leaves][V] -> [ceil(leaves / 1024)][V]."""
    partials = np.asarray(partials, np.float64)
    leaves, V = partials.shape
    groups = -(-leaves // TREE_FAN)
    a = _pad_rows(partials, groups * TREE_FAN).reshape(groups, THREADS, 4, V)
    t = (a[:, :, 0] + a[:, :, 1]) + (a[:, :, 2] + a[:, :, 3])
    t = t.reshape(groups, THREADS // LANES, LANES, V)
    return _four_waves(wave_tree_sum(np.moveaxis(t, 2, -1)))


def tree_levels(leaves: int) -> int:
    """How many levels `tree` runs over that many leaves (1 up to 1024, 2 up to 1024^2, ...)."""
    levels = 1
    while leaves > TREE_FAN:
        leaves = -(-leaves // TREE_FAN)
        levels += 1
    return levels


def tree(partials: np.ndarray) -> np.ndarray:
    """partials [leaves][V] -> [V]: levels of 1024 until one group is left."""
    p = tree_level(partials)
    while p.shape[0] > 1:
        p = tree_level(p)
    return p[0]


def rank_tree(all_sums: np.ndarray) -> np.ndarray:
    """all_sums [W][...] -> [...]: the binary tree over the rank index, an odd leftover passing through a level unchanged."""
    b = np.array(all_sums, np.float64)
    W = b.shape[0]
    stride = 1
    while stride < W:
        for w in range(0, W - stride, 2 * stride):
            b[w] = b[w] + b[w + stride]
        stride <<= 1
    return b[0]


def obs_sums(x: np.ndarray) -> np.ndarray:
    """x [K][n][O] -> sums [K][2 O] of one shard."""
    return np.stack([tree(obs_leaves(xk)) for xk in x])


def returns_update(ret: np.ndarray, r: np.ndarray, gamma: float) -> np.ndarray:
    """normalize.py:132, two roundings."""
    return np.asarray(ret, np.float64) * np.float64(gamma) + np.asarray(r, np.float64)


def returns_trajectory(ret0: np.ndarray, rew: np.ndarray, done: np.ndarray, gamma: float):
    """-> (rets [K][n]: the returns each step's sums see, final [n]: the accumulators after the last step's zeroing)."""
    ret = np.array(ret0, np.float64)
    rets = []
    for k in range(rew.shape[0]):
        ret = returns_update(ret, rew[k], gamma)
        rets.append(ret)
        ret = np.where(np.asarray(done[k]).astype(bool), 0.0, ret)
    return np.stack(rets), ret


def reward_sums(ret0: np.ndarray, rew: np.ndarray, done: np.ndarray, gamma: float):
    """rew [K][n], done [K][n] (terminated | truncated) -> (sums [K][2], final returns [n])."""
    rets, final = returns_trajectory(ret0, rew, done, gamma)
    return np.stack([tree(returns_leaves(r)) for r in rets]), final


# ---- exact references and the bound -------------------------------------------------------------------------------------------------

def significant_bits_at_most(a: np.ndarray, bits: int) -> bool:
    """Every finite element has at most `bits` significant bits (so its square is exact in float64 for bits <= 26)."""
    m, _ = np.frexp(np.asarray(a, np.float64))
    scaled = np.ldexp(m, bits)
    return bool(np.all(scaled == np.rint(scaled)))


def two_square(a: np.ndarray):
    """-> (p, e) with a * a == p + e exactly (Dekker / Veltkamp; no overflow or underflow at the magnitudes the tests use)."""
    a = np.asarray(a, np.float64)
    p = a * a
    c = 134217729.0 * a                 # 2^27 + 1
    hi = c - (c - a)
    lo = a - hi
    e = ((hi * hi - p) + 2.0 * hi * lo) + lo * lo
    return p, e


def exact_sum(*terms) -> float:
    """The exact sum of every element of every array, rounded once (math.fsum)."""
    return math.fsum(float(v) for t in terms for v in np.asarray(t, np.float64).ravel())


def depth_obs(n: int) -> int:
    """Additions a term of an observation column sum passes through: the lane's row loop, six butterfly stages, two for the four waves,
    then ten per tree level (two for a lane's four leaves, six, two)."""
    rows = min(n, OBS_LEAF_ROWS)
    return -(-rows // THREADS) + 6 + 2 + 10 * tree_levels(-(-n // OBS_LEAF_ROWS))


def depth_returns(n: int) -> int:
    """The same for the return sums: a lane's four envs, six butterfly stages (one wave per leaf), ten per tree level."""
    return 4 + 6 + 10 * tree_levels(-(-n // REW_LEAF_ENVS))


def sum_error_bound(d: int, abs_total: float) -> float:
    """|tree sum - exact sum| for terms that each pass through at most d roundings to nearest: (1 + u)^d - 1 <= d u (1 + 2^-40) for the
    depths here (d u < 2^-46), u = 2^-53."""
    return d * 2.0 ** -53 * abs_total * (1.0 + 2.0 ** -40)
