"""gym_amd.gae / gym_amd.discounted_returns on the device against tests/gae_host.py, the float64 twin of the rule (include/mxv_gae.h):
every output compared as uint32, so NaNs, the sign of zero and subnormals count.  Shapes around the ring depth D and the tile of 256
lanes; strided views of every alignment class with a guard pattern around them; flag patterns; the exact-rational case against
float32(Fraction); non-finite, huge, tiny and signed-zero values; N >= 2^21, where a lane owns four envs and the grid strides over the
tiles; the rollout methods; one capture into a torch.cuda.graph."""
import numpy as np
import pytest

import gae_host
from gae_host import bits

pytestmark = pytest.mark.gpu

GUARD_F32 = 0x7FABCDEF      # a NaN pattern no computation produces (NaN results are written as 0x7FC00000)
GUARD_U8 = 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def D():
    from gym_amd.returns import RING_DEPTH

    return RING_DEPTH


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host_bits(torch, x):
    return x.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def last_launch():
    from gym_amd.returns import last_launch

    return last_launch()


def make_case(K, N, seed, reward_dtype=np.float32, p=0.1):
    rng = np.random.default_rng(seed)
    return dict(reward=rng.standard_normal((K, N)).astype(reward_dtype), terminated=(rng.random((K, N)) < p).astype(np.uint8),
                truncated=(rng.random((K, N)) < p).astype(np.uint8), values=rng.standard_normal((K, N)).astype(np.float32),
                last_value=rng.standard_normal(N).astype(np.float32), final_values=rng.standard_normal((K, N)).astype(np.float32))


def check(torch, c, mode, with_final=True, with_last=True, gamma=0.99, lam=0.95, d=None, what=""):
    """Device against twin for the arrays of `c` (d: their device copies, made here when None); -> number of compared elements."""
    import gym_amd

    d = {k: dev(torch, v) for k, v in c.items()} if d is None else d
    fv, lv = ("final_values" if with_final else None), ("last_value" if with_last else None)
    if mode == "gae":
        want = gae_host.gae(c["reward"], c["terminated"], c["truncated"], c["values"], c[lv] if lv else None, gamma=gamma, lam=lam,
                            final_values=c[fv] if fv else None)
        got = gym_amd.gae(d["reward"], d["terminated"], d["truncated"], d["values"], d[lv] if lv else None, gamma=gamma, lam=lam,
                          final_values=d[fv] if fv else None)
    else:
        want = (gae_host.discounted_returns(c["reward"], c["terminated"], c["truncated"], gamma=gamma, last_value=c[lv] if lv else None,
                                            final_values=c[fv] if fv else None),)
        got = (gym_amd.discounted_returns(d["reward"], d["terminated"], d["truncated"], gamma=gamma, last_value=d[lv] if lv else None,
                                          final_values=d[fv] if fv else None),)
    for name, g, w in zip(("advantages", "returns") if mode == "gae" else ("returns",), got, want):
        assert g.dtype == torch.float32 and tuple(g.shape) == w.shape
        gb = host_bits(torch, g)
        bad = np.argwhere(gb != bits(w))
        assert bad.size == 0, f"{what} {mode} {name}: {len(bad)} of {w.size} differ, first at {bad[0]}: {gb[tuple(bad[0])]:#x} != {bits(w)[tuple(bad[0])]:#x}"
    return sum(w.size for w in want)


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------------
NS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 4100)


@pytest.mark.parametrize("reward_dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mode", ["gae", "returns"])
def test_shapes_around_the_ring_depth_and_the_tile(torch, D, reward_dtype, mode):
    """K in {1, 2, 3, D-1, D, D+1, 2D+3} x N in NS x final_values x last_value: one master case, sliced (and made contiguous) per shape."""
    Ks = sorted({1, 2, 3, D - 1, D, D + 1, 2 * D + 3})
    master = make_case(max(Ks), max(NS), 100, reward_dtype)
    dm = {k: dev(torch, v) for k, v in master.items()}
    n = 0
    for K in Ks:
        for N in NS:
            c = {k: np.ascontiguousarray(v[:K, :N] if v.ndim == 2 else v[:N]) for k, v in master.items()}
            d = {k: (v[:K, :N] if v.dim() == 2 else v[:N]).contiguous() for k, v in dm.items()}
            for with_final in (False, True):
                for with_last in (False, True):
                    n += check(torch, c, mode, with_final, with_last, d=d, what=f"K={K} N={N} final={with_final} last={with_last}")
            assert last_launch() == (1, -(-N // 256))          # below 2^21 envs: one env per lane, one workgroup per 256 envs
    assert n > 0


# ---- alignment classes -------------------------------------------------------------------------------------------------------------------------
def _parents(torch, c, K, N, off, width):
    """Every [K, N] array of `c` as the view [:, off:off+N] of a guard-filled [K, width] device buffer; -> (views, parents)."""
    views, parents = {}, {}
    for k, v in c.items():
        if v.ndim != 2:
            views[k] = dev(torch, v)
            continue
        if v.dtype == np.uint8:
            parent = torch.full((K, width), GUARD_U8, dtype=torch.uint8, device="cuda:0")
        else:
            parent = torch.full((K, width), 12345.0, dtype=torch.from_numpy(v[:1, :1]).dtype, device="cuda:0")
        parent[:, off:off + N] = dev(torch, v)
        views[k], parents[k] = parent[:, off:off + N], parent
    return views, parents


def _guarded_out(torch, K, N, off, width):
    parent = torch.full((K, width), GUARD_F32, dtype=torch.int32, device="cuda:0").view(torch.float32)
    return parent[:, off:off + N], parent


def _assert_guard_intact(torch, parent, off, N, what):
    pb = host_bits(torch, parent)
    outside = np.ones(pb.shape, bool)
    outside[:, off:off + N] = False
    assert (pb[outside] == GUARD_F32).all(), f"{what}: elements outside the view were written"


@pytest.mark.parametrize("off", [1, 2, 4])
@pytest.mark.parametrize("reward_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_strided_views_of_every_alignment_class(torch, off, reward_dtype):
    """Inputs and outputs sliced [:, off:] out of wider buffers: ld != N, the base off 16 bytes (off 4 bytes for the flags at off = 1, 2),
    an even and an odd ld.  What lies outside the views — of the inputs' parents and of the outputs' — is untouched."""
    import gym_amd

    K, N = 7, 257
    c = make_case(K, N, 200 + off, reward_dtype)
    for width in (off + N + 2, off + N + 3):
        views, parents = _parents(torch, c, K, N, off, width)
        before = {k: p.clone() for k, p in parents.items()}
        (oa, pa), (og, pg), (orr, pr) = (_guarded_out(torch, K, N, off, width + 4) for _ in range(3))
        gym_amd.gae(views["reward"], views["terminated"], views["truncated"], views["values"], views["last_value"], final_values=views["final_values"],
                    out=(oa, og))
        gym_amd.discounted_returns(views["reward"], views["terminated"], views["truncated"], last_value=views["last_value"],
                                   final_values=views["final_values"], out=orr)
        wa, wg = gae_host.gae(**c)
        wr = gae_host.discounted_returns(c["reward"], c["terminated"], c["truncated"], last_value=c["last_value"], final_values=c["final_values"])
        for name, g, w, p in (("advantages", oa, wa, pa), ("returns", og, wg, pg), ("returns-to-go", orr, wr, pr)):
            assert np.array_equal(host_bits(torch, g), bits(w)), (name, off, width)
            _assert_guard_intact(torch, p, off, N, f"{name} off={off} width={width}")
        for k, p in parents.items():
            assert torch.equal(p.view(torch.uint8), before[k].view(torch.uint8)), f"input {k} was written"


def test_inputs_and_outputs_as_column_blocks_of_one_buffer_each(torch):
    """reward | values | final_values as column blocks of one float32 buffer, advantages | returns of another: the ranges interleave
    with one row stride and share no byte, so the call is accepted — and each block holds exactly its own result."""
    import gym_amd

    K, N = 6, 130
    c = make_case(K, N, 250)
    fin = torch.full((K, 3 * N + 5), 12345.0, device="cuda:0")
    blocks = {k: fin[:, i * N + 1:(i + 1) * N + 1] for i, k in enumerate(("reward", "values", "final_values"))}
    for k, v in blocks.items():
        v.copy_(dev(torch, c[k]))
    flags = torch.full((K, 3 * N + 5), GUARD_U8, dtype=torch.uint8, device="cuda:0")
    te, tr = flags[:, 2:N + 2], flags[:, N + 3:2 * N + 3]
    te.copy_(dev(torch, c["terminated"]))
    tr.copy_(dev(torch, c["truncated"]))
    out = torch.full((K, 2 * N + 3), GUARD_F32, dtype=torch.int32, device="cuda:0").view(torch.float32)
    adv, ret = gym_amd.gae(blocks["reward"], te, tr, blocks["values"], dev(torch, c["last_value"]), final_values=blocks["final_values"],
                           out=(out[:, :N], out[:, N + 1:2 * N + 1]))
    wa, wg = gae_host.gae(**c)
    assert np.array_equal(host_bits(torch, adv), bits(wa)) and np.array_equal(host_bits(torch, ret), bits(wg))
    ob = host_bits(torch, out)
    assert (ob[:, N] == GUARD_F32).all() and (ob[:, 2 * N + 1:] == GUARD_F32).all()
    with pytest.raises(ValueError, match="overlap"):
        gym_amd.gae(blocks["reward"], te, tr, blocks["values"], out=(out[:, :N], out[:, N - 1:2 * N - 1]))
    with pytest.raises(ValueError, match="overlaps input values"):
        gym_amd.gae(blocks["reward"], te, tr, blocks["values"], out=(fin[:, N + 5:2 * N + 5], fin[:, 2 * N + 5:3 * N + 5]))


# ---- flags ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["p=0.1", "all", "none", "first", "last", "0xFF", "other-bytes"])
def test_flag_patterns(torch, pattern):
    K, N = 11, 300
    c = make_case(K, N, 300)
    rng = np.random.default_rng(301)
    if pattern == "p=0.1":
        assert ((c["terminated"] != 0) & (c["truncated"] != 0)).sum() > 0      # both set somewhere
    elif pattern in ("all", "none"):
        c["terminated"][:] = 0
        c["truncated"][:] = 0
        if pattern == "all":
            which = rng.integers(0, 3, (K, N))                # terminated, truncated or both: every row ends an episode
            c["terminated"][which != 1] = 1
            c["truncated"][which != 0] = 1
    elif pattern in ("first", "last"):
        t = 0 if pattern == "first" else K - 1
        keep_te, keep_tr = c["terminated"][t].copy(), c["truncated"][t].copy()
        c["terminated"][:] = 0
        c["truncated"][:] = 0
        c["terminated"][t], c["truncated"][t] = keep_te | (rng.random(N) < 0.4), keep_tr | (rng.random(N) < 0.4)
    elif pattern == "0xFF":
        c["terminated"] *= 0xFF
        c["truncated"] *= 0xFF
    else:
        c["terminated"] *= rng.choice(np.array([2, 0x80, 0x10, 3], np.uint8), (K, N))
        c["truncated"] *= rng.choice(np.array([4, 0x40, 0xFE, 7], np.uint8), (K, N))
    for mode in ("gae", "returns"):
        for with_final in (False, True):
            check(torch, c, mode, with_final, what=pattern)


def test_bool_flags_are_taken_as_views(torch):
    import gym_amd

    c = make_case(6, 130, 310)
    d = {k: dev(torch, v) for k, v in c.items()}
    want = gae_host.gae(**c)
    got = gym_amd.gae(d["reward"], d["terminated"].bool(), d["truncated"].bool(), d["values"], d["last_value"], final_values=d["final_values"])
    assert all(np.array_equal(host_bits(torch, g), bits(w)) for g, w in zip(got, want))


# ---- values --------------------------------------------------------------------------------------------------------------------------------------
def test_exact_rational_case_against_float32_of_fractions(torch):
    import gym_amd
    from test_gae_host import rational_case, rational_reference

    c = rational_case()
    want = rational_reference(c)
    d = {k: dev(torch, v) for k, v in c.items() if k not in ("gamma", "lam")}
    got = gym_amd.gae(d["reward"], d["terminated"], d["truncated"], d["values"], d["last_value"], gamma=c["gamma"], lam=c["lam"],
                      final_values=d["final_values"])
    mism = sum(int((host_bits(torch, g) != bits(w)).sum()) for g, w in zip(got, want))
    print(f"mismatches against float32(Fraction): {mism}")
    assert mism == 0


@pytest.mark.parametrize("reward_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_non_finite_values_just_after_episode_boundaries(torch, reward_dtype):
    """NaN and +-Inf in the rewards, values, final_values and last_value of the rows right after a boundary (t + 1 where a flag is set at
    t): they must fill their own episode's rows and none before the boundary — the twin says which."""
    K, N = 13, 260
    c = make_case(K, N, 400, reward_dtype, p=0.15)
    rng = np.random.default_rng(401)
    done = (c["terminated"] != 0) | (c["truncated"] != 0)
    after = np.zeros((K, N), bool)
    after[1:] = done[:-1]
    specials = np.array([np.nan, np.inf, -np.inf])
    for key in ("reward", "values", "final_values"):
        hit = after & (rng.random((K, N)) < 0.5)
        c[key][hit] = rng.choice(specials, int(hit.sum())).astype(c[key].dtype)
    c["last_value"][rng.random(N) < 0.3] = np.nan
    c["final_values"][done & (rng.random((K, N)) < 0.2)] = np.inf
    want = gae_host.gae(**c)[0]
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
    for mode in ("gae", "returns"):
        for with_final in (False, True):
            check(torch, c, mode, with_final, what="non-finite")


@pytest.mark.parametrize("reward_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_magnitudes_from_1e_30_to_1e30_subnormal_and_overflowing_results(torch, reward_dtype):
    K, N = 12, 520
    c = make_case(K, N, 500, reward_dtype)
    rng = np.random.default_rng(501)
    scale = 10.0 ** rng.integers(-30, 31, N)                         # one magnitude per env ...
    scale[:40], scale[40:80] = 1e-41, 1.0                            # ... float32-subnormal results, and (below) sums that overflow float32
    for key in ("reward", "values", "final_values"):
        with np.errstate(over="ignore"):
            c[key] = (c[key].astype(np.float64) * scale).astype(c[key].dtype)
    c["last_value"] = (c["last_value"].astype(np.float64) * scale).astype(np.float32)
    c["reward"][:, 40:80] = np.abs(c["reward"][:, 40:80]) + np.asarray(3e38, c["reward"].dtype)      # a few steps of +3e38 each: beyond 3.4e38
    c["terminated"][:, 40:80] = 0
    c["truncated"][:, 40:80] = 0
    if reward_dtype == np.float64:
        c["reward"][:, 80:120] = np.float64(1e-310) * rng.standard_normal((K, 40))      # float64 subnormals and rewards beyond float32's range
        c["reward"][:, 120:160] = np.float64(1e200) * rng.standard_normal((K, 40))
    want = gae_host.discounted_returns(c["reward"], c["terminated"], c["truncated"])
    sub = (np.abs(want) > 0) & (np.abs(want) < np.finfo(np.float32).tiny)
    assert sub.any() and np.isinf(want).any(), "the case must hold subnormal and overflowing float32 results"
    for mode in ("gae", "returns"):
        for with_final in (False, True):
            check(torch, c, mode, with_final, what="magnitudes")


def test_negative_zero_rewards(torch):
    K, N = 9, 140
    c = make_case(K, N, 600)
    c["reward"][:] = -0.0
    c["values"][:, ::2] = 0.0
    c["values"][:, 1::4] = -0.0
    c["final_values"][:, ::3] = -0.0
    c["last_value"][::2] = -0.0
    for gamma in (0.99, -0.5, 0.0):
        for mode in ("gae", "returns"):
            check(torch, c, mode, True, gamma=gamma, what=f"-0.0 gamma={gamma}")
            check(torch, c, mode, False, False, gamma=gamma, what=f"-0.0 gamma={gamma}")
    z = np.zeros_like(c["terminated"])
    want = gae_host.discounted_returns(c["reward"], z, z, gamma=0.99, last_value=np.full(N, -0.0, np.float32))
    assert (bits(want) == 0x80000000).all()         # -0 + 0.99 * -0 = -0 all the way up: the case does hold the sign of zero


# ---- four envs per lane, and the grid stride ---------------------------------------------------------------------------------------------------
BIG = 1 << 21


@pytest.fixture(scope="module")
def big(torch, D):
    """One [2D+3, 2^21 + 8] case shared by the tests below (its device copies too); they read it and leave it unchanged."""
    K = 2 * D + 3
    rng = np.random.default_rng(700)
    N = BIG + 8
    c = dict(reward=rng.standard_normal((K, N), dtype=np.float32), terminated=(rng.random((K, N), dtype=np.float32) < 0.05).astype(np.uint8),
             truncated=(rng.random((K, N), dtype=np.float32) < 0.05).astype(np.uint8), values=rng.standard_normal((K, N), dtype=np.float32),
             last_value=rng.standard_normal(N, dtype=np.float32), final_values=rng.standard_normal((K, N), dtype=np.float32))
    c["reward"][3, BIG // 2 + 5] = np.nan
    return c, {k: dev(torch, v) for k, v in c.items()}


def _big_view(c, d, K, off, N):
    cut = lambda v: v[:K, off:off + N] if v.ndim == 2 else v[off:off + N]
    return {k: cut(v) for k, v in c.items()}, {k: cut(v) for k, v in d.items()}


@pytest.mark.parametrize("K_of, off, N, mode, with_final, with_last, envs_per_lane", [
    ("2D+3", 0, BIG + 4, "gae", False, True, 4),       # 16-byte path; the last tile holds one live lane
    ("D+1", 4, BIG, "gae", True, False, 4),            # 16-byte path on a base 16 bytes into the rows
    ("D", 0, BIG, "returns", False, False, 4),
    ("1", 8, BIG, "returns", True, True, 4),
    ("3", 1, BIG, "gae", True, True, 1),               # base off 16 bytes: element path at a size where the grid strides over the tiles
    ("2", 0, BIG - 4, "returns", False, True, 1),      # below the threshold: element path, 8 191.98 tiles on 2 048 workgroups
], ids=lambda v: str(v))
def test_four_envs_per_lane_and_the_grid_stride(torch, D, big, K_of, off, N, mode, with_final, with_last, envs_per_lane):
    """N >= 2^21 with 16-byte alignment throughout takes the four-envs-per-lane path (strided views of one wide buffer: ld = 2^21 + 8);
    the same sizes off that alignment, or just below the threshold, take the element path with more tiles than workgroups.  Which
    instantiation ran is read back (mxv_gae_last_launch): a silent fall to the element path would otherwise pass bit for bit."""
    K = {"1": 1, "2": 2, "3": 3, "D": D, "D+1": D + 1, "2D+3": 2 * D + 3}[K_of]
    c, d = _big_view(*big, K, off, N)
    check(torch, c, mode, with_final, with_last, d=d, what=f"K={K} off={off} N={N}")
    assert last_launch() == (envs_per_lane, 2048)
    assert -(-N // (256 * envs_per_lane)) > 2048 or (N, envs_per_lane) == (BIG, 4)      # more tiles than workgroups (2 048 exactly at 2^21 / 4)


def test_four_envs_per_lane_float64_rewards_into_guarded_views(torch, D, big):
    import gym_amd

    K, off, N = D + 2, 4, BIG
    c, d = _big_view(*big, K, off, N)
    c, d = dict(c), dict(d)
    c["reward"] = c["reward"].astype(np.float64) * np.float64(1.0 + 2.0 ** -40)       # bits below float32's
    d["reward"] = torch.zeros((K, BIG + 8), dtype=torch.float64, device="cuda:0")[:, off:off + N]
    d["reward"].copy_(dev(torch, c["reward"]))
    (oa, pa), (og, pg) = (_guarded_out(torch, K, N, off, BIG + 8) for _ in range(2))
    gym_amd.gae(d["reward"], d["terminated"], d["truncated"], d["values"], d["last_value"], final_values=d["final_values"], out=(oa, og))
    assert last_launch() == (4, 2048)
    wa, wg = gae_host.gae(**c)
    for name, g, w, p in (("advantages", oa, wa, pa), ("returns", og, wg, pg)):
        assert torch.equal(g.contiguous().view(torch.int32), dev(torch, bits(w).view(np.int32))), name
        _assert_guard_intact(torch, p, off, N, name)


# ---- the rollout methods -----------------------------------------------------------------------------------------------------------------------
def _rollout_case(torch, make, want_final):
    r = make()
    r.reset(seed=3)
    K = 16
    traj = r.rollout_per_step(K, out=r.trajectory_buffers(K, want_final=True, layout="separate") if want_final else r.trajectory_buffers(K, layout="separate"))
    g = torch.Generator(device="cuda:0").manual_seed(5)
    n = r.num_envs
    values, final_values = (torch.randn((K, n), device="cuda:0", generator=g) for _ in range(2))
    last_value = torch.randn(n, device="cuda:0", generator=g)
    return r, traj, values, last_value, final_values


@pytest.mark.parametrize("kind", ["CartPole-v1", "FrozenLake-v1", "Blackjack-v1"])
def test_rollout_methods_equal_the_functions_on_the_same_tensors(torch, kind):
    import gym_amd
    from gym_amd._rollout_base import _RolloutBase
    from gym_amd.rollout import DeviceRollout
    from gym_amd.toy_text import BlackjackRollout, TabularRollout

    make = {"CartPole-v1": lambda: DeviceRollout("CartPole-v1", 256, seed=1, action_seed=2),
            "FrozenLake-v1": lambda: TabularRollout("FrozenLake-v1", 256, seed=1, action_seed=2),
            "Blackjack-v1": lambda: BlackjackRollout(256, seed=1, action_seed=2)}[kind]
    r, traj, values, last_value, final_values = _rollout_case(torch, make, want_final=kind == "CartPole-v1")
    assert isinstance(r, _RolloutBase)
    adv, ret = r.advantages(traj, values, last_value, gamma=0.98, lam=0.9, final_values=final_values)
    rtg = r.returns_to_go(traj, gamma=0.98, last_value=last_value, final_values=final_values)
    torch.cuda.synchronize()
    assert int(traj["terminated"].sum() + traj["truncated"].sum()) > 0
    wadv, wret = gym_amd.gae(traj["reward"], traj["terminated"], traj["truncated"], values, last_value, gamma=0.98, lam=0.9, final_values=final_values)
    wrtg = gym_amd.discounted_returns(traj["reward"], traj["terminated"], traj["truncated"], gamma=0.98, last_value=last_value, final_values=final_values)
    for got, want in ((adv, wadv), (ret, wret), (rtg, wrtg)):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    host = lambda x: x.cpu().numpy()
    tadv, tret = gae_host.gae(host(traj["reward"]), host(traj["terminated"]), host(traj["truncated"]), host(values), host(last_value),
                              gamma=0.98, lam=0.9, final_values=host(final_values))
    assert np.array_equal(host_bits(torch, adv), bits(tadv)) and np.array_equal(host_bits(torch, ret), bits(tret))
    out = (torch.empty_like(adv), torch.empty_like(ret))
    again = r.advantages(traj, values, last_value, gamma=0.98, lam=0.9, final_values=final_values, out=out)
    assert again[0] is out[0] and again[1] is out[1] and torch.equal(out[0].view(torch.int32), adv.view(torch.int32))
    r.close()


def test_values_of_the_pre_step_observations_give_the_one_step_td_error(torch):
    """The recipe of advantages()'s docstring on a real chunk: traj["obs"][t] is the observation AFTER step t, so values =
    V(pre_step_observations(first_obs, traj["obs"])) and last_value = V(traj["obs"][K-1]).  With lam = 0 every advantage is then the
    TD error of its own transition: reward + gamma * V(observation after the step) - V(observation before it) where the episode
    goes on, reward - V(observation before it) where it terminated — never a value of the next episode's reset observation."""
    from gym_amd.returns import pre_step_observations
    from gym_amd.rollout import DeviceRollout

    K, gamma = 16, 0.97
    r = DeviceRollout("CartPole-v1", 256, seed=1, action_seed=2)
    first = r.reset(seed=3).clone()
    traj = r.rollout_per_step(K, out=r.trajectory_buffers(K, want_final=True, layout="separate"))
    r.ready()
    w = torch.tensor([0.3, -0.2, 1.5, 0.1], device="cuda:0")
    V = lambda obs: obs @ w + 0.25
    pre = pre_step_observations(first, traj["obs"])
    assert torch.equal(pre[0], first) and torch.equal(pre[1:], traj["obs"][:-1])
    values = V(pre)
    last_value = V(traj["obs"][K - 1])
    adv, ret = r.advantages(traj, values, last_value, gamma=gamma, lam=0.0, final_values=V(traj["final_obs"]))
    term, trunc = traj["terminated"] != 0, traj["truncated"] != 0
    assert int(term.sum()) > 50 and not bool(trunc.any())
    value_after = torch.cat((values[1:], last_value[None]))      # = V(traj["obs"]) row by row: pre[t + 1] is traj["obs"][t]
    after = torch.where(term, torch.zeros((), dtype=torch.float64, device="cuda:0"), value_after.double())
    want = ((traj["reward"].double() + gamma * after) - values.double()).float()
    assert torch.equal(adv.view(torch.int32), want.view(torch.int32))
    # the mistake the docstring warns of is visible on this chunk: after an autoreset traj["obs"][t] is not the episode's last observation
    assert not torch.equal(traj["obs"][term], traj["final_obs"][term])
    r.close()


# ---- graph capture -----------------------------------------------------------------------------------------------------------------------------
def test_one_capture_replayed_on_changed_inputs(torch):
    import gym_amd

    K, N = 9, 1500
    cases = [make_case(K, N, 800 + i) for i in range(3)]
    d = {k: dev(torch, v) for k, v in cases[0].items()}
    out = (torch.empty((K, N), device="cuda:0"), torch.empty((K, N), device="cuda:0"))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):       # a warm-up launch outside the capture
        gym_amd.gae(d["reward"], d["terminated"], d["truncated"], d["values"], d["last_value"], final_values=d["final_values"], out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gym_amd.gae(d["reward"], d["terminated"], d["truncated"], d["values"], d["last_value"], final_values=d["final_values"], out=out)
    for c in cases[1:]:
        for k, v in c.items():
            d[k].copy_(dev(torch, v))
        out[0].zero_()
        out[1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = gae_host.gae(**c)
        assert all(np.array_equal(host_bits(torch, g), bits(w)) for g, w in zip(out, want))
