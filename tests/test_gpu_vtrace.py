"""gym_amd.vtrace on the device against tests/vtrace_host.py, the float64 twin of the rule (include/mxv_vtrace.h): every output compared
as uint32, so NaNs, the sign of zero and subnormals count.  Shapes around the ring depth D and the tile of 256 lanes; strided views of
every alignment class with a guard pattern around them; flag patterns; clip levels; log-ratios around the clamp at +-80; non-finite,
huge and tiny values; N >= 2^21, where a lane owns four envs; the two bit identities (on-policy vs = GAE returns, w = the PPO ratio) on
the device; the rollout method; one capture into a torch.cuda.graph; inputs that require grad."""
import numpy as np
import pytest

import vtrace_host
from vtrace_host import bits

pytestmark = pytest.mark.gpu

GUARD_F32 = 0x7FABCDEF      # a NaN pattern no computation produces (NaN results are written as 0x7FC00000)
GUARD_U8 = 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def D():
    from gym_amd.vtrace import RING_DEPTH

    return RING_DEPTH


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host_bits(torch, x):
    return x.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def last_launch():
    from gym_amd.vtrace import last_launch

    return last_launch()


def make_case(K, N, seed, reward_dtype=np.float32, p=0.1, spread=3.0):
    rng = np.random.default_rng(seed)
    old = -np.abs(rng.standard_normal((K, N))).astype(np.float32)
    return dict(log_prob=(old + rng.uniform(-spread, spread, (K, N))).astype(np.float32), old_log_prob=old,
                reward=rng.standard_normal((K, N)).astype(reward_dtype), terminated=(rng.random((K, N)) < p).astype(np.uint8),
                truncated=(rng.random((K, N)) < p).astype(np.uint8), values=rng.standard_normal((K, N)).astype(np.float32),
                last_value=rng.standard_normal(N).astype(np.float32), final_values=rng.standard_normal((K, N)).astype(np.float32))


def call(f, c, with_final=True, with_last=True, **kw):
    return f(c["log_prob"], c["old_log_prob"], c["reward"], c["terminated"], c["truncated"], c["values"], c["last_value"] if with_last else None,
             final_values=c["final_values"] if with_final else None, **kw)


def compare(torch, got, want, what=""):
    for name, g, w in zip(("vs", "pg_advantages"), got, want):
        assert g.dtype == torch.float32 and tuple(g.shape) == w.shape and not g.requires_grad
        gb = host_bits(torch, g)
        bad = np.argwhere(gb != bits(w))
        assert bad.size == 0, f"{what} {name}: {len(bad)} of {w.size} differ, first at {bad[0]}: {gb[tuple(bad[0])]:#x} != {bits(w)[tuple(bad[0])]:#x}"


def check(torch, c, with_final=True, with_last=True, d=None, what="", **kw):
    """Device against twin for the arrays of `c` (d: their device copies, made here when None)."""
    import gym_amd

    d = {k: dev(torch, v) for k, v in c.items()} if d is None else d
    compare(torch, call(gym_amd.vtrace, d, with_final, with_last, **kw), call(vtrace_host.vtrace, c, with_final, with_last, **kw), what)


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------------
NS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 4100)


@pytest.mark.parametrize("reward_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_shapes_around_the_ring_depth_and_the_tile(torch, D, reward_dtype):
    """K in {1, 2, 3, D-1, D, D+1, 2D+3} x N in NS x final_values x last_value: one master case, sliced (and made contiguous) per shape."""
    Ks = sorted({1, 2, 3, D - 1, D, D + 1, 2 * D + 3})
    master = make_case(max(Ks), max(NS), 100, reward_dtype)
    dm = {k: dev(torch, v) for k, v in master.items()}
    for K in Ks:
        for N in NS:
            c = {k: np.ascontiguousarray(v[:K, :N] if v.ndim == 2 else v[:N]) for k, v in master.items()}
            d = {k: (v[:K, :N] if v.dim() == 2 else v[:N]).contiguous() for k, v in dm.items()}
            for with_final in (False, True):
                for with_last in (False, True):
                    check(torch, c, with_final, with_last, d=d, lam=0.95, what=f"K={K} N={N} final={with_final} last={with_last}")
            assert last_launch() == (1, -(-N // 256))          # below 2^21 envs: one env per lane, one workgroup per 256 envs


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
    """Inputs and outputs sliced [:, off:] out of wider buffers: ld != N, an even and an odd ld.  What lies outside the views — of the
    inputs' parents and of the outputs' — is untouched."""
    import gym_amd

    K, N = 7, 257
    c = make_case(K, N, 200 + off, reward_dtype)
    want = call(vtrace_host.vtrace, c, c_bar=1.5)
    for width in (off + N + 2, off + N + 3):
        views, parents = _parents(torch, c, K, N, off, width)
        before = {k: p.clone() for k, p in parents.items()}
        (ov, pv), (og, pg) = (_guarded_out(torch, K, N, off, width + 4) for _ in range(2))
        got = call(gym_amd.vtrace, views, c_bar=1.5, out=(ov, og))
        assert got[0] is ov and got[1] is og
        compare(torch, got, want, f"off={off} width={width}")
        for name, p in (("vs", pv), ("pg_advantages", pg)):
            _assert_guard_intact(torch, p, off, N, f"{name} off={off} width={width}")
        for k, p in parents.items():
            assert torch.equal(p.view(torch.uint8), before[k].view(torch.uint8)), f"input {k} was written"


def test_inputs_and_outputs_as_column_blocks_of_one_buffer_each_and_overlapping_outputs(torch):
    """The float32 inputs as column blocks of one buffer, vs | pg_advantages of another: the ranges interleave with one row stride and
    share no byte, so the call is accepted, and each block holds exactly its own result.  Outputs that share bytes are refused."""
    import gym_amd

    K, N = 6, 130
    c = make_case(K, N, 250)
    names = ("log_prob", "old_log_prob", "reward", "values", "final_values")
    fin = torch.full((K, 6 * N + 5), 12345.0, device="cuda:0")
    d = {k: fin[:, i * N + 1:(i + 1) * N + 1] for i, k in enumerate(names)}
    for k, v in d.items():
        v.copy_(dev(torch, c[k]))
    flags = torch.full((K, 6 * N + 5), GUARD_U8, dtype=torch.uint8, device="cuda:0")
    d["terminated"], d["truncated"] = flags[:, 2:N + 2], flags[:, N + 3:2 * N + 3]
    d["terminated"].copy_(dev(torch, c["terminated"]))
    d["truncated"].copy_(dev(torch, c["truncated"]))
    d["last_value"] = dev(torch, c["last_value"])
    out = torch.full((K, 2 * N + 3), GUARD_F32, dtype=torch.int32, device="cuda:0").view(torch.float32)
    got = call(gym_amd.vtrace, d, out=(out[:, :N], out[:, N + 1:2 * N + 1]))
    compare(torch, got, call(vtrace_host.vtrace, c))
    ob = host_bits(torch, out)
    assert (ob[:, N] == GUARD_F32).all() and (ob[:, 2 * N + 1:] == GUARD_F32).all()
    with pytest.raises(ValueError, match="outputs vs and pg_advantages overlap"):
        call(gym_amd.vtrace, d, out=(out[:, :N], out[:, N - 1:2 * N - 1]))
    with pytest.raises(ValueError, match="outputs vs and pg_advantages overlap"):
        call(gym_amd.vtrace, d, out=(out[:, :N], out[:, :N]))
    with pytest.raises(ValueError, match="overlaps input old_log_prob"):
        call(gym_amd.vtrace, d, out=(fin[:, N + 5:2 * N + 5], fin[:, 5 * N + 2:6 * N + 2]))
    assert (host_bits(torch, out)[:, N] == GUARD_F32).all()       # the refused calls wrote nothing


# ---- flags ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["all", "none", "first", "last", "0xFF", "other-bytes", "bool"])
def test_flag_patterns(torch, pattern):
    import gym_amd

    K, N = 11, 300
    c = make_case(K, N, 300)
    rng = np.random.default_rng(301)
    if pattern in ("all", "none"):
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
    elif pattern == "other-bytes":
        c["terminated"] *= rng.choice(np.array([2, 0x80, 0x10, 3], np.uint8), (K, N))
        c["truncated"] *= rng.choice(np.array([4, 0x40, 0xFE, 7], np.uint8), (K, N))
    if pattern == "bool":
        d = {k: dev(torch, v) for k, v in c.items()}
        d["terminated"], d["truncated"] = d["terminated"].bool(), d["truncated"].bool()
        compare(torch, call(gym_amd.vtrace, d), call(vtrace_host.vtrace, c), pattern)
        return
    for with_final in (False, True):
        check(torch, c, with_final, what=pattern, lam=0.95)


# ---- clip levels ---------------------------------------------------------------------------------------------------------------------------------
def test_clip_levels_and_lambda(torch):
    """{0.5, 1, 2} for each of the three levels x lam in {0, 0.95, 1}, and pg_rho_bar=None = rho_bar; weights on both sides of every level."""
    K, N = 9, 300
    c = make_case(K, N, 350, spread=1.5)
    d = {k: dev(torch, v) for k, v in c.items()}
    w = vtrace_host.weights(c["log_prob"], c["old_log_prob"])
    assert (w < 0.5).any() and ((w > 0.5) & (w < 1)).any() and ((w > 1) & (w < 2)).any() and (w > 2).any()
    levels = (0.5, 1.0, 2.0)
    for rho_bar in levels:
        for c_bar in levels:
            for pg in levels + (None,):
                for lam in (0.0, 0.95, 1.0):
                    check(torch, c, d=d, rho_bar=rho_bar, c_bar=c_bar, pg_rho_bar=pg, lam=lam, gamma=0.97, what=f"{rho_bar} {c_bar} {pg} {lam}")
    import gym_amd

    a = call(gym_amd.vtrace, d, rho_bar=2.0, pg_rho_bar=None)
    b = call(gym_amd.vtrace, d, rho_bar=2.0, pg_rho_bar=2.0)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_log_ratios_on_both_sides_of_the_clamp(torch):
    """d = log_prob - old_log_prob at, next to and far beyond +-80, and +-Inf: the clamp, not an overflow of EXP."""
    K, N = 6, 260
    c = make_case(K, N, 360)
    ds = np.array([79.99999, 80.0, 80.00001, -79.99999, -80.0, -80.00001, 100.0, -100.0, 1e30, -1e30, 88.7, -104.0, 745.0, -746.0], np.float32)
    rng = np.random.default_rng(361)
    c["old_log_prob"][:] = 0.0
    c["log_prob"][:] = rng.choice(ds, (K, N))
    c["log_prob"][2, ::7] = np.inf
    c["log_prob"][3, ::5] = -np.inf
    c["old_log_prob"][4, ::9] = -np.inf        # d = +Inf from the other side
    c["old_log_prob"][1, 3::11] = 40.0
    c["log_prob"][1, 3::11] = -40.0            # d = -80 exactly, by subtraction
    w = vtrace_host.weights(c["log_prob"], c["old_log_prob"])
    assert np.isfinite(w).all() and w.max() == vtrace_host.EXP(np.float64(80.0)) and w.min() == vtrace_host.EXP(np.float64(-80.0))
    for levels in (dict(), dict(rho_bar=1e30, c_bar=1e30), dict(rho_bar=1e40, c_bar=1e-30, pg_rho_bar=1e36)):
        check(torch, c, what=f"clamp {levels}", **levels)


# ---- values --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reward_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_non_finite_values_just_after_episode_boundaries(torch, reward_dtype):
    """NaN and +-Inf in every input in the rows right after a boundary (t + 1 where a flag is set at t): they fill their own episode's
    rows and none before the boundary — the twin says which (tests/test_vtrace_host.py holds the twin to that)."""
    K, N = 13, 260
    c = make_case(K, N, 400, reward_dtype, p=0.15)
    rng = np.random.default_rng(401)
    done = (c["terminated"] != 0) | (c["truncated"] != 0)
    after = np.zeros((K, N), bool)
    after[1:] = done[:-1]
    specials = np.array([np.nan, np.inf, -np.inf])
    for key in ("reward", "values", "final_values", "log_prob", "old_log_prob"):
        hit = after & (rng.random((K, N)) < 0.3)
        c[key][hit] = rng.choice(specials, int(hit.sum())).astype(c[key].dtype)
    c["last_value"][rng.random(N) < 0.3] = np.nan
    c["final_values"][done & (rng.random((K, N)) < 0.2)] = np.inf
    want = call(vtrace_host.vtrace, c)[0]
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
    for with_final in (False, True):
        check(torch, c, with_final, what="non-finite", lam=0.95, c_bar=2.0)


@pytest.mark.parametrize("reward_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_magnitudes_from_1e_30_to_1e30_subnormal_and_overflowing_results(torch, reward_dtype):
    K, N = 12, 520
    c = make_case(K, N, 500, reward_dtype, spread=0.5)
    rng = np.random.default_rng(501)
    scale = 10.0 ** rng.integers(-30, 31, N)                         # one magnitude per env ...
    scale[:40], scale[40:80] = 1e-41, 1.0                            # ... float32-subnormal results, and (below) sums that overflow float32
    for key in ("reward", "values", "final_values"):
        with np.errstate(over="ignore"):
            c[key] = (c[key].astype(np.float64) * scale).astype(c[key].dtype)
    c["last_value"] = (c["last_value"].astype(np.float64) * scale).astype(np.float32)
    c["reward"][:, 40:80] = np.abs(c["reward"][:, 40:80]) + np.asarray(3e38, c["reward"].dtype)      # a few steps of +3e38 each: beyond 3.4e38
    c["values"][:, 40:80] = 0.0
    c["terminated"][:, 40:80] = 0
    c["truncated"][:, 40:80] = 0
    want = call(vtrace_host.vtrace, c)[0]
    sub = (np.abs(want) > 0) & (np.abs(want) < np.finfo(np.float32).tiny)
    assert sub.any() and np.isinf(want).any(), "the case must hold subnormal and overflowing float32 results"
    for with_final in (False, True):
        check(torch, c, with_final, what="magnitudes")


# ---- four envs per lane ---------------------------------------------------------------------------------------------------------------------------
BIG = 1 << 21


@pytest.fixture(scope="module")
def big(torch, D):
    """One [D+2, 2^21 + 8] case with float32 and float64 rewards, its device copies and the twin's results for K = D + 2 and (on the
    first row alone) K = 1: the recurrence is independent per env, so a column range of the case has that column range of the results.
    The tests below read it and leave it unchanged."""
    K, N = D + 2, BIG + 8
    rng = np.random.default_rng(700)
    old = -np.abs(rng.standard_normal((K, N), dtype=np.float32))
    c = dict(log_prob=old + rng.uniform(-1.5, 1.5, (K, N)).astype(np.float32), old_log_prob=old, reward=rng.standard_normal((K, N), dtype=np.float32),
             terminated=(rng.random((K, N), dtype=np.float32) < 0.05).astype(np.uint8),
             truncated=(rng.random((K, N), dtype=np.float32) < 0.05).astype(np.uint8), values=rng.standard_normal((K, N), dtype=np.float32),
             last_value=rng.standard_normal(N, dtype=np.float32), final_values=rng.standard_normal((K, N), dtype=np.float32))
    c["reward"][3, BIG // 2 + 5] = np.nan
    c["log_prob"][2, BIG // 4 + 1] = np.nan
    r64 = c["reward"].astype(np.float64) * np.float64(1.0 + 2.0 ** -40)       # bits below float32's
    d = {k: dev(torch, v) for k, v in c.items()}
    d64 = dev(torch, r64)
    want = {}
    for f64 in (False, True):
        cc = dict(c, reward=r64 if f64 else c["reward"])
        want[K, f64] = call(vtrace_host.vtrace, cc, lam=0.95, c_bar=1.25)
        want[1, f64] = call(vtrace_host.vtrace, {k: (v[:1] if v.ndim == 2 else v) for k, v in cc.items()}, lam=0.95, c_bar=1.25)
    return c, d, d64, want


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("N", [BIG, BIG + 4])
@pytest.mark.parametrize("K_of", ["1", "D+2"])
def test_four_envs_per_lane(torch, D, big, K_of, N, f64):
    """N >= 2^21 with 16-byte alignment throughout takes the four-envs-per-lane path (strided views of one wide buffer: ld = 2^21 + 8).
    Which instantiation ran is read back: a silent fall to the element path would otherwise pass bit for bit.  The same data at a view
    one element further takes the element path, and the bits are equal."""
    import gym_amd

    K = 1 if K_of == "1" else D + 2
    c, d, d64, want = big
    for off, envs_per_lane in ((4, 4), (1, 1)):
        v = {k: (x[:K, off:off + N] if x.dim() == 2 else x[off:off + N]) for k, x in d.items()}
        if f64:
            v["reward"] = d64[:K, off:off + N]
        (ov, pv), (og, pg) = (_guarded_out(torch, K, N, off, BIG + 8) for _ in range(2))
        call(gym_amd.vtrace, v, lam=0.95, c_bar=1.25, out=(ov, og))
        assert last_launch() == (envs_per_lane, 2048)
        for name, g, w, p in (("vs", ov, want[K, f64][0], pv), ("pg_advantages", og, want[K, f64][1], pg)):
            assert torch.equal(g.contiguous().view(torch.int32), dev(torch, bits(w[:, off:off + N]).view(np.int32))), (name, off)
            _assert_guard_intact(torch, p, off, N, name)


# ---- the two identities, on the device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 0.9, 0.95, 1.0])
def test_on_policy_vs_has_the_bits_of_gae_returns(torch, lam):
    import gym_amd

    c = make_case(19, 700, 900)
    c["log_prob"] = c["old_log_prob"].copy()
    d = {k: dev(torch, v) for k, v in c.items()}
    for levels in (dict(), dict(rho_bar=1.0, c_bar=3.0), dict(rho_bar=2.5, c_bar=1.0, pg_rho_bar=0.5)):
        for with_final in (False, True):
            vs, _ = call(gym_amd.vtrace, d, with_final, lam=lam, gamma=0.97, **levels)
            ret = gym_amd.gae(d["reward"], d["terminated"], d["truncated"], d["values"], d["last_value"], gamma=0.97, lam=lam,
                              final_values=d["final_values"] if with_final else None)[1]
            assert torch.equal(vs.view(torch.int32), ret.view(torch.int32)), (lam, levels, with_final)


def test_w_is_the_ratio_of_the_ppo_loss(torch):
    """A one-row batch (K = 1) with reward 1, values 0, no bootstrap and huge clip levels has pg_advantages = float32(w); the extrema of
    the same float32 numbers are ppo_clip_loss's ratio_min / ratio_max, which are float32(r) of the same inputs."""
    import gym_amd
    from gym_amd import ppo

    N = 3000
    c = make_case(1, N, 950, spread=4.0)
    c["log_prob"][0, 5], c["old_log_prob"][0, 5] = 90.0, 0.0
    c["log_prob"][0, 6], c["old_log_prob"][0, 6] = -90.0, 0.0
    d = {k: dev(torch, v) for k, v in c.items()}
    one, zero = torch.ones((1, N), device="cuda:0"), torch.zeros((1, N), device="cuda:0")
    flags = torch.zeros((1, N), dtype=torch.uint8, device="cuda:0")
    _, pg = gym_amd.vtrace(d["log_prob"], d["old_log_prob"], one, flags, flags, zero, None, gamma=0.0, rho_bar=1e300, c_bar=1e300)
    want = vtrace_host.to_f32(vtrace_host.weights(c["log_prob"], c["old_log_prob"]))
    assert np.array_equal(host_bits(torch, pg), bits(want))
    _, stats = gym_amd.ppo_clip_loss(d["log_prob"][0], d["old_log_prob"][0], one[0])
    torch.cuda.synchronize()
    assert torch.equal(stats[ppo.RATIO_MIN].view(torch.int32), pg.min().view(torch.int32))
    assert torch.equal(stats[ppo.RATIO_MAX].view(torch.int32), pg.max().view(torch.int32))


# ---- the rollout method ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["CartPole-v1", "FrozenLake-v1", "Blackjack-v1"])
def test_rollout_method_equals_the_function_on_the_same_tensors(torch, kind):
    import gym_amd
    from gym_amd._rollout_base import _RolloutBase
    from gym_amd.rollout import DeviceRollout
    from gym_amd.toy_text import BlackjackRollout, TabularRollout

    r = {"CartPole-v1": lambda: DeviceRollout("CartPole-v1", 256, seed=1, action_seed=2),
         "FrozenLake-v1": lambda: TabularRollout("FrozenLake-v1", 256, seed=1, action_seed=2),
         "Blackjack-v1": lambda: BlackjackRollout(256, seed=1, action_seed=2)}[kind]()
    assert isinstance(r, _RolloutBase)
    r.reset(seed=3)
    K, n = 16, r.num_envs
    traj = r.rollout_per_step(K, out=r.trajectory_buffers(K, layout="separate"))
    g = torch.Generator(device="cuda:0").manual_seed(5)
    values, final_values, old = (torch.randn((K, n), device="cuda:0", generator=g) for _ in range(3))
    lp = old + 0.5 * torch.randn((K, n), device="cuda:0", generator=g)
    last_value = torch.randn(n, device="cuda:0", generator=g)
    kw = dict(gamma=0.98, lam=0.9, rho_bar=1.0, c_bar=1.5, pg_rho_bar=2.0, final_values=final_values)
    got = r.vtrace(traj, values, lp, old, last_value, **kw)
    torch.cuda.synchronize()
    assert int(traj["terminated"].sum() + traj["truncated"].sum()) > 0
    want = gym_amd.vtrace(lp, old, traj["reward"], traj["terminated"], traj["truncated"], values, last_value, **kw)
    host = lambda x: x.cpu().numpy()
    twin = vtrace_host.vtrace(host(lp), host(old), host(traj["reward"]), host(traj["terminated"]), host(traj["truncated"]), host(values),
                              host(last_value), **dict(kw, final_values=host(final_values)))
    for a, b, w in zip(got, want, twin):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and np.array_equal(host_bits(torch, a), bits(w))
    out = (torch.empty_like(got[0]), torch.empty_like(got[1]))
    again = r.vtrace(traj, values, lp, old, last_value, out=out, **kw)
    assert again[0] is out[0] and again[1] is out[1] and torch.equal(out[1].view(torch.int32), got[1].view(torch.int32))
    r.close()


# ---- graph capture, autograd ---------------------------------------------------------------------------------------------------------------------
def test_one_capture_replayed_on_changed_inputs(torch):
    import gym_amd

    K, N = 9, 1500
    cases = [make_case(K, N, 800 + i) for i in range(3)]
    d = {k: dev(torch, v) for k, v in cases[0].items()}
    out = (torch.empty((K, N), device="cuda:0"), torch.empty((K, N), device="cuda:0"))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):       # a warm-up launch outside the capture
        call(gym_amd.vtrace, d, out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(gym_amd.vtrace, d, out=out)
    for c in cases[1:]:
        for k, v in c.items():
            d[k].copy_(dev(torch, v))
        out[0].zero_()
        out[1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        compare(torch, out, call(vtrace_host.vtrace, c), "replay")


def test_inputs_that_require_grad_give_outputs_without_a_graph(torch):
    import gym_amd

    c = make_case(5, 70, 850)
    d = {k: dev(torch, v) for k, v in c.items()}
    leaf = d["log_prob"].clone().requires_grad_(True)
    g = dict(d, log_prob=leaf * 1.0, values=d["values"].clone().requires_grad_(True), last_value=d["last_value"].clone().requires_grad_(True))
    assert g["log_prob"].grad_fn is not None
    got = call(gym_amd.vtrace, g)
    assert all(not x.requires_grad and x.grad_fn is None for x in got)
    compare(torch, got, call(vtrace_host.vtrace, c))
    with pytest.raises(ValueError, match="requires grad"):
        call(gym_amd.vtrace, d, out=(torch.empty((5, 70), device="cuda:0", requires_grad=True), torch.empty((5, 70), device="cuda:0")))
