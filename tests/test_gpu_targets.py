"""gym_amd.dqn_targets, categorical_targets and quantile_targets on the device (include/mxv_targets.h): bit-equal to the
NumPy twin tests/targets_host.py at every shape at which the kernels take another path — a partial tile, a full one, one row past it,
one row past 65 536 tiles where the grid grows along y; for the lane-per-row kernel one wave, one row past it and more than one
workgroup — with gamma= and with discount=, with and without the online selector, with poisoned rows; bit-equal to what the EXISTING
kernels compute (projected= of the fused categorical loss, targets_out= of the fused quantile loss, the loss, stats and gradient of the
scalar loss); the chain with the n-step prioritised buffer; graph capture; the example."""
import os
import sys

import numpy as np
import pytest

import c51_host as ch
import targets_host as th
from conftest import ROOT
from targets_host import bits, to_f32
from test_gpu_ppo import _captured_launches, _hip

pytestmark = pytest.mark.gpu

V_MIN, V_MAX = -10.0, 10.0
G32 = np.float32(0.99)
G2 = np.float32(np.float64(G32) * np.float64(G32))
THREE = np.array([G32, G2, np.float32(np.float64(G2) * np.float64(G32))], np.float32)      # as the n-step ring forms them
CHUNK = 1 << 15      # rows of the twin at a time at the large size


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host_bits(torch, x):
    return x.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1)


def _same32(torch, got, want32, what):
    assert got.dtype == torch.float32, what
    want = bits(np.asarray(want32, np.float32).reshape(-1))
    have = host_bits(torch, got)
    bad = np.flatnonzero(have != want) if have.shape == want.shape else None
    assert have.shape == want.shape and bad.size == 0, (what, bad[:8], have[bad[:8]], want[bad[:8]])


def make_batch(M, A, W, seed, poison=True):
    """M rows of A actions of W atoms or quantiles.  Cycling through the rows when `poison`: a NaN, a +Inf, a -Inf in the next rows or
    in the selector, a row of -Inf, a NaN reward, a NaN and an infinite discount — on running and on terminated rows alike."""
    rng = np.random.default_rng(seed)
    nxt = (rng.standard_normal((M, A, W)) * 2.0).astype(np.float32)
    online = (nxt + 0.7 * rng.standard_normal((M, A, W))).astype(np.float32)
    reward = rng.standard_normal(M).astype(np.float32)
    term = (rng.uniform(size=M) < 0.25).astype(np.uint8)
    discount = THREE[rng.integers(0, 3, M)].copy()
    k = np.arange(M)
    far = k % 11 == 5
    reward[far] = rng.choice(np.array([-50.0, 50.0, 10.0, -10.0], np.float32), far.sum())
    if poison and M >= 3:
        slot = k % 16
        nxt[slot == 1, rng.integers(0, A), rng.integers(0, W)] = np.nan
        online[slot == 2, rng.integers(0, A), rng.integers(0, W)] = np.inf
        nxt[slot == 3, rng.integers(0, A), rng.integers(0, W)] = -np.inf
        nxt[slot == 4, rng.integers(0, A)] = -np.inf
        online[slot == 4] = nxt[slot == 4]
        reward[slot == 6] = np.nan
        discount[slot == 7] = np.nan
        discount[slot == 8] = np.inf
        discount[slot == 9] = 0.0
        term[slot == 1] = k[slot == 1] % 32 == 1      # half of each kind of poisoned row is terminated
        term[slot == 7] = k[slot == 7] % 32 == 7
    return dict(next=nxt, online=online, reward=reward, term=term, discount=discount)


def factor(b, how):
    return dict(gamma=0.96875) if how == "gamma" else dict(gamma=0.99) if how == "gamma99" else dict(discount=b["discount"])


def factor_dev(torch, b, how):
    return {k: (dev(torch, v) if k == "discount" else v) for k, v in factor(b, how).items()}


OPTIONS = tuple((how, double) for how in ("gamma", "discount") for double in (False, True))


# ---- 1. bit-equal to the twin -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,Z", ((1, 2), (2, 51), (7, 64), (64, 2), (7, 51)))
@pytest.mark.parametrize("M", (1, 3, 4, 5, 37))
def test_categorical_targets_and_the_clipped_mass_match_the_twin(torch, M, A, Z):
    import gym_amd

    b = make_batch(M, A, Z, 100 * M + A + Z)
    d = {k: dev(torch, v) for k, v in b.items()}
    for how, double in OPTIONS:
        want_m, want_cm = th.c51_f32(b["next"], b["reward"], b["term"], v_min=V_MIN, v_max=V_MAX, next_logits_online=b["online"] if double else None,
                                     **factor(b, how))
        cm = torch.full((M,), 7.0, device="cuda:0")
        got = gym_amd.categorical_targets(d["next"], d["reward"], d["term"], v_min=V_MIN, v_max=V_MAX, next_logits_online=d["online"] if double else None,
                                          clipped_mass=cm, **factor_dev(torch, b, how))
        assert tuple(got.shape) == (M, Z) and not got.requires_grad
        _same32(torch, got, want_m, (M, A, Z, how, double, "m"))
        _same32(torch, cm, want_cm, (M, A, Z, how, double, "cm"))


@pytest.mark.parametrize("A,N", ((1, 1), (2, 32), (7, 64), (64, 1), (3, 51)))
@pytest.mark.parametrize("M", (1, 3, 4, 5, 37))
def test_quantile_targets_match_the_twin(torch, M, A, N):
    import gym_amd

    b = make_batch(M, A, N, 200 * M + A + N)
    d = {k: dev(torch, v) for k, v in b.items()}
    for how, double in OPTIONS:
        want = th.qr_f32(b["next"], b["reward"], b["term"], next_quantiles_online=b["online"] if double else None, **factor(b, how))
        got = gym_amd.quantile_targets(d["next"], d["reward"], d["term"], next_quantiles_online=d["online"] if double else None,
                                       **factor_dev(torch, b, how))
        assert tuple(got.shape) == (M, N)
        _same32(torch, got, want, (M, A, N, how, double))


@pytest.mark.parametrize("A", (1, 2, 7, 64))
@pytest.mark.parametrize("M", (1, 63, 64, 65, 257))
def test_dqn_targets_match_the_twin(torch, M, A):
    import gym_amd

    b = make_batch(M, A, 1, 300 * M + A)
    b["next"], b["online"] = b["next"][:, :, 0], b["online"][:, :, 0]
    d = {k: dev(torch, v) for k, v in b.items()}
    for how, double in OPTIONS:
        want = th.dqn_f32(b["next"], b["reward"], b["term"], next_q_online=b["online"] if double else None, **factor(b, how))
        got = gym_amd.dqn_targets(d["next"], d["reward"], d["term"], next_q_online=d["online"] if double else None, **factor_dev(torch, b, how))
        assert tuple(got.shape) == (M,)
        _same32(torch, got, want, (M, A, how, double))


def test_one_row_past_65536_tiles_where_the_grid_grows_along_y(torch):
    import gym_amd

    M = 262145
    b = make_batch(M, 2, 2, 5)
    d = {k: dev(torch, v) for k, v in b.items()}
    cm = torch.empty(M, device="cuda:0")
    got = gym_amd.categorical_targets(d["next"], d["reward"], d["term"], v_min=V_MIN, v_max=V_MAX, discount=d["discount"], next_logits_online=d["online"],
                                      clipped_mass=cm)
    gq = gym_amd.quantile_targets(d["next"][:, :, :1].contiguous(), d["reward"], d["term"], discount=d["discount"],
                                  next_quantiles_online=d["online"][:, :, :1].contiguous())
    gd = gym_amd.dqn_targets(d["next"][:, :, 0].contiguous(), d["reward"], d["term"], discount=d["discount"])
    have_m, have_cm, have_q, have_d = (host_bits(torch, x) for x in (got, cm, gq, gd))
    for lo in range(0, M, CHUNK):
        s = slice(lo, min(lo + CHUNK, M))
        want_m, want_cm = th.c51_f32(b["next"][s], b["reward"][s], b["term"][s], v_min=V_MIN, v_max=V_MAX, discount=b["discount"][s],
                                     next_logits_online=b["online"][s])
        assert np.array_equal(have_m[2 * s.start:2 * s.stop], bits(want_m.reshape(-1))) and np.array_equal(have_cm[s], bits(want_cm)), lo
        want_q = th.qr_f32(b["next"][s][:, :, :1], b["reward"][s], b["term"][s], discount=b["discount"][s], next_quantiles_online=b["online"][s][:, :, :1])
        assert np.array_equal(have_q[s], bits(want_q.reshape(-1))), lo
        assert np.array_equal(have_d[s], bits(th.dqn_f32(b["next"][s][:, :, 0], b["reward"][s], b["term"][s], discount=b["discount"][s]))), lo


def test_a_poisoned_row_changes_no_other_row(torch):
    import gym_amd

    M, A, Z = 37, 3, 51
    clean, dirty = make_batch(M, A, Z, 9, poison=False), make_batch(M, A, Z, 9, poison=True)
    same = np.array([all(np.array_equal(clean[k][i], dirty[k][i], equal_nan=True) for k in clean) for i in range(M)])
    assert 5 < same.sum() < M - 5
    rows = {}
    for name, b in (("clean", clean), ("dirty", dirty)):
        d = {k: dev(torch, v) for k, v in b.items()}
        rows[name] = (gym_amd.categorical_targets(d["next"], d["reward"], d["term"], v_min=V_MIN, v_max=V_MAX, discount=d["discount"], next_logits_online=d["online"]),
                      gym_amd.quantile_targets(d["next"], d["reward"], d["term"], discount=d["discount"], next_quantiles_online=d["online"]),
                      gym_amd.dqn_targets(d["next"][:, :, 0].contiguous(), d["reward"], d["term"], discount=d["discount"],
                                          next_q_online=d["online"][:, :, 0].contiguous()))
    keep = dev(torch, same)
    for c, x in zip(rows["clean"], rows["dirty"]):
        assert torch.equal(c[keep].view(torch.int32), x[keep].view(torch.int32))
        nan = x.view(torch.int32)[torch.isnan(x)]
        assert nan.numel() > 0 and bool((nan == 0x7FC00000).all())      # every NaN written is the one pattern


@pytest.mark.parametrize("A,W", ((3, 51), (7, 33)))
def test_strided_rows_leading_dims_flag_dtypes_and_out(torch, A, W):
    import gym_amd

    K, N = 3, 5
    M = K * N
    b = make_batch(M, A, W, 77)
    want_m, want_cm = th.c51_f32(b["next"], b["reward"], b["term"], v_min=V_MIN, v_max=V_MAX, discount=b["discount"], next_logits_online=b["online"])
    want_T = th.qr_f32(b["next"], b["reward"], b["term"], discount=b["discount"], next_quantiles_online=b["online"])
    want_y = th.dqn_f32(b["next"][:, :, 0], b["reward"], b["term"], discount=b["discount"], next_q_online=b["online"][:, :, 0])
    d = {k: dev(torch, v) for k, v in b.items()}
    # rows that are views into a wider buffer, the next rows and the selector with different strides
    wide = torch.full((M, A * W + 13), float("nan"), device="cuda:0")
    wide[:, 5:5 + A * W] = d["next"].view(M, -1)
    wide2 = torch.full((M, 2 * A * W), float("nan"), device="cuda:0")
    wide2[:, A * W:] = d["online"].view(M, -1)
    nx, on = wide[:, 5:5 + A * W].unflatten(1, (A, W)), wide2[:, A * W:].unflatten(1, (A, W))
    assert not nx.is_contiguous() and nx.stride(0) != on.stride(0)
    for flags in (d["term"], d["term"].bool()):
        _same32(torch, gym_amd.categorical_targets(nx, d["reward"], flags, v_min=V_MIN, v_max=V_MAX, discount=d["discount"], next_logits_online=on), want_m, "c51")
        _same32(torch, gym_amd.quantile_targets(nx, d["reward"], flags, discount=d["discount"], next_quantiles_online=on), want_T, "qr")
    wq = torch.full((M, A + 3), float("nan"), device="cuda:0")
    wq[:, 1:1 + A] = d["next"][:, :, 0]
    _same32(torch, gym_amd.dqn_targets(wq[:, 1:1 + A], d["reward"], d["term"].bool(), discount=d["discount"], next_q_online=d["online"][:, :, 0].contiguous()),
            want_y, "dqn")
    # [K, N, ...] leading dims, out= given
    lead = lambda x: x.view(K, N, *x.shape[1:])
    out_m, out_cm = torch.empty((K, N, W), device="cuda:0"), torch.empty((K, N), device="cuda:0")
    got = gym_amd.categorical_targets(lead(d["next"]), lead(d["reward"]), lead(d["term"]), v_min=V_MIN, v_max=V_MAX, discount=lead(d["discount"]),
                                      next_logits_online=lead(d["online"]), clipped_mass=out_cm, out=out_m)
    assert got is out_m
    _same32(torch, out_m, want_m, "lead c51")
    _same32(torch, out_cm, want_cm, "lead cm")
    out_T = torch.empty((K, N, W), device="cuda:0")
    assert gym_amd.quantile_targets(lead(d["next"]), lead(d["reward"]), lead(d["term"]), discount=lead(d["discount"]),
                                    next_quantiles_online=lead(d["online"]), out=out_T) is out_T
    _same32(torch, out_T, want_T, "lead qr")
    out_y = torch.empty((K, N), device="cuda:0")
    assert gym_amd.dqn_targets(lead(d["next"][:, :, 0].contiguous()), lead(d["reward"]), lead(d["term"]), discount=lead(d["discount"]),
                               next_q_online=lead(d["online"][:, :, 0].contiguous()), out=out_y) is out_y
    _same32(torch, out_y, want_y, "lead dqn")
    # inputs that require grad are read detached; the result carries no graph
    nx_g = d["next"].clone().requires_grad_()
    got = gym_amd.categorical_targets(nx_g, d["reward"], d["term"], v_min=V_MIN, v_max=V_MAX, discount=d["discount"], next_logits_online=d["online"])
    assert not got.requires_grad and got.grad_fn is None
    _same32(torch, got, want_m, "detached")
    with pytest.raises(ValueError, match="overlaps"):
        gym_amd.dqn_targets(d["next"][:, :, 0].contiguous(), d["reward"], d["term"], out=d["reward"])
    with pytest.raises(ValueError, match="out must have shape"):
        gym_amd.quantile_targets(d["next"], d["reward"], d["term"], out=torch.empty((M, W + 1), device="cuda:0"))


# ---- 2. against the existing kernels, not the twin -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,A,Z", ((5, 2, 51), (37, 7, 64), (1030, 3, 51)))
def test_categorical_targets_have_the_bits_of_the_fused_loss_projection(torch, M, A, Z):
    """With a scalar gamma: projected= of the fused bootstrap at that gamma.  With discounts of three values (gamma, float32(gamma gamma),
    float32 of that times gamma, as the ring forms them): group by group, projected= at gamma = float(d).  The clipped mass: the fused
    loss writes float32(tree_sum(cm_i) / M) of the float64 cm_i; here each cm_i is rounded to float32 first (relative 2^-24 each, so
    2^-24 of their mean), summed in float64 in whatever order (M 2^-53 relative, twice for the tree's own), and the fused figure is itself
    rounded to float32 (2^-24): |difference| <= (2 * 2^-24 + M * 2^-52) * mean(cm) + 2^-149."""
    import gym_amd

    b = make_batch(M, A, Z, 400 + M)
    rng = np.random.default_rng(M)
    logits = dev(torch, rng.standard_normal((M, A, Z)).astype(np.float32))
    act = dev(torch, rng.integers(0, A, M))
    d = {k: dev(torch, v) for k, v in b.items()}

    def fused(gamma, online):
        proj = torch.empty((M, Z), device="cuda:0")
        _, stats = gym_amd.categorical_dqn_loss(logits, act, v_min=V_MIN, v_max=V_MAX, reward=d["reward"], terminated=d["term"], next_logits=d["next"],
                                                next_logits_online=online, gamma=gamma, projected=proj)
        return proj, stats

    for online in (None, d["online"]):
        for gamma in (0.99, 0.5):
            proj, stats = fused(gamma, online)
            cm = torch.empty(M, device="cuda:0")
            got = gym_amd.categorical_targets(d["next"], d["reward"], d["term"], v_min=V_MIN, v_max=V_MAX, gamma=gamma, next_logits_online=online, clipped_mass=cm)
            assert torch.equal(got.view(torch.int32), proj.view(torch.int32)), (gamma, online is None)
        three = dev(torch, THREE[rng.permutation(M) % 3])      # every value is in the batch, also at five rows
        got = gym_amd.categorical_targets(d["next"], d["reward"], d["term"], v_min=V_MIN, v_max=V_MAX, discount=three, next_logits_online=online)
        for v in THREE:
            rows = three == float(v)
            proj, _ = fused(float(v), online)
            assert int(rows.sum()) > 0 and torch.equal(got[rows].view(torch.int32), proj[rows].view(torch.int32)), (float(v), online is None)
    # the clipped mass against the fused diagnostic, on rows without a NaN
    c = make_batch(M, A, Z, 500 + M, poison=False)
    d = {k: dev(torch, v) for k, v in c.items()}
    _, stats = fused(0.99, d["online"])
    cm = torch.empty(M, device="cuda:0")
    gym_amd.categorical_targets(d["next"], d["reward"], d["term"], v_min=V_MIN, v_max=V_MAX, gamma=0.99, next_logits_online=d["online"], clipped_mass=cm)
    mine, theirs = float(cm.double().mean()), float(stats[gym_amd.c51.CLIPPED_MASS_MEAN].double())
    bound = (2 * 2.0 ** -24 + M * 2.0 ** -52) * mine + 2.0 ** -149
    print(f"clipped mass mean: targets {mine!r}, fused {theirs!r}, |difference| {abs(mine - theirs):.3e}, bound {bound:.3e}")
    assert mine > 0.0 and abs(mine - theirs) <= bound


@pytest.mark.parametrize("M,A,N", ((5, 2, 32), (37, 7, 64), (1030, 3, 51)))
def test_quantile_targets_have_the_bits_of_the_fused_loss_targets_out(torch, M, A, N):
    import gym_amd

    b = make_batch(M, A, N, 600 + M)
    rng = np.random.default_rng(M)
    quantiles = dev(torch, rng.standard_normal((M, A, N)).astype(np.float32))
    act = dev(torch, rng.integers(0, A, M))
    d = {k: dev(torch, v) for k, v in b.items()}
    for online in (None, d["online"]):
        for kw in (dict(discount=d["discount"]), dict(gamma=0.99)):
            T = torch.empty((M, N), device="cuda:0")
            gym_amd.quantile_dqn_loss(quantiles, act, reward=d["reward"], terminated=d["term"], next_quantiles=d["next"], next_quantiles_online=online,
                                      targets_out=T, **kw)
            got = gym_amd.quantile_targets(d["next"], d["reward"], d["term"], next_quantiles_online=online, **kw)
            assert torch.equal(got.view(torch.int32), T.view(torch.int32)), (list(kw), online is None)


@pytest.mark.parametrize("M,A", ((65, 2), (257, 7), (1500, 4)))
def test_dqn_loss_on_dqn_targets_has_the_bits_of_its_bootstrap_mode(torch, M, A):
    """Rewards in {-1, 0, 1, 2}, next_q multiples of 1/8 in [-4, 4], discounts in {1, 0.5, 0.25}: every y is a multiple of 1/32 below 8 in
    magnitude, exact in float32, so handing it over as float32 loses nothing: the loss, the stats and the gradient of each discount
    group are those of the bootstrap mode at that scalar gamma, bit for bit."""
    import gym_amd

    rng = np.random.default_rng(M + A)
    nq = (rng.integers(-32, 33, (M, A)) / 8.0).astype(np.float32)
    on = (rng.integers(-32, 33, (M, A)) / 8.0).astype(np.float32)
    reward = rng.integers(-1, 3, M).astype(np.float32)
    term = (rng.uniform(size=M) < 0.2).astype(np.uint8)
    disc = np.array([1.0, 0.5, 0.25], np.float32)[rng.integers(0, 3, M)]
    q = (rng.standard_normal((M, A))).astype(np.float32)
    act = rng.integers(0, A, M)
    weights = rng.uniform(0.2, 2.0, M).astype(np.float32)
    nq_d, on_d, r_d, t_d, disc_d, q_d, a_d, w_d = (dev(torch, x) for x in (nq, on, reward, term, disc, q, act, weights))
    for online in (None, on_d):
        y = gym_amd.dqn_targets(nq_d, r_d, t_d, discount=disc_d, next_q_online=online)
        for v in (1.0, 0.5, 0.25):
            rows = disc_d == v
            assert int(rows.sum()) > 3
            results = []
            for kw in (dict(targets=y[rows]),
                       dict(reward=r_d[rows], terminated=t_d[rows], next_q=nq_d[rows], next_q_online=None if online is None else online[rows], gamma=v)):
                qq = q_d[rows].clone().requires_grad_()
                td = torch.empty(int(rows.sum()), device="cuda:0")
                loss, stats = gym_amd.dqn_loss(qq, a_d[rows], weights=w_d[rows], td_error=td, **kw)
                (loss * 2.5).backward()
                results.append((loss.detach(), stats, td, qq.grad))
            for given, boot in zip(*results):
                assert torch.equal(given.view(torch.int32), boot.view(torch.int32)), (v, online is None)


# ---- 3. the chain with the n-step prioritised buffer ----------------------------------------------------------------------------------------------
def test_nstep_sample_targets_loss_equals_the_twin_chain(torch):
    """An NStepPrioritizedReplayBuffer filled from one CartPole chunk of K = 8 steps with n = 3: sample -> categorical_targets(discount=
    batch["discount"]) -> categorical_dqn_loss(target_probs=) equals targets_host.c51 -> c51_host.loss_f32 on the sampled rows, bit for
    bit; rows cut at the chunk's end carry gamma^1 or gamma^2."""
    import gym_amd
    from gym_amd.rollout import DeviceRollout

    N, K, n, gamma, A, Z, B = 300, 8, 3, 0.99, 2, 51, 512
    env = DeviceRollout("CartPole-v1", N, seed=3, action_seed=4)
    env.reset(seed=3)
    sampler = env.policy_sampler()
    buf = env.nstep_replay_buffer(4096, n, gamma, prioritized=True)
    f32 = dict(dtype=torch.float32, device=env.device)
    traj = {"obs": torch.empty((K, N, 4), **f32), "final_obs": torch.zeros((K, N, 4), **f32),
            "actions": torch.empty((K, N), dtype=env.action_dtype, device=env.device), "reward": torch.empty((K, N), dtype=env.reward_dtype, device=env.device),
            "terminated": torch.empty((K, N), dtype=torch.uint8, device=env.device), "truncated": torch.empty((K, N), dtype=torch.uint8, device=env.device)}
    with torch.cuda.stream(env.stream):
        first = env.obs.clone()
        for k in range(K):
            actions = sampler.sample(torch.zeros((N, A), **f32))[0]
            env.step(actions)
            for name, src in (("actions", actions), ("obs", env.obs), ("final_obs", env.final_obs), ("reward", env.reward), ("terminated", env.terminated),
                              ("truncated", env.truncated)):
                traj[name][k].copy_(src)
        buf.add_chunk(first, traj)
        batch = buf.sample(B, beta=0.5)
        # a fixed head: logits from the observation, in torch
        Wm = torch.cos(torch.arange(4 * A * Z, **f32).view(4, A * Z) * 1.3)
        head = lambda obs, s: ((obs @ Wm) * s).view(-1, A, Z).contiguous()
        nxt, online, logits = head(batch["next_obs"], 1.0), head(batch["next_obs"], 1.7), head(batch["obs"], 0.6)
        cm, row_loss = torch.empty(B, **f32), torch.empty(B, **f32)
        m = gym_amd.categorical_targets(nxt, batch["reward"], batch["terminated"], v_min=0.0, v_max=20.0, discount=batch["discount"],
                                        next_logits_online=online, clipped_mass=cm)
        loss, stats = gym_amd.categorical_dqn_loss(logits, batch["actions"], v_min=0.0, v_max=20.0, target_probs=m, weights=batch["weights"], row_loss=row_loss)
        env.stream.synchronize()
    host = {k: v.cpu().numpy() for k, v in batch.items()}
    disc = host["discount"]
    assert len(np.unique(disc)) == 3 and 0.0 < disc.min() < disc.max() <= np.float32(gamma)      # windows cut at the chunk's end carry gamma^1 or gamma^2
    want_m, want_cm = th.c51_f32(nxt.cpu().numpy(), host["reward"], host["terminated"], v_min=0.0, v_max=20.0, discount=disc,
                                 next_logits_online=online.cpu().numpy())
    _same32(torch, m, want_m, "m")
    _same32(torch, cm, want_cm, "cm")
    want = ch.loss_f32(logits.cpu().numpy(), host["actions"], v_min=0.0, v_max=20.0, target_probs=want_m, weights=host["weights"])
    _same32(torch, loss, [want[0]], "loss")
    _same32(torch, stats, want[1], "stats")
    _same32(torch, row_loss, want[2], "row_loss")
    assert np.isfinite(want[2]).all()
    env.close()


# ---- 4. graph capture ---------------------------------------------------------------------------------------------------------------------------
def test_the_three_calls_replay_in_a_captured_graph_with_one_kernel_node_each(torch):
    import gym_amd
    from gym_amd import targets

    M, A, W = 1030, 3, 51
    batches = [make_batch(M, A, W, 40 + k) for k in range(3)]
    keys = ("next", "online", "reward", "term", "discount")
    bufs = {k: dev(torch, batches[0][k]) for k in keys}
    nq, onq = torch.empty((M, A), device="cuda:0"), torch.empty((M, A), device="cuda:0")
    out_m, out_cm, out_T, out_y = (torch.empty(s, device="cuda:0") for s in ((M, W), (M,), (M, W), (M,)))

    def step():
        gym_amd.categorical_targets(bufs["next"], bufs["reward"], bufs["term"], v_min=V_MIN, v_max=V_MAX, discount=bufs["discount"],
                                    next_logits_online=bufs["online"], clipped_mass=out_cm, out=out_m)
        gym_amd.quantile_targets(bufs["next"], bufs["reward"], bufs["term"], discount=bufs["discount"], next_quantiles_online=bufs["online"], out=out_T)
        gym_amd.dqn_targets(nq, bufs["reward"], bufs["term"], discount=bufs["discount"], next_q_online=onq, out=out_y)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                # warm-up outside the capture
        side.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        step()
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before      # with out= the calls allocate nothing
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            step()
        for k in (0, 1, 2):
            b = batches[k]
            for name in keys:
                bufs[name].copy_(dev(torch, b[name]))
            nq.copy_(bufs["next"][:, :, 0])
            onq.copy_(bufs["online"][:, :, 0])
            g.replay()
            side.synchronize()
            want_m, want_cm = th.c51_f32(b["next"], b["reward"], b["term"], v_min=V_MIN, v_max=V_MAX, discount=b["discount"], next_logits_online=b["online"])
            _same32(torch, out_m, want_m, k)
            _same32(torch, out_cm, want_cm, k)
            _same32(torch, out_T, th.qr_f32(b["next"], b["reward"], b["term"], discount=b["discount"], next_quantiles_online=b["online"]), k)
            _same32(torch, out_y, th.dqn_f32(b["next"][:, :, 0], b["reward"], b["term"], discount=b["discount"], next_q_online=b["online"][:, :, 0]), k)
            eager = (out_m.clone(), out_T.clone(), out_y.clone())
            step()                                                            # the eager calls: the same bits
            side.synchronize()
            for e, x in zip(eager, (out_m, out_T, out_y)):
                assert torch.equal(e.view(torch.int32), x.view(torch.int32))
        # one kernel node a call, counted in a raw stream capture (which also shows that a call neither synchronises nor allocates)
        hip, lib, s = _hip(), targets.lib, side.cuda_stream
        p = {k: v.data_ptr() for k, v in bufs.items()}
        calls = (lambda: lib.mxv_targets_dqn(s, M, A, nq.data_ptr(), A, onq.data_ptr(), A, p["reward"], p["term"], 0.99, p["discount"], out_y.data_ptr()),
                 lambda: lib.mxv_targets_c51(s, M, A, W, p["next"], A * W, p["online"], A * W, p["reward"], p["term"], 0.99, p["discount"], V_MIN, V_MAX,
                                             out_m.data_ptr(), out_cm.data_ptr()),
                 lambda: lib.mxv_targets_qr(s, M, A, W, p["next"], A * W, p["online"], A * W, p["reward"], p["term"], 0.99, p["discount"], out_T.data_ptr()))
        for call in calls:
            rc, n = _captured_launches(hip, s, call)
            assert (rc, n) == (0, 1), (rc, n, lib.mxv_targets_last_error())
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)


# ---- 5. the example -------------------------------------------------------------------------------------------------------------------------------
def test_the_example_repeats_itself(torch, capsys):
    """examples/rainbow_cartpole.py has no torch generator and no float atomic: two runs give the same history, number for number."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import rainbow_cartpole
    finally:
        sys.path.pop(0)
    kw = dict(num_envs=256, iterations=3, K=8, updates=2, batch=128, capacity=4096)
    first = rainbow_cartpole.train(**kw)
    assert "sample steps drawn" in capsys.readouterr().out
    again = rainbow_cartpole.train(**kw, verbose=False)
    assert first == again and len(first) == 3 and first[0]["beta"] == 0.4 and first[-1]["beta"] == 1.0
    for row in first:
        assert np.isfinite(list(row.values())).all() and row["row_loss_max"] >= row["loss_term"] > 0.0 and row["stored"] > 0
        assert 0.0 <= row["clipped_mass_mean"] <= 1.0 and 0.0 < row["discount_min"] <= row["discount_mean"] <= 0.99 + 1e-6
