"""gym_amd/csrc/mxv_subnorm.hip at every edge and on every path, bit for bit against oracle.SubEnvNorm (which tests/test_subnorm_host.py
pins to the literal NumPy twin of the reference on these very inputs: tests/subnorm_host.py holds the input lists).

Comparison: float outputs and all statistics as bit patterns (-0.0 is not +0.0); NaN matches any NaN (x86 and gfx950 sign their default NaN
differently) and may appear only at the envs where the test injected it — that set is asserted exactly.  Outputs are interior slices of
buffers pre-filled with a sentinel bit pattern: the guard elements before and after, and every final_y row of an env that did not finish,
must keep it."""
import numpy as np
import pytest

import subnorm_host as H

pytestmark = pytest.mark.gpu

PAD = 64                                     # guard elements on each side: 256 / 512 bytes, so the interior keeps every alignment
SENTINEL = {4: -1515870811, 8: -6510615555426900571}          # 0xA5A5A5A5 / 0xA5A5A5A5A5A5A5A5 as signed integers: normal negative floats


def _guarded(shape, dtype):
    """(whole buffer as integers, interior float view of `shape`) on the device."""
    import torch

    size = 4 if dtype == torch.float32 else 8
    total = int(np.prod(shape))
    buf = torch.full((total + 2 * PAD,), SENTINEL[size], dtype=torch.int32 if size == 4 else torch.int64, device="cuda")
    return buf, buf[PAD:PAD + total].view(dtype).view(*shape)


def _guards_kept(buf, what):
    g = buf.cpu().numpy()
    s = SENTINEL[g.dtype.itemsize]
    assert (g[:PAD] == s).all() and (g[-PAD:] == s).all(), f"{what}: a write outside the tensor"


def _dev(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _assert_bits(got, ref, what):
    assert H.same_bits(got, ref), f"{what}: {int((H.bits(got) != H.bits(ref)).sum())} elements differ in bits (NaN apart)"


def check_obs(state, x, fin, te, tr, epsilon, f32, final_y=True, nan=frozenset(), inplace=False, handle=None, what=""):
    """One device call against one oracle call on the same arrays; every assertion of the module's docstring.  Returns the device's
    (y, final_y, state)."""
    import torch

    from gym_amd import _native

    K, n, D = x.shape
    d = handle or _native.SubNorm(D, n)
    if state is not None:
        d.set_state(*state)
    state = d.get_state()[:3]
    dt = torch.float32 if f32 else torch.float64
    ybuf, y = _guarded((K, n, D), dt)
    if inplace:
        y.copy_(_dev(x))
    fbuf, fy = _guarded((K, n, D), torch.float64) if final_y and fin is not None else (None, None)
    d.observations(K, y if inplace else _dev(x), _dev(fin), _dev(te), _dev(tr), y, f32, fy, epsilon)
    y_o, yf_o, st_o = H.oracle_obs(state, x, fin, te, tr, epsilon, f32, final_y)
    y_d, st_d = y.cpu().numpy(), d.get_state()[:3]
    _guards_kept(ybuf, f"{what} y")
    _assert_bits(y_d, y_o, f"{what} y")
    seen = [(y_d, 1)] + [(a, 0) for a in st_d]
    yf_d = None
    if fy is not None:
        _guards_kept(fbuf, f"{what} final_y")
        done = (te | tr) != 0
        raw = fy.cpu().numpy()
        assert (raw.view(np.int64)[~done] == SENTINEL[8]).all(), f"{what}: a final_y row written for an env that did not finish"
        yf_d = np.where(done[..., None], raw, 0.0)
        _assert_bits(yf_d, yf_o, f"{what} final_y")
        seen.append((yf_d, 1))
    for a, b, name in zip(st_d, st_o, ("mean", "var", "count")):
        _assert_bits(a, b.reshape(a.shape), f"{what} {name}")
    assert H.nan_envs(*seen) == set(nan), f"{what}: NaN at envs {sorted(H.nan_envs(*seen))}, injected at {sorted(nan)}"
    if handle is None:
        d.close()
    return y_d, yf_d, st_d


def check_rew(state, rew, te, tr, gamma, epsilon=1e-8, inplace=False, nan=frozenset(), what=""):
    import torch

    from gym_amd import _native

    K, n = rew.shape
    f32 = rew.dtype == np.float32
    d = _native.SubNorm(1, n)
    if state is not None:
        d.set_state(state[0][:, None], state[1][:, None], state[2], state[3])
    obuf, out = _guarded((K, n), torch.float32 if f32 else torch.float64)
    if inplace:
        out.copy_(_dev(rew))
    d.rewards(K, out if inplace else _dev(rew), f32, _dev(te), _dev(tr), out, gamma, epsilon)
    out_o, st_o = H.oracle_rew(state, rew, te, tr, gamma, epsilon)
    out_d, st_d = out.cpu().numpy(), d.get_state()
    st_d = (st_d[0][:, 0], st_d[1][:, 0], st_d[2], st_d[3])
    _guards_kept(obuf, f"{what} out")
    _assert_bits(out_d, out_o, f"{what} out")
    for a, b, name in zip(st_d, st_o, ("mean", "var", "count", "returns")):
        _assert_bits(a, b, f"{what} {name}")
    seen = H.nan_envs((out_d, 1), *((a, 0) for a in st_d))
    assert seen == set(nan), f"{what}: NaN at envs {sorted(seen)}, injected at {sorted(nan)}"
    d.close()
    return out_d, st_d


# ---- the observation kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", H.DIMS)
@pytest.mark.parametrize("n", H.SIZES)
def test_observation_kernel_at_every_size_dim_step_count_and_flag_pattern(n, D):
    """n on both sides of a wave and of a workgroup (the tail lanes of the last workgroup load env 0's statistics and must write
    nothing), every flag pattern — none, all (2K events per env), step 0 only, step K-1 only, terminated only, truncated only, both, flag
    bytes 2 / 0x80 / 0xFF, one env per wave ending at every step while its 63 neighbours never do (drift = K), odd lanes ending at odd
    steps — with K in 1, 2, 7, 33 and both output dtypes dealt over them; two calls per handle so the second starts from real statistics."""
    from gym_amd import _native

    d = _native.SubNorm(D, n)
    for pattern, K, f32 in H.obs_grid(n, D):
        x, fin = H.rows(D, K, n)
        te, tr = H.flags(pattern, K, n, np.random.default_rng(K))
        check_obs(None, x, fin, te, tr, 1e-8, f32, handle=d, what=f"{pattern} K={K} f32={f32}")
    d.close()


@pytest.mark.parametrize("D", H.DIMS)
def test_observation_kernel_call_forms(D):
    """final without final_y (the statistics still take the terminal row); flags without final (ignored: the oracle called with
    fin = None); the reset form; float32 in place (y is x) at K = 7 under maximum drift, where drifted lanes read and write different
    [N] slices."""
    n, K = 257, 7
    x, fin = H.rows(D, K, n)
    te, tr = H.flags("drift", K, n, None)
    te[2::3, 70::9] = 1
    _, _, st = check_obs(None, x, fin, te, tr, 1e-8, True, final_y=False, what="final without final_y")
    _, _, st_full = check_obs(None, x, fin, te, tr, 1e-8, True, what="final with final_y")
    assert all(H.same_bits(a, b) for a, b in zip(st, st_full))
    y1, _, st1 = check_obs(None, x, None, te, tr, 1e-8, False, what="flags without final")
    y0, _, st0 = check_obs(None, x, None, None, None, 1e-8, False, what="reset form")
    assert H.same_bits(y0, y1) and all(H.same_bits(a, b) for a, b in zip(st0, st1))
    assert not H.same_bits(st0[0], st_full[0])                                          # (the terminal rows do count where they are given)
    y_in, yf_in, _ = check_obs(None, x, fin, te, tr, 1e-8, True, inplace=True, what="in place")
    y_out, yf_out, _ = check_obs(None, x, fin, te, tr, 1e-8, True, what="out of place")
    assert H.same_bits(y_in, y_out) and H.same_bits(yf_in, yf_out)


@pytest.mark.parametrize("D", H.DIMS)
def test_observation_kernel_is_invariant_under_splitting_the_steps(D):
    """One call of K = 16, sixteen calls of K = 1, and calls of 5 + 11 under the maximum-drift pattern: the same output bits, the same
    statistics bits."""
    from gym_amd import _native

    n, K = 257, 16
    x, fin = H.rows(D, K, n)
    te, tr = H.flags("drift", K, n, None)
    tr[3::4, 1::7] = 1
    results = []
    for cuts in ([0, 16], list(range(17)), [0, 5, 16]):
        d = _native.SubNorm(D, n)
        ys, fs = [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            y, yf, st = check_obs(None, x[a:b], fin[a:b], te[a:b], tr[a:b], 1e-8, False, handle=d, what=f"steps {a}..{b}")
            ys.append(y), fs.append(yf)
        results.append((np.concatenate(ys), np.concatenate(fs), st))
        d.close()
    for y, yf, st in results[1:]:
        assert H.same_bits(y, results[0][0]) and H.same_bits(yf, results[0][1])
        assert all(H.same_bits(a, b) for a, b in zip(st, results[0][2]))


@pytest.mark.parametrize("K", [1, 6])
@pytest.mark.parametrize("D", [1, 4])
def test_observation_kernel_on_every_guard_path(D, K):
    """Constructed statistics (tests/subnorm_host.py: obs_guard_case): extremes among ordinary lanes and alone, one lane and a whole wave
    whose M2 fails the second vote, lanes whose delta alone fails the first.  The twin's path report on exactly the uploaded arrays says
    that the short path, the plain `/` path and the M2 branch are each taken by a mixed and by an unmixed wave-iteration; the lanes that
    fail a vote alone carry dividends on which div_shared and `/` differ, so a guard that lets them through changes the stored bits."""
    state, x, fin, te, tr = H.obs_guard_case(D, K)
    report = H.obs_walk(*state, x, fin, te, tr, 1e-8)[4]
    assert H.paths_taken(report) == H.EVERY_PATH_BOTH_WAYS
    for f32 in (True, False):
        check_obs(state, x, fin, te, tr, 1e-8, f32, nan=H.GUARD_NAN_ENVS, what=f"guard paths f32={f32}")


@pytest.mark.parametrize("D", H.DIMS)
def test_observation_kernel_edge_rows_among_ordinary_ones(D):
    """At lanes 0, 63 and 64 of 130 envs: +-Inf and NaN components (the neighbours stay exact), -0.0 on fresh statistics, rows equal to the
    mean, float64 results below 2^-126 (float32 subnormal, rounded once) and above float32's maximum (Inf), epsilon = 0 with var = 0 and
    with a negative var, and the m_b cases: injected count = -0.0, and count = -0.5 with var = 0, where the reference's `+ m_b` makes the
    stored var +0.0."""
    for name, (state, x, eps, nan) in H.obs_edge_cases(D).items():
        for f32 in (True, False):
            _, _, st = check_obs(state, x, None, None, None, eps, f32, nan=nan, what=f"{name} f32={f32}")
        if name.startswith("count_minus"):
            _, _, st = check_obs(state, x[:1], None, None, None, eps, False, nan=nan, what=f"{name}, one step")
            assert (H.bits(st[1][list(H.EDGE_LANES)]) == 0).all(), f"{name}: var is not +0.0"


# ---- the reward kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", H.SIZES)
def test_reward_kernel_at_every_size_and_flag_pattern(n):
    """The same sizes and flag patterns; float32 and float64 rewards, K in 1, 9, in place and out of place into guarded buffers, and
    gamma in 0, 0.97, 1, -0.5 dealt over them."""
    for pattern, K, f32, inplace, gamma in H.rew_grid(n):
        te, tr = H.flags(pattern, K, n, np.random.default_rng(K))
        check_rew(None, H.rewards_for(K, n, f32), te, tr, gamma, inplace=inplace, what=f"{pattern} K={K} f32={f32} inplace={inplace} gamma={gamma}")


@pytest.mark.parametrize("f32", [True, False])
def test_reward_kernel_edge_rewards_among_ordinary_ones(f32):
    """Every gamma; gamma = 2 from returns of 1e306, which pass float64's maximum inside K = 9 (the later steps of that env run on Inf and
    NaN while its wave neighbours stay exact); rewards of -0.0 (the output's sign is compared); a NaN reward at one env."""
    n = H.EDGE_N
    for name, (rew, gamma, start, nan) in H.rew_edge_cases(f32).items():
        te, tr = H.flags("terminated", 9, n, np.random.default_rng(3))
        te[:, list(H.EDGE_LANES)] = 0
        for inplace in (False, True):
            out, _ = check_rew((np.zeros(n), np.ones(n), np.full(n, 1e-4), start), rew, te, tr, gamma, inplace=inplace, nan=nan, what=name)
        if name == "minus_zero_rewards":
            assert np.signbit(out[:, list(H.EDGE_LANES)]).all()


@pytest.mark.parametrize("K", [1, 6])
@pytest.mark.parametrize("f32", [True, False])
def test_reward_kernel_on_every_guard_path(f32, K):
    """The guard-path statistics through set_state, returns included (tests/subnorm_host.py: rew_guard_case); the path conditions asserted
    on the uploaded arrays (K = 1 is a single iteration with every lane at work, where a mixed short path cannot exist); all four state
    arrays compared by bits."""
    state, rew, te, tr, gamma = H.rew_guard_case(K, f32)
    report = H.rew_walk(*state, rew, te, tr, gamma, 1e-8)[2]
    assert H.paths_taken(report) == H.EVERY_PATH_BOTH_WAYS - ({(H.SHORT, True)} if K == 1 else set())
    for inplace in (False, True):
        check_rew(state, rew, te, tr, gamma, inplace=inplace, nan=H.GUARD_NAN_ENVS, what=f"guard paths inplace={inplace}")


# ---- the front ends at the other dims -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,D", [("MountainCar-v0", 2), ("Pendulum-v1", 3), ("Acrobot-v1", 6)])
def test_make_device_and_host_statistics_agree_bit_for_bit_at_the_other_dims(env_id, D):
    """tests/test_gpu_subnorm.py's device-against-host test of the wrappers (CartPole, D = 4, at SUBENV_DEVICE_MIN) at D = 2, 3 and 6:
    device=True against device=False over identically seeded engines, a few hundred envs, episodes of 5 steps so that well over 100 end."""
    import gym_amd
    from gym_amd import wrappers as W

    n = 300
    mk = lambda dev: W.SubEnvNormalizeReward(W.SubEnvNormalizeObservation(gym_amd.make(env_id, num_envs=n, max_episode_steps=5), device=dev),
                                             device=dev)        # noqa: E731
    a, b = mk(True), mk(False)
    assert a._sub is not None and a.env._sub is not None and a.env._sub.dim == D and b._sub is None and b.env._sub is None
    oa, _ = a.reset(seed=5)
    ob, _ = b.reset(seed=5)
    assert oa.dtype == np.float32 and oa.shape == (n, D) and H.same_bits(oa, ob)
    a.action_space.seed(1)
    finished = 0
    for t in range(20):
        act = a.action_space.sample()
        xa, xb = a.step(act), b.step(act)
        for u, v in zip(xa[:4], xb[:4]):
            assert u.dtype == v.dtype and H.same_bits(np.asarray(u), np.asarray(v)) if u.dtype.kind == "f" else np.array_equal(u, v), t
        done = xa[2] | xa[3]
        for i in np.flatnonzero(done)[:50]:
            fa, fb = xa[4]["final_observation"][i], xb[4]["final_observation"][i]
            assert fa.dtype == np.float64 and H.same_bits(fa, fb)
        finished += int(done.sum())
    assert finished > 100
    ra, rb = a.env.obs_rms, b.env.obs_rms
    for u, v in ((ra.mean, rb.mean), (ra.var, rb.var), (ra.count, rb.count), (a.returns, b.returns), (a.return_rms.var, b.return_rms.var)):
        assert H.same_bits(np.asarray(u, np.float64), np.asarray(v, np.float64))
    a.close(), b.close()
