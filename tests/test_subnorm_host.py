"""The per-sub-env normaliser's checker checked, without a GPU: oracle.SubEnvNorm (oracle/normalize.c: orc_subnorm_*), the authority of
tests/test_gpu_subnorm.py and tests/test_gpu_subnorm_edges.py, against tests/subnorm_host.py's literal NumPy restatement of the reference's
update_mean_var_count_from_moments on every input list those GPU tests use — bit for bit, zeros by sign, NaN matching NaN — and the
conditions on the constructed guard-path inputs: every one of the kernels' three paths is taken by a mixed and by an unmixed wave-iteration,
on operands where the short division form and `/` differ."""
import numpy as np
import pytest

import subnorm_host as H


def _obs_twin_equals_oracle(state, x, fin, te, tr, eps, f32, what):
    D, n = x.shape[2], x.shape[1]
    st = state if state is not None else (np.zeros((n, D)), np.ones((n, D)), np.full(n, 1e-4))
    y, yf, wrote, st_t, _ = H.obs_walk(*st, x, fin, te, tr, eps)
    y_o, yf_o, st_o = H.oracle_obs(state, x, fin, te, tr, eps, f32)
    with np.errstate(all="ignore"):
        assert H.same_bits(y.astype(np.float32) if f32 else y, y_o), what
    if yf_o is not None:
        assert H.same_bits(yf, yf_o), what
        assert np.array_equal(wrote, ((te | tr) != 0)), what
    for a, b, name in zip(st_t, st_o, ("mean", "var", "count")):
        assert H.same_bits(a, b.reshape(a.shape)), (what, name)
    return y, yf, st_t


def _rew_twin_equals_oracle(state, rew, te, tr, gamma, what):
    n = rew.shape[1]
    st = state if state is not None else (np.zeros(n), np.ones(n), np.full(n, 1e-4), np.zeros(n))
    out, st_t, _ = H.rew_walk(*st, rew, te, tr, gamma, 1e-8)
    out_o, st_o = H.oracle_rew(state, rew, te, tr, gamma, 1e-8)
    with np.errstate(all="ignore"):
        assert H.same_bits(out.astype(rew.dtype), out_o), what
    for a, b, name in zip(st_t, st_o, ("mean", "var", "count", "returns")):
        assert H.same_bits(a, b), (what, name)
    return out, st_t


@pytest.mark.parametrize("n", H.SIZES)
def test_oracle_equals_the_literal_twin_on_the_observation_grid(n):
    for D in H.DIMS:
        for pattern, K, f32 in H.obs_grid(n, D):
            x, fin = H.rows(D, K, n)
            te, tr = H.flags(pattern, K, n, np.random.default_rng(K))
            _obs_twin_equals_oracle(None, x, fin, te, tr, 1e-8, f32, (D, pattern, K, f32))
    x, fin = H.rows(3, 7, n)
    te, tr = H.flags("both", 7, n, np.random.default_rng(0))
    y0, _, st0 = _obs_twin_equals_oracle(None, x, None, None, None, 1e-8, True, "reset form")
    y1, _, st1 = _obs_twin_equals_oracle(None, x, None, te, tr, 1e-8, True, "flags without final")
    assert H.same_bits(y0, y1) and all(H.same_bits(a, b) for a, b in zip(st0, st1))      # flags without terminal rows are ignored


@pytest.mark.parametrize("n", H.SIZES)
def test_oracle_equals_the_literal_twin_on_the_reward_grid(n):
    for pattern, K, f32, _, gamma in H.rew_grid(n):
        te, tr = H.flags(pattern, K, n, np.random.default_rng(K))
        _rew_twin_equals_oracle(None, H.rewards_for(K, n, f32), te, tr, gamma, (pattern, K, f32, gamma))


@pytest.mark.parametrize("D", H.DIMS)
def test_oracle_equals_the_literal_twin_on_the_edge_rows(D):
    """... and the NaN sets are the injected ones, exactly; the m_b cases store var = +0.0 (the reference's bits)."""
    for name, (state, x, eps, nan) in H.obs_edge_cases(D).items():
        for f32 in (True, False):
            y, _, st = _obs_twin_equals_oracle(state, x, None, None, None, eps, f32, (name, f32))
            assert H.nan_envs((y, 1), (st[0], 0), (st[1], 0), (st[2], 0)) == nan, name
        L = list(H.EDGE_LANES)
        if name == "float32_subnormal_result":
            y32 = np.abs(y[0, L].astype(np.float32))
            assert ((y32 > 0) & (y32 < 2.0 ** -126)).all()
        if name == "float32_overflow_result":
            with np.errstate(over="ignore"):
                assert np.isfinite(y[0, L]).all() and np.isinf(y[0, L].astype(np.float32)).all()
        if name.startswith("count_minus"):
            one = H.obs_walk(*state, x[:1], None, None, None, eps)[3][1]
            assert (H.bits(one[L]) == 0).all(), name                      # var = +0.0 after the first update: m_a + (+0.0) + -0.0


@pytest.mark.parametrize("f32", [True, False])
def test_oracle_equals_the_literal_twin_on_the_edge_rewards(f32):
    n = H.EDGE_N
    for name, (rew, gamma, start, nan) in H.rew_edge_cases(f32).items():
        te, tr = H.flags("terminated", 9, n, np.random.default_rng(3))
        te[:, list(H.EDGE_LANES)] = 0
        out, st = _rew_twin_equals_oracle((np.zeros(n), np.ones(n), np.full(n, 1e-4), start), rew, te, tr, gamma, name)
        assert H.nan_envs((out, 1), *((a, 0) for a in st)) == nan, name
        if name == "gamma_2_overflow":
            L = list(H.EDGE_LANES)          # returns = Inf from the second step on, so delta = Inf - Inf: the statistics are NaN
            assert np.isinf(st[3][L]).all() and np.isnan(st[0][L]).all() and np.isfinite(st[3][1:63]).all()
        if name == "minus_zero_rewards":
            assert np.signbit(out[:, list(H.EDGE_LANES)]).all()


def test_guards_restated_on_the_host_sit_at_their_documented_edges():
    """plain_operand 2^-723 <= |x| < 2^678, plain_delta 2^-300 <= |x| < 2^301 (both pass 0, Inf, NaN), plain_divisor 2^-64 <= |d| < 2^65;
    short_count is plain_divisor without the negative half, plus +0.0 alone."""
    up, dn = lambda v: np.nextafter(v, np.inf), lambda v: np.nextafter(v, 0.0)
    for f, lo, hi in ((H.plain_operand, -723, 678), (H.plain_delta, -300, 301)):
        assert f(np.array([2.0 ** lo, dn(2.0 ** hi), -2.0 ** lo, 0.0, -0.0, np.inf, -np.inf, np.nan])).all()
        assert not f(np.array([dn(2.0 ** lo), 2.0 ** hi, -dn(2.0 ** lo), 5e-324, 2.0 ** -1030])).any()
    assert H.plain_divisor(np.array([2.0 ** -64, dn(2.0 ** 65), -1.0, 1.0001])).all()
    assert not H.plain_divisor(np.array([dn(2.0 ** -64), 2.0 ** 65, 0.0, np.inf, np.nan, 5e-324])).any()
    assert H.short_count(np.array([0.0, 2.0 ** -64, dn(2.0 ** 65), 1e-4, 1.0])).all()
    assert not H.short_count(np.array([-0.0, -0.5, -1.0, dn(2.0 ** -64), 2.0 ** 65, 5e-324, np.inf, np.nan, 1e300, 1e-300])).any()


def _differs(x, d):
    return H.div_shared_host(float(x), float(d)) != float(x) / float(d)


def _check_guard_operands(mean, var, count, D):
    """The lanes that fail one vote alone do so on dividends where the short form is not `/` — else the guard would not be tested."""
    assert H.div_shared_host(7.25, 6.0) == 7.25 / 6.0 and H.div_shared_host(-1e-3, 4099.0) == -1e-3 / 4099.0
    for lane in [H.OK2_LANE] + list(range(6 * H.WAVE, 7 * H.WAVE)):
        assert count[lane] == 5.0 and any(_differs(var[lane, j] * 5.0, 6.0) for j in range(D)), lane
    for lane in H.DELTA_LANES:
        assert count[lane] == 5.0 and _differs(-mean[lane, D - 1], 6.0), lane


@pytest.mark.parametrize("D", [1, 4])
def test_observation_guard_inputs_walk_every_path_mixed_and_unmixed(D):
    for K in (1, 6):
        state, x, fin, te, tr = H.obs_guard_case(D, K)
        _check_guard_operands(*state, D)
        y, yf, wrote, st, report = H.obs_walk(*state, x, fin, te, tr, 1e-8)
        assert H.paths_taken(report) == H.EVERY_PATH_BOTH_WAYS, (K, sorted(H.paths_taken(report)))
        first = {w: (p, m) for w, it, p, m in report if it == 0}
        assert first == {0: (H.SHORT, False), 1: (H.PLAIN, True), 2: (H.M2, True), 3: (H.PLAIN, False), 4: (H.SHORT, False),
                         5: (H.PLAIN, True), 6: (H.M2, False)}
        for f32 in (True, False):
            _obs_twin_equals_oracle(state, x, fin, te, tr, 1e-8, f32, (K, f32))
        assert H.nan_envs((y, 1), (yf, 1), (st[0], 0), (st[1], 0), (st[2], 0)) == H.GUARD_NAN_ENVS


@pytest.mark.parametrize("f32", [True, False])
def test_reward_guard_inputs_walk_every_path_mixed_and_unmixed(f32):
    """K = 1 is one iteration with every lane at work: the short path cannot be mixed there (nothing came before, nobody is through), so
    the single-step call is held to the other five."""
    for K in (1, 6):
        state, rew, te, tr, gamma = H.rew_guard_case(K, f32)
        _check_guard_operands(state[0][:, None], state[1][:, None], state[2], 1)
        out, st, report = H.rew_walk(*state, rew, te, tr, gamma, 1e-8)
        want = H.EVERY_PATH_BOTH_WAYS - ({(H.SHORT, True)} if K == 1 else set())
        assert H.paths_taken(report) == want, (K, sorted(H.paths_taken(report)))
        first = {w: p for w, it, p, m in report if it == 0}
        assert first == {0: H.SHORT, 1: H.PLAIN, 2: H.M2, 3: H.PLAIN, 4: H.SHORT, 5: H.PLAIN, 6: H.M2}
        _rew_twin_equals_oracle(state, rew, te, tr, gamma, (K, f32))
        assert H.nan_envs((out, 1), *((a, 0) for a in st)) == H.GUARD_NAN_ENVS
