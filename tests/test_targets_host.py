"""tests/targets_host.py — the NumPy twin of include/mxv_targets.h, which the device is compared with bit for bit — held to the three
existing twins (tests/c51_host.py, tests/dqn_host.py, tests/qr_host.py), to a literal float64 floor / ceil / scatter C51 projection with
per-row discounts written here, and to the exact cases of the rule; and what needs no device of the front end.

How the bar of the projection is derived (u = 2^-53; the derivation of tests/test_c51_host.py, nothing here is tuned to what the twin
gives):
  * a probability p_k = e_k / S: the twin's EXP (gaussian_host.B_EXP u), its atom tree (6 u), its quotient (u); the literal exp (2 u),
    its sum in whatever order ((Z - 1) u) and quotient; the subtraction of the maximum on both sides: E_P = (B_EXP + Z + 12) u.
  * the shifted atoms and b_j are the SAME float64 operations on both sides (reward + g * z_j with g the widened per-row discount and
    z_j = v_min + j * dz, the two clamps, (c - v_min) / dz), so b_j is bit-equal.  The triangular weight 1 - |b - k| is at most two
    roundings from the literal u - b and b - l: 2 u absolute per (j, k).  A mass m_k is a sum of at most 2 Z products pn_j w_jk in two
    different orders (2 (2 Z - 1) u m_k), each product one rounding, each pn_j within E_P, and sum_j pn_j <= 1 + Z E_P.  A terminated
    row is the literal projection of ALL of next's mass onto one point against the rule's 1 * w_k: within Z E_P.
    Together, absolute: E_M = (2 u + (4 Z + 2) u + (Z + 1) E_P) (1 + Z E_P).
The only discontinuity is the argmax: rows whose two largest Q_a are equal or adjacent floats are counted, and the inputs have none."""
import subprocess
import sys

import numpy as np
import pytest

import c51_host as ch
import dqn_host as dh
import qr_host as qh
import targets_host as th
from conftest import ROOT
from gaussian_host import B_EXP
from test_c51_host import make_batch, near_ties

U = 2.0 ** -53
V_MIN, V_MAX = -10.0, 10.0
EXACT_GAMMAS = (0.5, 0.96875)      # exact in float32: discount = full(gamma) widens to the scalar
G32 = np.float32(0.99)
THREE = np.array([G32, np.float32(np.float64(G32) * np.float64(G32)), np.float32(np.float64(np.float32(np.float64(G32) * np.float64(G32))) * np.float64(G32))],
                 np.float32)      # gamma, float32(gamma gamma), float32(that gamma): as the n-step ring forms them


def _u64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_u64(a), _u64(b))


@pytest.fixture(scope="module")
def batch():
    b = make_batch(600, 6, 51, 7)
    rng = np.random.default_rng(11)
    b["q"] = rng.standard_normal((600, 6)).astype(np.float32)
    b["next_q"] = rng.standard_normal((600, 6)).astype(np.float32)
    b["online_q"] = (b["next_q"] + 0.7 * rng.standard_normal((600, 6))).astype(np.float32)
    b["three"] = THREE[rng.integers(0, 3, 600)]
    b["any"] = rng.uniform(0.0, 1.0, 600).astype(np.float32)
    return b


# ---- against the three existing twins ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", (False, True))
@pytest.mark.parametrize("gamma", EXACT_GAMMAS)
def test_a_full_discount_and_the_scalar_gamma_have_the_bits_of_the_existing_twins(batch, gamma, double):
    b = batch
    M = len(b["reward"])
    full = np.full(M, gamma, np.float32)
    assert float(full[0]) == gamma
    on = b["online"] if double else None
    ref = ch.rows(b["logits"], b["act"], v_min=V_MIN, v_max=V_MAX, reward=b["reward"], terminated=b["term"], next_logits=b["next"],
                  next_logits_online=on, gamma=gamma)
    for kw in (dict(gamma=gamma), dict(discount=full)):
        p = th.c51(b["next"], b["reward"], b["term"], v_min=V_MIN, v_max=V_MAX, next_logits_online=on, **kw)
        assert _same(p["m"], ref["m"]) and _same(p["cm"], ref["cm"]) and np.array_equal(p["jstar"], ref["jstar"])
    on = b["online_q"] if double else None
    ref = dh.rows(b["q"], b["act"], reward=b["reward"], terminated=b["term"], next_q=b["next_q"], next_q_online=on, gamma=gamma)["y"]
    for kw in (dict(gamma=gamma), dict(discount=full)):
        assert _same(th.dqn(b["next_q"], b["reward"], b["term"], next_q_online=on, **kw), ref)
    on = b["online"] if double else None
    for kw in (dict(gamma=gamma), dict(discount=full), dict(discount=b["any"])):
        ref = qh.rows(b["logits"], b["act"], reward=b["reward"], terminated=b["term"], next_quantiles=b["next"], next_quantiles_online=on, **kw)["T"]
        assert _same(th.qr(b["next"], b["reward"], b["term"], next_quantiles_online=on, **kw), ref)


def test_three_discounts_in_one_batch_are_three_scalar_runs_of_the_existing_twins(batch):
    b = batch
    d = b["three"]
    assert len(set(THREE.tolist())) == 3 and all((d == v).sum() > 50 for v in THREE)
    p = th.c51(b["next"], b["reward"], b["term"], v_min=V_MIN, v_max=V_MAX, discount=d, next_logits_online=b["online"])
    y = th.dqn(b["next_q"], b["reward"], b["term"], discount=d, next_q_online=b["online_q"])
    T = th.qr(b["next"], b["reward"], b["term"], discount=d, next_quantiles_online=b["online"])
    for v in THREE:
        g, rows = float(v), d == v
        ref = ch.rows(b["logits"], b["act"], v_min=V_MIN, v_max=V_MAX, reward=b["reward"], terminated=b["term"], next_logits=b["next"],
                      next_logits_online=b["online"], gamma=g)
        assert _same(p["m"][rows], ref["m"][rows]) and _same(p["cm"][rows], ref["cm"][rows])
        ref = dh.rows(b["q"], b["act"], reward=b["reward"], terminated=b["term"], next_q=b["next_q"], next_q_online=b["online_q"], gamma=g)["y"]
        assert _same(y[rows], ref[rows])
        ref = qh.rows(b["logits"], b["act"], reward=b["reward"], terminated=b["term"], next_quantiles=b["next"], next_quantiles_online=b["online"],
                      gamma=g)["T"]
        assert _same(T[rows], ref[rows])
    # and the groups differ from one another: the discount is read
    other = th.c51(b["next"], b["reward"], b["term"], v_min=V_MIN, v_max=V_MAX, gamma=float(THREE[0]), next_logits_online=b["online"])
    live = (b["term"] == 0) & (d != THREE[0]) & (np.abs(b["reward"]) < 5.0)      # not the rows whose every atom clamps to one end
    assert not np.any(np.all(_u64(other["m"][live]) == _u64(p["m"][live]), axis=1))


# ---- against a literal floor / ceil / scatter projection ----------------------------------------------------------------------------------------
def literal_projection(nxt, sel, reward, term, discount, v_min, v_max):
    """softmax, expectation, argmax, gather, the Bellman shift with a per-row discount, clamp, floor / ceil with the l == u repair,
    scatter-add: float64 NumPy."""
    M, A, Z = nxt.shape
    rows = np.arange(M)
    dz = (v_max - v_min) / (Z - 1)
    z = v_min + np.arange(Z, dtype=np.float64) * dz

    def softmax(x):
        e = np.exp(x - x.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)

    q_next = (softmax(sel.astype(np.float64)) * z).sum(-1)
    pn = softmax(nxt.astype(np.float64))[rows, q_next.argmax(1)]
    g = discount.astype(np.float64)[:, None]
    r = reward.astype(np.float64)[:, None]
    tz_raw = np.where(term[:, None] != 0, r, r + g * z[None, :])
    tz = np.clip(tz_raw, v_min, v_max)
    pos = (tz - v_min) / dz
    lo, up = np.floor(pos).astype(np.int64), np.ceil(pos).astype(np.int64)
    lo[(up > 0) & (lo == up)] -= 1      # the usual repair: without it an atom that lands on a support point loses its mass
    up[(lo < Z - 1) & (lo == up)] += 1
    m = np.zeros(M * Z)
    offset = (rows * Z)[:, None]
    np.add.at(m, (lo + offset).reshape(-1), (pn * (up.astype(np.float64) - pos)).reshape(-1))
    np.add.at(m, (up + offset).reshape(-1), (pn * (pos - lo.astype(np.float64))).reshape(-1))
    clipped = (pn * ((tz_raw < v_min) | (tz_raw > v_max))).sum(-1)
    return m.reshape(M, Z), clipped


@pytest.mark.parametrize("double", (False, True))
def test_the_projection_is_within_its_derived_bar_of_the_literal_one_on_20000_rows(double):
    M, A, Z = 20_000, 6, 51
    b = make_batch(M, A, Z, 1)
    sel = b["online"] if double else b["next"]
    assert near_ties(sel) == 0
    d = THREE[np.random.default_rng(3).integers(0, 3, M)]
    p = th.c51(b["next"], b["reward"], b["term"], v_min=V_MIN, v_max=V_MAX, discount=d, next_logits_online=sel if double else None)
    ref_m, ref_cm = literal_projection(b["next"], sel, b["reward"], b["term"], d, V_MIN, V_MAX)
    E_P = (B_EXP + Z + 12) * U
    E_M = (2 * U + (4 * Z + 2) * U + (Z + 1) * E_P) * (1 + Z * E_P) * (1.0 + 1e-6)
    diff = np.abs(p["m"][:, :Z] - ref_m)
    worst = float(diff.max()) / U
    print(f"B_PROJECTED measured {worst:.2f} u, bar {E_M / U:.1f} u")
    assert np.all(diff <= E_M), (worst, E_M / U)
    assert np.all(p["m"][:, Z:] == 0.0)
    assert np.all(np.abs(p["cm"] - ref_cm) <= ((Z + 1) * E_P + (6 + Z) * U) * (1.0 + 1e-6))
    m32, cm32 = th.c51_f32(b["next"], b["reward"], b["term"], v_min=V_MIN, v_max=V_MAX, discount=d, next_logits_online=sel if double else None)
    ulp = np.spacing(np.abs(ref_m * (1 + 1e-6)).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(m32.astype(np.float64) - ref_m) <= E_M + ulp / 2) and m32.dtype == np.float32 and cm32.shape == (M,)


# ---- the exact cases of the rule -------------------------------------------------------------------------------------------------------------
NEG = -np.inf


def _onehot_logits(M, A, Z, at):
    x = np.full((M, A, Z), NEG, np.float32)
    x[:, :, at] = 0.0      # e = 1 there and 0 elsewhere, S = 1: p is exactly one-hot
    return x


def test_a_shifted_atom_exactly_on_an_atom_keeps_all_its_mass_there():
    # support -2 .. 2 with dz = 1; r = 1, g = 0.5: tz_2 = 1 + 0.5 * 0 = 1, b = 3 exactly
    nxt = _onehot_logits(3, 2, 5, 2)
    for kw in (dict(gamma=0.5), dict(discount=np.full(3, 0.5, np.float32))):
        p = th.c51(nxt, np.ones(3, np.float32), np.zeros(3, np.uint8), v_min=-2.0, v_max=2.0, **kw)
        assert np.array_equal(p["m"][:, :5], np.tile([0.0, 0.0, 0.0, 1.0, 0.0], (3, 1))) and np.all(p["cm"] == 0.0)
    # between two atoms: the mass splits by the distances, exactly
    p = th.c51(_onehot_logits(1, 1, 5, 3), np.ones(1, np.float32), np.zeros(1, np.uint8), v_min=-2.0, v_max=2.0, discount=np.full(1, 0.25, np.float32))
    assert np.array_equal(p["m"][0, :5], [0.0, 0.0, 0.0, 0.75, 0.25])      # tz = 1.25


def test_a_terminated_row_ignores_the_next_rows_and_a_nan_discount():
    M, A, Z = 4, 3, 5
    rng = np.random.default_rng(5)
    nxt = rng.standard_normal((M, A, Z)).astype(np.float32)
    on = nxt.copy()
    nxt[0] = np.nan
    on[1, 1, 2] = np.inf
    nxt[2] = NEG
    r = np.array([1.0, 0.25, -2.0, 0.5], np.float32)
    term = np.array([1, 1, 1, 0], np.uint8)
    d = np.array([np.nan, np.nan, np.inf, 0.5], np.float32)
    p = th.c51(nxt, r, term, v_min=-2.0, v_max=2.0, discount=d, next_logits_online=on)
    assert np.array_equal(p["m"][:3, :Z], [[0, 0, 0, 1, 0], [0, 0, 0.75, 0.25, 0], [1, 0, 0, 0, 0]]) and np.all(p["cm"][:3] == 0.0)
    assert np.all(np.isfinite(p["m"][3])) and abs(p["m"][3].sum() - 1.0) < 1e-14
    y = th.dqn(nxt[:, :, 0], r, term, discount=d, next_q_online=on[:, :, 0])
    assert _same(y[:3], r[:3].astype(np.float64)) and np.isfinite(y[3])
    T = th.qr(nxt, r, term, discount=d, next_quantiles_online=on)
    assert _same(T[:3, :Z], np.repeat(r[:3].astype(np.float64)[:, None], Z, 1)) and np.all(T[:, Z:] == 0.0) and np.all(np.isfinite(T[3]))


def test_a_nan_discount_on_a_live_row_is_nan_in_that_row_and_nowhere_else():
    M, A, Z = 5, 3, 7
    rng = np.random.default_rng(6)
    nxt = rng.standard_normal((M, A, Z)).astype(np.float32)
    r = rng.standard_normal(M).astype(np.float32)
    term = np.zeros(M, np.uint8)
    d = np.full(M, 0.5, np.float32)
    clean = (th.c51(nxt, r, term, v_min=-3.0, v_max=3.0, discount=d)["m"], th.dqn(nxt[:, :, 0], r, term, discount=d), th.qr(nxt, r, term, discount=d))
    d[2] = np.nan
    dirty = (th.c51(nxt, r, term, v_min=-3.0, v_max=3.0, discount=d)["m"], th.dqn(nxt[:, :, 0], r, term, discount=d), th.qr(nxt, r, term, discount=d))
    others = np.arange(M) != 2
    for c, x, width in zip(clean, dirty, (Z, None, Z)):
        assert _same(c[others], x[others])
        assert np.all(np.isnan(x[2] if width is None else x[2, :width]))
    assert np.all(th.to_f32(dirty[0][2, :Z]).view(np.uint32) == 0x7FC00000)


def test_a_zero_discount_is_the_terminated_projection_of_the_reward():
    M, A, Z = 6, 3, 5
    rng = np.random.default_rng(8)
    r = np.array([1.0, 0.25, -2.0, 0.5, 7.0, -0.75], np.float32)
    zero, live, dead = np.zeros(M, np.float32), np.zeros(M, np.uint8), np.ones(M, np.uint8)
    # all of next's mass on one atom: exactly the terminated row
    nxt = _onehot_logits(M, A, Z, 1)
    a, b = (th.c51(nxt, r, t, v_min=-2.0, v_max=2.0, discount=zero) for t in (live, dead))
    assert _same(a["m"], b["m"]) and _same(a["cm"], b["cm"]) and a["cm"][4] == 1.0
    # any distribution: the same weights times the sum of its mass, which is 1 within the probabilities' own error
    nxt = rng.standard_normal((M, A, Z)).astype(np.float32)
    a, b = (th.c51(nxt, r, t, v_min=-2.0, v_max=2.0, discount=zero) for t in (live, dead))
    assert np.all(np.abs(a["m"] - b["m"]) <= (2 * Z + 8) * U)      # Z products of one rounding each, Z - 1 additions, Z probabilities each within 4 u of p
    assert _same(th.dqn(nxt[:, :, 0], r, live, discount=zero), r.astype(np.float64))
    assert _same(th.qr(nxt, r, live, discount=zero)[:, :Z], np.repeat(r.astype(np.float64)[:, None], Z, 1))


def test_the_clipped_mass_counts_what_falls_outside_the_support():
    # support -2 .. 2; r = 1.5, g = 1: tz = -0.5, 0.5, 1.5, 2.5, 3.5 — atoms 3 and 4 leave; uniform mass 1 / 5 each
    nxt = np.zeros((2, 1, 5), np.float32)
    p = th.c51(nxt, np.full(2, 1.5, np.float32), np.zeros(2, np.uint8), v_min=-2.0, v_max=2.0, discount=np.ones(2, np.float32))
    fifth = np.float64(1.0) / np.float64(5.0)
    assert np.all(p["cm"] == fifth + fifth)
    assert np.array_equal(p["m"][0, :5], [0.0, 0.5 * fifth, (0.5 * fifth + 0.5 * fifth), (0.5 * fifth + 0.5 * fifth), ((0.5 * fifth + fifth) + fifth)])
    # a terminated reward below the support: all of it
    p = th.c51(nxt, np.full(2, -9.0, np.float32), np.ones(2, np.uint8), v_min=-2.0, v_max=2.0, gamma=0.99)
    assert np.all(p["cm"] == 1.0) and np.array_equal(p["m"][0, :5], [1.0, 0, 0, 0, 0])


# ---- the front end without a device ----------------------------------------------------------------------------------------------------------
def test_importing_the_module_does_not_import_torch_and_the_package_exports_the_functions():
    code = ("import sys; import gym_amd.targets as d; assert 'torch' not in sys.modules; import gym_amd; "
            "assert gym_amd.dqn_targets is d.dqn_targets and gym_amd.categorical_targets is d.categorical_targets "
            "and gym_amd.quantile_targets is d.quantile_targets; assert 'torch' not in sys.modules")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]


def test_the_front_end_refuses_bad_arguments_before_any_launch():
    import torch

    from gym_amd import targets

    nq, nl = torch.zeros(4, 3), torch.zeros(4, 3, 5)
    r, term = torch.zeros(4), torch.zeros(4, dtype=torch.bool)
    with pytest.raises(ValueError, match="gamma and discount are both given"):
        targets.dqn_targets(nq, r, term, gamma=0.9, discount=r)
    with pytest.raises(ValueError, match="gamma and discount are both given"):
        targets.categorical_targets(nl, r, term, v_min=-1.0, v_max=1.0, gamma=0.9, discount=r)
    with pytest.raises(ValueError, match="gamma and discount are both given"):
        targets.quantile_targets(nl, r, term, gamma=0.9, discount=r)
    with pytest.raises(ValueError, match="v_min must be below v_max"):
        targets.categorical_targets(nl, r, term, v_min=1.0, v_max=1.0)
    with pytest.raises(ValueError, match="gamma must be a finite number"):
        targets.quantile_targets(nl, r, term, gamma=float("nan"))
    with pytest.raises(ValueError, match="reward must have shape"):
        targets.dqn_targets(nq, torch.zeros(5), term)
    with pytest.raises(ValueError, match="terminated must be torch.uint8"):
        targets.dqn_targets(nq, r, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="next_logits_online must have shape"):
        targets.categorical_targets(nl, r, term, v_min=-1.0, v_max=1.0, next_logits_online=torch.zeros(4, 2, 5))
    with pytest.raises(ValueError, match="discount must be torch.float32"):
        targets.quantile_targets(nl, r, term, discount=r.double())
    with pytest.raises(ValueError, match="must be a device tensor"):
        targets.dqn_targets(nq, r, term)
    with pytest.raises(ValueError, match="Z"):
        targets.categorical_targets(torch.zeros(4, 3, 1), r, term, v_min=-1.0, v_max=1.0)
