"""tests/c51_host.py — the NumPy twin of include/mxv_c51.h, which the device is compared with bit for bit — held to a literal torch
float64 implementation of the categorical (C51) loss written here (softmax, expectation, argmax, gather, Bellman shift, clamp, floor /
ceil with the l == u repair, index_add_, -(m * log_softmax).sum(-1) times the weights, .mean(), autograd for the gradient), to exact
sums and to the exact cases of the rule; and what needs no device of the front end.

How the bars are derived (u = 2^-53; nothing here is tuned to what the twin gives):
  * a probability p_k = e_k / S: the twin's EXP (gaussian_host.B_EXP u), its atom tree (6 u), its quotient (u); torch's exp (2 u), its
    sum in whatever order ((Z - 1) u) and quotient; the subtraction of the maximum on both sides: E_P = (B_EXP + Z + 12) u, relative.
  * a log-probability lp_k = d_k - LOG(S): the same for S, the two logarithms (gaussian_host.B_LOG u and 2 u, absolute: S >= 1 and the
    logarithm's slope is at most 1), two subtractions: E_LP = E_P + (B_LOG + 4) u, of max(1, |lp_k|).
  * the shifted atoms and b_j are the SAME float64 operations on both sides (reward + gamma * z_j with z_j = v_min + j * dz, the two
    clamps, (c - v_min) / dz), so b_j is bit-equal.  The triangular weight 1 - |b - k| is at most two roundings from the literal u - b
    and b - l, which are exact or one rounding: 2 u absolute per (j, k).  A mass m_k is a sum of at most 2 Z products pn_j w_jk in two
    different orders (2 (2 Z - 1) u m_k), each product one rounding, each pn_j within E_P, and sum_j pn_j <= 1 + Z E_P.  A terminated
    row is the literal projection of ALL of next's mass onto one point, sum_j pn_j w_k, against the rule's 1 * w_k: within Z E_P.
    Together, absolute: E_M = (2 u + (4 Z + 2) u + (Z + 1) E_P) (1 + Z E_P).
  * a sum over the atoms of terms t_k: the terms' own bars, (6 + Z) u sum |t_k| for the two orders.
  * a mean over M rows: the rows' own bars, EB(sum |term|) = norm_tree_host.sum_error_bound(depth(M), sum |term|) for the twin's tree,
    (M - 1) u sum |term| for whatever order torch sums in, one rounding for each quotient and one for the weight.
  * the gradient gs w (p_k sm - m_k): E_P p_k sm and (6 + Z) u sm for the sum, E_M for m_k, four roundings: absolute, times |gs w|.
  * a float32 output: half a float32 ulp of the reference on top of its float64 bar.
The only discontinuity is the argmax: rows whose two largest Q_a are equal or adjacent floats are counted, and the inputs have none."""
import math
import subprocess
import sys

import numpy as np
import pytest

import c51_host as ch
import norm_tree_host as nt
import ppo_host as pp
from conftest import ROOT
from gaussian_host import B_EXP, B_LOG
from policy_eval_host import bar

U = 2.0 ** -53
M_BIG, A_BIG, Z_BIG = 20_000, 6, 51
V_MIN, V_MAX = -10.0, 10.0
GAMMA = 0.99
SLOP = 1.0 + 1e-6          # the second-order terms the first-order bounds above leave out
MODES = (("given", False), ("bootstrap", False), ("bootstrap", True))
SMALL = ((1, 2), (3, 51), (2, 64))


def _u64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64) * (1 + 1e-6)).astype(np.float32)).astype(np.float64)


def make_batch(M, A, Z, seed):
    """M rows of A actions of Z atoms on the support [-10, 10].  Cycling through the rows: a tenth terminated with a reward on a support
    point (an end of the support or, for Z = 51 and 33, its middle: b lands exactly on an atom), a tenth with rewards far outside the
    support, a tenth terminated with any reward; the rest ordinary."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((M, A, Z)) * 2.0).astype(np.float32)
    act = rng.integers(0, A, M)
    nxt = (rng.standard_normal((M, A, Z)) * 2.0).astype(np.float32)
    online = (nxt + 0.7 * rng.standard_normal((M, A, Z))).astype(np.float32)
    reward = rng.standard_normal(M).astype(np.float32)
    term = np.zeros(M, np.uint8)
    k = np.arange(M)
    on = k % 10 == 1
    reward[on] = rng.choice(np.array([-10.0, 0.0, 10.0], np.float32), on.sum())
    term[on] = 1
    far = k % 10 == 2
    reward[far] = rng.choice(np.array([-50.0, 50.0, 21.5], np.float32), far.sum())
    term[k % 10 == 3] = 1
    tp = rng.uniform(size=(M, Z)) ** 3
    tp[k % 10 == 4, : Z // 2] = 0.0      # exact zeros in a given target
    target_probs = (tp / tp.sum(1, keepdims=True)).astype(np.float32)
    weights = rng.uniform(0.2, 2.0, M).astype(np.float32)
    return dict(logits=logits, act=act, next=nxt, online=online, reward=reward, term=term, target_probs=target_probs, weights=weights)


def kwargs(b, mode, double, weighted, gamma=GAMMA, v_min=V_MIN, v_max=V_MAX):
    kw = dict(v_min=v_min, v_max=v_max, weights=b["weights"] if weighted else None)
    if mode == "given":
        kw["target_probs"] = b["target_probs"]
    else:
        kw.update(reward=b["reward"], terminated=b["term"], next_logits=b["next"], next_logits_online=b["online"] if double else None, gamma=gamma)
    return kw


def near_ties(sel):
    """Rows whose two largest expected values are equal or adjacent floats: where an argmax may legitimately differ."""
    Q = np.sort(ch.q_values(sel, v_min=V_MIN, v_max=V_MAX), axis=1)
    if Q.shape[1] < 2:
        return 0
    return int(np.count_nonzero(np.nextafter(Q[:, -2], np.inf) >= Q[:, -1]))


def torch_reference(b, mode, double, weighted, grad_loss=1.0, gamma=GAMMA, v_min=V_MIN, v_max=V_MAX):
    """The literal torch sequence in float64 on the CPU, and its autograd."""
    import torch

    f = lambda x: torch.from_numpy(np.asarray(x, np.float32).astype(np.float64))
    logits = f(b["logits"]).requires_grad_()
    M, A, Z = logits.shape
    a = torch.from_numpy(np.asarray(b["act"], np.int64))
    rows = torch.arange(M)
    dz = (v_max - v_min) / (Z - 1)
    z = v_min + torch.arange(Z, dtype=torch.float64) * dz
    if mode == "given":
        m = f(b["target_probs"]).reshape(M, Z)
        clipped = torch.zeros(M, dtype=torch.float64)
    else:
        nxt = f(b["next"])
        sel = f(b["online"]) if double else nxt
        q_next = (torch.softmax(sel, -1) * z).sum(-1)
        pn = torch.softmax(nxt, -1)[rows, q_next.argmax(1)]
        live = 1 - torch.from_numpy(b["term"].astype(np.float64))
        tz_raw = f(b["reward"])[:, None] + live[:, None] * gamma * z[None, :]
        tz = tz_raw.clamp(v_min, v_max)
        pos = (tz - v_min) / dz
        lo, up = pos.floor().long(), pos.ceil().long()
        lo[(up > 0) & (lo == up)] -= 1      # the usual repair: without it an atom that lands on a support point loses its mass
        up[(lo < Z - 1) & (lo == up)] += 1
        m = torch.zeros(M * Z, dtype=torch.float64)
        offset = (rows * Z)[:, None]
        m.index_add_(0, (lo + offset).view(-1), (pn * (up.double() - pos)).view(-1))
        m.index_add_(0, (up + offset).view(-1), (pn * (pos - lo.double())).view(-1))
        m = m.view(M, Z)
        clipped = (pn * ((tz_raw < v_min) | (tz_raw > v_max)).double()).sum(-1)
    taken = logits[rows, a]
    lp = torch.log_softmax(taken, -1)
    ce = -(m * lp).sum(-1)
    term = ce * f(b["weights"]) if weighted else ce
    loss = term.mean()
    (grad_loss * loss).backward()
    with torch.no_grad():
        p = torch.softmax(taken, -1)
        qa, y, ent = (p * z).sum(-1), (m * z).sum(-1), -(p * lp).sum(-1)
        stats = [float(loss), float(qa.mean()), float(y.mean()), float(ent.mean()), float(clipped.mean()), float(ce.max()), float(qa.min()), float(qa.max())]
    return dict(loss=float(loss.detach()), stats=np.array(stats), m=m.numpy(), ce=ce.detach().numpy(), grad=logits.grad.numpy(),
                p=p.numpy(), lp=lp.detach().numpy())


def row_bars(p, Z, z):
    """The derived bars of one configuration's rows -> dict of arrays (absolute)."""
    E_P = (B_EXP + Z + 12) * U
    E_LP = E_P + (B_LOG + 4) * U
    E_M = (2 * U + (4 * Z + 2) * U + (Z + 1) * E_P) * (1 + Z * E_P)
    given = p["jstar"] is None
    e_m = 0.0 if given else E_M      # a given target is an input: the same numbers on both sides
    pk, mk, lp = p["p"][:, :Z], p["m"][:, :Z], p["lp"][:, :Z]
    za, alp = np.abs(z[:Z]), np.abs(lp)
    atoms = (6 + Z) * U
    ce = (e_m * alp + mk * E_LP * np.maximum(1.0, alp) + atoms * mk * alp).sum(1)
    qa = ((E_P + atoms) * pk * za).sum(1)
    y = ((e_m + atoms * mk) * za).sum(1)
    ent = (pk * (E_P * alp + E_LP * np.maximum(1.0, alp)) + atoms * pk * alp).sum(1) + 4 * U * np.abs(p["ent"])
    cm = np.zeros(len(ce)) if given else np.full(len(ce), (Z + 1) * E_P + atoms)
    grad = pk * p["sm"][:, None] * (E_P + atoms) + e_m + 4 * U * (pk * p["sm"][:, None] + mk)
    return dict(m=e_m, ce=ce * SLOP, qa=qa * SLOP, y=y * SLOP, ent=ent * SLOP, cm=cm * SLOP, grad=grad * SLOP)


def mean_bar(M, rows_err, terms_abs):
    """|twin mean - torch mean| of M terms: the rows' own differences, the twin's tree, torch's order, the quotients."""
    t = float(np.sum(terms_abs)) * SLOP
    return (float(np.sum(rows_err)) + nt.sum_error_bound(ch.depth(M), t) + (M - 1) * U * t + 2 * U * t) / M * SLOP


def compare(b, mode, double, weighted, grad_loss=2.5):
    """One configuration against torch: asserts every derived bar -> the worst ratios (projected, row loss, loss, stats, gradient)."""
    M, A, Z = b["logits"].shape
    if mode == "bootstrap":
        assert near_ties(b["online"] if double else b["next"]) == 0
    kw = kwargs(b, mode, double, weighted)
    value, stats, p, _ = ch.loss(b["logits"], b["act"], **kw)
    grad = ch.backward(b["logits"], b["act"], np.float32(grad_loss), **kw)
    ref = torch_reference(b, mode, double, weighted, grad_loss)
    z = ch.support(Z, V_MIN, V_MAX)[3]
    rb = row_bars(p, Z, z)
    where = (M, A, Z, mode, double, weighted)
    m_diff = np.abs(p["m"][:, :Z] - ref["m"])
    assert np.all(m_diff <= rb["m"]), (where, m_diff.max(), rb["m"])
    assert np.all(p["m"][:, Z:] == 0.0)
    ce_diff = np.abs(p["ce"] - ref["ce"])
    assert np.all(ce_diff <= rb["ce"]), (where, float(np.max(ce_diff - rb["ce"])))
    w = np.ones(M) if p["w"] is None else p["w"]
    bars = np.array([mean_bar(M, w * rb["ce"] + U * np.abs(p["term"]), np.abs(p["term"])), mean_bar(M, rb["qa"], np.abs(p["qa"])),
                     mean_bar(M, rb["y"], np.abs(p["y"])), mean_bar(M, rb["ent"], np.abs(p["ent"])), mean_bar(M, rb["cm"], np.abs(p["cm"])),
                     rb["ce"].max(), rb["qa"].max(), rb["qa"].max()])
    diff = np.abs(stats - ref["stats"])
    assert np.all(diff <= bars), (where, diff, bars)
    assert abs(value - ref["loss"]) <= bars[0]
    loss32, stats32, rl32, pj32 = ch.loss_f32(b["logits"], b["act"], **kw)
    assert abs(float(loss32) - ref["loss"]) <= bars[0] + _ulp32(ref["loss"]) / 2
    assert np.all(np.abs(stats32.astype(np.float64) - ref["stats"]) <= bars + _ulp32(ref["stats"]) / 2)
    assert np.all(np.abs(rl32.astype(np.float64) - ref["ce"]) <= rb["ce"] + _ulp32(ref["ce"]) / 2) and np.all(rl32 >= 0.0)
    assert np.all(np.abs(pj32.astype(np.float64) - ref["m"]) <= rb["m"] + _ulp32(ref["m"]) / 2)
    scale = abs(grad_loss) / M * w
    taken = grad[np.arange(M), b["act"]]
    ref_taken = ref["grad"][np.arange(M), b["act"]]
    g_diff = np.abs(taken - ref_taken)
    bar_g = scale[:, None] * rb["grad"]
    assert np.all(g_diff <= bar_g), (where, float(np.max(g_diff - bar_g)))
    assert np.all(np.abs(ch.to_f32(taken).astype(np.float64) - ref_taken) <= bar_g + _ulp32(ref_taken) / 2)
    off = np.ones(grad.shape[:2], bool)
    off[np.arange(M), b["act"]] = False
    assert np.all(_u64(grad[off]) == 0) and np.all(ref["grad"][off] == 0.0)      # +0.0 outside the taken action
    w_ce = float(np.max(ce_diff / (U * np.maximum(1.0, np.abs(ref["ce"])))))
    # a mean may cancel, and so may an expectation over a support that straddles zero: the unit is the mean magnitude of what is summed
    za = np.abs(z)
    mags = np.array([np.mean(np.abs(p["term"])), np.mean((p["p"] * za).sum(1)), np.mean((p["m"] * za).sum(1)), np.mean(np.abs(p["ent"])), np.mean(p["cm"])])
    nzs = mags != 0.0
    w_stats = float(np.max(diff[:5][nzs] / (U * mags[nzs])))
    return np.array([float(m_diff.max()) / U, w_ce, abs(value - ref["loss"]) / (U * mags[0]), w_stats,
                     float(np.max(g_diff / (U * scale[:, None])))])


NAMES = ("PROJECTED", "ROW_LOSS", "LOSS", "STATS", "GRAD")


def _all_options(b):
    worst = np.zeros(5)
    for mode, double in MODES:
        for weighted in (True, False):
            worst = np.maximum(worst, compare(b, mode, double, weighted))
    return worst


# ---- against the literal torch implementation ------------------------------------------------------------------------------------------------
def test_the_twin_is_within_its_derived_bars_of_the_literal_implementation_on_20000_rows():
    b = make_batch(M_BIG, A_BIG, Z_BIG, 1)
    p = ch.rows(b["logits"], b["act"], **kwargs(b, "bootstrap", True, False))
    assert (b["term"] != 0).sum() >= M_BIG // 10 and (p["cm"] > 0.5).sum() >= M_BIG // 20 and (p["m"].max(1) == 1.0).sum() >= M_BIG // 40
    worst = _all_options(b)
    for name, w in zip(NAMES, worst):
        # the named constant is what was measured on this input (to its two decimals, rounded up); the derived bars are asserted above
        bnd = getattr(ch, "B_" + name)
        print(f"measured B_{name}: {w:.4f}")
        assert w <= bnd < w + 0.01, (name, w, bnd)


@pytest.mark.parametrize("M", (1, 2, 1023, 1025))
def test_small_batches_agree_with_the_literal_implementation(M):
    for A, Z in SMALL:
        worst = _all_options(make_batch(M, A, Z, 100 + M + A + Z))
        for name, w in zip(NAMES, worst):
            assert w <= bar(getattr(ch, "B_" + name)), (M, A, Z, name, w)


def test_every_sum_is_within_the_tree_bound_of_the_exact_sum():
    b = make_batch(M_BIG, A_BIG, Z_BIG, 1)
    _, _, p, sums = ch.loss(b["logits"], b["act"], **kwargs(b, "bootstrap", True, True))
    assert ch.depth(M_BIG) == 4 + 6 + 2 + 10
    for k, got in sums.items():
        exact, bound = math.fsum(p[k]), nt.sum_error_bound(ch.depth(M_BIG), math.fsum(np.abs(p[k])))
        assert abs(got - exact) <= bound, (k, got, exact, bound)


def test_atomsum_is_the_butterfly_of_the_loss_trees():
    v = np.random.default_rng(5).standard_normal((100, 64)) * 10.0 ** np.random.default_rng(6).integers(-8, 8, (100, 64))
    assert np.array_equal(_u64(ch.atomsum(v)), _u64(nt.wave_tree_sum(v)))


# ---- exact cases ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Z", (2, 33, 51, 64))
def test_b_on_an_atom_puts_the_whole_mass_there_and_no_mass_is_lost(Z):
    """On the support 0 .. Z-1 (dz = 1) with gamma = 1 and integer rewards every shifted atom lands exactly on a support point or is
    clamped to an end; and on the ordinary batch the mass sums to 1 within 8 u on every row."""
    M, A = 200, 3
    b = make_batch(M, A, Z, 40 + Z)
    b["reward"] = np.random.default_rng(Z).integers(-3, 4, M).astype(np.float32)
    kw = kwargs(b, "bootstrap", False, False, gamma=1.0, v_min=0.0, v_max=float(Z - 1))
    p = ch.rows(b["logits"], b["act"], **kw)
    tp = ch.soft(b["next"][np.arange(M), p["jstar"]])["p"]
    for i in range(M):
        want = np.zeros(64)
        if b["term"][i]:
            want[int(np.clip(b["reward"][i], 0, Z - 1))] = 1.0
            assert np.array_equal(p["m"][i], want)      # a one-hot, exactly
        else:
            for j in range(Z):      # ascending j, the same additions
                want[int(np.clip(j + b["reward"][i], 0, Z - 1))] += tp[i, j]
            assert np.array_equal(_u64(p["m"][i]), _u64(want)), i
    for mode, double in MODES[1:]:
        b = make_batch(1000, A, Z, 50 + Z)
        p = ch.rows(b["logits"], b["act"], **kwargs(b, mode, double, False))
        assert np.all(np.abs(p["sm"] - 1.0) <= 8 * U) and np.all(p["m"] >= 0.0)
        assert (b["term"] != 0).any() and np.all(p["sm"][b["term"] != 0] == 1.0)


def test_gamma_zero_with_a_reward_on_atom_k_gives_a_one_hot():
    Z, A = 41, 3      # dz = 0.5: every support point is a float32
    b = make_batch(Z, A, Z, 9)
    b["term"][:] = 0
    z = ch.support(Z, -10.0, 10.0)[3]
    b["reward"] = z[:Z].astype(np.float32)
    assert np.array_equal(b["reward"].astype(np.float64), z[:Z])
    p = ch.rows(b["logits"], b["act"], **kwargs(b, "bootstrap", True, False, gamma=0.0))
    for k in range(Z):
        assert p["m"][k, k] >= 1.0 - 8 * U and np.count_nonzero(p["m"][k]) == 1 and abs(p["y"][k] - z[k]) <= 8 * U * abs(z[k])
    assert np.all(np.abs(p["sm"] - 1.0) <= 8 * U)


def test_a_terminated_row_ignores_both_next_tensors_entirely():
    b = make_batch(40, 3, 51, 2)
    b["term"][:] = 0
    b["term"][[5, 6, 7]] = 1
    kw = lambda c: kwargs(c, "bootstrap", True, True)
    clean = ch.loss(b["logits"], b["act"], **kw(b))
    b["next"][5], b["online"][6], b["next"][7, 1] = np.nan, np.inf, -np.inf
    b["online"][7] = np.nan
    got = ch.loss(b["logits"], b["act"], **kw(b))
    assert np.isfinite(got[1]).all() and np.array_equal(_u64(got[1]), _u64(clean[1])) and np.array_equal(_u64(got[2]["ce"]), _u64(clean[2]["ce"]))
    assert np.array_equal(_u64(got[2]["m"]), _u64(clean[2]["m"]))


def test_a_nan_in_any_selecting_row_makes_that_row_nan_and_no_other():
    b = make_batch(300, 4, 51, 3)
    b["term"][:] = 0
    b["reward"][:] = np.clip(b["reward"], -1, 1)
    for double in (False, True):
        for poison in (np.nan, np.inf):
            c = {k: v.copy() for k, v in b.items()}
            (c["online"] if double else c["next"])[17, 2, 5] = poison
            kw = kwargs(c, "bootstrap", double, False)
            value, stats, p, _ = ch.loss(c["logits"], c["act"], **kw)
            g = ch.backward(c["logits"], c["act"], np.float32(1.0), **kw)
            others = np.arange(300) != 17
            assert np.isnan(value) and np.isnan(p["ce"][17]) and np.isnan(p["m"][17, :51]).all() and np.isfinite(p["ce"][others]).all()
            assert np.isnan(g[17, c["act"][17]]).all() and np.count_nonzero(np.isnan(g)) == 51
            assert np.all(ch.bits(ch.to_f32(g))[17, c["act"][17]] == 0x7FC00000) and ch.bits(ch.loss_f32(c["logits"], c["act"], **kw)[0]) == 0x7FC00000
            clean = ch.backward(b["logits"], b["act"], np.float32(1.0), **kwargs(b, "bootstrap", double, False))
            assert np.array_equal(_u64(g[others]), _u64(clean[others]))
            # the extrema skip the NaN row
            assert stats[5] == p["ce"][others].max() and stats[6] == p["qa"].min() and stats[7] == p["qa"].max()
    # a bad taken row: NaN in its Z columns and nowhere else
    c = {k: v.copy() for k, v in b.items()}
    c["logits"][9, c["act"][9], :] = -np.inf
    g = ch.backward(c["logits"], c["act"], np.float32(1.0), **kwargs(c, "given", False, True))
    assert np.isnan(g[9, c["act"][9]]).all() and np.count_nonzero(np.isnan(g)) == 51


def test_ties_take_the_first_action():
    Z = 5
    row = np.array([0.3, -1.0, 2.0, 0.5, 0.0], np.float32)
    other = np.array([5.0, 0.0, 0.0, 0.0, 0.0], np.float32)      # its mass sits low: a smaller expectation
    sel = np.stack([np.stack([other, row, row]), np.stack([row, row, other]), np.stack([row, other, row])])
    assert np.array_equal(ch.first_max(ch.q_values(sel, v_min=0.0, v_max=4.0)), [1, 0, 0])
    nxt = np.zeros((3, 3, Z), np.float32)
    for a in range(3):
        nxt[:, a, a] = 50.0      # the evaluating network puts action a's mass on atom a
    p = ch.rows(np.zeros((3, 3, Z), np.float32), [0] * 3, v_min=0.0, v_max=4.0, reward=np.zeros(3, np.float32), terminated=np.zeros(3, np.uint8),
                next_logits=nxt, next_logits_online=sel, gamma=1.0)
    assert np.array_equal(p["jstar"], [1, 0, 0]) and np.array_equal(np.argmax(p["m"], 1), [1, 0, 0])


def test_a_minus_inf_logit_under_zero_target_mass_costs_nothing():
    b = make_batch(20, 2, 51, 6)
    rows = np.flatnonzero(np.arange(20) % 10 == 4)      # the rows whose given target is zero on the lower half
    for i in rows:
        b["logits"][i, b["act"][i], :5] = -np.inf
    p = ch.rows(b["logits"], b["act"], **kwargs(b, "given", False, False))
    assert np.isfinite(p["ce"]).all() and np.all(p["ce"] >= 0.0)
    g = ch.backward(b["logits"], b["act"], np.float32(1.0), **kwargs(b, "given", False, False))
    assert np.isfinite(g).all() and np.all(g[rows[0], b["act"][rows[0]], :5] == 0.0)
    b["logits"][rows[0], b["act"][rows[0]], 40] = -np.inf      # under positive mass: the row's loss is +Inf
    p = ch.rows(b["logits"], b["act"], **kwargs(b, "given", False, False))
    assert p["ce"][rows[0]] == np.inf and np.isfinite(np.delete(p["ce"], rows[0])).all()


def test_an_action_out_of_range_gives_a_nan_loss_and_a_fully_nan_gradient_row():
    b = make_batch(50, 3, 33, 4)
    for wrong in (3, -1, 1 << 40, -(1 << 62)):
        act = b["act"].astype(np.int64)
        act[11] = wrong
        for mode, double in MODES:
            kw = kwargs(b, mode, double, True)
            value, stats, p, _ = ch.loss(b["logits"], act, **kw)
            g = ch.backward(b["logits"], act, np.float32(1.0), **kw)
            assert np.isnan(value) and np.isnan(p["ce"][11]) and np.isnan(g[11]).all() and np.count_nonzero(np.isnan(g)) == 3 * 33
            assert np.isnan(stats[[0, 1, 3]]).all() and np.isfinite(stats[[2, 4, 5, 6, 7]]).all() and np.all(ch.bits(ch.to_f32(g))[11] == 0x7FC00000)


def test_no_row_has_a_value_and_zero_extrema_are_positive_zero():
    x = np.zeros((3, 2, 4), np.float32)
    tp = np.full((3, 4), 0.25, np.float32)
    _, stats, _, _ = ch.loss(x, [5, 5, 5], v_min=-1.0, v_max=1.0, target_probs=tp)
    assert stats[5] == -np.inf and stats[6] == np.inf and stats[7] == -np.inf
    # a symmetric support under a uniform head: qa is a zero; a one-leaf tree passes +0.0
    _, stats, p, _ = ch.loss(x, [0, 1, 0], v_min=-1.5, v_max=1.5, target_probs=tp)
    assert np.all(p["qa"] == 0.0) and np.array_equal(_u64(stats[[1, 6, 7]]), [0, 0, 0])


def test_where_a_permutation_of_the_rows_keeps_the_bits():
    """The rows of lane t of a leaf exchanged with the rows of lane t ^ 1 (all four of them): the first butterfly stage adds the two lanes'
    totals, and an addition commutes."""
    M = 3000
    b = make_batch(M, 2, 33, 11)
    kw = lambda c: kwargs(c, "bootstrap", True, True)
    base = ch.loss(b["logits"], b["act"], **kw(b))
    order = np.arange(M)
    leaf, t = 1024, 37
    for j in range(4):
        x, y = leaf + t + 256 * j, leaf + (t ^ 1) + 256 * j
        order[x], order[y] = y, x
    c = {k: v[order] for k, v in b.items()}
    got = ch.loss(c["logits"], c["act"], **kw(c))
    assert not np.array_equal(b["logits"], c["logits"]) and np.array_equal(_u64(got[1]), _u64(base[1])) and np.array_equal(_u64(got[0]), _u64(base[0]))


def test_q_values_are_the_selecting_pass():
    b = make_batch(500, 6, 51, 12)
    p = ch.rows(b["logits"], b["act"], **kwargs(b, "bootstrap", True, False))
    Q = ch.q_values(b["online"], v_min=V_MIN, v_max=V_MAX)
    assert np.array_equal(ch.first_max(Q), p["jstar"]) and np.array_equal(np.argmax(ch.to_f32(Q), 1), p["jstar"])
    taken = ch.q_values(b["logits"], v_min=V_MIN, v_max=V_MAX)[np.arange(500), b["act"]]
    assert np.array_equal(_u64(taken), _u64(p["qa"]))
    x = b["logits"][:4].copy()
    x[0, 1, 3], x[1, 0, 0], x[2, 2, :] = np.nan, np.inf, -np.inf
    Q = ch.q_values(x, v_min=V_MIN, v_max=V_MAX)
    assert np.isnan(Q[0, 1]) and np.isnan(Q[1, 0]) and np.isnan(Q[2, 2]) and np.count_nonzero(np.isnan(Q)) == 3


# ---- the Python front end ---------------------------------------------------------------------------------------------------------------------
def test_the_front_end_validates_without_a_device():
    code = ("import sys; import gym_amd.c51 as d; assert 'torch' not in sys.modules; import gym_amd; "
            "assert gym_amd.categorical_dqn_loss is d.categorical_dqn_loss and gym_amd.categorical_q_values is d.categorical_q_values; "
            "assert 'torch' not in sys.modules; "
            "assert d.STAT_NAMES[d.Q_TAKEN_MAX] == 'q_taken_max' and d.STAT_NAMES[d.CLIPPED_MASS_MEAN] == 'clipped_mass_mean' and d.LOSS_TERM == 0; "
            "assert d.workspace_bytes(1) == 48 + 64 and d.workspace_bytes(1025) == 48 * 1025 + 128 and d.workspace_bytes((1 << 20) + 5) == 48 * ((1 << 20) + 5) + 64 * 1027; "
            "assert [d.launches(m) for m in (1, 1024, 1025, 1 << 20, (1 << 20) + 5, 1 << 30, (1 << 30) + 1)] == [2, 2, 3, 3, 4, 4, 5]")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
    import torch

    from gym_amd import c51

    assert c51.STAT_NAMES == ch.STAT_NAMES and c51.STATS == len(ch.STAT_NAMES) and c51.LEAF_ROWS == pp.LEAF_ROWS
    assert [c51.launches(m) for m in (1, 3, 1024, 1025, 1024 * 1024 + 5)] == [ch.launches(m) for m in (1, 3, 1024, 1025, 1024 * 1024 + 5)]
    x, a, v = torch.zeros((4, 3, 5)), torch.zeros(4, dtype=torch.int64), torch.zeros(4)
    tp = torch.zeros((4, 5))
    term = torch.zeros(4, dtype=torch.bool)
    boot = dict(reward=v, terminated=term, next_logits=x)
    sup = dict(v_min=0.0, v_max=1.0)
    for kw, what in ((dict(), "exactly one target mode"), (dict(target_probs=tp, reward=v), "exactly one target mode"),
                     (dict(target_probs=tp, next_logits=x), "exactly one target mode"), (dict(target_probs=tp, next_logits_online=x), "next_logits_online"),
                     (dict(reward=v, next_logits=x), "terminated missing"), (dict(reward=v, terminated=term), "next_logits missing"),
                     (dict(target_probs=tp, logits=x.double()), "float32"), (dict(target_probs=tp, logits=[0.0]), "torch tensor"),
                     (dict(target_probs=tp, logits=torch.zeros((4, 65, 5))), "shape"), (dict(target_probs=tp, logits=torch.zeros((4, 3, 65))), "shape"),
                     (dict(target_probs=tp, logits=torch.zeros((4, 3, 1))), "shape"), (dict(target_probs=tp, logits=torch.zeros((4, 5))), "shape"),
                     (dict(target_probs=tp, logits=torch.zeros((4, 5, 3)).transpose(1, 2)), "last two dimensions"),
                     (dict(target_probs=tp, actions=a.float()), "int64"), (dict(target_probs=tp, actions=torch.zeros(3, dtype=torch.int64)), "shape"),
                     (dict(target_probs=torch.zeros((4, 4))), "shape"), (dict(target_probs=tp.double()), "float32"), (dict(boot, reward=v.double()), "float32"),
                     (dict(boot, terminated=v), "uint8"), (dict(boot, next_logits=torch.zeros((4, 3, 4))), "shape"),
                     (dict(boot, next_logits_online=torch.zeros((5, 3, 5))), "shape"), (dict(boot, gamma=float("inf")), "finite"),
                     (dict(boot, gamma="0.9"), "finite"), (dict(target_probs=tp, v_min=1.0), "below v_max"), (dict(target_probs=tp, v_min=2.0), "below v_max"),
                     (dict(target_probs=tp, v_max=float("inf")), "finite"), (dict(target_probs=tp, v_min=float("nan")), "finite"),
                     (dict(target_probs=tp, v_max=True), "finite"), (dict(target_probs=tp, weights=torch.zeros(3)), "shape"),
                     (dict(target_probs=tp, row_loss=torch.zeros(4, dtype=torch.float64)), "float32"), (dict(target_probs=tp, projected=torch.zeros((4, 4))), "shape"),
                     (dict(target_probs=tp.clone().requires_grad_()), "must not require grad"),
                     (dict(boot, next_logits=x.clone().requires_grad_()), "must not require grad"),
                     (dict(target_probs=tp, weights=v.clone().requires_grad_()), "must not require grad"),
                     (dict(target_probs=tp, logits=x.clone().requires_grad_(), out=(torch.zeros(()), torch.zeros(8))), "requires grad"),
                     (dict(target_probs=tp, logits=x.clone().requires_grad_(), workspace=torch.zeros(64, dtype=torch.float64)), "requires grad"),
                     (dict(target_probs=tp, out=(torch.zeros(()),)), "2 entries"), (dict(target_probs=tp, out=(torch.zeros(()), torch.zeros(7))), "shape"),
                     (dict(target_probs=tp), "device tensor"), (dict(boot), "device tensor")):
        args = dict(sup, logits=x, actions=a)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            c51.categorical_dqn_loss(args.pop("logits"), args.pop("actions"), **args)
    with pytest.raises(TypeError):
        c51.categorical_dqn_loss(x, a, target_probs=tp)      # v_min and v_max have no default
    for kw, what in ((dict(logits=x.double()), "float32"), (dict(logits=torch.zeros((4, 5))), "shape"), (dict(v_min=1.0), "below v_max"),
                     (dict(out=torch.zeros((4, 2))), "shape"), (dict(), "device tensor")):
        args = dict(sup, logits=x)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            c51.categorical_q_values(args.pop("logits"), **args)
    with pytest.raises(ValueError, match="rows"):
        c51.workspace_bytes(0)
