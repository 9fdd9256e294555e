"""tests/qr_host.py — the NumPy twin of include/mxv_qr.h, which the device is compared with bit for bit — held to a literal torch float64
implementation of the quantile-regression (QR-DQN) loss written here (mean over the quantiles, argmax, gather, the Bellman step with a
scalar gamma or a per-row discount, the [M, N, N] tensor of pairwise errors, huber, |tau - 1{u < 0}|, mean over the targets, sum over the
head, times the weights, .mean(), autograd for the gradient) and to the exact cases of the rule; and what needs no device of the front
end.

How the comparison is scaled (u = 2^-53; the B_* constants of the twin are what was measured on the 20 000-row input below, nothing is
tuned): the targets T are the SAME float64 operations on both sides (reward + g * next), so they are held to max(1, |T|) u times their
bar; a row's loss is a sum of N^2 non-negative terms in two different orders, held relative to max(1, |reference|); the loss and the
four means are held in units of the mean magnitude of what they sum (a mean of signed values may cancel); a gradient element in units
of |g| / M times the row's weight (it is at most that: a mean over j of |dh / kappa| <= 1 times a weight <= 1, over N).  The small
shapes hold twice the measured maxima, rounded up (policy_eval_host.bar): the margin covers a different summation order of the literal
implementation at another shape.  The only discontinuity is the argmax: rows whose two largest Q_a are equal or adjacent floats are
counted, and the inputs have none.  (The weight |tau - 1{u < 0}| jumps at u = 0, where the Huber term and its derivative are 0.)"""
import subprocess
import sys

import numpy as np
import pytest

import dqn_host as dh
import ppo_host as pp
import qr_host as qh
from conftest import ROOT
from policy_eval_host import bar

U = 2.0 ** -53
M_BIG, A_BIG, N_BIG = 20_000, 6, 51
GAMMA = 0.99
# (target mode, double, bootstrap factor)
MODES = (("given", False, None), ("bootstrap", False, "gamma"), ("bootstrap", True, "gamma"), ("bootstrap", False, "discount"),
         ("bootstrap", True, "discount"))
SMALL = ((1, 1), (3, 51), (2, 64))
NAMES = ("TARGETS", "ROW_LOSS", "LOSS", "STATS", "GRAD")


def _u64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def make_batch(M, A, N, seed):
    """M rows of A actions of N quantiles.  Most heads are sorted (a trained head); every fifth row is left as drawn (crossings).
    Cycling through the rows: a tenth terminated, a tenth with rewards far from the head (the linear branch of the Huber term on every
    pair); the rest ordinary.  discount is gamma^n for n = 1 .. 5 cycling, as an n-step ring stores it (float32 of the float64 power)."""
    rng = np.random.default_rng(seed)
    k = np.arange(M)

    def head():
        x = rng.standard_normal((M, A, N)) * 2.0 + rng.standard_normal((M, A, 1))
        s = np.sort(x, -1)
        s[k % 5 == 0] = x[k % 5 == 0]
        return s.astype(np.float32)

    quantiles, nxt = head(), head()
    online = (nxt + 0.7 * rng.standard_normal((M, A, 1))).astype(np.float32)
    act = rng.integers(0, A, M)
    reward = rng.standard_normal(M).astype(np.float32)
    term = np.zeros(M, np.uint8)
    term[k % 10 == 1] = 1
    far = k % 10 == 2
    reward[far] = rng.choice(np.array([-50.0, 50.0, 21.5], np.float32), far.sum())
    discount = (np.float64(GAMMA) ** (1 + k % 5)).astype(np.float32)
    target_quantiles = np.sort(rng.standard_normal((M, N)) * 2.0 + rng.standard_normal((M, 1)), -1).astype(np.float32)
    weights = rng.uniform(0.2, 2.0, M).astype(np.float32)
    return dict(quantiles=quantiles, act=act, next=nxt, online=online, reward=reward, term=term, discount=discount,
                target_quantiles=target_quantiles, weights=weights)


def kwargs(b, mode, double, factor, weighted, kappa=1.0, gamma=GAMMA):
    kw = dict(kappa=kappa, weights=b["weights"] if weighted else None)
    if mode == "given":
        kw["target_quantiles"] = b["target_quantiles"]
    else:
        kw.update(reward=b["reward"], terminated=b["term"], next_quantiles=b["next"], next_quantiles_online=b["online"] if double else None)
        kw.update(dict(gamma=gamma) if factor == "gamma" else dict(discount=b["discount"]))
    return kw


def near_ties(sel):
    """Rows whose two largest expected values are equal or adjacent floats: where an argmax may legitimately differ."""
    Q = np.sort(qh.q_values(sel), axis=1)
    if Q.shape[1] < 2:
        return 0
    return int(np.count_nonzero(np.nextafter(Q[:, -2], np.inf) >= Q[:, -1]))


def torch_reference(b, mode, double, factor, weighted, grad_loss=1.0, kappa=1.0, gamma=GAMMA):
    """The literal torch sequence in float64 on the CPU, and its autograd."""
    import torch

    f = lambda x: torch.from_numpy(np.asarray(x, np.float32).astype(np.float64))
    quantiles = f(b["quantiles"]).requires_grad_()
    M, A, N = quantiles.shape
    a = torch.from_numpy(np.asarray(b["act"], np.int64))
    rows = torch.arange(M)
    tau = (2 * torch.arange(N, dtype=torch.float64) + 1) / (2 * N)
    if mode == "given":
        T = f(b["target_quantiles"]).reshape(M, N)
    else:
        nxt = f(b["next"])
        sel = f(b["online"]) if double else nxt
        nv = nxt[rows, sel.mean(-1).argmax(1)]
        g = gamma if factor == "gamma" else f(b["discount"])[:, None]
        live = torch.from_numpy(b["term"] == 0)[:, None]
        T = torch.where(live, f(b["reward"])[:, None] + g * nv, f(b["reward"])[:, None].expand(M, N))
    th = quantiles[rows, a]
    u = T[:, None, :] - th[:, :, None]                                   # [M, k, j]
    hub = torch.where(u.abs() <= kappa, 0.5 * u ** 2, kappa * (u.abs() - 0.5 * kappa))
    rho = (tau[None, :, None] - (u.detach() < 0).double()).abs() * hub / kappa
    ql = rho.mean(2).sum(1)
    term = ql * f(b["weights"]) if weighted else ql
    loss = term.mean()
    (grad_loss * loss).backward()
    with torch.no_grad():
        qa, y = th.mean(1), T.mean(1)
        cr = (th[:, 1:] < th[:, :-1]).double().mean(1) if N > 1 else torch.zeros(M, dtype=torch.float64)
        stats = [float(loss), float(qa.mean()), float(y.mean()), float((qa - y).abs().mean()), float(cr.mean()), float(ql.max()), float(qa.min()),
                 float(qa.max())]
    return dict(loss=float(loss.detach()), stats=np.array(stats), T=T.numpy(), ql=ql.detach().numpy(), grad=quantiles.grad.numpy())


def compare(b, mode, double, factor, weighted, grad_loss=2.5):
    """One configuration against torch -> the worst ratios (targets, row loss, loss, stats, gradient), in u."""
    M, A, N = b["quantiles"].shape
    if mode == "bootstrap":
        assert near_ties(b["online"] if double else b["next"]) == 0
    kw = kwargs(b, mode, double, factor, weighted)
    value, stats, p, _ = qh.loss(b["quantiles"], b["act"], **kw)
    grad = qh.backward(b["quantiles"], b["act"], np.float32(grad_loss), **kw)
    ref = torch_reference(b, mode, double, factor, weighted, grad_loss)
    assert np.all(p["T"][:, N:] == 0.0) and np.all(p["s"][:, N:] == 0.0)
    w_t = float(np.max(np.abs(p["T"][:, :N] - ref["T"]) / (U * np.maximum(1.0, np.abs(ref["T"])))))
    w_ql = float(np.max(np.abs(p["ql"] - ref["ql"]) / (U * np.maximum(1.0, np.abs(ref["ql"])))))
    diff = np.abs(stats - ref["stats"])
    mags = np.array([np.mean(np.abs(p["term"])), np.mean(np.abs(p["qa"])), np.mean(np.abs(p["y"])), np.mean(p["ae"]), np.mean(p["cr"])])
    nz = mags != 0.0
    assert np.all(diff[:5][~nz] == 0.0)
    w_stats = float(np.max(diff[1:5][nz[1:]] / (U * mags[1:][nz[1:]]))) if nz[1:].any() else 0.0
    w_loss = abs(value - ref["loss"]) / (U * mags[0])
    # the extrema are one row's value each: the row bar
    # (a mean of N values in two orders: each within (N - 1) u of the sum of the magnitudes, and a quotient each)
    assert abs(stats[5] - ref["stats"][5]) <= bar(qh.B_ROW_LOSS) * U * max(1.0, abs(ref["stats"][5]))
    assert np.all(diff[6:] <= 2 * (N + 1) * U * float(np.abs(b["quantiles"]).max()))
    w = np.ones(M) if p["w"] is None else p["w"]
    scale = abs(grad_loss) / M * w
    taken, ref_taken = grad[np.arange(M), b["act"]], ref["grad"][np.arange(M), b["act"]]
    w_g = float(np.max(np.abs(taken - ref_taken) / (U * scale[:, None])))
    off = np.ones(grad.shape[:2], bool)
    off[np.arange(M), b["act"]] = False
    assert np.all(_u64(grad[off]) == 0) and np.all(ref["grad"][off] == 0.0)      # +0.0 outside the taken action
    loss32, stats32, rl32, to32 = qh.loss_f32(b["quantiles"], b["act"], **kw)
    assert np.all(rl32 >= 0.0) and to32.shape == (M, N) and abs(float(loss32) - ref["loss"]) <= np.spacing(np.float32(abs(ref["loss"])))
    return np.array([w_t, w_ql, w_loss, w_stats, w_g])


def _all_options(b):
    worst = np.zeros(5)
    for mode, double, factor in MODES:
        for weighted in (True, False):
            worst = np.maximum(worst, compare(b, mode, double, factor, weighted))
    return worst


# ---- against the literal torch implementation ------------------------------------------------------------------------------------------------
def test_the_twin_against_the_literal_implementation_on_20000_rows():
    b = make_batch(M_BIG, A_BIG, N_BIG, 1)
    p = qh.rows(b["quantiles"], b["act"], **kwargs(b, "bootstrap", True, "discount", False))
    assert (b["term"] != 0).sum() >= M_BIG // 10 and (p["cr"] > 0.2).sum() >= M_BIG // 10 and (p["cr"] == 0.0).sum() >= M_BIG // 2
    assert (p["ae"] > 10.0).sum() >= M_BIG // 20 and len(set(b["discount"].tolist())) == 5
    worst = _all_options(b)
    for name, w in zip(NAMES, worst):
        # the named constant is what was measured on this input (to its two decimals, rounded up)
        bnd = getattr(qh, "B_" + name)
        print(f"measured B_{name}: {w:.4f}")
        assert w <= bnd < w + 0.01, (name, w, bnd)


@pytest.mark.parametrize("M", (1, 2, 1023, 1025))
def test_small_batches_agree_with_the_literal_implementation(M):
    for A, N in SMALL:
        worst = _all_options(make_batch(M, A, N, 100 + M + A + N))
        for name, w in zip(NAMES, worst):
            assert w <= bar(getattr(qh, "B_" + name)), (M, A, N, name, w)


# ---- exact cases ----------------------------------------------------------------------------------------------------------------------------
def test_one_quantile_with_kappa_one_is_half_the_huber_loss_of_the_scalar_twin():
    M, A = 300, 4
    b = make_batch(M, A, 1, 7)
    b["reward"][::7] *= 5.0      # both branches of the Huber term
    for weighted in (True, False):
        kw = kwargs(b, "bootstrap", True, "gamma", weighted)
        p = qh.rows(b["quantiles"], b["act"], **kw)
        q, nq, on = (b[k][:, :, 0] for k in ("quantiles", "next", "online"))
        d = dh.rows(q, b["act"], reward=b["reward"], terminated=b["term"], next_q=nq, next_q_online=on, gamma=GAMMA, delta=1.0,
                    weights=b["weights"] if weighted else None)
        assert np.array_equal(_u64(p["qa"]), _u64(d["qa"])) and np.array_equal(_u64(p["y"]), _u64(d["y"]))
        assert np.array_equal(_u64(p["ql"]), _u64(0.5 * d["h"])) and (d["ae"] > 1.0).sum() > 20 and (d["ae"] <= 1.0).sum() > 20
        g = qh.backward(b["quantiles"], b["act"], np.float32(2.5), **kw)[:, :, 0]
        gd = dh.backward(q, b["act"], np.float32(2.5), reward=b["reward"], terminated=b["term"], next_q=nq, next_q_online=on, gamma=GAMMA, delta=1.0,
                         weights=b["weights"] if weighted else None)
        assert np.array_equal(_u64(g + 0.0), _u64(0.5 * gd + 0.0)) and np.count_nonzero(g) > M // 2
        assert np.all(p["cr"] == 0.0)      # N = 1: no pair to cross


def test_a_constant_discount_gives_the_bits_of_the_scalar_gamma():
    b = make_batch(500, 3, 51, 8)
    b["discount"][:] = 0.96875
    for double in (False, True):
        one = qh.loss(b["quantiles"], b["act"], **kwargs(b, "bootstrap", double, "gamma", True, gamma=0.96875))
        per = qh.loss(b["quantiles"], b["act"], **kwargs(b, "bootstrap", double, "discount", True))
        assert np.array_equal(_u64(one[1]), _u64(per[1])) and np.array_equal(_u64(one[2]["ql"]), _u64(per[2]["ql"]))
        assert np.array_equal(_u64(one[2]["T"]), _u64(per[2]["T"])) and np.array_equal(_u64(one[2]["d"]), _u64(per[2]["d"]))


def test_a_discount_row_of_mixed_powers_matches_the_literal_form():
    M, A, N = 400, 3, 33
    b = make_batch(M, A, N, 9)
    steps = 1 + np.arange(M) % 5
    assert np.array_equal(b["discount"], (np.float64(GAMMA) ** steps).astype(np.float32)) and len(set(steps)) == 5
    p = qh.rows(b["quantiles"], b["act"], **kwargs(b, "bootstrap", False, "discount", False))
    ref = torch_reference(b, "bootstrap", False, "discount", False)
    assert np.array_equal(_u64(p["T"][:, :N]), _u64(ref["T"]))      # the same float64 operations on both sides
    live = b["term"] == 0
    j = p["jstar"]
    want = b["reward"].astype(np.float64)[:, None] + b["discount"].astype(np.float64)[:, None] * b["next"][np.arange(M), j].astype(np.float64)
    assert np.array_equal(_u64(p["T"][live, :N]), _u64(want[live])) and np.all(p["T"][~live, :N] == b["reward"][~live, None])


def test_a_terminated_row_ignores_both_next_tensors_and_the_discount_entirely():
    b = make_batch(40, 3, 51, 2)
    b["term"][:] = 0
    b["term"][[5, 6, 7, 8]] = 1
    kw = lambda c: kwargs(c, "bootstrap", True, "discount", True)
    clean = qh.loss(b["quantiles"], b["act"], **kw(b))
    gclean = qh.backward(b["quantiles"], b["act"], np.float32(1.0), **kw(b))
    b["next"][5], b["online"][6], b["next"][7, 1] = np.nan, np.inf, -np.inf
    b["online"][7] = np.nan
    b["discount"][[5, 6]], b["discount"][7], b["discount"][8] = np.nan, np.inf, -np.inf
    got = qh.loss(b["quantiles"], b["act"], **kw(b))
    assert np.isfinite(got[1]).all() and np.array_equal(_u64(got[1]), _u64(clean[1])) and np.array_equal(_u64(got[2]["ql"]), _u64(clean[2]["ql"]))
    assert np.array_equal(_u64(got[2]["T"]), _u64(clean[2]["T"]))
    assert np.array_equal(_u64(qh.backward(b["quantiles"], b["act"], np.float32(1.0), **kw(b))), _u64(gclean))


@pytest.mark.parametrize("A", (2, 4, 7, 64))
def test_ties_take_the_first_maximum(A):
    N = 5
    b = make_batch(50, A, N, 20 + A)
    b["term"][:] = 0
    b["online"][41] = b["online"][41, 0]                    # every action ties: the first
    b["online"][40] = b["online"][41, 0] - 3.0
    b["online"][40, [A // 2, A - 1]] = b["online"][41, 0]   # two maxima: the earlier
    for a in range(A):
        b["next"][40:42, a] = float(a)                      # the evaluating network marks action a by its value
    p = qh.rows(b["quantiles"], b["act"], **kwargs(b, "bootstrap", True, "gamma", False, gamma=1.0))
    assert p["jstar"][41] == 0 and p["jstar"][40] == A // 2
    assert np.all(p["T"][41, :N] == b["reward"][41]) and np.all(p["T"][40, :N] == np.float64(b["reward"][40]) + float(A // 2))
    assert np.array_equal(qh.first_max(qh.q_values(b["online"])), p["jstar"])


def test_the_crossing_fraction_of_ascending_descending_and_single_quantiles():
    M, A, N = 30, 3, 33
    b = make_batch(M, A, N, 4)
    asc = np.sort(b["quantiles"], -1)
    asc += np.arange(N, dtype=np.float32) * 0.01      # strictly
    for q, want in ((asc, 0.0), (asc[..., ::-1].copy(), 1.0)):
        value, stats, p, _ = qh.loss(q, b["act"], **kwargs(b, "given", False, None, True))
        assert np.all(p["cr"] == want) and stats[4] == want
    eq = np.zeros((M, A, N), np.float32)              # equal neighbours are not out of order
    assert np.all(qh.rows(eq, b["act"], **kwargs(b, "given", False, None, False))["cr"] == 0.0)
    one = make_batch(M, A, 1, 5)
    assert np.all(qh.rows(one["quantiles"], one["act"], **kwargs(one, "given", False, None, False))["cr"] == 0.0)
    half = asc.copy()
    half[:, :, 1::2] -= 100.0                         # every second pair crosses: 16 of 32
    assert np.all(qh.rows(half, b["act"], **kwargs(b, "given", False, None, False))["cr"] == 0.5)


def test_a_nan_in_one_taken_row_makes_that_row_nan_and_no_other():
    M, A, N = 300, 4, 51
    b = make_batch(M, A, N, 3)
    others = np.arange(M) != 17
    for mode, double, factor in MODES:
        kw = lambda c: kwargs(c, mode, double, factor, False)
        clean = qh.backward(b["quantiles"], b["act"], np.float32(1.0), **kw(b))
        c = {k: v.copy() for k, v in b.items()}
        c["quantiles"][17, c["act"][17], :] = np.nan
        value, stats, p, _ = qh.loss(c["quantiles"], c["act"], **kw(c))
        g = qh.backward(c["quantiles"], c["act"], np.float32(1.0), **kw(c))
        assert np.isnan(value) and np.isnan(p["ql"][17]) and np.isfinite(p["ql"][others]).all()
        assert np.isnan(g[17, c["act"][17]]).all() and np.count_nonzero(np.isnan(g)) == N
        assert np.all(qh.bits(qh.to_f32(g))[17, c["act"][17]] == 0x7FC00000) and qh.bits(qh.loss_f32(c["quantiles"], c["act"], **kw(c))[0]) == 0x7FC00000
        assert np.array_equal(_u64(g[others]), _u64(clean[others]))
        # the extrema skip the NaN row
        assert stats[5] == p["ql"][others].max() and stats[6] == p["qa"][others].min() and stats[7] == p["qa"][others].max()
    # one NaN quantile th_k: the row's loss is NaN; by the rule d_k alone meets it (lane k owns th_k), so column k is NaN and the other
    # columns keep the values they have against the same targets
    c = {k: v.copy() for k, v in b.items()}
    c["quantiles"][17, c["act"][17], 5] = np.nan
    kw = kwargs(c, "bootstrap", True, "discount", True)
    value, stats, p, _ = qh.loss(c["quantiles"], c["act"], **kw)
    g = qh.backward(c["quantiles"], c["act"], np.float32(1.0), **kw)
    clean = qh.backward(b["quantiles"], b["act"], np.float32(1.0), **kwargs(b, "bootstrap", True, "discount", True))
    assert np.isnan(value) and np.isnan(p["ql"][17]) and np.isnan(p["qa"][17]) and np.isnan(g[17, c["act"][17], 5]) and np.count_nonzero(np.isnan(g)) == 1
    assert np.array_equal(_u64(np.delete(g[17, c["act"][17]], 5)), _u64(np.delete(clean[17, c["act"][17]], 5))) and np.array_equal(_u64(g[others]), _u64(clean[others]))
    # one NaN target quantile T_j reaches every lane: the taken row's N columns
    c = {k: v.copy() for k, v in b.items()}
    c["target_quantiles"][17, 7] = np.nan
    g = qh.backward(c["quantiles"], c["act"], np.float32(1.0), **kwargs(c, "given", False, None, True))
    assert np.isnan(g[17, c["act"][17]]).all() and np.count_nonzero(np.isnan(g)) == N
    # a NaN in the selecting row: the targets are NaN, the taken row's N columns and nothing else
    c = {k: v.copy() for k, v in b.items()}
    c["term"][17] = 0
    c["online"][17, 2, 5] = np.nan
    kw = kwargs(c, "bootstrap", True, "discount", True)
    p = qh.rows(c["quantiles"], c["act"], **kw)
    g = qh.backward(c["quantiles"], c["act"], np.float32(1.0), **kw)
    assert np.isnan(p["T"][17, :N]).all() and np.isnan(p["ql"][17]) and np.isfinite(p["qa"]).all() and np.count_nonzero(np.isnan(g)) == N


def test_an_action_out_of_range_gives_a_nan_loss_and_a_fully_nan_gradient_row():
    b = make_batch(50, 3, 33, 4)
    for wrong in (-1, 3, 1 << 31, -(1 << 62)):
        act = b["act"].astype(np.int64)
        act[11] = wrong
        for mode, double, factor in MODES:
            kw = kwargs(b, mode, double, factor, True)
            value, stats, p, _ = qh.loss(b["quantiles"], act, **kw)
            g = qh.backward(b["quantiles"], act, np.float32(1.0), **kw)
            assert np.isnan(value) and np.isnan(p["ql"][11]) and np.isnan(g[11]).all() and np.count_nonzero(np.isnan(g)) == 3 * 33
            assert np.isnan(stats[[0, 1, 3, 4]]).all() and np.isfinite(stats[[2, 5, 6, 7]]).all() and np.all(qh.bits(qh.to_f32(g))[11] == 0x7FC00000)


def test_no_row_has_a_value_and_zero_extrema_are_positive_zero():
    x = np.zeros((3, 2, 4), np.float32)
    tq = np.zeros((3, 4), np.float32)
    _, stats, _, _ = qh.loss(x, [5, 5, 5], target_quantiles=tq)
    assert stats[5] == -np.inf and stats[6] == np.inf and stats[7] == -np.inf
    _, stats, p, _ = qh.loss(-x, [0, 1, 0], target_quantiles=tq)
    assert np.all(p["ql"] == 0.0) and np.array_equal(_u64(stats), np.zeros(8, np.uint64))


def test_q_values_are_the_selecting_pass_and_the_taken_mean():
    b = make_batch(500, 6, 51, 12)
    p = qh.rows(b["quantiles"], b["act"], **kwargs(b, "bootstrap", True, "gamma", False))
    Q = qh.q_values(b["online"])
    assert np.array_equal(qh.first_max(Q), p["jstar"]) and np.array_equal(np.argmax(qh.to_f32(Q), 1), p["jstar"])
    assert np.array_equal(_u64(qh.q_values(b["quantiles"])[np.arange(500), b["act"]]), _u64(p["qa"]))
    x = b["quantiles"][:3].copy()
    x[0, 1, 3], x[1, 0, 0], x[1, 0, 1] = np.nan, np.inf, -np.inf
    Q = qh.q_values(x)
    assert np.isnan(Q[0, 1]) and np.isnan(Q[1, 0]) and np.count_nonzero(np.isnan(Q)) == 2


def test_kappa_scales_the_two_branches():
    """rho_kappa = huber_kappa / kappa: for |u| <= kappa it is u^2 / (2 kappa), beyond it |u| - kappa / 2 — exactly, on values that are
    powers of two."""
    q = np.zeros((2, 1, 1), np.float32)
    for kappa, T, want in ((2.0, 1.0, 0.5 * 0.25), (2.0, 8.0, 0.5 * 7.0), (0.5, 0.25, 0.5 * 0.0625), (0.5, -4.0, 0.5 * 3.75)):
        p = qh.rows(q, [0, 0], target_quantiles=np.full((2, 1), T, np.float32), kappa=kappa)
        assert np.all(p["ql"] == want), (kappa, T, p["ql"])


# ---- the Python front end ---------------------------------------------------------------------------------------------------------------------
def test_the_front_end_validates_without_a_device():
    code = ("import sys; import gym_amd.qr as d; assert 'torch' not in sys.modules; import gym_amd; "
            "assert gym_amd.quantile_dqn_loss is d.quantile_dqn_loss and gym_amd.quantile_q_values is d.quantile_q_values; "
            "assert 'torch' not in sys.modules; "
            "assert d.STAT_NAMES[d.Q_TAKEN_MAX] == 'q_taken_max' and d.STAT_NAMES[d.CROSSING_FRACTION] == 'crossing_fraction' and d.LOSS_TERM == 0; "
            "assert d.MAX_QUANTILES == 64 and d.TD_ABS_MEAN == 3; "
            "assert d.workspace_bytes(1) == 48 + 64 and d.workspace_bytes(1025) == 48 * 1025 + 128 and d.workspace_bytes((1 << 20) + 5) == 48 * ((1 << 20) + 5) + 64 * 1027; "
            "assert [d.launches(m) for m in (1, 1024, 1025, 1 << 20, (1 << 20) + 5, 1 << 30, (1 << 30) + 1)] == [2, 2, 3, 3, 4, 4, 5]")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
    import torch

    from gym_amd import qr

    assert qr.STAT_NAMES == qh.STAT_NAMES and qr.STATS == len(qh.STAT_NAMES) and qr.LEAF_ROWS == pp.LEAF_ROWS
    assert [qr.launches(m) for m in (1, 3, 1024, 1025, 1024 * 1024 + 5)] == [qh.launches(m) for m in (1, 3, 1024, 1025, 1024 * 1024 + 5)]
    x, a, v = torch.zeros((4, 3, 5)), torch.zeros(4, dtype=torch.int64), torch.zeros(4)
    tq = torch.zeros((4, 5))
    term = torch.zeros(4, dtype=torch.bool)
    boot = dict(reward=v, terminated=term, next_quantiles=x)
    for kw, what in ((dict(), "exactly one target mode"), (dict(target_quantiles=tq, reward=v), "exactly one target mode"),
                     (dict(target_quantiles=tq, next_quantiles=x), "exactly one target mode"),
                     (dict(target_quantiles=tq, next_quantiles_online=x), "next_quantiles_online is given with target_quantiles"),
                     (dict(target_quantiles=tq, discount=v), "discount is given with target_quantiles"),
                     (dict(boot, gamma=0.9, discount=v), "gamma and discount are both given"),
                     (dict(reward=v, next_quantiles=x), "terminated missing"), (dict(reward=v, terminated=term), "next_quantiles missing"),
                     (dict(target_quantiles=tq, quantiles=x.double()), "float32"), (dict(target_quantiles=tq, quantiles=[0.0]), "torch tensor"),
                     (dict(target_quantiles=tq, quantiles=torch.zeros((4, 65, 5))), "shape"),
                     (dict(target_quantiles=tq, quantiles=torch.zeros((4, 3, 65))), "shape"), (dict(target_quantiles=tq, quantiles=torch.zeros((4, 5))), "shape"),
                     (dict(target_quantiles=tq, quantiles=torch.zeros((4, 5, 3)).transpose(1, 2)), "last two dimensions"),
                     (dict(target_quantiles=tq, actions=a.float()), "int64"), (dict(target_quantiles=tq, actions=torch.zeros(3, dtype=torch.int64)), "shape"),
                     (dict(target_quantiles=torch.zeros((4, 4))), "shape"), (dict(target_quantiles=tq.double()), "float32"),
                     (dict(boot, reward=v.double()), "float32"), (dict(boot, terminated=v), "uint8"), (dict(boot, discount=v.double()), "float32"),
                     (dict(boot, discount=torch.zeros(3)), "shape"), (dict(boot, next_quantiles=torch.zeros((4, 3, 4))), "shape"),
                     (dict(boot, next_quantiles_online=torch.zeros((5, 3, 5))), "shape"), (dict(boot, gamma=float("inf")), "finite"),
                     (dict(boot, gamma="0.9"), "finite"), (dict(target_quantiles=tq, kappa=0.0), "above 0"), (dict(target_quantiles=tq, kappa=-1.0), "above 0"),
                     (dict(target_quantiles=tq, kappa=float("inf")), "finite"), (dict(target_quantiles=tq, kappa=float("nan")), "finite"),
                     (dict(target_quantiles=tq, kappa=True), "finite"), (dict(target_quantiles=tq, weights=torch.zeros(3)), "shape"),
                     (dict(target_quantiles=tq, row_loss=torch.zeros(4, dtype=torch.float64)), "float32"),
                     (dict(target_quantiles=tq, targets_out=torch.zeros((4, 4))), "shape"),
                     (dict(target_quantiles=tq.clone().requires_grad_()), "must not require grad"),
                     (dict(boot, next_quantiles=x.clone().requires_grad_()), "must not require grad"),
                     (dict(boot, discount=v.clone().requires_grad_()), "must not require grad"),
                     (dict(target_quantiles=tq, weights=v.clone().requires_grad_()), "must not require grad"),
                     (dict(target_quantiles=tq, quantiles=x.clone().requires_grad_(), out=(torch.zeros(()), torch.zeros(8))), "requires grad"),
                     (dict(target_quantiles=tq, quantiles=x.clone().requires_grad_(), workspace=torch.zeros(64, dtype=torch.float64)), "requires grad"),
                     (dict(target_quantiles=tq, out=(torch.zeros(()),)), "2 entries"), (dict(target_quantiles=tq, out=(torch.zeros(()), torch.zeros(7))), "shape"),
                     (dict(target_quantiles=tq), "device tensor"), (dict(boot), "device tensor"), (dict(boot, discount=v), "device tensor")):
        args = dict(quantiles=x, actions=a)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            qr.quantile_dqn_loss(args.pop("quantiles"), args.pop("actions"), **args)
    for kw, what in ((dict(quantiles=x.double()), "float32"), (dict(quantiles=torch.zeros((4, 5))), "shape"), (dict(out=torch.zeros((4, 2))), "shape"),
                     (dict(), "device tensor")):
        args = dict(quantiles=x)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            qr.quantile_q_values(args.pop("quantiles"), **args)
    with pytest.raises(ValueError, match="rows"):
        qr.workspace_bytes(0)
