"""tests/sac_host.py — the NumPy twin of include/mxv_sac.h, which the device is compared with bit for bit — held to torch's float64 autograd
of the literal expressions of examples/sac_pendulum.py (torch.minimum, huber_loss, mean), to exact sums and to the exact cases of the
rule; and what needs no device of the front end.

How the bars are derived (u = 2^-53; nothing here is tuned to what the twin gives):
  * the soft target: min_c next_q is a selection, and nv - al * lp, g * v and r + ... are the same float64 operations on both sides (the
    factor (1 - terminated) of the literal expression is exactly 1 or 0, and g * 1 is g): y is EQUAL, which is asserted.
  * a row of the critics: e_c and |e_c| are then the same operations too.  A Huber value is two or three more operations whose order
    torch does not document, the sum over the C critics C - 1 roundings on either side, the weight one more: (4 + 2 C) u |term| per row.
    The means over the critics of |e_c| and q_c: C roundings on either side, 2 C u of the row's mean of magnitudes.  The gap max - min
    is one operation on selections: exact.
  * a row of the actor: al * lp - min_c q and the weight are the same operations on both sides: exact, which is asserted through a bar
    without a row term.
  * a mean of M terms: the rows' own differences, EB(sum |term|) = norm_tree_host.sum_error_bound(ppo_host.depth(M), sum |term|) for
    the twin's tree, (M - 1) u sum |term| for whatever order torch sums in, one rounding for each quotient.
  * a gradient g / M * w * dH (g / M * w * al, g / M * w): three roundings here, a handful in torch's chain: 8 u |gradient|.
  * a float32 output: half a float32 ulp of the reference on top of its float64 bar.
  * the extrema, td_error and the fraction of rows whose minimum is a later critic are selections and counts of identical float64
    values: exact.
The only discontinuities are the minimum over the critics and the farthest error: the inputs are continuous draws, and the test asserts
that no row holds a tied minimum or two equal |e_c|, so no row is excluded."""
import math
import sys

import numpy as np
import pytest

import norm_tree_host as nt
import sac_host as sh

U = 2.0 ** -53
M_BIG = 20_000
CRITICS = (1, 2, 5)
GAMMA, ALPHA = 0.99, 0.2
SLOP = 1.0 + 1e-6          # the second-order terms the first-order bounds above leave out
# (target mode, entropy term, per-row discount)
MODES = (("targets", False, False), ("bootstrap", False, False), ("bootstrap", True, False), ("bootstrap", False, True), ("bootstrap", True, True))


def _u64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64) * (1 + 1e-6)).astype(np.float32)).astype(np.float64)


def make_batch(M, C, seed):
    """M rows of C critic values, all continuous draws: TD errors on both sides of delta = 1, a tenth of the rows terminated, per-row
    discounts gamma^1 .. gamma^3."""
    rng = np.random.default_rng(seed)
    q = (rng.standard_normal((M, C)) * 2.0).astype(np.float32)
    next_q = (rng.standard_normal((M, C)) * 2.0).astype(np.float32)
    reward = rng.standard_normal(M).astype(np.float32)
    term = (rng.uniform(size=M) < 0.1).astype(np.uint8)
    targets = (q.mean(1) + 1.2 * rng.standard_normal(M)).astype(np.float32)
    weights = rng.uniform(0.2, 2.0, M).astype(np.float32)
    log_prob = (rng.standard_normal(M) * 1.5 - 1.0).astype(np.float32)
    next_lp = (rng.standard_normal(M) * 1.5 - 1.0).astype(np.float32)
    discount = (GAMMA ** rng.integers(1, 4, M)).astype(np.float32)
    return dict(q=q, next_q=next_q, reward=reward, term=term, targets=targets, weights=weights, log_prob=log_prob, next_lp=next_lp,
                discount=discount)


def kwargs(b, mode, entropy, per_row, weighted, delta):
    kw = dict(delta=delta, weights=b["weights"] if weighted else None)
    if mode == "targets":
        kw["targets"] = b["targets"]
        return kw
    kw.update(reward=b["reward"], terminated=b["term"], next_q=b["next_q"])
    kw.update(discount=b["discount"]) if per_row else kw.update(gamma=GAMMA)
    if entropy:
        kw.update(next_log_prob=b["next_lp"], alpha=ALPHA)
    return kw


def tied_rows(x):
    """Rows of x [M, C] whose two smallest values are equal: where a minimum may legitimately be either."""
    s = np.sort(np.asarray(x), axis=1)
    return 0 if s.shape[1] < 2 else int(np.count_nonzero(s[:, 0] == s[:, 1]))


def _f(x):
    import torch

    return torch.from_numpy(np.asarray(x, np.float32).astype(np.float64))


def torch_target(b, entropy, per_row):
    """The literal soft target of examples/sac_pendulum.py in float64."""
    import torch

    v = _f(b["next_q"]).min(dim=1).values      # torch.minimum over the critics' columns
    if entropy:
        v = v - ALPHA * _f(b["next_lp"])
    g = _f(b["discount"]) if per_row else GAMMA
    return _f(b["reward"]) + g * (1.0 - torch.from_numpy(b["term"].astype(np.float64))) * v


def torch_critics(b, mode, entropy, per_row, weighted, delta, grad_loss):
    import torch
    import torch.nn.functional as F

    q = _f(b["q"]).requires_grad_()
    y = _f(b["targets"]) if mode == "targets" else torch_target(b, entropy, per_row)
    H = F.huber_loss(q, y[:, None].expand_as(q), reduction="none", delta=delta) if math.isfinite(delta) else 0.5 * (q - y[:, None]) ** 2
    h = H[:, 0]
    for c in range(1, q.shape[1]):
        h = h + H[:, c]
    if weighted:
        h = h * _f(b["weights"])
    loss = h.mean()
    (grad_loss * loss).backward()
    with torch.no_grad():
        e = q - y[:, None]
        far = e.gather(1, e.abs().argmax(1, keepdim=True)).squeeze(1)
        stats = [float(loss), float(e.abs().mean(1).mean()), float(q.mean(1).mean()), float(y.mean()),
                 float((q.max(1).values - q.min(1).values).mean()), float(e.abs().max()), float(q.min()), float(q.max())]
    return dict(loss=float(loss.detach()), stats=np.array(stats), y=y.numpy(), e=e.numpy(), far=far.numpy(), grad=q.grad.numpy())


def torch_actor(b, weighted, grad_loss):
    import torch

    lp, q = _f(b["log_prob"]).requires_grad_(), _f(b["q"]).requires_grad_()
    q_pi = q[:, 0]
    for c in range(1, q.shape[1]):
        q_pi = torch.minimum(q_pi, q[:, c])
    t = ALPHA * lp - q_pi
    if weighted:
        t = _f(b["weights"]) * t
    loss = t.mean()
    (grad_loss * loss).backward()
    with torch.no_grad():
        stats = [float(loss), float(lp.mean()), float(q_pi.mean()), float((q.max(1).values - q.min(1).values).mean()),
                 float((q.argmin(1) != 0).double().mean()), float(lp.max()), float(q_pi.min()), float(q_pi.max())]
    return dict(loss=float(loss.detach()), stats=np.array(stats), t=t.detach().numpy(), g_lp=lp.grad.numpy(), g_q=q.grad.numpy())


def mean_bar(M, rows_err, terms_abs):
    """|twin mean - torch mean| of M terms: the rows' own differences, the twin's tree, torch's order, the quotients."""
    t = float(np.sum(terms_abs)) * SLOP
    return (float(np.sum(rows_err)) + nt.sum_error_bound(sh.depth(M), t) + (M - 1) * U * t + 2 * U * t) / M * SLOP


def _worst(diff, ref):
    nz = ref != 0.0
    return float(np.max(diff[nz] / (U * np.abs(ref[nz])))) if np.any(nz) else 0.0


def compare_critics(b, M, mode, entropy, per_row, weighted, delta, grad_loss=2.5):
    """One configuration of the critics against torch: asserts every derived bar -> the worst ratios (targets, loss, stats, gradient)."""
    C = b["q"].shape[1]
    kw = kwargs(b, mode, entropy, per_row, weighted, delta)
    value, stats, far, sums = sh.q_loss(b["q"], **kw)
    grad = sh.q_backward(b["q"], np.float32(grad_loss), **kw)
    ref = torch_critics(b, mode, entropy, per_row, weighted, delta, grad_loss)
    p = sh.q_rows(b["q"], **kw)
    assert np.array_equal(p["y"], ref["y"]), "the target is the same float64 operations"
    assert np.array_equal(_u64(p["e"]), _u64(ref["e"]))
    assert tied_rows(p["ae"]) == 0 and np.array_equal(_u64(far), _u64(ref["far"]))
    w_targets = 0.0
    if mode == "bootstrap":
        tkw = {k: v for k, v in kw.items() if k in ("next_log_prob", "alpha", "gamma", "discount")}
        y = sh.targets(b["next_q"], b["reward"], b["term"], **tkw)
        assert np.array_equal(_u64(y), _u64(p["y"]))
        y32 = sh.targets_f32(b["next_q"], b["reward"], b["term"], **tkw)
        assert np.all(np.abs(y32.astype(np.float64) - ref["y"]) <= _ulp32(ref["y"]) / 2)
        w_targets = _worst(np.abs(y - ref["y"]), ref["y"])
    mags = np.abs(p["qd"]).sum(1) / C
    bars = np.array([mean_bar(M, (4 + 2 * C) * U * np.abs(p["term"]), np.abs(p["term"])), mean_bar(M, 2 * C * U * p["am"], p["am"]),
                     mean_bar(M, 2 * C * U * mags, mags), mean_bar(M, 0.0, np.abs(p["y"])), mean_bar(M, 0.0, np.abs(p["gap"])), 0.0, 0.0, 0.0])
    diff = np.abs(stats - ref["stats"])
    assert np.all(diff <= bars), (M, C, mode, entropy, per_row, weighted, delta, diff, bars)
    assert abs(value - ref["loss"]) <= bars[0]
    loss32, stats32, td32 = sh.q_loss_f32(b["q"], **kw)
    assert abs(float(loss32) - ref["loss"]) <= bars[0] + _ulp32(ref["loss"]) / 2
    assert np.all(np.abs(stats32.astype(np.float64) - ref["stats"]) <= bars + _ulp32(ref["stats"]) / 2)
    assert np.all(np.abs(td32.astype(np.float64) - ref["far"]) <= _ulp32(ref["far"]) / 2)
    bar_g = 8 * U * np.abs(ref["grad"]) * SLOP
    gdiff = np.abs(grad - ref["grad"])
    assert np.all(gdiff <= bar_g), (M, C, mode, weighted, delta, float(np.max(gdiff - bar_g)))
    assert np.all(np.abs(sh.to_f32(grad).astype(np.float64) - ref["grad"]) <= bar_g + _ulp32(ref["grad"]) / 2)
    w_loss = abs(value - ref["loss"]) / (U * abs(ref["loss"])) if ref["loss"] else 0.0
    return w_targets, w_loss, _worst(diff[:5], ref["stats"][:5]), _worst(gdiff, ref["grad"])


def compare_actor(b, M, weighted, grad_loss=2.5):
    """One configuration of the actor against torch -> the worst ratios (loss, stats, gradients)."""
    C = b["q"].shape[1]
    kw = dict(alpha=ALPHA, weights=b["weights"] if weighted else None)
    value, stats, sums = sh.pi_loss(b["log_prob"], b["q"], **kw)
    g_lp, g_q = sh.pi_backward(b["log_prob"], b["q"], np.float32(grad_loss), **kw)
    ref = torch_actor(b, weighted, grad_loss)
    p = sh.pi_rows(b["log_prob"], b["q"], **kw)
    assert tied_rows(b["q"]) == 0
    assert np.array_equal(_u64(p["term"]), _u64(ref["t"])), "a row of the actor is the same float64 operations"
    bars = np.array([mean_bar(M, 0.0, np.abs(p["term"])), mean_bar(M, 0.0, np.abs(p["lp"])), mean_bar(M, 0.0, np.abs(p["qp"])),
                     mean_bar(M, 0.0, np.abs(p["gap"])), 0.0, 0.0, 0.0, 0.0])
    diff = np.abs(stats - ref["stats"])
    assert np.all(diff <= bars), (M, C, weighted, diff, bars)
    assert abs(value - ref["loss"]) <= bars[0]
    count = stats[4] * M
    assert count == np.rint(count) == np.count_nonzero(p["jmin"])
    loss32, stats32 = sh.pi_loss_f32(b["log_prob"], b["q"], **kw)
    assert abs(float(loss32) - ref["loss"]) <= bars[0] + _ulp32(ref["loss"]) / 2
    assert np.all(np.abs(stats32.astype(np.float64) - ref["stats"]) <= bars + _ulp32(ref["stats"]) / 2)
    worst = 0.0
    for got, want in ((g_lp, ref["g_lp"]), (g_q, ref["g_q"])):
        bar_g = 8 * U * np.abs(want) * SLOP
        gdiff = np.abs(got - want)
        assert np.all(gdiff <= bar_g), (M, C, weighted, float(np.max(gdiff - bar_g)))
        assert np.all(np.abs(sh.to_f32(got).astype(np.float64) - want) <= bar_g + _ulp32(want) / 2)
        worst = max(worst, _worst(gdiff, want))
    off = np.arange(C)[None, :] != p["jmin"][:, None]
    assert np.all(_u64(g_q[off]) == 0) and np.all(ref["g_q"][off] == 0.0)      # +0.0 outside the column of the minimum
    w_loss = abs(value - ref["loss"]) / (U * abs(ref["loss"])) if ref["loss"] else 0.0
    return w_loss, _worst(diff[:4], ref["stats"][:4]), worst


def _measured(name, worst):
    """The named constant is what was measured on this input (to its two decimals, rounded up), in units of 2^-53 of the reference's
    magnitude; the derived bars are asserted where the difference is taken."""
    bnd = getattr(sh, "B_" + name)
    print(f"measured B_{name}: {worst:.4f}")
    assert worst <= bnd < worst + 0.01, (name, worst, bnd)


# ---- against torch's float64 autograd ---------------------------------------------------------------------------------------------------------
def test_the_twin_is_within_its_derived_bars_of_torch_on_20000_rows():
    worst_q, worst_pi = np.zeros(4), np.zeros(3)
    for C in CRITICS:
        b = make_batch(M_BIG, C, 1 + C)
        assert tied_rows(b["q"]) == 0 and tied_rows(b["next_q"]) == 0 and (b["term"] != 0).sum() > 1500
        p = sh.q_rows(b["q"], targets=b["targets"], delta=1.0)
        assert 0.2 < (p["ae"] > 1.0).mean() < 0.8      # both sides of delta = 1
        for mode, entropy, per_row in MODES:
            for weighted in (True, False):
                for delta in (1.0, math.inf):
                    worst_q = np.maximum(worst_q, compare_critics(b, M_BIG, mode, entropy, per_row, weighted, delta))
        for weighted in (True, False):
            worst_pi = np.maximum(worst_pi, compare_actor(b, M_BIG, weighted))
    for name, w in zip(("TARGETS", "Q_LOSS", "Q_STATS", "GRAD_Q"), worst_q):
        _measured(name, w)
    for name, w in zip(("PI_LOSS", "PI_STATS", "GRAD_PI"), worst_pi):
        _measured(name, w)


@pytest.mark.parametrize("M", (1, 2, 1023, 1025))
def test_small_batches_agree_with_torch(M):
    for C in CRITICS:
        b = make_batch(M, C, 100 + M + C)
        for mode, entropy, per_row in MODES:
            for weighted in (True, False):
                for delta in (1.0, math.inf):
                    compare_critics(b, M, mode, entropy, per_row, weighted, delta)
        for weighted in (True, False):
            compare_actor(b, M, weighted)


def test_every_sum_is_within_the_tree_bound_of_the_exact_sum():
    b = make_batch(M_BIG, 2, 3)
    kw = kwargs(b, "bootstrap", True, True, True, 1.0)
    _, _, _, sums = sh.q_loss(b["q"], **kw)
    p = sh.q_rows(b["q"], **kw)
    assert sh.depth(M_BIG) == 4 + 6 + 2 + 10
    for k, got in sums.items():
        exact, bound = math.fsum(p[k]), nt.sum_error_bound(sh.depth(M_BIG), math.fsum(np.abs(p[k])))
        assert abs(got - exact) <= bound, (k, got, exact, bound)
    _, _, sums = sh.pi_loss(b["log_prob"], b["q"], alpha=ALPHA, weights=b["weights"])
    p = sh.pi_rows(b["log_prob"], b["q"], alpha=ALPHA, weights=b["weights"])
    for k, got in sums.items():
        exact, bound = math.fsum(p[k]), nt.sum_error_bound(sh.depth(M_BIG), math.fsum(np.abs(p[k])))
        assert abs(got - exact) <= bound, (k, got, exact, bound)
    assert sums["later"] == float(np.count_nonzero(p["jmin"]))


# ---- the exact cases of the rule -----------------------------------------------------------------------------------------------------------
def test_ties_take_the_first_minimum_also_between_the_two_zeros():
    q = np.array([[1.0, 1.0, 3.0], [2.0, -1.0, -1.0], [-0.0, 0.0, 5.0], [0.0, -0.0, 5.0], [4.0, 3.0, 2.0]], np.float32)
    m = sh.ends(q)
    assert list(m["jmin"]) == [0, 1, 0, 0, 2]
    assert np.signbit(m["mn"][2]) and not np.signbit(m["mn"][3])      # -0.0 < +0.0 is false: the first zero stays, with its sign
    lp = np.zeros(5, np.float32)
    g_lp, g_q = sh.pi_backward(lp, q, np.float32(1.0), alpha=0.5)
    want = np.zeros((5, 3))
    want[np.arange(5), [0, 1, 0, 0, 2]] = -1.0 / 5.0      # the whole gradient in the first minimum's column (torch.minimum splits it in halves)
    assert np.array_equal(g_q, want) and np.all(_u64(g_q[want == 0.0]) == 0)
    assert np.array_equal(g_lp, np.full(5, 0.5 / 5.0))
    _, stats, _ = sh.pi_loss(lp, q, alpha=0.5)
    assert stats[4] == 2.0 / 5.0
    y = sh.targets(q, np.zeros(5, np.float32), np.zeros(5, np.uint8), gamma=1.0)
    assert np.array_equal(y, [1.0, -1.0, 0.0, 0.0, 2.0])


def test_a_nan_in_a_row_spoils_that_row_alone():
    b = make_batch(7, 3, 5)
    clean = sh.q_rows(b["q"], reward=b["reward"], terminated=np.zeros(7, np.uint8), next_q=b["next_q"], gamma=GAMMA)
    q, nq = b["q"].copy(), b["next_q"].copy()
    q[2, 1] = np.nan
    nq[4, 0] = np.nan
    kw = dict(reward=b["reward"], terminated=np.zeros(7, np.uint8), next_q=nq, gamma=GAMMA)
    p = sh.q_rows(q, **kw)
    assert np.isnan(p["y"][4]) and np.array_equal(np.isnan(p["y"]), np.arange(7) == 4)
    g = sh.q_backward(q, np.float32(1.0), **kw)
    want_nan = np.zeros((7, 3), bool)
    want_nan[2, 1] = True      # a NaN critic: its own column only
    want_nan[4, :] = True      # a NaN target: every column
    assert np.array_equal(np.isnan(g), want_nan)
    rest = ~np.isin(np.arange(7), (2, 4))
    assert np.array_equal(p["h"][rest], clean["h"][rest]) and np.isnan(p["h"][2]) and np.isnan(p["far"][2]) and np.isnan(p["gap"][2])
    _, stats, far, _ = sh.q_loss(q, **kw)
    assert np.isnan(stats[:5]).all()
    finite = np.delete(q.reshape(-1), 2 * 3 + 1)
    assert stats[6] == finite.min() and stats[7] == finite.max() and stats[5] == np.nanmax(p["ae"])      # the extrema skip the NaN
    lp = b["log_prob"][:7]
    g_lp, g_q = sh.pi_backward(lp, q, np.float32(1.0), alpha=ALPHA)
    assert np.array_equal(np.isnan(g_q), np.repeat((np.arange(7) == 2)[:, None], 3, 1)) and not np.isnan(g_lp).any()
    _, stats, _ = sh.pi_loss(lp, q, alpha=ALPHA)
    qp = np.delete(q.min(1), 2)
    assert np.isnan(stats[[0, 2, 3]]).all() and not np.isnan(stats[[1, 4, 5]]).any() and stats[6] == qp.min() and stats[7] == qp.max()


def test_a_terminated_row_ignores_every_input_of_the_bootstrap():
    b = make_batch(6, 2, 9)
    term = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    nq, lp, disc = b["next_q"].copy(), b["next_lp"].copy(), b["discount"].copy()
    base = sh.targets(nq, b["reward"], term, next_log_prob=lp, alpha=ALPHA, discount=disc)
    nq[0] = np.nan
    nq[2, 1] = np.inf
    lp[3] = np.nan
    lp[0] = -np.inf
    disc[5] = np.nan
    disc[2] = np.inf
    y = sh.targets(nq, b["reward"], term, next_log_prob=lp, alpha=ALPHA, discount=disc)
    assert np.array_equal(_u64(y), _u64(base)) and np.array_equal(y[term != 0], b["reward"][term != 0].astype(np.float64))
    p = sh.q_rows(b["q"], reward=b["reward"], terminated=term, next_q=nq, next_log_prob=lp, alpha=ALPHA, discount=disc)
    assert np.array_equal(_u64(p["y"]), _u64(base)) and not np.isnan(p["h"]).any()


def test_td_error_is_the_first_of_equal_errors_and_delta_is_on_the_quadratic_side():
    q = np.array([[3.0, -1.0], [-1.0, 3.0], [0.5, 4.0], [1.0, 1.0]], np.float32)
    y = np.array([1.0, 1.0, 2.0, 0.0], np.float32)
    p = sh.q_rows(q, targets=y, delta=2.0)
    assert np.array_equal(p["far"], [2.0, -2.0, 2.0, 1.0])      # rows 0, 1: |e| = 2 twice, the first column's sign; row 3: two equal errors
    # ae == delta: quadratic, H = 0.5 * 4 = 2 = delta * (2 - 1), dH = e
    assert np.array_equal(p["H"][0], [2.0, 2.0]) and np.array_equal(p["dH"][0], [2.0, -2.0]) and np.array_equal(p["dH"][2], [-1.5, 2.0])
    p3 = sh.q_rows(q, targets=y, delta=np.nextafter(2.0, 0.0))
    assert np.array_equal(p3["dH"][0], [np.nextafter(2.0, 0.0), -np.nextafter(2.0, 0.0)])      # just below: the linear side
    inf = sh.q_rows(q, targets=y, delta=math.inf)
    assert np.array_equal(inf["H"], 0.5 * (inf["e"] * inf["e"])) and np.array_equal(inf["dH"], inf["e"])
    _, stats, far, _ = sh.q_loss(q, targets=y, delta=2.0)
    assert stats[0] == (4.0 + 4.0 + (0.5 * 2.25 + 2.0) + 1.0) / 4.0 and stats[5] == 2.0 and stats[6] == -1.0 and stats[7] == 4.0
    assert stats[4] == (4.0 + 4.0 + 3.5 + 0.0) / 4.0 and stats[1] == (2.0 + 2.0 + 1.75 + 1.0) / 4.0


# ---- the front end without a device ----------------------------------------------------------------------------------------------------------
def test_the_module_matches_the_twin_and_does_not_import_torch():
    import subprocess

    from conftest import ROOT

    p = subprocess.run([sys.executable, "-c", "import sys; import gym_amd.sac as s; import gym_amd; gym_amd.soft_q_targets; gym_amd.twin_q_loss; "
                        "gym_amd.soft_policy_loss; assert 'torch' not in sys.modules; print(s.workspace_bytes(4099))"], cwd=ROOT, capture_output=True,
                       text=True)
    assert p.returncode == 0 and p.stdout.strip() == str(5 * 8 * 8), p.stderr[-1500:]
    from gym_amd import dqn, sac

    assert sac.Q_STAT_NAMES == sh.Q_STAT_NAMES and sac.PI_STAT_NAMES == sh.PI_STAT_NAMES and sac.STATS == 8 == len(sac.Q_STAT_NAMES)
    assert [sac.Q_STAT_NAMES.index(n) for n in ("loss_term", "td_abs_mean", "q_mean", "target_mean", "critic_gap_mean", "td_abs_max", "q_min", "q_max")] == \
        [sac.Q_LOSS_TERM, sac.Q_TD_ABS_MEAN, sac.Q_MEAN, sac.Q_TARGET_MEAN, sac.Q_CRITIC_GAP_MEAN, sac.Q_TD_ABS_MAX, sac.Q_MIN, sac.Q_MAX]
    assert sac.PI_STAT_NAMES[sac.PI_LOG_PROB_MEAN] == "log_prob_mean" and sac.PI_STAT_NAMES[sac.PI_LATER_CRITIC_FRACTION] == "later_critic_fraction"
    for M in (1, 1024, 1025, 1 << 20, (1 << 20) + 1, 1 << 30):
        assert sac.launches(M) == sh.launches(M) == dqn.launches(M) and sac.workspace_bytes(M) == dqn.workspace_bytes(M)
    assert sac.launches(1 << 20) == 2 and sac.launches((1 << 20) + 5) == 3
    for bad in (0, -1, (1 << 40) + 1):
        with pytest.raises(ValueError, match="rows must be in"):
            sac.workspace_bytes(bad)
