"""tests/dqn_host.py — the NumPy twin of include/mxv_dqn.h, which the device is compared with bit for bit — held to torch's float64 autograd
of the literal gather / argmax / huber_loss / mean expression, to exact sums and to the exact cases of the rule; Peng's Q(lambda) target as
the `returns` of the GAE twin; and what needs no device of the front end.

How the bars are derived (u = 2^-53; nothing here is tuned to what the twin gives):
  * a row: q[i, a_i], the target y (r + gamma * nv: the factor (1 - terminated) of the literal expression is exactly 1 or 0), the error
    e and |e| are the same float64 operations on both sides.  The Huber value is two or three more operations whose order torch does
    not document, and the weight one more: 4 u |term| per row.
  * a mean of M terms: the rows' own differences, EB(sum |term|) = norm_tree_host.sum_error_bound(ppo_host.depth(M), sum |term|) for
    the twin's tree, (M - 1) u sum |term| for whatever order torch sums in, one rounding for each quotient.
  * the gradient g / M * w * dh: three roundings here, a handful in torch's chain: 8 u |gradient|.
  * a float32 output: half a float32 ulp of the reference on top of its float64 bar.
  * the extrema and the fraction in the linear zone are selections and counts of identical float64 values: exact.
The only discontinuity is the argmax: rows whose two largest selector values are equal or adjacent floats are counted, and the inputs
have none."""
import math
import subprocess
import sys

import numpy as np
import pytest

import dqn_host as dq
import gae_host
import norm_tree_host as nt
import ppo_host as pp
from conftest import ROOT

U = 2.0 ** -53
M_BIG, A_BIG = 20_000, 6
GAMMA = 0.99
SLOP = 1.0 + 1e-6          # the second-order terms the first-order bounds above leave out
MODES = (("targets", False), ("bootstrap", False), ("bootstrap", True))


def _u64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64) * (1 + 1e-6)).astype(np.float32)).astype(np.float64)


def make_batch(M, A, seed):
    """M rows of A action values: TD errors on both sides of delta = 1, a tenth of the rows terminated, and — cycling through the
    rows — an error of exactly zero and errors far in the linear zone of both signs."""
    rng = np.random.default_rng(seed)
    q = (rng.standard_normal((M, A)) * 2.0).astype(np.float32)
    act = rng.integers(0, A, M)
    next_q = (rng.standard_normal((M, A)) * 2.0).astype(np.float32)
    online = (next_q + 0.7 * rng.standard_normal((M, A))).astype(np.float32)
    reward = rng.standard_normal(M).astype(np.float32)
    term = (rng.uniform(size=M) < 0.1).astype(np.uint8)
    qa = q[np.arange(M), act]
    targets = (qa + 1.2 * rng.standard_normal(M)).astype(np.float32)
    k = np.arange(M)
    targets[k % 10 == 0] = qa[k % 10 == 0]
    targets[k % 10 == 1] = (qa[k % 10 == 1] + 5.0).astype(np.float32)
    targets[k % 10 == 2] = (qa[k % 10 == 2] - 5.0).astype(np.float32)
    weights = rng.uniform(0.2, 2.0, M).astype(np.float32)
    return dict(q=q, act=act, next_q=next_q, online=online, reward=reward, term=term, targets=targets, weights=weights)


def kwargs(b, mode, double, weighted, delta):
    kw = dict(delta=delta, weights=b["weights"] if weighted else None)
    if mode == "targets":
        kw["targets"] = b["targets"]
    else:
        kw.update(reward=b["reward"], terminated=b["term"], next_q=b["next_q"], next_q_online=b["online"] if double else None, gamma=GAMMA)
    return kw


def near_ties(sel):
    """Rows whose two largest values are equal or adjacent floats: where an argmax may legitimately differ."""
    s = np.sort(np.asarray(sel, np.float32), axis=1)
    if s.shape[1] < 2:
        return 0
    return int(np.count_nonzero(np.nextafter(s[:, -2], np.float32(np.inf)) >= s[:, -1]))


def torch_reference(b, mode, double, weighted, delta, grad_loss=1.0):
    """The literal torch sequence in float64 on the CPU, and its autograd."""
    import torch
    import torch.nn.functional as F

    f = lambda x: torch.from_numpy(np.asarray(x, np.float32).astype(np.float64))
    q = f(b["q"]).requires_grad_()
    a = torch.from_numpy(np.asarray(b["act"], np.int64))
    if mode == "targets":
        y = f(b["targets"])
    else:
        next_q = f(b["next_q"])
        sel = f(b["online"]) if double else next_q
        nv = next_q.gather(1, sel.argmax(1, keepdim=True)).squeeze(1)
        y = f(b["reward"]) + (1 - torch.from_numpy(b["term"].astype(np.float64))) * GAMMA * nv
    qa = q.gather(1, a[:, None]).squeeze(1)
    h = F.huber_loss(qa, y, reduction="none", delta=delta)
    if weighted:
        h = h * f(b["weights"])
    loss = h.mean()
    (grad_loss * loss).backward()
    with torch.no_grad():
        e = qa - y
        stats = [float(loss), float(e.abs().mean()), float(qa.mean()), float(y.mean()), float((e.abs() > delta).double().mean()),
                 float(e.abs().max()), float(qa.min()), float(qa.max())]
    return dict(loss=float(loss.detach()), stats=np.array(stats), e=e.detach().numpy(), h=h.detach().numpy(), grad=q.grad.numpy())


def mean_bar(M, rows_err, terms_abs):
    """|twin mean - torch mean| of M terms: the rows' own differences, the twin's tree, torch's order, the quotients."""
    t = float(np.sum(terms_abs)) * SLOP
    return (float(np.sum(rows_err)) + nt.sum_error_bound(dq.depth(M), t) + (M - 1) * U * t + 2 * U * t) / M * SLOP


def compare(b, M, mode, double, weighted, delta, grad_loss=2.5):
    """One configuration against torch: asserts every derived bar -> the worst ratios (loss, stats, gradient) in units of u."""
    if mode == "bootstrap":
        assert near_ties(b["online"] if double else b["next_q"]) == 0
    kw = kwargs(b, mode, double, weighted, delta)
    value, stats, e, sums = dq.loss(b["q"], b["act"], **kw)
    grad = dq.backward(b["q"], b["act"], np.float32(grad_loss), **kw)
    ref = torch_reference(b, mode, double, weighted, delta, grad_loss)
    p = dq.rows(b["q"], b["act"], **kw)
    assert np.array_equal(_u64(e), _u64(ref["e"])), "the TD errors are the same float64 operations"
    bars = np.array([mean_bar(M, 4 * U * np.abs(p["term"]), np.abs(p["term"])), mean_bar(M, 0.0, p["ae"]), mean_bar(M, 0.0, np.abs(p["qa"])),
                     mean_bar(M, 0.0, np.abs(p["y"])), 0.0, 0.0, 0.0, 0.0])
    diff = np.abs(stats - ref["stats"])
    assert np.all(diff <= bars), (M, mode, double, weighted, delta, diff, bars)
    assert abs(value - ref["loss"]) <= bars[0]
    count = stats[4] * M
    assert count == np.rint(count) == np.count_nonzero(p["lin"])
    loss32, stats32, td32 = dq.loss_f32(b["q"], b["act"], **kw)
    assert abs(float(loss32) - ref["loss"]) <= bars[0] + _ulp32(ref["loss"]) / 2
    assert np.all(np.abs(stats32.astype(np.float64) - ref["stats"]) <= bars + _ulp32(ref["stats"]) / 2)
    assert np.all(np.abs(td32.astype(np.float64) - ref["e"]) <= _ulp32(ref["e"]) / 2)
    bar_g = 8 * U * np.abs(ref["grad"]) * SLOP
    gdiff = np.abs(grad - ref["grad"])
    assert np.all(gdiff <= bar_g), (M, mode, double, weighted, delta, float(np.max(gdiff - bar_g)))
    assert np.all(np.abs(dq.to_f32(grad).astype(np.float64) - ref["grad"]) <= bar_g + _ulp32(ref["grad"]) / 2)
    off = np.ones_like(grad, bool)
    off[np.arange(M), b["act"]] = False
    assert np.all(_u64(grad[off]) == 0) and np.all(ref["grad"][off] == 0.0)      # +0.0 outside the taken column
    nz = ref["grad"] != 0.0
    w_loss = abs(value - ref["loss"]) / (U * abs(ref["loss"])) if ref["loss"] else 0.0
    nzs = ref["stats"][:4] != 0.0
    w_stats = float(np.max(diff[:4][nzs] / (U * np.abs(ref["stats"][:4][nzs])))) if nzs.any() else 0.0
    w_grad = float(np.max(gdiff[nz] / (U * np.abs(ref["grad"][nz])))) if nz.any() else 0.0
    return w_loss, w_stats, w_grad


def _measured(name, worst):
    """The named constant is what was measured on this input (to its two decimals, rounded up), in units of 2^-53 of the reference's
    magnitude; the derived bars are asserted where the difference is taken."""
    bnd = getattr(dq, "B_" + name)
    print(f"measured B_{name}: {worst:.4f}")
    assert worst <= bnd < worst + 0.01, (name, worst, bnd)


# ---- against torch's float64 autograd ---------------------------------------------------------------------------------------------------------
def test_the_twin_is_within_its_derived_bars_of_torch_on_20000_rows():
    b = make_batch(M_BIG, A_BIG, 1)
    assert near_ties(b["next_q"]) == 0 and near_ties(b["online"]) == 0
    p = dq.rows(b["q"], b["act"], targets=b["targets"])
    assert (p["e"] == 0.0).sum() >= M_BIG // 10 and 0.3 < p["lin"].mean() < 0.6 and (b["term"] != 0).sum() > 1500
    worst = np.zeros(3)
    for mode, double in MODES:
        for weighted in (True, False):
            for delta in (1.0, math.inf):
                worst = np.maximum(worst, compare(b, M_BIG, mode, double, weighted, delta))
    _measured("LOSS", worst[0])
    _measured("STATS", worst[1])
    _measured("GRAD_Q", worst[2])


@pytest.mark.parametrize("M", (1, 2, 1023, 1025))
def test_small_batches_agree_with_torch(M):
    for A in (1, 3, 6):
        b = make_batch(M, A, 100 + M + A)
        for mode, double in MODES:
            for weighted in (True, False):
                for delta in (1.0, math.inf):
                    compare(b, M, mode, double, weighted, delta)


def test_every_sum_is_within_the_tree_bound_of_the_exact_sum():
    b = make_batch(M_BIG, A_BIG, 1)
    kw = kwargs(b, "bootstrap", True, True, 1.0)
    _, _, _, sums = dq.loss(b["q"], b["act"], **kw)
    p = dq.rows(b["q"], b["act"], **kw)
    assert dq.depth(M_BIG) == 4 + 6 + 2 + 10
    for k, got in sums.items():
        exact, bound = math.fsum(p[k]), nt.sum_error_bound(dq.depth(M_BIG), math.fsum(np.abs(p[k])))
        assert abs(got - exact) <= bound, (k, got, exact, bound)
    assert sums["lin"] == float(np.count_nonzero(p["lin"]))


# ---- Peng's Q(lambda) is the GAE twin's `returns` with values = max_a Q ----------------------------------------------------------------------------
def test_q_lambda_targets_are_the_returns_of_gae_with_values_max_q():
    """G_t = r_t + gamma [(1 - lam) max_a Q(s_t+1, a) + lam G_t+1], cut at an episode end (terminated: G = r; truncated: G = r + gamma
    final value), as a literal float64 loop, against gae_host.gae(..., values=max_a Q)[1].  Both sides are float64 recursions of the same
    inputs that differ by a few u per step (negligible: 64 K u of the largest magnitude is allowed for it), and each result is rounded to
    float32 once: two half ulps of float32."""
    K, N, gamma, lam = 32, 257, 0.99, 0.65
    rng = np.random.default_rng(7)
    reward = rng.standard_normal((K, N)).astype(np.float32)
    term = (rng.uniform(size=(K, N)) < 0.05).astype(np.uint8)
    trunc = (rng.uniform(size=(K, N)) < 0.05).astype(np.uint8)
    qmax = (rng.standard_normal((K, N)) * 2 + 1).astype(np.float32)                # max_a Q of the observation each action was taken from
    last = (rng.standard_normal(N) * 2 + 1).astype(np.float32)
    final = (rng.standard_normal((K, N)) * 2 + 1).astype(np.float32)
    ret = gae_host.gae(reward, term, trunc, qmax, last, gamma=gamma, lam=lam, final_values=final)[1]
    G = np.zeros((K, N))
    nxt_q, nxt_G = last.astype(np.float64), last.astype(np.float64)
    for t in range(K - 1, -1, -1):
        r = reward[t].astype(np.float64)
        inner = r + gamma * ((1 - lam) * nxt_q + lam * nxt_G)
        cut = np.where(term[t] != 0, r, r + gamma * final[t].astype(np.float64))
        G[t] = np.where((term[t] | trunc[t]) != 0, cut, inner)
        nxt_q, nxt_G = qmax[t].astype(np.float64), G[t]
    scale = max(float(np.abs(G).max()), float(np.abs(qmax).max()))
    bar = _ulp32(G) + 64 * K * U * scale
    diff = np.abs(ret.astype(np.float64) - pp.to_f32(G).astype(np.float64))
    print("Q(lambda) max difference:", diff.max(), "values up to", scale)
    assert np.all(diff <= bar) and scale > 4.0 and (term & ~trunc).sum() > 100 and (trunc & ~term).sum() > 100


# ---- exact cases ----------------------------------------------------------------------------------------------------------------------------
def test_the_edge_of_the_linear_zone_is_quadratic():
    q = np.array([[0.0, 3.0], [0.0, 3.0], [0.0, 3.0]], np.float32)
    p = dq.rows(q, [1, 1, 1], targets=np.array([2.0, 4.0, 1.0], np.float32), delta=1.0)      # e = 1, -1, 2
    assert np.array_equal(p["h"], [0.5, 0.5, 1.5]) and np.array_equal(p["dh"], [1.0, -1.0, 1.0]) and np.array_equal(p["lin"], [0.0, 0.0, 1.0])
    g = dq.backward(q, [1, 1, 1], np.float32(3.0), targets=np.array([2.0, 4.0, 1.0], np.float32), delta=1.0)
    assert np.array_equal(g, [[0.0, 1.0], [0.0, -1.0], [0.0, 1.0]])
    p = dq.rows(q, [1, 1, 1], targets=np.array([2.0, 4.0, -97.0], np.float32), delta=math.inf)
    assert np.array_equal(p["h"], [0.5, 0.5, 5000.0]) and np.array_equal(p["dh"], [1.0, -1.0, 100.0]) and not p["lin"].any()


def test_a_terminated_row_ignores_next_q_entirely():
    b = make_batch(40, 3, 2)
    b["term"][:] = 0
    b["term"][[5, 6, 7]] = 1
    clean = dq.loss(b["q"], b["act"], **kwargs(b, "bootstrap", True, True, 1.0))
    b["next_q"][5], b["online"][6], b["next_q"][7, 1] = np.nan, np.inf, -np.inf
    b["online"][7] = np.nan
    got = dq.loss(b["q"], b["act"], **kwargs(b, "bootstrap", True, True, 1.0))
    assert np.isfinite(got[1]).all() and np.array_equal(_u64(got[1]), _u64(clean[1])) and np.array_equal(_u64(got[2]), _u64(clean[2]))


def test_a_nan_in_the_selector_row_makes_that_row_nan_and_nothing_else():
    b = make_batch(300, 4, 3)
    b["term"][:] = 0
    for double in (False, True):
        c = {k: v.copy() for k, v in b.items()}
        (c["online"] if double else c["next_q"])[17, 2] = np.nan
        kw = kwargs(c, "bootstrap", double, False, 1.0)
        value, stats, e, _ = dq.loss(c["q"], c["act"], **kw)
        g = dq.backward(c["q"], c["act"], np.float32(1.0), **kw)
        others = np.arange(300) != 17
        assert np.isnan(value) and np.isnan(e[17]) and np.isfinite(e[others]).all() and np.isfinite(stats[5:]).all()
        assert np.isnan(stats[[0, 1, 3]]).all() and np.isfinite(stats[2]) and np.isfinite(stats[4])
        assert np.isnan(g[17, c["act"][17]]) and np.count_nonzero(np.isnan(g)) == 1
        assert dq.bits(dq.to_f32(g))[17, c["act"][17]] == 0x7FC00000 and dq.bits(dq.loss_f32(c["q"], c["act"], **kw)[0]) == 0x7FC00000
        clean = dq.backward(b["q"], b["act"], np.float32(1.0), **kwargs(b, "bootstrap", double, False, 1.0))
        assert np.array_equal(_u64(g[others]), _u64(clean[others]))
        # the extrema skip the NaN row
        pr = dq.rows(c["q"], c["act"], **kw)
        assert stats[5] == pr["ae"][others].max() and stats[6] == pr["qa"].min() and stats[7] == pr["qa"].max()


def test_ties_take_the_first_index_also_between_the_two_zeros():
    sel = np.array([[1.0, 2.0, 2.0, 0.0], [-0.0, 0.0, -1.0, 0.0], [0.0, -0.0, -1.0, -1.0], [-np.inf] * 4, [3.0, np.inf, np.inf, 1.0]], np.float32)
    j, bad = dq.first_max(sel)
    assert np.array_equal(j, [1, 0, 0, 0, 1]) and not bad.any()
    next_q = np.arange(20, dtype=np.float32).reshape(5, 4)
    p = dq.rows(np.zeros((5, 4), np.float32), [0] * 5, reward=np.zeros(5, np.float32), terminated=np.zeros(5, np.uint8), next_q=next_q,
                next_q_online=sel, gamma=1.0)
    assert np.array_equal(p["y"], [1.0, 4.0, 8.0, 12.0, 17.0])
    # next_q selecting itself: the sign of the first of two zeros reaches the target
    p = dq.rows(np.zeros((2, 2), np.float32), [0, 0], reward=np.array([-0.0, -0.0], np.float32), terminated=np.zeros(2, np.uint8),
                next_q=np.array([[-0.0, 0.0], [0.0, -0.0]], np.float32), gamma=1.0)
    assert np.array_equal(np.signbit(p["y"]), [True, False])


def test_an_action_out_of_range_gives_a_nan_loss_and_a_fully_nan_gradient_row():
    b = make_batch(50, 3, 4)
    for bad in (3, -1, 1 << 40, -(1 << 62)):
        act = b["act"].astype(np.int64)
        act[11] = bad
        value, stats, e, _ = dq.loss(b["q"], act, targets=b["targets"])
        g = dq.backward(b["q"], act, np.float32(1.0), targets=b["targets"])
        assert np.isnan(value) and np.isnan(e[11]) and np.isnan(g[11]).all() and np.count_nonzero(np.isnan(g)) == 3
        assert np.isnan(stats[2]) and np.isfinite(stats[5:]).all() and np.all(dq.bits(dq.to_f32(g))[11] == 0x7FC00000)


def test_no_row_has_a_value_and_zero_extrema_are_positive_zero():
    q = np.zeros((3, 2), np.float32)
    _, stats, _, _ = dq.loss(q, [5, 5, 5], targets=np.zeros(3, np.float32))
    assert stats[5] == -np.inf and stats[6] == np.inf and stats[7] == -np.inf
    q[:] = -0.0
    _, stats, _, _ = dq.loss(q, [0, 1, 0], targets=np.full(3, -0.0, np.float32))
    assert np.array_equal(_u64(stats[5:]), [0, 0, 0])


def test_where_a_permutation_of_the_rows_keeps_the_bits():
    """The rows of lane t of a leaf exchanged with the rows of lane t ^ 1 (all four of them): the first butterfly stage adds the two lanes'
    totals, and an addition commutes."""
    M = 3000
    b = make_batch(M, 4, 11)
    kw = lambda c: kwargs(c, "bootstrap", True, True, 1.0)
    base = dq.loss(b["q"], b["act"], **kw(b))
    order = np.arange(M)
    leaf, t = 1024, 37
    for j in range(4):
        x, y = leaf + t + 256 * j, leaf + (t ^ 1) + 256 * j
        order[x], order[y] = y, x
    c = {k: v[order] for k, v in b.items()}
    got = dq.loss(c["q"], c["act"], **kw(c))
    assert not np.array_equal(b["q"], c["q"]) and np.array_equal(_u64(got[1]), _u64(base[1])) and np.array_equal(_u64(got[0]), _u64(base[0]))
    # (that other exchanges do move the bits of this tree is shown on wider-ranging terms in tests/test_ppo_host.py)


# ---- the Python front end ---------------------------------------------------------------------------------------------------------------------
def test_the_front_end_validates_without_a_device():
    code = ("import sys; import gym_amd.dqn as d; assert 'torch' not in sys.modules; import gym_amd; "
            "assert gym_amd.dqn_loss is d.dqn_loss; assert 'torch' not in sys.modules; "
            "assert d.STAT_NAMES[d.Q_TAKEN_MAX] == 'q_taken_max' and d.STAT_NAMES[d.LINEAR_FRACTION] == 'linear_fraction' and d.LOSS_TERM == 0; "
            "assert d.workspace_bytes(1) == 64 and d.workspace_bytes(1 << 20) == 65536 and d.workspace_bytes((1 << 20) + 5) == 64 * 1027; "
            "assert [d.launches(m) for m in (1, 1024, 1 << 20, (1 << 20) + 5, 1 << 30, (1 << 30) + 1)] == [2, 2, 2, 3, 3, 4]")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
    import torch

    from gym_amd import dqn

    assert dqn.STAT_NAMES == dq.STAT_NAMES and dqn.STATS == len(dq.STAT_NAMES) and dqn.LEAF_ROWS == pp.LEAF_ROWS
    assert [dqn.launches(m) for m in (1, 3, 1025, 1024 * 1024 + 5)] == [dq.launches(m) for m in (1, 3, 1025, 1024 * 1024 + 5)]
    q, a, v = torch.zeros((4, 3)), torch.zeros(4, dtype=torch.int64), torch.zeros(4)
    term = torch.zeros(4, dtype=torch.bool)
    boot = dict(reward=v, terminated=term, next_q=q)
    for kw, what in ((dict(), "exactly one target mode"), (dict(targets=v, reward=v), "exactly one target mode"),
                     (dict(targets=v, next_q=q), "exactly one target mode"), (dict(targets=v, next_q_online=q), "next_q_online"),
                     (dict(reward=v, next_q=q), "terminated missing"), (dict(reward=v, terminated=term), "next_q missing"),
                     (dict(targets=v, q=q.double()), "float32"), (dict(targets=v, q=[0.0]), "torch tensor"), (dict(targets=v, q=torch.zeros((4, 65))), "shape"),
                     (dict(targets=v, q=torch.zeros(4)), "shape"), (dict(targets=v, actions=a.float()), "int64"), (dict(targets=v, actions=torch.zeros(3, dtype=torch.int64)), "shape"),
                     (dict(targets=torch.zeros(5)), "shape"), (dict(targets=v.double()), "float32"), (dict(boot, reward=v.double()), "float32"),
                     (dict(boot, terminated=v), "uint8"), (dict(boot, next_q=torch.zeros((4, 2))), "shape"), (dict(boot, next_q_online=torch.zeros((5, 3))), "shape"),
                     (dict(boot, gamma=float("inf")), "finite"), (dict(boot, gamma="0.9"), "finite"), (dict(targets=v, delta=0.0), "delta"),
                     (dict(targets=v, delta=-1.0), "delta"), (dict(targets=v, delta=float("nan")), "finite"), (dict(targets=v, delta=True), "finite"),
                     (dict(targets=v, weights=torch.zeros(3)), "shape"), (dict(targets=v, td_error=torch.zeros(4, dtype=torch.float64)), "float32"),
                     (dict(targets=v.clone().requires_grad_()), "must not require grad"), (dict(boot, next_q=q.clone().requires_grad_()), "must not require grad"),
                     (dict(targets=v, weights=v.clone().requires_grad_()), "must not require grad"),
                     (dict(targets=v, q=q.clone().requires_grad_(), out=(torch.zeros(()), torch.zeros(8))), "requires grad"),
                     (dict(targets=v, q=q.clone().requires_grad_(), workspace=torch.zeros(8, dtype=torch.float64)), "requires grad"),
                     (dict(targets=v, out=(torch.zeros(()),)), "2 entries"), (dict(targets=v, out=(torch.zeros(()), torch.zeros(7))), "shape"),
                     (dict(targets=v), "device tensor"), (dict(boot), "device tensor")):
        args = dict(q=q, actions=a)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            dqn.dqn_loss(args.pop("q"), args.pop("actions"), **args)
    with pytest.raises(ValueError, match="rows"):
        dqn.workspace_bytes(0)
    assert dqn._delta(math.inf) == math.inf and dqn._delta(np.float32(np.inf)) == math.inf and dqn._delta(2) == 2.0
