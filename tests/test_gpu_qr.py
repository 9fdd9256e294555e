"""gym_amd.quantile_dqn_loss and quantile_q_values on the device against tests/qr_host.py, bit for bit — the loss, the eight diagnostics,
row_loss, targets_out and the dense gradient: every size at which the tree changes shape (a partial tile, a partial leaf, two leaves,
the extra launch) times every kind of head (one quantile, the quantile counts below, at and beside a wave, the action limit), every
target mode, double on and off, weights on and off, the scalar gamma and the per-row discount; the sizes at which the grids stride;
strided rows, leading dims, both action widths and both flag dtypes; the exact cases of the rule; the expected values and their argmax;
a real Linear head; the allocation-free forward recorded in a graph; the launch counts and the absence of a synchronisation; a full
n-step prioritised-replay loop; the example run twice; the front end's refusals."""
import os
import sys

import numpy as np
import pytest

import dqn_host as dh
import nstep_host as nh
import prio_host as ph
import qr_host as qh
from conftest import ROOT
from qr_host import bits, to_f32
from test_gpu_ppo import _captured_launches, _hip
from test_qr_host import GAMMA, MODES, kwargs, make_batch

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099)
HEADS = ((1, 1), (2, 51), (3, 51), (6, 32), (4, 64), (2, 63), (7, 33), (64, 2))
GRAD = 2.5
CHUNK = 1 << 16      # rows of the twin at a time, at the sizes where its [M, 64] float64 arrays would not fit


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host_bits(torch, x):
    return x.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1)


def _same32(torch, got, want64, what):
    assert got.dtype == torch.float32, what
    want = bits(to_f32(np.asarray(want64, np.float64).reshape(-1)))
    have = host_bits(torch, got)
    bad = np.flatnonzero(have != want) if have.shape == want.shape else None
    assert have.shape == want.shape and bad.size == 0, (what, bad[:8], have[bad[:8]], want[bad[:8]])


def device_kwargs(torch, b, mode, double, factor, weighted, view=lambda x: x, rows=lambda x: x, **over):
    kw = dict(weights=view(dev(torch, b["weights"])) if weighted else None)
    if mode == "given":
        kw["target_quantiles"] = view(dev(torch, b["target_quantiles"]))
    else:
        kw.update(reward=view(dev(torch, b["reward"])), terminated=view(dev(torch, b["term"])), next_quantiles=rows(dev(torch, b["next"])),
                  next_quantiles_online=rows(dev(torch, b["online"])) if double else None)
        kw.update(dict(gamma=GAMMA) if factor == "gamma" else dict(discount=view(dev(torch, b["discount"]))))
    kw.update(over)
    return kw


def twin(b, mode, double, factor, weighted, **over):
    """The twin's forward and backward on the batch, a chunk of rows at a time -> (loss, stats, ql [M], T [M, N], grad [M, A, N])."""
    M, A, N = b["quantiles"].shape
    cols = {k: [] for k in ("term", "qa", "y", "ae", "cr", "ql")}
    Ts, grads = [], []
    for r0 in range(0, M, CHUNK):
        c = {k: v[r0:r0 + CHUNK] for k, v in b.items()}
        kw = kwargs(c, mode, double, factor, weighted, **over)
        p = qh.rows(c["quantiles"], c["act"], **kw)
        for k in cols:
            cols[k].append(p[k])
        Ts.append(p["T"][:, :N])
        grads.append(to_f32(qh.grad_of(p, np.float32(GRAD), batch_rows=M)))
    p = {k: np.concatenate(v) for k, v in cols.items()}
    value, stats, _ = qh.finish(p)
    return value, stats, p["ql"], np.concatenate(Ts), np.concatenate(grads)


def check(torch, b, mode, double, factor, weighted, *, view=lambda x: x, rows=lambda x: x, act=None, out_path=True, what=None, **over):
    """One forward and one backward of the device on the batch `b` against the twin: everything bit for bit.  -> (stats, grad,
    targets_out) on the host."""
    import gym_amd

    M, A, N = b["quantiles"].shape
    what = (what, M, A, N, mode, double, factor, weighted)
    want_loss, want_stats, want_ql, want_T, want_g = twin(b, mode, double, factor, weighted, **over)
    over_d = {k: v for k, v in over.items() if k != "gamma" or factor == "gamma"}
    kw_d = device_kwargs(torch, b, mode, double, factor, weighted, view, rows, **over_d)
    quantiles = rows(dev(torch, b["quantiles"])).requires_grad_()
    actions = view(dev(torch, b["act"]) if act is None else act)
    row_loss = torch.full(tuple(actions.shape), 7.0, device="cuda:0")
    targets_out = torch.full(tuple(actions.shape) + (N,), 7.0, device="cuda:0")
    loss, stats = gym_amd.quantile_dqn_loss(quantiles, actions, row_loss=row_loss, targets_out=targets_out, **kw_d)
    assert loss.dim() == 0 and loss.requires_grad and tuple(stats.shape) == (8,) and not stats.requires_grad
    _same32(torch, loss, [want_loss], (what, "loss"))
    _same32(torch, stats, want_stats, (what, "stats"))
    _same32(torch, row_loss, want_ql, (what, "row_loss"))
    _same32(torch, targets_out, want_T, (what, "targets_out"))
    assert host_bits(torch, stats)[0] == host_bits(torch, loss)[0]
    (GRAD * loss).backward()
    assert tuple(quantiles.grad.shape) == tuple(quantiles.shape) and quantiles.grad.is_contiguous(), what
    have = host_bits(torch, quantiles.grad)
    assert np.array_equal(have, bits(want_g).reshape(-1)), (what, "grad_quantiles", np.flatnonzero(have != bits(want_g).reshape(-1))[:8])
    if out_path:      # the same forward without autograd, into the caller's tensors
        out = (torch.empty((), device="cuda:0"), torch.empty(8, device="cuda:0"))
        with torch.no_grad():
            got = gym_amd.quantile_dqn_loss(quantiles, actions, out=out, **kw_d)
        assert got[0] is out[0] and got[1] is out[1]
        _same32(torch, out[0], [want_loss], (what, "out loss"))
        _same32(torch, out[1], want_stats, (what, "out stats"))
    return stats.cpu().numpy(), quantiles.grad.cpu().numpy().reshape(M, A, N), targets_out.cpu().numpy().reshape(M, N)


# ---- every size, every kind of head, every mode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,N", HEADS)
@pytest.mark.parametrize("M", SIZES)
def test_loss_stats_row_loss_targets_and_gradient_match_the_twin(torch, M, A, N):
    b = make_batch(M, A, N, 3000 + M % 1000 + A + N)
    for mode, double, factor in MODES:
        for weighted in (True, False):
            check(torch, b, mode, double, factor, weighted, out_path=weighted)


@pytest.mark.parametrize("kappa", (0.25, 3.0))
def test_another_kappa(torch, kappa):
    b = make_batch(257, 3, 51, 17)
    check(torch, b, "bootstrap", True, "discount", True, kappa=kappa)
    check(torch, b, "given", False, None, False, kappa=kappa)


def test_the_smallest_batch_that_takes_the_extra_launch(torch):
    from gym_amd import qr

    M = qr.LEAF_ROWS * qr.LEAF_ROWS + 1
    assert qr.launches(M) == qh.launches(M) == 4 and qr.launches(M - 1) == 3
    b = make_batch(M, 1, 1, 5)
    check(torch, b, "bootstrap", True, "discount", True, out_path=False)


def test_the_sizes_at_which_the_grids_stride(torch):
    """quantile_q_values: workgroups stride over tiles of TILE_ROWS (row, action) pairs — three iterations of the first workgroups, a
    partial last tile.  The rows and the backward kernels take one tile per workgroup and a grid that grows along y beyond GRID_X
    tiles: the second slice of the grid, with a partial last tile.  At the smallest head."""
    import gym_amd
    from gym_amd import qr

    A, N = 1, 1
    M = 2 * qr.MAX_BLOCKS * qr.TILE_ROWS + qr.TILE_ROWS + 1
    x = make_batch(M, A, N, 6)["quantiles"]
    q = gym_amd.quantile_q_values(dev(torch, x))
    _same32(torch, q, qh.q_values(x), "q_values strided")
    M = qr.GRID_X * qr.TILE_ROWS + qr.TILE_ROWS + 1
    b = make_batch(M, A, N, 7)
    check(torch, b, "bootstrap", False, "gamma", True, out_path=False)


# ---- tensor forms -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,N", ((3, 51), (7, 33)))
def test_strided_rows_leading_dims_action_widths_and_flag_dtypes(torch, A, N):
    import gym_amd

    K, B = 3, 87
    M = K * B
    b = make_batch(M, A, N, 60 + A)

    def wide(x):      # rows of a wider buffer: ld = A * N + 5
        buf = torch.full((x.shape[0], A * N + 5), float("nan"), device="cuda:0")
        buf[:, 2:2 + A * N] = x.reshape(x.shape[0], A * N)
        v = buf[:, 2:2 + A * N].unflatten(1, (A, N))
        assert v.stride(0) == A * N + 5 and not v.is_contiguous()
        return v

    def lead(x):
        return x.view((K, B) + tuple(x.shape[1:]))

    for mode, double, factor in MODES:
        check(torch, b, mode, double, factor, True, rows=wide, what="strided")
        check(torch, b, mode, double, factor, False, view=lead, rows=lead, what="[K, B, A, N]")
        check(torch, b, mode, double, factor, True, act=dev(torch, b["act"].astype(np.int32)), what="int32 actions")
    # bool and uint8 flags give the same bits
    kw = device_kwargs(torch, b, "bootstrap", True, "discount", False)
    x, a = dev(torch, b["quantiles"]), dev(torch, b["act"])
    l8, s8 = gym_amd.quantile_dqn_loss(x, a, **kw)
    lb, sb = gym_amd.quantile_dqn_loss(x, a, **dict(kw, terminated=kw["terminated"].bool()))
    l2, s2 = gym_amd.quantile_dqn_loss(x, a, **dict(kw, terminated=kw["terminated"] * 200))      # nonzero = set
    assert torch.equal(s8, sb) and torch.equal(l8, lb) and torch.equal(s8, s2) and int(kw["terminated"].sum()) > 0


# ---- the exact cases of the rule, one special row among ordinary ones ---------------------------------------------------------------------------------
def _special(torch, A, N, edit, mode="bootstrap", double=True, factor="discount", **over):
    """A batch of 70 ordinary rows edited by `edit(batch)`; checked against the twin with and without weights."""
    b = make_batch(70, A, N, 70 + A + N)
    b["term"][:] = 0
    b["term"][[3, 44]] = 1
    b["reward"] = np.clip(b["reward"], -2.0, 2.0)
    edit(b)
    s, g, T = check(torch, b, mode, double, factor, True, **over)
    check(torch, b, mode, double, factor, False, out_path=False, **over)
    return b, s, g, T


def test_one_quantile_with_kappa_one_is_half_the_huber_loss_of_the_scalar_twin(torch):
    import gym_amd

    M, A = 300, 4
    b = make_batch(M, A, 1, 7)
    b["reward"][::7] *= 5.0
    kw = kwargs(b, "bootstrap", True, "gamma", True)
    q, nq, on = (b[k][:, :, 0] for k in ("quantiles", "next", "online"))
    scalar = dict(reward=b["reward"], terminated=b["term"], next_q=nq, next_q_online=on, gamma=GAMMA, delta=1.0, weights=b["weights"])
    d = dh.rows(q, b["act"], **scalar)
    x = dev(torch, b["quantiles"]).requires_grad_()
    row_loss = torch.empty(M, device="cuda:0")
    loss, _ = gym_amd.quantile_dqn_loss(x, dev(torch, b["act"]), row_loss=row_loss, **device_kwargs(torch, b, "bootstrap", True, "gamma", True))
    _same32(torch, row_loss, 0.5 * d["h"], "half the huber term")
    (GRAD * loss).backward()
    gd = to_f32(0.5 * dh.backward(q, b["act"], np.float32(GRAD), **scalar)) + np.float32(0.0)
    assert np.array_equal(host_bits(torch, x.grad + 0.0), bits(gd).reshape(-1)) and np.count_nonzero(gd) > M // 2
    assert np.array_equal(bits(to_f32(qh.rows(b["quantiles"], b["act"], **kw)["ql"])), host_bits(torch, row_loss))


def test_a_constant_discount_gives_the_bits_of_the_scalar_gamma(torch):
    import gym_amd

    b = make_batch(500, 3, 51, 8)
    x, a = dev(torch, b["quantiles"]), dev(torch, b["act"])
    outs = []
    for factor in ("gamma", "discount"):
        kw = device_kwargs(torch, b, "bootstrap", True, factor, True)
        if factor == "gamma":
            kw["gamma"] = 0.96875
        else:
            kw["discount"] = torch.full((500,), 0.96875, device="cuda:0")
        row_loss, T = torch.empty(500, device="cuda:0"), torch.empty((500, 51), device="cuda:0")
        xg = x.clone().requires_grad_()
        loss, stats = gym_amd.quantile_dqn_loss(xg, a, row_loss=row_loss, targets_out=T, **kw)
        loss.backward()
        outs.append((loss.detach(), stats, row_loss, T, xg.grad))
    for one, per in zip(*outs):
        assert np.array_equal(host_bits(torch, one), host_bits(torch, per))
    b["discount"][:] = 0.96875
    check(torch, b, "bootstrap", True, "discount", True)


def test_a_discount_row_of_mixed_powers_matches_the_literal_form(torch):
    import gym_amd

    M, A, N = 400, 3, 33
    b = make_batch(M, A, N, 9)
    s, g, T = check(torch, b, "bootstrap", False, "discount", False)
    nxt, r, disc = dev(torch, b["next"]).double(), dev(torch, b["reward"]).double(), dev(torch, b["discount"]).double()
    j = gym_amd.quantile_q_values(dev(torch, b["next"])).argmax(1)
    live = dev(torch, b["term"] == 0)[:, None]
    want = torch.where(live, r[:, None] + disc[:, None] * nxt[torch.arange(M, device="cuda:0"), j], r[:, None].expand(M, N)).float()
    assert np.array_equal(want.cpu().numpy(), T) and len(set(b["discount"].tolist())) == 5


@pytest.mark.parametrize("A,N", ((3, 51), (7, 33)))
@pytest.mark.parametrize("value", (np.nan, np.inf, -np.inf))
def test_non_finite_next_quantiles_and_discounts_of_a_terminated_and_of_a_running_row(torch, A, N, value):
    def edit(b):
        b["next"][44] = value      # terminated: ignored entirely, and so is its discount
        b["online"][3, 1] = value
        b["discount"][3], b["discount"][44] = value, np.nan
        b["online"][41, A - 1, 5] = value      # running: a NaN mean makes the row NaN; an infinite one only decides the argmax

    b, s, g, T = _special(torch, A, N, edit)
    clean, _, gc, Tc = _special(torch, A, N, lambda b: None)
    others = np.arange(70) != 41
    assert np.array_equal(bits(g[others]), bits(gc[others])) and np.array_equal(bits(T[others]), bits(Tc[others]))
    assert np.isfinite(g[others]).all() and np.isfinite(T[others]).all() and np.isfinite(s[[1, 6, 7]]).all()
    if np.isnan(value):
        assert np.isnan(s[[0, 2, 3]]).all() and np.isnan(T[41]).all() and np.isnan(g[41, b["act"][41]]).all() and np.count_nonzero(np.isnan(g)) == N
        assert np.all(bits(g[41, b["act"][41]]) == 0x7FC00000)
    else:
        assert np.isfinite(s).all() and np.isfinite(g).all()


@pytest.mark.parametrize("A", (2, 4, 7, 64))
def test_ties_take_the_first_maximum(torch, A):
    N = 5

    def edit(b):
        b["online"][41] = b["online"][41, 0]                    # every action ties: the first
        b["online"][40] = b["online"][41, 0] - 3.0
        b["online"][40, [A // 2, A - 1]] = b["online"][41, 0]   # two maxima: the earlier
        for a in range(A):
            b["next"][40:42, a] = float(a)                      # the evaluating network marks action a by its value

    b, s, g, T = _special(torch, A, N, edit, factor="gamma", gamma=1.0)
    assert np.all(T[41] == b["reward"][41]) and np.all(T[40] == to_f32(np.float64(b["reward"][40]) + float(A // 2))) and np.isfinite(s).all()


def test_the_crossing_fraction_of_ascending_descending_and_single_quantiles(torch):
    M, A, N = 70, 3, 33
    b = make_batch(M, A, N, 4)
    asc = np.sort(b["quantiles"], -1) + np.arange(N, dtype=np.float32) * np.float32(0.01)
    for q, want in ((asc, 0.0), (asc[..., ::-1].copy(), 1.0)):
        s, _, _ = check(torch, dict(b, quantiles=q), "given", False, None, True)
        assert s[4] == want
    s, _, _ = check(torch, make_batch(M, A, 1, 5), "given", False, None, True)
    assert s[4] == 0.0


def test_a_nan_in_one_taken_row_makes_that_row_nan_and_no_other(torch):
    A, N = 4, 51

    def whole(b):
        b["quantiles"][17, b["act"][17], :] = np.nan

    def single(b):
        b["quantiles"][17, b["act"][17], 5] = np.nan

    clean, sc, gc, _ = _special(torch, A, N, lambda b: None)
    others = np.arange(70) != 17
    for edit, count in ((whole, N), (single, 1)):
        b, s, g, T = _special(torch, A, N, edit)
        assert np.isnan(s[[0, 1, 3]]).all() and np.isfinite(s[[2, 5, 6, 7]]).all() and np.count_nonzero(np.isnan(g)) == count
        assert np.isnan(g[17, b["act"][17], 5]) and np.array_equal(bits(g[others]), bits(gc[others])) and np.all(bits(g[np.isnan(g)]) == 0x7FC00000)
        p = qh.rows(clean["quantiles"], clean["act"], **kwargs(clean, "bootstrap", True, "discount", True))
        assert s[5] == np.float32(p["ql"][others].max()) and s[6] == np.float32(p["qa"][others].min()) and s[7] == np.float32(p["qa"][others].max())

    def target(b):
        b["target_quantiles"][17, 7] = np.nan

    b, s, g, T = _special(torch, A, N, target, mode="given", double=False, factor=None)
    assert np.isnan(g[17, b["act"][17]]).all() and np.count_nonzero(np.isnan(g)) == N and np.isnan(s[[0, 2, 3]]).all() and np.isfinite(s[1])


@pytest.mark.parametrize("A,N", ((1, 1), (3, 51), (7, 33)))
@pytest.mark.parametrize("width", ("int32", "int64"))
def test_actions_out_of_range_and_negative(torch, A, N, width):
    big = {"int32": 2 ** 31 - 1, "int64": 2 ** 31}[width]

    def edit(b):
        b["act"] = b["act"].astype(width)
        b["act"][41], b["act"][12], b["act"][13] = A, -1, big

    b, s, g, T = _special(torch, A, N, edit)
    rows_bad = np.isin(np.arange(70), (12, 13, 41))
    assert np.isnan(g[rows_bad]).all() and np.isfinite(g[~rows_bad]).all() and np.isnan(s[[0, 1, 3, 4]]).all() and np.isfinite(s[[2, 5, 6, 7]]).all()
    assert np.all(bits(g[rows_bad]) == 0x7FC00000) and np.isfinite(T).all()


# ---- the expected values -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,N", HEADS)
def test_q_values_equal_the_twin_and_their_argmax_is_the_j_star_of_the_loss(torch, A, N):
    """The probe: the evaluating network marks action a by the value a in all its quantiles; with reward 0 and gamma 1 every target
    quantile of a row reads the j* the loss selected."""
    import gym_amd

    M = 257
    b = make_batch(M, A, N, 90 + A + N)
    x = dev(torch, b["online"])
    q = gym_amd.quantile_q_values(x)
    assert tuple(q.shape) == (M, A)
    Q64 = qh.q_values(b["online"])
    _same32(torch, q, Q64, ("q_values", A, N))
    out = torch.empty((M, A), device="cuda:0")
    assert gym_amd.quantile_q_values(x.view(1, M, A, N), out=out.view(1, M, A)).data_ptr() == out.data_ptr()
    assert torch.equal(out, q)
    tied = np.sort(Q64, 1)
    assert A == 1 or not np.any(to_f32(tied[:, -1]) == to_f32(tied[:, -2]))      # no two expected values round to one float32
    marks = np.broadcast_to(np.arange(A, dtype=np.float32)[None, :, None], (M, A, N)).copy()
    T = torch.empty((M, N), device="cuda:0")
    gym_amd.quantile_dqn_loss(dev(torch, b["quantiles"]), dev(torch, b["act"]), reward=torch.zeros(M, device="cuda:0"),
                              terminated=torch.zeros(M, dtype=torch.uint8, device="cuda:0"), next_quantiles=dev(torch, marks), next_quantiles_online=x,
                              gamma=1.0, targets_out=T)
    jstar = q.argmax(1)
    assert torch.equal(T[:, 0].long(), jstar) and bool((T == T[:, :1]).all()) and np.array_equal(jstar.cpu().numpy(), qh.first_max(Q64))
    # non-finite rows
    bad = b["online"][:4].copy()
    bad[0, 0, 0], bad[1, A - 1, 0] = np.nan, np.inf
    _same32(torch, gym_amd.quantile_q_values(dev(torch, bad)), qh.q_values(bad), "bad rows")


# ---- the backward ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,N", ((2, 51), (7, 33)))
def test_the_gradient_through_a_linear_head(torch, A, N):
    """loss.backward() through a real torch.nn.Linear: d loss / d quantiles has the twin's bits, and the head's own gradients are what
    torch's linear backward makes of the twin's gradient — the same call on the same bits; an order of float32 additions of its own is
    allowed for, M 2^-24 sum |term| per element."""
    import gym_amd

    M = 257
    b = make_batch(M, A, N, 80 + A)
    rng = np.random.default_rng(81)
    obs = dev(torch, rng.standard_normal((M, 4)).astype(np.float32))
    torch.manual_seed(3)
    head = torch.nn.Linear(4, A * N).to("cuda:0")
    kw_d = device_kwargs(torch, b, "bootstrap", True, "discount", True)
    raw = head(obs)
    raw.retain_grad()
    loss, _ = gym_amd.quantile_dqn_loss(raw.unflatten(1, (A, N)), dev(torch, b["act"]), **kw_d)
    (GRAD * loss).backward()
    x_h = raw.detach().cpu().numpy().reshape(M, A, N)
    want = to_f32(qh.backward(x_h, b["act"], np.float32(GRAD), **kwargs(b, "bootstrap", True, "discount", True)))
    assert np.array_equal(host_bits(torch, raw.grad), bits(want).reshape(-1))
    got_w, got_b = head.weight.grad.clone(), head.bias.grad.clone()
    head.zero_grad()
    g = dev(torch, want.reshape(M, A * N))
    head(obs).backward(gradient=g)
    bar_w = M * 2.0 ** -24 * (g.abs().t().double() @ obs.abs().double())
    bar_b = M * 2.0 ** -24 * g.abs().double().sum(0)
    assert bool(((got_w - head.weight.grad).abs().double() <= bar_w).all()) and bool(((got_b - head.bias.grad).abs().double() <= bar_b).all())
    assert float(got_w.abs().max()) > 0.0


def test_no_gradient_is_computed_when_nothing_asks(torch):
    import gym_amd
    from gym_amd import qr

    b = make_batch(300, 4, 51, 9)
    x, a, t = dev(torch, b["quantiles"]), dev(torch, b["act"]), dev(torch, b["target_quantiles"])
    loss, stats = gym_amd.quantile_dqn_loss(x, a, target_quantiles=t)
    assert not loss.requires_grad and not stats.requires_grad
    with torch.no_grad():
        loss2, _ = gym_amd.quantile_dqn_loss(x.clone().requires_grad_(), a, target_quantiles=t)
    assert not loss2.requires_grad and torch.equal(loss, loss2)
    # without grad the call is its forward launches and nothing else: no autograd node that a backward could run is made
    assert loss.grad_fn is None and loss2.grad_fn is None
    ws = torch.empty(qr.workspace_bytes(300), dtype=torch.uint8, device="cuda:0")
    out = (torch.empty((), device="cuda:0"), torch.empty(8, device="cuda:0"))
    hip, side = _hip(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        gym_amd.quantile_dqn_loss(x, a, target_quantiles=t, workspace=ws, out=out)      # once outside the capture
        side.synchronize()
        rc, n = _captured_launches(hip, side.cuda_stream, lambda: int(gym_amd.quantile_dqn_loss(x, a, target_quantiles=t, workspace=ws, out=out)[0].requires_grad))
    side.synchronize()
    assert (rc, n) == (0, qr.launches(300)) and n == 2 and torch.equal(out[0], loss)


# ---- graph capture, launch counts, no synchronisation ------------------------------------------------------------------------------------------
def test_the_allocation_free_forward_replays_in_a_captured_graph(torch):
    import gym_amd
    from gym_amd import qr

    M, A, N = 3000, 3, 51
    batches = [make_batch(M, A, N, 40 + k) for k in range(3)]
    keys = ("quantiles", "act", "reward", "term", "next", "online", "discount", "weights")
    bufs = {k: dev(torch, batches[0][k]) for k in keys}
    ws = torch.empty(qr.workspace_bytes(M), dtype=torch.uint8, device="cuda:0")
    out = (torch.empty((), device="cuda:0"), torch.empty(8, device="cuda:0"))
    row_loss, targets_out = torch.empty(M, device="cuda:0"), torch.empty((M, N), device="cuda:0")

    def step():
        gym_amd.quantile_dqn_loss(bufs["quantiles"], bufs["act"], reward=bufs["reward"], terminated=bufs["term"], next_quantiles=bufs["next"],
                                  next_quantiles_online=bufs["online"], discount=bufs["discount"], weights=bufs["weights"], row_loss=row_loss,
                                  targets_out=targets_out, workspace=ws, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                # warm-up outside the capture
        side.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        step()
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before      # with out= and workspace= the call allocates nothing
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            step()
        for k in (0, 1, 2):
            for name in keys:
                bufs[name].copy_(dev(torch, batches[k][name]))
            g.replay()
            side.synchronize()
            want_loss, want_stats, want_ql, want_T = qh.loss_f32(batches[k]["quantiles"], batches[k]["act"], **kwargs(batches[k], "bootstrap", True, "discount", True))
            _same32(torch, out[0], [want_loss], k)
            _same32(torch, out[1], want_stats, k)
            _same32(torch, row_loss, want_ql, k)
            _same32(torch, targets_out, want_T, k)
    torch.cuda.current_stream().wait_stream(side)


@pytest.mark.parametrize("M,A,N", ((3, 2, 51), (1024, 7, 33), (1025, 6, 32), (1024 * 1024, 1, 1), (1024 * 1024 + 1, 1, 1)))
def test_launch_counts_and_no_synchronisation(torch, M, A, N):
    """2 launches forwards up to 1024 rows, 3 up to 2^20, 4 beyond; 1 backwards; 1 for the expected values — counted as the kernel nodes
    that the calls leave in a stream capture, which also shows that they neither synchronise nor allocate."""
    from gym_amd import qr

    hip = _hip()
    f32 = dict(dtype=torch.float32, device="cuda:0")
    x, nx, on, grad = (torch.zeros((M, A, N), **f32) for _ in range(4))
    reward, weights, row_loss, discount = (torch.zeros(M, **f32) for _ in range(4))
    targets_out, q = torch.zeros((M, N), **f32), torch.zeros((M, A), **f32)
    act = torch.zeros(M, dtype=torch.int64, device="cuda:0")
    term = torch.zeros(M, dtype=torch.uint8, device="cuda:0")
    ws = torch.empty(qr.workspace_bytes(M), dtype=torch.uint8, device="cuda:0")
    loss, stats, g = torch.empty((), **f32), torch.empty(8, **f32), torch.ones((), **f32)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = side.cuda_stream
    lib = qr.lib
    want = 2 if M <= 1024 else 3 if M <= 1024 * 1024 else 4
    assert qr.launches(M) == qh.launches(M) == want
    ins = (s, M, A, N, x.data_ptr(), A * N, act.data_ptr(), 8, None, reward.data_ptr(), term.data_ptr(), nx.data_ptr(), A * N, on.data_ptr(), A * N,
           GAMMA, discount.data_ptr(), 1.0, weights.data_ptr())
    calls = ((lambda: lib.mxv_qr_loss(*ins, ws.data_ptr(), ws.numel(), row_loss.data_ptr(), targets_out.data_ptr(), loss.data_ptr(), stats.data_ptr()), want),
             (lambda: lib.mxv_qr_loss_backward(*ins, g.data_ptr(), grad.data_ptr()), 1),
             (lambda: lib.mxv_qr_q_values(s, M, A, N, x.data_ptr(), A * N, q.data_ptr()), 1))
    for call, _ in calls:                                                     # once outside a capture: the kernels' code is loaded
        assert call() == 0, lib.mxv_qr_last_error()
    side.synchronize()
    for call, nodes in calls:
        rc, n = _captured_launches(hip, s, call)
        assert (rc, n) == (0, nodes), (rc, n, lib.mxv_qr_last_error())
    side.synchronize()


# ---- the loop with the n-step prioritised buffer --------------------------------------------------------------------------------------------------
def test_add_chunk_sample_loss_update_priorities_equals_the_twins_composition(torch):
    """NStepPrioritizedReplayBuffer.add_chunk -> sample -> quantile_dqn_loss(discount=batch["discount"], weights=, row_loss=) ->
    update_priorities, three rounds: the ring, the tree, the draws and the losses are those of tests/nstep_host.py, tests/prio_host.py and
    tests/qr_host.py composed."""
    import gym_amd
    from test_gpu_nstep import nstep_buffer_same_as, nstep_twin_insert
    from test_gpu_prio import sampled_same_as, tree_same_as
    from test_gpu_replay import down, typed_chunk

    C, W, A, N, B, n, gamma = 257, 4, 3, 51, 200, 3, 0.97      # the chunks' actions are 0..2
    alpha, eps, seed = 0.6, 1e-6, 9
    rng = np.random.default_rng(31)
    buf = gym_amd.NStepPrioritizedReplayBuffer(C, (W,), n, gamma, alpha=alpha, eps=eps, seed=seed, device=0)
    ring, tree, count = nh.Ring(C, W), ph.Tree(C), 0
    table = {k: make_batch(C, A, N, 50 + i)["quantiles"] for i, k in enumerate(("quantiles", "next", "online"))}      # a head per slot
    table_d = {k: dev(torch, v) for k, v in table.items()}
    row_loss = torch.empty(B, device="cuda:0")
    distinct = set()
    for rnd in range(3):
        first, traj, host = typed_chunk(torch, rng, 4, 25, (W,), np.float32, np.int32, np.float64)
        buf.add_chunk(first, traj)
        tree.insert(count, 100)
        count = nstep_twin_insert(ring, count, n, gamma, host)
        nstep_buffer_same_as(torch, buf, ring, (rnd, "ring"))
        beta = 0.4 + 0.3 * rnd
        batch = buf.sample(B, beta=beta)
        want_b = ph.sample(tree, ring, seed, rnd, B, beta)
        sampled_same_as(torch, batch, want_b, buf, B, (rnd, "sample"))
        k = want_b["indices"]
        disc = ring.discount[k].view(np.float32)
        assert np.array_equal(down(torch, batch["discount"].view(torch.int32)), ring.discount[k])
        distinct |= set(disc.tolist())
        loss, stats = gym_amd.quantile_dqn_loss(table_d["quantiles"][batch["indices"]], batch["actions"], reward=batch["reward"],
                                                terminated=batch["terminated"], next_quantiles=table_d["next"][batch["indices"]],
                                                next_quantiles_online=table_d["online"][batch["indices"]], discount=batch["discount"],
                                                weights=batch["weights"], row_loss=row_loss)
        want = qh.loss_f32(table["quantiles"][k], batch["actions"].cpu().numpy(), reward=batch["reward"].cpu().numpy(),
                           terminated=batch["terminated"].cpu().numpy(), next_quantiles=table["next"][k], next_quantiles_online=table["online"][k],
                           discount=disc, weights=want_b["weights"])
        _same32(torch, loss, [want[0]], rnd)
        _same32(torch, stats, want[1], rnd)
        _same32(torch, row_loss, want[2], rnd)
        buf.update_priorities(batch["indices"], row_loss)
        tree.update(count, k, want[2], alpha, eps)
        tree_same_as(torch, buf, tree, (rnd, "update"))
        assert np.isfinite(want[2]).all() and want[2].min() > 0.0
    assert len(distinct) >= 3      # windows of one, two and three steps were all drawn


# ---- the example --------------------------------------------------------------------------------------------------------------------------------
def test_the_example_repeats_itself(torch, capsys):
    """examples/qr_dqn_nstep_cartpole.py has no torch generator and no float atomic: two runs give the same history, number for number."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import qr_dqn_nstep_cartpole
    finally:
        sys.path.pop(0)
    kw = dict(num_envs=64, iterations=3, K=8, updates=2, batch=128, capacity=1024)
    first = qr_dqn_nstep_cartpole.train(**kw)
    assert "sample steps drawn" in capsys.readouterr().out
    again = qr_dqn_nstep_cartpole.train(**kw, verbose=False)
    assert first == again and len(first) == 3 and first[0]["beta"] == 0.4 and first[-1]["beta"] == 1.0
    for row in first:
        assert np.isfinite(list(row.values())).all() and row["row_loss_max"] >= row["loss_term"] > 0.0 and row["stored"] > 0
        assert 0.0 <= row["crossing_fraction"] <= 1.0 and 0.0 < row["discount_min"] <= row["discount_mean"] <= 0.99 + 1e-6


# ---- the Python front end on the device ----------------------------------------------------------------------------------------------------------
def test_python_argument_errors(torch):
    import gym_amd
    from gym_amd import qr

    M, A, N = 16, 3, 5
    f32 = dict(dtype=torch.float32, device="cuda:0")
    x, v, tq = torch.zeros((M, A, N), **f32), torch.zeros(M, **f32), torch.zeros((M, N), **f32)
    a = torch.zeros(M, dtype=torch.int64, device="cuda:0")
    term = torch.zeros(M, dtype=torch.bool, device="cuda:0")
    boot = dict(reward=v, terminated=term, next_quantiles=x)
    out = (torch.empty((), **f32), torch.empty(8, **f32))
    small = qr.workspace_bytes(M) - 8
    for kw, what in ((dict(), "exactly one target mode"), (dict(boot, target_quantiles=tq), "exactly one target mode"),
                     (dict(target_quantiles=tq, next_quantiles_online=x), "next_quantiles_online is given with target_quantiles"),
                     (dict(target_quantiles=tq, discount=v), "discount is given with target_quantiles"),
                     (dict(boot, gamma=0.99, discount=v), "gamma and discount are both given"),
                     (dict(reward=v, terminated=term), "next_quantiles missing"), (dict(target_quantiles=tq[:8]), "shape"),
                     (dict(boot, next_quantiles=torch.zeros((M, A + 1, N), **f32)), "shape"), (dict(target_quantiles=tq.double()), "float32"),
                     (dict(boot, terminated=v), "uint8"), (dict(boot, discount=v.double()), "float32"), (dict(boot, discount=v[:8]), "shape"),
                     (dict(target_quantiles=tq, actions=a.to(torch.int16)), "int64"),
                     (dict(target_quantiles=tq.cpu()), "device tensor"), (dict(boot, next_quantiles=x.cpu()), "device tensor"),
                     (dict(boot, discount=v.cpu()), "device tensor"), (dict(target_quantiles=tq, weights=v.cpu()), "device tensor"),
                     (dict(target_quantiles=tq.clone().requires_grad_()), "must not require grad"),
                     (dict(boot, next_quantiles=x.clone().requires_grad_()), "must not require grad"),
                     (dict(boot, next_quantiles_online=x.clone().requires_grad_()), "must not require grad"),
                     (dict(boot, discount=v.clone().requires_grad_()), "must not require grad"),
                     (dict(target_quantiles=tq, quantiles=x.clone().requires_grad_(), out=out), "requires grad"),
                     (dict(target_quantiles=tq, quantiles=x.clone().requires_grad_(), workspace=torch.empty(2048, dtype=torch.uint8, device="cuda:0")), "requires grad"),
                     (dict(target_quantiles=tq, workspace=torch.empty(small, dtype=torch.uint8, device="cuda:0")), "workspace holds"),
                     (dict(target_quantiles=tq, targets_out=tq), "targets_out overlaps the target_quantiles"), (dict(boot, row_loss=v), "row_loss overlaps the reward"),
                     (dict(target_quantiles=tq, kappa=0.0), "above 0"),
                     (dict(target_quantiles=tq, kappa=float("inf")), "finite"), (dict(target_quantiles=tq, quantiles=torch.zeros((M, A, 65), **f32)), "shape"),
                     (dict(boot, gamma=float("nan")), "finite")):
        args = dict(quantiles=x, actions=a)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            gym_amd.quantile_dqn_loss(args.pop("quantiles"), args.pop("actions"), **args)
    d = torch.zeros(M, **f32)
    with pytest.raises(ValueError, match="row_loss overlaps the discount"):
        gym_amd.quantile_dqn_loss(x, a, reward=v, terminated=term, next_quantiles=x, discount=d, row_loss=d)
    with pytest.raises(ValueError, match="q_out overlaps the quantiles"):
        gym_amd.quantile_q_values(x, out=x.view(-1)[:M * A].view(M, A))
    with pytest.raises(ValueError, match="device tensor"):
        gym_amd.quantile_q_values(x, out=torch.zeros((M, A)))
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="one device"):
            gym_amd.quantile_dqn_loss(x, a, target_quantiles=tq.to("cuda:1"))
