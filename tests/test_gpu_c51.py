"""gym_amd.categorical_dqn_loss and categorical_q_values on the device against tests/c51_host.py, bit for bit — the loss, the eight
diagnostics, row_loss, projected and the dense gradient: every size at which the tree changes shape (a partial tile, a partial leaf,
two leaves, the extra launch) times every kind of head (one action, the atom counts below, at and beside a wave, the action limit),
every target mode, double on and off, weights on and off; the sizes at which the grids stride; strided rows, leading dims, both action
widths and both flag dtypes; the exact cases of the rule; the expected values and their argmax; a real Linear head; the allocation-free
forward recorded in a graph; the launch counts and the absence of a synchronisation; a full prioritised-replay loop; the example run
twice; the front end's refusals."""
import os
import sys

import numpy as np
import pytest

import c51_host as ch
from c51_host import bits, to_f32
from conftest import ROOT
from test_c51_host import GAMMA, MODES, V_MAX, V_MIN, kwargs, make_batch
from test_gpu_ppo import _captured_launches, _hip

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099)
HEADS = ((1, 2), (2, 51), (3, 51), (6, 51), (4, 64), (2, 63), (7, 33), (64, 2))
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


def device_kwargs(torch, b, mode, double, weighted, view=lambda x: x, rows=lambda x: x, **over):
    kw = dict(v_min=V_MIN, v_max=V_MAX, weights=view(dev(torch, b["weights"])) if weighted else None)
    if mode == "given":
        kw["target_probs"] = view(dev(torch, b["target_probs"]))
    else:
        kw.update(reward=view(dev(torch, b["reward"])), terminated=view(dev(torch, b["term"])), next_logits=rows(dev(torch, b["next"])),
                  next_logits_online=rows(dev(torch, b["online"])) if double else None, gamma=GAMMA)
    kw.update(over)
    return kw


def twin(b, mode, double, weighted, **over):
    """The twin's forward and backward on the batch, a chunk of rows at a time -> (loss, stats, ce [M], m [M, Z], grad [M, A, Z])."""
    M, A, Z = b["logits"].shape
    cols = {k: [] for k in ("term", "qa", "y", "ent", "cm", "ce")}
    ms, grads = [], []
    for r0 in range(0, M, CHUNK):
        c = {k: v[r0:r0 + CHUNK] for k, v in b.items()}
        kw = kwargs(c, mode, double, weighted, **over)
        p = ch.rows(c["logits"], c["act"], **kw)
        for k in cols:
            cols[k].append(p[k])
        ms.append(p["m"][:, :Z])
        grads.append(to_f32(ch.grad_of(p, np.float32(GRAD), batch_rows=M)))
    p = {k: np.concatenate(v) for k, v in cols.items()}
    value, stats, _ = ch.finish(p)
    return value, stats, p["ce"], np.concatenate(ms), np.concatenate(grads)


def check(torch, b, mode, double, weighted, *, view=lambda x: x, rows=lambda x: x, act=None, out_path=True, what=None, **over):
    """One forward and one backward of the device on the batch `b` against the twin: everything bit for bit.  -> (stats, grad, projected)
    on the host."""
    import gym_amd

    M, A, Z = b["logits"].shape
    what = (what, M, A, Z, mode, double, weighted)
    want_loss, want_stats, want_ce, want_m, want_g = twin(b, mode, double, weighted, **over)
    kw_d = device_kwargs(torch, b, mode, double, weighted, view, rows, **over)
    logits = rows(dev(torch, b["logits"])).requires_grad_()
    actions = view(dev(torch, b["act"]) if act is None else act)
    row_loss = torch.full(tuple(actions.shape), 7.0, device="cuda:0")
    projected = torch.full(tuple(actions.shape) + (Z,), 7.0, device="cuda:0")
    loss, stats = gym_amd.categorical_dqn_loss(logits, actions, row_loss=row_loss, projected=projected, **kw_d)
    assert loss.dim() == 0 and loss.requires_grad and tuple(stats.shape) == (8,) and not stats.requires_grad
    _same32(torch, loss, [want_loss], (what, "loss"))
    _same32(torch, stats, want_stats, (what, "stats"))
    _same32(torch, row_loss, want_ce, (what, "row_loss"))
    _same32(torch, projected, want_m, (what, "projected"))
    assert host_bits(torch, stats)[0] == host_bits(torch, loss)[0]
    (GRAD * loss).backward()
    assert tuple(logits.grad.shape) == tuple(logits.shape) and logits.grad.is_contiguous(), what
    have = host_bits(torch, logits.grad)
    assert np.array_equal(have, bits(want_g).reshape(-1)), (what, "grad_logits", np.flatnonzero(have != bits(want_g).reshape(-1))[:8])
    if out_path:      # the same forward without autograd, into the caller's tensors
        out = (torch.empty((), device="cuda:0"), torch.empty(8, device="cuda:0"))
        with torch.no_grad():
            got = gym_amd.categorical_dqn_loss(logits, actions, out=out, **kw_d)
        assert got[0] is out[0] and got[1] is out[1]
        _same32(torch, out[0], [want_loss], (what, "out loss"))
        _same32(torch, out[1], want_stats, (what, "out stats"))
    return stats.cpu().numpy(), logits.grad.cpu().numpy().reshape(M, A, Z), projected.cpu().numpy().reshape(M, Z)


# ---- every size, every kind of head, every mode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", SIZES)
def test_loss_stats_row_loss_projected_and_gradient_match_the_twin(torch, M):
    for A, Z in HEADS:
        b = make_batch(M, A, Z, 3000 + M % 1000 + A + Z)
        for mode, double in MODES:
            for weighted in (True, False):
                check(torch, b, mode, double, weighted, out_path=weighted)


def test_the_smallest_batch_that_takes_the_extra_launch(torch):
    from gym_amd import c51

    M = c51.LEAF_ROWS * c51.LEAF_ROWS + 1
    assert c51.launches(M) == ch.launches(M) == 4 and c51.launches(M - 1) == 3
    b = make_batch(M, 1, 2, 5)
    check(torch, b, "bootstrap", True, True, out_path=False)


def test_the_sizes_at_which_the_grids_stride(torch):
    """categorical_q_values: workgroups stride over tiles of TILE_ROWS (row, action) pairs — three iterations of the first workgroups,
    a partial last tile.  The rows and the backward kernels take one tile per workgroup and a grid that grows along y beyond GRID_X
    tiles: the second slice of the grid, with a partial last tile.  At the smallest head."""
    import gym_amd
    from gym_amd import c51

    A, Z = 1, 2
    M = 2 * c51.MAX_BLOCKS * c51.TILE_ROWS + c51.TILE_ROWS + 1
    x = make_batch(M, A, Z, 6)["logits"]
    q = gym_amd.categorical_q_values(dev(torch, x), v_min=V_MIN, v_max=V_MAX)
    _same32(torch, q, ch.q_values(x, v_min=V_MIN, v_max=V_MAX), "q_values strided")
    M = c51.GRID_X * c51.TILE_ROWS + c51.TILE_ROWS + 1
    b = make_batch(M, A, Z, 7)
    check(torch, b, "bootstrap", False, True, out_path=False)


# ---- tensor forms -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,Z", ((3, 51), (7, 33)))
def test_strided_rows_leading_dims_action_widths_and_flag_dtypes(torch, A, Z):
    import gym_amd

    K, N = 3, 87
    M = K * N
    b = make_batch(M, A, Z, 60 + A)

    def wide(x):      # rows of a wider buffer: ld = A * Z + 5
        buf = torch.full((x.shape[0], A * Z + 5), float("nan"), device="cuda:0")
        buf[:, 2:2 + A * Z] = x.reshape(x.shape[0], A * Z)
        v = buf[:, 2:2 + A * Z].unflatten(1, (A, Z))
        assert v.stride(0) == A * Z + 5 and not v.is_contiguous()
        return v

    def lead(x):
        return x.view((K, N) + tuple(x.shape[1:]))

    for mode, double in MODES:
        check(torch, b, mode, double, True, rows=wide, what="strided")
        check(torch, b, mode, double, False, view=lead, rows=lead, what="[K, N, A, Z]")
        check(torch, b, mode, double, True, act=dev(torch, b["act"].astype(np.int32)), what="int32 actions")
    # bool and uint8 flags give the same bits
    kw = device_kwargs(torch, b, "bootstrap", True, False)
    x, a = dev(torch, b["logits"]), dev(torch, b["act"])
    l8, s8 = gym_amd.categorical_dqn_loss(x, a, **kw)
    lb, sb = gym_amd.categorical_dqn_loss(x, a, **dict(kw, terminated=kw["terminated"].bool()))
    l2, s2 = gym_amd.categorical_dqn_loss(x, a, **dict(kw, terminated=kw["terminated"] * 200))      # nonzero = set
    assert torch.equal(s8, sb) and torch.equal(l8, lb) and torch.equal(s8, s2) and int(kw["terminated"].sum()) > 0


# ---- the exact cases of the rule, one special row among ordinary ones ---------------------------------------------------------------------------------
def _special(torch, A, Z, edit, mode="bootstrap", double=True, **over):
    """A batch of 70 ordinary rows edited by `edit(batch)`; checked against the twin with and without weights."""
    b = make_batch(70, A, Z, 70 + A + Z)
    b["term"][:] = 0
    b["term"][[3, 44]] = 1
    b["reward"] = np.clip(b["reward"], -2.0, 2.0)
    edit(b)
    s, g, m = check(torch, b, mode, double, True, **over)
    check(torch, b, mode, double, False, out_path=False, **over)
    return b, s, g, m


@pytest.mark.parametrize("Z", (2, 33, 51, 64))
def test_b_on_an_atom_puts_the_whole_mass_there(torch, Z):
    def edit(b):
        b["reward"] = np.random.default_rng(Z).integers(-3, 4, 70).astype(np.float32)

    b, s, g, m = _special(torch, 3, Z, edit, double=False, gamma=1.0, v_min=0.0, v_max=float(Z - 1))
    for i in (3, 44):      # terminated: a one-hot at the clamped reward
        want = np.zeros(Z, np.float32)
        want[int(np.clip(b["reward"][i], 0, Z - 1))] = 1.0
        assert np.array_equal(m[i], want)
    assert np.all(np.abs(m.astype(np.float64).sum(1) - 1.0) <= Z * 2.0 ** -24) and np.isfinite(s).all()


def test_gamma_zero_with_a_reward_on_atom_k_gives_a_one_hot(torch):
    Z = 41      # dz = 0.5: every support point is a float32

    def edit(b):
        b["term"][:] = 0
        b["reward"] = (V_MIN + 0.5 * (np.arange(70) % Z)).astype(np.float32)

    b, s, g, m = _special(torch, 3, Z, edit, gamma=0.0)
    assert np.array_equal(np.argmax(m, 1), np.arange(70) % Z) and np.all((m != 0).sum(1) == 1) and np.all(m.max(1) >= 1.0 - 2.0 ** -23)


@pytest.mark.parametrize("A,Z", ((3, 51), (7, 33)))
@pytest.mark.parametrize("value", (np.nan, np.inf, -np.inf))
def test_non_finite_next_logits_of_a_terminated_and_of_a_running_row(torch, A, Z, value):
    def edit(b):
        b["next"][44] = value      # terminated: ignored entirely
        b["online"][3, 1] = value
        b["online"][41, A - 1, 5] = value      # running: NaN and +Inf make the row NaN; one -Inf logit is an atom without mass

    b, s, g, m = _special(torch, A, Z, edit)
    others = np.arange(70) != 41
    assert np.isfinite(g[others]).all() and np.isfinite(m[others]).all() and np.isfinite(s[[1, 3, 6, 7]]).all()
    if value == -np.inf:
        assert np.isfinite(s).all() and np.isfinite(g).all()
    else:
        assert np.isnan(s[[0, 2]]).all() and np.isnan(m[41]).all() and np.isnan(g[41, b["act"][41]]).all() and np.count_nonzero(np.isnan(g)) == Z
        assert np.all(bits(g[41, b["act"][41]]) == 0x7FC00000)


@pytest.mark.parametrize("A", (2, 4, 7, 64))
def test_ties_take_the_first_maximum(torch, A):
    Z = 5

    def edit(b):
        b["online"][41] = b["online"][41, 0]                          # every action ties: the first
        low = np.array([5.0, 0.0, 0.0, 0.0, 0.0], np.float32)         # its mass sits on the lowest atom
        b["online"][40] = low
        b["online"][40, [A // 2, A - 1]] = b["online"][41, 0]         # two maxima: the earlier
        for a in range(A):
            b["next"][40:42, a] = 0.0
            b["next"][40:42, a, a % Z] = 50.0                         # the evaluating network marks action a by atom a % Z

    b, s, g, m = _special(torch, A, Z, edit, gamma=1.0, v_min=0.0, v_max=4.0)
    p = ch.rows(b["logits"], b["act"], **kwargs(b, "bootstrap", True, False, gamma=1.0, v_min=0.0, v_max=4.0))
    assert p["jstar"][41] == 0 and p["jstar"][40] == A // 2 and np.isfinite(s).all()


def test_a_minus_inf_logit_under_zero_target_mass_costs_nothing(torch):
    def edit(b):
        for i in (4, 14):      # the rows whose given target is zero on the lower half
            b["logits"][i, b["act"][i], :5] = -np.inf
        b["logits"][24, b["act"][24], 40] = -np.inf      # under positive mass: +Inf

    b, s, g, m = _special(torch, 2, 51, edit, mode="given", double=False)
    assert s[0] == np.inf and s[5] == np.inf and np.isfinite(np.delete(g, 24, 0)).all()
    assert np.all(g[4, b["act"][4], :5] == 0.0)


@pytest.mark.parametrize("A,Z", ((1, 2), (3, 51), (7, 33)))
@pytest.mark.parametrize("width", ("int32", "int64"))
def test_actions_out_of_range_and_negative(torch, A, Z, width):
    big = {"int32": 2 ** 31 - 1, "int64": 2 ** 40 + 1}[width]

    def edit(b):
        b["act"] = b["act"].astype(width)
        b["act"][41], b["act"][12], b["act"][13] = A, -1, big

    b, s, g, m = _special(torch, A, Z, edit)
    rows_bad = np.isin(np.arange(70), (12, 13, 41))
    assert np.isnan(g[rows_bad]).all() and np.isfinite(g[~rows_bad]).all() and np.isnan(s[[0, 1, 3]]).all() and np.isfinite(s[[2, 4, 5, 6, 7]]).all()
    assert np.all(bits(g[rows_bad]) == 0x7FC00000) and np.isfinite(m).all()


# ---- the expected values -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,Z", HEADS)
def test_q_values_equal_the_twin_and_their_argmax_is_the_j_star_of_the_loss(torch, A, Z):
    """The probe: the evaluating network marks action a by all its mass on atom a % Z; with reward 0 and gamma 1 on the support 0 .. Z-1
    the projected target is that one-hot, so its argmax reads the j* the loss selected.  (gamma = 0 would move every atom to the reward
    and leave no trace of j*.)"""
    import gym_amd

    M = 257
    b = make_batch(M, A, Z, 90 + A + Z)
    x = dev(torch, b["online"])
    for lo, hi in ((V_MIN, V_MAX), (0.0, float(Z - 1))):
        q = gym_amd.categorical_q_values(x, v_min=lo, v_max=hi)
        assert tuple(q.shape) == (M, A)
        _same32(torch, q, ch.q_values(b["online"], v_min=lo, v_max=hi), ("q_values", A, Z))
    out = torch.empty((M, A), device="cuda:0")
    assert gym_amd.categorical_q_values(x.view(1, M, A, Z), v_min=0.0, v_max=float(Z - 1), out=out.view(1, M, A)).data_ptr() == out.data_ptr()
    assert torch.equal(out, q)
    Q64 = ch.q_values(b["online"], v_min=0.0, v_max=float(Z - 1))
    tied = np.sort(Q64, 1)
    assert A == 1 or not np.any(to_f32(tied[:, -1]) == to_f32(tied[:, -2]))      # no two expected values round to one float32
    marks = np.zeros((M, A, Z), np.float32)
    for a in range(A):
        marks[:, a, a % Z] = 80.0
    projected = torch.empty((M, Z), device="cuda:0")
    gym_amd.categorical_dqn_loss(dev(torch, b["logits"]), dev(torch, b["act"]), v_min=0.0, v_max=float(Z - 1), reward=torch.zeros(M, device="cuda:0"),
                                 terminated=torch.zeros(M, dtype=torch.uint8, device="cuda:0"), next_logits=dev(torch, marks), next_logits_online=x,
                                 gamma=1.0, projected=projected)
    jstar = q.argmax(1)
    assert torch.equal(projected.argmax(1), jstar % Z) and np.array_equal(jstar.cpu().numpy(), ch.first_max(Q64))
    # non-finite rows
    bad = b["online"][:4].copy()
    bad[0, 0, 1], bad[1, A - 1, 0], bad[2, 0, :] = np.nan, np.inf, -np.inf
    _same32(torch, gym_amd.categorical_q_values(dev(torch, bad), v_min=V_MIN, v_max=V_MAX), ch.q_values(bad, v_min=V_MIN, v_max=V_MAX), "bad rows")


# ---- the backward ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,Z", ((2, 51), (7, 33)))
def test_the_gradient_through_a_linear_head(torch, A, Z):
    """loss.backward() through a real torch.nn.Linear: d loss / d logits has the twin's bits, and the head's own gradients are what
    torch's linear backward makes of the twin's gradient — the same call on the same bits; an order of float32 additions of its own is
    allowed for, M 2^-24 sum |term| per element."""
    import gym_amd

    M = 257
    b = make_batch(M, A, Z, 80 + A)
    rng = np.random.default_rng(81)
    obs = dev(torch, rng.standard_normal((M, 4)).astype(np.float32))
    torch.manual_seed(3)
    head = torch.nn.Linear(4, A * Z).to("cuda:0")
    kw_d = device_kwargs(torch, b, "bootstrap", True, True)
    raw = head(obs)
    raw.retain_grad()
    loss, _ = gym_amd.categorical_dqn_loss(raw.unflatten(1, (A, Z)), dev(torch, b["act"]), **kw_d)
    (GRAD * loss).backward()
    x_h = raw.detach().cpu().numpy().reshape(M, A, Z)
    want = to_f32(ch.backward(x_h, b["act"], np.float32(GRAD), **kwargs(b, "bootstrap", True, True)))
    assert np.array_equal(host_bits(torch, raw.grad), bits(want).reshape(-1))
    got_w, got_b = head.weight.grad.clone(), head.bias.grad.clone()
    head.zero_grad()
    g = dev(torch, want.reshape(M, A * Z))
    head(obs).backward(gradient=g)
    bar_w = M * 2.0 ** -24 * (g.abs().t().double() @ obs.abs().double())
    bar_b = M * 2.0 ** -24 * g.abs().double().sum(0)
    assert bool(((got_w - head.weight.grad).abs().double() <= bar_w).all()) and bool(((got_b - head.bias.grad).abs().double() <= bar_b).all())
    assert float(got_w.abs().max()) > 0.0


def test_no_gradient_is_computed_when_nothing_asks(torch):
    import gym_amd

    b = make_batch(300, 4, 51, 9)
    x, a, t = dev(torch, b["logits"]), dev(torch, b["act"]), dev(torch, b["target_probs"])
    loss, stats = gym_amd.categorical_dqn_loss(x, a, v_min=V_MIN, v_max=V_MAX, target_probs=t)
    assert not loss.requires_grad and not stats.requires_grad
    with torch.no_grad():
        loss2, _ = gym_amd.categorical_dqn_loss(x.clone().requires_grad_(), a, v_min=V_MIN, v_max=V_MAX, target_probs=t)
    assert not loss2.requires_grad and torch.equal(loss, loss2)


# ---- graph capture, launch counts, no synchronisation ------------------------------------------------------------------------------------------
def test_the_allocation_free_forward_replays_in_a_captured_graph(torch):
    import gym_amd
    from gym_amd import c51

    M, A, Z = 3000, 3, 51
    batches = [make_batch(M, A, Z, 40 + k) for k in range(3)]
    keys = ("logits", "act", "reward", "term", "next", "online", "weights")
    bufs = {k: dev(torch, batches[0][k]) for k in keys}
    ws = torch.empty(c51.workspace_bytes(M), dtype=torch.uint8, device="cuda:0")
    out = (torch.empty((), device="cuda:0"), torch.empty(8, device="cuda:0"))
    row_loss, projected = torch.empty(M, device="cuda:0"), torch.empty((M, Z), device="cuda:0")

    def step():
        gym_amd.categorical_dqn_loss(bufs["logits"], bufs["act"], v_min=V_MIN, v_max=V_MAX, reward=bufs["reward"], terminated=bufs["term"],
                                     next_logits=bufs["next"], next_logits_online=bufs["online"], gamma=GAMMA, weights=bufs["weights"],
                                     row_loss=row_loss, projected=projected, workspace=ws, out=out)

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
            want_loss, want_stats, want_ce, want_m = ch.loss_f32(batches[k]["logits"], batches[k]["act"], **kwargs(batches[k], "bootstrap", True, True))
            _same32(torch, out[0], [want_loss], k)
            _same32(torch, out[1], want_stats, k)
            _same32(torch, row_loss, want_ce, k)
            _same32(torch, projected, want_m, k)
    torch.cuda.current_stream().wait_stream(side)


@pytest.mark.parametrize("M,A,Z", ((3, 2, 51), (1024, 7, 33), (1025, 6, 51), (1024 * 1024, 1, 2), (1024 * 1024 + 1, 1, 2)))
def test_launch_counts_and_no_synchronisation(torch, M, A, Z):
    """2 launches forwards up to 1024 rows, 3 up to 2^20, 4 beyond; 1 backwards; 1 for the expected values — counted as the kernel nodes
    that the calls leave in a stream capture, which also shows that they neither synchronise nor allocate."""
    from gym_amd import c51

    hip = _hip()
    f32 = dict(dtype=torch.float32, device="cuda:0")
    x, nx, on, grad = (torch.zeros((M, A, Z), **f32) for _ in range(4))
    reward, weights, row_loss = (torch.zeros(M, **f32) for _ in range(3))
    projected, q = torch.zeros((M, Z), **f32), torch.zeros((M, A), **f32)
    act = torch.zeros(M, dtype=torch.int64, device="cuda:0")
    term = torch.zeros(M, dtype=torch.uint8, device="cuda:0")
    ws = torch.empty(c51.workspace_bytes(M), dtype=torch.uint8, device="cuda:0")
    loss, stats, g = torch.empty((), **f32), torch.empty(8, **f32), torch.ones((), **f32)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = side.cuda_stream
    lib = c51.lib
    want = 2 if M <= 1024 else 3 if M <= 1024 * 1024 else 4
    assert c51.launches(M) == ch.launches(M) == want
    ins = (s, M, A, Z, x.data_ptr(), A * Z, act.data_ptr(), 8, None, reward.data_ptr(), term.data_ptr(), nx.data_ptr(), A * Z, on.data_ptr(), A * Z,
           GAMMA, V_MIN, V_MAX, weights.data_ptr())
    calls = ((lambda: lib.mxv_c51_loss(*ins, ws.data_ptr(), ws.numel(), row_loss.data_ptr(), projected.data_ptr(), loss.data_ptr(), stats.data_ptr()), want),
             (lambda: lib.mxv_c51_loss_backward(*ins, g.data_ptr(), grad.data_ptr()), 1),
             (lambda: lib.mxv_c51_q_values(s, M, A, Z, x.data_ptr(), A * Z, V_MIN, V_MAX, q.data_ptr()), 1))
    for call, _ in calls:                                                     # once outside a capture: the kernels' code is loaded
        assert call() == 0, lib.mxv_c51_last_error()
    side.synchronize()
    for call, nodes in calls:
        rc, n = _captured_launches(hip, s, call)
        assert (rc, n) == (0, nodes), (rc, n, lib.mxv_c51_last_error())
    side.synchronize()


# ---- the loop with the prioritised buffer --------------------------------------------------------------------------------------------------------
def test_sample_loss_update_priorities_equals_the_twins_composition(torch):
    """PrioritizedReplayBuffer.sample -> categorical_dqn_loss(weights=, row_loss=) -> update_priorities, three rounds: the tree, the
    draws and the losses are those of tests/prio_host.py composed with tests/c51_host.py."""
    import gym_amd
    from test_gpu_prio import Pair, tree_same_as

    C, W, A, Z, B = 257, 4, 3, 51, 200      # the chunks' actions are 0..2
    rng = np.random.default_rng(31)
    p = Pair(torch, C, W, seed=9)
    p.add(rng, 2, 100, "first chunk")
    table = {k: (rng.standard_normal((C, A, Z)) * 2.0).astype(np.float32) for k in ("logits", "next", "online")}      # a head per slot
    table_d = {k: dev(torch, v) for k, v in table.items()}
    row_loss = torch.empty(B, device="cuda:0")
    for rnd in range(3):
        batch = p.sample(B, 0.4 + 0.3 * rnd, rnd)      # equal to the twin's draw, weights included
        idx = batch["indices"]
        kw = dict(v_min=-3.0, v_max=3.0, gamma=GAMMA)
        loss, stats = gym_amd.categorical_dqn_loss(table_d["logits"][idx], batch["actions"], reward=batch["reward"], terminated=batch["terminated"],
                                                   next_logits=table_d["next"][idx], next_logits_online=table_d["online"][idx],
                                                   weights=batch["weights"], row_loss=row_loss, **kw)
        k = idx.cpu().numpy()
        want = ch.loss_f32(table["logits"][k], batch["actions"].cpu().numpy(), reward=batch["reward"].cpu().numpy(),
                           terminated=batch["terminated"].cpu().numpy(), next_logits=table["next"][k], next_logits_online=table["online"][k],
                           weights=batch["weights"].cpu().numpy(), **kw)
        _same32(torch, loss, [want[0]], rnd)
        _same32(torch, stats, want[1], rnd)
        _same32(torch, row_loss, want[2], rnd)
        p.buf.update_priorities(idx, row_loss)
        p.tree.update(p.count, k, want[2], p.alpha, p.eps)
        tree_same_as(torch, p.buf, p.tree, (rnd, "update"))
        assert np.isfinite(want[2]).all() and want[2].min() > 0.0


# ---- the example --------------------------------------------------------------------------------------------------------------------------------
def test_the_example_repeats_itself(torch, capsys):
    """examples/c51_cartpole.py has no torch generator and no float atomic: two runs give the same history, number for number."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import c51_cartpole
    finally:
        sys.path.pop(0)
    kw = dict(num_envs=64, iterations=3, K=8, updates=2, batch=128, capacity=1024)
    first = c51_cartpole.train(**kw)
    assert "sample steps drawn" in capsys.readouterr().out
    again = c51_cartpole.train(**kw, verbose=False)
    assert first == again and len(first) == 3 and first[0]["beta"] == 0.4 and first[-1]["beta"] == 1.0
    for row in first:
        assert np.isfinite(list(row.values())).all() and row["row_loss_max"] >= row["loss_term"] > 0.0 and row["stored"] > 0
        assert 0.0 < row["entropy_mean"] <= np.log(51) + 1e-5 and 0.0 <= row["clipped_mass_mean"] <= 1.0


# ---- the Python front end on the device ----------------------------------------------------------------------------------------------------------
def test_python_argument_errors(torch):
    import gym_amd
    from gym_amd import c51

    M, A, Z = 16, 3, 5
    f32 = dict(dtype=torch.float32, device="cuda:0")
    x, v, tp = torch.zeros((M, A, Z), **f32), torch.zeros(M, **f32), torch.zeros((M, Z), **f32)
    a = torch.zeros(M, dtype=torch.int64, device="cuda:0")
    term = torch.zeros(M, dtype=torch.bool, device="cuda:0")
    boot = dict(reward=v, terminated=term, next_logits=x)
    out = (torch.empty((), **f32), torch.empty(8, **f32))
    small = c51.workspace_bytes(M) - 8
    for kw, what in ((dict(), "exactly one target mode"), (dict(boot, target_probs=tp), "exactly one target mode"),
                     (dict(target_probs=tp, next_logits_online=x), "next_logits_online is given with target_probs"),
                     (dict(reward=v, terminated=term), "next_logits missing"), (dict(target_probs=tp[:8]), "shape"),
                     (dict(boot, next_logits=torch.zeros((M, A + 1, Z), **f32)), "shape"), (dict(target_probs=tp.double()), "float32"),
                     (dict(boot, terminated=v), "uint8"), (dict(target_probs=tp, actions=a.to(torch.int16)), "int64"),
                     (dict(target_probs=tp.cpu()), "device tensor"), (dict(boot, next_logits=x.cpu()), "device tensor"),
                     (dict(target_probs=tp, weights=v.cpu()), "device tensor"), (dict(target_probs=tp.clone().requires_grad_()), "must not require grad"),
                     (dict(boot, next_logits=x.clone().requires_grad_()), "must not require grad"),
                     (dict(boot, next_logits_online=x.clone().requires_grad_()), "must not require grad"),
                     (dict(target_probs=tp, logits=x.clone().requires_grad_(), out=out), "requires grad"),
                     (dict(target_probs=tp, logits=x.clone().requires_grad_(), workspace=torch.empty(2048, dtype=torch.uint8, device="cuda:0")), "requires grad"),
                     (dict(target_probs=tp, workspace=torch.empty(small, dtype=torch.uint8, device="cuda:0")), "workspace holds"),
                     (dict(target_probs=tp, projected=tp), "projected overlaps the target_probs"), (dict(boot, row_loss=v), "row_loss overlaps the reward"),
                     (dict(target_probs=tp, v_min=1.0, v_max=1.0), "below v_max"), (dict(target_probs=tp, v_max=float("inf")), "finite"),
                     (dict(target_probs=tp, logits=torch.zeros((M, A, 65), **f32)), "shape"), (dict(boot, gamma=float("nan")), "finite")):
        args = dict(logits=x, actions=a, v_min=0.0, v_max=1.0)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            gym_amd.categorical_dqn_loss(args.pop("logits"), args.pop("actions"), **args)
    with pytest.raises(ValueError, match="q_out overlaps the logits"):
        gym_amd.categorical_q_values(x, v_min=0.0, v_max=1.0, out=x.view(-1)[:M * A].view(M, A))
    with pytest.raises(ValueError, match="device tensor"):
        gym_amd.categorical_q_values(x, v_min=0.0, v_max=1.0, out=torch.zeros((M, A)))
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="one device"):
            gym_amd.categorical_dqn_loss(x, a, v_min=0.0, v_max=1.0, target_probs=tp.to("cuda:1"))
