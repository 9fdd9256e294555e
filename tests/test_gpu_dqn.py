"""gym_amd.dqn_loss on the device against tests/dqn_host.py, bit for bit — the loss, the eight diagnostics, td_error and the dense gradient:
every size at which the tree changes shape (a partial wave, a partial workgroup, a partial leaf, two leaves, the third launch) times
every kind of action count (1, the four straight-line ones, the loops, the limit), both target modes, double on and off, weights on
and off, delta 1 and inf; strided rows, leading dims, both action widths and both flag dtypes; one special row among ordinary ones;
an incoming gradient other than 1 and a real Linear head; the allocation-free forward recorded in a graph; the launch counts and the
absence of a synchronisation; targets that are gae's returns on a real rollout chunk; the example run twice; the front end's refusals."""
import math

import numpy as np
import pytest

import dqn_host as dq
from dqn_host import bits, to_f32
from test_dqn_host import GAMMA, MODES, kwargs, make_batch
from test_gpu_ppo import _captured_launches, _hip

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099)
ACTIONS = (1, 2, 3, 4, 6, 7, 64)
GRAD = 2.5


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


def device_kwargs(torch, b, mode, double, weighted, delta, view=lambda x: x, rows=lambda x: x):
    kw = dict(delta=delta, weights=view(dev(torch, b["weights"])) if weighted else None)
    if mode == "targets":
        kw["targets"] = view(dev(torch, b["targets"]))
    else:
        kw.update(reward=view(dev(torch, b["reward"])), terminated=view(dev(torch, b["term"])), next_q=rows(dev(torch, b["next_q"])),
                  next_q_online=rows(dev(torch, b["online"])) if double else None, gamma=GAMMA)
    return kw


def check(torch, b, mode, double, weighted, delta, *, view=lambda x: x, rows=lambda x: x, act=None, out_path=True, what=None):
    """One forward and one backward of the device on the batch `b` against the twin: everything bit for bit.  -> (stats, grad) on the host."""
    import gym_amd

    M, A = b["q"].shape
    what = (what, M, A, mode, double, weighted, delta)
    kw_h = kwargs(b, mode, double, weighted, delta)
    want_loss, want_stats, want_td = dq.loss_f32(b["q"], b["act"], **kw_h)
    want_g = dq.backward(b["q"], b["act"], np.float32(GRAD), **kw_h)
    kw_d = device_kwargs(torch, b, mode, double, weighted, delta, view, rows)
    q = rows(dev(torch, b["q"])).requires_grad_()
    actions = view(dev(torch, b["act"]) if act is None else act)
    td = view(torch.full((M,), 7.0, device="cuda:0"))
    loss, stats = gym_amd.dqn_loss(q, actions, td_error=td, **kw_d)
    assert loss.dim() == 0 and loss.requires_grad and tuple(stats.shape) == (8,) and not stats.requires_grad
    _same32(torch, loss, [want_loss], (what, "loss"))
    _same32(torch, stats, want_stats, (what, "stats"))
    _same32(torch, td, want_td, (what, "td_error"))
    assert host_bits(torch, stats)[0] == host_bits(torch, loss)[0]
    (GRAD * loss).backward()
    assert tuple(q.grad.shape) == tuple(q.shape) and q.grad.is_contiguous(), what
    _same32(torch, q.grad, want_g, (what, "grad_q"))
    if out_path:      # the same forward without autograd, into the caller's tensors
        out = (torch.empty((), device="cuda:0"), torch.empty(8, device="cuda:0"))
        with torch.no_grad():
            got = gym_amd.dqn_loss(q, actions, out=out, **kw_d)
        assert got[0] is out[0] and got[1] is out[1]
        _same32(torch, out[0], [want_loss], (what, "out loss"))
        _same32(torch, out[1], want_stats, (what, "out stats"))
    return stats.cpu().numpy(), q.grad.cpu().numpy()


# ---- every size, every kind of action count, every mode -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", SIZES)
def test_loss_stats_td_error_and_gradient_match_the_twin(torch, M):
    for A in ACTIONS:
        b = make_batch(M, A, 3000 + M % 1000 + A)
        for mode, double in MODES:
            for weighted in (True, False):
                for delta in (1.0, math.inf):
                    check(torch, b, mode, double, weighted, delta, out_path=weighted and delta == 1.0)


def test_the_smallest_batch_that_takes_a_third_launch(torch):
    from gym_amd import dqn

    M = 1024 * 1024 + 5
    assert dqn.launches(M) == dq.launches(M) == 3 and dqn.launches(M - 5) == 2
    b = make_batch(M, 2, 5)
    check(torch, b, "bootstrap", True, True, 1.0, out_path=False)
    check(torch, b, "targets", False, False, 1.0, out_path=False)


# ---- tensor forms -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", (3, 7))
def test_strided_rows_leading_dims_action_widths_and_flag_dtypes(torch, A):
    import gym_amd

    K, N = 3, 87
    M = K * N
    b = make_batch(M, A, 60 + A)

    def wide(x):      # rows of a wider buffer: ld = A + 5
        buf = torch.full((x.shape[0], A + 5), float("nan"), device="cuda:0")
        buf[:, 2:2 + A] = x
        v = buf[:, 2:2 + A]
        assert v.stride(0) == A + 5 and not v.is_contiguous()
        return v

    for mode, double in MODES:
        check(torch, b, mode, double, True, 1.0, rows=wide, what="strided")
        check(torch, b, mode, double, False, 1.0, view=lambda x: x.view(K, N), rows=lambda x: x.view(K, N, A), what="[K, N, A]")
        check(torch, b, mode, double, True, 1.0, act=dev(torch, b["act"].astype(np.int32)), what="int32 actions")
    # bool and uint8 flags give the same bits
    kw = device_kwargs(torch, b, "bootstrap", True, False, 1.0)
    q, a = dev(torch, b["q"]), dev(torch, b["act"])
    l8, s8 = gym_amd.dqn_loss(q, a, **kw)
    lb, sb = gym_amd.dqn_loss(q, a, **dict(kw, terminated=kw["terminated"].bool()))
    l2, s2 = gym_amd.dqn_loss(q, a, **dict(kw, terminated=kw["terminated"] * 200))      # nonzero = set
    assert torch.equal(s8, sb) and torch.equal(l8, lb) and torch.equal(s8, s2) and int(kw["terminated"].sum()) > 0


# ---- special rows: one among ordinary ones --------------------------------------------------------------------------------------------------------
def _special(torch, A, edit, mode="bootstrap", double=True):
    """A batch of 70 ordinary rows with row 41 edited by `edit(batch)`; checked against the twin with and without weights."""
    b = make_batch(70, A, 70 + A)
    b["term"][:] = 0
    b["term"][[3, 44]] = 1
    edit(b)
    s, g = check(torch, b, mode, double, True, 1.0)
    check(torch, b, mode, double, False, math.inf, out_path=False)
    return b, s, g


@pytest.mark.parametrize("A", (3, 7))
@pytest.mark.parametrize("value", (np.nan, np.inf, -np.inf))
def test_a_non_finite_taken_q(torch, A, value):
    def edit(b):
        b["q"][41, b["act"][41]] = value

    b, s, g = _special(torch, A, edit, mode="targets", double=False)
    others = np.arange(70) != 41
    assert np.isfinite(g[others]).all() and np.count_nonzero(g[41] != 0) == 1
    if np.isnan(value):
        assert np.isnan(s[:3]).all() and np.isfinite(s[3:]).all() and np.isnan(g[41, b["act"][41]])
    else:      # an infinite error is in the linear zone: a gradient of +-delta times the weight, an infinite loss
        gs = np.float64(np.float32(GRAD)) / np.float64(70)
        assert s[0] == np.inf and s[5] == np.inf and g[41, b["act"][41]] == np.float32(gs * (np.float64(b["weights"][41]) * np.sign(value)))


@pytest.mark.parametrize("A", (3, 7))
@pytest.mark.parametrize("value", (np.nan, np.inf, -np.inf))
def test_a_non_finite_next_q_of_a_terminated_and_of_a_running_row(torch, A, value):
    def edit(b):
        b["next_q"][44] = value      # terminated: ignored entirely
        b["online"][3, 1] = value
        b["next_q"][41, int(np.argmax(b["online"][41]))] = value      # running: reaches the target

    b, s, g = _special(torch, A, edit)
    others = np.arange(70) != 41
    assert np.isfinite(g[others]).all() and np.isfinite(s[[2, 6, 7]]).all()
    assert (np.isnan(s[0]) and np.isnan(g[41, b["act"][41]])) if np.isnan(value) else np.isinf(s[0])


@pytest.mark.parametrize("A", (3, 7))
@pytest.mark.parametrize("double", (False, True))
def test_a_nan_in_the_selecting_row(torch, A, double):
    def edit(b):
        (b["online"] if double else b["next_q"])[41, A - 1] = np.nan
        (b["online"] if double else b["next_q"])[44, 0] = np.nan      # terminated: ignored

    b, s, g = _special(torch, A, edit, double=double)
    assert np.isnan(s[[0, 1, 3]]).all() and np.isfinite(s[[2, 4, 5, 6, 7]]).all() and np.count_nonzero(np.isnan(g)) == 1 and np.isnan(g[41, b["act"][41]])


@pytest.mark.parametrize("A", (2, 4, 7, 64))
def test_ties_take_the_first_maximum(torch, A):
    def edit(b):
        b["online"][41] = 1.5                       # every action ties: the first
        b["online"][40, :] = -1.0
        b["online"][40, [A // 2, A - 1]] = 2.0      # two maxima: the earlier
        b["online"][39] = -0.0
        b["online"][39, A - 1] = 0.0                # -0.0 before +0.0: equal, the first
        b["online"][38] = -np.inf                   # nothing but -inf: the first

    b, s, g = _special(torch, A, edit)
    p = dq.rows(b["q"], b["act"], **kwargs(b, "bootstrap", True, False, 1.0))
    nq = b["next_q"].astype(np.float64)
    r = b["reward"].astype(np.float64)
    assert np.array_equal(p["y"][[41, 40, 39, 38]], r[[41, 40, 39, 38]] + GAMMA * np.array([nq[41, 0], nq[40, A // 2], nq[39, 0], nq[38, 0]]))
    assert np.isfinite(s).all()


@pytest.mark.parametrize("A", (1, 3, 7))
@pytest.mark.parametrize("width", ("int32", "int64"))
def test_actions_out_of_range_and_negative(torch, A, width):
    big = {"int32": 2 ** 31 - 1, "int64": 2 ** 40 + 1}[width]

    def edit(b):
        b["act"] = b["act"].astype(width)
        b["act"][41], b["act"][12], b["act"][13] = A, -1, big

    b, s, g = _special(torch, A, edit, mode="targets", double=False)
    rows_bad = np.isin(np.arange(70), (12, 13, 41))
    assert np.isnan(g[rows_bad]).all() and np.isfinite(g[~rows_bad]).all() and np.isnan(s[[0, 1, 2]]).all() and np.isfinite(s[3:]).all()
    assert np.all(bits(g[rows_bad]) == 0x7FC00000)


# ---- the backward ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", (2, 7))
def test_the_gradient_through_a_linear_head(torch, A):
    """loss.backward() through a real torch.nn.Linear: d loss / d q has the twin's bits, and the head's own gradients are what torch's
    linear backward makes of the twin's grad_q — the same call on the same bits; an order of float32 additions of its own is allowed
    for, M 2^-24 sum |term| per element."""
    import gym_amd

    M = 257
    b = make_batch(M, A, 80 + A)
    rng = np.random.default_rng(81)
    obs = dev(torch, rng.standard_normal((M, 4)).astype(np.float32))
    torch.manual_seed(3)
    head = torch.nn.Linear(4, A).to("cuda:0")
    kw_d = device_kwargs(torch, b, "bootstrap", True, True, 1.0)
    q = head(obs)
    q.retain_grad()
    loss, _ = gym_amd.dqn_loss(q, dev(torch, b["act"]), **kw_d)
    (GRAD * loss).backward()
    q_h = q.detach().cpu().numpy()
    want = to_f32(dq.backward(q_h, b["act"], np.float32(GRAD), **kwargs(b, "bootstrap", True, True, 1.0)))
    assert np.array_equal(host_bits(torch, q.grad), bits(want).reshape(-1))
    got_w, got_b = head.weight.grad.clone(), head.bias.grad.clone()
    head.zero_grad()
    g = dev(torch, want)
    head(obs).backward(gradient=g)
    bar_w = M * 2.0 ** -24 * (g.abs().t().double() @ obs.abs().double())
    bar_b = M * 2.0 ** -24 * g.abs().double().sum(0)
    assert bool(((got_w - head.weight.grad).abs().double() <= bar_w).all()) and bool(((got_b - head.bias.grad).abs().double() <= bar_b).all())
    assert float(got_w.abs().max()) > 0.0


def test_no_gradient_is_computed_for_a_q_that_does_not_ask(torch):
    import gym_amd

    b = make_batch(300, 4, 9)
    q, a, t = dev(torch, b["q"]), dev(torch, b["act"]), dev(torch, b["targets"])
    loss, stats = gym_amd.dqn_loss(q, a, targets=t)
    assert not loss.requires_grad and not stats.requires_grad
    with torch.no_grad():
        loss2, _ = gym_amd.dqn_loss(q.clone().requires_grad_(), a, targets=t)
    assert not loss2.requires_grad and torch.equal(loss, loss2)


# ---- graph capture, launch counts, no synchronisation ------------------------------------------------------------------------------------------
def test_the_allocation_free_forward_replays_in_a_captured_graph(torch):
    import gym_amd
    from gym_amd import dqn

    M, A = 5000, 6
    batches = [make_batch(M, A, 40 + k) for k in range(3)]
    keys = ("q", "act", "reward", "term", "next_q", "online", "weights")
    bufs = {k: dev(torch, batches[0][k]) for k in keys}
    ws = torch.empty(dqn.workspace_bytes(M), dtype=torch.uint8, device="cuda:0")
    out = (torch.empty((), device="cuda:0"), torch.empty(8, device="cuda:0"))
    td = torch.empty(M, device="cuda:0")

    def step():
        gym_amd.dqn_loss(bufs["q"], bufs["act"], reward=bufs["reward"], terminated=bufs["term"], next_q=bufs["next_q"], next_q_online=bufs["online"],
                         gamma=GAMMA, weights=bufs["weights"], td_error=td, workspace=ws, out=out)

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
        for k in (1, 2):
            for name in keys:
                bufs[name].copy_(dev(torch, batches[k][name]))
            g.replay()
            side.synchronize()
            want_loss, want_stats, want_td = dq.loss_f32(batches[k]["q"], batches[k]["act"], **kwargs(batches[k], "bootstrap", True, True, 1.0))
            _same32(torch, out[0], [want_loss], k)
            _same32(torch, out[1], want_stats, k)
            _same32(torch, td, want_td, k)
    torch.cuda.current_stream().wait_stream(side)


@pytest.mark.parametrize("M,A", ((3, 2), (1024, 7), (4099, 6), (1024 * 1024, 2), (1024 * 1024 + 5, 2)))
def test_launch_counts_and_no_synchronisation(torch, M, A):
    """2 launches forwards up to 2^20 rows, 3 beyond; 1 backwards — counted as the kernel nodes that the calls leave in a stream capture,
    which also shows that they neither synchronise nor allocate."""
    from gym_amd import dqn

    hip = _hip()
    f32 = dict(dtype=torch.float32, device="cuda:0")
    q, nq, on, grad = (torch.zeros((M, A), **f32) for _ in range(4))
    reward, weights, td = (torch.zeros(M, **f32) for _ in range(3))
    act = torch.zeros(M, dtype=torch.int64, device="cuda:0")
    term = torch.zeros(M, dtype=torch.uint8, device="cuda:0")
    ws = torch.empty(dqn.workspace_bytes(M), dtype=torch.uint8, device="cuda:0")
    loss, stats, g = torch.empty((), **f32), torch.empty(8, **f32), torch.ones((), **f32)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = side.cuda_stream
    lib = dqn.lib
    want = 2 if M <= 1024 * 1024 else 3
    assert dqn.launches(M) == dq.launches(M) == want
    ins = (s, M, A, q.data_ptr(), A, act.data_ptr(), 8, None, reward.data_ptr(), term.data_ptr(), nq.data_ptr(), A, on.data_ptr(), A, GAMMA, 1.0,
           weights.data_ptr())
    calls = ((lambda: lib.mxv_dqn_loss(*ins, ws.data_ptr(), ws.numel(), td.data_ptr(), loss.data_ptr(), stats.data_ptr()), want),
             (lambda: lib.mxv_dqn_loss_backward(*ins, g.data_ptr(), grad.data_ptr()), 1))
    for call, _ in calls:                                                     # once outside a capture: the kernels' code is loaded
        assert call() == 0, lib.mxv_dqn_last_error()
    side.synchronize()
    for call, nodes in calls:
        rc, n = _captured_launches(hip, s, call)
        assert (rc, n) == (0, nodes), (rc, n, lib.mxv_dqn_last_error())
    side.synchronize()


# ---- targets from gae on a real chunk --------------------------------------------------------------------------------------------------------------
def test_a_q_that_equals_its_q_lambda_targets_has_no_loss(torch):
    """targets = gae(...)[1] with values = max_a Q on a real DeviceRollout chunk, and q whose taken column equals those targets: the
    loss and every td_error are exactly 0."""
    import gym_amd
    from gym_amd.rollout import DeviceRollout

    r = DeviceRollout("CartPole-v1", 256, seed=1, action_seed=2)
    r.reset(seed=3)
    K, n = 16, r.num_envs
    traj = r.rollout_per_step(K, out=r.trajectory_buffers(K, layout="separate"))
    g = torch.Generator(device="cuda:0").manual_seed(5)
    q = torch.randn((K, n, 2), device="cuda:0", generator=g)
    last = torch.randn(n, device="cuda:0", generator=g)
    targets = r.advantages(traj, q.max(dim=-1).values, last, gamma=0.99, lam=0.65)[1]
    assert int(traj["terminated"].sum() + traj["truncated"].sum()) > 0
    q.scatter_(2, traj["actions"].long().unsqueeze(-1), targets.unsqueeze(-1))
    td = torch.full((K, n), 7.0, device="cuda:0")
    loss, stats = gym_amd.dqn_loss(q, traj["actions"], targets=targets, td_error=td)
    assert float(loss) == 0.0 and bool((td == 0.0).all()) and stats[:2].tolist() == [0.0, 0.0] and float(stats[4]) == 0.0 and float(stats[5]) == 0.0
    assert float(stats[2]) == float(stats[3])
    r.close()


# ---- the example --------------------------------------------------------------------------------------------------------------------------------
def test_the_example_repeats_itself_in_both_target_modes(torch, capsys):
    """examples/pqn_cartpole.py has no torch generator: two runs give the same history, number for number; every diagnostic is finite."""
    import os
    import sys

    from conftest import ROOT

    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import pqn_cartpole
    finally:
        sys.path.pop(0)
    first = pqn_cartpole.train(256, 3, K=8, epochs=2)
    assert f"{3 + 3 * 8} policy steps drawn" in capsys.readouterr().out
    again = pqn_cartpole.train(256, 3, K=8, epochs=2, verbose=False)
    double = pqn_cartpole.train(256, 3, K=8, epochs=2, double=True, verbose=False)
    assert first == again and len(first) == 3 and len(double) == 3
    for row in first + double:
        assert np.isfinite(list(row.values())).all() and row["td_abs_max"] >= row["td_abs_mean"] > 0.0 and row["episodes"] > 0


# ---- the Python front end on the device ----------------------------------------------------------------------------------------------------------
def test_python_argument_errors(torch):
    import gym_amd

    M, A = 16, 3
    f32 = dict(dtype=torch.float32, device="cuda:0")
    q, v = torch.zeros((M, A), **f32), torch.zeros(M, **f32)
    a = torch.zeros(M, dtype=torch.int64, device="cuda:0")
    term = torch.zeros(M, dtype=torch.bool, device="cuda:0")
    boot = dict(reward=v, terminated=term, next_q=q)
    out = (torch.empty((), **f32), torch.empty(8, **f32))
    for kw, what in ((dict(), "exactly one target mode"), (dict(boot, targets=v), "exactly one target mode"),
                     (dict(targets=v, next_q_online=q), "next_q_online is given with targets"), (dict(reward=v, terminated=term), "next_q missing"),
                     (dict(targets=v[:8]), "shape"), (dict(boot, next_q=torch.zeros((M, A + 1), **f32)), "shape"), (dict(targets=v.double()), "float32"),
                     (dict(boot, terminated=v), "uint8"), (dict(targets=v, actions=a.to(torch.int16)), "int64"), (dict(targets=v.cpu()), "device tensor"),
                     (dict(boot, next_q=q.cpu()), "device tensor"), (dict(targets=v, weights=v.cpu()), "device tensor"),
                     (dict(targets=v.clone().requires_grad_()), "must not require grad"), (dict(boot, next_q=q.clone().requires_grad_()), "must not require grad"),
                     (dict(boot, next_q_online=q.clone().requires_grad_()), "must not require grad"),
                     (dict(targets=v, q=q.clone().requires_grad_(), out=out), "requires grad"),
                     (dict(targets=v, q=q.clone().requires_grad_(), workspace=torch.empty(64, dtype=torch.uint8, device="cuda:0")), "requires grad"),
                     (dict(targets=v, workspace=torch.empty(56, dtype=torch.uint8, device="cuda:0")), "workspace holds"),
                     (dict(targets=v, td_error=v), "td_error overlaps the targets"), (dict(targets=v, delta=0.0), "delta"), (dict(boot, gamma=math.nan), "finite")):
        args = dict(q=q, actions=a)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            gym_amd.dqn_loss(args.pop("q"), args.pop("actions"), **args)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="one device"):
            gym_amd.dqn_loss(q, a, targets=v.to("cuda:1"))
