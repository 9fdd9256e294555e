"""gym_amd.soft_q_targets, twin_q_loss and soft_policy_loss on the device against tests/sac_host.py, bit for bit — the targets, the losses,
their diagnostics, td_error and every gradient: every size at which the tree changes shape (a partial wave, a partial workgroup, a
partial leaf, two leaves, the third launch) times every kind of critic count (the two straight-line ones, the loops, the limit), both
target modes, with and without the entropy term, gamma and discount, weights on and off, delta 1 and inf; strided rows, leading dims and
both flag dtypes; the temperature as a number and as a device tensor; one special row among ordinary ones; the cross-checks against
gym_amd.dqn_loss and between the three functions; a real Linear critic pair; the allocation-free forwards recorded in a graph; the
launch counts and the absence of a synchronisation; the example run twice; the front end's refusals."""
import math

import numpy as np
import pytest

import sac_host as sh
from sac_host import bits, to_f32
from test_gpu_ppo import _captured_launches, _hip
from test_sac_host import ALPHA, GAMMA, MODES, kwargs, make_batch

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099)
CRITICS = (1, 2, 3, 5, 64)
GRAD = 2.5
BOOT_KEYS = ("next_log_prob", "alpha", "gamma", "discount")


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


def device_kwargs(torch, kw_h, view=lambda x: x, rows=lambda x: x):
    """The twin's keyword arguments as the device's: vectors through `view`, rows through `rows`, numbers as they are."""
    kw = {}
    for k, v in kw_h.items():
        if v is None or np.isscalar(v):
            kw[k] = v
        else:
            kw[k] = rows(dev(torch, v)) if k == "next_q" else view(dev(torch, v))
    return kw


def check_targets(torch, b, entropy, per_row, *, view=lambda x: x, rows=lambda x: x, what=None):
    import gym_amd

    kw_h = {k: v for k, v in kwargs(b, "bootstrap", entropy, per_row, False, 1.0).items() if k in BOOT_KEYS}
    want = sh.targets_f32(b["next_q"], b["reward"], b["term"], **kw_h)
    y = gym_amd.soft_q_targets(rows(dev(torch, b["next_q"])), view(dev(torch, b["reward"])), view(dev(torch, b["term"])),
                               **device_kwargs(torch, kw_h, view, rows))
    assert not y.requires_grad and tuple(y.shape) == tuple(view(dev(torch, b["reward"])).shape)
    _same32(torch, y, want, (what, "targets", b["q"].shape, entropy, per_row))
    return y


def check_q(torch, b, mode, entropy, per_row, weighted, delta, *, view=lambda x: x, rows=lambda x: x, out_path=True, what=None):
    """One forward and one backward of the critics' loss on the batch `b` against the twin: everything bit for bit.
    -> (stats, td_error, grad) on the host."""
    import gym_amd

    M, C = b["q"].shape
    what = (what, M, C, mode, entropy, per_row, weighted, delta)
    kw_h = kwargs(b, mode, entropy, per_row, weighted, delta)
    want_loss, want_stats, want_td = sh.q_loss_f32(b["q"], **kw_h)
    want_g = sh.q_backward(b["q"], np.float32(GRAD), **kw_h)
    kw_d = device_kwargs(torch, kw_h, view, rows)
    q = rows(dev(torch, b["q"])).requires_grad_()
    td = view(torch.full((M,), 7.0, device="cuda:0"))
    loss, stats = gym_amd.twin_q_loss(q, td_error=td, **kw_d)
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
            got = gym_amd.twin_q_loss(q, out=out, **kw_d)
        assert got[0] is out[0] and got[1] is out[1]
        _same32(torch, out[0], [want_loss], (what, "out loss"))
        _same32(torch, out[1], want_stats, (what, "out stats"))
    return stats.cpu().numpy(), td.cpu().numpy().reshape(-1), q.grad.cpu().numpy().reshape(M, C)


def check_pi(torch, b, weighted, *, alpha=ALPHA, view=lambda x: x, rows=lambda x: x, out_path=True, what=None):
    """One forward and one backward of the actor's loss against the twin -> (stats, grad_log_prob, grad_q) on the host."""
    import gym_amd

    M, C = b["q"].shape
    what = (what, M, C, weighted)
    kw_h = dict(alpha=alpha, weights=b["weights"] if weighted else None)
    want_loss, want_stats = sh.pi_loss_f32(b["log_prob"], b["q"], **kw_h)
    want_lp, want_q = sh.pi_backward(b["log_prob"], b["q"], np.float32(GRAD), **kw_h)
    kw_d = dict(alpha=alpha, weights=view(dev(torch, b["weights"])) if weighted else None)
    q = rows(dev(torch, b["q"])).requires_grad_()
    lp = view(dev(torch, b["log_prob"])).requires_grad_()
    loss, stats = gym_amd.soft_policy_loss(lp, q, **kw_d)
    assert loss.dim() == 0 and loss.requires_grad and tuple(stats.shape) == (8,) and not stats.requires_grad
    _same32(torch, loss, [want_loss], (what, "loss"))
    _same32(torch, stats, want_stats, (what, "stats"))
    (GRAD * loss).backward()
    assert tuple(q.grad.shape) == tuple(q.shape) and tuple(lp.grad.shape) == tuple(lp.shape), what
    _same32(torch, lp.grad, want_lp, (what, "grad_log_prob"))
    _same32(torch, q.grad, want_q, (what, "grad_q"))
    if out_path:
        out = (torch.empty((), device="cuda:0"), torch.empty(8, device="cuda:0"))
        with torch.no_grad():
            got = gym_amd.soft_policy_loss(lp, q, out=out, **kw_d)
        assert got[0] is out[0] and got[1] is out[1]
        _same32(torch, out[0], [want_loss], (what, "out loss"))
        _same32(torch, out[1], want_stats, (what, "out stats"))
    return stats.cpu().numpy(), lp.grad.cpu().numpy().reshape(-1), q.grad.cpu().numpy().reshape(M, C)


# ---- every size, every kind of critic count, every mode -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", SIZES)
def test_targets_losses_stats_td_error_and_gradients_match_the_twin(torch, M):
    for C in CRITICS:
        b = make_batch(M, C, 3000 + M % 1000 + C)
        for mode, entropy, per_row in MODES:
            if mode == "bootstrap":
                check_targets(torch, b, entropy, per_row)
            for weighted in (True, False):
                for delta in (1.0, math.inf):
                    check_q(torch, b, mode, entropy, per_row, weighted, delta, out_path=weighted and delta == 1.0)
        for weighted in (True, False):
            check_pi(torch, b, weighted, out_path=weighted)


def test_the_smallest_batch_that_takes_a_third_launch(torch):
    from gym_amd import sac

    M = 1024 * 1024 + 5
    assert sac.launches(M) == sh.launches(M) == 3 and sac.launches(M - 5) == 2
    b = make_batch(M, 2, 5)
    check_targets(torch, b, True, True)
    check_q(torch, b, "bootstrap", True, True, True, 1.0, out_path=False)
    check_pi(torch, b, True, out_path=False)


# ---- tensor forms -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (2, 5))
def test_strided_rows_leading_dims_and_flag_dtypes(torch, C):
    import gym_amd

    K, N = 3, 87
    M = K * N
    b = make_batch(M, C, 60 + C)

    def wide(x):      # rows of a wider buffer: ld = C + 5
        buf = torch.full((x.shape[0], C + 5), float("nan"), device="cuda:0")
        buf[:, 2:2 + C] = x
        v = buf[:, 2:2 + C]
        assert v.stride(0) == C + 5 and not v.is_contiguous()
        return v

    lead, lead_rows = (lambda x: x.view(K, N)), (lambda x: x.view(K, N, C))
    for mode, entropy, per_row in MODES:
        check_q(torch, b, mode, entropy, per_row, True, 1.0, rows=wide, what="strided")
        check_q(torch, b, mode, entropy, per_row, False, 1.0, view=lead, rows=lead_rows, what="[K, N, C]")
    check_targets(torch, b, True, True, rows=wide, what="strided")
    assert tuple(check_targets(torch, b, True, False, view=lead, rows=lead_rows, what="[K, N, C]").shape) == (K, N)
    check_pi(torch, b, True, rows=wide, what="strided")
    check_pi(torch, b, False, view=lead, rows=lead_rows, what="[K, N, C]")
    # bool and uint8 flags give the same bits
    kw = device_kwargs(torch, kwargs(b, "bootstrap", True, True, False, 1.0))
    q = dev(torch, b["q"])
    l8, s8 = gym_amd.twin_q_loss(q, **kw)
    lb, sb = gym_amd.twin_q_loss(q, **dict(kw, terminated=kw["terminated"].bool()))
    l2, s2 = gym_amd.twin_q_loss(q, **dict(kw, terminated=kw["terminated"] * 200))      # nonzero = set
    assert torch.equal(s8, sb) and torch.equal(l8, lb) and torch.equal(s8, s2) and int(kw["terminated"].sum()) > 0
    tk = {k: v for k, v in kw.items() if k in BOOT_KEYS}
    y8 = gym_amd.soft_q_targets(kw["next_q"], kw["reward"], kw["terminated"], **tk)
    assert torch.equal(y8, gym_amd.soft_q_targets(kw["next_q"], kw["reward"], kw["terminated"].bool(), **tk))


@pytest.mark.parametrize("C", (1, 2, 5))
def test_alpha_as_a_number_and_as_a_device_tensor_give_the_same_bits(torch, C):
    """0.25 is exact in float32: the kernel's widened read of the tensor is the number."""
    import gym_amd

    b = make_batch(777, C, 90 + C)
    kw = device_kwargs(torch, kwargs(b, "bootstrap", True, True, True, 1.0))
    q, lp = dev(torch, b["q"]), dev(torch, b["log_prob"])
    for a_t in (torch.tensor(0.25, device="cuda:0"), torch.tensor([0.25], device="cuda:0")):      # 0-dim and one-element
        tk = {k: v for k, v in kw.items() if k in BOOT_KEYS}
        y_f = gym_amd.soft_q_targets(kw["next_q"], kw["reward"], kw["terminated"], **dict(tk, alpha=0.25))
        y_t = gym_amd.soft_q_targets(kw["next_q"], kw["reward"], kw["terminated"], **dict(tk, alpha=a_t))
        assert torch.equal(y_f, y_t)
        lf, sf = gym_amd.twin_q_loss(q, **dict(kw, alpha=0.25))
        lt, st = gym_amd.twin_q_loss(q, **dict(kw, alpha=a_t))
        assert np.array_equal(host_bits(torch, sf), host_bits(torch, st)) and np.array_equal(host_bits(torch, lf), host_bits(torch, lt))
        pf, psf = gym_amd.soft_policy_loss(lp, q, alpha=0.25, weights=kw["weights"])
        pt, pst = gym_amd.soft_policy_loss(lp, q, alpha=a_t, weights=kw["weights"])
        assert np.array_equal(host_bits(torch, psf), host_bits(torch, pst)) and np.array_equal(host_bits(torch, pf), host_bits(torch, pt))
    # a temperature that is no float32-exact number: the tensor's own value is what the twin gets, and both gradients follow it
    a_t = torch.tensor(0.2, device="cuda:0")
    check_pi(torch, b, True, alpha=float(np.float32(0.2)), out_path=False)
    lp_g, q_g = lp.clone().requires_grad_(), q.clone().requires_grad_()
    loss, stats = gym_amd.soft_policy_loss(lp_g, q_g, alpha=a_t, weights=kw["weights"])
    want_loss, want_stats = sh.pi_loss_f32(b["log_prob"], b["q"], alpha=float(np.float32(0.2)), weights=b["weights"])
    _same32(torch, stats, want_stats, "alpha tensor 0.2")
    (GRAD * loss).backward()
    want_lp, want_q = sh.pi_backward(b["log_prob"], b["q"], np.float32(GRAD), alpha=float(np.float32(0.2)), weights=b["weights"])
    _same32(torch, lp_g.grad, want_lp, "alpha tensor grad_log_prob")
    _same32(torch, q_g.grad, want_q, "alpha tensor grad_q")


# ---- special rows: one among ordinary ones --------------------------------------------------------------------------------------------------------
def _special(C, edit):
    """A batch of 70 ordinary rows, rows 3 and 44 terminated, edited by `edit(batch)`."""
    b = make_batch(70, C, 70 + C)
    b["term"][:] = 0
    b["term"][[3, 44]] = 1
    edit(b)
    return b


@pytest.mark.parametrize("C", (1, 2, 5))
@pytest.mark.parametrize("value", (np.nan, np.inf, -np.inf))
def test_a_non_finite_critic_value_changes_its_row_and_the_sums_and_nothing_else(torch, C, value):
    col = C - 1

    def edit(b):
        b["q"][41, col] = value

    b = _special(C, edit)
    clean = _special(C, lambda b: None)
    for mode in ("targets", "bootstrap"):
        s, td, g = check_q(torch, b, mode, True, True, True, 1.0)
        s0, td0, g0 = check_q(torch, clean, mode, True, True, True, 1.0, out_path=False)
        check_q(torch, b, mode, False, False, False, math.inf, out_path=False)
        others = np.arange(70) != 41
        assert np.array_equal(bits(g[others]), bits(g0[others])) and np.array_equal(bits(td[others]), bits(td0[others]))
        rest = np.ones(C, bool)
        rest[col] = False
        assert np.array_equal(bits(g[41, rest]), bits(g0[41, rest]))      # the other critics of the row keep their gradient
        assert bits(s[3:4])[0] == bits(s0[3:4])[0]                         # the target's mean does not see q
        if np.isnan(value):      # a NaN in one critic column: only that column's gradient is NaN; the extrema skip it
            assert np.isnan(g[41, col]) and np.count_nonzero(np.isnan(g)) == 1 and np.isnan(td[41]) and np.isnan(s[[0, 1, 2, 4]]).all()
            assert np.isfinite(s[[5, 6, 7]]).all() and s[6] == np.delete(b["q"].reshape(-1), 41 * C + col).min()
        else:                    # an infinite error is in the linear zone: +-delta times the weight, an infinite loss
            gs = np.float64(np.float32(GRAD)) / np.float64(70)
            assert g[41, col] == np.float32(gs * (np.float64(b["weights"][41]) * np.sign(value))) and td[41] == value
            assert s[0] == np.inf and s[5] == np.inf and s[6 if value < 0 else 7] == value
    s, g_lp, g_q = check_pi(torch, b, True)
    s0, g_lp0, g_q0 = check_pi(torch, clean, True, out_path=False)
    others = np.arange(70) != 41
    assert np.array_equal(bits(g_q[others]), bits(g_q0[others])) and np.array_equal(bits(g_lp), bits(g_lp0)) and bits(s[1:2])[0] == bits(s0[1:2])[0]
    if np.isnan(value):          # a NaN anywhere in a row of q: the whole row of the actor's gradient
        assert np.isnan(g_q[41]).all() and np.count_nonzero(np.isnan(g_q)) == C and np.all(bits(g_q[41]) == 0x7FC00000)
        assert np.isnan(s[[0, 2, 3]]).all() and np.isfinite(s[[1, 4, 5, 6, 7]]).all()
    else:
        assert np.isfinite(g_q).all()


@pytest.mark.parametrize("C", (1, 2, 5))
def test_terminated_rows_ignore_every_input_of_the_bootstrap_and_running_rows_do_not(torch, C):
    def edit(b):
        b["next_q"][44] = np.nan              # terminated: ignored entirely
        b["next_lp"][44] = np.inf
        b["discount"][44] = np.nan
        b["next_q"][3, C - 1] = -np.inf
        b["next_lp"][3] = np.nan
        b["discount"][3] = np.inf
        b["next_q"][41, C - 1] = np.nan       # running: reaches the target
        b["next_lp"][12] = np.nan

    b = _special(C, edit)
    clean = _special(C, lambda b: None)
    y = check_targets(torch, b, True, True).cpu().numpy()
    y0 = check_targets(torch, clean, True, True).cpu().numpy()
    nan_rows = np.isin(np.arange(70), (12, 41))
    assert np.array_equal(np.isnan(y), nan_rows) and np.array_equal(bits(y[~nan_rows]), bits(y0[~nan_rows]))
    assert np.array_equal(y[[3, 44]], b["reward"][[3, 44]])
    s, td, g = check_q(torch, b, "bootstrap", True, True, True, 1.0)
    assert np.array_equal(np.isnan(g), np.repeat(nan_rows[:, None], C, 1)) and np.isnan(s[[0, 1, 3]]).all() and np.isfinite(s[[2, 4, 5, 6, 7]]).all()
    check_q(torch, b, "bootstrap", True, True, False, math.inf, out_path=False)


@pytest.mark.parametrize("C", (2, 5, 64))
def test_tied_minima_take_the_first(torch, C):
    def edit(b):
        for x in (b["q"], b["next_q"]):
            x[41] = 1.5                          # every critic ties: the first
            x[40, :] = 3.0
            x[40, [C // 2, C - 1]] = -2.0        # two minima: the earlier
            x[39] = 0.0
            x[39, 0] = -0.0                      # -0.0 before +0.0: equal, the first
            x[38] = 0.0
            x[38, C - 1] = -0.0                  # +0.0 before -0.0: equal, the first
            x[37] = np.inf                       # nothing but +inf: the first

    b = _special(C, edit)
    s, g_lp, g_q = check_pi(torch, b, False)
    for row, col in ((41, 0), (40, C // 2), (39, 0), (38, 0), (37, 0)):
        assert g_q[row, col] < 0.0 and np.count_nonzero(g_q[row]) == 1, (row, col, g_q[row])      # the whole gradient, in the first minimum's column
    check_pi(torch, b, True, out_path=False)
    y = check_targets(torch, b, False, False).cpu().numpy()
    assert y[41] == np.float32(np.float64(b["reward"][41]) + GAMMA * 1.5) and y[40] == np.float32(np.float64(b["reward"][40]) + GAMMA * -2.0)
    check_q(torch, b, "bootstrap", True, True, True, 1.0)


def test_td_error_is_the_first_of_equal_errors_and_delta_is_on_the_quadratic_side(torch):
    import gym_amd

    q = np.array([[3.0, -1.0], [-1.0, 3.0], [0.5, 4.0], [1.0, 1.0]], np.float32)
    y = np.array([1.0, 1.0, 2.0, 0.0], np.float32)
    b = dict(q=q, targets=y, weights=np.ones(4, np.float32))
    s, td, g = check_q(torch, b, "targets", False, False, False, 2.0)
    assert td.tolist() == [2.0, -2.0, 2.0, 1.0] and s[0] == (4.0 + 4.0 + 3.125 + 1.0) / 4.0
    gs = np.float64(np.float32(GRAD)) / 4.0
    assert np.array_equal(g, np.array([[2.0, -2.0], [-2.0, 2.0], [-1.5, 2.0], [1.0, 1.0]]) * gs)


# ---- cross-checks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (1, 257, 4099))
@pytest.mark.parametrize("delta", (1.0, math.inf))
def test_one_critic_with_given_targets_has_the_bits_of_dqn_loss(torch, M, delta):
    import gym_amd

    b = make_batch(M, 1, 500 + M)
    q1, q2 = dev(torch, b["q"]).requires_grad_(), dev(torch, b["q"]).requires_grad_()
    y, w = dev(torch, b["targets"]), dev(torch, b["weights"])
    zeros = torch.zeros(M, dtype=torch.int64, device="cuda:0")
    td1, td2 = torch.empty(M, device="cuda:0"), torch.empty(M, device="cuda:0")
    for weights in (None, w):
        q1.grad = q2.grad = None
        l1, s1 = gym_amd.twin_q_loss(q1, targets=y, delta=delta, weights=weights, td_error=td1)
        l2, s2 = gym_amd.dqn_loss(q2, zeros, targets=y, delta=delta, weights=weights, td_error=td2)
        (GRAD * l1).backward()
        (GRAD * l2).backward()
        assert np.array_equal(host_bits(torch, l1), host_bits(torch, l2)) and np.array_equal(host_bits(torch, td1), host_bits(torch, td2))
        assert np.array_equal(host_bits(torch, q1.grad), host_bits(torch, q2.grad))
        keep = [0, 1, 2, 3, 5, 6, 7]      # slot 4 is the critics' gap there and the fraction in the linear zone here
        assert np.array_equal(host_bits(torch, s1)[keep], host_bits(torch, s2)[keep]) and float(s1[4]) == 0.0


@pytest.mark.parametrize("C", (1, 2, 5))
def test_the_loss_on_soft_q_targets_is_the_twin_on_that_path(torch, C):
    import gym_amd

    b = make_batch(1500, C, 600 + C)
    for entropy, per_row in ((True, True), (False, False)):
        y = check_targets(torch, b, entropy, per_row)
        kw_h = {k: v for k, v in kwargs(b, "bootstrap", entropy, per_row, False, 1.0).items() if k in BOOT_KEYS}
        y_h = sh.targets_f32(b["next_q"], b["reward"], b["term"], **kw_h)
        want_loss, want_stats, want_td = sh.q_loss_f32(b["q"], targets=y_h, delta=1.0, weights=b["weights"])
        q = dev(torch, b["q"]).requires_grad_()
        td = torch.empty(1500, device="cuda:0")
        loss, stats = gym_amd.twin_q_loss(q, targets=y, delta=1.0, weights=dev(torch, b["weights"]), td_error=td)
        _same32(torch, loss, [want_loss], "loss on targets")
        _same32(torch, stats, want_stats, "stats on targets")
        _same32(torch, td, want_td, "td on targets")
        (GRAD * loss).backward()
        _same32(torch, q.grad, sh.q_backward(b["q"], np.float32(GRAD), targets=y_h, delta=1.0, weights=b["weights"]), "grad on targets")


def test_the_gradient_through_a_linear_critic_pair_and_cat(torch):
    """loss.backward() through two real torch.nn.Linear critics joined by torch.cat: d loss / d q has the twin's bits, and the critics' own
    gradients are what torch's cat and linear backward make of the twin's grad_q — the same calls on the same bits; an order of float32
    additions of its own is allowed for, M 2^-24 sum |term| per element.  The same for the actor's loss, in both of its inputs."""
    import gym_amd

    M = 257
    b = make_batch(M, 2, 82)
    rng = np.random.default_rng(83)
    obs = dev(torch, rng.standard_normal((M, 4)).astype(np.float32))
    torch.manual_seed(3)
    heads = [torch.nn.Linear(4, 1).to("cuda:0") for _ in range(2)]
    lp_head = torch.nn.Linear(4, 1).to("cuda:0")
    kw_h = kwargs(b, "bootstrap", True, True, True, 1.0)

    def bars(g, x):
        return M * 2.0 ** -24 * (g.abs().t().double() @ x.abs().double()), M * 2.0 ** -24 * g.abs().double().sum(0)

    def run(loss_of, want_of):
        for h in heads + [lp_head]:
            h.zero_grad()
        q = torch.cat([h(obs) for h in heads], dim=1)
        q.retain_grad()
        lp = lp_head(obs).view(-1)
        lp.retain_grad()
        (GRAD * loss_of(lp, q)).backward()
        want_lp, want_q = want_of(lp.detach().cpu().numpy(), q.detach().cpu().numpy())
        assert np.array_equal(host_bits(torch, q.grad), bits(to_f32(want_q)).reshape(-1))
        got = [(h.weight.grad.clone(), h.bias.grad.clone()) for h in heads]
        g = dev(torch, to_f32(want_q))
        for c, h in enumerate(heads):
            h.zero_grad()
            h(obs).backward(gradient=g[:, c:c + 1].contiguous())
            bar_w, bar_b = bars(g[:, c:c + 1], obs)
            assert bool(((got[c][0] - h.weight.grad).abs().double() <= bar_w).all()) and bool(((got[c][1] - h.bias.grad).abs().double() <= bar_b).all())
            assert float(got[c][0].abs().max()) > 0.0
        if want_lp is not None:
            assert np.array_equal(host_bits(torch, lp.grad), bits(to_f32(want_lp)).reshape(-1)) and float(lp_head.weight.grad.abs().max()) > 0.0

    kw_d = device_kwargs(torch, kw_h)
    run(lambda lp, q: gym_amd.twin_q_loss(q, **kw_d)[0], lambda lp, q: (None, sh.q_backward(q, np.float32(GRAD), **kw_h)))
    w = dev(torch, b["weights"])
    run(lambda lp, q: gym_amd.soft_policy_loss(lp, q, alpha=ALPHA, weights=w)[0],
        lambda lp, q: sh.pi_backward(lp, q, np.float32(GRAD), alpha=ALPHA, weights=b["weights"]))
    # only one of the actor's two inputs asks for a gradient: the other gets none, the bits stay
    q, lp = dev(torch, b["q"]), dev(torch, b["log_prob"]).requires_grad_()
    loss, _ = gym_amd.soft_policy_loss(lp, q, alpha=ALPHA)
    loss.backward()
    assert q.grad is None
    _same32(torch, lp.grad, sh.pi_backward(b["log_prob"], b["q"], np.float32(1.0), alpha=ALPHA)[0], "grad_log_prob alone")


def test_no_gradient_is_computed_for_inputs_that_do_not_ask(torch):
    import gym_amd

    b = make_batch(300, 2, 9)
    q, t, lp = dev(torch, b["q"]), dev(torch, b["targets"]), dev(torch, b["log_prob"])
    loss, stats = gym_amd.twin_q_loss(q, targets=t)
    pl, ps = gym_amd.soft_policy_loss(lp, q, alpha=ALPHA)
    assert not loss.requires_grad and not stats.requires_grad and not pl.requires_grad and not ps.requires_grad
    with torch.no_grad():
        loss2, _ = gym_amd.twin_q_loss(q.clone().requires_grad_(), targets=t)
        pl2, _ = gym_amd.soft_policy_loss(lp.clone().requires_grad_(), q.clone().requires_grad_(), alpha=ALPHA)
    assert not loss2.requires_grad and torch.equal(loss, loss2) and not pl2.requires_grad and torch.equal(pl, pl2)
    # the targets carry no graph, whatever their inputs ask for
    y = gym_amd.soft_q_targets(q.clone().requires_grad_(), dev(torch, b["reward"]), dev(torch, b["term"]), gamma=GAMMA)
    assert not y.requires_grad


# ---- graph capture, launch counts, no synchronisation ------------------------------------------------------------------------------------------
def test_the_allocation_free_calls_replay_in_a_captured_graph(torch):
    import gym_amd
    from gym_amd import sac

    M, C = 5000, 2
    batches = [make_batch(M, C, 40 + k) for k in range(3)]
    keys = ("q", "reward", "term", "next_q", "next_lp", "discount", "weights", "log_prob")
    bufs = {k: dev(torch, batches[0][k]) for k in keys}
    alpha = torch.tensor(0.25, device="cuda:0")
    ws_q, ws_pi = (torch.empty(sac.workspace_bytes(M), dtype=torch.uint8, device="cuda:0") for _ in range(2))
    out_q, out_pi = ((torch.empty((), device="cuda:0"), torch.empty(8, device="cuda:0")) for _ in range(2))
    td, y = torch.empty(M, device="cuda:0"), torch.empty(M, device="cuda:0")

    def step():
        gym_amd.soft_q_targets(bufs["next_q"], bufs["reward"], bufs["term"], next_log_prob=bufs["next_lp"], alpha=alpha, discount=bufs["discount"], out=y)
        gym_amd.twin_q_loss(bufs["q"], reward=bufs["reward"], terminated=bufs["term"], next_q=bufs["next_q"], next_log_prob=bufs["next_lp"], alpha=alpha,
                            discount=bufs["discount"], delta=1.0, weights=bufs["weights"], td_error=td, workspace=ws_q, out=out_q)
        gym_amd.soft_policy_loss(bufs["log_prob"], bufs["q"], alpha=alpha, weights=bufs["weights"], workspace=ws_pi, out=out_pi)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                # warm-up outside the capture
        side.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        step()
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before      # with out= and workspace= the calls allocate nothing
        eager = [x.clone() for x in (y, td) + out_q + out_pi]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            step()
        g.replay()
        side.synchronize()
        for have, want in zip((y, td) + out_q + out_pi, eager):
            assert np.array_equal(host_bits(torch, have), host_bits(torch, want))      # the replay has the eager call's bits
        for k in (1, 2):
            for name in keys:
                bufs[name].copy_(dev(torch, batches[k][name]))
            alpha.fill_(0.25 * k)                                                 # the kernel reads the temperature at every replay
            g.replay()
            side.synchronize()
            bk = batches[k]
            boot = dict(next_log_prob=bk["next_lp"], alpha=0.25 * k, discount=bk["discount"])
            _same32(torch, y, sh.targets_f32(bk["next_q"], bk["reward"], bk["term"], **boot), k)
            want_loss, want_stats, want_td = sh.q_loss_f32(bk["q"], reward=bk["reward"], terminated=bk["term"], next_q=bk["next_q"], delta=1.0,
                                                           weights=bk["weights"], **boot)
            _same32(torch, out_q[0], [want_loss], k)
            _same32(torch, out_q[1], want_stats, k)
            _same32(torch, td, want_td, k)
            want_loss, want_stats = sh.pi_loss_f32(bk["log_prob"], bk["q"], alpha=0.25 * k, weights=bk["weights"])
            _same32(torch, out_pi[0], [want_loss], k)
            _same32(torch, out_pi[1], want_stats, k)
    torch.cuda.current_stream().wait_stream(side)


@pytest.mark.parametrize("M,C", ((3, 2), (1024, 5), (4099, 1), (1024 * 1024, 2), (1024 * 1024 + 5, 2)))
def test_launch_counts_and_no_synchronisation(torch, M, C):
    """The target 1 launch; the losses 2 launches forwards up to 2^20 rows, 3 beyond, and 1 backwards: a critic update is 3 launches, an
    actor update 3 — counted as the kernel nodes that the calls leave in a stream capture, which also shows that they neither
    synchronise nor allocate."""
    from gym_amd import sac

    hip = _hip()
    f32 = dict(dtype=torch.float32, device="cuda:0")
    q, nq, grad = (torch.zeros((M, C), **f32) for _ in range(3))
    reward, weights, td, lp, nlp, disc, y, grad_lp = (torch.zeros(M, **f32) for _ in range(8))
    term = torch.zeros(M, dtype=torch.uint8, device="cuda:0")
    ws = torch.empty(sac.workspace_bytes(M), dtype=torch.uint8, device="cuda:0")
    loss, stats, g, alpha = torch.empty((), **f32), torch.empty(8, **f32), torch.ones((), **f32), torch.ones((), **f32)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = side.cuda_stream
    lib = sac.lib
    want = 2 if M <= 1024 * 1024 else 3
    assert sac.launches(M) == sh.launches(M) == want
    ins = (s, M, C, q.data_ptr(), C, None, reward.data_ptr(), term.data_ptr(), nq.data_ptr(), C, nlp.data_ptr(), 0.0, alpha.data_ptr(), GAMMA,
           disc.data_ptr(), 1.0, weights.data_ptr())
    pins = (s, M, C, lp.data_ptr(), q.data_ptr(), C, 0.0, alpha.data_ptr(), weights.data_ptr())
    calls = ((lambda: lib.mxv_sac_targets(s, M, C, nq.data_ptr(), C, reward.data_ptr(), term.data_ptr(), nlp.data_ptr(), 0.0, alpha.data_ptr(), GAMMA,
                                          disc.data_ptr(), y.data_ptr()), 1),
             (lambda: lib.mxv_sac_loss(*ins, ws.data_ptr(), ws.numel(), td.data_ptr(), loss.data_ptr(), stats.data_ptr()), want),
             (lambda: lib.mxv_sac_loss_backward(*ins, g.data_ptr(), grad.data_ptr()), 1),
             (lambda: lib.mxv_sac_policy_loss(*pins, ws.data_ptr(), ws.numel(), loss.data_ptr(), stats.data_ptr()), want),
             (lambda: lib.mxv_sac_policy_loss_backward(*pins, g.data_ptr(), grad_lp.data_ptr(), grad.data_ptr()), 1))
    for call, _ in calls:                                                     # once outside a capture: the kernels' code is loaded
        assert call() == 0, lib.mxv_sac_last_error()
    side.synchronize()
    for call, nodes in calls:
        rc, n = _captured_launches(hip, s, call)
        assert (rc, n) == (0, nodes), (rc, n, lib.mxv_sac_last_error())
    side.synchronize()


# ---- the example --------------------------------------------------------------------------------------------------------------------------------
def test_the_fused_example_repeats_itself(torch, capsys):
    """examples/sac_pendulum_fused.py has no torch generator: two runs give the same history, number for number; every diagnostic is finite."""
    import os
    import sys

    from conftest import ROOT

    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import sac_pendulum_fused
    finally:
        sys.path.pop(0)
    first = sac_pendulum_fused.train(256, 3, K=8, batch=512, updates=2)
    assert "action draws made" in capsys.readouterr().out
    again = sac_pendulum_fused.train(256, 3, K=8, batch=512, updates=2, verbose=False)
    assert first == again and len(first) == 3
    for row in first:
        assert np.isfinite(list(row.values())).all() and row["td_abs_max"] >= row["td_abs_mean"] > 0.0 and row["critic_gap"] >= 0.0
        assert 0.0 <= row["later_critic_fraction"] <= 1.0 and row["q_min"] <= row["q_mean"] <= row["q_max"] and row["alpha"] > 0.0


# ---- the Python front end on the device ----------------------------------------------------------------------------------------------------------
def test_python_argument_errors(torch):
    import gym_amd

    M, C = 16, 2
    f32 = dict(dtype=torch.float32, device="cuda:0")
    q, v = torch.zeros((M, C), **f32), torch.zeros(M, **f32)
    term = torch.zeros(M, dtype=torch.bool, device="cuda:0")
    boot = dict(reward=v, terminated=term, next_q=q)
    out = (torch.empty((), **f32), torch.empty(8, **f32))
    ws = torch.empty(64, dtype=torch.uint8, device="cuda:0")
    a_t = torch.tensor(0.2, **f32)
    for kw, what in ((dict(), "exactly one target mode"), (dict(boot, targets=v), "exactly one target mode"),
                     (dict(targets=v, discount=v), "discount is given with targets"), (dict(targets=v, alpha=0.2), "alpha is given with targets"),
                     (dict(targets=v, next_log_prob=v), "next_log_prob is given with targets"), (dict(reward=v, terminated=term), "next_q missing"),
                     (dict(boot, gamma=0.99, discount=v), "gamma and discount are both given"), (dict(boot, alpha=0.2), "alpha is given without next_log_prob"),
                     (dict(boot, next_log_prob=v), "next_log_prob is given without alpha"), (dict(targets=v[:8]), "shape"),
                     (dict(boot, next_q=torch.zeros((M, C + 1), **f32)), "shape"), (dict(boot, next_log_prob=v[:8], alpha=0.2), "shape"),
                     (dict(q=torch.zeros((M, 0), **f32), targets=v), "1 <= C <= 64"), (dict(q=torch.zeros((M, 65), **f32), targets=v), "1 <= C <= 64"),
                     (dict(q=torch.zeros(M, **f32), targets=v), "shape"), (dict(targets=v.double()), "float32"), (dict(q=q.double(), targets=v), "float32"),
                     (dict(boot, terminated=v), "uint8"), (dict(boot, discount=v.double()), "float32"), (dict(targets=v.cpu()), "device tensor"),
                     (dict(boot, next_q=q.cpu()), "device tensor"), (dict(targets=v, weights=v.cpu()), "device tensor"),
                     (dict(boot, next_log_prob=v, alpha=a_t.cpu()), "device tensor"), (dict(boot, next_log_prob=v, alpha=a_t.double()), "alpha tensor"),
                     (dict(boot, next_log_prob=v, alpha=torch.zeros(2, **f32)), "alpha tensor"), (dict(boot, next_log_prob=v, alpha=math.nan), "finite"),
                     (dict(boot, next_log_prob=v, alpha=a_t.clone().requires_grad_()), "alpha must not require grad"),
                     (dict(targets=v.clone().requires_grad_()), "must not require grad"), (dict(boot, next_q=q.clone().requires_grad_()), "must not require grad"),
                     (dict(boot, next_log_prob=v.clone().requires_grad_(), alpha=0.2), "must not require grad"),
                     (dict(targets=v, weights=v.clone().requires_grad_()), "must not require grad"),
                     (dict(targets=v, q=q.clone().requires_grad_(), out=out), "requires grad"),
                     (dict(targets=v, q=q.clone().requires_grad_(), workspace=ws), "requires grad"),
                     (dict(targets=v, workspace=torch.empty(56, dtype=torch.uint8, device="cuda:0")), "workspace holds"),
                     (dict(targets=v, out=out[:1]), "2 entries"), (dict(targets=v, td_error=v), "td_error overlaps the targets"),
                     (dict(targets=v, delta=0.0), "delta"), (dict(boot, gamma=math.nan), "finite")):
        args = dict(q=q)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            gym_amd.twin_q_loss(args.pop("q"), **args)
    for kw, what in ((dict(alpha=None), "alpha is required"), (dict(log_prob=v[:8]), "shape"), (dict(log_prob=v.double()), "float32"),
                     (dict(q=torch.zeros((M, 65), **f32)), "1 <= C <= 64"), (dict(q=torch.zeros((M, 0), **f32)), "1 <= C <= 64"), (dict(q=q.cpu()), "device tensor"),
                     (dict(weights=v.cpu()), "device tensor"), (dict(weights=v[:3]), "shape"), (dict(alpha="0.2"), "finite"), (dict(alpha=math.inf), "finite"),
                     (dict(alpha=a_t.clone().requires_grad_()), "alpha must not require grad"), (dict(alpha=a_t.cpu()), "device tensor"),
                     (dict(weights=v.clone().requires_grad_()), "must not require grad"), (dict(log_prob=v.clone().requires_grad_(), out=out), "requires grad"),
                     (dict(q=q.clone().requires_grad_(), workspace=ws), "requires grad"), (dict(out=(out[1], out[1])), "shape"),
                     (dict(workspace=torch.empty(8, dtype=torch.uint8, device="cuda:0")), "workspace holds"), (dict(out=(v[0], out[1]), log_prob=v), "overlaps")):
        args = dict(log_prob=v, q=q, alpha=0.2)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            gym_amd.soft_policy_loss(args.pop("log_prob"), args.pop("q"), **args)
    for kw, what in ((dict(alpha=0.2), "alpha is given without next_log_prob"), (dict(next_log_prob=v), "next_log_prob is given without alpha"),
                     (dict(gamma=0.9, discount=v), "gamma and discount are both given"), (dict(reward=v[:8]), "shape"), (dict(terminated=v), "uint8"),
                     (dict(next_q=torch.zeros((M, 65), **f32)), "1 <= C <= 64"), (dict(next_q=q.cpu()), "device tensor"), (dict(discount=v.cpu()), "device tensor"),
                     (dict(out=torch.zeros(M - 1, **f32)), "shape"), (dict(out=v.clone().requires_grad_()), "out must not require grad"),
                     (dict(out=v), "targets_out overlaps the reward"), (dict(gamma=math.inf), "finite"), (dict(reward=None), "reward"),
                     (dict(next_log_prob=v, alpha=torch.zeros((1, 1), **f32)), "alpha tensor")):
        args = dict(next_q=q, reward=v, terminated=term)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            gym_amd.soft_q_targets(args.pop("next_q"), args.pop("reward"), args.pop("terminated"), **args)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="one device"):
            gym_amd.twin_q_loss(q, targets=v.to("cuda:1"))
