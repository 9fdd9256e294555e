"""gym_amd.rsample_squashed_gaussian / SquashedGaussianSampler on the device against tests/squashed_host.py, bit for bit — the action
bits, the bits of log_prob and the bits of both gradients: every D, shape class, offset and step, 2048 * 256 + 257 rows (the tile loop
strides), strided views with guarded outputs, absent outputs and gradients, degenerate and extreme rows, loss.backward() against the
backward entry point, agreement with torch.distributions, the device step counter under graph replay with step_used, checkpoints, and
the samplers of the two Box envs end to end."""
import numpy as np
import pytest

import squashed_host as sh
from squashed_host import bits

pytestmark = pytest.mark.gpu

GUARD_F32 = 0x7FABCDEF      # a NaN pattern no computation produces (NaN results are written as 0x7FC00000)
SIZES = (1, 3, 63, 64, 65, 255, 257, 4099)
DIMS = (1, 2, 3, 4)
OFFSETS = (0, 1, 6)
STEPS = (0, 5, 2 ** 32 + 1)
SEED = 2 ** 63 + 17
SCALE = np.asarray([2.0, 1.0, 0.375, 64.0], np.float32)
BIAS = np.asarray([0.0, -0.5, 3.0, 100.0], np.float32)


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host_bits(torch, x):
    return x.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _head(rng, N, D):
    """Means of scale 0.1 / 1 / 10 and log_std over [-5, 2]."""
    mean = (rng.standard_normal((N, D)) * rng.choice([0.1, 1.0, 10.0], size=(N, 1))).astype(np.float32)
    return mean, rng.uniform(-5.0, 2.0, (N, D)).astype(np.float32)


def _grads(rng, N, D):
    return rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal(N).astype(np.float32)


def _same(torch, got, want, what):
    assert tuple(got.shape) == want.shape and np.array_equal(host_bits(torch, got), bits(want)), what


def _forward(torch, md, lsd, *, seed, step, env_offset, scale=None, bias=None, out=None, step_used=None):
    """mxv_squashed_sample through the module's binding, with every pointer the test wants to control."""
    from gym_amd import squashed

    N, D = md.shape
    af = squashed._affine(D, None, None, scale, bias)
    act, lp = (torch.empty((N, D), device="cuda:0"), torch.empty(N, device="cuda:0")) if out is None else out
    step_t = step if isinstance(step, torch.Tensor) else None
    squashed._forward(torch, md, lsd, af, seed, env_offset, 0 if step_t is not None else step, step_t, step_used, act, lp)
    return act, lp


def _backward(torch, md, lsd, *, seed, step, env_offset, scale=None, ga=None, glp=None, need=(True, True)):
    from gym_amd import squashed

    N, D = md.shape
    af = squashed._affine(D, None, None, scale, None)
    gm = torch.empty((N, D), device="cuda:0") if need[0] else None
    gs = torch.empty((N, D), device="cuda:0") if need[1] else None
    step_t = step if isinstance(step, torch.Tensor) else None
    squashed._backward(torch, md, lsd, af, seed, env_offset, 0 if step_t is not None else step, step_t, ga, glp, gm, gs)
    return gm, gs


@pytest.mark.parametrize("D", DIMS)
def test_every_shape_offset_and_step_matches_the_twin(torch, D):
    import gym_amd

    rng = np.random.default_rng(7 + D)
    case = 0
    for N in SIZES:
        mean, ls = _head(rng, N, D)
        ga, glp = _grads(rng, N, D)
        md, lsd, ls1d, gad, glpd = dev(torch, mean), dev(torch, ls), dev(torch, ls[0]), dev(torch, ga), dev(torch, glp)
        for off in OFFSETS:
            for step in STEPS:
                shared, affine = case % 2 == 1, case % 3 != 0                # alternate log_std [N, D] and [D]; with and without scale / bias
                case += 1
                kw = dict(scale=SCALE[:D], bias=BIAS[:D]) if affine else {}
                ls_ref, ls_arg = (ls[0], ls1d) if shared else (ls, lsd)
                what = (N, D, off, step, shared, affine)
                act, lp = gym_amd.rsample_squashed_gaussian(md, ls_arg, seed=SEED, step=step, env_offset=off, **kw)
                assert act.dtype == lp.dtype == torch.float32
                want = sh.sample(mean, ls_ref, seed=SEED, step=step, env_offset=off, **kw)
                _same(torch, act, want[0], what)
                _same(torch, lp, want[1], what)
                gm, gs = _backward(torch, md, ls_arg, seed=SEED, step=step, env_offset=off, scale=kw.get("scale"), ga=gad, glp=glpd)
                wm, ws = sh.sample_backward(mean, ls_ref, seed=SEED, step=step, env_offset=off, scale=kw.get("scale"), grad_actions=ga,
                                            grad_log_prob=glp)
                _same(torch, gm, wm, what)
                _same(torch, gs, ws, what)


def _guarded(torch, shape, lead, tail=5):
    """A contiguous tensor of `shape` inside a guard-filled parent, `lead` elements in; -> (view, parent)."""
    n = int(np.prod(shape))
    parent = torch.empty(n + lead + tail, dtype=torch.float32, device="cuda:0")
    parent.view(torch.int32).fill_(GUARD_F32)
    return parent[lead:lead + n].view(shape), parent


def _guard_bits(torch, t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _gaps_hold(torch, parent, lead, N, ld, off, D, what):
    """The cells of a guarded [N, ld] parent outside the columns off .. off + D still hold the guard."""
    wide = _guard_bits(torch, parent)
    gaps = np.ones((N, ld), bool)
    gaps[:, off:off + D] = False
    assert np.all(wide[:lead] == GUARD_F32) and np.all(wide[lead + N * ld:] == GUARD_F32), what
    assert np.all(wide[lead:lead + N * ld].reshape(N, ld)[gaps] == GUARD_F32), what


@pytest.mark.parametrize("D", DIMS)
def test_views_of_wider_buffers_guarded_outputs_and_absent_arguments(torch, D):
    rng = np.random.default_rng(40 + D)
    N = 259
    for k, off in enumerate((1, 2, 4)):
        ld_m, ld_s, ld_a = D + 5 + off, D + 2 + off, D + 3 + off
        wide_m = rng.standard_normal((N, ld_m)).astype(np.float32)
        wide_s = rng.uniform(-3.0, 1.0, (N, ld_s)).astype(np.float32)
        wide_g = rng.standard_normal((N, ld_a)).astype(np.float32)
        glp = rng.standard_normal(N).astype(np.float32)
        wm, ws, wg, glpd = dev(torch, wide_m), dev(torch, wide_s), dev(torch, wide_g), dev(torch, glp)
        md, sd, gad = wm[:, off:off + D], ws[:, 1:1 + D], wg[:, off:off + D]
        assert md.stride(0) == ld_m and md.data_ptr() == wm.data_ptr() + 4 * off
        mean, ls, ga = wide_m[:, off:off + D], wide_s[:, 1:1 + D], wide_g[:, off:off + D]
        shared = k == 1
        ls_arg, ls_ref = (sd[0], ls[0]) if shared else (sd, ls)
        kw = dict(seed=5, step=9, env_offset=off)
        sc = SCALE[:D] if k else None
        want = sh.sample(mean, ls_ref, scale=sc, bias=BIAS[:D] if k else None, **kw)
        wa, pa = _guarded(torch, (N, ld_a), 3)                              # the actions: a strided view into a guarded wide buffer
        a = wa[:, off:off + D]
        lp, plp = _guarded(torch, (N,), 1)
        for with_lp in (True, False):
            pa.view(torch.int32).fill_(GUARD_F32)
            plp.view(torch.int32).fill_(GUARD_F32)
            _forward(torch, md, ls_arg, scale=sc, bias=BIAS[:D] if k else None, out=(a, lp if with_lp else None), **kw)
            _same(torch, a, want[0], (D, off, with_lp))
            _gaps_hold(torch, pa, 3, N, ld_a, off, D, (D, off, with_lp, "actions"))
            p = _guard_bits(torch, plp)
            if with_lp:
                _same(torch, lp, want[1], (D, off))
                assert np.all(p[:1] == GUARD_F32) and np.all(p[1 + N:] == GUARD_F32), (D, off)
            else:
                assert np.all(p == GUARD_F32), (D, off)                     # an omitted output is not written at all
        # the backward: strided gradient rows in and out, each of grad_actions, grad_log_prob and one output absent
        for ga_on, glp_on, need in ((True, True, (True, True)), (False, True, (True, True)), (True, False, (True, True)),
                                    (True, True, (True, False)), (True, True, (False, True))):
            (wgm, pgm), (wgs, pgs) = _guarded(torch, (N, ld_a), 2), _guarded(torch, (N, ld_a), 4)
            from gym_amd import squashed

            af = squashed._affine(D, None, None, sc, None)
            gm, gs = (wgm[:, off:off + D] if need[0] else None), (wgs[:, off:off + D] if need[1] else None)
            with torch.cuda.device(0):
                squashed._check(squashed.lib.mxv_squashed_sample_backward(
                    torch.cuda.current_stream().cuda_stream, N, D, md.data_ptr(), ld_m, ls_arg.data_ptr(), 0 if shared else ld_s, af[0], af[1], 5, off, 9,
                    None, gad.data_ptr() if ga_on else None, ld_a, glpd.data_ptr() if glp_on else None, None if gm is None else gm.data_ptr(), ld_a,
                    None if gs is None else gs.data_ptr(), ld_a))
            wmn, wsn = sh.sample_backward(mean, ls_ref, scale=sc, grad_actions=ga if ga_on else None, grad_log_prob=glp if glp_on else None, **kw)
            what = (D, off, ga_on, glp_on, need)
            for g, w, parent, lead in ((gm, wmn, pgm, 2), (gs, wsn, pgs, 4)):
                if g is None:
                    assert np.all(_guard_bits(torch, parent) == GUARD_F32), what
                else:
                    _same(torch, g, w, what)
                    _gaps_hold(torch, parent, lead, N, ld_a, off, D, what)
            if not ga_on:                                                   # absent means zeros, bit for bit
                zm, zs = sh.sample_backward(mean, ls_ref, scale=sc, grad_actions=np.zeros_like(ga), grad_log_prob=glp, **kw)
                assert np.array_equal(bits(zm), bits(wmn)) and np.array_equal(bits(zs), bits(wsn))
        assert torch.equal(wm.cpu(), torch.from_numpy(wide_m)) and torch.equal(ws.cpu(), torch.from_numpy(wide_s))      # inputs are read only
        assert torch.equal(wg.cpu(), torch.from_numpy(wide_g))


# kMaxBlocks * kThreads + 257 rows: the tile loops stride (every smaller N above gives each workgroup one tile); workgroup 0 takes a
# second, full tile (rows 524 288 ..) and workgroup 1 a second tile of one row
STRIDING = 2048 * 256 + 257


@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("D", (1, 4))                                       # the narrowest and the widest instantiation
def test_above_2048_tiles_every_workgroup_takes_a_second_tile(torch, D, shared):
    N = STRIDING
    rng = np.random.default_rng(1400 + D)
    mean, ls = _head(rng, N, D)
    ga, glp = _grads(rng, N, D)
    ls_ref = ls[0] if shared else ls
    (a, pa), (lp, plp) = _guarded(torch, (N, D), 3), _guarded(torch, (N,), 1)
    off, step = ((6, 5), (0, 2 ** 32 + 1))[shared]
    md, lsd = dev(torch, mean), dev(torch, ls_ref)
    _forward(torch, md, lsd, seed=SEED, step=step, env_offset=off, scale=SCALE[:D], bias=BIAS[:D], out=(a, lp))
    want = sh.sample(mean, ls_ref, seed=SEED, step=step, env_offset=off, scale=SCALE[:D], bias=BIAS[:D])
    _same(torch, a, want[0], (N, D, shared))
    _same(torch, lp, want[1], (N, D, shared))
    for parent, lead, n, name in ((pa, 3, N * D, "actions"), (plp, 1, N, "log_prob")):
        p = _guard_bits(torch, parent)
        assert np.all(p[:lead] == GUARD_F32) and np.all(p[lead + n:] == GUARD_F32), (D, shared, name)      # behind row N - 1 too
    gm, gs = _backward(torch, md, lsd, seed=SEED, step=step, env_offset=off, scale=SCALE[:D], ga=dev(torch, ga), glp=dev(torch, glp))
    wm, ws = sh.sample_backward(mean, ls_ref, seed=SEED, step=step, env_offset=off, scale=SCALE[:D], grad_actions=ga, grad_log_prob=glp)
    _same(torch, gm, wm, (N, D, shared))
    _same(torch, gs, ws, (N, D, shared))


def test_overlapping_outputs_raise(torch):
    N, D = 40, 2
    wide = torch.zeros((N, 8), device="cuda:0")
    mean, ls = wide[:, 0:2], torch.zeros(D, device="cuda:0")
    other = torch.zeros((N, D), device="cuda:0")
    flat = torch.zeros(3 * N, device="cuda:0")
    kw = dict(seed=0, step=0, env_offset=0)
    with pytest.raises(ValueError, match="actions overlaps the mean"):
        _forward(torch, mean, ls, out=(wide[:, 4:6], None), **kw)          # interleaved with the mean's rows
    with pytest.raises(ValueError, match="log_prob overlaps the mean"):
        _forward(torch, mean, ls, out=(other, wide.view(-1)[3:3 + N]), **kw)
    with pytest.raises(ValueError, match="outputs actions and log_prob overlap"):
        _forward(torch, mean, ls, out=(flat[:2 * N].view(N, D), flat[2 * N - 1:3 * N - 1]), **kw)
    buf = torch.zeros(N + 8, device="cuda:0")                              # a counter inside the log_prob buffer
    counter = buf.view(torch.int64)[2:3]
    with pytest.raises(ValueError, match="log_prob overlaps step_dev"):
        _forward(torch, mean, ls, seed=0, step=counter, env_offset=0, out=(other, buf[:N]))
    with pytest.raises(ValueError, match="step_used overlaps step_dev"):
        _forward(torch, mean, ls, seed=0, step=counter, env_offset=0, step_used=counter)
    with pytest.raises(ValueError, match="grad_mean overlaps the mean"):
        from gym_amd import squashed

        squashed._backward(torch, mean, ls, squashed._affine(D, None, None, None, None), 0, 0, 0, None, None, other.view(-1)[:N], wide[:, 1:3], None)
    with pytest.raises(ValueError, match="out .actions."):
        from gym_amd import SquashedGaussianSampler

        SquashedGaussianSampler(D, low=-1, high=1).sample(mean, ls, out=(torch.zeros((N, D + 1), device="cuda:0"), None))
    torch.cuda.synchronize()
    assert int(counter.item()) == 0 and float(other.abs().sum()) == 0.0     # refused before anything was launched


@pytest.mark.parametrize("D", (1, 2, 4))
def test_degenerate_and_extreme_rows(torch, D):
    inf, nan = np.inf, np.nan
    rng = np.random.default_rng(60 + D)
    mean, ls = [], []

    def add(mv=None, sv=None, at=0):
        m, s = rng.standard_normal(D), rng.uniform(-2, 1, D)
        if mv is not None:
            m[at] = mv
        if sv is not None:
            s[at] = sv
        mean.append(m)
        ls.append(s)

    for at in range(D):
        for mv in (nan, inf, -inf):
            add(mv=mv, at=at)
            add()                                                            # a good row between the bad ones
        for sv in (nan, 80.0001, -80.0001, inf, -inf):
            add(sv=sv, at=at)
            add()
    n_marked = len(mean)
    top = float(np.finfo(np.float32).max)
    for at in range(D):
        for sv in (80.0, -80.0):
            add(sv=sv, at=at)
        for mv in (1e30, -1e30, top, -top, 0.0, 1e-45, 354.0, -354.5, 400.0, -1000.0):      # at and past the cut of E
            add(mv=mv, sv=-80.0, at=at)
        for mv in (2.0 ** -27, -2.0 ** -28, 2.0 ** -40, 1e-38, 0.0):          # |u| below the switch: sigma = EXP(-80) adds 1.8e-35 |z|
            add(mv=mv, sv=-80.0, at=at)
    add(mv=top, sv=80.0)
    mean, ls = np.asarray(mean, np.float32), np.asarray(ls, np.float32)
    rows = len(mean)
    n_reps = 16                                                             # each row at 16 rows: other normals, some of them large
    mean, ls = np.tile(mean, (n_reps, 1)), np.tile(ls, (n_reps, 1))
    N = len(mean)
    ga, glp = _grads(rng, N, D)
    md, lsd = dev(torch, mean), dev(torch, ls)
    kw = dict(seed=8, step=2, env_offset=3)
    got = _forward(torch, md, lsd, scale=SCALE[:D], bias=BIAS[:D], **kw)
    want = sh.sample(mean, ls, scale=SCALE[:D], bias=BIAS[:D], **kw)
    gm, gs = _backward(torch, md, lsd, scale=SCALE[:D], ga=dev(torch, ga), glp=dev(torch, glp), **kw)
    wm, ws = sh.sample_backward(mean, ls, scale=SCALE[:D], grad_actions=ga, grad_log_prob=glp, **kw)
    for g, w in zip(got + (gm, gs), want + (wm, ws)):
        _same(torch, g, w, D)
    bad = np.tile((np.arange(rows) < n_marked) & (np.arange(rows) % 2 == 0), n_reps)
    for x in got + (gm, gs):
        b, v = host_bits(torch, x), x.cpu().numpy()
        assert np.all(b[bad] == 0x7FC00000) and not np.isnan(v[~bad]).any()      # NaN in every output and gradient of a bad row, nowhere else
    a = got[0].cpu().numpy()
    lo, hi = (BIAS[:D].astype(np.float64) - SCALE[:D]).astype(np.float32), (BIAS[:D].astype(np.float64) + SCALE[:D]).astype(np.float32)
    assert np.all((a[~bad] >= lo) & (a[~bad] <= hi))
    r = sh.evaluate(mean, ls, sh.words(8, 3 + np.arange(N, dtype=np.uint64), 2), SCALE[:D], BIAS[:D])
    good = ~bad[:, None] & np.ones((1, D), bool)
    assert (good & (r["e"] == 0)).any() and (good & (r["v"] < 2.0 ** -27)).any() and (good & (r["v"] == 354.0)).any()
    sat = good & (r["e"] == 0)
    assert np.array_equal(a[sat], np.where(r["u"] > 0, hi, lo)[sat])        # past the cut the action is the end of the interval, exactly
    lpv = got[1].cpu().numpy()
    assert np.isposinf(lpv[~bad]).any() and np.isfinite(lpv[~bad]).any()    # the density of a saturated action past float32's range: +Inf, no NaN


def test_backward_through_autograd_equals_the_entry_point(torch):
    import gym_amd

    rng = np.random.default_rng(123)
    K, N, D = 3, 70, 3
    mean, ls = _head(rng, K * N, D)
    ga, glp = _grads(rng, K * N, D)
    kw = dict(seed=77, step=4, env_offset=9)
    gad, glpd = dev(torch, ga).view(K, N, D), dev(torch, glp).view(K, N)
    want_m, want_s = sh.sample_backward(mean, ls, scale=SCALE[:D], grad_actions=ga, grad_log_prob=glp, **kw)
    # [K, N, D] inputs and a per-row log_std
    m3 = dev(torch, mean).view(K, N, D).requires_grad_()
    s3 = dev(torch, ls).view(K, N, D).requires_grad_()
    act, lp = gym_amd.rsample_squashed_gaussian(m3, s3, scale=SCALE[:D], bias=BIAS[:D], **kw)
    assert tuple(act.shape) == (K, N, D) and tuple(lp.shape) == (K, N) and act.requires_grad and lp.requires_grad
    wa, wl = sh.sample(mean, ls, scale=SCALE[:D], bias=BIAS[:D], **kw)
    _same(torch, act.detach().view(-1, D), wa, "actions")
    _same(torch, lp.detach().view(-1), wl, "log_prob")
    ((act * gad).sum() + (lp * glpd).sum()).backward()
    _same(torch, m3.grad.view(-1, D), want_m, "grad_mean")
    _same(torch, s3.grad.view(-1, D), want_s, "grad_log_std")
    gm, gs = _backward(torch, m3.detach().view(-1, D), s3.detach().view(-1, D), scale=SCALE[:D], ga=gad.view(-1, D), glp=glpd.view(-1), **kw)
    assert torch.equal(gm, m3.grad.view(-1, D)) and torch.equal(gs, s3.grad.view(-1, D))
    # only log_prob used: grad_actions arrives absent; only actions used: grad_log_prob absent; mean alone requires grad
    for use in ("lp", "act"):
        m3.grad = s3.grad = None
        act, lp = gym_amd.rsample_squashed_gaussian(m3, s3, scale=SCALE[:D], bias=BIAS[:D], **kw)
        ((lp * glpd).sum() if use == "lp" else (act * gad).sum()).backward()
        wm, ws = sh.sample_backward(mean, ls, scale=SCALE[:D], grad_actions=None if use == "lp" else ga, grad_log_prob=glp if use == "lp" else None, **kw)
        _same(torch, m3.grad.view(-1, D), wm, use)
        _same(torch, s3.grad.view(-1, D), ws, use)
    m_only = dev(torch, mean).requires_grad_()
    act, lp = gym_amd.rsample_squashed_gaussian(m_only, dev(torch, ls), scale=SCALE[:D], bias=BIAS[:D], **kw)
    ((act * gad.view(-1, D)).sum() + (lp * glpd.view(-1)).sum()).backward()
    _same(torch, m_only.grad, want_m, "mean alone")
    # a shared log_std: its gradient is the sum of the per-row gradients, by torch
    s1 = dev(torch, ls[0]).requires_grad_()
    m3.grad = None
    act, lp = gym_amd.rsample_squashed_gaussian(m3, s1, low=[-2, -1.5, 2.625], high=[2, 0.5, 3.375], **kw)      # = SCALE, BIAS
    ((act * gad).sum() + (lp * glpd).sum()).backward()
    wm, ws = sh.sample_backward(mean, ls[0], scale=SCALE[:D], grad_actions=ga, grad_log_prob=glp, **kw)
    _same(torch, m3.grad.view(-1, D), wm, "shared: grad_mean")
    assert torch.equal(s1.grad, dev(torch, ws).sum(dim=0)) and tuple(s1.grad.shape) == (D,)
    _same(torch, act.detach().view(-1, D), sh.sample(mean, ls[0], scale=SCALE[:D], bias=BIAS[:D], **kw)[0], "low / high")
    # no graph without a gradient to compute
    with torch.no_grad():
        act, lp = gym_amd.rsample_squashed_gaussian(m3, s3, **kw)
    assert not act.requires_grad and not lp.requires_grad


def _ulp32(v):
    return np.spacing(np.abs(v * (1 + 1e-6)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("D", DIMS)
def test_agreement_with_torch_distributions(torch, D):
    """log_prob against torch.distributions.TransformedDistribution(Normal, [TanhTransform, AffineTransform]) in float64, evaluated on the
    twin's pre-squash values u (TanhTransform(cache_size=1) takes the cached u back instead of atanh of the action), and the actions
    against the same transform of u.

    With eps = 2^-53 and E the exact value: the device equals the twin bit for bit, and the twin is held to
    |float32 log_prob - E| <= ulp32(E) / 2 + bar(B_LOG_PROB) eps S (tests/test_squashed_host.py), S = sum_j (z_j^2 / 2 + |ls_j| + 1 +
    |log scale_j| + |corr_j| + |n_j| + |u_j|).  torch evaluates, per dim, Normal.log_prob(u) = -(u - mu)^2 / (2 sigma^2) - log sigma -
    log sqrt(2 pi) with sigma = exp(ls) from libm (2 eps relative): u - mu recovers n (1 + d) with the rounding of u, |d| <= eps |u| / |n|,
    so the quotient carries z^2 d = eps |u| |z| / sigma, doubled for the second order, and 5 eps z^2 / 2 from sigma^2 and its own
    roundings; log sigma 2 eps + 2 eps |ls|; then TanhTransform's log |det| = 2 (log 2 - u - softplus(-2 u)), three terms of
    magnitude at most 2 |u| + 2 with an ulp each and two roundings of their sum: 8 eps (|u| + 1); the affine log |scale| one ulp; and
    the subtractions and the sum over dims, at most 8 roundings of a partial sum below S.  Together
        8 eps sum_j (z_j^2 + |ls_j| + |u_j| + 1) + 8 eps S + 2 eps sum_j |u_j| |z_j| / sigma_j.
    The rows keep log_std in [-5, 2], where the last term stays small.  ulp32 is taken of the reference widened by 1e-6, which covers E
    on the other side of a power of two.  The float32 action: half a float32 ulp of the reference plus 4 eps (|bias| + scale)."""
    import gym_amd
    from torch.distributions import AffineTransform, Normal, TanhTransform, TransformedDistribution

    rng = np.random.default_rng(90 + D)
    N = 4099
    mean, ls = _head(rng, N, D)
    md, lsd = dev(torch, mean), dev(torch, ls)
    act, lp = gym_amd.rsample_squashed_gaussian(md, lsd, seed=77, step=3, env_offset=2, scale=SCALE[:D], bias=BIAS[:D])
    r = sh.evaluate(mean, ls, sh.words(77, 2 + np.arange(N, dtype=np.uint64), 3), SCALE[:D], BIAS[:D])
    _same(torch, lp, sh.to_f32(r["log_prob"]), D)
    u = torch.from_numpy(r["u"])
    sc, bi = torch.from_numpy(SCALE[:D].astype(np.float64)), torch.from_numpy(BIAS[:D].astype(np.float64))
    tanh = TanhTransform(cache_size=1)
    dist = TransformedDistribution(Normal(torch.from_numpy(mean.astype(np.float64)), torch.from_numpy(ls.astype(np.float64)).exp()),
                                   [tanh, AffineTransform(bi, sc)])
    y = tanh(u)                                                             # cached: log_prob(a) below inverts to this very u
    a_ref = bi + sc * y
    ref_lp = (dist.base_dist.log_prob(u) - tanh.log_abs_det_jacobian(u, y) - sc.abs().log()).sum(-1).numpy()
    assert np.allclose(ref_lp[np.abs(r["u"]).max(1) < 3], dist.log_prob(a_ref).sum(-1).numpy()[np.abs(r["u"]).max(1) < 3], rtol=0, atol=1e-6)
    eps = 2.0 ** -53
    z, n, absu, abs_ls = np.abs(r["z"]), np.abs(r["n"]), np.abs(r["u"]), np.abs(ls.astype(np.float64))
    S = (0.5 * z * z + abs_ls + 1.0 + np.abs(sh.LOG(r["scale"])) + np.abs(r["corr"]) + n + absu).sum(1)
    tol = (_ulp32(ref_lp) / 2 + sh.bar(sh.B_LOG_PROB) * eps * S + 8 * eps * (z * z + abs_ls + absu + 1).sum(1) + 8 * eps * S
           + 2 * eps * (absu * z / r["sigma"]).sum(1))
    err = np.abs(lp.cpu().numpy().astype(np.float64) - ref_lp)
    print(f"D={D}: worst log_prob error / tolerance {np.max(err / tol):.3f}")
    assert np.all(err <= tol), (D, np.max(err / tol))
    a_err = np.abs(act.cpu().numpy().astype(np.float64) - a_ref.numpy())
    assert np.all(a_err <= _ulp32(a_ref.numpy()) / 2 + 4 * eps * (np.abs(BIAS[:D]) + SCALE[:D]))
    # moments of the recovered z, as in the Gaussian test: atanh of the unit-interval action where it is not saturated
    if D == 1:
        a1, _ = gym_amd.rsample_squashed_gaussian(torch.zeros((1 << 16, 1), device="cuda:0"), torch.zeros(1, device="cuda:0"), seed=5, step=1)
        a1 = a1.double().cpu().numpy()
        zr = np.arctanh(a1[np.abs(a1) < 1 - 1e-6])
        assert zr.size > 0.999 * a1.size and abs(zr.mean()) < 5 / np.sqrt(zr.size) and abs(zr.var() - 1) < 5 * np.sqrt(2 / zr.size) + 1e-3
    assert np.abs(r["z"]).max() < sh.Z_MAX
    assert abs(r["z"].mean()) < 5 / np.sqrt(r["z"].size) and abs(r["z"].var() - 1) < 5 * np.sqrt(2 / r["z"].size)


def test_device_step_counter_graph_replay_and_step_used(torch):
    import gym_amd

    N, D, calls, replays = 300, 3, 6, 3
    mean, ls = _head(np.random.default_rng(77), N, D)
    md, lsd = dev(torch, mean), dev(torch, ls[0])
    s = gym_amd.SquashedGaussianSampler(D, low=[-2, -1.5, 2.625], high=[2, 0.5, 3.375], seed=31, env_offset=2, device=0)
    assert s.scale == tuple(SCALE[:D]) and s.bias == tuple(BIAS[:D])
    rows = [torch.zeros((calls, N, D), device="cuda:0"), torch.zeros((calls, N), device="cuda:0")]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for k in range(3):                                                  # eager: the counter advances by one per draw
            s.sample(md, lsd, out=(rows[0][0], rows[1][0]))
            assert s.step_index() == k + 1
        s.load_state_dict(dict(s.state_dict(), step=0))
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for k in range(calls):
                s.sample(md, lsd, out=(rows[0][k], rows[1][k]))
        got = []
        for _ in range(replays):
            g.replay()
            side.synchronize()
            got.append([r.clone() for r in rows])
    assert s.step_index() == calls * replays
    for i in range(calls * replays):
        eager = gym_amd.rsample_squashed_gaussian(md, lsd, seed=31, step=i, env_offset=2, scale=SCALE[:D], bias=BIAS[:D])
        graphed = tuple(r[i % calls] for r in got[i // calls])
        for a, b in zip(graphed, eager):
            assert np.array_equal(host_bits(torch, a), host_bits(torch, b)), i
        if i % 5 == 0:
            want = sh.sample(mean, ls[0], seed=31, step=i, env_offset=2, scale=SCALE[:D], bias=BIAS[:D])
            _same(torch, eager[0], want[0], i)
            _same(torch, eager[1], want[1], i)
    assert len({host_bits(torch, got[r][0][k]).tobytes() for r in range(replays) for k in range(calls)}) == calls * replays
    # step_used: a backward that runs after later draws reproduces its own forward's noise
    t0 = s.step_index()
    mg = md.clone().requires_grad_()
    sg = lsd.clone().requires_grad_()
    act, lp = s.rsample(mg, sg)
    for _ in range(4):
        s.sample(md, lsd)                                                   # later draws advance the counter
        s.rsample(mg, sg)
    assert s.step_index() == t0 + 9
    ga, glp = _grads(np.random.default_rng(3), N, D)
    ((act * dev(torch, ga)).sum() + (lp * dev(torch, glp)).sum()).backward()
    wm, ws = sh.sample_backward(mean, ls[0], seed=31, step=t0, env_offset=2, scale=SCALE[:D], grad_actions=ga, grad_log_prob=glp)
    _same(torch, mg.grad, wm, "step_used: grad_mean")
    assert torch.equal(sg.grad, dev(torch, ws).sum(dim=0))
    wa, wl = sh.sample(mean, ls[0], seed=31, step=t0, env_offset=2, scale=SCALE[:D], bias=BIAS[:D])
    _same(torch, act.detach(), wa, "step_used: actions")
    _same(torch, lp.detach(), wl, "step_used: log_prob")
    assert s.step_index() == t0 + 9                                         # the backward advanced nothing
    # the entry point writes the step it used
    used = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    counter = torch.full((1,), 2 ** 32 + 1, dtype=torch.int64, device="cuda:0")
    a, l = _forward(torch, md, lsd, seed=31, step=counter, env_offset=2, step_used=used)
    assert int(used.item()) == 2 ** 32 + 1 and int(counter.item()) == 2 ** 32 + 2
    _same(torch, a, sh.sample(mean, ls[0], seed=31, step=2 ** 32 + 1, env_offset=2)[0], "counter")
    gm, _ = _backward(torch, md, lsd, seed=31, step=used, env_offset=2, glp=dev(torch, glp))
    _same(torch, gm, sh.sample_backward(mean, ls[0], seed=31, step=2 ** 32 + 1, env_offset=2, grad_log_prob=glp)[0], "step_dev = step_used")
    assert int(used.item()) == 2 ** 32 + 1


def test_a_restored_sampler_continues_with_the_same_bits(torch):
    import gym_amd

    mean, ls = _head(np.random.default_rng(78), 130, 4)
    md, lsd = dev(torch, mean), dev(torch, ls)
    s = gym_amd.SquashedGaussianSampler(4, low=-3.0, high=1.0, seed=2 ** 64 - 3, env_offset=2 ** 40 + 1)
    for _ in range(5):
        s.sample(md, lsd)
    state = s.state_dict()
    assert state["step"] == 5 and state["seed"] == 2 ** 64 - 3 and state["env_offset"] == 2 ** 40 + 1 and state["action_dim"] == 4
    fresh = gym_amd.SquashedGaussianSampler(4, low=-3.0, high=1.0)
    fresh.load_state_dict(state)
    for i in range(3):
        a, b = s.sample(md, lsd), fresh.rsample(md, lsd)
        want = sh.sample(mean, ls, seed=2 ** 64 - 3, step=5 + i, env_offset=2 ** 40 + 1, scale=[2.0] * 4, bias=[-1.0] * 4)
        _same(torch, a[0], want[0], i)
        _same(torch, a[1], want[1], i)
        for x, y in zip(a, b):
            assert np.array_equal(host_bits(torch, x), host_bits(torch, y))
    assert s.step_index() == fresh.step_index() == 8
    with pytest.raises(ValueError, match="columns"):
        s.sample(md[:, :3], lsd[:, :3])
    with pytest.raises(ValueError, match="action_dim"):
        gym_amd.SquashedGaussianSampler(3, low=-1, high=1).load_state_dict(state)


@pytest.mark.parametrize("env_id,bound", [("Pendulum-v1", 2.0), ("MountainCarContinuous-v0", 1.0)])
def test_box_rollouts_eager_and_sharded(torch, env_id, bound):
    from gym_amd.rollout import DeviceRollout

    n, K = 64, 12
    log_std = np.asarray([0.5], np.float32)

    def run(num, off):
        r = DeviceRollout(env_id, num, seed=4, action_seed=9, env_offset=off)
        r.reset(seed=4)
        s = r.squashed_gaussian_sampler()
        assert (s.action_dim, s.seed, s.env_offset, s.device, s.scale, s.bias) == (1, 9, off, r.device, (bound,), (0.0,))
        assert r.squashed_gaussian_sampler(seed=12).seed == 12
        W = torch.from_numpy(np.random.default_rng(1).standard_normal((r.O, 1)).astype(np.float32)).to(r.device)
        lsd = torch.from_numpy(log_std).to(r.device)
        acts, obs, heads = [], [], []
        with torch.cuda.stream(r.stream):
            for _ in range(K):
                mean = r.obs @ W
                a, lp = s.sample(mean, lsd)
                assert tuple(a.shape) == (num, 1) and a.dtype == r.action_dtype
                heads.append((mean.clone(), lp))
                r.step(a)
                acts.append(a.clone())
                obs.append(r.obs.clone())
        r.synchronize()
        assert s.step_index() == K
        r.close()
        return torch.stack(acts), torch.stack(obs), heads

    acts, obs, heads = run(n, 0)
    for t in (0, K - 1):                                                    # the draws are the twin's for the means the device computed
        want = sh.sample(heads[t][0].cpu().numpy(), log_std, seed=9, step=t, scale=[bound], bias=[0.0])
        _same(torch, acts[t], want[0], (env_id, t))
        _same(torch, heads[t][1], want[1], (env_id, t))
    assert torch.isfinite(obs).all() and float(acts.std()) > 0.1
    assert float(acts.abs().max()) <= bound                                 # every action lies within the env's bounds
    parts = [run(n // 2, off)[:2] for off in (0, n // 2)]
    assert torch.equal(torch.cat((parts[0][0], parts[1][0]), dim=1), acts)
    assert torch.equal(torch.cat((parts[0][1], parts[1][1]), dim=1), obs)


def test_discrete_envs_raise_and_name_policy_sampler(torch):
    from gym_amd.rollout import DeviceRollout

    r = DeviceRollout("CartPole-v1", 8)
    with pytest.raises(ValueError, match=r"policy_sampler\(\)"):
        r.squashed_gaussian_sampler()
    r.close()


def test_the_example_prints_the_same_history_twice(torch, capsys):
    import os
    import sys

    from conftest import ROOT

    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import sac_pendulum
    finally:
        sys.path.pop(0)
    printed = []
    for _ in range(2):
        h = sac_pendulum.train(256, 3, K=8, batch=512, updates=2)
        printed.append(capsys.readouterr().out)
        assert len(h) == 3 and all(np.isfinite(list(row.values())).all() for row in h)
        assert h[0]["alpha"] > 0 and h[0]["mean_log_prob"] == h[0]["mean_log_prob"]
    assert printed[0] == printed[1] and "iteration   2" in printed[0]
