"""gym_amd.evaluate_categorical / evaluate_gaussian on the device against tests/policy_eval_host.py, bit for bit — log_prob, entropy and
the gradients of both: every A and D, shape class, action dtype and absent output or incoming gradient; strided views with guarded
outputs; 2048 * 256 + 257 rows (the tile loops of all four kernels stride); degenerate rows, bad actions, masks and non-finite
values; the samplers' own bits back (the probability ratio 1); autograd through a linear head, leading dims and agreement with torch's
float64 autograd; graph capture; the PPO example end to end."""
import numpy as np
import pytest

import policy_eval_host as pe
import policy_host as ph
from policy_eval_host import bits, to_f32

pytestmark = pytest.mark.gpu

GUARD_F32 = 0x7FABCDEF      # a NaN pattern no computation produces (NaN results are written as 0x7FC00000)
SIZES = (1, 3, 63, 64, 65, 255, 257, 4099)
ACTIONS = (1, 2, 3, 4, 5, 6, 17, 64)
DIMS = (1, 2, 3, 4)
U = 2.0 ** -53


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host_bits(torch, x):
    return x.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _same(torch, got, want64, what):
    assert got.dtype == torch.float32 and tuple(got.shape) == want64.shape, what
    assert np.array_equal(host_bits(torch, got), bits(to_f32(want64))), what


def _logits(rng, M, A):
    """Standard normals of scale 0.1 / 1 / 5 / 30 per row: the input class the twin's bars were measured on."""
    return (rng.standard_normal((M, A)) * rng.choice([0.1, 1.0, 5.0, 30.0], size=(M, 1))).astype(np.float32)


def _head(rng, M, D):
    mean = (rng.standard_normal((M, D)) * rng.choice([0.1, 1.0, 10.0], size=(M, 1))).astype(np.float32)
    ls = rng.uniform(-5.0, 2.0, (M, D)).astype(np.float32)
    act = (mean + np.exp(ls) * rng.standard_normal((M, D))).astype(np.float32)
    return mean, ls, act


def _backward(torch, outs, grads):
    torch.autograd.backward(list(outs), [g for g in grads])


# ---- every shape ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", ACTIONS)
def test_categorical_shapes_dtypes_and_absent_terms_match_the_twin(torch, A):
    from gym_amd import policy_eval

    rng = np.random.default_rng(300 + A)
    for case, M in enumerate(SIZES):
        x = _logits(rng, M, A)
        act = rng.integers(0, A, M)
        gl, gH = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
        adt = (torch.int32, torch.int64)[case % 2]
        xd, ad, gld, gHd = dev(torch, x), dev(torch, act).to(adt), dev(torch, gl), dev(torch, gH)
        want_lp, want_en = pe.categorical(x, act)
        lp, en = policy_eval.evaluate_categorical(xd, ad)
        _same(torch, lp, want_lp, (A, M, "log_prob"))
        _same(torch, en, want_en, (A, M, "entropy"))
        for keep in (0, 1):                                                  # each output absent in turn
            out = [torch.empty(M, device="cuda:0"), torch.empty(M, device="cuda:0")]
            out[1 - keep] = None
            got = policy_eval.evaluate_categorical(xd, ad, out=tuple(out))
            assert got[keep] is out[keep] and got[1 - keep] is None
            _same(torch, got[keep], (want_lp, want_en)[keep], (A, M, "out", keep))
        for use in ((True, True), (True, False), (False, True)):             # each incoming gradient absent in turn
            leaf = xd.clone().requires_grad_()
            lp, en = policy_eval.evaluate_categorical(leaf, ad)
            _same(torch, lp, want_lp, (A, M, "log_prob with grad"))
            outs, grads = zip(*[(o, g) for o, g, u in ((lp, gld, use[0]), (en, gHd, use[1])) if u])
            _backward(torch, outs, grads)
            want = pe.categorical_backward(x, act, gl if use[0] else None, gH if use[1] else None)
            _same(torch, leaf.grad, want, (A, M, "grad", use))


@pytest.mark.parametrize("D", DIMS)
def test_gaussian_shapes_shared_log_std_and_absent_terms_match_the_twin(torch, D):
    from gym_amd import policy_eval

    rng = np.random.default_rng(400 + D)
    for case, M in enumerate(SIZES):
        mean, ls, act = _head(rng, M, D)
        shared = case % 2 == 1                                               # alternate log_std [M, D] and [D]
        ls_ref = ls[0] if shared else ls
        gl, gH = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
        md, lsd, ad, gld, gHd = dev(torch, mean), dev(torch, ls_ref), dev(torch, act), dev(torch, gl), dev(torch, gH)
        want_lp, want_en = pe.gaussian(mean, ls_ref, act)
        lp, en = policy_eval.evaluate_gaussian(md, lsd, ad)
        _same(torch, lp, want_lp, (D, M, "log_prob"))
        _same(torch, en, want_en, (D, M, "entropy"))
        for keep in (0, 1):
            out = [torch.empty(M, device="cuda:0"), torch.empty(M, device="cuda:0")]
            out[1 - keep] = None
            got = policy_eval.evaluate_gaussian(md, lsd, ad, out=tuple(out))
            assert got[keep] is out[keep] and got[1 - keep] is None
            _same(torch, got[keep], (want_lp, want_en)[keep], (D, M, "out", keep))
        for use in ((True, True), (True, False), (False, True)):
            m_leaf, s_leaf = md.clone().requires_grad_(), lsd.clone().requires_grad_()
            lp, en = policy_eval.evaluate_gaussian(m_leaf, s_leaf, ad)
            outs, grads = zip(*[(o, g) for o, g, u in ((lp, gld, use[0]), (en, gHd, use[1])) if u])
            _backward(torch, outs, grads)
            want_m, want_s = pe.gaussian_backward(mean, ls_ref, act, gl if use[0] else None, gH if use[1] else None)
            _same(torch, m_leaf.grad, want_m, (D, M, "grad_mean", use))
            if not shared:
                _same(torch, s_leaf.grad, want_s, (D, M, "grad_log_std", use))
            else:
                # the shared row's gradient is a torch float32 sum of the per-row values: any summation order is within
                # (M - 1) 2^-24 sum |g_i| of their float64 sum
                rows = to_f32(want_s).astype(np.float64)
                err = np.abs(s_leaf.grad.cpu().numpy().astype(np.float64) - rows.sum(0))
                tol = (M - 1) * 2.0 ** -24 * np.abs(rows).sum(0)
                assert s_leaf.grad.shape == (D,) and np.all(err <= tol), (D, M, use, err, tol)
            # only one of the two inputs needs a gradient: the other output is not computed
            m_only = md.clone().requires_grad_()
            lp, en = policy_eval.evaluate_gaussian(m_only, lsd, ad)
            _backward(torch, outs=[o for o, u in ((lp, use[0]), (en, use[1])) if u], grads=grads)
            _same(torch, m_only.grad, want_m, (D, M, "grad_mean alone", use))


# ---- views into wider buffers, guarded outputs ------------------------------------------------------------------------------------------------
def _guarded(torch, shape, lead, tail=5):
    """A contiguous tensor of `shape` inside a guard-filled parent, `lead` elements in; -> (view, parent)."""
    n = int(np.prod(shape))
    parent = torch.empty(n + lead + tail, dtype=torch.float32, device="cuda:0")
    parent.view(torch.int32).fill_(GUARD_F32)
    return parent[lead:lead + n].view(shape), parent


def _check_vector_guards(torch, parent, lead, n, what):
    p = host_bits(torch, parent)
    assert np.all(p[:lead] == GUARD_F32) and np.all(p[lead + n:] == GUARD_F32), what


def _check_row_guards(torch, parent, lead, M, ld, off, W, what):
    wide = host_bits(torch, parent)
    gaps = np.ones((M, ld), bool)
    gaps[:, off:off + W] = False
    assert np.all(wide[:lead] == GUARD_F32) and np.all(wide[lead + M * ld:] == GUARD_F32), what
    assert np.all(wide[lead:lead + M * ld].reshape(M, ld)[gaps] == GUARD_F32), what


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("A", (2, 5, 6))
def test_categorical_views_of_wider_buffers_and_guarded_outputs(torch, A):
    from gym_amd import policy_eval

    rng = np.random.default_rng(500 + A)
    M = 259
    for off in (1, 2, 4):
        ld, gld_ = A + 3 + off, A + 2 + off
        wide = (rng.standard_normal((M, ld)) * 3).astype(np.float32)
        act = rng.integers(0, A, M)
        gl, gH = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
        wd, ad, gl_d, gH_d = dev(torch, wide), dev(torch, act).to(torch.int32 if off == 2 else torch.int64), dev(torch, gl), dev(torch, gH)
        xd, x = wd[:, off:off + A], wide[:, off:off + A]
        assert xd.stride(0) == ld and xd.data_ptr() == wd.data_ptr() + 4 * off
        (lp, plp), (en, pen) = _guarded(torch, (M,), off), _guarded(torch, (M,), off)
        policy_eval.evaluate_categorical(xd, ad, out=(lp, en))
        want_lp, want_en = pe.categorical(x, act)
        _same(torch, lp, want_lp, (A, off))
        _same(torch, en, want_en, (A, off))
        _check_vector_guards(torch, plp, off, M, (A, off, "log_prob"))
        _check_vector_guards(torch, pen, off, M, (A, off, "entropy"))
        # the backward entry point itself, into a strided view of a guarded wide buffer
        gw, pg = _guarded(torch, (M, gld_), off)
        g = gw[:, off:off + A]
        rc = policy_eval.lib.mxv_policy_eval_categorical_backward(_stream(torch), M, A, xd.data_ptr(), ld, ad.data_ptr(), int(ad.dtype == torch.int64),
                                                                  gl_d.data_ptr(), gH_d.data_ptr(), g.data_ptr(), gld_)
        assert rc == 0, policy_eval.lib.mxv_policy_eval_last_error()
        _same(torch, g, pe.categorical_backward(x, act, gl, gH), (A, off, "grad"))
        _check_row_guards(torch, pg, off, M, gld_, off, A, (A, off, "grad guards"))
        # and autograd through the strided view: the gradient of the wide buffer is zero outside the view
        leaf = wd.clone().requires_grad_()
        lp2, en2 = policy_eval.evaluate_categorical(leaf[:, off:off + A], ad)
        _backward(torch, (lp2, en2), (gl_d, gH_d))
        want_wide = np.zeros((M, ld))
        want_wide[:, off:off + A] = to_f32(pe.categorical_backward(x, act, gl, gH))
        assert np.array_equal(host_bits(torch, leaf.grad), bits(want_wide.astype(np.float32))), (A, off)
        assert torch.equal(wd.cpu(), torch.from_numpy(wide))                 # inputs are read only


@pytest.mark.parametrize("D", DIMS)
def test_gaussian_views_of_wider_buffers_and_guarded_outputs(torch, D):
    from gym_amd import policy_eval

    rng = np.random.default_rng(600 + D)
    M = 259
    for k, off in enumerate((1, 2, 4)):
        ld_m, ld_s, ld_a, ld_gm, ld_gs = D + 5 + off, D + 2 + off, D + 3 + off, D + 1 + off, D + 4 + off
        mean, ls, act = _head(rng, M, D)
        wm, ws, wa = (np.zeros((M, ld), np.float32) for ld in (ld_m, ld_s, ld_a))
        wm[:, off:off + D], ws[:, 1:1 + D], wa[:, off:off + D] = mean, ls, act
        wmd, wsd, wad = dev(torch, wm), dev(torch, ws), dev(torch, wa)
        md, sd, ad = wmd[:, off:off + D], wsd[:, 1:1 + D], wad[:, off:off + D]
        shared = k == 1
        ls_arg, ls_ref = (sd[0], ls[0]) if shared else (sd, ls)
        gl, gH = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
        gl_d, gH_d = dev(torch, gl), dev(torch, gH)
        (lp, plp), (en, pen) = _guarded(torch, (M,), off), _guarded(torch, (M,), off)
        policy_eval.evaluate_gaussian(md, ls_arg, ad, out=(lp, en))
        want_lp, want_en = pe.gaussian(mean, ls_ref, act)
        _same(torch, lp, want_lp, (D, off))
        _same(torch, en, want_en, (D, off))
        _check_vector_guards(torch, plp, off, M, (D, off, "log_prob"))
        _check_vector_guards(torch, pen, off, M, (D, off, "entropy"))
        (gmw, pgm), (gsw, pgs) = _guarded(torch, (M, ld_gm), off), _guarded(torch, (M, ld_gs), off)
        gm, gs = gmw[:, off:off + D], gsw[:, 1:1 + D]
        want_m, want_s = pe.gaussian_backward(mean, ls_ref, act, gl, gH)
        for skip in (None, "mean", "log_std"):
            pgm.view(torch.int32).fill_(GUARD_F32)
            pgs.view(torch.int32).fill_(GUARD_F32)
            rc = policy_eval.lib.mxv_policy_eval_gaussian_backward(
                _stream(torch), M, D, md.data_ptr(), ld_m, ls_arg.data_ptr(), 0 if shared else ld_s, ad.data_ptr(), ld_a, gl_d.data_ptr(), gH_d.data_ptr(),
                None if skip == "mean" else gm.data_ptr(), ld_gm, None if skip == "log_std" else gs.data_ptr(), ld_gs)
            assert rc == 0, policy_eval.lib.mxv_policy_eval_last_error()
            if skip == "mean":
                assert np.all(host_bits(torch, pgm) == GUARD_F32)              # an absent output is not written at all
            else:
                _same(torch, gm, want_m, (D, off, skip, "grad_mean"))
                _check_row_guards(torch, pgm, off, M, ld_gm, off, D, (D, off, skip, "grad_mean guards"))
            if skip == "log_std":
                assert np.all(host_bits(torch, pgs) == GUARD_F32)
            else:
                _same(torch, gs, want_s, (D, off, skip, "grad_log_std"))
                _check_row_guards(torch, pgs, off, M, ld_gs, 1, D, (D, off, skip, "grad_log_std guards"))
        assert torch.equal(wmd.cpu(), torch.from_numpy(wm)) and torch.equal(wad.cpu(), torch.from_numpy(wa))


# ---- above 2048 tiles ---------------------------------------------------------------------------------------------------------------------------
# kMaxBlocks * kThreads + 257 rows: the tile loops of the four kernels stride (every smaller M above gives each workgroup one tile);
# workgroup 0 takes a second, full tile (rows 524 288 ..) and workgroup 1 a second tile of one row
STRIDING = 2048 * 256 + 257
SECOND_TRIP = 2048 * 256 + np.array([0, 1, 63, 64, 255, 256])               # rows of the second tiles: both of them, every wave's edge


@pytest.mark.parametrize("A", (3, 7))                                       # a straight-line instantiation and the loop over A
def test_categorical_above_2048_tiles_every_workgroup_takes_a_second_tile(torch, A):
    from gym_amd import policy_eval

    M = STRIDING
    rng = np.random.default_rng(1500 + A)
    x = _logits(rng, M, A)
    act = rng.integers(0, A, M)
    x[SECOND_TRIP[0], 1] = np.nan                                           # the degenerate rows sit where only a second trip reaches
    x[SECOND_TRIP[1]] = -np.inf
    x[SECOND_TRIP[5], 0] = np.inf
    act[SECOND_TRIP[2:5]] = (A, -1, 2 ** 40 + 1)
    gl, gH = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
    xd, ad, gl_d, gH_d = dev(torch, x), dev(torch, act), dev(torch, gl), dev(torch, gH)
    (lp, plp), (en, pen), (g, pg) = _guarded(torch, (M,), 1), _guarded(torch, (M,), 2), _guarded(torch, (M, A), 3)
    policy_eval.evaluate_categorical(xd, ad, out=(lp, en))
    want_lp, want_en = pe.categorical(x, act)
    _same(torch, lp, want_lp, (A, "log_prob"))
    _same(torch, en, want_en, (A, "entropy"))
    assert np.all(host_bits(torch, lp)[SECOND_TRIP] == 0x7FC00000) and np.all(host_bits(torch, en)[SECOND_TRIP] == 0x7FC00000)
    _check_vector_guards(torch, plp, 1, M, (A, "log_prob guards"))          # behind row M - 1 too
    _check_vector_guards(torch, pen, 2, M, (A, "entropy guards"))
    for use in ((True, True), (False, True)):                               # both incoming gradients, then one
        pg.view(torch.int32).fill_(GUARD_F32)
        rc = policy_eval.lib.mxv_policy_eval_categorical_backward(_stream(torch), M, A, xd.data_ptr(), A, ad.data_ptr(), 1,
                                                                  gl_d.data_ptr() if use[0] else None, gH_d.data_ptr() if use[1] else None, g.data_ptr(), A)
        assert rc == 0, policy_eval.lib.mxv_policy_eval_last_error()
        _same(torch, g, pe.categorical_backward(x, act, gl if use[0] else None, gH if use[1] else None), (A, "grad", use))
        assert np.all(host_bits(torch, g).reshape(M, A)[SECOND_TRIP] == 0x7FC00000)
        _check_vector_guards(torch, pg, 3, M * A, (A, "grad guards", use))


@pytest.mark.parametrize("D", (1, 3))
def test_gaussian_above_2048_tiles_every_workgroup_takes_a_second_tile(torch, D):
    from gym_amd import policy_eval

    M = STRIDING
    rng = np.random.default_rng(1600 + D)
    mean, ls, act = _head(rng, M, D)
    mean[SECOND_TRIP[:3], 0] = (np.nan, np.inf, -np.inf)                    # the degenerate rows sit where only a second trip reaches
    ls[SECOND_TRIP[3:], D - 1] = (np.nan, 80.0001, -np.inf)
    gl, gH = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
    md, lsd, ad, gl_d, gH_d = dev(torch, mean), dev(torch, ls), dev(torch, act), dev(torch, gl), dev(torch, gH)
    (lp, plp), (en, pen), (gm, pgm), (gs, pgs) = _guarded(torch, (M,), 1), _guarded(torch, (M,), 2), _guarded(torch, (M, D), 3), _guarded(torch, (M, D), 1)
    policy_eval.evaluate_gaussian(md, lsd, ad, out=(lp, en))
    want_lp, want_en = pe.gaussian(mean, ls, act)
    _same(torch, lp, want_lp, (D, "log_prob"))
    _same(torch, en, want_en, (D, "entropy"))
    assert np.all(host_bits(torch, lp)[SECOND_TRIP] == 0x7FC00000) and np.all(host_bits(torch, en)[SECOND_TRIP] == 0x7FC00000)
    _check_vector_guards(torch, plp, 1, M, (D, "log_prob guards"))          # behind row M - 1 too
    _check_vector_guards(torch, pen, 2, M, (D, "entropy guards"))
    for use in ((True, True), (True, False)):                               # both incoming gradients, then one
        pgm.view(torch.int32).fill_(GUARD_F32)
        pgs.view(torch.int32).fill_(GUARD_F32)
        rc = policy_eval.lib.mxv_policy_eval_gaussian_backward(_stream(torch), M, D, md.data_ptr(), D, lsd.data_ptr(), D, ad.data_ptr(), D,
                                                               gl_d.data_ptr() if use[0] else None, gH_d.data_ptr() if use[1] else None,
                                                               gm.data_ptr(), D, gs.data_ptr(), D)
        assert rc == 0, policy_eval.lib.mxv_policy_eval_last_error()
        want_m, want_s = pe.gaussian_backward(mean, ls, act, gl if use[0] else None, gH if use[1] else None)
        for got, want, parent, lead, name in ((gm, want_m, pgm, 3, "grad_mean"), (gs, want_s, pgs, 1, "grad_log_std")):
            _same(torch, got, want, (D, name, use))
            assert np.all(host_bits(torch, got).reshape(M, D)[SECOND_TRIP] == 0x7FC00000)
            _check_vector_guards(torch, parent, lead, M * D, (D, name, "guards", use))
    # the shared log_std row: a second launch shape of the same loops (log_std_ld = 0)
    lp2, _ = policy_eval.evaluate_gaussian(md, lsd[7], ad)
    _same(torch, lp2, pe.gaussian(mean, ls[7], act)[0], (D, "shared log_std"))


# ---- edge rows --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", (3, 4, 5))
@pytest.mark.parametrize("adt", ("int32", "int64"))
def test_categorical_edge_rows(torch, A, adt):
    from gym_amd import policy_eval

    inf, nan = np.inf, np.nan
    rng = np.random.default_rng(700 + A)
    rows, acts = [], []

    def add(action, **at):
        r = rng.standard_normal(A) * 2
        for k, v in at.items():
            r[int(k[1:])] = v
        rows.append(r)
        acts.append(action)

    for a in range(A):
        add(0, **{f"a{a}": nan})
        add(0, **{f"a{a}": inf})
    rows.append(np.full(A, -inf))
    acts.append(0)
    big = 2 ** 31 - 1 if adt == "int32" else 2 ** 40 + 1                    # an int64 action whose low word is in range stays out of range
    for bad in (A, -1, big, -big, A + 1000):
        add(bad)
    n_bad = len(rows)
    for a in range(A):                                                      # masks: -Inf and a gap beyond 708, chosen and not
        add(a, a1=-inf)
        add(a, a0=0.0, a1=-709.0, a2=-1.0)
        add(a, a0=3e38, a1=-3e38)
    add(0, a0=-3e38, a1=-3e38, a2=-3e38)
    x, act = np.asarray(rows, np.float32), np.asarray(acts, np.int64)
    M = len(x)
    bad = np.arange(M) < n_bad
    gl = rng.standard_normal(M).astype(np.float32)
    gH = rng.standard_normal(M).astype(np.float32)
    gl[-3:] = (inf, -inf, nan)                                               # non-finite incoming gradients follow the arithmetic
    gH[-6:-3] = (nan, inf, -inf)
    xd, ad = dev(torch, x), dev(torch, act).to(getattr(torch, adt))
    (lp, plp), (en, pen), (g, pg) = _guarded(torch, (M,), 1), _guarded(torch, (M,), 2), _guarded(torch, (M, A), 4)
    policy_eval.evaluate_categorical(xd, ad, out=(lp, en))
    gl_d, gH_d = dev(torch, gl), dev(torch, gH)
    rc = policy_eval.lib.mxv_policy_eval_categorical_backward(_stream(torch), M, A, xd.data_ptr(), A, ad.data_ptr(), int(adt == "int64"),
                                                              gl_d.data_ptr(), gH_d.data_ptr(), g.data_ptr(), A)
    assert rc == 0
    want_lp, want_en = pe.categorical(x, act)
    _same(torch, lp, want_lp, A)
    _same(torch, en, want_en, A)
    _same(torch, g, pe.categorical_backward(x, act, gl, gH), A)
    _check_vector_guards(torch, plp, 1, M, "log_prob")                       # a bad action index writes nothing outside its row
    _check_vector_guards(torch, pen, 2, M, "entropy")
    _check_vector_guards(torch, pg, 4, M * A, "grad")
    lpb, enb, gb = host_bits(torch, lp), host_bits(torch, en), host_bits(torch, g)
    assert np.all(lpb[bad] == 0x7FC00000) and np.all(enb[bad] == 0x7FC00000) and np.all(gb[bad] == 0x7FC00000)
    lph, enh = lp.cpu().numpy(), en.cpu().numpy()
    assert not np.isnan(lph[~bad]).any() and np.all(np.isfinite(enh[~bad]))
    masked_chosen = (~bad) & (act == 1) & (np.arange(M) < M - 1)
    assert masked_chosen.sum() == 3 and np.all(lph[masked_chosen] < -708)    # -Inf, or d_a - L for the gap
    nans = np.isnan(g.cpu().numpy())
    assert np.all(gb[nans] == 0x7FC00000) and nans[-6:].any()


@pytest.mark.parametrize("D", (1, 2, 4))
def test_gaussian_edge_rows(torch, D):
    from gym_amd import policy_eval

    inf, nan = np.inf, np.nan
    rng = np.random.default_rng(800 + D)
    mean, ls, act = [], [], []

    def add(mv=None, sv=None, av=None, at=0):
        m, s = rng.standard_normal(D), rng.uniform(-2, 1, D)
        a = m + np.exp(s) * rng.standard_normal(D)
        for arr, v in ((m, mv), (s, sv), (a, av)):
            if v is not None:
                arr[at] = v
        mean.append(m)
        ls.append(s)
        act.append(a)

    for at in range(D):
        for mv in (nan, inf, -inf):
            add(mv=mv, at=at)
        for sv in (nan, 80.0001, -80.0001, inf, -inf):
            add(sv=sv, at=at)
    n_bad = len(mean)
    for at in range(D):
        for sv in (80.0, -80.0):
            add(sv=sv, at=at)
        for av in (inf, -inf, nan, 3e38, 0.0):
            add(av=av, at=at)
    for _ in range(6):
        add()
    mean, ls, act = (np.asarray(v, np.float32) for v in (mean, ls, act))
    M = len(mean)
    bad = np.arange(M) < n_bad
    gl, gH = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
    gl[-3:] = (inf, -inf, nan)
    gH[-6:-3] = (nan, inf, -inf)
    md, lsd, ad = dev(torch, mean), dev(torch, ls), dev(torch, act)
    (lp, plp), (en, pen), (gm, pgm), (gs, pgs) = _guarded(torch, (M,), 1), _guarded(torch, (M,), 2), _guarded(torch, (M, D), 4), _guarded(torch, (M, D), 1)
    policy_eval.evaluate_gaussian(md, lsd, ad, out=(lp, en))
    gl_d, gH_d = dev(torch, gl), dev(torch, gH)
    rc = policy_eval.lib.mxv_policy_eval_gaussian_backward(_stream(torch), M, D, md.data_ptr(), D, lsd.data_ptr(), D, ad.data_ptr(), D,
                                                           gl_d.data_ptr(), gH_d.data_ptr(), gm.data_ptr(), D, gs.data_ptr(), D)
    assert rc == 0
    want_lp, want_en = pe.gaussian(mean, ls, act)
    want_m, want_s = pe.gaussian_backward(mean, ls, act, gl, gH)
    for got, want, parent, lead in ((lp, want_lp, plp, 1), (en, want_en, pen, 2), (gm, want_m, pgm, 4), (gs, want_s, pgs, 1)):
        _same(torch, got, want, D)
        _check_vector_guards(torch, parent, lead, got.numel(), D)
        assert np.all(host_bits(torch, got)[bad] == 0x7FC00000)
        h = got.cpu().numpy()
        assert np.all(host_bits(torch, got)[np.isnan(h)] == 0x7FC00000)
    assert np.all(np.isfinite(en.cpu().numpy()[~bad]))                       # the entropy does not depend on the stored action
    lph = lp.cpu().numpy()
    stored_inf = np.isinf(act).any(1) & ~bad
    assert stored_inf.sum() == 2 * D and np.all(np.isneginf(lph[stored_inf])) and np.isnan(lph[np.isnan(act).any(1) & ~bad]).all()


# ---- the probability ratio of an unchanged policy is 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", ACTIONS)
def test_categorical_evaluation_returns_the_samplers_bits(torch, A):
    from gym_amd import policy, policy_eval

    x = _logits(np.random.default_rng(900 + A), 4099, A)
    x[::11, A // 2] = -np.inf                                                # masks among them (a whole row when A = 1: degenerate, NaN == NaN bits)
    xd = dev(torch, x)
    for adt in (torch.int64, torch.int32):
        act, lp, en = policy.sample_categorical(xd, seed=77, step=3, env_offset=5, action_dtype=adt)
        lp2, en2 = policy_eval.evaluate_categorical(xd, act)
        assert np.array_equal(host_bits(torch, lp2), host_bits(torch, lp)) and np.array_equal(host_bits(torch, en2), host_bits(torch, en)), A
    want = ph.sample_categorical(x, seed=77, step=3, env_offset=5)
    assert np.array_equal(host_bits(torch, lp2), bits(want[1]))


@pytest.mark.parametrize("D", DIMS)
def test_gaussian_evaluation_returns_the_samplers_bits(torch, D):
    from gym_amd import policy, policy_eval

    mean, ls, _ = _head(np.random.default_rng(950 + D), 4099, D)
    md = dev(torch, mean)
    for lsd in (dev(torch, ls), dev(torch, ls[0])):
        act, lp, en = policy.sample_gaussian(md, lsd, seed=78, step=4, env_offset=6)
        lp2, en2 = policy_eval.evaluate_gaussian(md, lsd, act)
        assert np.array_equal(host_bits(torch, lp2), host_bits(torch, lp)) and np.array_equal(host_bits(torch, en2), host_bits(torch, en)), D


@pytest.mark.parametrize("env_id", ["CartPole-v1", "Pendulum-v1"])
def test_rollout_samplers_evaluate_their_own_actions_to_ratio_one(torch, env_id):
    from gym_amd.rollout import DeviceRollout

    r = DeviceRollout(env_id, 257, seed=4, action_seed=9)
    r.reset(seed=4)
    rng = np.random.default_rng(1)
    with torch.cuda.stream(r.stream):
        if env_id == "CartPole-v1":
            s = r.policy_sampler()
            W = dev(torch, rng.standard_normal((r.O, 2)).astype(np.float32))
            for _ in range(3):
                logits = r.obs @ W
                a, lp, en = s.sample(logits)
                lp2, en2 = s.evaluate(logits, a)
                assert a.dtype == r.action_dtype and torch.equal(lp2, lp) and torch.equal(en2, en)
                assert float(((lp2 - lp).exp() - 1).abs().max()) == 0.0
                r.step(a)
            with pytest.raises(ValueError, match="columns"):
                s.evaluate(logits[:, :1], a)
        else:
            s = r.gaussian_sampler()
            W = dev(torch, rng.standard_normal((r.O, 1)).astype(np.float32))
            lsd = dev(torch, np.asarray([-0.5], np.float32))
            for _ in range(3):
                mean = r.obs @ W
                a, lp, en = s.sample(mean, lsd)
                lp2, en2 = s.evaluate(mean, lsd, a)
                assert torch.equal(lp2, lp) and torch.equal(en2, en)
                assert float(((lp2 - lp).exp() - 1).abs().max()) == 0.0
                r.step(a)
        assert s.step_index() == 3                                           # evaluating draws nothing
    r.synchronize()
    r.close()


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------------
def _ulp32(v):
    return np.spacing(np.abs(v * (1 + 1e-6)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("A", (2, 6, 17))
def test_categorical_autograd_through_a_linear_head_and_against_torch_float64(torch, A):
    """logits.grad of a [K, N, A] head against the twin's bits, and against torch's float64 autograd of log_softmax.

    With u = 2^-53: the device equals the twin bit for bit; the twin's float64 dlp_a and dH_a are within BAR_LP u and BAR_EN u of the
    exact ones (tests/test_policy_eval_host.py), the two products and the sum round once each, and the float32 rounding adds half a
    float32 ulp: |got - exact| <= ulp32 / 2 + u (BAR_LP |gl| + BAR_EN |gh| + |gl dlp| + |gh dH| + |g|).  torch's float64 chain
    (log_softmax with libm's exp and log, exp, mul, sum, and their backward) is no more than 3 A + 20 operations deep on any value,
    each rounding at most u relative to a magnitude bounded by |gl| + |gh| (1 + |log p_a| + |H|): that is added for its side."""
    from gym_amd import policy_eval

    K, N, O = 3, 65, 5
    rng = np.random.default_rng(1000 + A)
    obs = rng.standard_normal((K, N, O)).astype(np.float32)
    W0 = (rng.standard_normal((O, A)) * 1.5).astype(np.float32)
    act = rng.integers(0, A, (K, N))
    gl, gH = rng.standard_normal((K, N)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)
    W = dev(torch, W0).requires_grad_()
    logits = dev(torch, obs) @ W                                             # [K, N, A]
    logits.retain_grad()
    ad = dev(torch, act)
    lp, en = policy_eval.evaluate_categorical(logits, ad)
    assert tuple(lp.shape) == tuple(en.shape) == (K, N) and lp.requires_grad and en.requires_grad
    ((lp * dev(torch, gl)).sum() + (en * dev(torch, gH)).sum()).backward()
    x = logits.detach().cpu().numpy().reshape(K * N, A)
    want = pe.categorical_backward(x, act.reshape(-1), gl.reshape(-1), gH.reshape(-1))
    _same(torch, logits.grad.view(K * N, A), want, A)
    assert torch.allclose(W.grad, dev(torch, obs).reshape(K * N, O).t() @ logits.grad.view(K * N, A), rtol=1e-4, atol=1e-4)      # the head's own backward ran on it
    # torch's float64 autograd on the same float32 logits
    x64 = logits.detach().double().requires_grad_()
    lsm = torch.log_softmax(x64, dim=-1)
    lp64 = lsm.gather(-1, ad.long().unsqueeze(-1)).squeeze(-1)
    en64 = -(lsm.exp() * lsm).sum(-1)
    ((lp64 * dev(torch, gl).double()).sum() + (en64 * dev(torch, gH).double()).sum()).backward()
    ref = x64.grad.cpu().numpy().reshape(K * N, A)
    got = logits.grad.cpu().numpy().reshape(K * N, A).astype(np.float64)
    logp = lsm.detach().cpu().numpy().reshape(K * N, A)
    agl, agh = np.abs(gl.reshape(-1, 1)).astype(np.float64), np.abs(gH.reshape(-1, 1)).astype(np.float64)
    p = np.exp(logp)
    H = -(p * logp).sum(1, keepdims=True)
    onehot = np.arange(A)[None, :] == act.reshape(-1, 1)
    mag = agl * np.abs(onehot - p) + agh * p * np.abs(logp + H)
    tol = (_ulp32(ref) / 2 + U * (pe.bar(pe.B_GRAD_LOG_PROB) * agl + pe.bar(pe.B_GRAD_ENTROPY) * agh + 2 * mag + np.abs(ref))
           + (3 * A + 20) * U * (agl + agh * (1 + np.abs(logp) + np.abs(H))))
    err = np.abs(got - ref)
    print(f"A={A}: worst error / tolerance {np.max(err / tol):.3f}")
    assert np.all(err <= tol), (A, np.max(err / tol))
    # a layout that view(-1, A) cannot flatten raises, and says so
    base = torch.zeros((N, K, A + 2), device="cuda:0")
    with pytest.raises(ValueError, match=r"view\(-1, "):
        policy_eval.evaluate_categorical(base.transpose(0, 1)[:, :, :A], ad)
    # no gradient flows when neither output is used, and out= is refused when one could
    leaf = dev(torch, x).requires_grad_()
    with pytest.raises(ValueError, match="requires grad"):
        policy_eval.evaluate_categorical(leaf, ad.view(-1), out=(torch.empty(K * N, device="cuda:0"), None))
    with torch.no_grad():
        lp3, _ = policy_eval.evaluate_categorical(leaf, ad.view(-1))
    assert not lp3.requires_grad and np.array_equal(host_bits(torch, lp3), host_bits(torch, lp.view(-1)))


@pytest.mark.parametrize("D", (1, 3))
def test_gaussian_autograd_against_torch_float64(torch, D):
    """grad_mean and grad_log_std of a [K, N, D] head against the twin's bits and against torch.distributions.Normal in float64.

    With u = 2^-53: the twin's zq / sigma is within BAR_MEAN u of the exact one relatively, zq^2 - 1 within BAR_LS u (zq^2 + 1); the
    product with gl and the sum with gh round once each; the float32 rounding adds half a float32 ulp.  torch's float64 chain (libm's exp
    within 1 ulp, a subtraction, squares, a division, log, sums and their backward) is at most 12 operations deep, each rounding at
    most u relative to a magnitude bounded by the value's own terms: |gl| |zq / sigma| and |gl| (zq^2 + 1) + |gh|."""
    from gym_amd import policy_eval

    K, N = 3, 65
    rng = np.random.default_rng(1100 + D)
    mean, ls, act = _head(rng, K * N, D)
    gl, gH = rng.standard_normal((K, N)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)
    want_m, want_s = pe.gaussian_backward(mean, ls, act, gl.reshape(-1), gH.reshape(-1))
    md, lsd = dev(torch, mean).view(K, N, D).requires_grad_(), dev(torch, ls).view(K, N, D).requires_grad_()
    ad = dev(torch, act).view(K, N, D)
    lp, en = policy_eval.evaluate_gaussian(md, lsd, ad)
    assert tuple(lp.shape) == tuple(en.shape) == (K, N)
    ((lp * dev(torch, gl)).sum() + (en * dev(torch, gH)).sum()).backward()
    _same(torch, md.grad.view(K * N, D), want_m, D)
    _same(torch, lsd.grad.view(K * N, D), want_s, D)
    m64, s64 = dev(torch, mean).double().requires_grad_(), dev(torch, ls).double().requires_grad_()
    dist = torch.distributions.Normal(m64, s64.exp())
    lp64, en64 = dist.log_prob(dev(torch, act).double()).sum(-1), dist.entropy().sum(-1)
    ((lp64 * dev(torch, gl).double().view(-1)).sum() + (en64 * dev(torch, gH).double().view(-1)).sum()).backward()
    ref_m, ref_s = m64.grad.cpu().numpy(), s64.grad.cpu().numpy()
    p = pe.gaussian_parts(mean, ls, act)
    agl, agh = np.abs(gl.reshape(-1, 1)).astype(np.float64), np.abs(gH.reshape(-1, 1)).astype(np.float64)
    mag_m = agl * np.abs(p["zq"] / p["sigma"])
    mag_s = agl * (p["zq"] * p["zq"] + 1) + agh
    tol_m = _ulp32(ref_m) / 2 + U * (pe.bar(pe.B_GRAD_MEAN) + 1 + 12) * mag_m
    tol_s = _ulp32(ref_s) / 2 + U * (pe.bar(pe.B_GRAD_LOG_STD) + 2 + 12) * mag_s
    err_m = np.abs(md.grad.view(K * N, D).cpu().numpy().astype(np.float64) - ref_m)
    err_s = np.abs(lsd.grad.view(K * N, D).cpu().numpy().astype(np.float64) - ref_s)
    print(f"D={D}: worst error / tolerance: mean {np.max(err_m / tol_m):.3f}, log_std {np.max(err_s / tol_s):.3f}")
    assert np.all(err_m <= tol_m) and np.all(err_s <= tol_s), (D, np.max(err_m / tol_m), np.max(err_s / tol_s))
    base = torch.zeros((N, K, D + 2), device="cuda:0")
    with pytest.raises(ValueError, match=r"view\(-1, "):
        policy_eval.evaluate_gaussian(base.transpose(0, 1)[:, :, :D], lsd.detach(), ad)


# ---- graph capture ----------------------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_replay_in_a_captured_graph(torch):
    from gym_amd import policy_eval

    M, A = 300, 6
    rng = np.random.default_rng(1200)
    xs = [_logits(rng, M, A) for _ in range(3)]
    act = rng.integers(0, A, M)
    gl, gH = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
    x = dev(torch, xs[0]).requires_grad_()
    ad, gld, gHd = dev(torch, act), dev(torch, gl), dev(torch, gH)

    def step():
        lp, en = policy_eval.evaluate_categorical(x, ad)
        ((lp * gld).sum() + (en * gHd).sum()).backward()
        return lp, en

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                                                   # warm-up outside the capture
            x.grad = None
            step()
        side.synchronize()
        x.grad = None
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            lp, en = step()
        for k in (1, 2):                                                     # replay twice, the logits buffer rewritten in between
            with torch.no_grad():
                x.copy_(dev(torch, xs[k]))
            g.replay()
            side.synchronize()
            want_lp, want_en = pe.categorical(xs[k], act)
            _same(torch, lp, want_lp, k)
            _same(torch, en, want_en, k)
            _same(torch, x.grad, pe.categorical_backward(xs[k], act, gl, gH), k)
    torch.cuda.current_stream().wait_stream(side)


# ---- the example ------------------------------------------------------------------------------------------------------------------------------
def test_the_ppo_example_starts_every_iteration_at_ratio_one_and_repeats_itself(torch, capsys):
    import os
    import sys

    from conftest import ROOT

    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import ppo_clip
    finally:
        sys.path.pop(0)
    printed = []
    for _ in range(2):
        h = ppo_clip.train(256, 2, K=16)
        printed.append(capsys.readouterr().out)
        assert len(h) == 2
        for row in h:
            first = row["epochs"][0]
            assert first["ratio_min"] == 1.0 and first["ratio_max"] == 1.0 and first["approx_kl"] == 0.0 and first["clipped"] == 0.0
            assert all(np.isfinite(list(e.values())).all() for e in row["epochs"]) and len(row["epochs"]) == 4
            assert row["epochs"][-1]["ratio_max"] > 1.0 > row["epochs"][-1]["ratio_min"]      # and the later epochs have moved
    assert printed[0] == printed[1] and "iteration   1" in printed[0] and f"{3 + 2 * 16} policy steps drawn" in printed[0]
