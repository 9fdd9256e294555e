"""scan_kernel and the two *_apply_kernel of gym_amd/csrc/mxv_norm.hip on the MI355X, driven on their own: mxv_norm_obs_apply /
mxv_norm_reward_apply take the ranks' sums [W][K][2 O] from the caller, so the running update can be fed SYNTHETIC sums with a handful of
rows — any K (one chunk of 256 steps, the chunk edge, three chunks), any world size up to 64 (odd leftovers in the rank tree), any
total_rows — and compared with oracle.RunningNorm (mode 1, oracle/normalize.c) on the same sums.  Everything after the sums is IEEE
arithmetic in the reference's order on both sides, so the bar is equality of every bit: the outputs, and mean / var / count afterwards.

One reading of "bit for bit": IEEE 754 leaves the sign of the NaN that an invalid operation (inf - inf, 0 * inf) produces to the
implementation — x86 makes its default quiet NaN negative, the GPU positive — so where the oracle holds a default quiet NaN (quiet bit alone,
either sign) the device may hold it with either sign.  Every other value, NaNs with a payload and the sign of zero included, is compared as bits.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIMS = (1, 2, 3, 4, 6)
KS = (1, 255, 256, 257, 600)
WORLDS = (1, 2, 3, 5, 8, 63, 64)
TAIL_NS = (1, 255, 256, 257, 1023)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.dtype in (np.float32, np.float64), (a.dtype, b.dtype, a.shape, b.shape)
    iv, sign, qnan = (np.uint32, 0x80000000, 0x7FC00000) if a.dtype == np.float32 else (np.uint64, 1 << 63, 0x7FF8 << 48)
    ab, bb = a.view(iv), b.view(iv)
    default_nan = ((bb & iv(~sign & (2 * sign - 1))) == iv(qnan)) & ((ab | iv(sign)) == (bb | iv(sign)))
    return bool(np.all((ab == bb) | default_nan))


def _f64(*v):
    return np.array(v, np.float64).ravel()


def _synthetic_sums(rng, W, K, O, rows):
    """[W][K][2 O]: per (step, column) a mean and a spread, every rank's (sum, sum of squares) of `rows` rows scattered around them"""
    mu = rng.standard_normal((1, K, O)) * 3.0
    sigma = np.exp(rng.uniform(-3.0, 2.0, (1, K, O)))
    S = rows * mu + np.sqrt(rows) * sigma * rng.standard_normal((W, K, O))
    Q = rows * (sigma ** 2 + mu ** 2) * (1.0 + 0.01 * rng.standard_normal((W, K, O)))
    return np.ascontiguousarray(np.concatenate([S, Q], axis=2))


def _oracle(n, O, eps=1e-8):
    from oracle.oracle import RunningNorm

    return RunningNorm(n, O, obs_epsilon=eps, rew_epsilon=eps, mode=1)


def _check_obs(nm, orc, x, sums, total_rows, eps=1e-8, where=None):
    """one mxv_norm_obs_apply call in both output dtypes' worth of checks: y (float64) and the state against the oracle, y (float32) ==
    the rounded float64 output (from a twin handle in the same state)"""
    import torch
    from gym_amd import _native

    K, n, O = x.shape
    W = sums.shape[0]
    twin = _native.Norm(O, n)
    twin.set_state(*nm.get_state())
    xd, sd = _dev(x), _dev(sums)
    y = torch.full((K, n, O), np.nan, dtype=torch.float64, device="cuda")
    y32 = torch.full((K, n, O), np.nan, dtype=torch.float32, device="cuda")
    nm.obs_apply(K, xd, y, False, eps, sd, W, total_rows)
    twin.obs_apply(K, xd, y32, True, eps, sd, W, total_rows)
    torch.cuda.synchronize()
    y, y32 = y.cpu().numpy(), y32.cpu().numpy()
    want = orc.obs_apply(x, sums, total_rows)
    assert _same(y, want), (where, np.argwhere(y != want)[:4])
    with np.errstate(over="ignore"):
        assert _same(y32, y.astype(np.float32)), where
    for h in (nm, twin):
        mean, var, count = h.get_state()
        assert _same(mean, orc.obs_mean) and _same(var, orc.obs_var) and _same(_f64(count), orc.obs_count), (where, mean, orc.obs_mean)
    twin.close()


def _check_rew(nm, orc, r, sums, total_rows, eps=1e-8, where=None, shifted=False):
    """one mxv_norm_reward_apply call (r float32 or float64 [K][n]) against the oracle; `shifted`: views one element into an allocation"""
    import torch

    K, n = r.shape
    W = sums.shape[0]
    f32 = r.dtype == np.float32
    rd = _dev(r)
    out = torch.full((K, n), np.nan, dtype=rd.dtype, device="cuda")
    if shifted:
        flat = torch.empty(r.size + 1, dtype=rd.dtype, device="cuda")
        flat[1:].view(K, n).copy_(rd)
        rd = flat[1:].view(K, n)
        out = torch.full((r.size + 1,), np.nan, dtype=rd.dtype, device="cuda")[1:].view(K, n)
        assert rd.data_ptr() % 16 == r.itemsize and out.data_ptr() % 16 == r.itemsize
    else:
        assert rd.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    nm.reward_apply(K, rd, f32, out, eps, _dev(sums), W, total_rows)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = orc.reward_apply(r, sums, total_rows)                      # float64 arithmetic on the (exactly converted) rewards
    with np.errstate(over="ignore"):
        assert _same(got, want.astype(r.dtype)), (where, np.argwhere(got != want.astype(r.dtype))[:4])
    mean, var, count = nm.get_state()
    assert _same(mean, orc.ret_mean) and _same(var, orc.ret_var) and _same(_f64(count), orc.ret_count), (where, mean, var, orc.ret_mean, orc.ret_var)


# ---- K across the chunks of 256 steps, W across the rank tree --------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("O", DIMS)
def test_obs_scan_against_oracle_at_every_chunking_and_world_size(O, K):
    from gym_amd import _native

    rng = np.random.default_rng(10 * K + O)
    n = 3
    x = (rng.standard_normal((K, n, O)) * 3.0).astype(np.float32)
    for W in WORLDS:
        rows = 37 + W                                                  # rows per rank, nothing to do with n
        sums = _synthetic_sums(rng, W, K, O, rows)
        nm, orc = _native.Norm(O, n), _oracle(n, O)
        _check_obs(nm, orc, x, sums, W * rows, where=("W", W))
        nm.close()


@pytest.mark.parametrize("K", KS)
def test_reward_scan_against_oracle_at_every_chunking_and_world_size(K):
    from gym_amd import _native

    rng = np.random.default_rng(K)
    n = 6
    r = rng.standard_normal((K, n)) * 2.0 + 1.0
    for W in WORLDS:
        rows = 37 + W
        sums = _synthetic_sums(rng, W, K, 1, rows)
        for rr in (r, r.astype(np.float32)):
            nm, orc = _native.Norm(1, n), _oracle(n, 1)
            _check_rew(nm, orc, rr, sums, W * rows, where=("W", W, rr.dtype))
            nm.close()


def test_one_handle_regrows_from_a_short_chunk_to_longer_ones():
    """K = 1, then 257, 600, 2 on the SAME handles: the coefficient buffers regrow, the statistics carry over."""
    from gym_amd import _native

    rng = np.random.default_rng(7)
    n, O, W, rows = 4, 3, 3, 50
    a, b = _native.Norm(O, n), _native.Norm(1, n)
    orc = _oracle(n, O)
    for K in (1, 257, 600, 2):
        x = (rng.standard_normal((K, n, O)) * 3.0).astype(np.float32)
        _check_obs(a, orc, x, _synthetic_sums(rng, W, K, O, rows), W * rows, where=("obs", K))
        _check_rew(b, orc, rng.standard_normal((K, n)), _synthetic_sums(rng, W, K, 1, rows), W * rows, where=("reward", K))
    assert abs(a.get_state()[2] - 860 * W * rows) < 1e-3                # 1 + 257 + 600 + 2 batches
    a.close(), b.close()


def test_world_and_total_rows_out_of_range_are_refused():
    import torch
    from gym_amd import _native

    n, O, K = 4, 2, 2
    a, b = _native.Norm(O, n), _native.Norm(1, n)
    x = torch.ones((K, n, O), dtype=torch.float32, device="cuda")
    y = torch.zeros((K, n, O), dtype=torch.float64, device="cuda")
    r = torch.ones((K, n), dtype=torch.float64, device="cuda")
    o = torch.zeros((K, n), dtype=torch.float64, device="cuda")
    so = torch.ones((65, K, 2 * O), dtype=torch.float64, device="cuda")
    sr = torch.ones((65, K, 2), dtype=torch.float64, device="cuda")
    for world, total in ((0, 100), (65, 100), (-1, 100), (1, 0), (1, -5), (64, 0)):
        with pytest.raises(_native.MxvError) as ei:
            a.obs_apply(K, x, y, False, 1e-8, so, world, total)
        assert ei.value.code == _native.ERR_INVALID_ARG, (world, total)
        with pytest.raises(_native.MxvError) as ei:
            b.reward_apply(K, r, False, o, 1e-8, sr, world, total)
        assert ei.value.code == _native.ERR_INVALID_ARG, (world, total)
    torch.cuda.synchronize()
    for h in (a, b):                                                   # a refused call changes nothing
        mean, var, count = h.get_state()
        assert np.all(mean == 0) and np.all(var == 1) and count == 1e-4
    assert float(y.abs().sum()) == 0 and float(o.abs().sum()) == 0
    a.obs_apply(K, x, y, False, 1e-8, so, 64, 100)                     # the bounds themselves are accepted
    b.reward_apply(K, r, False, o, 1e-8, sr, 64, 1)
    torch.cuda.synchronize()
    a.close(), b.close()


# ---- the apply kernels' tails and forms ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", TAIL_NS)
@pytest.mark.parametrize("O", DIMS)
def test_obs_apply_tails(O, n):
    from gym_amd import _native

    rng = np.random.default_rng(n * 10 + O)
    K, W, rows = 2, 2, 500
    x = (rng.standard_normal((K, n, O)) * 3.0 + 1.0).astype(np.float32)
    nm, orc = _native.Norm(O, n), _oracle(n, O)
    _check_obs(nm, orc, x, _synthetic_sums(rng, W, K, O, rows), W * rows)
    nm.close()


@pytest.mark.parametrize("n", TAIL_NS + (258, 1022, 1024))             # n % 2, n % 4: float64 takes 16-byte lanes at even n, float32 at n % 4 == 0
def test_reward_apply_vector_and_element_forms(n):
    from gym_amd import _native

    rng = np.random.default_rng(n)
    K, W, rows = 3, 2, 500
    r = rng.standard_normal((K, n)) * 2.0 + 1.0
    sums = _synthetic_sums(rng, W, K, 1, rows)
    for rr in (r, r.astype(np.float32)):
        for shifted in (False, True):
            nm, orc = _native.Norm(1, n), _oracle(n, 1)
            _check_rew(nm, orc, rr, sums, W * rows, where=(rr.dtype, shifted), shifted=shifted)
            nm.close()


# ---- sums that stress the moment arithmetic --------------------------------------------------------------------------------------------

def _stress_sums(case, rng, W, K, O, rows, float32_moments):
    """-> (sums [W][K][2 O], column values [K] that rows of the stressed column 0 hold); the other columns are ordinary"""
    sums = _synthetic_sums(rng, W, K, O, rows)
    val = np.ones(K)
    if case == "constant":                                             # Q - 2 m S + N m^2 (resp. Q / N - mean^2) cancels to zero or just below
        val = np.array([0.1, -7.3, 1e-3, 12345.678, 3.0])[:K]
        if float32_moments:
            val = val.astype(np.float32).astype(np.float64)
        sums[:, :, 0] = rows * val
        sums[:, :, O] = rows * (val * val)
    elif case == "float32 scale 1e30":
        val = np.float32(1e30) * np.array([1.0, -2.5, 0.75, 1.5, -1.0])[:K].astype(np.float64)
        sums[:, :, 0] = rows * val * (1.0 + 0.1 * rng.standard_normal((W, K)))
        sums[:, :, O] = rows * val * val * 1.02
    elif case == "nan":
        sums[W - 1, 1, 0] = np.nan
    elif case == "inf":
        sums[0, 1, 0] = np.inf
        sums[0, 1, O] = np.inf
    else:
        raise AssertionError(case)
    return sums, val


@pytest.mark.parametrize("count", [1e-4, 1.0, 2.0 ** 52])
@pytest.mark.parametrize("case", ["constant", "float32 scale 1e30", "nan", "inf"])
def test_stressed_sums_and_injected_statistics(case, count):
    from gym_amd import _native

    rng = np.random.default_rng(int(np.log2(count) + 60))
    K, W, rows, n, O = 5, 2, 500, 5, 3
    mean0, var0 = rng.standard_normal(O) * 2.0, np.exp(rng.uniform(-2, 2, O))
    # observations: float32 batch moments
    sums, val = _stress_sums(case, rng, W, K, O, rows, True)
    x = (rng.standard_normal((K, n, O)) * 3.0).astype(np.float32)
    x[:, :, 0] = val[:, None].astype(np.float32)
    if case == "constant":                                             # the case is what it says: the clamp at zero is taken
        S, Q, N = sums[0, :, 0] + sums[1, :, 0], sums[0, :, O] + sums[1, :, O], float(W * rows)
        m = (S / N).astype(np.float32).astype(np.float64)
        v = ((Q - 2.0 * m * S) + N * m * m) / N
        assert np.all(np.abs(v) <= 1e-9 * val * val) and np.any(v <= 0)
    nm, orc = _native.Norm(O, n), _oracle(n, O)
    nm.set_state(mean0, var0, count)
    orc.obs_mean[:], orc.obs_var[:], orc.obs_count[:] = mean0, var0, count
    _check_obs(nm, orc, x, sums, W * rows, where=(case, count))
    if case in ("nan", "inf"):
        assert np.isnan(orc.obs_mean[0]) and np.all(np.isfinite(orc.obs_mean[1:])) and np.all(np.isfinite(orc.obs_var[1:]))
    nm.close()
    # returns: float64 batch moments
    sums, val = _stress_sums(case, rng, W, K, 1, rows, False)
    if case == "constant":
        bm = (sums[0, :, 0] + sums[1, :, 0]) / (W * rows)
        v = (sums[0, :, 1] + sums[1, :, 1]) / (W * rows) - bm * bm
        assert np.all(np.abs(v) <= 1e-12 * val * val) and np.any(v <= 0)
    r = rng.standard_normal((K, n)) * val[:, None]
    for rr in (r, r.astype(np.float32)):
        nm, orc = _native.Norm(1, n), _oracle(n, 1)
        nm.set_state(mean0[:1], var0[:1], count)
        orc.ret_mean[:], orc.ret_var[:], orc.ret_count[:] = mean0[:1], var0[:1], count
        _check_rew(nm, orc, rr, sums, W * rows, where=(case, count, rr.dtype))
        nm.close()
