"""gym_amd.sample_gaussian / GaussianSampler on the device against tests/gaussian_host.py, bit for bit — the action bits, the bits of
log_prob and the bits of entropy: every D, shape class, offset and step, 2048 * 256 + 257 rows (the tile loop strides), strided views
with guarded outputs, degenerate and extreme rows, agreement with torch.distributions.Normal, the device step counter under graph
replay, checkpoints, and the samplers of the two Box envs end to end."""
import numpy as np
import pytest

import gaussian_host as gh
import replay_host as rh
from gaussian_host import bits

pytestmark = pytest.mark.gpu

GUARD_F32 = 0x7FABCDEF      # a NaN pattern no computation produces (NaN results are written as 0x7FC00000)
SIZES = (1, 3, 63, 64, 65, 255, 257, 4099)
DIMS = (1, 2, 3, 4)
OFFSETS = (0, 1, 6)
STEPS = (0, 5, 2 ** 32 + 1)
SEED = 2 ** 63 + 17         # one seed for every D: the twin's Philox words are shared between the cases


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host_bits(torch, x):
    return x.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _head(rng, N, D):
    """Means of scale 0.1 / 1 / 10 and log_std over [-5, 2]: the input class the twin's bars were measured on."""
    mean = (rng.standard_normal((N, D)) * rng.choice([0.1, 1.0, 10.0], size=(N, 1))).astype(np.float32)
    return mean, rng.uniform(-5.0, 2.0, (N, D)).astype(np.float32)


def _assert_equal(torch, got, want, what):
    a, lp, en = got
    wa, wlp, wen = want
    assert tuple(a.shape) == wa.shape and np.array_equal(host_bits(torch, a), bits(wa)), what
    if lp is not None:
        assert np.array_equal(host_bits(torch, lp), bits(wlp)), what
    if en is not None:
        assert np.array_equal(host_bits(torch, en), bits(wen)), what


@pytest.mark.parametrize("D", DIMS)
def test_every_shape_offset_and_step_matches_the_twin(torch, D):
    from gym_amd import policy

    rng = np.random.default_rng(7 + D)
    case = 0
    for N in SIZES:
        mean, ls = _head(rng, N, D)
        md, lsd, ls1d = dev(torch, mean), dev(torch, ls), dev(torch, ls[0])
        for off in OFFSETS:
            for step in STEPS:
                shared = case % 2 == 1                                      # alternate log_std [N, D] and [D]
                case += 1
                got = policy.sample_gaussian(md, ls1d if shared else lsd, seed=SEED, step=step, env_offset=off)
                assert got[0].dtype == got[1].dtype == got[2].dtype == torch.float32
                _assert_equal(torch, got, gh.sample_gaussian(mean, ls[0] if shared else ls, seed=SEED, step=step, env_offset=off),
                              (N, D, off, step, shared))


def _guarded(torch, shape, lead, tail=5):
    """A contiguous tensor of `shape` inside a guard-filled parent, `lead` elements in; -> (view, parent)."""
    n = int(np.prod(shape))
    parent = torch.empty(n + lead + tail, dtype=torch.float32, device="cuda:0")
    parent.view(torch.int32).fill_(GUARD_F32)
    return parent[lead:lead + n].view(shape), parent


def _guard_bits(torch, t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("D", DIMS)
def test_views_of_wider_buffers_and_guarded_outputs(torch, D):
    from gym_amd import policy

    rng = np.random.default_rng(40 + D)
    N = 259
    for k, off in enumerate((1, 2, 4)):
        ld_m, ld_s, ld_a = D + 5 + off, D + 2 + off, D + 3 + off
        wide_m = rng.standard_normal((N, ld_m)).astype(np.float32)
        wide_s = rng.uniform(-3.0, 1.0, (N, ld_s)).astype(np.float32)
        wm, ws = dev(torch, wide_m), dev(torch, wide_s)
        md, sd = wm[:, off:off + D], ws[:, 1:1 + D]
        assert md.stride(0) == ld_m and md.data_ptr() == wm.data_ptr() + 4 * off
        mean, ls = wide_m[:, off:off + D], wide_s[:, 1:1 + D]
        shared = k == 1
        ls_arg, ls_ref = (sd[0], ls[0]) if shared else (sd, ls)
        wa, pa = _guarded(torch, (N, ld_a), 3)                              # the actions: a strided view into a guarded wide buffer
        a = wa[:, off:off + D]
        (lp, plp), (en, pen) = _guarded(torch, (N,), 1), _guarded(torch, (N,), 2)
        want = gh.sample_gaussian(mean, ls_ref, seed=5, step=9, env_offset=off)
        for omit in (None, 1, 2, (1, 2)):
            out = [a, lp, en]
            for o in (() if omit is None else (omit,) if isinstance(omit, int) else omit):
                out[o] = None
                (plp if o == 1 else pen).view(torch.int32).fill_(GUARD_F32)
            pa.view(torch.int32).fill_(GUARD_F32)
            got = policy.sample_gaussian(md, ls_arg, seed=5, step=9, env_offset=off, out=tuple(out))
            assert got[0] is a and got[1] is out[1] and got[2] is out[2]
            _assert_equal(torch, got, want, (D, off, omit))
            for o, parent in ((1, plp), (2, pen)):
                if out[o] is None:                                          # an omitted output is not written at all
                    assert np.all(_guard_bits(torch, parent) == GUARD_F32), (D, off, omit)
            # the gaps between the action rows and the elements around every output still hold the guard
            gaps = np.ones((N, ld_a), bool)
            gaps[:, off:off + D] = False
            wide = _guard_bits(torch, pa)
            assert np.all(wide[:3] == GUARD_F32) and np.all(wide[3 + N * ld_a:] == GUARD_F32), (D, off, omit, "actions")
            assert np.all(wide[3:3 + N * ld_a].reshape(N, ld_a)[gaps] == GUARD_F32), (D, off, omit, "action gaps")
            for parent, lead, name in ((plp, 1, "log_prob"), (pen, 2, "entropy")):
                p = _guard_bits(torch, parent)
                assert np.all(p[:lead] == GUARD_F32) and np.all(p[lead + N:] == GUARD_F32), (D, off, omit, name)
        assert torch.equal(wm.cpu(), torch.from_numpy(wide_m)) and torch.equal(ws.cpu(), torch.from_numpy(wide_s))      # inputs are read only


# kMaxBlocks * kThreads + 257 rows: the tile loop of gaussian_kernel strides (every smaller N above gives each workgroup one tile);
# workgroup 0 takes a second, full tile (rows 524 288 ..) and workgroup 1 a second tile of one row
STRIDING = 2048 * 256 + 257


def _twin_at_scale(mean, log_std, seed, step, env_offset):
    """gh.sample_gaussian with the rule's words from replay_host's vectorised Philox4x32-10 (held to Random123's known answers by
    tests/test_replay_host.py): gh.words makes one Python call per env, 7 s at this N.  Rows of both trips are checked against it."""
    N = len(mean)
    G = np.uint64(env_offset) + np.arange(N, dtype=np.uint64)
    w4 = np.stack(rh.philox4x32_10(G & np.uint64(0xFFFFFFFF), G >> np.uint64(32), step & 0xFFFFFFFF,
                                   ((step >> 32) & 0x0FFFFFFF) | (gh.STREAM_GAUSSIAN << 28), seed & 0xFFFFFFFF, seed >> 32), axis=1)
    spot = [0, 1, 255, 256, 2048 * 256 - 1, 2048 * 256, N - 2, N - 1]
    assert np.array_equal(w4[spot], gh.words(seed, [env_offset + i for i in spot], step))
    r = gh.evaluate(mean, log_std, w4)
    return gh.to_f32(r["act"]).reshape(mean.shape), gh.to_f32(r["log_prob"]), gh.to_f32(r["entropy"])


@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("D", (1, 4))                                       # the narrowest and the widest instantiation
def test_above_2048_tiles_every_workgroup_takes_a_second_tile(torch, D, shared):
    from gym_amd import policy

    N = STRIDING
    mean, ls = _head(np.random.default_rng(1400 + D), N, D)
    ls_ref = ls[0] if shared else ls
    (a, pa), (lp, plp), (en, pen) = _guarded(torch, (N, D), 3), _guarded(torch, (N,), 1), _guarded(torch, (N,), 2)
    off, step = ((6, 5), (0, 2 ** 32 + 1))[shared]
    got = policy.sample_gaussian(dev(torch, mean), dev(torch, ls_ref), seed=SEED, step=step, env_offset=off, out=(a, lp, en))
    _assert_equal(torch, got, _twin_at_scale(mean, ls_ref, SEED, step, off), (N, D, shared))
    for parent, lead, n, name in ((pa, 3, N * D, "actions"), (plp, 1, N, "log_prob"), (pen, 2, N, "entropy")):
        p = _guard_bits(torch, parent)
        assert np.all(p[:lead] == GUARD_F32) and np.all(p[lead + n:] == GUARD_F32), (D, shared, name)      # behind row N - 1 too


def test_overlapping_outputs_raise(torch):
    from gym_amd import policy

    N, D = 40, 2
    wide = torch.zeros((N, 8), device="cuda:0")
    mean, ls = wide[:, 0:2], torch.zeros(D, device="cuda:0")
    other = torch.zeros((N, D), device="cuda:0")
    flat = torch.zeros(3 * N, device="cuda:0")
    with pytest.raises(ValueError, match="actions overlaps the mean"):
        policy.sample_gaussian(mean, ls, seed=0, step=0, out=(wide[:, 4:6], None, None))      # interleaved with the mean's rows
    with pytest.raises(ValueError, match="log_prob overlaps the mean"):
        policy.sample_gaussian(mean, ls, seed=0, step=0, out=(other, wide.view(-1)[3:3 + N], None))
    with pytest.raises(ValueError, match="entropy overlaps the log_std"):
        policy.sample_gaussian(other, flat[:2 * N].view(N, D), seed=0, step=0, out=(torch.zeros((N, D), device="cuda:0"), None, flat[N:2 * N]))
    with pytest.raises(ValueError, match="outputs actions and log_prob overlap"):
        policy.sample_gaussian(mean, ls, seed=0, step=0, out=(flat[:2 * N].view(N, D), flat[2 * N - 1:3 * N - 1], None))
    with pytest.raises(ValueError, match="outputs log_prob and entropy overlap"):
        policy.sample_gaussian(mean, ls, seed=0, step=0, out=(other, flat[:N], flat[N - 1:2 * N - 1]))
    buf = torch.zeros(N + 8, device="cuda:0")                              # a counter inside the log_prob buffer
    counter = buf.view(torch.int64)[2:3]
    with pytest.raises(ValueError, match="log_prob overlaps step_dev"):
        policy.sample_gaussian(mean, ls, seed=0, step=counter, out=(other, buf[:N], None))
    torch.cuda.synchronize()
    assert int(counter.item()) == 0 and float(other.abs().sum()) == 0.0     # refused before anything was launched


@pytest.mark.parametrize("D", (1, 2, 4))
def test_degenerate_and_extreme_rows(torch, D):
    from gym_amd import policy

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
        for sv in (nan, 80.0001, -80.0001, inf, -inf):
            add(sv=sv, at=at)
    n_bad = len(mean)
    for at in range(D):
        for sv in (80.0, -80.0):
            add(sv=sv, at=at)
        for mv in (1e30, -1e30, 3e38, -3e38, 0.0, 1e-45):
            add(mv=mv, at=at)
    top = float(np.finfo(np.float32).max)                                   # sigma = EXP(80) = 5.5e34 is 5 000 of its ulps: about half the
    add(mv=top, sv=80.0)                                                    # draws round past the range
    add(mv=-top, sv=80.0)
    mean, ls = np.asarray(mean, np.float32), np.asarray(ls, np.float32)
    n_reps = 16                                                             # each row at 16 envs: other normals, some of them large
    mean, ls = np.tile(mean, (n_reps, 1)), np.tile(ls, (n_reps, 1))
    got = policy.sample_gaussian(dev(torch, mean), dev(torch, ls), seed=8, step=2, env_offset=3)
    want = gh.sample_gaussian(mean, ls, seed=8, step=2, env_offset=3)
    _assert_equal(torch, got, want, D)
    rows = len(mean) // n_reps
    bad = np.tile(np.arange(rows) < n_bad, n_reps)
    a, lp, en = (host_bits(torch, x) for x in got)
    assert np.all(a[bad] == 0x7FC00000) and np.all(lp[bad] == 0x7FC00000) and np.all(en[bad] == 0x7FC00000)
    assert not np.isnan(got[0].cpu().numpy()[~bad]).any() and not np.isnan(got[1].cpu().numpy()[~bad]).any()
    assert np.all(np.isfinite(got[2].cpu().numpy()[~bad]))
    # a float32 action past the range is +-Inf and its log_prob -Inf: what the arithmetic gives, not a NaN
    over = np.isinf(got[0].cpu().numpy()).any(1)
    assert over.any() and np.all(np.isneginf(got[1].cpu().numpy()[over]))


def _ulp32(v):
    return np.spacing(np.abs(v * (1 + 1e-6)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("D", DIMS)
def test_agreement_with_torch_distributions(torch, D):
    """log_prob and entropy against torch.distributions.Normal in float64 on the same float32 inputs and the float32 actions returned.

    With u = 2^-53 and E the exact value: the device equals the twin bit for bit, and the twin is held to
    |float32 result - E| <= ulp32(E) / 2 + BAR * u (tests/test_gaussian_host.py; BAR = bar(B_LOG_PROB), bar(B_ENTROPY)).
    torch evaluates -(x - mu)^2 / (2 sigma^2) - log sigma - log sqrt(2 pi) per dim and sums, with sigma = exp(ls) from libm, within 1 ulp
    (2u relative).  Per dim: the numerator carries 3u relative, sigma^2 5u, the quotient one more: 9u on zq^2 / 2, i.e. 4.5 u zq^2;
    log sigma carries the 2u of sigma plus one ulp of its result, <= 2u + 2u |ls|; the three subtractions and up to three additions
    of the sum each round at most u times the partial sum, which never exceeds sum_j (zq_j^2 / 2 + |ls_j| + 1): 6 of them.  Together
    <= u * sum_j (7.5 zq_j^2 + 8 |ls_j| + 8) <= 8u * sum_j (zq_j^2 + |ls_j| + 1).  The entropy has no quadratic term: 8u * sum_j (|ls_j| + 2).
    ulp32 is taken of the reference widened by 1e-6, which covers E on the other side of a power of two."""
    from gym_amd import policy

    rng = np.random.default_rng(90 + D)
    N = 4099
    mean, ls = _head(rng, N, D)
    md, lsd = dev(torch, mean), dev(torch, ls)
    act, lp, en = policy.sample_gaussian(md, lsd, seed=77, step=3, env_offset=2)
    dist = torch.distributions.Normal(md.double(), lsd.double().exp())
    ref_lp = dist.log_prob(act.double()).sum(-1).cpu().numpy()
    ref_en = dist.entropy().sum(-1).cpu().numpy()
    zq = gh.evaluate(mean, ls, gh.words(77, range(2, 2 + N), 3))["zq"]
    u = 2.0 ** -53
    abs_ls = np.abs(ls.astype(np.float64))
    tol_lp = _ulp32(ref_lp) / 2 + gh.bar(gh.B_LOG_PROB) * u + 8 * u * (zq * zq + abs_ls + 1).sum(1)
    tol_en = _ulp32(ref_en) / 2 + gh.bar(gh.B_ENTROPY) * u + 8 * u * (abs_ls + 2).sum(1)
    err_lp = np.abs(lp.cpu().numpy().astype(np.float64) - ref_lp)
    err_en = np.abs(en.cpu().numpy().astype(np.float64) - ref_en)
    print(f"D={D}: worst log_prob error / tolerance {np.max(err_lp / tol_lp):.3f}, entropy {np.max(err_en / tol_en):.3f}")
    assert np.all(err_lp <= tol_lp), (D, np.max(err_lp / tol_lp))
    assert np.all(err_en <= tol_en), (D, np.max(err_en / tol_en))
    # and the actions are mean + sigma z with standard normal z: zq is z up to the float32 rounding
    z = ((act.double() - md.double()) / lsd.double().exp()).cpu().numpy()
    assert np.abs(z).max() < gh.Z_MAX + 1e-3 and abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.var() - 1) < 5 * np.sqrt(2 / z.size)


def test_device_step_counter_under_graph_replay(torch):
    from gym_amd import policy

    N, D, calls, replays = 300, 3, 8, 3
    mean, ls = _head(np.random.default_rng(77), N, D)
    md, lsd = dev(torch, mean), dev(torch, ls[0])
    s = policy.GaussianSampler(D, seed=31, env_offset=2, device=0)
    rows = [torch.zeros((calls, N, D), device="cuda:0"), torch.zeros((calls, N), device="cuda:0"), torch.zeros((calls, N), device="cuda:0")]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for k in range(3):                                                  # eager: the counter advances by one per sample
            s.sample(md, lsd, out=(rows[0][0], rows[1][0], rows[2][0]))
            assert s.step_index() == k + 1
        s.load_state_dict(dict(s.state_dict(), step=0))
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for k in range(calls):
                s.sample(md, lsd, out=(rows[0][k], rows[1][k], rows[2][k]))
        got = []
        for _ in range(replays):
            g.replay()
            side.synchronize()
            got.append([r.clone() for r in rows])
    assert s.step_index() == calls * replays
    for i in range(calls * replays):
        eager = policy.sample_gaussian(md, lsd, seed=31, step=i, env_offset=2)
        graphed = tuple(r[i % calls] for r in got[i // calls])
        for a, b in zip(graphed, eager):
            assert np.array_equal(host_bits(torch, a), host_bits(torch, b)), i
        if i % 5 == 0:
            _assert_equal(torch, eager, gh.sample_gaussian(mean, ls[0], seed=31, step=i, env_offset=2), i)
    assert len({host_bits(torch, got[r][0][k]).tobytes() for r in range(replays) for k in range(calls)}) == calls * replays


def test_a_restored_sampler_continues_with_the_same_bits(torch):
    from gym_amd import policy

    mean, ls = _head(np.random.default_rng(78), 130, 4)
    md, lsd = dev(torch, mean), dev(torch, ls)
    s = policy.GaussianSampler(4, seed=2 ** 64 - 3, env_offset=2 ** 40 + 1)
    for _ in range(5):
        s.sample(md, lsd)
    state = s.state_dict()
    assert state["step"] == 5 and state["seed"] == 2 ** 64 - 3 and state["env_offset"] == 2 ** 40 + 1 and state["action_dim"] == 4
    fresh = policy.GaussianSampler(4)
    fresh.load_state_dict(state)
    for i in range(3):
        a, b = s.sample(md, lsd), fresh.sample(md, lsd)
        _assert_equal(torch, a, gh.sample_gaussian(mean, ls, seed=2 ** 64 - 3, step=5 + i, env_offset=2 ** 40 + 1), i)
        for x, y in zip(a, b):
            assert np.array_equal(host_bits(torch, x), host_bits(torch, y))
    assert s.step_index() == fresh.step_index() == 8
    with pytest.raises(ValueError, match="columns"):
        s.sample(md[:, :3], lsd[:, :3])
    with pytest.raises(ValueError, match="action_dim"):
        policy.GaussianSampler(3).load_state_dict(state)


@pytest.mark.parametrize("env_id", ["Pendulum-v1", "MountainCarContinuous-v0"])
def test_box_rollouts_eager_and_sharded(torch, env_id):
    from gym_amd.rollout import DeviceRollout

    n, K = 64, 12
    log_std = np.asarray([-0.5], np.float32)

    def run(num, off):
        r = DeviceRollout(env_id, num, seed=4, action_seed=9, env_offset=off)
        r.reset(seed=4)
        s = r.gaussian_sampler()
        assert (s.action_dim, s.seed, s.env_offset, s.device) == (1, 9, off, r.device)
        assert r.gaussian_sampler(seed=12).seed == 12
        W = torch.from_numpy(np.random.default_rng(1).standard_normal((r.O, 1)).astype(np.float32)).to(r.device)
        lsd = torch.from_numpy(log_std).to(r.device)
        acts, obs, heads = [], [], []
        with torch.cuda.stream(r.stream):
            for _ in range(K):
                mean = r.obs @ W
                a, lp, en = s.sample(mean, lsd)
                assert tuple(a.shape) == (num, 1) and a.dtype == r.action_dtype
                heads.append((mean.clone(), lp, en))
                r.step(a)
                acts.append(a.clone())
                obs.append(r.obs.clone())
        r.synchronize()
        assert s.step_index() == K
        r.close()
        return torch.stack(acts), torch.stack(obs), heads

    acts, obs, heads = run(n, 0)
    for t in (0, K - 1):                                                    # the draws are the twin's for the means the device computed
        want = gh.sample_gaussian(heads[t][0].cpu().numpy(), log_std, seed=9, step=t)
        _assert_equal(torch, (acts[t], heads[t][1], heads[t][2]), want, (env_id, t))
    assert torch.isfinite(obs).all() and float(acts.std()) > 0.1
    parts = [run(n // 2, off)[:2] for off in (0, n // 2)]
    assert torch.equal(torch.cat((parts[0][0], parts[1][0]), dim=1), acts)
    assert torch.equal(torch.cat((parts[0][1], parts[1][1]), dim=1), obs)


def test_each_sampler_names_the_other_for_the_wrong_action_space(torch):
    from gym_amd.rollout import DeviceRollout

    r = DeviceRollout("CartPole-v1", 8)
    with pytest.raises(ValueError, match=r"policy_sampler\(\)"):
        r.gaussian_sampler()
    r.close()
    r = DeviceRollout("Pendulum-v1", 8)
    with pytest.raises(ValueError, match="Gaussian") as e:
        r.policy_sampler()
    assert "gaussian_sampler()" in str(e.value)
    r.close()


def test_the_example_prints_the_same_history_twice(torch, capsys):
    import os
    import sys

    from conftest import ROOT

    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import actor_critic_gaussian
    finally:
        sys.path.pop(0)
    printed = []
    for _ in range(2):
        h = actor_critic_gaussian.train(256, 2, K=16)
        printed.append(capsys.readouterr().out)
        assert len(h) == 2 and all(np.isfinite(list(row.values())).all() for row in h)
        assert h[0]["mean_entropy"] == pytest.approx(-0.5 + float(gh.ENT_C), abs=1e-6) and h[0]["mean_log_prob"] < 0
    assert printed[0] == printed[1] and "iteration   1" in printed[0] and f"{3 + 2 * 16} policy steps drawn" in printed[0]
