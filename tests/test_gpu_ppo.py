"""gym_amd.ppo_clip_loss / gym_amd.advantage_moments on the device against tests/ppo_host.py, bit for bit — the loss, the eight
diagnostics, the three gradients and the moments: every size at which the tree changes shape (a partial wave, a partial workgroup, a
partial leaf, two leaves, the third launch), each optional input absent in turn, with and without the normalisation, leading dims,
non-finite rows, an incoming gradient other than 1; the samplers' own bits (ratio exactly 1); the allocation-free forward recorded in
a graph; the launch counts and the absence of a synchronisation; the fused PPO example end to end."""
import ctypes
import os
import sys

import numpy as np
import pytest

import ppo_host as pp
from conftest import ROOT
from ppo_host import bits, to_f32
from test_ppo_host import CLIP, ENTROPY_COEF, EPS, VALUE_COEF, make_batch

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099, 1024 * 1024 + 5)      # the last: the smallest that takes the third launch
GRAD = 2.5


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host_bits(torch, x):
    return x.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1)


def host_bits64(torch, x):
    return x.detach().contiguous().view(torch.int64).cpu().numpy().view(np.uint64).reshape(-1)


def _same32(torch, got, want64, what):
    assert got.dtype == torch.float32, what
    want = bits(to_f32(np.asarray(want64, np.float64).reshape(-1)))
    have = host_bits(torch, got)
    assert have.shape == want.shape and np.array_equal(have, want), (what, have[:8], want[:8])


def check(torch, b, *, moments=True, entropy=True, values=True, shape=None, what=None):
    """One forward and one backward of the device on the batch `b` against the twin: everything bit for bit.  -> stats (host)."""
    import gym_amd

    M = b["lp"].shape[0]
    view = (lambda x: x) if shape is None else (lambda x: x.view(shape))
    lp, old, adv = (view(dev(torch, b[k])) for k in ("lp", "old", "adv"))
    ent = view(dev(torch, b["ent"])) if entropy else None
    val, ret = (view(dev(torch, b["val"])), view(dev(torch, b["ret"]))) if values else (None, None)
    mom_h = mom_d = None
    if moments:
        mom_d = gym_amd.advantage_moments(adv, eps=EPS)
        mom_h = pp.advantage_moments(b["adv"], EPS)
        assert mom_d.dtype == torch.float64 and tuple(mom_d.shape) == (2,)
        assert np.array_equal(host_bits64(torch, mom_d), mom_h.view(np.uint64)), (what, M, mom_d.cpu().numpy(), mom_h)
    kw_h = dict(clip=CLIP, moments=mom_h, entropy=b["ent"] if entropy else None, entropy_coef=ENTROPY_COEF,
                values=b["val"] if values else None, returns=b["ret"] if values else None, value_coef=VALUE_COEF)
    want_loss, want_stats = pp.clip_loss_f32(b["lp"], b["old"], b["adv"], **kw_h)
    want_g = pp.clip_loss_backward(b["lp"], b["old"], b["adv"], np.float32(GRAD), **kw_h)
    lp.requires_grad_()
    if entropy:
        ent.requires_grad_()
    if values:
        val.requires_grad_()
    loss, stats = gym_amd.ppo_clip_loss(lp, old, adv, clip=CLIP, moments=mom_d, entropy=ent, entropy_coef=ENTROPY_COEF, values=val, returns=ret,
                                        value_coef=VALUE_COEF)
    assert loss.dim() == 0 and loss.requires_grad and tuple(stats.shape) == (8,) and not stats.requires_grad
    _same32(torch, loss, [want_loss], (what, M, "loss"))
    _same32(torch, stats, want_stats, (what, M, "stats"))
    (GRAD * loss).backward()
    for name, leaf, want in (("log_prob", lp, want_g[0]), ("entropy", ent, want_g[1]), ("values", val, want_g[2])):
        if leaf is None:
            continue
        assert tuple(leaf.grad.shape) == tuple(leaf.shape), (what, M, name)
        _same32(torch, leaf.grad, want, (what, M, "grad " + name))
    # the same forward without autograd, into the caller's tensors
    out = (torch.empty((), device="cuda:0"), torch.empty(8, device="cuda:0"))
    with torch.no_grad():
        got = gym_amd.ppo_clip_loss(lp, old, adv, clip=CLIP, moments=mom_d, entropy=ent, entropy_coef=ENTROPY_COEF, values=val, returns=ret,
                                    value_coef=VALUE_COEF, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    _same32(torch, out[0], [want_loss], (what, M, "out loss"))
    _same32(torch, out[1], want_stats, (what, M, "out stats"))
    return stats.cpu().numpy()


# ---- every size ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", SIZES)
def test_loss_stats_gradients_and_moments_match_the_twin(torch, M):
    b = make_batch(M, 2000 + M % 1000)
    check(torch, b, moments=True, what="normalised")
    check(torch, b, moments=False, what="as given")


@pytest.mark.parametrize("M", (257, 4099))
def test_each_optional_input_absent_in_turn(torch, M):
    b = make_batch(M, 31)
    for moments in (True, False):
        check(torch, b, moments=moments, entropy=False, what="no entropy")
        check(torch, b, moments=moments, values=False, what="no values")
        check(torch, b, moments=moments, entropy=False, values=False, what="surrogate alone")


def test_only_the_inputs_that_require_grad_get_one(torch):
    import gym_amd

    M = 1500
    b = make_batch(M, 32)
    lp, old, adv, ent, val, ret = (dev(torch, b[k]) for k in ("lp", "old", "adv", "ent", "val", "ret"))
    kw_h = dict(clip=CLIP, entropy=b["ent"], entropy_coef=ENTROPY_COEF, values=b["val"], returns=b["ret"], value_coef=VALUE_COEF)
    want = pp.clip_loss_backward(b["lp"], b["old"], b["adv"], np.float32(1.0), **kw_h)
    for k, name in enumerate(("log_prob", "entropy", "values")):
        leaves = [lp.clone(), ent.clone(), val.clone()]
        leaves[k].requires_grad_()
        loss, _ = gym_amd.ppo_clip_loss(leaves[0], old, adv, clip=CLIP, entropy=leaves[1], entropy_coef=ENTROPY_COEF, values=leaves[2], returns=ret,
                                        value_coef=VALUE_COEF)
        loss.backward()
        _same32(torch, leaves[k].grad, want[k], name)
        assert all(x.grad is None for i, x in enumerate(leaves) if i != k)
    with pytest.raises(ValueError, match="requires grad"):
        gym_amd.ppo_clip_loss(lp.clone().requires_grad_(), old, adv, out=(torch.empty((), device="cuda:0"), torch.empty(8, device="cuda:0")))
    with pytest.raises(ValueError, match="workspace holds"):
        gym_amd.ppo_clip_loss(lp, old, adv, workspace=torch.empty(64, dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(ValueError, match="moments must be a device tensor"):
        gym_amd.ppo_clip_loss(lp, old, adv, moments=torch.zeros(2, dtype=torch.float64))


def test_leading_dims(torch):
    K, N = 3, 65
    b = make_batch(K * N, 33)
    check(torch, b, shape=(K, N), what="[K, N]")
    check(torch, b, moments=False, shape=(K, 5, 13), what="[K, 5, 13]")


# ---- non-finite rows ----------------------------------------------------------------------------------------------------------------------------
def test_nan_inf_and_saturated_rows(torch):
    inf, nan = np.inf, np.nan
    b = make_batch(2100, 34)
    edits = (("lp", 5, nan), ("old", 300, nan), ("adv", 700, nan), ("lp", 1030, inf), ("lp", 1031, -inf), ("old", 1032, inf), ("old", 1033, -inf),
             ("lp", 1034, 200.0), ("lp", 1035, -200.0), ("adv", 1500, inf), ("adv", 1501, -inf), ("ent", 1600, nan), ("val", 1700, inf), ("ret", 1800, nan))
    # one kind at a time (the finite ones together): what each does to the loss, the diagnostics and the gradients is the twin's
    finite = dict(lp=b["lp"].copy(), old=b["old"].copy(), adv=b["adv"].copy(), ent=b["ent"], val=b["val"], ret=b["ret"])
    for field, i, v in edits[3:9]:
        finite[field][i] = v
    stats = check(torch, finite, moments=False, what="saturated")
    assert stats[pp.STAT_NAMES.index("ratio_max")] == np.float32(pp.EXP(80.0)) and stats[pp.STAT_NAMES.index("ratio_min")] == np.float32(pp.EXP(-80.0))
    assert np.isfinite(stats).all()
    for field, i, v in edits[:3] + edits[9:]:
        c = {k: x.copy() for k, x in b.items()}
        c[field][i] = v
        check(torch, c, moments=False, what=(field, v))
        check(torch, c, moments=True, what=(field, v, "normalised"))
    both = {k: x.copy() for k, x in b.items()}
    both["lp"][7], both["old"][7] = inf, inf           # Inf - Inf: a NaN d
    both["lp"][:3] = nan
    stats = check(torch, both, moments=False, what="inf - inf")
    assert np.isnan(stats[0]) and np.isfinite(stats[5:]).all()
    none = dict(make_batch(3, 35), lp=np.full(3, nan, np.float32))
    stats = check(torch, none, moments=False, what="no ratio")
    assert stats[6] == inf and stats[7] == -inf


# ---- the probability ratio of an unchanged policy is 1 --------------------------------------------------------------------------------------------
def test_on_the_samplers_own_outputs_the_ratio_is_one_and_the_kl_zero(torch):
    import gym_amd

    M, A = 4099, 6
    rng = np.random.default_rng(36)
    logits = dev(torch, (rng.standard_normal((M, A)) * 2).astype(np.float32))
    adv = dev(torch, rng.standard_normal(M).astype(np.float32))
    act, old_lp, old_en = gym_amd.sample_categorical(logits, seed=5, step=2)
    x = logits.clone().requires_grad_()
    lp, en = gym_amd.evaluate_categorical(x, act)
    loss, stats = gym_amd.ppo_clip_loss(lp, old_lp, adv, clip=CLIP, moments=gym_amd.advantage_moments(adv), entropy=en, entropy_coef=ENTROPY_COEF)
    loss.backward()
    s = stats.cpu().numpy()
    assert s[6] == 1.0 and s[7] == 1.0 and s[3] == 0.0 and s[4] == 0.0 and s[5] == 0.0 and np.isfinite(s).all()
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0.0
    mom = pp.advantage_moments(adv.cpu().numpy())
    want, _ = pp.clip_loss_f32(old_lp.cpu().numpy(), old_lp.cpu().numpy(), adv.cpu().numpy(), clip=CLIP, moments=mom, entropy=old_en.cpu().numpy(),
                               entropy_coef=ENTROPY_COEF)
    assert host_bits(torch, loss)[0] == bits(np.array([want]))[0]


# ---- graph capture, launch counts, no synchronisation ------------------------------------------------------------------------------------------
def test_the_allocation_free_forward_replays_in_a_captured_graph(torch):
    import gym_amd
    from gym_amd import ppo

    M = 5000
    batches = [make_batch(M, 40 + k) for k in range(3)]
    keys = ("lp", "old", "adv", "ent", "val", "ret")
    bufs = {k: dev(torch, batches[0][k]) for k in keys}
    mom = torch.empty(2, dtype=torch.float64, device="cuda:0")
    ws = torch.empty(ppo.workspace_bytes(M), dtype=torch.uint8, device="cuda:0")
    out = (torch.empty((), device="cuda:0"), torch.empty(8, device="cuda:0"))

    def step():
        gym_amd.advantage_moments(bufs["adv"], eps=EPS, out=mom, workspace=ws)
        gym_amd.ppo_clip_loss(bufs["lp"], bufs["old"], bufs["adv"], clip=CLIP, moments=mom, entropy=bufs["ent"], entropy_coef=ENTROPY_COEF,
                              values=bufs["val"], returns=bufs["ret"], value_coef=VALUE_COEF, workspace=ws, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                # warm-up outside the capture
        side.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        step()
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before      # with out= and workspace= the calls allocate nothing
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            step()
        for k in (1, 2):
            for name in keys:
                bufs[name].copy_(dev(torch, batches[k][name]))
            g.replay()
            side.synchronize()
            b = batches[k]
            mom_h = pp.advantage_moments(b["adv"], EPS)
            want_loss, want_stats = pp.clip_loss_f32(b["lp"], b["old"], b["adv"], clip=CLIP, moments=mom_h, entropy=b["ent"], entropy_coef=ENTROPY_COEF,
                                                     values=b["val"], returns=b["ret"], value_coef=VALUE_COEF)
            assert np.array_equal(host_bits64(torch, mom), mom_h.view(np.uint64)), k
            _same32(torch, out[0], [want_loss], k)
            _same32(torch, out[1], want_stats, k)
    torch.cuda.current_stream().wait_stream(side)


def _hip():
    """The HIP runtime this process already uses (torch's), for the stream-capture calls."""
    paths = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert len(paths) == 1, paths
    hip = ctypes.CDLL(paths[0])
    vp = ctypes.c_void_p
    hip.hipStreamBeginCapture.argtypes = [vp, ctypes.c_int]
    hip.hipStreamEndCapture.argtypes = [vp, ctypes.POINTER(vp)]
    hip.hipGraphGetNodes.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphDestroy.argtypes = [vp]
    return hip


def _captured_launches(hip, stream, call):
    """Records `call` (entry points of the library on `stream`) into a hipGraph and -> (its status, the number of nodes).  Nothing runs;
    a synchronisation or any other call that a capture forbids would fail the capture."""
    graph = ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 1) == 0                          # hipStreamCaptureModeThreadLocal
    try:
        rc = call()
    finally:
        end = hip.hipStreamEndCapture(stream, ctypes.byref(graph))
    assert end == 0 and graph.value, end
    n = ctypes.c_size_t()
    try:
        assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    finally:
        hip.hipGraphDestroy(graph)
    return rc, n.value


@pytest.mark.parametrize("M", (3, 1024, 4099, 1024 * 1024, 1024 * 1024 + 5))
def test_launch_counts_and_no_synchronisation(torch, M):
    """2 launches forwards up to 2^20 rows, 3 beyond; the same for the moments; 1 backwards — counted as the kernel nodes that the calls
    leave in a stream capture, which also shows that they neither synchronise nor allocate."""
    from gym_amd import ppo

    hip = _hip()
    f32 = dict(dtype=torch.float32, device="cuda:0")
    lp, old, adv, ent, val, ret, g_lp, g_en, g_val = (torch.zeros(M, **f32) for _ in range(9))
    mom = torch.zeros(2, dtype=torch.float64, device="cuda:0")
    ws = torch.empty(ppo.workspace_bytes(M), dtype=torch.uint8, device="cuda:0")
    loss, stats, g = torch.empty((), **f32), torch.empty(8, **f32), torch.ones((), **f32)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = side.cuda_stream
    lib = ppo.lib
    want = 2 if M <= 1024 * 1024 else 3
    assert ppo.launches(M) == pp.launches(M) == want
    ins = (lp.data_ptr(), old.data_ptr(), adv.data_ptr(), mom.data_ptr(), ent.data_ptr(), val.data_ptr(), ret.data_ptr())
    calls = ((lambda: lib.mxv_ppo_advantage_moments(s, M, adv.data_ptr(), EPS, ws.data_ptr(), ws.numel(), mom.data_ptr()), want),
             (lambda: lib.mxv_ppo_clip_loss(s, M, *ins, CLIP, ENTROPY_COEF, VALUE_COEF, ws.data_ptr(), ws.numel(), loss.data_ptr(), stats.data_ptr()), want),
             (lambda: lib.mxv_ppo_clip_loss_backward(s, M, *ins, CLIP, ENTROPY_COEF, VALUE_COEF, g.data_ptr(), g_lp.data_ptr(), g_en.data_ptr(),
                                                     g_val.data_ptr()), 1))
    for call, _ in calls:                                                     # once outside a capture: the kernels' code is loaded
        assert call() == 0, lib.mxv_ppo_last_error()
    side.synchronize()
    for call, nodes in calls:
        rc, n = _captured_launches(hip, s, call)
        assert (rc, n) == (0, nodes), (rc, n, lib.mxv_ppo_last_error())
    side.synchronize()


# ---- the example --------------------------------------------------------------------------------------------------------------------------------
def test_the_fused_ppo_example_starts_every_iteration_at_ratio_one(torch, capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import ppo_clip_fused
    finally:
        sys.path.pop(0)
    h = ppo_clip_fused.train(256, 2, K=16)
    printed = capsys.readouterr().out
    assert len(h) == 2 and "iteration   1" in printed and f"{3 + 2 * 16} policy steps drawn" in printed
    for row in h:
        first = row["epochs"][0]
        assert first["ratio_min"] == 1.0 and first["ratio_max"] == 1.0 and first["approx_kl"] == 0.0 and first["approx_kl3"] == 0.0
        assert first["clip_fraction"] == 0.0 and len(row["epochs"]) == 4
        assert all(np.isfinite(list(e.values())).all() for e in row["epochs"])      # every loss and every diagnostic
        assert row["epochs"][-1]["ratio_max"] > 1.0 > row["epochs"][-1]["ratio_min"]      # and the later epochs have moved
