"""What gym_amd.gae, gym_amd.discounted_returns and gym_amd.vtrace share (gym_amd/csrc/mxv_trajectory.hpp), on the device: the walk over
the K rows behind the register ring at every remainder of its group loop, and the two families' separate records of their last launch.
Bit for bit against tests/gae_host.py and tests/vtrace_host.py; the V = 4 path, the alignment classes and the special values have their
tests in tests/test_gpu_gae.py and tests/test_gpu_vtrace.py."""
import numpy as np
import pytest

import gae_host
import vtrace_host
from test_vtrace_host import random_case

pytestmark = pytest.mark.gpu

N = 257          # one full tile of 256 lanes and one lane of a second
LEVELS = dict(gamma=0.97, lam=0.9, rho_bar=1.5, c_bar=0.8, pg_rho_bar=1.2)


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host_bits(torch, x):
    return x.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def test_the_two_families_keep_separate_records_of_their_last_launch(torch):
    import gym_amd
    from gym_amd import returns, vtrace

    small, wide = random_case(3, 5, 1), random_case(3, 300, 2)
    s, w = ({k: dev(torch, v) for k, v in c.items()} for c in (small, wide))

    def gae():
        gym_amd.gae(s["reward"], s["terminated"], s["truncated"], s["values"], s["last_value"])

    def vt():
        gym_amd.vtrace(w["log_prob"], w["old_log_prob"], w["reward"], w["terminated"], w["truncated"], w["values"], w["last_value"])

    for first, second in ((gae, vt), (vt, gae)):
        first()
        second()
        assert returns.last_launch() == (1, 1) and vtrace.last_launch() == (1, 2)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def masters(torch):
    """reward dtype -> (the host arrays of the longest case, their device copies)"""
    from gym_amd.returns import RING_DEPTH

    out = {}
    for dtype, seed in ((np.float32, 41), (np.float64, 42)):
        c = random_case(2 * (RING_DEPTH + 1) + 1, N, seed, dtype, p=0.15)
        out[dtype] = (c, {k: dev(torch, v) for k, v in c.items()})
    return out


@pytest.mark.parametrize("reward_dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("with_final, with_last", [(True, True), (False, True), (True, False), (False, False)])
def test_every_remainder_of_the_group_loop_is_bit_equal_to_the_twins(torch, masters, reward_dtype, with_final, with_last):
    """K = 1 ... 2 (RING_DEPTH + 1) + 1: the prologue's overfetch at K < RING_DEPTH, none to two full groups, every count of remainder
    steps; N = 257: a partial second tile.  The first K rows of one master case, for all three functions."""
    import gym_amd
    from gym_amd import returns, vtrace

    master, dm = masters[reward_dtype]
    K_max = master["reward"].shape[0]
    assert K_max == 2 * (returns.RING_DEPTH + 1) + 1 == 11 and vtrace.RING_DEPTH == returns.RING_DEPTH
    flags = master["terminated"].astype(bool) | master["truncated"].astype(bool)
    assert flags.any() and not flags.all() and (master["truncated"].astype(bool) & ~master["terminated"].astype(bool)).any()
    for K in range(1, K_max + 1):
        c = {k: np.ascontiguousarray(v[:K]) if v.ndim == 2 else v for k, v in master.items()}
        d = {k: v[:K].contiguous() if v.dim() == 2 else v for k, v in dm.items()}
        lv, fv = ("last_value" if with_last else None), ("final_values" if with_final else None)
        pick = lambda x, k: x[k] if k else None
        want = {
            "gae": gae_host.gae(c["reward"], c["terminated"], c["truncated"], c["values"], pick(c, lv), gamma=0.97, lam=0.9, final_values=pick(c, fv)),
            "returns": (gae_host.discounted_returns(c["reward"], c["terminated"], c["truncated"], gamma=0.97, last_value=pick(c, lv),
                                                    final_values=pick(c, fv)),),
            "vtrace": vtrace_host.vtrace(c["log_prob"], c["old_log_prob"], c["reward"], c["terminated"], c["truncated"], c["values"], pick(c, lv),
                                         final_values=pick(c, fv), **LEVELS),
        }
        got = {
            "gae": gym_amd.gae(d["reward"], d["terminated"], d["truncated"], d["values"], pick(d, lv), gamma=0.97, lam=0.9, final_values=pick(d, fv)),
            "returns": (gym_amd.discounted_returns(d["reward"], d["terminated"], d["truncated"], gamma=0.97, last_value=pick(d, lv),
                                                   final_values=pick(d, fv)),),
            "vtrace": gym_amd.vtrace(d["log_prob"], d["old_log_prob"], d["reward"], d["terminated"], d["truncated"], d["values"], pick(d, lv),
                                     final_values=pick(d, fv), **LEVELS),
        }
        assert returns.last_launch() == (1, 2) and vtrace.last_launch() == (1, 2)
        for name in want:
            assert len(got[name]) == len(want[name])
            for i, (g, w) in enumerate(zip(got[name], want[name])):
                assert g.dtype == torch.float32 and tuple(g.shape) == (K, N) == w.shape
                bad = np.argwhere(host_bits(torch, g) != vtrace_host.bits(w))
                assert bad.size == 0, f"K={K} {name} output {i}: {len(bad)} of {w.size} differ, first at {bad[0]}"
