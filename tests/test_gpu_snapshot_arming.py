"""ShardedRollout arms the fused kernel's in-kernel final snapshot (mxv_set_final_snapshot) only once a gather has been asked for
(DESIGN.md §7): a job that never gathers never pays the second set of stores; the first gather copies the final tensors and switches
arming on; gathers return the same tensors in both states.  World size 1.  What is attached, and whether a launch was handed the
buffers as kernel arguments, is read from the native handle (mxv_last_launch_snapshot) through last_launch()["snapshot"] and
Handle.final_snapshot_attached — not from what the Python front end believes it did."""
import pytest

pytestmark = pytest.mark.gpu


def _equal(got, want):
    import torch

    return all(torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("comm", ["torch", "mxv"])
def test_the_snapshot_is_attached_by_the_first_gather_and_gathers_are_equal_in_both_states(comm):
    import torch
    from gym_amd.distributed import ShardedRollout

    n, K = 1000, 6
    sr = ShardedRollout("CartPole-v1", n, rank=0, world_size=1, device=0, seed=3, action_seed=4, comm=comm, max_episode_steps=9)
    h = sr.engine.handle
    sr.reset(seed=3)
    out = sr.engine.trajectory_buffers(K, layout="separate")
    for _ in range(3):                                          # no gather requested yet: nothing attached, whatever the call
        sr.rollout_per_step(K, out=out)
        li = h.last_launch()
        assert li["kernel"] == 1 and li["snapshot"] == 0 and not h.final_snapshot_attached and sr._snap is None, li
        sr.rollout(K)
        assert h.last_launch()["snapshot"] == 0 and not h.final_snapshot_attached
    sr.synchronize()

    def gathered_equals_finals(what):
        sr.synchronize()
        want = [t.clone() for t in sr.engine.final_tensors()]
        got = list(sr.gather())
        sr.synchronize()
        torch.cuda.synchronize()
        assert _equal(got, want), (comm, what)

    gathered_equals_finals("first gather: never armed, the finals are copied")
    assert not h.final_snapshot_attached                        # attached by the next rollout, not by the gather
    for alternation in range(3):
        sr.rollout_per_step(K, out=out)                         # armed: deposits in-kernel, into the set the last gather did not read
        li = h.last_launch()
        assert h.final_snapshot_attached and sr._cur_written and li["kernel"] == 1 and li["snapshot"] == 1, li
        gathered_equals_finals(f"alternation {alternation}: in-kernel deposit")
        if alternation == 1:
            gathered_equals_finals("a second gather of the same chunk: copied again")
        sr.rollout(K)
        assert sr._cur_written and h.last_launch()["snapshot"] == 1
        gathered_equals_finals(f"alternation {alternation}: in-kernel deposit of rollout()")
    sr.close()


def test_a_job_that_never_gathers_leaves_the_snapshot_detached_at_the_drivers_size():
    """2^17 + 128 envs (two envs per lane, the driver's instantiation), the driver's K: nothing attached, no snapshot buffers allocated."""
    from gym_amd.distributed import ShardedRollout

    n = (1 << 17) + 128
    sr = ShardedRollout("CartPole-v1", n, rank=0, world_size=1, device=0, seed=0, action_seed=1)
    sr.reset(seed=0)
    out = sr.engine.trajectory_buffers(20, layout="separate")
    for _ in range(2):
        sr.rollout_per_step(20, mode="fused", out=out, record_actions=True)
    sr.synchronize()
    li = sr.engine.handle.last_launch()
    assert li["kernel"] == 1 and li["envs_per_lane"] == 2 and li["steps"] == 20 and li["snapshot"] == 0, li
    assert not sr.engine.handle.final_snapshot_attached and sr._snap is None and not sr._cur_written
    sr.close()


def test_the_getter_reads_the_handle_not_the_python_wrapper():
    """Buffers attached behind the wrapper's back (the C entry point called directly) are seen; a fused launch reports that it was handed
    them, a launch of single steps (which copies the snapshot afterwards) and a launch after detaching report that they were not."""
    import torch
    from gym_amd import _native
    from gym_amd.rollout import DeviceRollout

    n, K = 1000, 4
    r = DeviceRollout("CartPole-v1", n, seed=1, action_seed=2)
    r.reset(seed=1)
    h = r.handle
    assert not h.final_snapshot_attached and h.last_launch()["snapshot"] == 0
    with torch.cuda.stream(r.stream):
        snap = [torch.empty_like(t) for t in (r.obs, r.reward, r.terminated, r.truncated)]
    r.stream.synchronize()
    h._check(_native.lib.mxv_set_final_snapshot(h._h, *(t.data_ptr() for t in snap)))
    assert h.final_snapshot_attached and h.last_launch()["snapshot"] == 0          # attached, but no launch has run with it yet
    out = r.rollout_per_step(K, mode="fused")
    assert h.last_launch()["kernel"] == 1 and h.last_launch()["snapshot"] == 1
    r.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(snap[0], out["obs"][K - 1]) and torch.equal(snap[2], out["terminated"][K - 1])
    r.rollout_per_step(K, mode="eager", out=out)
    assert h.last_launch()["kernel"] == 0 and h.last_launch()["snapshot"] == 0 and h.final_snapshot_attached
    h.set_final_snapshot()
    r.rollout_per_step(K, mode="fused", out=out)
    assert h.last_launch()["kernel"] == 1 and h.last_launch()["snapshot"] == 0 and not h.final_snapshot_attached
    r.synchronize()
    r.close()
