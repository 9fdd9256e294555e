"""The handle's error latch (gym_amd/csrc/mxv_host.hpp: alloc_latch, take_latched): kernels raise their single-bit codes with plain stores
into pinned host memory, the host reads and clears the words after the stream synchronisation — no copy command.  What callers see is
unchanged: an error raised by any launch since the last synchronisation is reported by the next one, exactly once, with its own code and
message, and the latch is clear afterwards.  Every path here is one of the library's validated error paths (an out-of-range Discrete action,
an out-of-range frame index): nothing faults."""
import pytest

pytestmark = pytest.mark.gpu


def _tape(r, K, victim, value=7):
    """K rows of action 0, one entry set to `value`."""
    import torch

    tape = torch.zeros((K, r.num_envs), dtype=r.action_dtype, device=r.device)
    tape[K // 2, victim] = value
    torch.cuda.synchronize()
    return tape


@pytest.mark.parametrize("n", [1000, (1 << 17) + 128])
def test_a_tape_with_one_bad_action_is_reported_once_by_the_next_synchronise(n):
    from gym_amd.rollout import DeviceRollout

    r = DeviceRollout("CartPole-v1", n, seed=1, action_seed=2)
    r.reset(seed=1)
    r.synchronize()
    good = _tape(r, 6, 0, value=1)
    r.rollout_tape(good)
    r.synchronize()                                     # nothing latched
    r.rollout_tape(_tape(r, 6, n - 3))
    r.rollout_tape(good)                                # a clean launch behind it does not clear the latch
    with pytest.raises(AssertionError) as e:
        r.synchronize()
    assert "Discrete.contains" in str(e.value)
    r.synchronize()                                     # reported once: the latch is clear
    r.rollout_tape(good)
    r.synchronize()
    r.close()


def test_step_with_a_bad_action_is_reported_once():
    import torch
    from gym_amd.rollout import DeviceRollout

    n = 1000
    r = DeviceRollout("MountainCar-v0", n, seed=1, action_seed=2)
    r.reset(seed=1)
    acts = torch.zeros(n, dtype=r.action_dtype, device=r.device)
    bad = acts.clone()
    bad[n - 1] = 3
    torch.cuda.synchronize()
    r.step(acts)
    r.synchronize()
    r.step(bad)
    with pytest.raises(AssertionError):
        r.synchronize()
    r.synchronize()
    r.step(acts)
    r.synchronize()
    r.close()


@pytest.mark.parametrize("compact", [False, True])
def test_a_tabular_rollout_with_a_bad_action_is_reported_once(compact):
    import torch
    from gym_amd import _native
    from gym_amd.toy_text import TabularRollout

    n, K = 3000, 5
    r = TabularRollout("FrozenLake-v1", n, seed=3, action_seed=4, compact=compact)
    r.reset(seed=3)
    tape = torch.zeros((K, n), dtype=r.int_dtype, device=r.device)
    bad = tape.clone()
    bad[2, 1234] = 4                                    # Discrete(4)
    torch.cuda.synchronize()
    out = r.trajectory_buffers(K, layout="separate")
    r.rollout_tape(tape, out=out)
    r.synchronize()
    r.rollout_tape(bad, out=out)
    with pytest.raises(_native.MxvError) as e:
        r.synchronize()
    assert e.value.code == _native.ERR_INVALID_ACTION
    r.synchronize()
    r.rollout_per_step(K, out=out)
    r.synchronize()
    r.close()


def test_a_blackjack_rollout_with_a_bad_action_is_reported_once():
    import torch
    from gym_amd import _native
    from gym_amd.toy_text import BlackjackRollout

    n, K = 3000, 5
    r = BlackjackRollout(n, seed=5, action_seed=6)
    r.reset(seed=5)
    tape = torch.zeros((K, n), dtype=torch.int64, device=r.device)
    bad = tape.clone()
    bad[4, 17] = 2                                      # Discrete(2)
    torch.cuda.synchronize()
    out = r.trajectory_buffers(K, layout="separate")
    r.rollout_tape(tape, out=out)
    r.synchronize()
    r.rollout_tape(bad, out=out)
    with pytest.raises(_native.MxvError) as e:
        r.synchronize()
    assert e.value.code == _native.ERR_INVALID_ACTION
    r.synchronize()
    r.rollout_per_step(K, out=out)
    r.synchronize()
    r.close()


def test_a_render_index_error_keeps_its_own_message_and_shares_one_report_with_a_bad_action():
    import torch
    from gym_amd import _native, _render
    from gym_amd.rollout import DeviceRollout

    n = 300
    r = DeviceRollout("CartPole-v1", n, seed=1, action_seed=2)
    r.reset(seed=1)
    h = r.handle
    with torch.cuda.stream(r.stream):
        idx = torch.tensor([1, n, -1, 2], dtype=torch.int32, device=r.device)
        frames = torch.full((4, 400, 600, 3), 7, dtype=torch.uint8, device=r.device)
    r.stream.synchronize()
    # the render error alone: its own code and message, once
    _render.render_device(h, frames, idx)
    with pytest.raises(_native.MxvError) as e:
        h.sync()
    assert e.value.code == _native.ERR_INVALID_ARG and "render: env index outside [0, 300)" in e.value.message
    got = frames.cpu().numpy()
    assert got[0].any() and got[3].any() and not got[1].any() and not got[2].any()       # the bad frames were written as zeros
    h.sync()
    # a bad action and a bad frame index before one synchronisation: one error covers both, and the next synchronisation is clean
    r.rollout_tape(_tape(r, 4, 5))
    _render.render_device(h, frames, idx)
    with pytest.raises(_native.MxvError) as e:
        h.sync()
    assert e.value.code == _native.ERR_INVALID_ACTION
    h.sync()
    _render.render_device(h, frames, idx[:1])
    h.sync()
    r.close()


def test_the_latch_survives_a_launch_recorded_in_a_graph_and_replayed():
    import torch
    from gym_amd.rollout import DeviceRollout

    n, K = 1000, 4
    r = DeviceRollout("CartPole-v1", n, seed=1, action_seed=2)
    r.reset(seed=1)
    tape = _tape(r, K, 0, value=1)
    out = r.trajectory_buffers(K, layout="separate")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(r.stream):
        r.enable_graph_capture()
        r.rollout_tape(tape, out=out)                   # once outside the capture
        r.stream.synchronize()
        with torch.cuda.graph(g, stream=r.stream):
            r.rollout_tape(tape, out=out)
        g.replay()
    r.synchronize()                                     # valid tape: nothing latched
    tape[1, 999] = -1                                   # the recorded launch reads the same buffer: now it holds a bad action
    torch.cuda.synchronize()
    for _ in range(2):                                  # every replay raises it again, through the pointer the graph recorded
        with torch.cuda.stream(r.stream):
            g.replay()
        with pytest.raises(AssertionError):
            r.synchronize()
        r.synchronize()
    tape[1, 999] = 0
    torch.cuda.synchronize()
    with torch.cuda.stream(r.stream):
        g.replay()
    r.synchronize()
    assert r.handle.get_counters()[0] == 5 * K          # one launch outside the capture, four replays
    r.close()
