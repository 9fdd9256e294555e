"""The calls of include/mxv_replay.h where their workgroups stride, against tests/replay_host.py bit for bit: tests/test_gpu_replay.py stops
at 1025 rows, where every workgroup of the narrow kernels takes one tile and every workgroup of the wide kernels one row.  Here the
narrow insert and sample run above kMaxBlocks * kThreads = 2048 * 256 rows (a second trip round the tile loop, the ring's wrap inside
it) and the wide insert and sample above kWideRows = 16384 rows (a second row per blockIdx.y, in one piece and in two).  All through
the C entry points, on rings and outputs with canaries around what must be written."""
import numpy as np
import pytest

import replay_host as rh
from test_gpu_replay import CANARY, CANARY_FINAL, DeviceRing, c_insert, down, make_chunk, same_batch, up

pytestmark = pytest.mark.gpu

TILE_ROWS = 2048 * 256      # kMaxBlocks * kThreads: the rows one trip of the narrow kernels' tile loop covers
WIDE_ROWS = 16384           # kWideRows: gridDim.y of the wide kernels at most
TAIL = 37                   # canary words behind the last output row


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def insert_equals_the_twin(torch, C, W, K, N, count, *, pad=0, shift=0, by_state=False):
    from gym_amd import replay

    rng = np.random.default_rng(C + W + pad)
    chunk = make_chunk(rng, K, N, W, np.float64, np.int64, with_final=True)
    twin, dring = rh.Ring(C, W, fill=CANARY), DeviceRing(torch, C, W)
    state = up(torch, np.array([count, 0], np.int64)) if by_state else None
    rc = c_insert(torch, dring, 0 if by_state else count, chunk, pad=pad, shift=shift, state=state)      # with state_dev the count by value is not read
    assert rc == 0, replay.lib.mxv_replay_last_error()
    after = rh.insert(twin, count, *chunk)
    what = (C, W, K, N, count, pad, shift, by_state)
    dring.same_as(twin, what)
    if by_state:
        assert state.tolist() == [after, 0], what
    written = K * N
    untouched = (count + written + np.arange(C - written)) % C                # the slots behind the chunk: they kept the canary
    assert (twin.action[untouched] == CANARY).all() and (twin.obs[untouched] == CANARY).all() and (twin.term[untouched] == CANARY & 0xFF).all(), what
    assert (down(torch, dring.action)[untouched] == CANARY).all() and (down(torch, dring.obs).reshape(C, W)[untouched] == CANARY).all(), what
    for x in (dring.obs, dring.next):
        assert not (down(torch, x) == CANARY_FINAL).any(), what              # no row of an unfinished step's final_obs was read


# ---- insert ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_state", (False, True))
@pytest.mark.parametrize("W", (1, 4))                                        # replay_insert_rows<0>: the loop copier; <4>: the 16-byte copier
def test_narrow_insert_wraps_the_ring_inside_a_second_trip(torch, W, by_state):
    """2048 * 256 + 293 rows: the tile loop of replay_insert_rows strides — workgroups 0 and 1 take a second tile.  The ring wraps at row
    2048 * 256 + 100: lane 36 of the second wave of workgroup 0's second tile."""
    C = TILE_ROWS + 300
    wrap_row = TILE_ROWS + 100
    count = 3 * C + (C - wrap_row)                                           # row r lands in slot (count + r) mod C: slot 0 at r = wrap_row
    assert (count + wrap_row) % C == 0 and wrap_row % 64 == 36 and wrap_row // 256 == 2048
    insert_equals_the_twin(torch, C, W, 1, C - 7, count, by_state=by_state)


@pytest.mark.parametrize("pad,shift", ((0, 0), (3, 1)))                      # packed sources; rows W + 3 dwords apart from a base 4 bytes off
@pytest.mark.parametrize("W", (12, 9, 1028))                                 # replay_insert_wide<true> (packed only), <false>, two pieces
def test_wide_insert_strides_over_the_rows(torch, W, pad, shift):
    """16384 + 257 rows: the blockIdx.y loop of replay_insert_wide takes a second row in 257 workgroups per piece; the wrap is in the
    second trip (row 16384 + 100) and the chunk has three steps, so that rows of the second trip read obs[r - N]."""
    R = WIDE_ROWS + 257
    C = R + 5
    K, N = 3, R // 3
    assert K * N == R
    wrap_row = WIDE_ROWS + 100
    insert_equals_the_twin(torch, C, W, K, N, 2 * C + (C - wrap_row), pad=pad, shift=shift)


# ---- sample ----------------------------------------------------------------------------------------------------------------------------------------
def filled_ring(torch, C, W, seed):
    rng = np.random.default_rng(seed)
    ring = rh.Ring(C, W)
    ring.obs[:] = rng.integers(0, 1 << 32, size=(C, W), dtype=np.int64).astype(np.uint32)
    ring.next[:] = rng.integers(0, 1 << 32, size=(C, W), dtype=np.int64).astype(np.uint32)
    ring.action[:] = rng.integers(0, 1 << 32, size=C, dtype=np.int64).astype(np.uint32)
    ring.reward[:] = rng.integers(0, 1 << 32, size=C, dtype=np.int64).astype(np.uint32)
    ring.term[:] = rng.integers(0, 2, size=C).astype(np.uint8)
    dring = DeviceRing(torch, C, W)
    dring.load(ring)
    return ring, dring


def sample_with_tails(torch, dring, count, seed, step, B, action_bytes):
    """mxv_replay_sample into outputs with TAIL canary elements behind row B - 1, which must survive; -> the batch as NumPy arrays."""
    from gym_amd import replay

    W, aw = dring.W, action_bytes // 4
    out = dict(indices=up(torch, np.full(B + TAIL, 77, np.int64)), obs=up(torch, np.full(B * W + TAIL, CANARY, np.uint32)),
               next_obs=up(torch, np.full(B * W + TAIL, CANARY, np.uint32)), actions=up(torch, np.full((B + TAIL) * aw, CANARY, np.uint32)),
               reward=up(torch, np.full(B + TAIL, CANARY, np.uint32)), terminated=up(torch, np.full(B + TAIL, 0xCA, np.uint8)))
    torch.cuda.synchronize()
    rc = replay.lib.mxv_replay_sample(None, dring.C, W, B, *dring.pointers(), seed, count, step, None, out["indices"].data_ptr(), out["obs"].data_ptr(),
                                      out["next_obs"].data_ptr(), out["actions"].data_ptr(), action_bytes, out["reward"].data_ptr(),
                                      out["terminated"].data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, replay.lib.mxv_replay_last_error()
    host = dict(indices=down(torch, out["indices"], np.int64), obs=down(torch, out["obs"]), next_obs=down(torch, out["next_obs"]),
                actions=down(torch, out["actions"]), reward=down(torch, out["reward"]), terminated=down(torch, out["terminated"], np.uint8))
    assert (host["indices"][B:] == 77).all() and (host["obs"][B * W:] == CANARY).all() and (host["next_obs"][B * W:] == CANARY).all()
    assert (host["actions"][B * aw:] == CANARY).all() and (host["reward"][B:] == CANARY).all() and (host["terminated"][B:] == 0xCA).all()
    act = host["actions"][:B * aw]
    return dict(indices=host["indices"][:B], obs=host["obs"][:B * W].reshape(B, W), next_obs=host["next_obs"][:B * W].reshape(B, W),
                actions=act.view(np.int64) if action_bytes == 8 else act, reward=host["reward"][:B], terminated=host["terminated"][:B])


def sample_equals_the_twin(torch, ring, dring, count, seed, step, B, action_bytes):
    got = sample_with_tails(torch, dring, count, seed, step, B, action_bytes)
    what = (ring.C, ring.W, B, count, action_bytes)
    same_batch(got, rh.sample(ring, count, seed, step, B, action_bytes=action_bytes), what)
    k = got["indices"]
    assert k.min() >= 0 and k.max() < min(count, ring.C), what
    # whatever the twin says: every output row is the ring's row at the index beside it
    assert np.array_equal(got["obs"], ring.obs[k]) and np.array_equal(got["next_obs"], ring.next[k]) and np.array_equal(got["reward"], ring.reward[k]), what
    assert np.array_equal(got["terminated"], ring.term[k]), what
    dring.same_as(ring, "sampling writes nothing to the ring")


@pytest.mark.parametrize("action_bytes", (4, 8))
@pytest.mark.parametrize("W", (1, 4))                                        # replay_sample_rows<0> and <4>
def test_narrow_sample_strides_over_the_tiles(torch, W, action_bytes):
    """2048 * 256 + 257 rows: the tile loop of replay_sample_rows strides — workgroup 0 takes a second, full tile and workgroup 1 a
    second tile of one row."""
    ring, dring = filled_ring(torch, 257, W, 200 + W)
    sample_equals_the_twin(torch, ring, dring, 3 * 257 + 1, 1000 + W, (1 << 33) + 5, TILE_ROWS + 257, action_bytes)


@pytest.mark.parametrize("W", (9, 12))                                       # replay_sample_wide<false> and <true>
def test_wide_sample_strides_over_the_rows(torch, W):
    """16384 + 257 rows: the blockIdx.y loop of replay_sample_wide takes a second row in 257 workgroups."""
    ring, dring = filled_ring(torch, 1025, W, 300 + W)
    for count, action_bytes in ((1025, 4), (600, 8)):                        # full, and part full: n = min(count, C) either way
        sample_equals_the_twin(torch, ring, dring, count, 2000 + W, 7, WIDE_ROWS + 257, action_bytes)
