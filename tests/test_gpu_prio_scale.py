"""The calls of include/mxv_prio.h where their workgroups stride and where the tree is deep, against tests/prio_host.py bit for bit:
tests/test_gpu_prio.py stops at 1025-row batches, one 65 537-row insert and H <= 5.  Here every tree-writing workgroup (kTreeBlocks = 256
of them) takes three or four tiles and sums its LDS top words across them; prio_clear, prio_draw and the narrow gather run above
kMaxBlocks * kThreads = 2048 * 256 rows; the weights reduce 128 workgroup minima (the second iteration of log_of_minimum); the wide gather
takes a second row per blockIdx.y; and the tree is 6 and 7 levels high (three and four levels below the LDS-summed top).

After every call the leaves, every level and qmax are the twin's, and the downloaded arrays hold the tree's invariant by themselves.
Every sample is also held to three references that do not walk the tree: the flat prefix sum of the leaves, the liveness of what was
drawn, and the float64 quotient (qmin / q) ** beta."""
import numpy as np
import pytest

import prio_host as ph
from test_gpu_prio import Pair, td_errors, tree_same_as
from test_gpu_replay import CANARY, buffer_same_as, down, same_batch, up
from test_gpu_replay_scale import filled_ring

pytestmark = pytest.mark.gpu

TREE_ROWS = 256 * 256       # kTreeBlocks * kThreads: the rows one trip of prio_insert's and prio_raise's tile loops covers
TILE_ROWS = 2048 * 256      # kMaxBlocks * kThreads: the same of prio_clear, prio_draw and prio_gather_rows
WIDE_ROWS = 16384           # kWideRows: gridDim.y of prio_gather_wide at most
MINIMA_ROWS = 64 * 256      # the rows whose workgroup minima one iteration of log_of_minimum reads
TAIL = 37                   # canary words behind the last output row
ALPHA, EPS = 0.6, 1e-6


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


# ---- the references that do not walk the tree ------------------------------------------------------------------------------------------------------
def holds_the_invariant(leaf, node, C, what):
    """On arrays as downloaded: every node is the NumPy sum of its 16 children, and every padding word is zero."""
    n = ph.layout(C)[3]
    assert not leaf[C:].any(), (what, "leaf padding")
    below, at = leaf.astype(np.uint64), 0
    for l in range(1, len(n)):
        words = -(-n[l] // ph.FANOUT) * ph.FANOUT
        level = node[at:at + words]
        sums = below.reshape(-1, ph.FANOUT).sum(axis=1, dtype=np.uint64)
        assert len(sums) == n[l]
        bad = np.flatnonzero(level[:n[l]] != sums)
        assert bad.size == 0, (what, "level", l, bad[:8], level[bad[:8]], sums[bad[:8]])
        assert not level[n[l]:].any(), (what, "padding of level", l)
        below, at = level, at + words
    assert at == len(node)


def tree_is_sound(torch, buf, tree, what):
    """The twin's leaves, levels and qmax; and the invariant on the device's own arrays."""
    tree_same_as(torch, buf, tree, what)
    holds_the_invariant(down(torch, buf._leaf), down(torch, buf._node, np.uint64), tree.C, what)


def sample_is_sound(leaf, C, count, seed, step, B, beta, indices, weights, what):
    """indices int64 [B] and weights float32 [B] of one sample step against the flat exact prefix sum of leaf[:C] (no descent), the
    liveness of the drawn leaves, and float32((qmin / q) ** beta) computed in float64.  The weights may be a neighbouring float32 and
    no further: tests/test_prio_host.py holds the rule's float64 value to 2^-44 relative of that quotient, so the rounding to float32
    lands on the same float32 or, next to a rounding boundary, on its neighbour."""
    cum = np.cumsum(leaf[:C], dtype=np.uint64)
    u = ph.mulhi64(ph.words64(seed, step, np.arange(B)), np.uint64(cum[-1]))
    flat = np.searchsorted(cum, u, side="right")
    bad = np.flatnonzero(indices != flat)
    assert bad.size == 0, (what, "flat prefix sum", bad[:8], indices[bad[:8]], flat[bad[:8]])
    q = leaf[indices]
    assert (q > 0).all() and indices.min() >= 0 and indices.max() < min(count, C), (what, "drawn leaves are live")
    qmin = q.min()
    ref = ((np.float64(qmin) / q.astype(np.float64)) ** np.float64(beta)).astype(np.float32)
    assert weights.dtype == np.float32
    ulps = np.abs(weights.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    print(f"{what}: weights off the float64 quotient by at most {int(ulps.max())} ulp, {int((ulps != 0).sum())} of {B} rows differ")
    assert ulps.max() <= 1, (what, "weights", int(ulps.max()), int((ulps > 1).sum()))
    assert (weights[q == qmin] == np.float32(1.0)).all(), (what, "weight at the minimum")


# ---- a tree on the device, driven through the C entry points beside its twin ----------------------------------------------------------------------
class DeviceTree:
    def __init__(self, torch, C):
        from gym_amd import prioritized

        self.torch, self.C, self.lib = torch, C, prioritized.lib
        self.tree = ph.Tree(C)
        self.leaf_words, self.node_words, self.H = prioritized.layout(C)
        assert (self.leaf_words, self.node_words, self.H) == (self.tree.leaf_words, self.tree.node_words, self.tree.H)
        self._leaf = torch.zeros(self.leaf_words, dtype=torch.int32, device="cuda:0")
        self._node = torch.zeros(self.node_words, dtype=torch.int64, device="cuda:0")
        self._qmax = torch.full((1,), ph.ONE, dtype=torch.int32, device="cuda:0")
        self._work = torch.zeros(prioritized.WORKSPACE_WORDS, dtype=torch.int32, device="cuda:0")

    def pointers(self):
        return self._leaf.data_ptr(), self.leaf_words, self._node.data_ptr(), self.node_words

    def load(self, leaves, qmax):
        """The twin and the device from leaf values uint32 [C]."""
        t = self.tree
        t.leaf[:self.C] = leaves
        t.qmax = int(qmax)
        t._sum_up()
        self._leaf.copy_(up(self.torch, t.leaf))
        self._node.copy_(up(self.torch, t.node))
        self._qmax.fill_(int(np.uint32(qmax).view(np.int32)))
        return self

    def ok(self, rc):
        self.torch.cuda.synchronize()
        assert rc == 0, self.lib.mxv_prio_last_error()

    def insert(self, count, R, what, by_state=False):
        state = up(self.torch, np.array([count, 0], np.int64)) if by_state else None
        self.ok(self.lib.mxv_prio_insert(None, self.C, 1, R, 0 if by_state else count, None if state is None else state.data_ptr(), *self.pointers(),
                                         self._qmax.data_ptr()))
        self.tree.insert(count, R)
        tree_is_sound(self.torch, self, self.tree, what)

    def update(self, count, indices, td, what):
        B = len(indices)
        idx, tdd = up(self.torch, np.asarray(indices, np.int64)), up(self.torch, np.asarray(td, np.float32))
        saved = self.torch.zeros(B, dtype=self.torch.int32, device="cuda:0")
        self.ok(self.lib.mxv_prio_update(None, self.C, B, idx.data_ptr(), tdd.data_ptr(), ALPHA, EPS, count, None, *self.pointers(), self._qmax.data_ptr(),
                                         saved.data_ptr()))
        self.tree.update(count, indices, td, ALPHA, EPS)
        tree_is_sound(self.torch, self, self.tree, what)

    def sample(self, ring_pointers, W, B, seed, step, beta, action_bytes=4):
        """mxv_prio_sample into outputs with TAIL canary elements behind row B - 1, which must survive; -> the batch as NumPy arrays."""
        t, aw = self.torch, action_bytes // 4
        out = dict(indices=up(t, np.full(B + TAIL, 77, np.int64)), obs=up(t, np.full(B * W + TAIL, CANARY, np.uint32)),
                   next_obs=up(t, np.full(B * W + TAIL, CANARY, np.uint32)), actions=up(t, np.full((B + TAIL) * aw, CANARY, np.uint32)),
                   reward=up(t, np.full(B + TAIL, CANARY, np.uint32)), terminated=up(t, np.full(B + TAIL, 0xCA, np.uint8)),
                   weights=up(t, np.full(B + TAIL, CANARY, np.uint32)))
        t.cuda.synchronize()
        self.ok(self.lib.mxv_prio_sample(None, self.C, W, B, *ring_pointers, *self.pointers(), seed, step, None, beta, self._work.data_ptr(),
                                         out["indices"].data_ptr(), out["obs"].data_ptr(), out["next_obs"].data_ptr(), out["actions"].data_ptr(), action_bytes,
                                         out["reward"].data_ptr(), out["terminated"].data_ptr(), out["weights"].data_ptr()))
        host = {k: down(t, v, {"indices": np.int64, "terminated": np.uint8}.get(k, np.uint32)) for k, v in out.items()}
        for k, words, canary in (("indices", B, 77), ("obs", B * W, CANARY), ("next_obs", B * W, CANARY), ("actions", B * aw, CANARY), ("reward", B, CANARY),
                                 ("terminated", B, 0xCA), ("weights", B, CANARY)):
            assert (host[k][words:] == canary).all(), ("the tail behind row B - 1", k)
            host[k] = host[k][:words]
        host["obs"], host["next_obs"] = host["obs"].reshape(B, W), host["next_obs"].reshape(B, W)
        if action_bytes == 8:
            host["actions"] = host["actions"].view(np.int64)
        host["weights"] = host["weights"].view(np.float32)
        return host


def same_sample(got, want, what):
    same_batch(got, want, what)
    assert np.array_equal(got["weights"].view(np.uint32), want["weights"].view(np.uint32)), (what, "weights")


def decade_leaves(rng, C):
    """Quantised TD errors over four decades, with no zero TD error among them: the smallest leaf is unique or nearly so."""
    return ph.quantise((10.0 ** rng.uniform(-2.0, 2.0, C)).astype(np.float32), ALPHA, EPS)


# ---- insert ----------------------------------------------------------------------------------------------------------------------------------------
SCALE_ROWS = 3 * TREE_ROWS + 257      # prio_insert / prio_raise: workgroup 0 takes four tiles (the fourth full), workgroup 1 four (one row), the others three
SCALE_C = SCALE_ROWS + 40             # 16^4 < C <= 16^5: H = 5


@pytest.mark.parametrize("by_state", (False, True))
def test_insert_sums_the_top_words_over_three_and_four_tiles(torch, by_state):
    """prio_insert above 256 * 256 rows in every workgroup (tests/test_gpu_prio.py: one extra tile in one workgroup): the LDS top words
    accumulate over the trips, the segmented scan runs in every one of them, and the ring wraps inside a wave of workgroup 0's third
    tile.  Then again over leaves on both sides of the insert priority: the deltas are of both signs, and negative ones wrap in uint64."""
    d = DeviceTree(torch, SCALE_C)
    assert d.H == 5
    wrap_row = 2 * TREE_ROWS + 100                                           # lane 36 of the second wave
    count = 2 * SCALE_C + (SCALE_C - wrap_row)
    assert (count + wrap_row) % SCALE_C == 0
    d.insert(count, SCALE_ROWS, "into the empty tree", by_state)
    assert d.tree.total == SCALE_ROWS * ph.ONE
    rng = np.random.default_rng(31)
    leaves = decade_leaves(rng, SCALE_C)
    leaves[rng.random(SCALE_C) < 0.1] = 0                                    # slots never written among them
    qmax = int(np.median(leaves))
    d.load(leaves, qmax)
    tree_is_sound(torch, d, d.tree, "loaded")
    before = d.tree.leaf.copy()
    d.insert(count + 12345, SCALE_ROWS, "over mixed priorities", by_state)
    changed = before != d.tree.leaf
    assert (before[changed] > qmax).sum() > 50000 and (before[changed] < qmax).sum() > 50000      # deltas of both signs


# ---- update ----------------------------------------------------------------------------------------------------------------------------------------
def update_rows(rng, B, C):
    """A third of the rows at 50 slots, a third anywhere, the rest out of range; TD errors with NaN, Inf and 0 among them; shuffled, so
    that the rows of one slot lie in many workgroups and tiles."""
    hot = rng.choice(C, 50, replace=False)
    third = B // 3
    out = np.concatenate((rng.integers(-3, 0, size=(B - 2 * third) // 2), rng.integers(C, C + 4, size=B - 2 * third - (B - 2 * third) // 2)))
    out[::7] = 1 << 40
    idx = np.concatenate((rng.choice(hot, third), rng.integers(0, C, size=third), out))
    rng.shuffle(idx)
    td = td_errors(rng, B)
    td[5::1001], td[6::1003], td[7::1005] = np.nan, np.inf, -np.inf
    return hot, idx.astype(np.int64), td


def filled_tree(torch, C, seed):
    d = DeviceTree(torch, C)
    rng = np.random.default_rng(seed)
    leaves = decade_leaves(rng, C)
    return d.load(leaves, leaves.max()), rng


@pytest.mark.parametrize("B", (SCALE_ROWS, TILE_ROWS + 257))
def test_update_with_heavy_duplicates_across_workgroups_and_tiles(torch, B):
    """B = 3 * 65536 + 257: prio_raise strides (every workgroup three or four tiles; `best` and the top words are kept across them).
    B = 2048 * 256 + 257: prio_clear strides as well (prio_raise then takes nine tiles per workgroup)."""
    C = SCALE_C
    d, rng = filled_tree(torch, C, 41 + B)
    hot, idx, td = update_rows(rng, B, C)
    assert ((idx < 0) | (idx >= C)).sum() > B // 4
    d.update(C, idx, td, ("update", B))
    q = ph.quantise(td, ALPHA, EPS)
    leaf = down(torch, d._leaf)
    for k in hot:                                                            # whatever the twin says: the largest of the slot's rows
        assert int(leaf[k]) == int(q[idx == k].max()), k
    assert d.tree.qmax == ph.QMAX == int(down(torch, d._qmax)[0])            # a NaN td error among the rows in range
    # and once more over the tree this left: other slots are hot, and the leaves the first update raised to QMAX come down
    _, idx, td = update_rows(rng, B, C)
    d.update(C, idx, td, ("second update", B))


# ---- draw, minima, weights -------------------------------------------------------------------------------------------------------------------------
# (B, seed, the half of the rows that holds every row which drew the batch's smallest leaf).  The seeds are the first from 0 with the
# property, found with the twin on the CPU (below 16 for each, as the chance of one half per seed suggests); the test asserts it anew.
#   * 2 * 16384 rows: 128 workgroup minima, so lanes of log_of_minimum take a second iteration; the minimum is among the words 64 .. 127.
#   * 2 * 2048 * 256 + 1 rows: prio_draw strides — workgroup 0 takes a third tile of one row — and its running minimum crosses tiles.  With
#     the minimum in the upper half a kernel that keeps only a workgroup's first tile loses it; in the lower half, one that keeps only the last.
DRAWS = ((2 * MINIMA_ROWS, 0, "upper"), (2 * TILE_ROWS + 1, 3, "upper"), (2 * TILE_ROWS + 1, 0, "lower"))
DRAW_C, DRAW_TREE_SEED, DRAW_STEP, DRAW_BETA = SCALE_C, 51, (1 << 33) + 3, 0.7


def draw_tree_leaves():
    return decade_leaves(np.random.default_rng(DRAW_TREE_SEED), DRAW_C)


def rows_of_the_minimum(tree, seed, B):
    _, q = tree.draw(seed, DRAW_STEP, B)
    return np.flatnonzero(q == q.min())


@pytest.mark.parametrize("B,seed,half", DRAWS)
def test_draws_and_weights_where_the_minimum_crosses_workgroups_and_tiles(torch, B, seed, half):
    leaves = draw_tree_leaves()
    d = DeviceTree(torch, DRAW_C).load(leaves, leaves.max())
    rows = rows_of_the_minimum(d.tree, seed, B)
    assert (rows >= B // 2).all() if half == "upper" else (rows < B // 2).all(), (B, seed, half, rows)
    ring, dring = filled_ring(torch, DRAW_C, 1, 61)
    got = d.sample(dring.pointers(), 1, B, seed, DRAW_STEP, DRAW_BETA, action_bytes=8 if half == "lower" else 4)
    same_sample(got, ph.sample(d.tree, ring, seed, DRAW_STEP, B, DRAW_BETA, action_bytes=8 if half == "lower" else 4), (B, seed))
    sample_is_sound(d.tree.leaf, DRAW_C, DRAW_C, seed, DRAW_STEP, B, DRAW_BETA, got["indices"], got["weights"], (B, seed))
    assert np.array_equal(got["obs"], ring.obs[got["indices"]]) and np.array_equal(got["next_obs"], ring.next[got["indices"]])
    tree_is_sound(torch, d, d.tree, "sampling writes nothing to the tree")


# ---- the wide gather -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", (12, 9))                                       # prio_gather_wide<true> and <false>
def test_wide_gather_strides_over_the_rows(torch, W):
    """16384 + 257 rows: the blockIdx.y loop of prio_gather_wide takes a second row in 257 workgroups, each of whose first waves has
    reduced the 66 workgroup minima itself.  Then the all-zero tree at that size."""
    B, C = WIDE_ROWS + 257, 4097
    d, _ = filled_tree(torch, C, 71 + W)
    ring, dring = filled_ring(torch, C, W, 81 + W)
    for seed, beta, ab in ((5, 0.4, 4), (6, 1.0, 8)):
        got = d.sample(dring.pointers(), W, B, seed, 9, beta, action_bytes=ab)
        same_sample(got, ph.sample(d.tree, ring, seed, 9, B, beta, action_bytes=ab), (W, seed))
        sample_is_sound(d.tree.leaf, C, C, seed, 9, B, beta, got["indices"], got["weights"], (W, seed))
        assert np.array_equal(got["obs"], ring.obs[got["indices"]]) and np.array_equal(got["next_obs"], ring.next[got["indices"]])
    empty = DeviceTree(torch, C)
    got = empty.sample(dring.pointers(), W, B, 5, 9, 0.4)
    same_sample(got, ph.sample(empty.tree, ring, 5, 9, B, 0.4), (W, "the all-zero tree"))
    assert (got["indices"] == -1).all() and not got["weights"].view(np.uint32).any() and not got["obs"].any() and not got["next_obs"].any()
    assert not got["actions"].any() and not got["reward"].any() and not got["terminated"].any()


# ---- deep trees ------------------------------------------------------------------------------------------------------------------------------------
def test_a_tree_of_six_levels_through_the_front_end(torch):
    """C = 16^5 + 1: H = 6, the first height with three levels below the LDS-summed top — the segmented scan of an insert and the
    per-lane adds of an update run at levels 1, 2 and 3 in one trip, and a draw makes five dependent node rounds before the leaves."""
    C = 16 ** 5 + 1
    rng = np.random.default_rng(C)
    p = Pair(torch, C, 1, seed=C + 1)
    assert p.buf.levels == p.tree.H == 6
    for i, ((K, N), B) in enumerate(zip(((1, 1), (2, 40000), (1, C), (1, 300)), (1025, WIDE_ROWS + 257, 1025, WIDE_ROWS + 257))):
        p.add(rng, K, N, (C, i))
        tree_is_sound(torch, p.buf, p.tree, (C, i, "insert"))
        beta, step = (0.4, 1.0, 0.0, 0.7)[i], p.step
        batch = p.sample(B, beta, (C, i))
        k = down(torch, batch["indices"], np.int64)
        sample_is_sound(p.tree.leaf, C, p.count, p.seed, step, B, beta, k, down(torch, batch["weights"], np.float32), (C, i))
        p.update(k, td_errors(rng, B), (C, i))
        tree_is_sound(torch, p.buf, p.tree, (C, i, "update"))
        p.update(rng.integers(-3, C + 3, size=B), td_errors(rng, B), (C, i, "own indices"))
        tree_is_sound(torch, p.buf, p.tree, (C, i, "own indices"))
    buffer_same_as(torch, p.buf, p.ring, C)
    assert p.buf.count == p.count == 1 + 80000 + C + 300 and p.buf.sample_step == p.step == 4


def boundary_slots(C):
    """Every slot within one of m * 16^k, k = 1 .. 6, m = 1 and 15: where a node of some level ends and the next begins."""
    s = {0, C - 1}
    for k in range(1, 7):
        for m in (1, 15):
            s.update((m * 16 ** k - 1, m * 16 ** k, m * 16 ** k + 1))
    return np.array(sorted(x for x in s if 0 <= x < C), np.int64)


def test_a_tree_of_seven_levels_through_the_c_entry_points(torch):
    """C = 16^6 + 1: H = 7, four levels below the LDS-summed top and the last slot alone under its own chain of nodes up to the root's
    second child.  The leaves are non-zero at a few hundred slots only — around every power of 16 and at 300 others — so every check
    stays cheap.  H = 8 needs over 1 GiB of leaves and is not run."""
    C, W, B = 16 ** 6 + 1, 1, 1025
    rng = np.random.default_rng(7)
    d = DeviceTree(torch, C)
    assert d.H == 7
    edge = boundary_slots(C)
    assert {0, 15, 16, 17, 255, 256, 257, 16 ** 6 - 1, 16 ** 6} <= set(edge.tolist()) and edge[-1] == C - 1
    slots = np.unique(np.concatenate((edge, rng.integers(0, C, size=300))))
    leaves = np.zeros(C, np.uint32)
    leaves[slots] = decade_leaves(rng, len(slots))
    d.load(leaves, leaves.max())
    tree_is_sound(torch, d, d.tree, "loaded")
    ring = [torch.zeros(C, dtype=torch.int32, device="cuda:0") for _ in range(4)] + [torch.zeros(C, dtype=torch.uint8, device="cuda:0")]
    pointers = [x.data_ptr() for x in ring]

    def sample(seed, what):
        got = d.sample(pointers, W, B, seed, 3, 0.5)
        k, q = d.tree.draw(seed, 3, B)
        assert np.array_equal(got["indices"], k) and np.array_equal(got["weights"].view(np.uint32), ph.weights(q, 0.5).view(np.uint32)), what
        sample_is_sound(d.tree.leaf, C, 2 * C, seed, 3, B, 0.5, got["indices"], got["weights"], what)
        assert not got["obs"].any() and not got["next_obs"].any() and not got["reward"].any() and not got["terminated"].any(), what

    sample(1, "the loaded tree")
    d.update(C, rng.choice(edge, B), td_errors(rng, B), "update at the boundaries")
    sample(2, "after the update")
    d.insert(C + 16 ** 6 - 150, 300, "insert across slot 16^6 - 1 .. 16^6 and the wrap")      # C = 16^6 + 1: the last 149 rows start again at slot 0
    d.insert(2 * C - 150, 300, "insert across the wrap")
    assert d.tree.leaf[C - 1] == d.tree.leaf[0] == d.tree.qmax
    sample(3, "after the inserts")
