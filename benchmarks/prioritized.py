#!/usr/bin/env python3
"""Prioritised replay on the device: PrioritizedReplayBuffer.add_chunk of a [K, N] chunk, sample(B) and
update_priorities on a full ring, next to the literal torch sequence on the same tensors.  One pass of ours is one of each.  The torch
pass is, for the chunk, the store of benchmarks/replay.py (`cat`, `where`, five `index_copy_`) and an `index_copy_` of the new slots'
priorities, and then the sequence a torch user writes for proportional replay over a float32 priority vector:
  `cumsum`, `rand` * total, `searchsorted` (and the `clamp_` that keeps a rounded-up draw inside the ring), five `index_select`, the
  weight arithmetic with its `min` (`index_select` of the priorities, `min`, `div`, `pow`), and `abs` / `add` / `pow` / `index_put_` /
  `max` / `maximum` for the update.
Both halves are reported apart, so that ours — the whole pass — can be held against the sample-and-update half of torch alone.  Timed with
`rocprofv3 --kernel-trace`, one child process per shape under `timeout -k 10`, stopping at the first failure (no counters: they are
never combined with tracing; the program goes after `--`); times are medians over --iters passes of the kernels' trace durations:
  * `insert_us` (prio_insert + replay_insert_*), `draw_us`, `gather_us`, `clear_us`, `raise_us`;
  * `kernels_us`, `span_us`, `launches`                      every kernel of one pass of ours: durations summed, first start to last end, count;
  * `torch_store_kernels_us`, `torch_kernels_us`, `torch_span_us`, `torch_launches`      the store half, and the sample-and-update half alone.

    python benchmarks/prioritized.py [--iters 20] [--warmup 3] [--out profiles/prio/prio.jsonl]     # one JSON line per shape
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import replay as replay_bench  # noqa: E402  (benchmarks/replay.py: the shapes)

# (C, obs shape, uint8 pixels?, K, N, B): benchmarks/replay.py's
SHAPES = replay_bench.SHAPES
ALPHA, EPS, BETA = 0.6, 1e-6, 0.4


def torch_store(torch, ring, prio, max_prio, slots, first, traj, done):
    R = slots.shape[0]
    pre = torch.cat([first.unsqueeze(0), traj["obs"][:-1]]).reshape(R, -1)
    nxt = torch.where(done, traj["final_obs"], traj["obs"]).reshape(R, -1)
    ring["obs"].index_copy_(0, slots, pre)
    ring["next_obs"].index_copy_(0, slots, nxt)
    ring["actions"].index_copy_(0, slots, traj["actions"].reshape(R))
    ring["reward"].index_copy_(0, slots, traj["reward"].reshape(R))
    ring["terminated"].index_copy_(0, slots, traj["terminated"].reshape(R))
    prio.index_copy_(0, slots, max_prio.expand(R))


def torch_draw_and_update(torch, ring, prio, max_prio, B, td):
    cs = torch.cumsum(prio, 0)
    u = torch.rand(B, device=prio.device) * cs[-1]
    idx = torch.searchsorted(cs, u).clamp_(max=prio.shape[0] - 1)
    batch = {k: ring[k].index_select(0, idx) for k in ("obs", "next_obs", "actions", "reward", "terminated")}
    p = prio.index_select(0, idx)
    batch["weights"] = (p.min() / p) ** BETA
    new = (td.abs() + EPS) ** ALPHA
    prio.index_put_((idx,), new)
    max_prio.copy_(torch.maximum(max_prio, new.max()))
    return batch, idx


def child(C, shape, pixels, K, N, B, iters, warmup):
    import torch

    import gym_amd

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    R = K * N
    if pixels:
        make = lambda lead: torch.randint(0, 256, lead + shape, device=dev, generator=g, dtype=torch.uint8)
        obs_dtype = torch.uint8
    else:
        make = lambda lead: torch.randn(lead + shape, device=dev, generator=g)
        obs_dtype = torch.float32
    first = make((N,))
    traj = {"obs": make((K, N)), "final_obs": make((K, N)), "actions": torch.randint(0, 2, (K, N), device=dev, generator=g),
            "reward": torch.randn((K, N), device=dev, generator=g, dtype=torch.float64),
            "terminated": (torch.rand((K, N), device=dev, generator=g) < 0.03).to(torch.uint8),
            "truncated": (torch.rand((K, N), device=dev, generator=g) < 0.01).to(torch.uint8)}
    td = torch.randn(B, device=dev, generator=g)
    buf = gym_amd.PrioritizedReplayBuffer(C, shape, obs_dtype=obs_dtype, action_dtype=torch.int64, seed=3, device=0, alpha=ALPHA, eps=EPS)
    out = buf.sample_buffers(B)
    numel = 1
    for s in shape:
        numel *= s
    ring = {"obs": torch.zeros((C, numel), dtype=obs_dtype, device=dev), "next_obs": torch.zeros((C, numel), dtype=obs_dtype, device=dev),
            "actions": torch.zeros(C, dtype=torch.int64, device=dev), "reward": torch.zeros(C, dtype=torch.float64, device=dev),
            "terminated": torch.zeros(C, dtype=torch.uint8, device=dev)}
    prio, max_prio = torch.ones(C, device=dev), torch.ones(1, device=dev)
    done = ((traj["terminated"] != 0) | (traj["truncated"] != 0)).view((K, N) + (1,) * len(shape))
    # the ring is full before the first timed pass, as in steady state, and its priorities are spread by one update of every slot
    fills = -(-C // R)
    for _ in range(fills):
        buf.add_chunk(first, traj)
    every = torch.arange(C, device=dev)
    spread = torch.randn(C, device=dev, generator=g)
    buf.update_priorities(every, spread)
    prio.copy_((spread.abs() + EPS) ** ALPHA)
    max_prio.copy_(prio.max())
    count = fills * R
    slots = (count + torch.arange(R, device=dev)) % C
    one = torch.zeros((1, 2), device=dev)
    mark_out = (torch.empty(1, dtype=torch.int64, device=dev), None, None)

    def mark():     # a one-row launch of the categorical sampler: the delimiter in the trace
        gym_amd.sample_categorical(one, seed=0, step=0, out=mark_out)

    mark()
    for _ in range(warmup + iters):
        buf.add_chunk(first, traj)
        buf.sample(B, beta=BETA, out=out)
        buf.update_priorities(out["indices"], td)
        mark()
    for _ in range(warmup + iters):
        torch_store(torch, ring, prio, max_prio, slots, first, traj, done)
        mark()
        torch_draw_and_update(torch, ring, prio, max_prio, B, td)
        mark()
    torch.cuda.synchronize()
    # the tree holds its invariant after all passes, and the last batch was gathered at the drawn slots with weights in (0, 1]
    leaf = buf._leaf.view(-1).long() & 0xFFFFFFFF
    level1 = leaf.view(-1, 16).sum(1)
    n1 = level1.shape[0]
    invariant = bool(torch.equal(level1, buf._node[:n1]) and int(buf._node[-16]) == int(leaf.sum()))
    idx = out["indices"]
    gathered = bool(torch.equal(out["obs"].view(B, -1), buf._obs[idx]) and torch.equal(out["next_obs"].view(B, -1), buf._next[idx]) and int(idx.max()) < C
                    and float(out["weights"].max()) == 1.0 and float(out["weights"].min()) > 0.0)
    print(json.dumps({"child": True, "tree_invariant_holds": invariant, "gathered_rows_equal_ring": gathered}), flush=True)


def profile(spec, iters, warmup):
    """The ordered kernel trace of one child process: [(start ns, end ns, name)], and the child's own JSON line."""
    d = tempfile.mkdtemp(prefix="prio_bench_")
    try:
        C, shape, pixels, K, N, B = spec
        cmd = ["timeout", "-k", "10", str(replay_bench.CHILD_TIMEOUT_S), "rocprofv3", "--kernel-trace", "-d", d, "-o", "trace", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--iters", str(iters), "--warmup", str(warmup), "--child", str(C), ",".join(map(str, shape)),
               str(pixels), str(K), str(N), str(B)]
        p = subprocess.run(cmd, check=True, capture_output=True, text=True)
        info = {}
        for line in p.stdout.splitlines():
            if line.startswith('{"child"'):
                info = json.loads(line)
        trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not trace:
            raise RuntimeError(f"rocprofv3 wrote no kernel trace under {d}")
        ks = []
        with open(trace[0]) as f:
            for rec in csv.DictReader(f):
                ks.append((int(rec["Start_Timestamp"]), int(rec["End_Timestamp"]), rec.get("Kernel_Name", "")))
        ks.sort()
        return ks, info
    finally:
        shutil.rmtree(d, ignore_errors=True)


def analyse(ks, iters, warmup):
    """-> dict of medians from the ordered trace of child(): the LAST 3 (warmup + iters) + 1 marks delimit our passes, then the two halves
    of every torch pass."""
    n = warmup + iters
    marks = [i for i, k in enumerate(ks) if "policy_kernel" in k[2]]
    assert len(marks) >= 3 * n + 1, (len(marks), n)
    marks = marks[-(3 * n + 1):]
    segs = [ks[a + 1:b] for a, b in zip(marks[:-1], marks[1:])]
    us = lambda seg: sum(e - s for s, e, _ in seg) / 1e3
    span = lambda seg: (max(e for _, e, _ in seg) - seg[0][0]) / 1e3
    med = replay_bench._median
    mine = [(segs[i][:2], segs[i][2:]) for i in range(warmup, n)]      # the two insert kernels; the draw, the gather and the update
    torchs = [(segs[n + 2 * i], segs[n + 2 * i + 1]) for i in range(warmup, n)]
    parts = {"insert_us": [], "draw_us": [], "gather_us": [], "clear_us": [], "raise_us": []}
    for store, rest in mine:
        names = [k[2] for k in store + rest]
        assert len(names) == 6 and "prio_insert" in names[0] and "replay_insert" in names[1] and "prio_draw" in names[2] and "prio_gather" in names[3] \
            and "prio_clear" in names[4] and "prio_raise" in names[5], names
        parts["insert_us"].append(us(store))
        for key, k in zip(("draw_us", "gather_us", "clear_us", "raise_us"), rest):
            parts[key].append(us([k]))
    assert not any("prio_" in k[2] or "replay_" in k[2] for pair in torchs for seg in pair for k in seg)
    out = {k: med(v) for k, v in parts.items()}
    out.update({"kernels_us": med([us(a + b) for a, b in mine]), "span_us": med([span(a + b) for a, b in mine]), "launches": len(mine[0][0]) + len(mine[0][1]),
                "draw_update_kernels_us": med([us(b) for _, b in mine]), "draw_update_span_us": med([span(b) for _, b in mine]),
                "torch_store_kernels_us": med([us(a) for a, _ in torchs]), "torch_store_launches": len(torchs[0][0]),
                "torch_kernels_us": med([us(b) for _, b in torchs]), "torch_span_us": med([span(b) for _, b in torchs]), "torch_launches": len(torchs[0][1])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", type=int, action="append", help="index into the shape list (default: all five)")
    ap.add_argument("--out", help="append the JSON lines to this file as well (profiles/prio/prio.jsonl)")
    ap.add_argument("--child", nargs=6, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        C, shape, pixels, K, N, B = a.child
        child(int(C), tuple(int(s) for s in shape.split(",")), int(pixels), int(K), int(N), int(B), a.iters, a.warmup)
        return
    for i, spec in enumerate(SHAPES):
        if a.only and i not in a.only:
            continue
        C, shape, pixels, K, N, B = spec
        W = 1
        for s in shape:
            W *= s
        W = W // 4 if pixels else W
        ks, info = profile(spec, a.iters, a.warmup)      # a failed child raises: nothing more is started
        r = analyse(ks, a.iters, a.warmup)
        row = {"C": C, "W": W, "K": K, "N": N, "B": B, "rows_inserted": K * N}
        row.update({k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items()})
        # ours, the WHOLE pass with the chunk's store, against the sample-and-update half of torch alone
        row.update({"speedup_kernels_vs_torch_kernels": round(r["torch_kernels_us"] / r["kernels_us"], 2),
                    "speedup_span_vs_torch_span": round(r["torch_span_us"] / r["span_us"], 2), "source": "rocprofv3 kernel-trace (median)"})
        row.update({k: v for k, v in info.items() if k != "child"})
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
