#!/usr/bin/env python3
"""The device replay buffer: ReplayBuffer.add_chunk of a [K, N] chunk plus ReplayBuffer.sample(B), next to the literal torch
sequence they replace on the same tensors — `cat` (the pre-step observations), `where` (the final observation where a step ended), five
`index_copy_` into the ring, `torch.randint`, five `index_select`.  One pass is one of each; the torch ring keeps the rollout's own
dtypes (float64 rewards, int64 actions), so that no cast is charged to it, and its slot indices and `done` mask are made outside the
pass.  Timed with `rocprofv3 --kernel-trace`, one child process per shape under `timeout -k 10`, stopping at the first failure (no
counters: they are never combined with tracing; the program goes after `--`); times are medians over --iters passes of the kernels'
trace durations:
  * `insert_us`, `sample_us`                                 replay_insert_* and replay_sample_*;
  * `kernels_us`, `span_us`, `launches`                      every kernel of one pass of ours: durations summed, first start to last end, count;
  * `torch_kernels_us`, `torch_span_us`, `torch_launches`    the same for one pass of the torch sequence.
Algorithmic bytes: sample 2 (8 W + 9) + 8 a row (both rows read and written, action, reward, flag read and written, the index written);
insert 2 (8 W + 9) a row plus the wider source reward and action (4 + 4 more for float64 and int64) and the truncated flag.

    python benchmarks/replay.py [--iters 20] [--warmup 3] [--out profiles/replay/replay.jsonl]     # one JSON line per shape
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# (C, obs shape, uint8 pixels?, K, N, B): the classic widths on a ring of 2^20 with a 32 x 4096 chunk; a pixel ring of 8192 stacks of
# 4 x 84 x 84 bytes (7056 dwords), whose chunk is 8 x 256 rows — a chunk may not exceed the ring
SHAPES = ((1 << 20, (4,), 0, 32, 4096, 1 << 12), (1 << 20, (4,), 0, 32, 4096, 1 << 18), (1 << 20, (6,), 0, 32, 4096, 1 << 12),
          (1 << 20, (6,), 0, 32, 4096, 1 << 18), (8192, (4, 84, 84), 1, 8, 256, 256))
HBM_PEAK_GBS = 8000.0
CHILD_TIMEOUT_S = 600


def sample_bytes(W):
    return 2 * (8 * W + 9) + 8


def insert_bytes(W):
    return 2 * (8 * W + 9) + 4 + 4 + 1


def torch_pass(torch, ring, slots, n, B, first, traj, done):
    """The literal torch sequence: store the chunk, draw B rows, fetch them."""
    R = slots.shape[0]
    pre = torch.cat([first.unsqueeze(0), traj["obs"][:-1]]).reshape(R, -1)
    nxt = torch.where(done, traj["final_obs"], traj["obs"]).reshape(R, -1)
    ring["obs"].index_copy_(0, slots, pre)
    ring["next_obs"].index_copy_(0, slots, nxt)
    ring["actions"].index_copy_(0, slots, traj["actions"].reshape(R))
    ring["reward"].index_copy_(0, slots, traj["reward"].reshape(R))
    ring["terminated"].index_copy_(0, slots, traj["terminated"].reshape(R))
    idx = torch.randint(0, n, (B,), device=slots.device)
    return {k: ring[k].index_select(0, idx) for k in ("obs", "next_obs", "actions", "reward", "terminated")}, idx


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
    buf = gym_amd.ReplayBuffer(C, shape, obs_dtype=obs_dtype, action_dtype=torch.int64, seed=3, device=0)
    out = buf.sample_buffers(B)
    numel = 1
    for s in shape:
        numel *= s
    ring = {"obs": torch.zeros((C, numel), dtype=obs_dtype, device=dev), "next_obs": torch.zeros((C, numel), dtype=obs_dtype, device=dev),
            "actions": torch.zeros(C, dtype=torch.int64, device=dev), "reward": torch.zeros(C, dtype=torch.float64, device=dev),
            "terminated": torch.zeros(C, dtype=torch.uint8, device=dev)}
    done = ((traj["terminated"] != 0) | (traj["truncated"] != 0)).view((K, N) + (1,) * len(shape))
    # the ring is full before the first timed pass, as in steady state: every draw reaches the whole ring
    fills = -(-C // R)
    for _ in range(fills):
        buf.add_chunk(first, traj)
    count = fills * R
    slots = (count + torch.arange(R, device=dev)) % C
    one = torch.zeros((1, 2), device=dev)
    mark_out = (torch.empty(1, dtype=torch.int64, device=dev), None, None)

    def mark():     # a one-row launch of the categorical sampler: the delimiter between passes in the trace
        gym_amd.sample_categorical(one, seed=0, step=0, out=mark_out)

    def ours():
        buf.add_chunk(first, traj)
        buf.sample(B, out=out)

    mark()
    for f in (ours, lambda: torch_pass(torch, ring, slots, C, B, first, traj, done)):
        for _ in range(warmup + iters):
            f()
            mark()
    torch.cuda.synchronize()
    # the two store the same rows: the last chunk of ours sits where the torch sequence put the same chunk
    mine = (fills + warmup + iters - 1) * R
    s_mine = (mine + torch.arange(R, device=dev)) % C
    same = bool(torch.equal(buf._obs[s_mine], ring["obs"][slots]) and torch.equal(buf._next[s_mine], ring["next_obs"][slots])
                and torch.equal(buf._reward[s_mine], ring["reward"][slots].float()) and torch.equal(buf._term[s_mine], (ring["terminated"][slots] != 0).to(torch.uint8)))
    idx = out["indices"]
    gathered = bool(torch.equal(out["obs"].view(B, -1), buf._obs[idx]) and torch.equal(out["next_obs"].view(B, -1), buf._next[idx]) and int(idx.max()) < C)
    print(json.dumps({"child": True, "stored_rows_equal_torch": same, "gathered_rows_equal_ring": gathered}), flush=True)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else float("nan")


def profile(spec, iters, warmup):
    d = tempfile.mkdtemp(prefix="replay_bench_")
    try:
        C, shape, pixels, K, N, B = spec
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), "rocprofv3", "--kernel-trace", "-d", d, "-o", "trace", "--output-format", "csv", "--",
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
    """-> dict of medians from the ordered trace of child(): the LAST 2 (warmup + iters) + 1 marks delimit the passes, ours first."""
    n = warmup + iters
    marks = [i for i, k in enumerate(ks) if "policy_kernel" in k[2]]
    assert len(marks) >= 2 * n + 1, (len(marks), n)
    marks = marks[-(2 * n + 1):]
    segs = [ks[a + 1:b] for a, b in zip(marks[:-1], marks[1:])]
    us = lambda seg: sum(e - s for s, e, _ in seg) / 1e3
    span = lambda seg: (max(e for _, e, _ in seg) - seg[0][0]) / 1e3
    mine, torchs = segs[warmup:n], segs[n + warmup:2 * n]
    parts = {"insert_us": [], "sample_us": []}
    for seg in mine:
        names = [k[2] for k in seg]
        assert len(names) == 2 and "replay_insert" in names[0] and "replay_sample" in names[1], names
        parts["insert_us"].append(us(seg[:1]))
        parts["sample_us"].append(us(seg[1:]))
    assert not any("replay_" in k[2] for seg in torchs for k in seg)
    out = {k: _median(v) for k, v in parts.items()}
    name = lambda k: (re.search(r"replay_\w+<[^>]*>", k[2]) or re.search(r"replay_\w+", k[2])).group(0)
    out.update({"insert_kernel": name(mine[0][0]), "sample_kernel": name(mine[0][1]),
                "kernels_us": _median([us(seg) for seg in mine]), "span_us": _median([span(seg) for seg in mine]), "launches": len(mine[0]),
                "torch_kernels_us": _median([us(seg) for seg in torchs]), "torch_span_us": _median([span(seg) for seg in torchs]),
                "torch_launches": len(torchs[0])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", type=int, action="append", help="index into the shape list (default: all five)")
    ap.add_argument("--out", help="append the JSON lines to this file as well (profiles/replay/replay.jsonl)")
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
        R = K * N
        row = {"C": C, "W": W, "K": K, "N": N, "B": B, "rows_inserted": R}
        row.update({k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items()})
        ins_gbs, smp_gbs = R * insert_bytes(W) / r["insert_us"] / 1e3, B * sample_bytes(W) / r["sample_us"] / 1e3
        row.update({"speedup_kernels_vs_torch_kernels": round(r["torch_kernels_us"] / r["kernels_us"], 2),
                    "speedup_span_vs_torch_span": round(r["torch_span_us"] / r["span_us"], 2),
                    "insert_bytes_per_row": insert_bytes(W), "insert_gbs": round(ins_gbs, 1), "sample_bytes_per_row": sample_bytes(W),
                    "sample_gbs": round(smp_gbs, 1), "sample_roofline_frac": round(smp_gbs / HBM_PEAK_GBS, 4),
                    "ring_mib": round(C * (8 * W + 9) / 2 ** 20, 1), "source": "rocprofv3 kernel-trace (median)"})
        row.update({k: v for k, v in info.items() if k != "child"})
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
