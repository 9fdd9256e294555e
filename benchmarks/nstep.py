#!/usr/bin/env python3
"""The n-step windowed insert: NStepReplayBuffer.add_chunk of a [K, N] chunk next to the one-step ReplayBuffer.add_chunk
of the same chunk — the kernel of mxv_replay.hip, which this change leaves as it was — and next to the literal torch sequence the n-step
insert replaces: per extra step of the window a handful of `where` / `mul` / `add` launches over shifted views of reward, terminated and
done and one `where` over the observation rows, then `cat` for the pre-step observations and a flat ReplayBuffer.add of the result, which
copies every observation row a second time.  One pass is one of each; the torch sequence selects with `where` as the kernel's branch does,
so the three store the same bits and the child checks that they did.  Timed with `rocprofv3 --kernel-trace`, one child process per (shape,
n) under `timeout -k 10`, stopping at the first failure (no counters: they are never combined with tracing; the program goes after `--`);
times are medians over --iters passes of the kernels' trace durations:
  * `nstep_insert_us`, `onestep_insert_us`, `ratio`          nstep_insert_* and replay_insert_* on the same chunk, and their quotient;
  * `torch_kernels_us`, `torch_span_us`, `torch_launches`    every kernel of one pass of the torch sequence: durations summed, first start to
                                                             last end, count (its last launch is the flat add's replay_insert_*).
Algorithmic bytes of an insert: 2 (8 W + 9) a row plus the wider source reward and action and the truncated flag, as benchmarks/replay.py
counts them, plus the 4 of the discount; the window's extra reads of reward and flags come from the cache.

    python benchmarks/nstep.py [--iters 10] [--warmup 2] [--out profiles/nstep/nstep.jsonl]     # one JSON line per shape and n
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
# (C, obs shape, uint8 pixels?, K, N): the classic widths on a ring of 2^20 with a 32 x 4096 chunk; the pixel ring of benchmarks/replay.py,
# 8192 stacks of 4 x 84 x 84 bytes (7056 dwords) with a chunk of 8 x 256 rows
SHAPES = ((1 << 20, (4,), 0, 32, 4096), (1 << 20, (6,), 0, 32, 4096), (8192, (4, 84, 84), 1, 8, 256))
STEPS = (1, 3, 5)
GAMMA = 0.99
CHILD_TIMEOUT_S = 600


def insert_bytes(W):
    return 2 * (8 * W + 9) + 4 + 4 + 1 + 4


def torch_nstep(torch, flat, n, gamma, first, traj, done, term, base_next):
    """The literal torch sequence: the n-step return, flag, discount and next row of every step by shifted views, then a flat add."""
    K = traj["reward"].shape[0]
    R = K * traj["reward"].shape[1]
    G = traj["reward"].clone()
    g = torch.ones_like(G)
    alive = ~done
    flag = term.clone()
    nxt = base_next.clone()
    wide = (slice(None), slice(None)) + (None,) * (nxt.dim() - 2)
    for j in range(1, min(n, K)):
        a = alive[:K - j]                                    # the windows that still walk into step t + j
        g[:K - j] = torch.where(a, g[:K - j] * gamma, g[:K - j])
        G[:K - j] = torch.where(a, G[:K - j] + g[:K - j] * traj["reward"][j:], G[:K - j])
        flag[:K - j] = torch.where(a, term[j:], flag[:K - j])
        nxt[:K - j] = torch.where(a[wide], base_next[j:], nxt[:K - j])
        alive[:K - j] = a & ~done[j:]
    discount = (g * gamma).reshape(R)
    pre = torch.cat([first.unsqueeze(0), traj["obs"][:-1]])
    flat.add(pre.reshape((R,) + tuple(first.shape[1:])), traj["actions"].reshape(R), G.reshape(R), flag.reshape(R), nxt.reshape((R,) + tuple(first.shape[1:])))
    return discount


def child(C, shape, pixels, K, N, n, iters, warmup):
    import torch

    import gym_amd

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    R = K * N
    if pixels:
        make = lambda lead: torch.randint(0, 256, lead + shape, device=dev, generator=gen, dtype=torch.uint8)
        obs_dtype = torch.uint8
    else:
        make = lambda lead: torch.randn(lead + shape, device=dev, generator=gen)
        obs_dtype = torch.float32
    first = make((N,))
    traj = {"obs": make((K, N)), "final_obs": make((K, N)), "actions": torch.randint(0, 2, (K, N), device=dev, generator=gen),
            "reward": torch.randn((K, N), device=dev, generator=gen, dtype=torch.float64),
            "terminated": (torch.rand((K, N), device=dev, generator=gen) < 0.03).to(torch.uint8),
            "truncated": (torch.rand((K, N), device=dev, generator=gen) < 0.01).to(torch.uint8)}
    kw = dict(obs_dtype=obs_dtype, action_dtype=torch.int64, seed=3, device=0)
    nst = gym_amd.NStepReplayBuffer(C, shape, n, GAMMA, **kw)
    one = gym_amd.ReplayBuffer(C, shape, **kw)
    flat = gym_amd.ReplayBuffer(C, shape, **kw)      # the ring the torch sequence stores into
    term = traj["terminated"] != 0
    done = term | (traj["truncated"] != 0)
    base_next = torch.where(done.view((K, N) + (1,) * len(shape)), traj["final_obs"], traj["obs"])      # made outside the pass, as the done mask
    # the rings are full before the first timed pass, as in steady state
    fills = -(-C // R)
    for _ in range(fills):
        nst.add_chunk(first, traj)
        one.add_chunk(first, traj)
        flat.add_chunk(first, traj)
    mark_logits = torch.zeros((1, 2), device=dev)
    mark_out = (torch.empty(1, dtype=torch.int64, device=dev), None, None)

    def mark():     # a one-row launch of the categorical sampler: the delimiter between passes in the trace
        gym_amd.sample_categorical(mark_logits, seed=0, step=0, out=mark_out)

    disc, term8 = None, term.to(torch.uint8)

    def torch_leg():
        nonlocal disc
        disc = torch_nstep(torch, flat, n, GAMMA, first, traj, done, term8, base_next)

    mark()
    for f in (lambda: nst.add_chunk(first, traj), lambda: one.add_chunk(first, traj), torch_leg):
        for _ in range(warmup + iters):
            f()
            mark()
    torch.cuda.synchronize()
    # the fused insert and the torch sequence stored the same rows in the same slots
    s = ((fills + warmup + iters - 1) * R + torch.arange(R, device=dev)) % C      # the slots of the last chunk
    same = bool(torch.equal(nst._obs[s], flat._obs[s]) and torch.equal(nst._next[s], flat._next[s]) and torch.equal(nst._action[s], flat._action[s])
                and torch.equal(nst._reward[s].view(torch.int32), flat._reward[s].view(torch.int32)) and torch.equal(nst._term[s], flat._term[s]))
    same_disc = bool(torch.equal(nst._discount[s], disc.float()))
    pre_same = bool(torch.equal(nst._obs, one._obs) and torch.equal(nst._action, one._action))
    print(json.dumps({"child": True, "stored_rows_equal_torch": same, "discount_equals_torch": same_disc, "pre_rows_equal_one_step": pre_same}), flush=True)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else float("nan")


def profile(spec, n, iters, warmup):
    d = tempfile.mkdtemp(prefix="nstep_bench_")
    try:
        C, shape, pixels, K, N = spec
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), "rocprofv3", "--kernel-trace", "-d", d, "-o", "trace", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--iters", str(iters), "--warmup", str(warmup), "--child", str(C), ",".join(map(str, shape)),
               str(pixels), str(K), str(N), str(n)]
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
    """-> dict of medians from the ordered trace of child(): the LAST 3 (warmup + iters) + 1 marks delimit the passes — the n-step inserts,
    then the one-step inserts, then the torch sequences."""
    n = warmup + iters
    marks = [i for i, k in enumerate(ks) if "policy_kernel" in k[2]]
    assert len(marks) >= 3 * n + 1, (len(marks), n)
    marks = marks[-(3 * n + 1):]
    segs = [ks[a + 1:b] for a, b in zip(marks[:-1], marks[1:])]
    us = lambda seg: sum(e - s for s, e, _ in seg) / 1e3
    span = lambda seg: (max(e for _, e, _ in seg) - seg[0][0]) / 1e3
    mine, ones, torchs = segs[warmup:n], segs[n + warmup:2 * n], segs[2 * n + warmup:3 * n]
    for seg in mine:
        assert len(seg) == 1 and "nstep_insert" in seg[0][2], [k[2] for k in seg]
    for seg in ones:
        assert len(seg) == 1 and "replay_insert" in seg[0][2], [k[2] for k in seg]
    assert not any("nstep_" in k[2] for seg in torchs for k in seg) and all("replay_insert" in seg[-1][2] for seg in torchs)
    name = lambda k: (re.search(r"(?:nstep|replay)_\w+<[^>]*>", k[2]) or re.search(r"(?:nstep|replay)_\w+", k[2])).group(0)
    a, b = _median([us(seg) for seg in mine]), _median([us(seg) for seg in ones])
    return {"nstep_insert_us": a, "onestep_insert_us": b, "ratio": a / b, "nstep_kernel": name(mine[0][0]), "onestep_kernel": name(ones[0][0]),
            "torch_kernels_us": _median([us(seg) for seg in torchs]), "torch_span_us": _median([span(seg) for seg in torchs]),
            "torch_launches": len(torchs[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", type=int, action="append", help="index into the shape list (default: all three)")
    ap.add_argument("--steps", type=int, action="append", help="n of the window (default: 1, 3 and 5)")
    ap.add_argument("--out", help="append the JSON lines to this file as well (profiles/nstep/nstep.jsonl)")
    ap.add_argument("--child", nargs=6, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        C, shape, pixels, K, N, n = a.child
        child(int(C), tuple(int(s) for s in shape.split(",")), int(pixels), int(K), int(N), int(n), a.iters, a.warmup)
        return
    for i, spec in enumerate(SHAPES):
        if a.only and i not in a.only:
            continue
        C, shape, pixels, K, N = spec
        W = 1
        for s in shape:
            W *= s
        W = W // 4 if pixels else W
        for n in a.steps or STEPS:
            ks, info = profile(spec, n, a.iters, a.warmup)      # a failed child raises: nothing more is started
            r = analyse(ks, a.iters, a.warmup)
            R = K * N
            row = {"C": C, "W": W, "K": K, "N": N, "n": n, "gamma": GAMMA, "rows_inserted": R}
            row.update({k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()})
            row.update({"speedup_vs_torch_kernels": round(r["torch_kernels_us"] / r["nstep_insert_us"], 2),
                        "speedup_vs_torch_span": round(r["torch_span_us"] / r["nstep_insert_us"], 2), "insert_bytes_per_row": insert_bytes(W),
                        "nstep_insert_gbs": round(R * insert_bytes(W) / r["nstep_insert_us"] / 1e3, 1), "source": "rocprofv3 kernel-trace (median)"})
            row.update({k: v for k, v in info.items() if k != "child"})
            line = json.dumps(row)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
