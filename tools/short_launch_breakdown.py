"""Where one short fused launch's time goes (profiles/r7/r7_breakdown.md): the timed region of `bench.py --steps 20` — fence, event,
rollout_per_step(K), event, synchronize(), torch.cuda.synchronize() — repeated in one process at 2^20 CartPole envs on class-sorted
trajectory tensors.  Per iteration: wall time, event time of the launch, host time until rollout_per_step returns, host time inside
synchronize() (mxv_sync) and inside the device synchronise.  Run from the root of the tree under test (MXV_LIB_PATH selects a library):
    python tools/short_launch_breakdown.py --label parent --out DIR [--iters 200] [--only NAME]
Configurations: k20 (the tree's own arming of the final snapshot), k256, k20_attached / k20_detached (snapshot forced on / off), twice.
Under `rocprofv3 --kernel-trace --stats -- python tools/short_launch_breakdown.py --only k20 --iters 40 ...` the trace gives the
kernel's own duration and what is queued behind it."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())

ap = argparse.ArgumentParser()
ap.add_argument("--label", required=True)
ap.add_argument("--out", required=True)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--only", default=None)
ap.add_argument("--envs", type=int, default=1 << 20)
args = ap.parse_args()

import torch

from gym_amd.distributed import ShardedRollout

torch.cuda.set_device(0)
N = args.envs
sr = ShardedRollout("CartPole-v1", N, rank=0, world_size=1, device=0, seed=0, action_seed=1)
eng = sr.engine
sr.reset(seed=0)
traj256 = eng.trajectory_buffers(256, layout="sorted")
placement = dict(getattr(eng, "last_placement", None) or {})
traj20 = {k: v[:20] for k, v in traj256.items()}


def fence():
    sr.synchronize()
    torch.cuda.synchronize()


def summarize(xs):
    xs = sorted(xs)
    n = len(xs)
    return {"min": xs[0], "p10": xs[n // 10], "median": statistics.median(xs), "p90": xs[(9 * n) // 10], "max": xs[-1], "mean": sum(xs) / n}


def measure(K, traj, iters):
    rows = {k: [] for k in ("wall_us", "event_us", "host_launch_us", "host_event1_us", "host_sync_us", "host_devsync_us")}
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for i in range(iters):
        ev0, ev1 = evs[i]
        fence()
        t0 = time.perf_counter()
        ev0.record(eng.stream)
        sr.rollout_per_step(K, mode="fused", out=traj, record_actions=True)
        t1 = time.perf_counter()
        ev1.record(eng.stream)
        t2 = time.perf_counter()
        sr.synchronize()
        t3 = time.perf_counter()
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        rows["wall_us"].append((t4 - t0) * 1e6)
        rows["host_launch_us"].append((t1 - t0) * 1e6)
        rows["host_event1_us"].append((t2 - t1) * 1e6)
        rows["host_sync_us"].append((t3 - t2) * 1e6)
        rows["host_devsync_us"].append((t4 - t3) * 1e6)
    for ev0, ev1 in evs:
        rows["event_us"].append(ev0.elapsed_time(ev1) * 1e3)
    return rows


# settle clocks with the long launch first, as the bench does
t_end = time.perf_counter() + 3.0
while time.perf_counter() < t_end:
    sr.rollout_per_step(256, mode="fused", out=traj256, record_actions=True)
    sr.synchronize()
sr.reset(seed=0)

h = eng.handle
snap = None


def attach():
    global snap
    if snap is None:
        snap = [torch.empty_like(t) for t in eng.final_tensors()]
    h.set_final_snapshot(*snap)


configs = [("k20", 20, traj20, None), ("k256", 256, traj256, None), ("k20_attached", 20, traj20, "attach"),
           ("k20_detached", 20, traj20, "detach"), ("k20_attached_again", 20, traj20, "attach"), ("k20_detached_again", 20, traj20, "detach")]
result = {"label": args.label, "envs": N, "iters": args.iters, "placement": {k: placement.get(k) for k in ("kind", "balanced", "seconds", "mode")},
          "configs": {}}
raw = {}
for name, K, traj, snapmode in configs:
    if args.only and name != args.only:
        continue
    sr.rollout_per_step(K, mode="fused", out=traj, record_actions=True)   # the tree's own arming happens here
    if snapmode == "detach":
        h.set_final_snapshot()
    elif snapmode == "attach":
        attach()
    for _ in range(5):
        sr.rollout_per_step(K, mode="fused", out=traj, record_actions=True)
    fence()
    rows = measure(K, traj, args.iters)
    if snapmode is not None:
        h.set_final_snapshot()
    raw[name] = rows
    result["configs"][name] = {"K": K, "launch_info": h.last_launch(), **{k: summarize(v) for k, v in rows.items()}}
    s = result["configs"][name]
    print(f"[{args.label}] {name}: wall median {s['wall_us']['median']:.1f} us (min {s['wall_us']['min']:.1f}), event {s['event_us']['median']:.1f}, "
          f"launch host {s['host_launch_us']['median']:.1f}, sync host {s['host_sync_us']['median']:.1f}, devsync {s['host_devsync_us']['median']:.1f}", flush=True)

os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, f"breakdown_{args.label}.json"), "w") as f:
    json.dump(result, f, indent=1)
with open(os.path.join(args.out, f"breakdown_{args.label}_raw.json"), "w") as f:
    json.dump({k: {m: [round(x, 2) for x in v] for m, v in rows.items()} for k, rows in raw.items()}, f)
sr.close()
