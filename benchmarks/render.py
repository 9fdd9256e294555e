#!/usr/bin/env python3
"""rgb_array frames on the device: frames per second and the share of the HBM store roofline of one mxv_render launch,
for 1, 64, 1 024 and 4 096 frames per launch and every renderable kind, plus the host render() cost of one env (HipEnv.render(): the
launch, the D2H copy of one frame and the synchronisation).

    python benchmarks/render.py                 # CUDA-event timings, one JSON line per (kind, frames)
    python benchmarks/render.py --rocprof       # the same launches under `rocprofv3 --kernel-trace --stats` in a child process of
                                                # its own; kernel times come from its stats (render_kernel rows)

Roofline: frames x H x W x 3 bytes at 8 TB/s (the MI355X's HBM3E peak); the launch is store-bound by design.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KINDS = ["CartPole-v1", "Acrobot-v1", "MountainCar-v0", "MountainCarContinuous-v0"]
COUNTS = [1, 64, 1024, 4096]
HBM_BYTES_PER_S = 8e12


def frame_bytes(gid):
    return (500 * 500 if gid.startswith("Acrobot") else 400 * 600) * 3


def run_launches(iters, warmup, timed=True):
    import torch

    from gym_amd.rollout import DeviceRollout

    out = []
    for gid in KINDS:
        r = DeviceRollout(gid, max(COUNTS), seed=1, action_seed=2)
        r.reset(seed=1)
        for count in COUNTS:
            idx = torch.arange(count, dtype=torch.int32, device=r.device)
            frames = r.render(idx)
            with torch.cuda.stream(r.stream):
                for _ in range(warmup):
                    r.render(idx, out=frames)
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(r.stream)
                for _ in range(iters):
                    r.render(idx, out=frames)
                stop.record(r.stream)
            r.stream.synchronize()
            r.handle.sync()
            if timed:
                ms = start.elapsed_time(stop) / iters
                out.append(row(gid, count, ms * 1e3, "cuda_events"))
            del frames
        r.close()
    return out


def row(gid, count, us, source):
    b = count * frame_bytes(gid)
    return {"kind": gid, "frames": count, "us_per_launch": round(us, 2), "frames_per_s": round(count / (us * 1e-6)),
            "bytes": b, "store_roofline_share": round(b / HBM_BYTES_PER_S / (us * 1e-6), 3), "source": source}


def host_render_cost(reps=50):
    from gym_amd.single_env import HipEnv

    res = []
    for gid in KINDS:
        env = HipEnv(gid, render_mode="rgb_array")
        env.reset(seed=0)
        for _ in range(5):
            env.render()
        t = time.perf_counter()
        for _ in range(reps):
            env.render()
        res.append({"kind": gid, "host_render_us": round((time.perf_counter() - t) / reps * 1e6, 1), "source": "HipEnv.render"})
        env.close()
    return res


def rocprof_rows(iters, warmup):
    d = tempfile.mkdtemp(prefix="render_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "render", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--child", "--iters", str(iters), "--warmup", str(warmup)]
    subprocess.run(cmd, check=True, timeout=900)
    trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not trace:
        return [{"rocprof": "no kernel trace written", "dir": d}]
    launches = []
    with open(trace[0]) as f:
        for rec in csv.DictReader(f):
            if "render_kernel" in rec.get("Kernel_Name", ""):
                launches.append((int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])) / 1e3)
    # launches come in program order: per kind, per count, 1 + warmup + iters launches
    out, k = [], 0
    per = 1 + warmup + iters
    for gid in KINDS:
        for count in COUNTS:
            timed = list(launches[k + 1 + warmup:k + per])
            k += per
            if timed:
                timed.sort()
                out.append(row(gid, count, timed[len(timed) // 2], "rocprofv3 kernel-trace (median)"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        run_launches(a.iters, a.warmup, timed=False)
        return
    rows = rocprof_rows(a.iters, a.warmup) if a.rocprof else run_launches(a.iters, a.warmup) + host_render_cost()
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
