#!/usr/bin/env python3
"""Pendulum-v1 frames on the device, timed with `rocprofv3 --kernel-trace`, one child process per configuration:
  * `render` / `pixels`  one mxv_render launch (500 x 500 x 3 frames) / one mxv_pixels launch (84 x 84 gray) per launch of 1, 64, 1 024
                         and 4 096 frames, for Pendulum (arrow image attached, every env with an arrow) next to Acrobot (also 500 x 500);
  * `track`              the last_u launch behind each step(actions) of a Pendulum handle with an image, at 4 096 and 2^20 envs, next to
                         the step launch itself;
  * `track_sampled`      the same behind each step_sampled(): the redraw of the step's actions from the action stream (sample_kernel)
                         plus the last_u launch, next to the step launch.
Times are medians of the kernels' trace durations.

    python benchmarks/pendulum_frames.py [--iters 20] [--warmup 3]     # one JSON line per (kind, frames or envs, what)
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
ARROW = os.path.join(ROOT, "tests", "golden", "clockwise.png")
FRAMES = [1, 64, 1024, 4096]
TRACK_ENVS = [4096, 1 << 20]


def child_frames(gid, count, iters, warmup):
    import torch

    from gym_amd import pendulum_arrow_image
    from gym_amd.rollout import DeviceRollout

    pend = gid.startswith("Pendulum")
    r = DeviceRollout(gid, count, seed=1, action_seed=2, **({"arrow_image": pendulum_arrow_image(ARROW)} if pend else {}))
    r.reset(seed=1)
    if pend:   # every env shows an arrow: a step with torques across the range
        r.step(torch.linspace(-2, 2, count, device=r.device, dtype=torch.float32))
    idx = torch.arange(count, dtype=torch.int32, device=r.device)
    frames = r.render(idx)
    out = r.pixels(idx, height=84, width=84)
    with torch.cuda.stream(r.stream):
        for _ in range(warmup + iters):
            r.render(idx, out=frames)
        for _ in range(warmup + iters):
            r.pixels(idx, height=84, width=84, out=out)
    r.synchronize()
    r.close()


def child_track(count, iters, warmup, sampled=False):
    import torch

    from gym_amd import pendulum_arrow_image
    from gym_amd.rollout import DeviceRollout

    r = DeviceRollout("Pendulum-v1", count, seed=1, action_seed=2, arrow_image=pendulum_arrow_image(ARROW))
    r.reset(seed=1)
    a = torch.linspace(-3, 3, count, device=r.device, dtype=torch.float32)
    with torch.cuda.stream(r.stream):
        for _ in range(warmup + iters):
            if sampled:
                r.step_sampled(record_actions=False)
            else:
                r.step(a, want_final=False)
    r.synchronize()
    r.close()


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else float("nan")


def profile(args, iters, warmup):
    d = tempfile.mkdtemp(prefix="pendulum_frames_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "trace", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--iters", str(iters), "--warmup", str(warmup), "--child"] + [str(x) for x in args]
    subprocess.run(cmd, check=True, timeout=600)
    trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not trace:
        raise RuntimeError(f"rocprofv3 wrote no kernel trace under {d}")
    ks = []
    with open(trace[0]) as f:
        for rec in csv.DictReader(f):
            ks.append((int(rec["Start_Timestamp"]), rec.get("Kernel_Name", ""), (int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])) / 1e3))
    ks.sort()
    return ks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", nargs="+", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        if a.child[0] in ("track", "track_sampled"):
            child_track(int(a.child[1]), a.iters, a.warmup, sampled=a.child[0] == "track_sampled")
        else:
            child_frames(a.child[0], int(a.child[1]), a.iters, a.warmup)
        return
    src = "rocprofv3 kernel-trace (median)"
    for gid in ("Pendulum-v1", "Acrobot-v1"):
        for count in FRAMES:
            ks = profile([gid, count], a.iters, a.warmup)
            for what, name in (("render", "render_kernel"), ("pixels", "pixels_kernel")):
                t = [us for _, n, us in ks if name in n][1 + a.warmup:]
                us = _median(t)
                print(json.dumps({"kind": gid, "frames": count, "what": what + (" 84x84" if what == "pixels" else ""),
                                  "us_per_launch": round(us, 2), "frames_per_s": round(count / (us * 1e-6)), "source": src}), flush=True)
    for what in ("track", "track_sampled"):
        for count in TRACK_ENVS:
            ks = profile([what, count], a.iters, a.warmup)
            track = [us for _, n, us in ks if "track_step_kernel" in n][a.warmup:]
            redraw = [us for _, n, us in ks if "sample_kernel" in n][a.warmup:]
            step = [us for _, n, us in ks if "step_kernel" in n and "track" not in n][a.warmup:]
            row = {"kind": "Pendulum-v1", "envs": count, "what": what, "track_us": round(_median(track), 2)}
            if what == "track_sampled":
                row["redraw_us"] = round(_median(redraw), 2)
            row.update(step_us=round(_median(step), 2), source=src)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
