#!/usr/bin/env python3
"""Pixel observations on the device: per renderable kind, envs per launch and observation size,
  * `pixels`     one mxv_pixels launch (render -> gray -> area resize fused, nothing but the observations written);
  * `composite`  what a user assembles without it: mxv_render full frames, then torch gray + adaptive_avg_pool2d + rounding, on the
                 same stream (integer gray over the whole batch: int32 temporaries of several GB at 4 096 frames);
  * `composite_lean` the same frames reduced as a careful user would: uint8 read once, float32 64 frames at a time (gray as a
                 weighted sum of the channels), pooled and rounded into a preallocated output;
  * `step`       one full PixelRollout.step (stack=4): dynamics, stack shift, newest frame, final stacks, masked reset, reset frames.

    python benchmarks/pixels.py                 # CUDA-event timings, one JSON line per (kind, envs, size, what)
    python benchmarks/pixels.py --rocprof       # the same launches under `rocprofv3 --kernel-trace --stats`, one child process per
                                                # (kind, envs, size); times are sums of the kernels of one iteration (median)
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

KINDS = ["CartPole-v1", "Acrobot-v1", "MountainCar-v0", "MountainCarContinuous-v0"]
COUNTS = [64, 1024, 4096]
SIZES = [(84, 84, True), (100, 150, False)]     # (height, width, grayscale)
STACK = 4


def _composite(r, idx, frames, h, w, gray):
    import torch

    r.render(idx, out=frames)
    f = frames.to(torch.int32)
    if gray:
        f = ((4899 * f[..., 0] + 9617 * f[..., 1] + 1868 * f[..., 2] + 8192) >> 14)[:, None]
    else:
        f = f.permute(0, 3, 1, 2)
    step = max(1, (2 ** 31 - 1) // (f[0].numel()))              # adaptive_avg_pool2d's HIP kernel takes < 2^31 elements per call
    p = torch.cat([torch.nn.functional.adaptive_avg_pool2d(c.float(), (h, w)) for c in f.split(step)])
    out = torch.floor(p + 0.5).to(torch.uint8)
    return out[:, 0] if gray else out.permute(0, 2, 3, 1).contiguous()


GRAY_W = (4899 / 16384, 9617 / 16384, 1868 / 16384)
LEAN_CHUNK = 64                                                  # frames per piece: 46 MB of uint8, its float32 copy stays in cache


def _composite_lean(r, idx, frames, h, w, gray, out, wts):
    """The same chain as a careful user writes it: frames read once as uint8, converted to float32 64 frames at a time (gray as a
    weighted sum of the channels), pooled and rounded into a preallocated output."""
    import torch

    r.render(idx, out=frames)
    for s in range(0, frames.shape[0], LEAN_CHUNK):
        c = frames[s:s + LEAN_CHUNK]
        if gray:
            x = c.float()
            x = x[..., 0].mul(wts[0]).add_(x[..., 1], alpha=wts[1]).add_(x[..., 2], alpha=wts[2])[:, None]
        else:
            x = c.permute(0, 3, 1, 2).float()
        p = torch.nn.functional.adaptive_avg_pool2d(x, (h, w)).add_(0.5).floor_()
        out[s:s + LEAN_CHUNK].copy_(p[:, 0] if gray else p.permute(0, 2, 3, 1))


def run_config(gid, count, size, iters, warmup, timed=True):
    """composite, lean composite, then pixels, then PixelRollout.step, in this order (the --rocprof parser relies on it)."""
    import torch

    from gym_amd.pixels import PixelRollout
    from gym_amd.rollout import DeviceRollout

    h, w, gray = size
    rows = []
    r = DeviceRollout(gid, count, seed=1, action_seed=2)
    r.reset(seed=1)
    idx = torch.arange(count, dtype=torch.int32, device=r.device)
    frames = r.render(idx)
    out = r.pixels(idx, height=h, width=w, grayscale=gray)
    r.stream.synchronize()

    def timeit(fn, n_warm):
        with torch.cuda.stream(r.stream):
            for _ in range(n_warm):
                fn()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(r.stream)
            for _ in range(iters):
                fn()
            stop.record(r.stream)
        r.stream.synchronize()
        return start.elapsed_time(stop) / iters * 1e3

    us_c = timeit(lambda: _composite(r, idx, frames, h, w, gray), warmup)
    with torch.cuda.stream(r.stream):
        wts = GRAY_W
        lean_out = torch.empty_like(out)
    us_l = timeit(lambda: _composite_lean(r, idx, frames, h, w, gray, lean_out, wts), warmup)
    us_p = timeit(lambda: r.pixels(idx, height=h, width=w, grayscale=gray, out=out), warmup)
    r.handle.sync()
    r.close()
    pr = PixelRollout(gid, count, height=h, width=w, grayscale=gray, stack=STACK, seed=1, action_seed=2)
    pr.reset()
    pr.synchronize()
    with torch.cuda.stream(pr.stream):
        for _ in range(warmup):
            pr.step(None)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(pr.stream)
        for _ in range(iters):
            pr.step(None)
        stop.record(pr.stream)
    pr.synchronize()
    us_s = start.elapsed_time(stop) / iters * 1e3
    pr.close()
    if timed:
        for what, us in (("composite", us_c), ("composite_lean", us_l), ("pixels", us_p), ("step", us_s)):
            rows.append(row(gid, count, size, what, us, "cuda_events"))
        rows.append(ratio(gid, count, size, us_c, us_p, "cuda_events"))
        rows.append(ratio(gid, count, size, us_l, us_p, "cuda_events", "composite_lean / pixels"))
    return rows


def row(gid, count, size, what, us, source):
    h, w, gray = size
    return {"kind": gid, "envs": count, "size": f"{h}x{w}{'' if gray else 'x3'}", "what": what, "us_per_launch": round(us, 2),
            "frames_per_s": round(count / (us * 1e-6)), "source": source}


def ratio(gid, count, size, us_c, us_p, source, what="composite / pixels"):
    h, w, gray = size
    return {"kind": gid, "envs": count, "size": f"{h}x{w}{'' if gray else 'x3'}", "what": what,
            "ratio": round(us_c / us_p, 2), "source": source}


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else float("nan")


def rocprof_config(gid, count, size, iters, warmup):
    d = tempfile.mkdtemp(prefix="pixels_prof_")
    h, w, gray = size
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "pixels", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--child", gid, str(count), str(h), str(w), str(int(gray)),
           "--iters", str(iters), "--warmup", str(warmup)]
    subprocess.run(cmd, check=True, timeout=900)
    trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not trace:
        return [{"rocprof": "no kernel trace written", "dir": d}]
    ks = []
    with open(trace[0]) as f:
        for rec in csv.DictReader(f):
            ks.append((int(rec["Start_Timestamp"]), rec.get("Kernel_Name", ""),
                       (int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])) / 1e3))
    ks = [(n, t) for _, n, t in sorted(ks)]                      # program order (one stream at a time)
    rend = [i for i, (n, _) in enumerate(ks) if "render_kernel" in n]
    pix = [i for i, (n, _) in enumerate(ks) if "pixels_kernel" in n]
    # run_config's order: one render and one pixels launch of set-up; warmup + iters composite iterations, then as many lean composite
    # iterations (each starts at its render launch and ends before the next one, the last before the first pixels launch of the next
    # phase); warmup + iters pixels launches; PixelRollout.reset (one pixels launch); warmup + iters steps (each ends with its second
    # pixels launch)
    comp_its = rend[1:]
    P = 1 + warmup + iters
    comp = [sum(t for _, t in ks[a:b]) for a, b in zip(comp_its, comp_its[1:] + [pix[1]])]
    lean = comp[2 * warmup + iters:]
    pixl = [ks[i][1] for i in pix[1 + warmup:P]]
    steps = [sum(t for _, t in ks[pix[P + 2 * j] + 1:pix[P + 2 * j + 2] + 1]) for j in range(warmup, warmup + iters)
             if P + 2 * j + 2 < len(pix)]
    src = "rocprofv3 kernel-trace (median, kernel sums)"
    us_c, us_l, us_p, us_s = _median(comp[warmup:warmup + iters]), _median(lean), _median(pixl), _median(steps)
    return [row(gid, count, size, "composite", us_c, src), row(gid, count, size, "composite_lean", us_l, src),
            row(gid, count, size, "pixels", us_p, src), row(gid, count, size, "step", us_s, src),
            ratio(gid, count, size, us_c, us_p, src), ratio(gid, count, size, us_l, us_p, src, "composite_lean / pixels")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--child", nargs=5, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        gid, count, h, w, gray = a.child
        run_config(gid, int(count), (int(h), int(w), bool(int(gray))), a.iters, a.warmup, timed=False)
        return
    for gid in a.kinds.split(","):
        for count in COUNTS:
            for size in SIZES:
                rows = rocprof_config(gid, count, size, a.iters, a.warmup) if a.rocprof else run_config(gid, count, size, a.iters, a.warmup)
                for r in rows:
                    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
