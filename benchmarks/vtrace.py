#!/usr/bin/env python3
"""V-trace targets and advantages over [K, N] rollouts: the one-launch kernel behind gym_amd.vtrace next to the torch
float64 K-loop of the same rule (episode cuts as selects, float32 results; its exp is torch's, not the rule's bit-defined EXP, so the
two agree to rounding, not bit for bit — `max_abs_diff` says how closely).  Timed with `rocprofv3 --kernel-trace`, one child process per
shape; times are medians over --iters calls of the kernels' trace durations:
  * `kernel_us`            the vtrace_kernel launch;
  * `torch_loop_kernel_us` the sum of the durations of every kernel one pass of the torch loop launches (what the GPU is busy for);
  * `torch_loop_span_us`   first kernel start to last kernel end of that pass (what the stream is held for: launch gaps included).
`roofline_frac` is the kernel's algorithmic bytes — 26 B per env-step without final_values (float32 log_prob, old_log_prob, reward and
values, two flag bytes, two float32 outputs) — over kernel_us, as a share of the 8 TB/s HBM peak.

    python benchmarks/vtrace.py [--iters 20] [--warmup 3]     # one JSON line per (K, N)
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
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
SHAPES = [(64, 4096), (128, 1 << 17), (32, 1 << 20), (16, 1 << 21)]      # the last one: from 2^21 envs on a lane owns four envs
BYTES = 26
HBM_PEAK_GBS = 8000.0
GAMMA, LAM, RHO_BAR, C_BAR = 0.99, 0.95, 1.0, 1.0


def torch_vtrace(torch, log_prob, old_log_prob, reward, terminated, truncated, values, last_value, vs, pg):
    acc, nv = torch.zeros_like(last_value, dtype=torch.float64), last_value.double()
    vs_next = nv
    zero = torch.zeros_like(acc)
    for k in range(reward.shape[0] - 1, -1, -1):
        w = (log_prob[k].double() - old_log_prob[k].double()).clamp(-80.0, 80.0).exp()
        rho = w.clamp(max=RHO_BAR)
        cs = LAM * w.clamp(max=C_BAR)
        done = (terminated[k] | truncated[k]) != 0
        v, r = values[k].double(), reward[k].double()
        nxt = torch.where(done, zero, nv)
        delta = rho * ((r + GAMMA * nxt) - v)
        acc = torch.where(done, delta, delta + (GAMMA * cs) * acc)
        target = acc + v
        pg[k] = rho * ((r + GAMMA * torch.where(done, nxt, vs_next)) - v)
        vs[k] = target
        vs_next, nv = target, v


def child(K, N, iters, warmup):
    import torch

    import gym_amd
    from gym_amd.vtrace import last_launch

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    reward, values, old_log_prob = (torch.randn((K, N), device=dev, generator=g) for _ in range(3))
    log_prob = old_log_prob + 0.3 * torch.randn((K, N), device=dev, generator=g)
    terminated, truncated = ((torch.rand((K, N), device=dev, generator=g) < 0.01).to(torch.uint8) for _ in range(2))
    last_value = torch.randn(N, device=dev, generator=g)
    vs, pg = torch.empty_like(reward), torch.empty_like(reward)
    tvs, tpg = torch.empty_like(reward), torch.empty_like(reward)
    one = torch.zeros((1, 1), device=dev)
    flag = torch.zeros((1, 1), dtype=torch.uint8, device=dev)
    mark_out = (torch.empty((1, 1), device=dev), torch.empty((1, 1), device=dev))

    def ours():
        gym_amd.vtrace(log_prob, old_log_prob, reward, terminated, truncated, values, last_value, gamma=GAMMA, lam=LAM, rho_bar=RHO_BAR,
                       c_bar=C_BAR, out=(vs, pg))

    def mark():     # a [1, 1] launch of the kernel: the delimiter between the passes of the torch loop in the trace
        gym_amd.vtrace(one, one, one, flag, flag, one, out=mark_out)

    for _ in range(warmup + iters):
        ours()
    torch.cuda.synchronize()
    mark()
    for _ in range(warmup + iters):
        torch_vtrace(torch, log_prob, old_log_prob, reward, terminated, truncated, values, last_value, tvs, tpg)
        mark()
    ours()
    torch.cuda.synchronize()
    diff = max(float((vs - tvs).abs().max()), float((pg - tpg).abs().max()))
    print(json.dumps({"child": True, "K": K, "N": N, "max_abs_diff": diff, "envs_per_lane": last_launch()[0]}), flush=True)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else float("nan")


def profile(K, N, iters, warmup):
    d = tempfile.mkdtemp(prefix="vtrace_bench_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "trace", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--iters", str(iters), "--warmup", str(warmup), "--child", str(K), str(N)]
        p = subprocess.run(cmd, check=True, timeout=900, capture_output=True, text=True)
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
    """-> (kernel_us, torch_loop_kernel_us, torch_loop_span_us, launches of one pass) from the ordered trace of child()."""
    n = warmup + iters
    ours = [i for i, k in enumerate(ks) if "vtrace_kernel" in k[2]]
    assert len(ours) == n + 1 + n + 1, (len(ours), n)      # the timed calls, the marks, the child's closing launch
    dur = lambda i: (ks[i][1] - ks[i][0]) / 1e3
    kernel = _median([dur(i) for i in ours[warmup:n]])
    marks = ours[n:2 * n + 1]
    sums, spans = [], []
    for a, b in list(zip(marks[:-1], marks[1:]))[warmup:]:
        seg = ks[a + 1:b]
        sums.append(sum(e - s for s, e, _ in seg) / 1e3)
        spans.append((max(e for _, e, _ in seg) - seg[0][0]) / 1e3)
    return kernel, _median(sums), _median(spans), len(ks[marks[0] + 1:marks[1]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", nargs=2, type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.iters, a.warmup)
        return
    for K, N in SHAPES:
        ks, info = profile(K, N, a.iters, a.warmup)
        us, loop_us, span_us, launches = analyse(ks, a.iters, a.warmup)
        gbs = K * N * BYTES / us / 1e3
        print(json.dumps({"K": K, "N": N, "kernel_us": round(us, 2), "torch_loop_kernel_us": round(loop_us, 2),
                          "torch_loop_span_us": round(span_us, 2), "torch_loop_launches": launches,
                          "speedup_vs_torch_loop_kernels": round(loop_us / us, 2), "envs_per_lane": info.get("envs_per_lane"),
                          "algorithmic_bytes_per_env_step": BYTES, "env_steps_per_us": round(K * N / us, 1),
                          "achieved_gbs": round(gbs, 1), "roofline_frac": round(gbs / HBM_PEAK_GBS, 4),
                          "max_abs_diff_vs_torch_loop": info.get("max_abs_diff"), "source": "rocprofv3 kernel-trace (median)"}), flush=True)


if __name__ == "__main__":
    main()
