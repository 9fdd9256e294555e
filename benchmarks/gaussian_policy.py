#!/usr/bin/env python3
"""Diagonal-Gaussian policy draws from mean and log_std: the one-launch kernel behind gym_amd.sample_gaussian next to
the torch sequence it replaces — log_std.exp(), randn_like, mean + std * eps, the Normal.log_prob arithmetic and its sum over the action
dims, the entropy sum, and the casts to float32.  Timed with `rocprofv3 --kernel-trace`, one child process per shape; times are medians
over --iters calls of the kernels' trace durations:
  * `kernel_us`              the gaussian_kernel launch (step given by the host);
  * `with_counter_span_us`   start of gaussian_kernel to end of the single-lane kernel that advances the device step counter (2 launches);
  * `torch_kernel_us`        the sum of the durations of every kernel one pass of the torch sequence launches;
  * `torch_span_us`          first kernel start to last kernel end of that pass (launch gaps included); `torch_launches` their number.
`achieved_gbs` is the kernel's algorithmic bytes — 4 D each of mean, log_std and actions, 8 of log_prob and entropy per env — over
kernel_us; `fp64_gflops` counts the rule's float64 operations per env (OPS_PER_PAIR per Box-Muller pair, OPS_PER_DIM per dim).

    python benchmarks/gaussian_policy.py [--iters 20] [--warmup 3]     # one JSON line per (N, D)
"""
import argparse
import csv
import glob
import json
import math
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
SHAPES = [(4096, 1), (4096, 4), (1 << 20, 1), (1 << 20, 4)]
HBM_PEAK_GBS = 8000.0
OPS_PER_PAIR = 95      # u01, LOG (division counted once), sqrt, SINCOS2PI, the two products
OPS_PER_DIM = 45       # EXP, the action, zq (division counted once), the log_prob and entropy terms


def torch_sequence(torch, mean, log_std):
    std = log_std.exp()
    eps = torch.randn_like(mean)
    act = mean + std * eps
    zq = (act - mean) / std
    log_prob = (-0.5 * zq * zq - log_std - 0.5 * math.log(2.0 * math.pi)).sum(dim=-1)
    entropy = (log_std + (0.5 + 0.5 * math.log(2.0 * math.pi))).sum(dim=-1)
    return act.to(torch.float32), log_prob.to(torch.float32), entropy.to(torch.float32)


def child(N, D, iters, warmup):
    import torch

    import gym_amd

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    mean = torch.randn((N, D), device=dev, generator=g)
    log_std = torch.rand((N, D), device=dev, generator=g) * 2.0 - 1.5
    out = (torch.empty((N, D), device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev))
    one = torch.zeros((1, 1), device=dev)
    mark_out = (torch.empty((1, 1), device=dev), None, None)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)

    def mark():     # a [1, 1] launch of the kernel: the delimiter between the passes of the torch sequence in the trace
        gym_amd.sample_gaussian(one, one, seed=0, step=0, out=mark_out)

    for i in range(warmup + iters):
        gym_amd.sample_gaussian(mean, log_std, seed=1, step=i, out=out)
    for _ in range(warmup + iters):
        gym_amd.sample_gaussian(mean, log_std, seed=1, step=counter, out=out)
    torch.cuda.synchronize()
    mark()
    for _ in range(warmup + iters):
        torch_sequence(torch, mean, log_std)
        mark()
    torch.cuda.synchronize()
    # the two agree as far as float32 library calls do: log pi of the kernel's own actions and the entropies
    a, lp, en = gym_amd.sample_gaussian(mean, log_std, seed=1, step=0)
    dist = torch.distributions.Normal(mean.double(), log_std.double().exp())
    err_lp = float((dist.log_prob(a.double()).sum(-1) - lp.double()).abs().max())
    err_en = float((dist.entropy().sum(-1) - en.double()).abs().max())
    z = (a.double() - mean.double()) / log_std.double().exp()
    print(json.dumps({"child": True, "N": N, "D": D, "max_abs_diff_log_prob_vs_torch_f64": err_lp, "max_abs_diff_entropy_vs_torch_f64": err_en,
                      "z_mean": float(z.mean()), "z_var": float(z.var()), "counter": int(counter.item())}), flush=True)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else float("nan")


def profile(N, D, iters, warmup):
    d = tempfile.mkdtemp(prefix="gaussian_bench_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "trace", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--iters", str(iters), "--warmup", str(warmup), "--child", str(N), str(D)]
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
    """-> (kernel_us, with_counter_span_us, torch_kernel_us, torch_span_us, torch_launches) from the ordered trace of child()."""
    n = warmup + iters
    ours = [i for i, k in enumerate(ks) if "gaussian_kernel" in k[2]]
    assert len(ours) == 3 * n + 1 + 1, (len(ours), n)      # + the child's closing launch
    dur = lambda i: (ks[i][1] - ks[i][0]) / 1e3
    kernel = _median([dur(i) for i in ours[warmup:n]])
    with_counter = []
    for i in ours[n + warmup:2 * n]:
        assert "add_word" in ks[i + 1][2], ks[i + 1][2]
        with_counter.append((ks[i + 1][1] - ks[i][0]) / 1e3)
    marks = ours[2 * n:3 * n + 1]
    sums, spans = [], []
    for a, b in list(zip(marks[:-1], marks[1:]))[warmup:]:
        seg = ks[a + 1:b]
        sums.append(sum(e - s for s, e, _ in seg) / 1e3)
        spans.append((max(e for _, e, _ in seg) - seg[0][0]) / 1e3)
    return kernel, _median(with_counter), _median(sums), _median(spans), len(ks[marks[0] + 1:marks[1]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", nargs=2, type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.iters, a.warmup)
        return
    for N, D in SHAPES:
        ks, info = profile(N, D, a.iters, a.warmup)
        us, counter_us, torch_us, span_us, launches = analyse(ks, a.iters, a.warmup)
        per_env = 12 * D + 8
        gbs = N * per_env / us / 1e3
        flops = N * (OPS_PER_PAIR * ((D + 1) // 2) + OPS_PER_DIM * D) / us / 1e3
        print(json.dumps({"N": N, "D": D, "kernel_us": round(us, 2), "launches": 1, "with_counter_span_us": round(counter_us, 2),
                          "with_counter_launches": 2, "torch_kernel_us": round(torch_us, 2), "torch_span_us": round(span_us, 2),
                          "torch_launches": launches, "speedup_vs_torch_kernels": round(torch_us / us, 2),
                          "speedup_vs_torch_span": round(span_us / us, 2),
                          "algorithmic_bytes_per_env": per_env, "achieved_gbs": round(gbs, 1), "roofline_frac": round(gbs / HBM_PEAK_GBS, 4),
                          "fp64_gflops": round(flops, 1),
                          "max_abs_diff_log_prob_vs_torch_f64": info.get("max_abs_diff_log_prob_vs_torch_f64"),
                          "max_abs_diff_entropy_vs_torch_f64": info.get("max_abs_diff_entropy_vs_torch_f64"),
                          "z_mean": info.get("z_mean"), "z_var": info.get("z_var"),
                          "source": "rocprofv3 kernel-trace (median)"}), flush=True)


if __name__ == "__main__":
    main()
