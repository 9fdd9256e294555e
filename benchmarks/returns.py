#!/usr/bin/env python3
"""GAE(lambda) advantages and discounted returns over [K, N] rollouts: the one-launch kernel behind gym_amd.gae /
gym_amd.discounted_returns next to the torch K-loop it replaces — the loop of examples/policy_gradient_graphed.py generalised to the same
rule (float64 arithmetic, episode cuts as selects, float32 results).  Timed with `rocprofv3 --kernel-trace`, one child process per
shape; times are medians over --iters calls of the kernels' trace durations:
  * `kernel_us`            the gae_kernel launch;
  * `torch_loop_kernel_us` the sum of the durations of every kernel one pass of the torch loop launches (what the GPU is busy for);
  * `torch_loop_span_us`   first kernel start to last kernel end of that pass (what the stream is held for: launch gaps included).
`roofline_frac` is the kernel's algorithmic bytes — 18 B per env-step for GAE without final_values (float32 reward and values, two flag
bytes, two float32 outputs), 10 B for returns — over kernel_us, as a share of the 8 TB/s HBM peak.

    python benchmarks/returns.py [--iters 20] [--warmup 3]     # one JSON line per (K, N, what)
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
BYTES = {"gae": 18, "returns": 10}
HBM_PEAK_GBS = 8000.0
GAMMA, LAM = 0.99, 0.95


def torch_gae(torch, reward, terminated, truncated, values, last_value, adv, ret):
    c = GAMMA * LAM
    A, nv = torch.zeros_like(last_value, dtype=torch.float64), last_value.double()
    zero = torch.zeros_like(A)
    for k in range(reward.shape[0] - 1, -1, -1):
        done = (terminated[k] | truncated[k]) != 0
        v = values[k].double()
        delta = (reward[k].double() + GAMMA * torch.where(done, zero, nv)) - v
        A = torch.where(done, delta, delta + c * A)
        adv[k] = A
        ret[k] = A + v
        nv = v


def torch_returns(torch, reward, terminated, truncated, last_value, ret):
    G = last_value.double()
    zero = torch.zeros_like(G)
    for k in range(reward.shape[0] - 1, -1, -1):
        done = (terminated[k] | truncated[k]) != 0
        G = reward[k].double() + GAMMA * torch.where(done, zero, G)
        ret[k] = G


def child(K, N, iters, warmup):
    import torch

    import gym_amd

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    reward, values = (torch.randn((K, N), device=dev, generator=g) for _ in range(2))
    terminated, truncated = ((torch.rand((K, N), device=dev, generator=g) < 0.01).to(torch.uint8) for _ in range(2))
    last_value = torch.randn(N, device=dev, generator=g)
    adv, ret = torch.empty_like(reward), torch.empty_like(reward)
    tadv, tret = torch.empty_like(reward), torch.empty_like(reward)
    one = torch.zeros((1, 1), device=dev)
    flag = torch.zeros((1, 1), dtype=torch.uint8, device=dev)
    mark_out = torch.empty((1, 1), device=dev)

    def mark():     # a [1, 1] launch of the kernel: the delimiter between the passes of the torch loop in the trace
        gym_amd.discounted_returns(one, flag, flag, out=mark_out)

    for _ in range(warmup + iters):
        gym_amd.gae(reward, terminated, truncated, values, last_value, gamma=GAMMA, lam=LAM, out=(adv, ret))
    for _ in range(warmup + iters):
        gym_amd.discounted_returns(reward, terminated, truncated, gamma=GAMMA, last_value=last_value, out=ret)
    torch.cuda.synchronize()
    mark()
    for _ in range(warmup + iters):
        torch_gae(torch, reward, terminated, truncated, values, last_value, tadv, tret)
        mark()
    gym_amd.gae(reward, terminated, truncated, values, last_value, gamma=GAMMA, lam=LAM, out=(adv, ret))
    torch.cuda.synchronize()
    # the two compute the same thing: the loop in torch's float64 ops, one rounding each, agrees with the kernel bit for bit
    same = bool(torch.equal(adv.view(torch.int32), tadv.view(torch.int32)) and torch.equal(ret.view(torch.int32), tret.view(torch.int32)))
    mark()
    for _ in range(warmup + iters):
        torch_returns(torch, reward, terminated, truncated, last_value, tret)
        mark()
    torch.cuda.synchronize()
    from gym_amd.returns import last_launch

    gym_amd.gae(reward, terminated, truncated, values, last_value, gamma=GAMMA, lam=LAM, out=(adv, ret))
    torch.cuda.synchronize()
    print(json.dumps({"child": True, "K": K, "N": N, "torch_loop_equals_kernel": same, "envs_per_lane": last_launch()[0]}), flush=True)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else float("nan")


def profile(K, N, iters, warmup):
    d = tempfile.mkdtemp(prefix="returns_bench_")
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
    """-> {what: (kernel_us, torch_loop_kernel_us, torch_loop_span_us)} from the ordered trace of child()."""
    n = warmup + iters
    ours = [i for i, k in enumerate(ks) if "gae_kernel" in k[2]]
    assert len(ours) == 2 * n + 1 + n + 2 + n + 1, (len(ours), n)      # + the child's closing launch
    dur = lambda i: (ks[i][1] - ks[i][0]) / 1e3
    kernel = {"gae": _median([dur(i) for i in ours[warmup:n]]), "returns": _median([dur(i) for i in ours[n + warmup:2 * n]])}
    marks = {"gae": ours[2 * n:3 * n + 1], "returns": ours[3 * n + 2:4 * n + 3]}
    out = {}
    for what, m in marks.items():
        sums, spans = [], []
        for a, b in list(zip(m[:-1], m[1:]))[warmup:]:
            seg = ks[a + 1:b]
            sums.append(sum(e - s for s, e, _ in seg) / 1e3)
            spans.append((max(e for _, e, _ in seg) - seg[0][0]) / 1e3)
        out[what] = (kernel[what], _median(sums), _median(spans), len(ks[m[0] + 1:m[1]]))
    return out


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
        same = info.get("torch_loop_equals_kernel")
        for what, (us, loop_us, span_us, launches) in analyse(ks, a.iters, a.warmup).items():
            gbs = K * N * BYTES[what] / us / 1e3
            print(json.dumps({"K": K, "N": N, "what": what, "kernel_us": round(us, 2), "torch_loop_kernel_us": round(loop_us, 2),
                              "torch_loop_span_us": round(span_us, 2), "torch_loop_launches": launches,
                              "speedup_vs_torch_loop_kernels": round(loop_us / us, 2), "envs_per_lane": info.get("envs_per_lane"),
                              "algorithmic_bytes_per_env_step": BYTES[what],
                              "achieved_gbs": round(gbs, 1), "roofline_frac": round(gbs / HBM_PEAK_GBS, 4),
                              "torch_loop_equals_kernel": same if what == "gae" else None,
                              "source": "rocprofv3 kernel-trace (median)"}), flush=True)


if __name__ == "__main__":
    main()
