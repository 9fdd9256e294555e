#!/usr/bin/env python3
"""The quantile-regression (QR-DQN) value-based update, fused: gym_amd.quantile_dqn_loss in the bootstrap mode with
next_quantiles_online (double DQN), a per-row discount, weights and row_loss — the forward alone, and the forward with loss.backward() —
next to the literal torch float32 sequence on the same inputs: the mean over the quantiles, argmax, gather, the Bellman step, the
[M, N, N] tensor of pairwise errors, huber, |tau - 1{u < 0}|, the mean over the targets, the sum over the head, the weights, .mean(),
and autograd behind it.  Neither side reads anything back inside the timed window.

Two modes, never in one process:
  * the default: end-to-end times with the profiler off.  One child process per shape under `timeout -k 10`, stopping at the first
    child that fails.  A window is --passes passes between two device events, ending in a synchronise; the four kinds of pass (ours
    and torch's, forward and forward + backward) alternate window by window, --reps windows each after --warmup; the figures are
    medians with the quartiles beside them.
  * --trace: `rocprofv3 --kernel-trace` around one child per shape (no counters: they are never combined with tracing; the program goes
    after `--`): the median duration of qr_rows, of qr_leaf with its qr_tree levels, and of qr_bwd over the passes.
`achieved_gbs` is the algorithmic bytes of the two calls over the traced kernel time, `fp64_gops` the rule's float64 operations by the
model of `ops_per_row` (a count of the rule's lines, not of instructions) over the same.

The torch sequence materialises [M, N, N] float32 tensors several times over: where ten of them would not fit --torch-limit-gib the
torch side is not run at that shape and the line says so.

    python benchmarks/qr_loss.py [--passes 10] [--reps 15] [--warmup 3] [--trace]     # one JSON line per shape
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
SHAPES = tuple((M, A, N) for M in (256, 2048, 32768, 1 << 20) for A, N in ((2, 51), (6, 32), (18, 64)))
HBM_PEAK_GBS = 8000.0
KAPPA = 1.0
CHILD_TIMEOUT_S = 600
TORCH_LIVE_TENSORS = 10      # [M, N, N] float32 tensors the torch sequence and its autograd graph hold at once, about


def bytes_per_row(A, N):
    """forward: the taken row 4 N (and its neighbours again for the crossing count: the same lines), action 8, reward 4, terminated 1,
    discount 4, weight 4, the selecting head 4 A N, next_quantiles[i, j*] 4 N, six float64 columns written and read again, row_loss 4;
    backward: the same reads, and the gradient row 4 A N."""
    reads = 8 * N + 21 + 4 * A * N
    return (reads + 2 * 48 + 4) + (reads + 4 * A * N)


def ops_per_row(A, N):
    """float64 operations of the rule per row, both calls: 13 per (j, k) pair (the difference, the square and its half or the linear
    branch, two quotients, two products, two sums, the selects not counted), a butterfly of 6 per lane for each of A + 5 sums over the
    quantiles; the backward recomputes all of it."""
    return 2 * (13 * N * N + 6 * 64 * (A + 5))


def torch_pass(torch, quantiles, actions, reward, terminated, next_q, next_online, discount, weights, backward=True):
    """The literal torch sequence of a quantile double-DQN update with n-step discounts, without the optimizer."""
    M, A, N = quantiles.shape
    rows = torch.arange(M, device=quantiles.device)
    tau = (2 * torch.arange(N, device=quantiles.device, dtype=quantiles.dtype) + 1) / (2 * N)
    with torch.no_grad():
        nv = next_q[rows, next_online.mean(-1).argmax(1)]
        T = reward[:, None] + (discount * (1 - terminated.to(quantiles.dtype)))[:, None] * nv
    th = quantiles[rows, actions]
    u = T[:, None, :] - th[:, :, None]
    au = u.abs()
    hub = torch.where(au <= KAPPA, 0.5 * u * u, KAPPA * (au - 0.5 * KAPPA))
    rho = (tau[None, :, None] - (u.detach() < 0).to(quantiles.dtype)).abs() * hub / KAPPA
    ql = rho.mean(2).sum(1)
    loss = (ql * weights).mean()
    if backward:
        loss.backward()
    return loss, ql


def fused_pass(gym_amd, row_loss, quantiles, actions, reward, terminated, next_q, next_online, discount, weights, backward=True):
    loss, stats = gym_amd.quantile_dqn_loss(quantiles, actions, reward=reward, terminated=terminated, next_quantiles=next_q,
                                            next_quantiles_online=next_online, discount=discount, kappa=KAPPA, weights=weights, row_loss=row_loss)
    if backward:
        loss.backward()
    return loss, stats


def inputs(torch, M, A, N):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    quantiles = (torch.randn((M, A, N), device=dev, generator=g) * 2.0).sort(-1).values.contiguous().requires_grad_()
    next_q = (torch.randn((M, A, N), device=dev, generator=g) * 2.0).sort(-1).values.contiguous()
    next_online = next_q + 0.7 * torch.randn((M, A, 1), device=dev, generator=g)
    actions = torch.randint(0, A, (M,), device=dev, generator=g)
    reward = torch.randn(M, device=dev, generator=g)
    terminated = torch.rand(M, device=dev, generator=g) < 0.1
    discount = torch.tensor(0.99, device=dev) ** torch.randint(1, 4, (M,), device=dev, generator=g)
    weights = torch.rand(M, device=dev, generator=g) * 1.8 + 0.2
    return quantiles, actions, reward, terminated, next_q, next_online, discount, weights


def torch_fits(M, N, limit_gib):
    return TORCH_LIVE_TENSORS * M * N * N * 4 <= limit_gib * (1 << 30)


def agreement(torch, gym_amd, args, with_torch):
    """The two sides on the same inputs, the torch one in float64: how far the float32 results are from it."""
    quantiles = args[0]
    row_loss = torch.empty(quantiles.shape[0], device=quantiles.device)
    quantiles.grad = None
    loss, stats = fused_pass(gym_amd, row_loss, *args)
    out = {"loss": float(loss), "crossing_fraction": float(stats[4])}
    if with_torch:
        x64 = quantiles.detach().double().requires_grad_()
        ref, ql = torch_pass(torch, x64, args[1], args[2].double(), args[3], args[4].double(), args[5].double(), args[6].double(), args[7].double())
        out.update({"loss_torch_f64": float(ref), "max_abs_diff_row_loss_vs_torch_f64": float((row_loss.double() - ql).abs().max()),
                    "max_abs_diff_grad_vs_torch_f64": float((quantiles.grad.double() - x64.grad).abs().max())})
    return out


def child_events(M, A, N, passes, reps, warmup, with_torch):
    import torch

    import gym_amd

    args = inputs(torch, M, A, N)
    quantiles = args[0]
    row_loss = torch.empty(M, device=quantiles.device)

    def window(f):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(passes):
            quantiles.grad = None
            f()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e3 / passes      # microseconds a pass

    def no_grad(f):
        def g():
            with torch.no_grad():
                f(backward=False)
        return g

    kinds = {"fwd_us": no_grad(lambda backward: fused_pass(gym_amd, row_loss, *args, backward=backward)),
             "fwd_bwd_us": lambda: fused_pass(gym_amd, row_loss, *args)}
    if with_torch:
        kinds["torch_fwd_us"] = no_grad(lambda backward: torch_pass(torch, *args, backward=backward))
        kinds["torch_fwd_bwd_us"] = lambda: torch_pass(torch, *args)
    times = {k: [] for k in kinds}
    for rep in range(warmup + reps):      # the kinds alternate window by window
        for k, f in kinds.items():
            t = window(f)
            if rep >= warmup:
                times[k].append(t)
    out = {"child": True}
    for k, v in times.items():
        v = sorted(v)
        out[k] = round(v[len(v) // 2], 2)
        out[k.replace("_us", "_q1_q3_us")] = [round(v[len(v) // 4], 2), round(v[(3 * len(v)) // 4], 2)]
    out.update(agreement(torch, gym_amd, args, with_torch))
    print(json.dumps(out), flush=True)


def child_trace(M, A, N, passes, warmup):
    import torch

    import gym_amd

    args = inputs(torch, M, A, N)
    row_loss = torch.empty(M, device=args[0].device)
    for _ in range(warmup + passes):
        args[0].grad = None
        fused_pass(gym_amd, row_loss, *args)
    torch.cuda.synchronize()
    print(json.dumps({"child": True}), flush=True)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else float("nan")


def run_child(extra, trace_dir=None):
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S)]
    if trace_dir:
        cmd += ["rocprofv3", "--kernel-trace", "-d", trace_dir, "-o", "trace", "--output-format", "csv", "--"]
    cmd += [sys.executable, os.path.abspath(__file__)] + extra
    p = subprocess.run(cmd, check=True, capture_output=True, text=True)      # a failed child ends the benchmark
    for line in p.stdout.splitlines():
        if line.startswith('{"child"'):
            return json.loads(line)
    raise RuntimeError("the child printed no result line: " + p.stdout[-500:] + p.stderr[-500:])


def traced(M, A, N, passes, warmup, launches):
    d = tempfile.mkdtemp(prefix="qr_loss_bench_")
    try:
        run_child(["--passes", str(passes), "--warmup", str(warmup), "--child-trace", str(M), str(A), str(N)], trace_dir=d)
        trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not trace:
            raise RuntimeError(f"rocprofv3 wrote no kernel trace under {d}")
        ks = []
        with open(trace[0]) as f:
            for rec in csv.DictReader(f):
                name = rec.get("Kernel_Name", "")
                if any(w in name for w in ("qr_rows", "qr_leaf", "qr_tree", "qr_bwd")):
                    ks.append((int(rec["Start_Timestamp"]), int(rec["End_Timestamp"]), name))
        ks.sort()
        per = launches + 1
        assert len(ks) == per * (warmup + passes), (len(ks), per, warmup + passes)
        parts = {"rows_us": [], "sum_us": [], "bwd_us": []}
        for i in range(warmup, warmup + passes):
            seg = ks[i * per:(i + 1) * per]
            assert "qr_rows" in seg[0][2] and "qr_leaf" in seg[1][2] and "qr_bwd" in seg[-1][2], [k[2] for k in seg]
            us = lambda s: sum(e - b for b, e, _ in s) / 1e3
            parts["rows_us"].append(us(seg[:1]))
            parts["sum_us"].append(us(seg[1:launches]))
            parts["bwd_us"].append(us(seg[launches:]))
        return {k: _median(v) for k, v in parts.items()}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=10, help="passes in a timed window (and traced passes with --trace)")
    ap.add_argument("--reps", type=int, default=15, help="timed windows of each kind")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="kernel times of the fused path from rocprofv3 --kernel-trace instead of end-to-end times")
    ap.add_argument("--torch-limit-gib", type=float, default=48.0, help="the torch side is not run where its [M, N, N] tensors would need more")
    ap.add_argument("--shape", nargs=3, type=int, action="append", help="rows A N (default: 256, 2048, 32768 and 2^20 rows x (2, 51), (6, 32), (18, 64))")
    ap.add_argument("--child-events", nargs=4, help=argparse.SUPPRESS)
    ap.add_argument("--child-trace", nargs=3, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_events:
        M, A, N, with_torch = (int(x) for x in a.child_events)
        child_events(M, A, N, a.passes, a.reps, a.warmup, bool(with_torch))
        return
    if a.child_trace:
        child_trace(*(int(x) for x in a.child_trace), a.passes, a.warmup)
        return
    from gym_amd.qr import launches

    for M, A, N in (a.shape or SHAPES):
        row = {"rows": M, "A": A, "N": N}
        if a.trace:
            r = traced(M, A, N, a.passes, a.warmup, launches(M))
            three = r["rows_us"] + r["sum_us"] + r["bwd_us"]
            gbs = M * bytes_per_row(A, N) / three / 1e3
            row.update({k: round(v, 2) for k, v in r.items()})
            row.update({"kernels_us": round(three, 2), "launches": launches(M) + 1, "algorithmic_bytes_per_row": bytes_per_row(A, N),
                        "achieved_gbs": round(gbs, 1), "hbm_frac": round(gbs / HBM_PEAK_GBS, 4), "fp64_gops": round(M * ops_per_row(A, N) / three / 1e3, 1),
                        "source": "rocprofv3 kernel-trace (median)"})
        else:
            fits = torch_fits(M, N, a.torch_limit_gib)
            r = run_child(["--passes", str(a.passes), "--reps", str(a.reps), "--warmup", str(a.warmup), "--child-events", str(M), str(A), str(N), str(int(fits))])
            row.update({k: v for k, v in r.items() if k != "child"})
            if fits:
                row.update({"speedup_fwd_vs_torch": round(r["torch_fwd_us"] / r["fwd_us"], 2),
                            "speedup_fwd_bwd_vs_torch": round(r["torch_fwd_bwd_us"] / r["fwd_bwd_us"], 2)})
            else:
                row["torch"] = f"not run: about {TORCH_LIVE_TENSORS} [M, N, N] float32 tensors = {TORCH_LIVE_TENSORS * M * N * N * 4 / (1 << 30):.0f} GiB"
            row["source"] = f"device events, {a.passes} passes a window, median of {a.reps} windows, the kinds alternating"
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
