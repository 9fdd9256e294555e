#!/usr/bin/env python3
"""Stored actions re-evaluated under the current head, forwards and backwards: the two launches behind
gym_amd.evaluate_categorical / gym_amd.evaluate_gaussian next to the torch sequence with autograd they replace — log_softmax, gather,
exp, mul, sum for a categorical head; exp, the Normal.log_prob arithmetic and its sum, the entropy sum for a Gaussian one; and in both
cases whatever kernels autograd launches going backwards.  One pass is: outputs from a leaf that requires grad, then
torch.autograd.backward([log_prob, entropy], [g_lp, g_en]) with given incoming gradients, so that every kernel of a pass belongs to the
evaluation and its backward.  Timed with `rocprofv3 --kernel-trace`, one child process per shape; times are medians over --iters passes
of the kernels' trace durations:
  * `fwd_us`, `bwd_us`      the eval_*_fwd and eval_*_bwd launches;
  * `kernels_us`, `span_us`, `launches`                   every kernel of one pass of ours: durations summed, first start to last end, count;
  * `torch_kernels_us`, `torch_span_us`, `torch_launches` the same for one pass of the torch sequence.
`achieved_gbs` is the two kernels' algorithmic bytes over fwd_us + bwd_us; `fp64_gops` counts the rules' float64 operations per row
(a division counted as one).

    python benchmarks/policy_eval.py [--iters 20] [--warmup 3]     # one JSON line per (head, M, width)
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
ROWS = (4096, 1 << 18, 1 << 20)
SHAPES = [("categorical", M, A) for M in ROWS for A in (2, 6)] + [("gaussian", M, D) for M in ROWS for D in (1, 4)]
HBM_PEAK_GBS = 8000.0
# float64 operations per row, forwards + backwards (straight-line instantiations: EXP once per logit in each pass)
CAT_OPS = lambda A: (45 * A + 40) + (53 * A + 42)
GAUSS_OPS = lambda D: 45 * D + 43 * D
CAT_BYTES = lambda A: (4 * A + 8 + 8) + (4 * A + 8 + 8 + 4 * A)              # int64 actions
GAUSS_BYTES = lambda D: (12 * D + 8) + (12 * D + 8 + 8 * D)


def torch_categorical(torch, logits, actions):
    lsm = torch.log_softmax(logits, dim=-1)
    log_prob = lsm.gather(-1, actions.unsqueeze(-1)).squeeze(-1)
    entropy = -(lsm.exp() * lsm).sum(dim=-1)
    return log_prob, entropy


def torch_gaussian(torch, mean, log_std, actions):
    zq = (actions - mean) / log_std.exp()
    log_prob = (-0.5 * zq * zq - log_std - 0.5 * math.log(2.0 * math.pi)).sum(dim=-1)
    entropy = (log_std + (0.5 + 0.5 * math.log(2.0 * math.pi))).sum(dim=-1)
    return log_prob, entropy


def child(head, M, W, iters, warmup):
    import torch

    import gym_amd

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    g_lp, g_en = torch.randn(M, device=dev, generator=g), torch.randn(M, device=dev, generator=g)
    if head == "categorical":
        leaves = [torch.randn((M, W), device=dev, generator=g).requires_grad_()]
        actions = torch.randint(0, W, (M,), device=dev, generator=g)
        ours = lambda: gym_amd.evaluate_categorical(leaves[0], actions)
        theirs = lambda: torch_categorical(torch, leaves[0], actions)
        ref = lambda xs: torch_categorical(torch, xs[0], actions)
    else:
        leaves = [torch.randn((M, W), device=dev, generator=g).requires_grad_(),
                  (torch.rand((M, W), device=dev, generator=g) * 2.0 - 1.5).requires_grad_()]
        actions = (leaves[0] + leaves[1].exp() * torch.randn((M, W), device=dev, generator=g)).detach()
        ours = lambda: gym_amd.evaluate_gaussian(leaves[0], leaves[1], actions)
        theirs = lambda: torch_gaussian(torch, leaves[0], leaves[1], actions)
        ref = lambda xs: torch_gaussian(torch, xs[0], xs[1], actions.double())
    one = torch.zeros((1, 2), device=dev)
    mark_out = (torch.empty(1, dtype=torch.int64, device=dev), None, None)

    def mark():     # a one-row launch of the categorical sampler: the delimiter between passes in the trace
        gym_amd.sample_categorical(one, seed=0, step=0, out=mark_out)

    def one_pass(f):
        for x in leaves:
            x.grad = None
        lp, en = f()
        torch.autograd.backward([lp, en], [g_lp, g_en])

    mark()
    for f in (ours, theirs):
        for _ in range(warmup + iters):
            one_pass(f)
            mark()
    torch.cuda.synchronize()
    # the two agree as far as float32 arithmetic does: gradients against torch's float64 autograd
    one_pass(ours)
    got = [x.grad.double() for x in leaves]
    xs = [x.detach().double().requires_grad_() for x in leaves]
    lp, en = ref(xs)
    torch.autograd.backward([lp, en], [g_lp.double(), g_en.double()])
    err = max(float((a - b.grad).abs().max()) for a, b in zip(got, xs))
    print(json.dumps({"child": True, "head": head, "M": M, "W": W, "max_abs_diff_grad_vs_torch_f64": err}), flush=True)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else float("nan")


def profile(head, M, W, iters, warmup):
    d = tempfile.mkdtemp(prefix="policy_eval_bench_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "-d", d, "-o", "trace", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--iters", str(iters), "--warmup", str(warmup), "--child", head, str(M), str(W)]
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
    """-> dict of medians from the ordered trace of child(): marks delimit 2 (warmup + iters) passes, ours first."""
    n = warmup + iters
    marks = [i for i, k in enumerate(ks) if "policy_kernel" in k[2]]
    assert len(marks) >= 2 * n + 1, (len(marks), n)
    segs = [ks[a + 1:b] for a, b in zip(marks[:2 * n], marks[1:2 * n + 1])]
    us = lambda seg: sum(e - s for s, e, _ in seg) / 1e3
    span = lambda seg: (max(e for _, e, _ in seg) - seg[0][0]) / 1e3
    mine, torchs = segs[warmup:n], segs[n + warmup:2 * n]
    for seg in mine:
        assert sum("eval_" in k[2] and "_fwd" in k[2] for k in seg) == 1 and sum("eval_" in k[2] and "_bwd" in k[2] for k in seg) == 1, [k[2] for k in seg]
    assert not any("eval_" in k[2] for seg in torchs for k in seg)
    return {"fwd_us": _median([us([k for k in seg if "_fwd" in k[2] and "eval_" in k[2]]) for seg in mine]),
            "bwd_us": _median([us([k for k in seg if "_bwd" in k[2] and "eval_" in k[2]]) for seg in mine]),
            "kernels_us": _median([us(seg) for seg in mine]), "span_us": _median([span(seg) for seg in mine]), "launches": len(mine[0]),
            "torch_kernels_us": _median([us(seg) for seg in torchs]), "torch_span_us": _median([span(seg) for seg in torchs]),
            "torch_launches": len(torchs[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", nargs=3, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), int(a.child[2]), a.iters, a.warmup)
        return
    for head, M, W in SHAPES:
        ks, info = profile(head, M, W, a.iters, a.warmup)
        r = analyse(ks, a.iters, a.warmup)
        both = r["fwd_us"] + r["bwd_us"]
        per_row = (CAT_BYTES if head == "categorical" else GAUSS_BYTES)(W)
        ops = (CAT_OPS if head == "categorical" else GAUSS_OPS)(W)
        gbs = M * per_row / both / 1e3
        row = {"head": head, "M": M, "A" if head == "categorical" else "D": W}
        row.update({k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items()})
        row.update({"speedup_kernels_vs_torch_kernels": round(r["torch_kernels_us"] / r["kernels_us"], 2),
                    "speedup_span_vs_torch_span": round(r["torch_span_us"] / r["span_us"], 2),
                    "algorithmic_bytes_per_row": per_row, "achieved_gbs": round(gbs, 1), "roofline_frac": round(gbs / HBM_PEAK_GBS, 4),
                    "fp64_gops": round(M * ops / both / 1e3, 1),
                    "max_abs_diff_grad_vs_torch_f64": info.get("max_abs_diff_grad_vs_torch_f64"), "source": "rocprofv3 kernel-trace (median)"})
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
