#!/usr/bin/env python3
"""Reparameterised tanh-squashed Gaussian draws: gym_amd.rsample_squashed_gaussian forwards plus its backward — two
launches — next to the torch sequence it replaces, on the same card in the same process: log_std.exp(), randn_like, mul, add, tanh, the
affine map, the Normal.log_prob arithmetic, softplus for log(1 - tanh^2), the sums over the action dims, and the backward of that graph.

One pass of either side is the forward and `torch.autograd.backward((actions, log_prob), (grad_actions, grad_log_prob))`: the incoming
gradients are given, so neither side pays for a loss in front.  Method: every shape is warmed up on both sides; a repetition is `--inner`
passes between two device events; the two sides alternate, repetition by repetition, so that a drift of the clocks or of a neighbour's
load falls on both; the figure is the median over `--reps` repetitions of the time per pass, with the smallest and the largest beside
it.  `launches` counts the kernels of one pass with torch's profiler (in a pass of its own, outside the timed ones).

The yardstick is the torch sequence: `not_slower` says whether the fused pair's median is at most torch's.  The exit status is 1 if it
is slower at any point.

    python -m benchmarks.squashed [--reps 30] [--inner 20] [--warmup 5] [--out FILE]     # one JSON line per (N, D)
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
SHAPES = [(4096, 1), (4096, 4), (65536, 1), (65536, 4), (1 << 20, 1), (1 << 20, 4)]
LOW, HIGH = -2.0, 2.0


def torch_pass(torch, mean, log_std, scale, bias, ga, glp):
    """The textbook sequence: what a SAC actor written in torch runs for one reparameterised draw and its backward."""
    std = log_std.exp()
    eps = torch.randn_like(mean)
    u = mean + std * eps
    actions = bias + scale * torch.tanh(u)
    log_prob = torch.distributions.Normal(mean, std).log_prob(u).sum(dim=-1)
    log_prob = log_prob - (2.0 * (math.log(2.0) - u - torch.nn.functional.softplus(-2.0 * u))).sum(dim=-1) - math.log(scale) * mean.shape[-1]
    torch.autograd.backward((actions, log_prob), (ga, glp))
    return actions, log_prob


def fused_pass(torch, gym_amd, mean, log_std, step, ga, glp):
    actions, log_prob = gym_amd.rsample_squashed_gaussian(mean, log_std, seed=1, step=step, low=LOW, high=HIGH)
    torch.autograd.backward((actions, log_prob), (ga, glp))
    return actions, log_prob


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _launches(torch, fn):
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower())


def measure(N, D, reps, inner, warmup):
    import torch

    import gym_amd

    if not torch.cuda.is_available():
        raise RuntimeError("benchmarks.squashed needs a HIP device: a timing taken without one says nothing")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    mean = torch.randn((N, D), device=dev, generator=g).requires_grad_()
    log_std = (torch.rand((N, D), device=dev, generator=g) * 2.0 - 1.5).requires_grad_()
    ga = torch.randn((N, D), device=dev, generator=g)
    glp = torch.randn(N, device=dev, generator=g)
    scale, bias = (HIGH - LOW) / 2, (HIGH + LOW) / 2
    step = [0]

    def ours():
        mean.grad = log_std.grad = None
        fused_pass(torch, gym_amd, mean, log_std, step[0], ga, glp)
        step[0] += 1

    def theirs():
        mean.grad = log_std.grad = None
        torch_pass(torch, mean, log_std, scale, bias, ga, glp)

    for _ in range(warmup):
        ours()
        theirs()
    torch.cuda.synchronize()
    times = {"fused": [], "torch": []}
    for _ in range(reps):
        for name, fn in (("fused", ours), ("torch", theirs)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / inner)      # us per pass
    try:
        launches = {"fused": _launches(torch, ours), "torch": _launches(torch, theirs)}
    except Exception as e:      # the count is an annotation; the timing does not depend on the profiler
        launches = {"fused": None, "torch": None, "error": repr(e)[:200]}
    # the two compute the same thing: on the fused draw's own noise the textbook formula in float64 gives its log_prob and gradients
    mean.grad = log_std.grad = None
    act, lp = fused_pass(torch, gym_amd, mean, log_std, 7, ga, glp)
    gm, gs = mean.grad.clone(), log_std.grad.clone()
    m64, s64 = mean.detach().double().requires_grad_(), log_std.detach().double().requires_grad_()
    y = ((act.detach().double() - bias) / scale).clamp(-1 + 1e-15, 1 - 1e-15)
    z = ((torch.atanh(y) - m64.detach()) / s64.detach().exp())      # the noise, recovered where the action is not saturated
    ok = (y.abs() < 0.99).all(dim=-1)
    u = m64 + s64.exp() * z
    a64 = bias + scale * torch.tanh(u)
    lp64 = (torch.distributions.Normal(m64, s64.exp()).log_prob(u) - 2.0 * (math.log(2.0) - u - torch.nn.functional.softplus(-2.0 * u))
            - math.log(scale)).sum(-1)
    torch.autograd.backward((a64[ok], lp64[ok]), (ga.double()[ok], glp.double()[ok]))
    return {"N": N, "D": D, "fused_us": round(_median(times["fused"]), 2), "fused_min_us": round(min(times["fused"]), 2),
            "fused_max_us": round(max(times["fused"]), 2), "torch_us": round(_median(times["torch"]), 2),
            "torch_min_us": round(min(times["torch"]), 2), "torch_max_us": round(max(times["torch"]), 2),
            "torch_over_fused": round(_median(times["torch"]) / _median(times["fused"]), 2),
            "not_slower": _median(times["fused"]) <= _median(times["torch"]), "fused_launches": launches["fused"],
            "torch_launches": launches["torch"], "reps": reps, "inner": inner,
            "max_abs_diff_log_prob_vs_torch_f64": float((lp.detach().double() - lp64.detach())[ok].abs().max()),
            "max_abs_diff_grad_mean_vs_torch_f64": float((gm.double() - m64.grad)[ok].abs().max()),
            "max_abs_diff_grad_log_std_vs_torch_f64": float((gs.double() - s64.grad)[ok].abs().max()),
            "rows_compared": int(ok.sum()), "source": "device events around `inner` passes, median of `reps`, sides alternating"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", help="also append the JSON lines to this file")
    a = ap.parse_args()
    slower = []
    for N, D in SHAPES:
        row = measure(N, D, a.reps, a.inner, a.warmup)
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
        if not row["not_slower"]:
            slower.append((N, D))
    if slower:
        print(f"the fused pair is slower than the torch sequence at {slower}", flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
