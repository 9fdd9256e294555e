#!/usr/bin/env python3
"""The last stage of a PPO update, fused: gym_amd.advantage_moments + gym_amd.ppo_clip_loss + loss.backward() + one read
of the diagnostics vector, next to the torch sequence of examples/ppo_clip.py that they replace — the advantage normalisation, exp,
clamp, two products, minimum, three means, the scalar arithmetic, loss.backward() and the five float(...) reads of the diagnostics.
One pass is one of each on the same inputs (log_prob, entropy and values are leaves that require grad), so that every kernel of a pass
belongs to the stage.  Timed with `rocprofv3 --kernel-trace`, one child process per shape (no counters: they are never combined with
tracing); times are medians over --iters passes of the kernels' trace durations:
  * `moments_us`, `fwd_us`, `bwd_us`                        the moments_leaf / ppo_leaf launches with their ppo_tree levels, and ppo_bwd;
  * `kernels_us`, `span_us`, `launches`                     every kernel of one pass of ours: durations summed, first start to last end, count;
  * `torch_kernels_us`, `torch_span_us`, `torch_launches`   the same for one pass of the torch sequence.
`achieved_gbs` is the algorithmic bytes of the three calls (4 + 24 + 36 bytes a row) over moments_us + fwd_us + bwd_us; `fp64_gops`
counts the rule's float64 operations per row (EXP as its 35, a division as one).

    python benchmarks/ppo_loss.py [--iters 20] [--warmup 3]     # one JSON line per shape
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
SHAPES = ((64, 4096), (32, 1 << 20))
HBM_PEAK_GBS = 8000.0
BYTES_PER_ROW = 4 + 24 + (24 + 12)        # moments: adv; forward: six inputs; backward: six inputs and three gradients
OPS_PER_ROW = 3 + (2 + 35 + 20 + 8) + (2 + 35 + 12)
CLIP, VALUE_COEF, ENTROPY_COEF = 0.2, 0.5, 0.01


def torch_pass(torch, log_prob, old_log_prob, adv, entropy, value, ret):
    """examples/ppo_clip.py, lines 83-99, without the optimizer."""
    clip, value_coef, entropy_coef = CLIP, VALUE_COEF, ENTROPY_COEF
    with torch.no_grad():
        norm = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = (log_prob - old_log_prob).exp()
    surrogate = torch.minimum(ratio * norm, ratio.clamp(1.0 - clip, 1.0 + clip) * norm)
    err = value - ret
    loss = -surrogate.mean() + value_coef * 0.5 * (err * err).mean() - entropy_coef * entropy.mean()
    loss.backward()
    with torch.no_grad():
        return {"loss": float(loss), "ratio_min": float(ratio.min()), "ratio_max": float(ratio.max()),
                "approx_kl": float((old_log_prob - log_prob).mean()), "clipped": float(((ratio - 1.0).abs() > clip).float().mean())}


def fused_pass(gym_amd, log_prob, old_log_prob, adv, entropy, value, ret):
    moments = gym_amd.advantage_moments(adv)
    loss, stats = gym_amd.ppo_clip_loss(log_prob, old_log_prob, adv, clip=CLIP, moments=moments, entropy=entropy, entropy_coef=ENTROPY_COEF,
                                        values=value, returns=ret, value_coef=VALUE_COEF)
    loss.backward()
    return loss, stats.tolist()


def child(K, N, iters, warmup):
    import torch

    import gym_amd

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    rand = lambda: torch.randn((K, N), device=dev, generator=g)
    old_log_prob = -rand().abs() - 0.1
    log_prob = (old_log_prob + 0.1 * rand()).requires_grad_()
    adv, ret = rand() * 2.0 + 0.3, rand()
    entropy = (torch.rand((K, N), device=dev, generator=g) * 0.6 + 0.1).requires_grad_()
    value = (ret + 0.5 * rand()).requires_grad_()
    leaves = (log_prob, entropy, value)
    args = (log_prob, old_log_prob, adv, entropy, value, ret)
    one = torch.zeros((1, 2), device=dev)
    mark_out = (torch.empty(1, dtype=torch.int64, device=dev), None, None)

    def mark():     # a one-row launch of the categorical sampler: the delimiter between passes in the trace
        gym_amd.sample_categorical(one, seed=0, step=0, out=mark_out)

    def one_pass(f):
        for x in leaves:
            x.grad = None
        return f()

    mark()
    for f in (lambda: fused_pass(gym_amd, *args), lambda: torch_pass(torch, *args)):
        for _ in range(warmup + iters):
            one_pass(f)
            mark()
    torch.cuda.synchronize()
    # the two agree as far as float32 arithmetic does: loss and gradients against the torch sequence in float64
    loss, stats = one_pass(lambda: fused_pass(gym_amd, *args))
    got = [x.grad.double() for x in leaves]
    xs = [x.detach().double().requires_grad_() for x in leaves]
    ref = torch_pass(torch, xs[0], old_log_prob.double(), adv.double(), xs[1], xs[2], ret.double())
    err = max(float((a - b.grad).abs().max()) for a, b in zip(got, xs))
    print(json.dumps({"child": True, "K": K, "N": N, "loss": float(loss), "loss_torch_f64": ref["loss"], "clip_fraction": stats[5],
                      "clip_fraction_torch_f64": ref["clipped"], "max_abs_diff_grad_vs_torch_f64": err}), flush=True)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else float("nan")


def profile(K, N, iters, warmup):
    d = tempfile.mkdtemp(prefix="ppo_loss_bench_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "-d", d, "-o", "trace", "--output-format", "csv", "--",
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


def analyse(ks, iters, warmup, launches):
    """-> dict of medians from the ordered trace of child(): marks delimit 2 (warmup + iters) passes, ours first.  `launches`: kernels of
    one forward of ours (and of the moments) at this size."""
    n = warmup + iters
    marks = [i for i, k in enumerate(ks) if "policy_kernel" in k[2]]
    assert len(marks) >= 2 * n + 1, (len(marks), n)
    segs = [ks[a + 1:b] for a, b in zip(marks[:2 * n], marks[1:2 * n + 1])]
    us = lambda seg: sum(e - s for s, e, _ in seg) / 1e3
    span = lambda seg: (max(e for _, e, _ in seg) - seg[0][0]) / 1e3
    mine, torchs = segs[warmup:n], segs[n + warmup:2 * n]
    ours = lambda k: any(w in k[2] for w in ("ppo_leaf", "moments_leaf", "ppo_tree", "ppo_bwd"))
    parts = {"moments_us": [], "fwd_us": [], "bwd_us": []}
    for seg in mine:
        names = [k[2] for k in seg if ours(k)]
        assert len(names) == 2 * launches + 1 and "moments_leaf" in names[0] and "ppo_leaf" in names[launches] and "ppo_bwd" in names[-1], names
        mk = [k for k in seg if ours(k)]
        parts["moments_us"].append(us(mk[:launches]))
        parts["fwd_us"].append(us(mk[launches:2 * launches]))
        parts["bwd_us"].append(us(mk[2 * launches:]))
    assert not any(ours(k) for seg in torchs for k in seg)
    out = {k: _median(v) for k, v in parts.items()}
    out.update({"kernels_us": _median([us(seg) for seg in mine]), "span_us": _median([span(seg) for seg in mine]), "launches": len(mine[0]),
                "torch_kernels_us": _median([us(seg) for seg in torchs]), "torch_span_us": _median([span(seg) for seg in torchs]),
                "torch_launches": len(torchs[0])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", nargs=2, type=int, action="append", help="K N (default: 64 4096 and 32 1048576)")
    ap.add_argument("--child", nargs=2, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), int(a.child[1]), a.iters, a.warmup)
        return
    from gym_amd.ppo import launches

    for K, N in (a.shape or SHAPES):
        M = K * N
        ks, info = profile(K, N, a.iters, a.warmup)
        r = analyse(ks, a.iters, a.warmup, launches(M))
        three = r["moments_us"] + r["fwd_us"] + r["bwd_us"]
        gbs = M * BYTES_PER_ROW / three / 1e3
        row = {"K": K, "N": N, "rows": M}
        row.update({k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items()})
        row.update({"speedup_kernels_vs_torch_kernels": round(r["torch_kernels_us"] / r["kernels_us"], 2),
                    "speedup_span_vs_torch_span": round(r["torch_span_us"] / r["span_us"], 2),
                    "algorithmic_bytes_per_row": BYTES_PER_ROW, "achieved_gbs": round(gbs, 1), "roofline_frac": round(gbs / HBM_PEAK_GBS, 4),
                    "fp64_gops": round(M * OPS_PER_ROW / three / 1e3, 1), "source": "rocprofv3 kernel-trace (median)"})
        row.update({k: v for k, v in info.items() if k not in ("child", "K", "N")})
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
