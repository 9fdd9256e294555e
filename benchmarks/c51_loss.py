#!/usr/bin/env python3
"""The categorical (C51) value-based update, fused: gym_amd.categorical_dqn_loss in the bootstrap mode with
next_logits_online (double DQN), weights and row_loss, loss.backward() and one read of the diagnostics vector, next to the literal torch
sequence they replace — two softmaxes, the expectation, argmax, gather, the Bellman shift, clamp, floor / ceil with the l == u repair, two
index_add_, log_softmax, the product and its reductions, loss.backward() and the float(...) reads of the same diagnostics.  One pass is
one of each on the same inputs (logits is a leaf that requires grad), so that every kernel of a pass belongs to the update.  Timed with
`rocprofv3 --kernel-trace`, one child process per shape under `timeout -k 10`, stopping at the first child that fails (no counters:
they are never combined with tracing; the program goes after `--`); times are medians over --iters passes of the kernels' trace
durations:
  * `rows_us`, `sum_us`, `bwd_us`                           c51_rows, c51_leaf with its c51_tree levels, and c51_bwd;
  * `kernels_us`, `span_us`, `launches`                     every kernel of one pass of ours: durations summed, first start to last end, count;
  * `torch_kernels_us`, `torch_span_us`, `torch_launches`   the same for one pass of the torch sequence.
`achieved_gbs` is the algorithmic bytes of the two calls over rows_us + sum_us + bwd_us; `fp64_gops` counts the rule's float64
operations by the model of `ops_per_row` (a count of the rule's lines, not of instructions).

    python benchmarks/c51_loss.py [--iters 20] [--warmup 3]     # one JSON line per shape
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
SHAPES = tuple((M, A, 51) for M in (256, 4096, 1 << 18) for A in (2, 6))
HBM_PEAK_GBS = 8000.0
GAMMA, V_MIN, V_MAX = 0.99, -10.0, 10.0
CHILD_TIMEOUT_S = 600


def bytes_per_row(A, Z):
    """forward: the taken row 4 Z, action 8, reward 4, terminated 1, weight 4, the selecting head 4 A Z, next_logits[i, j*] 4 Z, six
    float64 columns written and read again, row_loss 4; backward: the same reads, and the gradient row 4 A Z."""
    reads = 8 * Z + 17 + 4 * A * Z
    return (reads + 2 * 48 + 4) + (reads + 4 * A * Z)


def ops_per_row(A, Z):
    """float64 operations of the rule per row, both calls: a SOFT is about 45 per atom (EXP 32, the quotient, the three butterflies); the
    forward has A + 2 of them, the projection 6 per (j, k) pair, the loss terms about 40 per atom; the backward recomputes all of it."""
    return 2 * ((A + 2) * 45 * Z + 6 * Z * Z + 40 * Z)


def torch_pass(torch, logits, actions, reward, terminated, next_logits, next_online, weights):
    """The literal torch sequence of a categorical double-DQN update, without the optimizer."""
    M, A, Z = logits.shape
    rows = torch.arange(M, device=logits.device)
    dz = (V_MAX - V_MIN) / (Z - 1)
    z = V_MIN + torch.arange(Z, device=logits.device, dtype=logits.dtype) * dz
    with torch.no_grad():
        q_next = (torch.softmax(next_online, -1) * z).sum(-1)
        pn = torch.softmax(next_logits, -1)[rows, q_next.argmax(1)]
        tz_raw = reward[:, None] + (1 - terminated.to(logits.dtype))[:, None] * GAMMA * z[None, :]
        pos = (tz_raw.clamp(V_MIN, V_MAX) - V_MIN) / dz
        lo, up = pos.floor().long(), pos.ceil().long()
        lo[(up > 0) & (lo == up)] -= 1
        up[(lo < Z - 1) & (lo == up)] += 1
        m = torch.zeros(M * Z, device=logits.device, dtype=logits.dtype)
        offset = (rows * Z)[:, None]
        m.index_add_(0, (lo + offset).view(-1), (pn * (up.to(logits.dtype) - pos)).view(-1))
        m.index_add_(0, (up + offset).view(-1), (pn * (pos - lo.to(logits.dtype))).view(-1))
        m = m.view(M, Z)
        clipped = (pn * ((tz_raw < V_MIN) | (tz_raw > V_MAX)).to(logits.dtype)).sum(-1)
    taken = logits[rows, actions]
    lp = torch.log_softmax(taken, -1)
    ce = -(m * lp).sum(-1)
    loss = (ce * weights).mean()
    loss.backward()
    with torch.no_grad():
        p = lp.exp()
        qa = (p * z).sum(-1)
        return {"loss": float(loss), "q_taken_mean": float(qa.mean()), "target_mean": float((m * z).sum(-1).mean()),
                "entropy_mean": float(-(p * lp).sum(-1).mean()), "clipped_mass_mean": float(clipped.mean()), "row_loss_max": float(ce.max()),
                "q_taken_min": float(qa.min()), "q_taken_max": float(qa.max())}


def fused_pass(gym_amd, row_loss, logits, actions, reward, terminated, next_logits, next_online, weights):
    loss, stats = gym_amd.categorical_dqn_loss(logits, actions, v_min=V_MIN, v_max=V_MAX, reward=reward, terminated=terminated,
                                               next_logits=next_logits, next_logits_online=next_online, gamma=GAMMA, weights=weights,
                                               row_loss=row_loss)
    loss.backward()
    return loss, stats.tolist()


def child(M, A, Z, iters, warmup):
    import torch

    import gym_amd

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    logits = (torch.randn((M, A, Z), device=dev, generator=g) * 2.0).requires_grad_()
    next_logits = torch.randn((M, A, Z), device=dev, generator=g) * 2.0
    next_online = next_logits + 0.7 * torch.randn((M, A, Z), device=dev, generator=g)
    actions = torch.randint(0, A, (M,), device=dev, generator=g)
    reward = torch.randn(M, device=dev, generator=g)
    terminated = torch.rand(M, device=dev, generator=g) < 0.1
    weights = torch.rand(M, device=dev, generator=g) * 1.8 + 0.2
    row_loss = torch.empty(M, device=dev)
    args = (logits, actions, reward, terminated, next_logits, next_online, weights)
    one = torch.zeros((1, 2), device=dev)
    mark_out = (torch.empty(1, dtype=torch.int64, device=dev), None, None)

    def mark():     # a one-row launch of the categorical sampler: the delimiter between passes in the trace
        gym_amd.sample_categorical(one, seed=0, step=0, out=mark_out)

    def one_pass(f):
        logits.grad = None
        return f()

    mark()
    for f in (lambda: fused_pass(gym_amd, row_loss, *args), lambda: torch_pass(torch, *args)):
        for _ in range(warmup + iters):
            one_pass(f)
            mark()
    torch.cuda.synchronize()
    # the two agree as far as float32 arithmetic does: loss and gradient against the torch sequence in float64
    loss, stats = one_pass(lambda: fused_pass(gym_amd, row_loss, *args))
    got = logits.grad.double()
    x64 = logits.detach().double().requires_grad_()
    ref = torch_pass(torch, x64, actions, reward.double(), terminated, next_logits.double(), next_online.double(), weights.double())
    print(json.dumps({"child": True, "rows": M, "A": A, "Z": Z, "loss": float(loss), "loss_torch_f64": ref["loss"], "entropy_mean": stats[3],
                      "entropy_mean_torch_f64": ref["entropy_mean"], "clipped_mass_mean": stats[4], "clipped_mass_mean_torch_f64": ref["clipped_mass_mean"],
                      "max_abs_diff_grad_vs_torch_f64": float((got - x64.grad).abs().max())}), flush=True)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else float("nan")


def profile(M, A, Z, iters, warmup):
    d = tempfile.mkdtemp(prefix="c51_loss_bench_")
    try:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), "rocprofv3", "--kernel-trace", "-d", d, "-o", "trace", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--iters", str(iters), "--warmup", str(warmup), "--child", str(M), str(A), str(Z)]
        p = subprocess.run(cmd, check=True, capture_output=True, text=True)      # a failed child ends the benchmark
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
    one forward of ours at this size."""
    n = warmup + iters
    marks = [i for i, k in enumerate(ks) if "policy_kernel" in k[2]]
    assert len(marks) >= 2 * n + 1, (len(marks), n)
    segs = [ks[a + 1:b] for a, b in zip(marks[:2 * n], marks[1:2 * n + 1])]
    us = lambda seg: sum(e - s for s, e, _ in seg) / 1e3
    span = lambda seg: (max(e for _, e, _ in seg) - seg[0][0]) / 1e3
    mine, torchs = segs[warmup:n], segs[n + warmup:2 * n]
    ours = lambda k: any(w in k[2] for w in ("c51_rows", "c51_leaf", "c51_tree", "c51_bwd"))
    parts = {"rows_us": [], "sum_us": [], "bwd_us": []}
    for seg in mine:
        mk = [k for k in seg if ours(k)]
        names = [k[2] for k in mk]
        assert len(names) == launches + 1 and "c51_rows" in names[0] and "c51_leaf" in names[1] and all("c51_tree" in x for x in names[2:launches]) \
            and "c51_bwd" in names[-1], names
        parts["rows_us"].append(us(mk[:1]))
        parts["sum_us"].append(us(mk[1:launches]))
        parts["bwd_us"].append(us(mk[launches:]))
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
    ap.add_argument("--shape", nargs=3, type=int, action="append", help="rows A Z (default: 256, 4096 and 262144 rows, A = 2 and 6, Z = 51)")
    ap.add_argument("--child", nargs=3, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), int(a.child[1]), int(a.child[2]), a.iters, a.warmup)
        return
    from gym_amd.c51 import launches

    for M, A, Z in (a.shape or SHAPES):
        ks, info = profile(M, A, Z, a.iters, a.warmup)
        r = analyse(ks, a.iters, a.warmup, launches(M))
        three = r["rows_us"] + r["sum_us"] + r["bwd_us"]
        gbs = M * bytes_per_row(A, Z) / three / 1e3
        row = {"rows": M, "A": A, "Z": Z}
        row.update({k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items()})
        row.update({"speedup_kernels_vs_torch_kernels": round(r["torch_kernels_us"] / r["kernels_us"], 2),
                    "speedup_span_vs_torch_span": round(r["torch_span_us"] / r["span_us"], 2),
                    "algorithmic_bytes_per_row": bytes_per_row(A, Z), "achieved_gbs": round(gbs, 1), "roofline_frac": round(gbs / HBM_PEAK_GBS, 4),
                    "fp64_gops": round(M * ops_per_row(A, Z) / three / 1e3, 1), "source": "rocprofv3 kernel-trace (median)"})
        row.update({k: v for k, v in info.items() if k not in ("child", "rows", "A", "Z")})
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
