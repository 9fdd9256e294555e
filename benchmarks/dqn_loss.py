#!/usr/bin/env python3
"""The value-based update, fused: gym_amd.dqn_loss in the bootstrap mode with next_q_online (double DQN) and td_error,
loss.backward() and one read of the diagnostics vector, next to the torch sequence they replace — gather, argmax, gather, the target
arithmetic, huber_loss, mean, loss.backward() and the float(...) reads of the loss, mean |TD|, mean Q, max Q and the fraction in the
linear zone.  One pass is one of each on the same inputs (q is a leaf that requires grad), so that every kernel of a pass belongs to
the update.  Timed with `rocprofv3 --kernel-trace`, one child process per shape under `timeout -k 10` (no counters: they are never
combined with tracing; the program goes after `--`); times are medians over --iters passes of the kernels' trace durations:
  * `leaf_us`, `tree_us`, `bwd_us`                          dqn_leaf, its dqn_tree levels, and dqn_bwd;
  * `kernels_us`, `span_us`, `launches`                     every kernel of one pass of ours: durations summed, first start to last end, count;
  * `torch_kernels_us`, `torch_span_us`, `torch_launches`   the same for one pass of the torch sequence.
`achieved_gbs` is the algorithmic bytes of the two calls (25 + 4 A forwards, 21 + 8 A backwards, a row) over leaf_us + tree_us + bwd_us;
`fp64_gops` counts the rule's float64 operations per row (about 12 forwards with the five additions of the sums, 8 backwards).

    python benchmarks/dqn_loss.py [--iters 20] [--warmup 3]     # one JSON line per shape
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
SHAPES = ((64, 4096, 2), (64, 4096, 6), (32, 1 << 20, 2), (32, 1 << 20, 6))
HBM_PEAK_GBS = 8000.0
OPS_PER_ROW = 12 + 8
GAMMA, DELTA = 0.99, 1.0
CHILD_TIMEOUT_S = 600


def bytes_per_row(A):
    """forward: q[i, a] 4, action 8, reward 4, terminated 1, the selecting row 4 A, next_q[i, j*] 4, td_error 4; backward: the same reads
    without td_error, and the gradient row 4 A."""
    return (25 + 4 * A) + (21 + 8 * A)


def torch_pass(torch, q, actions, reward, terminated, next_q, next_q_online):
    """The literal torch sequence of a double-DQN update, without the optimizer."""
    import torch.nn.functional as F

    with torch.no_grad():
        best = next_q_online.argmax(1, keepdim=True)
        y = reward + (1 - terminated.float()) * GAMMA * next_q.gather(1, best).squeeze(1)
    qa = q.gather(1, actions.unsqueeze(1)).squeeze(1)
    loss = F.huber_loss(qa, y, delta=DELTA, reduction="none").mean()
    loss.backward()
    with torch.no_grad():
        td = (qa - y).abs()
        return {"loss": float(loss), "td_abs_mean": float(td.mean()), "q_mean": float(qa.mean()), "q_max": float(qa.max()),
                "linear_fraction": float((td > DELTA).float().mean())}


def fused_pass(gym_amd, td_error, q, actions, reward, terminated, next_q, next_q_online):
    loss, stats = gym_amd.dqn_loss(q, actions, reward=reward, terminated=terminated, next_q=next_q, next_q_online=next_q_online, gamma=GAMMA,
                                   delta=DELTA, td_error=td_error)
    loss.backward()
    return loss, stats.tolist()


def child(K, N, A, iters, warmup):
    import torch

    import gym_amd

    dev = torch.device("cuda", 0)
    M = K * N
    g = torch.Generator(device=dev).manual_seed(1)
    q = (torch.randn((M, A), device=dev, generator=g) * 2.0).requires_grad_()
    next_q = torch.randn((M, A), device=dev, generator=g) * 2.0
    next_q_online = next_q + 0.7 * torch.randn((M, A), device=dev, generator=g)
    actions = torch.randint(0, A, (M,), device=dev, generator=g)
    reward = torch.randn(M, device=dev, generator=g)
    terminated = torch.rand(M, device=dev, generator=g) < 0.1
    td_error = torch.empty(M, device=dev)
    args = (q, actions, reward, terminated, next_q, next_q_online)
    one = torch.zeros((1, 2), device=dev)
    mark_out = (torch.empty(1, dtype=torch.int64, device=dev), None, None)

    def mark():     # a one-row launch of the categorical sampler: the delimiter between passes in the trace
        gym_amd.sample_categorical(one, seed=0, step=0, out=mark_out)

    def one_pass(f):
        q.grad = None
        return f()

    mark()
    for f in (lambda: fused_pass(gym_amd, td_error, *args), lambda: torch_pass(torch, *args)):
        for _ in range(warmup + iters):
            one_pass(f)
            mark()
    torch.cuda.synchronize()
    # the two agree as far as float32 arithmetic does: loss and gradient against the torch sequence in float64
    loss, stats = one_pass(lambda: fused_pass(gym_amd, td_error, *args))
    got = q.grad.double()
    q64 = q.detach().double().requires_grad_()
    ref = torch_pass(torch, q64, actions, reward.double(), terminated, next_q.double(), next_q_online.double())
    print(json.dumps({"child": True, "K": K, "N": N, "A": A, "loss": float(loss), "loss_torch_f64": ref["loss"], "linear_fraction": stats[4],
                      "linear_fraction_torch_f64": ref["linear_fraction"], "max_abs_diff_grad_vs_torch_f64": float((got - q64.grad).abs().max())}),
          flush=True)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else float("nan")


def profile(K, N, A, iters, warmup):
    d = tempfile.mkdtemp(prefix="dqn_loss_bench_")
    try:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), "rocprofv3", "--kernel-trace", "-d", d, "-o", "trace", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--iters", str(iters), "--warmup", str(warmup), "--child", str(K), str(N), str(A)]
        p = subprocess.run(cmd, check=True, capture_output=True, text=True)
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
    ours = lambda k: any(w in k[2] for w in ("dqn_leaf", "dqn_tree", "dqn_bwd"))
    parts = {"leaf_us": [], "tree_us": [], "bwd_us": []}
    for seg in mine:
        mk = [k for k in seg if ours(k)]
        names = [k[2] for k in mk]
        assert len(names) == launches + 1 and "dqn_leaf" in names[0] and all("dqn_tree" in x for x in names[1:launches]) and "dqn_bwd" in names[-1], names
        parts["leaf_us"].append(us(mk[:1]))
        parts["tree_us"].append(us(mk[1:launches]))
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
    ap.add_argument("--shape", nargs=3, type=int, action="append", help="K N A (default: 64 x 4096 and 32 x 1048576 rows, A = 2 and 6)")
    ap.add_argument("--child", nargs=3, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), int(a.child[1]), int(a.child[2]), a.iters, a.warmup)
        return
    from gym_amd.dqn import launches

    for K, N, A in (a.shape or SHAPES):
        M = K * N
        ks, info = profile(K, N, A, a.iters, a.warmup)
        r = analyse(ks, a.iters, a.warmup, launches(M))
        three = r["leaf_us"] + r["tree_us"] + r["bwd_us"]
        gbs = M * bytes_per_row(A) / three / 1e3
        row = {"K": K, "N": N, "A": A, "rows": M}
        row.update({k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items()})
        row.update({"speedup_kernels_vs_torch_kernels": round(r["torch_kernels_us"] / r["kernels_us"], 2),
                    "speedup_span_vs_torch_span": round(r["torch_span_us"] / r["span_us"], 2),
                    "algorithmic_bytes_per_row": bytes_per_row(A), "achieved_gbs": round(gbs, 1), "roofline_frac": round(gbs / HBM_PEAK_GBS, 4),
                    "fp64_gops": round(M * OPS_PER_ROW / three / 1e3, 1), "source": "rocprofv3 kernel-trace (median)"})
        row.update({k: v for k, v in info.items() if k not in ("child", "K", "N", "A")})
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
