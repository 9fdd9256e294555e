#!/usr/bin/env python3
"""The SAC update, fused: one critic update — gym_amd.twin_q_loss in the bootstrap mode on the critics' outputs as one
[M, 2] tensor, with next_log_prob, a device temperature and td_error, and loss.backward() — plus one actor update —
gym_amd.soft_policy_loss and loss.backward() — and one read of each diagnostics vector, next to the literal torch sequence of
examples/sac_pendulum.py that they replace: minimum, float, the target arithmetic and contiguous; the two half squared errors, their
means and their sum, loss.backward(); alpha * log_prob - minimum(q1, q2), mean, loss.backward(); and the float(...) reads of the two
losses, mean Q and mean log_prob.  One pass is one of each on the same inputs (the critic values and log_prob are leaves that require
grad), so that every kernel of a pass belongs to the update.  Timed with `rocprofv3 --kernel-trace` alone, one child process per shape
under `timeout -k 10` (no counters: they are never combined with tracing; the program goes after `--`); times are medians over --iters
passes of the kernels' trace durations:
  * `critic_us`, `actor_us`                                 sac_q_leaf + its sac_tree levels + sac_q_bwd, and sac_pi_leaf + sac_tree + sac_pi_bwd;
  * `kernels_us`, `span_us`, `launches`                     every kernel of one pass of ours: durations summed, first start to last end, count;
  * `torch_kernels_us`, `torch_span_us`, `torch_launches`   the same for one pass of the torch sequence.
`achieved_gbs` is the algorithmic bytes of the four calls over critic_us + actor_us; `fp64_gops` counts the rule's float64 operations per
row.  Not wired into bench.py.

    python benchmarks/sac_loss.py [--iters 20] [--warmup 3]     # one JSON line per shape
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
SHAPES = ((64, 4096, 2), (32, 1 << 20, 2))
HBM_PEAK_GBS = 8000.0
GAMMA, ALPHA = 0.99, 0.2
CHILD_TIMEOUT_S = 600


def bytes_per_row(C):
    """critics forward: q and next_q 8 C, reward 4, terminated 1, next_log_prob 4, td_error 4; backward: the same reads without td_error
    and the gradient rows 4 C.  actor forward: log_prob 4 and q 4 C; backward: q 4 C, grad_log_prob 4 and the gradient rows 4 C."""
    return (13 + 8 * C) + (9 + 12 * C) + (4 + 4 * C) + (4 + 8 * C)


def ops_per_row(C):
    """float64 operations of the rule, about: critics forward 12 + 10 C (the target 4, a column 10, the row's quotients, gap, weight and
    the five additions of the sums), backward 5 + 3 C; actor forward 8, backward 3."""
    return (12 + 10 * C) + (5 + 3 * C) + 8 + 3


def torch_pass(torch, q1, q2, q1_pi, q2_pi, lp, reward, terminated, nq1, nq2, next_lp, alpha):
    """The literal torch sequence of examples/sac_pendulum.py between the networks and the optimizers."""
    with torch.no_grad():
        q_next = torch.minimum(nq1, nq2)
        y = (reward + GAMMA * (1.0 - terminated.float()) * (q_next.view(-1) - alpha * next_lp)).contiguous()
    critic_loss = (0.5 * (q1.view(-1) - y) ** 2).mean() + (0.5 * (q2.view(-1) - y) ** 2).mean()
    critic_loss.backward()
    q_pi = torch.minimum(q1_pi, q2_pi)
    actor_loss = (alpha * lp - q_pi.view(-1)).mean()
    actor_loss.backward()
    return {"critic_loss": float(critic_loss), "actor_loss": float(actor_loss), "q_mean": float(q1.detach().mean()), "log_prob_mean": float(lp.detach().mean())}


def fused_pass(gym_amd, td_error, q12, q12_pi, lp, reward, terminated, nq12, next_lp, alpha):
    critic_loss, q_stats = gym_amd.twin_q_loss(q12, reward=reward, terminated=terminated, next_q=nq12, next_log_prob=next_lp, alpha=alpha, gamma=GAMMA,
                                               td_error=td_error)
    critic_loss.backward()
    actor_loss, pi_stats = gym_amd.soft_policy_loss(lp, q12_pi, alpha=alpha)
    actor_loss.backward()
    return q_stats.tolist(), pi_stats.tolist()


def child(K, N, C, iters, warmup):
    import torch

    import gym_amd

    assert C == 2, "the torch sequence of the example has two critics"
    dev = torch.device("cuda", 0)
    M = K * N
    g = torch.Generator(device=dev).manual_seed(1)
    q12 = (torch.randn((M, C), device=dev, generator=g) * 2.0).requires_grad_()
    q12_pi = (torch.randn((M, C), device=dev, generator=g) * 2.0).requires_grad_()
    nq12 = torch.randn((M, C), device=dev, generator=g) * 2.0
    lp = (torch.randn(M, device=dev, generator=g) * 1.5 - 1.0).requires_grad_()
    next_lp = torch.randn(M, device=dev, generator=g) * 1.5 - 1.0
    reward = torch.randn(M, device=dev, generator=g)
    terminated = (torch.rand(M, device=dev, generator=g) < 0.1).to(torch.uint8)
    alpha = torch.tensor(ALPHA, device=dev)
    td_error = torch.empty(M, device=dev)
    cols = [x[:, c:c + 1].detach().clone().requires_grad_() for x in (q12, q12_pi) for c in range(C)]      # q1, q2, q1_pi, q2_pi as the example has them
    nq = [nq12[:, c:c + 1].contiguous() for c in range(C)]
    leaves = [q12, q12_pi, lp] + cols
    one = torch.zeros((1, 2), device=dev)
    mark_out = (torch.empty(1, dtype=torch.int64, device=dev), None, None)

    def mark():     # a one-row launch of the categorical sampler: the delimiter between passes in the trace
        gym_amd.sample_categorical(one, seed=0, step=0, out=mark_out)

    def one_pass(f):
        for x in leaves:
            x.grad = None
        return f()

    ours = lambda: fused_pass(gym_amd, td_error, q12, q12_pi, lp, reward, terminated, nq12, next_lp, alpha)
    theirs = lambda: torch_pass(torch, cols[0], cols[1], cols[2], cols[3], lp, reward, terminated, nq[0], nq[1], next_lp, alpha)
    mark()
    for f in (ours, theirs):
        for _ in range(warmup + iters):
            one_pass(f)
            mark()
    torch.cuda.synchronize()
    # the two agree as far as float32 arithmetic does: losses and gradients against the torch sequence in float64
    q_stats, pi_stats = one_pass(ours)
    got_q, got_pi, got_lp = q12.grad.double(), q12_pi.grad.double(), lp.grad.double()
    c64 = [x.detach().double().requires_grad_() for x in cols]
    lp64 = lp.detach().double().requires_grad_()
    ref = torch_pass(torch, c64[0], c64[1], c64[2], c64[3], lp64, reward.double(), terminated, nq[0].double(), nq[1].double(), next_lp.double(),
                     alpha.double())
    print(json.dumps({"child": True, "K": K, "N": N, "C": C, "critic_loss": q_stats[0], "critic_loss_torch_f64": ref["critic_loss"],
                      "actor_loss": pi_stats[0], "actor_loss_torch_f64": ref["actor_loss"],
                      "max_abs_diff_grad_q_vs_torch_f64": float((got_q - torch.cat((c64[0].grad, c64[1].grad), 1)).abs().max()),
                      "max_abs_diff_grad_q_pi_vs_torch_f64": float((got_pi - torch.cat((c64[2].grad, c64[3].grad), 1)).abs().max()),
                      "max_abs_diff_grad_log_prob_vs_torch_f64": float((got_lp - lp64.grad).abs().max())}), flush=True)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else float("nan")


def profile(K, N, C, iters, warmup):
    d = tempfile.mkdtemp(prefix="sac_loss_bench_")
    try:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), "rocprofv3", "--kernel-trace", "-d", d, "-o", "trace", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--iters", str(iters), "--warmup", str(warmup), "--child", str(K), str(N), str(C)]
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
    ours = lambda k: any(w in k[2] for w in ("sac_q_leaf", "sac_q_bwd", "sac_pi_leaf", "sac_pi_bwd", "sac_tree"))
    parts = {"critic_us": [], "actor_us": []}
    for seg in mine:
        mk = [k for k in seg if ours(k)]
        names = [k[2] for k in mk]
        assert len(names) == 2 * (launches + 1) and "sac_q_leaf" in names[0] and "sac_q_bwd" in names[launches] and "sac_pi_leaf" in names[launches + 1] \
            and "sac_pi_bwd" in names[-1] and all("sac_tree" in x for x in names[1:launches] + names[launches + 2:-1]), names
        parts["critic_us"].append(us(mk[:launches + 1]))
        parts["actor_us"].append(us(mk[launches + 1:]))
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
    ap.add_argument("--shape", nargs=3, type=int, action="append", help="K N C (default: 64 x 4096 and 32 x 1048576 rows, C = 2)")
    ap.add_argument("--child", nargs=3, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), int(a.child[1]), int(a.child[2]), a.iters, a.warmup)
        return
    from gym_amd.sac import launches

    for K, N, C in (a.shape or SHAPES):
        M = K * N
        ks, info = profile(K, N, C, a.iters, a.warmup)
        r = analyse(ks, a.iters, a.warmup, launches(M))
        both = r["critic_us"] + r["actor_us"]
        gbs = M * bytes_per_row(C) / both / 1e3
        row = {"K": K, "N": N, "C": C, "rows": M}
        row.update({k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items()})
        row.update({"speedup_kernels_vs_torch_kernels": round(r["torch_kernels_us"] / r["kernels_us"], 2),
                    "speedup_span_vs_torch_span": round(r["torch_span_us"] / r["span_us"], 2),
                    "algorithmic_bytes_per_row": bytes_per_row(C), "achieved_gbs": round(gbs, 1), "roofline_frac": round(gbs / HBM_PEAK_GBS, 4),
                    "fp64_gops": round(M * ops_per_row(C) / both / 1e3, 1), "source": "rocprofv3 kernel-trace (median)"})
        row.update({k: v for k, v in info.items() if k not in ("child", "K", "N", "C")})
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
