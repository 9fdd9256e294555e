"""tests/policy_host.py — the NumPy twin of include/mxv_policy.h, which the device is compared with bit for bit — held to 200-bit
mpmath: the accuracy of log_prob and entropy, the selected action against the exact rule, the distribution of the draws, and what the
rule promises structurally (sharding, the high step word, masks, degenerate rows).  Also: the constants in the kernel source are the
generator's, and the Python front end validates without a device."""
import os
import re
import sys

import mpmath as mp
import numpy as np
import pytest

import policy_host as ph
from conftest import ROOT


ACTIONS = (2, 3, 4, 6, 17)
ROWS = 3000
SCALES = (0.1, 1.0, 5.0, 30.0)


def _rows(A):
    """The input the bars B_LOG_PROB / B_ENTROPY were measured on: standard normals scaled by 0.1 / 1 / 5 / 30, cast to float32."""
    rng = np.random.default_rng(100 + A)
    x = (rng.standard_normal((ROWS, A)) * np.repeat(SCALES, ROWS // len(SCALES))[:, None]).astype(np.float32)
    w = rng.integers(0, 2 ** 32, ROWS, dtype=np.uint64).astype(np.uint32)
    return x, w


@pytest.fixture(scope="module")
def exact():
    """Per A: the twin's results and, per row, the exact (200-bit) log_prob of the twin's action, entropy, cumulative sums and S."""
    out = {}
    with mp.workprec(200):
        for A in ACTIONS:
            x, w = _rows(A)
            r = ph.evaluate(x, w)
            rows = []
            for i in range(ROWS):
                xs = [mp.mpf(float(v)) for v in x[i]]
                m = max(xs)
                e = [mp.exp(v - m) for v in xs]
                c = [mp.fsum(e[:a + 1]) for a in range(A)]
                S = c[-1]
                L = mp.log(S)
                a = int(r["action"][i])
                rows.append((xs[a] - m - L, L - mp.fsum(e_ * (v - m) for e_, v in zip(e, xs)) / S, c, S))
            out[A] = (x, w, r, rows)
    return out


def _ulp32(v):
    return float(np.spacing(np.abs(np.float32(v)))) if v != 0 else float(np.float32(2.0 ** -149))


def test_log_prob_and_entropy_are_accurate(exact):
    worst_lp = worst_en = 0.0
    with mp.workprec(200):
        for A in ACTIONS:
            x, w, r, rows = exact[A]
            lp32, en32 = ph.to_f32(r["log_prob"]), ph.to_f32(r["entropy"])
            for i, (lp, en, _, _) in enumerate(rows):
                elp = float(abs(mp.mpf(float(r["log_prob"][i])) - lp) * 2 ** 53)
                een = float(abs(mp.mpf(float(r["entropy"][i])) - en) * 2 ** 53)
                worst_lp, worst_en = max(worst_lp, elp), max(worst_en, een)
                # the float32 results: half a float32 ulp of the exact value plus the float64 bar
                assert abs(mp.mpf(float(lp32[i])) - lp) <= mp.mpf(_ulp32(float(lp))) / 2 + mp.mpf(ph.BAR_LOG_PROB) * mp.mpf(2) ** -53, (A, i)
                assert abs(mp.mpf(float(en32[i])) - en) <= mp.mpf(_ulp32(float(en))) / 2 + mp.mpf(ph.BAR_ENTROPY) * mp.mpf(2) ** -53, (A, i)
    print(f"measured B: log_prob {worst_lp:.3f}, entropy {worst_en:.3f} (x 2^-53)")
    assert worst_lp <= ph.BAR_LOG_PROB and worst_en <= ph.BAR_ENTROPY, (worst_lp, worst_en)
    # the named constants are what was measured on this input (to their two decimals, rounded up), the bars twice that, rounded up
    assert worst_lp <= ph.B_LOG_PROB < worst_lp + 0.01 and worst_en <= ph.B_ENTROPY < worst_en + 0.01, (worst_lp, worst_en)
    assert ph.BAR_LOG_PROB == int(np.ceil(2 * ph.B_LOG_PROB)) and ph.BAR_ENTROPY == int(np.ceil(2 * ph.B_ENTROPY))


def test_selected_action_is_the_exact_rules(exact):
    left_out = total = 0
    with mp.workprec(200):
        for A in ACTIONS:
            x, w, r, rows = exact[A]
            for i, (_, _, c, S) in enumerate(rows):
                thr = (mp.mpf(int(w[i])) + mp.mpf("0.5")) * mp.mpf(2) ** -32 * S
                want = next((a for a in range(A) if c[a] > thr), A - 1)
                total += 1
                if min(abs(ca - thr) for ca in c) / S < mp.mpf(2) ** -45:
                    left_out += 1
                    continue
                assert int(r["action"][i]) == want, (A, i)
    print(f"left out: {left_out} of {total} rows")
    assert left_out * 10 ** 4 <= total, (left_out, total)


def test_exp_and_log_sequences():
    """EXP within 1.5 ulp on [-708, 0], LOG within 8 * 2^-53 on [1, 64]; the end points and exact powers of two."""
    rng = np.random.default_rng(5)
    d = np.concatenate((-rng.uniform(0, 708, 4000), [0.0, -708.0, -1e-300, -0.5 * np.log(2.0)]))
    e = ph.EXP(d)
    S = np.concatenate((rng.uniform(1, 64, 4000), 2.0 ** np.arange(7), [np.nextafter(2.0, 1.0), np.sqrt(2.0)]))
    L = ph.LOG(S)
    with mp.workprec(200):
        for a, b in zip(d, e):
            assert abs(mp.mpf(float(b)) - mp.exp(mp.mpf(float(a)))) <= 1.5 * float(np.spacing(b)), a
        for a, b in zip(S, L):
            assert abs(mp.mpf(float(b)) - mp.log(mp.mpf(float(a)))) * 2 ** 53 <= 8, a
    assert ph.EXP(0.0) == 1.0 and ph.LOG(1.0) == 0.0 and np.all(e[:-4] >= np.finfo(np.float64).tiny)


def _softmax(row):
    with mp.workprec(200):
        xs = [mp.mpf(float(v)) for v in np.asarray(row, np.float32)]
        m = max(xs)
        e = [mp.exp(v - m) for v in xs]
        return [float(v / mp.fsum(e)) for v in e]


DIST_ROWS = {2: [0.3, -0.9], 3: [1.5, -np.inf, 0.25], 6: [0.1, -2.0, 1.0, 0.0, -0.5, 2.5]}


@pytest.mark.parametrize("A", sorted(DIST_ROWS))
def test_distribution_over_envs_and_over_steps(A):
    n = 1 << 16
    row = np.asarray(DIST_ROWS[A], np.float32)
    p = np.asarray(_softmax(row))
    x = np.broadcast_to(row, (n, A))
    over_envs = ph.sample_categorical(x, seed=2024 + A, step=3, env_offset=5)[0]
    G = 77
    w = np.concatenate([ph.words(99 + A, [G], t) for t in range(n)])
    over_steps = ph.evaluate(x, w)["action"]
    for acts in (over_envs, over_steps):
        counts = np.bincount(acts, minlength=A)
        sd = np.sqrt(n * p * (1 - p))
        assert np.all(np.abs(counts - n * p) <= 5 * sd), (A, counts, n * p, sd)
        for a in np.flatnonzero(np.isneginf(row)):
            assert counts[a] == 0


def test_a_draw_depends_on_seed_env_and_step_alone():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((301, 6)).astype(np.float32)
    off = 1001                                            # not a multiple of 4
    whole = ph.sample_categorical(x, seed=9, step=12, env_offset=off)
    cut = 130                                             # the second shard's offset 1131 is not one either
    a = ph.sample_categorical(x[:cut], seed=9, step=12, env_offset=off)
    b = ph.sample_categorical(x[cut:], seed=9, step=12, env_offset=off + cut)
    for k in range(3):
        assert np.array_equal(ph.bits(whole[k]) if k else whole[k], np.concatenate((ph.bits(a[k]), ph.bits(b[k]))) if k else np.concatenate((a[k], b[k])))
    # another seed, another step or another env: other words
    assert not np.array_equal(ph.words(9, np.arange(64), 12), ph.words(10, np.arange(64), 12))
    assert not np.array_equal(ph.words(9, np.arange(64), 12), ph.words(9, np.arange(64), 13))
    assert not np.array_equal(ph.words(9, np.arange(64), 12), ph.words(9, np.arange(64) + 64, 12))


def test_the_high_step_word_and_the_stream_tag():
    from oracle import oracle

    G = np.arange(8, dtype=np.uint64) + 3
    lo, hi = ph.words(1, G, 5), ph.words(1, G, 2 ** 32 + 5)
    assert not np.array_equal(lo, hi)
    for t in (5, 2 ** 32 + 5, 2 ** 61 + 2 ** 32 + 5):
        w4 = oracle.philox4x32_10((1, 0, t & 0xffffffff, ((t >> 32) & 0x0fffffff) | (7 << 28)), (1, 0))
        assert np.array_equal(ph.words(1, np.arange(4, 8), t), w4)
    # bits 28 and up of t_hi belong to the stream tag
    assert np.array_equal(ph.words(1, G, 5), ph.words(1, G, 2 ** 60 + 5))
    # the engine's word-per-step action stream (tag 1) under the same key and counter is another stream
    assert not np.array_equal(oracle.philox4x32_10((1, 0, 5, 1 << 28), (1, 0)), ph.words(1, np.arange(4, 8), 5))


def test_masks_extremes_and_degenerate_rows():
    inf, nan = np.inf, np.nan
    n = 4096
    masked = np.broadcast_to(np.asarray([0.5, -inf, 0.1], np.float32), (n, 3))
    a, lp, en = ph.sample_categorical(masked, seed=3, step=0)
    assert not np.any(a == 1) and np.all(np.isfinite(lp)) and np.all(np.isfinite(en))
    two = ph.evaluate(np.asarray([[0.5, 0.1]], np.float32), ph.words(3, [0], 0))
    assert ph.bits(en[:1]) == ph.bits(ph.to_f32(two["entropy"]))                     # a masked action adds nothing to the entropy
    rows = np.asarray([[nan, 0, 0], [0, inf, 0], [-inf, -inf, -inf], [0, -inf, nan], [3e38, -3e38, 0], [0, -709, -800], [1, 1, 1],
                       [-3e38, -3e38, -3e38], [-inf, 2, -inf]], np.float32)
    a, lp, en = ph.sample_categorical(rows, seed=4, step=1)
    assert np.array_equal(a[:4], [0, 0, 0, 0])
    assert np.all(ph.bits(lp[:4]) == ph.CANONICAL_NAN) and np.all(ph.bits(en[:4]) == ph.CANONICAL_NAN)
    assert a[4] == 0 and lp[4] == 0 and en[4] == 0                                   # gaps beyond 708: one action carries everything
    assert a[5] == 0 and lp[5] == 0 and en[5] == 0
    assert np.all(lp[6:8] == np.float32(-np.log(3.0))) and np.all(en[6:8] == np.float32(np.log(3.0)))
    assert a[8] == 1 and lp[8] == 0 and en[8] == 0


def test_the_kernel_source_carries_the_generated_constants():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gaussian_coefficients
        import policy_coefficients
    finally:
        sys.path.pop(0)
    block, src = ph.rule_block("mxv_policy.hip")
    assert block == gaussian_coefficients.block() and block.startswith(policy_coefficients.block() + "\n")
    tag = re.search(r"kStreamPolicy = (\d+)u", src)
    assert tag and int(tag.group(1)) == ph.STREAM_POLICY == 7
    assert "7<<28" in open(os.path.join(ROOT, "include", "mxv.h")).read().replace(" ", "")


def test_the_front_end_validates_without_a_device():
    import subprocess

    code = ("import sys; import gym_amd.policy as p; assert 'torch' not in sys.modules; import gym_amd; "
            "assert gym_amd.sample_categorical is p.sample_categorical and gym_amd.PolicySampler is p.PolicySampler")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
    import torch

    from gym_amd import _native, policy
    from gym_amd.returns import GAE_EXPORTS

    assert not set(policy.POLICY_EXPORTS) & (set(_native.EXPORTS) | set(GAE_EXPORTS))
    x = torch.zeros((4, 3))
    for kw, what in ((dict(logits=x.double()), "float32"), (dict(logits=x[0]), "shape"), (dict(logits=torch.zeros((4, 65))), "shape"),
                     (dict(logits=torch.zeros((3, 4)).t()), "contiguous"), (dict(seed=-1), "seed"), (dict(seed=1.5), "seed"),
                     (dict(step=True), "step"), (dict(step=torch.zeros(1, dtype=torch.int32)), "int64"), (dict(env_offset=2 ** 64), "env_offset"),
                     (dict(action_dtype=torch.float32), "action_dtype"), (dict(out=(torch.zeros(4, dtype=torch.int64),)), "3 entries"),
                     (dict(out=(torch.zeros(5, dtype=torch.int64), None, None)), "shape"),
                     (dict(out=(torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.float64), None)), "float32"),
                     (dict(), "device tensor")):
        args = dict(logits=x, seed=0, step=0)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            policy.sample_categorical(**args)
    with pytest.raises(ValueError, match="num_actions"):
        policy.PolicySampler(0)
