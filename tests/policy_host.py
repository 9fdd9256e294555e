"""NumPy float64 twin of the rule in include/mxv_policy.h: categorical draws from logits, their log-probabilities and
the entropy.  Every line below is one IEEE float64 operation on whole columns (NumPy neither fuses nor re-associates them), in the order
the rule states; EXP and LOG are the header's operation sequences, not libm.  The device must produce the same bits
(tests/test_gpu_policy.py), and tests/test_policy_host.py holds this file to 200-bit mpmath.  The Philox words come from
oracle.philox4x32_10, the constants from tools/policy_coefficients.py."""
import os
import re
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
try:
    import policy_coefficients as _coef
finally:
    sys.path.pop(0)

CANONICAL_NAN = np.uint32(0x7FC00000)
STREAM_POLICY = 7
EXP_CUT = -708.0
# measured on this rule with the input of tests/test_policy_host.py (15 000 rows, A in 2, 3, 4, 6, 17; scales 0.1, 1, 5, 30), in units
# of 2^-53, against 200-bit mpmath, before the float32 rounding; the tests hold twice that, rounded up
B_LOG_PROB = 7.70
B_ENTROPY = 6.14
BAR_LOG_PROB = int(np.ceil(2 * B_LOG_PROB))
BAR_ENTROPY = int(np.ceil(2 * B_ENTROPY))

_C = _coef.constants()
INV_LN2, LN2_HI, LN2_LO, SQRT_HALF = (np.float64(_C[k]) for k in ("inv_ln2", "ln2_hi", "ln2_lo", "sqrt_half"))
EXP_C = [np.float64(x) for x in _C["exp_c"]]
LOG_C = [np.float64(x) for x in _C["log_c"]]
# the names of the generated constant block (tools/gaussian_coefficients.py), as a C++ file would define them
RULE_NAMES = re.compile(r"constexpr double k(InvLn2|Ln2Hi|Ln2Lo|SqrtHalf|ExpC|LogC|Pio2Hi|Pio2Lo|HalfLog2Pi|EntC|SinC|CosC)\b")


def rule_block(kernel_file):
    """The generated constant block of gym_amd/csrc/mxv_policy_rule.hpp, the one text of it: `kernel_file` includes that header and
    defines none of the block's names itself.  -> (the block, the kernel file's source)"""
    csrc = os.path.join(ROOT, "gym_amd", "csrc")
    src = open(os.path.join(csrc, kernel_file)).read()
    assert '#include "mxv_policy_rule.hpp"' in src and not RULE_NAMES.search(src), kernel_file
    rule = open(os.path.join(csrc, "mxv_policy_rule.hpp")).read()
    assert len(RULE_NAMES.findall(rule)) == 12      # each name once
    block = rule[rule.index("gaussian_coefficients.py, verbatim"):rule.index("end of the generated block")]
    return "\n".join(block.splitlines()[1:-1]), src


def EXP(d):
    """d in [-708, 0] (categorical) or |d| <= 80 (Gaussian, tests/gaussian_host.py), float64."""
    d = np.asarray(d, np.float64)
    k = np.rint(d * INV_LN2)
    r = (d - k * LN2_HI) - k * LN2_LO
    p = np.full_like(d, EXP_C[-1])
    for c in EXP_C[-2::-1]:
        p = p * r + c
    return np.ldexp(p, k.astype(np.int32))


def LOG(S):
    """S in [1, 64] (categorical) or 2^-33 <= S < 1 (Gaussian), float64."""
    S = np.asarray(S, np.float64)
    f, e = np.frexp(S)                        # f in [1/2, 1)
    low = f < SQRT_HALF
    f = np.where(low, f * 2.0, f)             # exact: f in [sqrt 1/2, sqrt 2)
    e = np.where(low, e - 1, e).astype(np.float64)
    s = (f - 1.0) / (f + 1.0)
    z = s * s
    p = np.full_like(S, LOG_C[-1])
    for c in LOG_C[-2::-1]:
        p = p * z + c
    return ((e * LN2_HI) + (2.0 * s) * p) + e * LN2_LO


def to_f32(x):
    with np.errstate(all="ignore"):
        y = np.asarray(x, np.float64).astype(np.float32)
    b = y.view(np.uint32).copy()
    b[np.isnan(y)] = CANONICAL_NAN
    return b.view(np.float32)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


_words_cache = {}


def words(seed, G, t):
    """The rule's word w of the global env indices G (uint64 array) at step t."""
    from oracle import oracle

    G = np.asarray(G, np.uint64)
    seed, t = int(seed) & (2 ** 64 - 1), int(t) & (2 ** 64 - 1)
    key = (seed & 0xffffffff, seed >> 32)
    out = np.empty(G.shape, np.uint32)
    for i, g in enumerate(G.tolist()):
        q = g >> 2
        ck = (seed, q, t)
        w4 = _words_cache.get(ck)
        if w4 is None:
            ctr = (q & 0xffffffff, q >> 32, t & 0xffffffff, ((t >> 32) & 0x0fffffff) | (STREAM_POLICY << 28))
            w4 = oracle.philox4x32_10(ctr, key)
            if len(_words_cache) > (1 << 18):
                _words_cache.clear()
            _words_cache[ck] = w4
        out[i] = w4[g & 3]
    return out


def u01(w):
    return (np.asarray(w, np.uint32).astype(np.float64) + 0.5) * np.float64(2.0 ** -32)


def evaluate(logits, w):
    """The rule on float32 logits [N, A] with the words w [N] -> dict of float64 / int arrays (before the float32 rounding):
    action, log_prob, entropy, S, thr, c [N, A], e [N, A], d [N, A], degenerate."""
    x32 = np.asarray(logits, np.float32)
    N, A = x32.shape
    x = x32.astype(np.float64)
    with np.errstate(all="ignore"):
        degenerate = np.isnan(x).any(1) | (x == np.inf).any(1) | (x == -np.inf).all(1)
        m = x[:, 0].copy()
        for a in range(1, A):
            m = np.where(x[:, a] > m, x[:, a], m)
        m = np.where(degenerate, 0.0, m)
        xs = np.where(degenerate[:, None], 0.0, x)           # keep the arithmetic of degenerate rows quiet; their results are replaced
        d = xs - m[:, None]
        live = ~(d < EXP_CUT)
        e = np.where(live, EXP(np.where(live, d, 0.0)), 0.0)
        c = np.empty_like(e)
        acc = np.zeros(N, np.float64)
        T = np.zeros(N, np.float64)
        for a in range(A):
            acc = acc + e[:, a]
            c[:, a] = acc
            T = T + np.where(e[:, a] == 0.0, 0.0, e[:, a] * np.where(live[:, a], d[:, a], 0.0))
        S = acc
        thr = u01(w) * S
        action = np.full(N, A - 1, np.int64)
        for a in range(A - 1, -1, -1):
            action = np.where(c[:, a] > thr, a, action)
        L = LOG(S)
        log_prob = d[np.arange(N), action] - L
        entropy = L - T / S
    action = np.where(degenerate, 0, action)
    log_prob = np.where(degenerate, np.nan, log_prob)
    entropy = np.where(degenerate, np.nan, entropy)
    return dict(action=action, log_prob=log_prob, entropy=entropy, S=S, thr=thr, c=c, e=e, d=d, degenerate=degenerate)


def sample_categorical(logits, *, seed, step, env_offset=0):
    """-> (actions int64 [N], log_prob float32 [N], entropy float32 [N])."""
    x = np.asarray(logits, np.float32)
    G = np.uint64(env_offset) + np.arange(x.shape[0], dtype=np.uint64)
    r = evaluate(x, words(seed, G, step))
    return r["action"], to_f32(r["log_prob"]), to_f32(r["entropy"])
