"""NumPy float64 twin of include/mxv_c51.h: the categorical (C51) Q-learning loss of a batch — the projected target
distribution, the cross-entropy, the diagnostics — its dense gradient, and the expected action values of a categorical head.  Every
line below is one IEEE float64 operation on whole columns (NumPy neither fuses nor re-associates them), in the order the rule states;
EXP and LOG are the operation sequences of tests/policy_host.py, not libm.  The sums over the rows are the fixed trees of
tests/ppo_host.py, used from there, not copied; the sum over the atoms is `atomsum` below.  The device must produce the same bits
(tests/test_gpu_c51.py), and tests/test_c51_host.py holds this file to a literal torch float64 implementation and to the exact cases
of the rule.

Not a test module.  Nothing under gym_amd/ imports it."""
import numpy as np

import policy_host as ph
import ppo_host as pp

EXP, LOG, EXP_CUT = ph.EXP, ph.LOG, ph.EXP_CUT
to_f32, bits, tree_sum, depth = pp.to_f32, pp.bits, pp.tree_sum, pp.depth
SLOTS = 64              # the slots of ATOMSUM: the lanes of a wave
LEAF_ROWS = pp.LEAF_ROWS
STAT_NAMES = ("loss_term", "q_taken_mean", "target_mean", "entropy_mean", "clipped_mass_mean", "row_loss_max", "q_taken_min", "q_taken_max")
# measured with the input of tests/test_c51_host.py (20 000 rows of 6 actions and 51 atoms; both target modes, double on and off, with
# and without weights) against the literal torch float64 implementation written in that test, in units of 2^-53: `projected` absolute
# (a mass is at most 1); a row's loss of max(1, |reference|); the loss and the means of the mean magnitude of what they sum (a mean and
# an expectation over a support that straddles zero may cancel); the gradient of |g| / M times the row's weight.  The tests hold the
# derived bars of that test's docstring and, at the small shapes, twice these rounded up (policy_eval_host.bar).
B_PROJECTED = 6.00
B_ROW_LOSS = 7.99
B_LOSS = 1.40
B_STATS = 1.82
B_GRAD = 7.91


def launches(M):
    """Kernel launches of one forward: the rows, the leaves (which finish a batch of one leaf), then one per tree level."""
    return 2 if int(M) <= LEAF_ROWS else 1 + pp.launches(M)


def atomsum(v):
    """ATOMSUM: [..., 64] -> [...]: s[k] <- s[2k] + s[2k+1], six times."""
    v = np.asarray(v, np.float64)
    assert v.shape[-1] == SLOTS
    with np.errstate(all="ignore"):
        for _ in range(6):
            v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def support(Z, v_min, v_max):
    """-> (v_min, v_max, dz, z [64]) as float64: z_k of every slot (the slots k >= Z only ever meet a zero)."""
    v_min, v_max = np.float64(v_min), np.float64(v_max)
    dz = (v_max - v_min) / np.float64(Z - 1)
    z = v_min + np.arange(SLOTS, dtype=np.float64) * dz
    return v_min, v_max, dz, z


def soft(x):
    """SOFT of float32 rows [..., Z] -> dict of d, e, p [..., 64], S [...], bad [...]."""
    x = np.asarray(x, np.float32)
    Z = x.shape[-1]
    lead = x.shape[:-1]

    def slots(v, fill):      # the Z atoms in the 64 slots
        out = np.full(lead + (SLOTS,), fill, np.float64)
        out[..., :Z] = v
        return out

    with np.errstate(all="ignore"):
        bad = np.isnan(x).any(-1) | (x == np.inf).any(-1) | (x == -np.inf).all(-1)
        xs = np.where(bad[..., None], 0.0, x.astype(np.float64))      # a bad row computes on zeros and is replaced
        mx = xs.max(-1) + 0.0
        d = xs - mx[..., None]
        live = ~(d < EXP_CUT)
        e = slots(np.where(live, EXP(np.where(live, d, 0.0)), 0.0), 0.0)      # a slot k >= Z is a logit of -Inf: d = -Inf, e = 0
        d = slots(d, -np.inf)
        S = atomsum(e)
        p = e / S[..., None]
        d = np.where(bad[..., None], np.nan, d)
        p = np.where(bad[..., None], np.nan, p)
    return dict(d=d, e=e, p=p, S=S, bad=bad)


def q_values(logits, *, v_min, v_max):
    """float32 [..., A, Z] -> float64 [..., A] before the float32 rounding: ATOMSUM(p_k z_k), NaN where the row is bad."""
    logits = np.asarray(logits, np.float32)
    z = support(logits.shape[-1], v_min, v_max)[3]
    with np.errstate(all="ignore"):
        return atomsum(soft(logits)["p"] * z)


def first_max(Q):
    """Q [M, A] -> j* [M]: the first maximum by strict >."""
    best, j = Q[:, 0].copy(), np.zeros(Q.shape[0], np.int64)
    with np.errstate(all="ignore"):
        for a in range(1, Q.shape[1]):
            up = Q[:, a] > best
            best = np.where(up, Q[:, a], best)
            j = np.where(up, a, j)
    return j


def _f64(x):
    return None if x is None else np.asarray(x, np.float32).reshape(-1).astype(np.float64)


def rows(logits, actions, *, v_min, v_max, target_probs=None, reward=None, terminated=None, next_logits=None, next_logits_online=None,
         gamma=0.99, weights=None):
    """The per-row quantities of the rule -> dict.  logits float32 [M, A, Z]."""
    logits = np.asarray(logits, np.float32)
    M, A, Z = logits.shape
    a = np.asarray(actions).astype(np.int64).reshape(-1)
    assert a.shape[0] == M and (target_probs is None) != (reward is None and terminated is None and next_logits is None)
    assert target_probs is None or next_logits_online is None
    idx, k = np.arange(M), np.arange(SLOTS, dtype=np.float64)
    inside = np.arange(SLOTS) < Z
    v_min, v_max, dz, z = support(Z, v_min, v_max)
    z_top, gamma = np.float64(Z - 1), np.float64(gamma)
    with np.errstate(all="ignore"):
        ok = (a >= 0) & (a < A)
        s = soft(logits[idx, np.where(ok, a, 0)])
        L = LOG(s["S"])
        lp = s["d"] - L[:, None]
        qa = atomsum(s["p"] * z)
        ent = L - atomsum(np.where(s["e"] == 0.0, 0.0, s["e"] * s["d"])) / s["S"]
        jstar = None
        if target_probs is not None:
            m = np.zeros((M, SLOTS))
            m[:, :Z] = np.asarray(target_probs, np.float32).reshape(M, Z).astype(np.float64)
            cm = np.zeros(M)
        else:
            nl = np.asarray(next_logits, np.float32)
            assert nl.shape == logits.shape
            sa = soft(nl if next_logits_online is None else np.asarray(next_logits_online, np.float32))
            jstar = first_max(atomsum(sa["p"] * z))
            selbad = sa["bad"].any(1)
            tp = soft(nl[idx, jstar])["p"]
            term = (np.asarray(terminated).reshape(-1).astype(np.uint8) != 0)[:, None]
            first = np.where(np.arange(SLOTS) == 0, 1.0, 0.0)[None, :]
            pn = np.where(term, first, np.where(selbad[:, None], np.nan, tp))
            r = _f64(reward)[:, None]
            boot = r + gamma * z[None, :]
            tz = np.where(term, r, boot)
            c = np.where(tz < v_min, v_min, tz)
            c = np.where(c > v_max, v_max, c)
            b = (c - v_min) / dz
            b = np.where(b > z_top, z_top, b)
            cm = atomsum(np.where(inside & ((tz < v_min) | (tz > v_max)), pn, 0.0))
            m = np.zeros((M, SLOTS))
            for j in range(Z):
                w = 1.0 - np.abs(b[:, j:j + 1] - k)
                w = np.where(w < 0.0, 0.0, w)
                m = m + pn[:, j:j + 1] * w
            m = np.where(inside, m, 0.0)
        sm = atomsum(m)
        y = atomsum(m * z)
        ce = -atomsum(np.where(m == 0.0, 0.0, m * lp))
        qa, ent, ce = (np.where(ok, v, np.nan) for v in (qa, ent, ce))
        w = _f64(weights)
        term_ = ce if w is None else w * ce
    return dict(ok=ok, a=a, p=s["p"], lp=lp, m=m, sm=sm, qa=qa, y=y, ent=ent, cm=cm, ce=ce, w=w, term=term_, jstar=jstar, A=A, Z=Z)


def finish(p):
    """The per-row columns term, qa, y, ent, cm, ce -> (loss float64, stats float64 [8], sums dict): the trees and the finish."""
    Mf = np.float64(p["ce"].shape[0])
    sums = {k: tree_sum(p[k]) for k in ("term", "qa", "y", "ent", "cm")}
    with np.errstate(all="ignore"):
        # the extrema skip a NaN; a maximum of numbers does not depend on the order of the selects, and a zero leaves as +0.0
        ce_max = np.fmax.reduce(p["ce"], initial=-np.inf) + 0.0
        qa_min = np.fmin.reduce(p["qa"], initial=np.inf) + 0.0
        qa_max = np.fmax.reduce(p["qa"], initial=-np.inf) + 0.0
        value = sums["term"] / Mf
        stats = np.array([value, sums["qa"] / Mf, sums["y"] / Mf, sums["ent"] / Mf, sums["cm"] / Mf, ce_max, qa_min, qa_max], np.float64)
    return np.float64(value), stats, sums


def loss(logits, actions, **kw):
    """-> (loss float64, stats float64 [8], row dict, sums dict), before the float32 rounding."""
    p = rows(logits, actions, **kw)
    value, stats, sums = finish(p)
    return value, stats, p, sums


def loss_f32(logits, actions, **kw):
    """-> (loss, stats, row_loss [M], projected [M, Z]) as the device writes them: float32, NaNs canonical."""
    value, stats, p, _ = loss(logits, actions, **kw)
    return to_f32(np.array([value]))[0], to_f32(stats), to_f32(p["ce"]), to_f32(p["m"][:, :p["Z"]])


def grad_of(p, grad_loss, batch_rows=None):
    """The rows `p` -> grad_logits float64 [M, A, Z], before the float32 rounding; grad_loss: the float32 incoming gradient of the loss.
    batch_rows: the M of the whole batch when these rows are a slice of it (the rows are independent but for Mf)."""
    M, A, Z = p["ce"].shape[0], p["A"], p["Z"]
    with np.errstate(all="ignore"):
        gs = np.float64(np.float32(grad_loss)) / np.float64(M if batch_rows is None else batch_rows)
        dl = p["p"] * p["sm"][:, None] - p["m"]
        val = gs * (dl if p["w"] is None else p["w"][:, None] * dl)
    g = np.zeros((M, A, Z), np.float64)
    ok = p["ok"]
    g[np.arange(M)[ok], p["a"][ok]] = val[ok][:, :Z]
    g[~ok] = np.nan
    return g


def backward(logits, actions, grad_loss, **kw):
    """-> grad_logits float64 [M, A, Z], before the float32 rounding."""
    return grad_of(rows(logits, actions, **kw), grad_loss)
