"""NumPy float64 twin of include/mxv_dqn.h: the Q-learning loss of a batch — TD targets, Huber loss, diagnostics — and its
dense gradient.  Every line below is one IEEE float64 operation on whole columns (NumPy neither fuses nor re-associates them), in the
order the rule states.  The sums are the fixed trees of tests/ppo_host.py (leaf_sums, then tests/norm_tree_host.py's `tree`), used
from there, not copied.  The device must produce the same bits (tests/test_gpu_dqn.py), and tests/test_dqn_host.py holds this file to
torch's float64 autograd and to the exact cases of the rule.

Not a test module.  Nothing under gym_amd/ imports it."""
import numpy as np

import ppo_host as pp

to_f32, bits, tree_sum, leaf_sums, depth, launches = pp.to_f32, pp.bits, pp.tree_sum, pp.leaf_sums, pp.depth, pp.launches
STAT_NAMES = ("loss_term", "td_abs_mean", "q_taken_mean", "target_mean", "linear_fraction", "td_abs_max", "q_taken_min", "q_taken_max")
# measured with the input of tests/test_dqn_host.py (20 000 rows of 6 actions; both target modes, double on and off, with and without
# weights) against torch's float64 autograd of the literal gather / argmax / huber_loss / mean expression, in units of 2^-53 of the
# reference's magnitude.  The tests hold the derived bars — sum_error_bound(depth(M), sum |term|) for the tree,
# (M - 1) 2^-53 sum |term| for torch's order, half a float32 ulp for a float32 output — and these record what is used of them.
B_LOSS = 2.44
B_STATS = 2.44
B_GRAD_Q = 2.68


def _f64(x):
    return None if x is None else np.asarray(x, np.float32).reshape(-1).astype(np.float64)


def first_max(sel):
    """sel float32 [M, A] -> (j* [M], bad [M]): the first maximum by strict >, and whether the row holds a NaN."""
    sel = np.asarray(sel, np.float32)
    best, j = sel[:, 0].copy(), np.zeros(sel.shape[0], np.int64)
    with np.errstate(all="ignore"):
        for a in range(1, sel.shape[1]):
            up = sel[:, a] > best
            best = np.where(up, sel[:, a], best)
            j = np.where(up, a, j)
    return j, np.isnan(sel).any(axis=1)


def rows(q, actions, *, targets=None, reward=None, terminated=None, next_q=None, next_q_online=None, gamma=0.99, delta=1.0, weights=None):
    """The per-row quantities of the rule -> dict of float64 / bool arrays [M].  q float32 [M, A]."""
    q = np.asarray(q, np.float32)
    M, A = q.shape
    a = np.asarray(actions).astype(np.int64).reshape(-1)
    assert a.shape[0] == M and (targets is None) != (reward is None and terminated is None and next_q is None)
    assert targets is None or next_q_online is None
    idx = np.arange(M)
    delta, gamma = np.float64(delta), np.float64(gamma)
    with np.errstate(all="ignore"):
        ok = (a >= 0) & (a < A)
        qa = np.where(ok, q[idx, np.where(ok, a, 0)].astype(np.float64), np.nan)
        if targets is not None:
            y = _f64(targets)
        else:
            nq = np.asarray(next_q, np.float32)
            assert nq.shape == q.shape
            j, bad = first_max(nq if next_q_online is None else next_q_online)
            nv = np.where(bad, np.nan, nq[idx, j].astype(np.float64))
            r = _f64(reward)
            boot = r + gamma * nv
            y = np.where(np.asarray(terminated).reshape(-1).astype(np.uint8) != 0, r, boot)
        e = qa - y
        ae = np.abs(e)
        nan_e, quad = np.isnan(e), ae <= delta
        h = np.where(quad, 0.5 * (e * e), delta * (ae - 0.5 * delta))
        h = np.where(nan_e, np.nan, h)
        dh = np.where(quad, e, np.where(e < 0.0, -delta, delta))
        dh = np.where(nan_e, np.nan, dh)
        w = _f64(weights)
        term = h if w is None else w * h
        lin = np.where(ae > delta, 1.0, 0.0)
    return dict(ok=ok, a=a, qa=qa, y=y, e=e, ae=ae, h=h, dh=dh, w=w, term=term, lin=lin, A=A)


def loss(q, actions, **kw):
    """-> (loss float64, stats float64 [8], td_error float64 [M]), before the float32 rounding, and the sums in a dict."""
    p = rows(q, actions, **kw)
    Mf = np.float64(p["e"].shape[0])
    sums = {k: tree_sum(p[k]) for k in ("term", "ae", "qa", "y", "lin")}
    with np.errstate(all="ignore"):
        # the extrema skip a NaN; a maximum of numbers does not depend on the order of the selects, and a zero leaves as +0.0
        ae_max = np.fmax.reduce(p["ae"], initial=-np.inf) + 0.0
        qa_min = np.fmin.reduce(p["qa"], initial=np.inf) + 0.0
        qa_max = np.fmax.reduce(p["qa"], initial=-np.inf) + 0.0
        value = sums["term"] / Mf
        stats = np.array([value, sums["ae"] / Mf, sums["qa"] / Mf, sums["y"] / Mf, sums["lin"] / Mf, ae_max, qa_min, qa_max], np.float64)
    return np.float64(value), stats, p["e"], sums


def loss_f32(q, actions, **kw):
    """-> (loss, stats, td_error) as the device writes them: float32, NaNs canonical."""
    value, stats, e, _ = loss(q, actions, **kw)
    return to_f32(np.array([value]))[0], to_f32(stats), to_f32(e)


def backward(q, actions, grad_loss, **kw):
    """-> grad_q float64 [M, A], before the float32 rounding; grad_loss: the float32 incoming gradient of the loss."""
    p = rows(q, actions, **kw)
    M, A = p["e"].shape[0], p["A"]
    with np.errstate(all="ignore"):
        gs = np.float64(np.float32(grad_loss)) / np.float64(M)
        val = gs * (p["dh"] if p["w"] is None else p["w"] * p["dh"])
    g = np.zeros((M, A), np.float64)
    ok = p["ok"]
    g[np.arange(M)[ok], p["a"][ok]] = val[ok]
    g[~ok, :] = np.nan
    return g
