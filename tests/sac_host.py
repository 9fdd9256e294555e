"""NumPy float64 twin of include/mxv_sac.h: the soft twin-critic target, the loss of the C critics against it with its
diagnostics and its dense gradient, and the actor's loss with its diagnostics and both gradients.  Every line below is one IEEE float64
operation on whole columns (NumPy neither fuses nor re-associates them), in the order the rule states, and carries the rule's own line
as its comment.  The sums are the fixed trees of tests/ppo_host.py and the first extremum of a row is tests/dqn_host.py's first_max,
used from there, not copied: the first minimum by strict < of x is the first maximum by strict > of -x (negation is exact, a NaN
compares false either way, and of two zeros of either sign the first stays).  The device must produce the same bits
(tests/test_gpu_sac.py), and tests/test_sac_host.py holds this file to torch's float64 autograd and to the exact cases of the rule.

Not a test module.  Nothing under gym_amd/ imports it."""
import numpy as np

import dqn_host as dh
import ppo_host as pp

to_f32, bits, tree_sum, depth, launches = pp.to_f32, pp.bits, pp.tree_sum, pp.depth, pp.launches
Q_STAT_NAMES = ("loss_term", "td_abs_mean", "q_mean", "target_mean", "critic_gap_mean", "td_abs_max", "q_min", "q_max")
PI_STAT_NAMES = ("loss_term", "log_prob_mean", "q_pi_mean", "critic_gap_mean", "later_critic_fraction", "log_prob_max", "q_pi_min", "q_pi_max")
# measured with the input of tests/test_sac_host.py (20 000 rows of 1, 2 and 5 critics; both target modes, with and without the entropy
# term, gamma and discount, with and without weights, delta 1 and inf) against torch's float64 autograd of the literal minimum /
# huber_loss / mean expressions, in units of 2^-53 of the reference's magnitude.  The tests hold the derived bars —
# sum_error_bound(depth(M), sum |term|) for the tree, (M - 1) 2^-53 sum |term| for torch's order, a few roundings of a row for a
# gradient — and these record what is used of them.
B_TARGETS = 0.0
B_Q_LOSS = 2.19
B_Q_STATS = 3.39
B_GRAD_Q = 3.23
B_PI_LOSS = 1.71
B_PI_STATS = 1.71
B_GRAD_PI = 2.49


def _f64(x):
    return None if x is None else np.asarray(x, np.float32).reshape(-1).astype(np.float64)


def ends(x):
    """x float32 [M, C] -> dict of mn, mx (float64), jmin, bad, gap of every row."""
    x = np.asarray(x, np.float32)
    idx = np.arange(x.shape[0])
    with np.errstate(all="ignore"):
        jmin, bad = dh.first_max(-x)      # mn = x[i, 0], jmin = 0;  for c = 1 .. C-1:  if x[i, c] < mn: mn = x[i, c], jmin = c
        jmax, _ = dh.first_max(x)         # mx = x[i, 0];  for c = 1 .. C-1:  if x[i, c] > mx: mx = x[i, c]
        mn, mx = x[idx, jmin].astype(np.float64), x[idx, jmax].astype(np.float64)
        # a NaN in column 0 stays the running extremum (every compare is false); the row is bad and mn, mx are replaced wherever used
        gap = np.where(bad, np.nan, mx - mn)      # gap = bad ? NaN : (double)mx - (double)mn
    return dict(mn=mn, mx=mx, jmin=jmin, bad=bad, gap=gap)      # bad = any x[i, c] is NaN


def targets(next_q, reward, terminated, *, next_log_prob=None, alpha=None, gamma=None, discount=None):
    """-> y float64 [M], before the float32 rounding.  next_q float32 [M, C]; alpha a number (a device tensor's float32 value)."""
    assert (next_log_prob is None) == (alpha is None) and (gamma is None or discount is None)
    m = ends(next_q)
    r = _f64(reward)
    term = np.asarray(terminated).reshape(-1).astype(np.uint8) != 0      # term = terminated[i] != 0
    g = np.float64(0.99 if gamma is None else gamma) if discount is None else _f64(discount)      # g    = discount ? (double)discount[i] : gamma
    with np.errstate(all="ignore"):
        nv = np.where(m["bad"], np.nan, m["mn"])      # nv  = bad ? NaN : (double)mn
        v = nv
        if next_log_prob is not None:
            al = np.float64(alpha)                    # al   = alpha_dev ? (double)alpha_dev[0] : alpha
            v = nv - al * _f64(next_log_prob)         # v   = next_log_prob ? nv - al * (double)next_log_prob[i] : nv
        boot = r + g * v
        return np.where(term, r, boot)                # y   = term ? r : r + g * v


def targets_f32(next_q, reward, terminated, **kw):
    """-> targets_out [M] as the device writes it: float32, NaNs canonical."""
    return to_f32(targets(next_q, reward, terminated, **kw))      # targets_out[i] = float32(y)


def _y(q, given, reward, terminated, next_q, kw):
    assert (given is None) != (reward is None and terminated is None and next_q is None)
    if given is not None:
        assert not kw
        return _f64(given)
    assert np.asarray(next_q).shape == np.asarray(q).shape
    return targets(next_q, reward, terminated, **kw)


def q_rows(q, *, targets=None, reward=None, terminated=None, next_q=None, delta=np.inf, weights=None, **kw):
    """The per-row and per-column quantities of the critics' rule -> dict.  q float32 [M, C]; kw: next_log_prob, alpha, gamma, discount."""
    q = np.asarray(q, np.float32)
    M, C = q.shape
    delta = np.float64(delta)
    y = _y(q, targets, reward, terminated, next_q, kw)
    w = _f64(weights)
    with np.errstate(all="ignore"):
        qd = q.astype(np.float64)
        e = qd - y[:, None]      # e_c = (double)q[i, c] - y;  ae_c = |e_c|
        ae = np.abs(e)
        nan_e, quad = np.isnan(e), ae <= delta
        H = np.where(nan_e, np.nan, np.where(quad, 0.5 * (e * e), delta * (ae - 0.5 * delta)))      # H(e_c)  = ae_c <= delta ? 0.5 * (e_c * e_c) : delta * (ae_c - 0.5 * delta)
        dH = np.where(nan_e, np.nan, np.where(quad, e, np.where(e < 0.0, -delta, delta)))           # dH(e_c) = ae_c <= delta ? e_c : (e_c < 0 ? -delta : delta)
        h, sa, sq = np.zeros(M), np.zeros(M), np.zeros(M)
        far, fa = e[:, 0].copy(), ae[:, 0].copy()      # far = e_0, fa = ae_0;  for c = 1 .. C-1:  if ae_c > fa: far = e_c, fa = ae_c
        for c in range(C):
            h = h + H[:, c]        # h   = +0.0;  for c ascending: h = h + H(e_c)
            sa = sa + ae[:, c]     # sa  = +0.0;  for c ascending: sa = sa + ae_c
            sq = sq + qd[:, c]     # sq  = +0.0;  for c ascending: sq = sq + (double)q[i, c]
            if c:
                up = ae[:, c] > fa
                far, fa = np.where(up, e[:, c], far), np.where(up, ae[:, c], fa)
        far = np.where(nan_e.any(1), np.nan, far)
        term = h if w is None else w * h      # term_i = weights ? w_i * h : h
        am, qm = sa / np.float64(C), sq / np.float64(C)      # am = sa / (double)C;  qm = sq / (double)C
    return dict(y=y, e=e, ae=ae, H=H, dH=dH, h=h, term=term, am=am, qm=qm, far=far, w=w, gap=ends(q)["gap"], qd=qd, C=C)


def _finish(p, sum_keys, mx5, mn6, mx7):
    Mf = np.float64(p[sum_keys[0]].shape[0])
    sums = {k: tree_sum(p[k]) for k in sum_keys}
    with np.errstate(all="ignore"):
        # the extrema skip a NaN; an extremum of numbers does not depend on the order of the selects, and a zero leaves as +0.0
        ext = [np.fmax.reduce(mx5.reshape(-1), initial=-np.inf) + 0.0, np.fmin.reduce(mn6.reshape(-1), initial=np.inf) + 0.0,
               np.fmax.reduce(mx7.reshape(-1), initial=-np.inf) + 0.0]
        stats = np.array([sums[k] / Mf for k in sum_keys] + ext, np.float64)
    return np.float64(stats[0]), stats, sums


def q_loss(q, **kw):
    """-> (loss float64, stats float64 [8], td_error float64 [M], the sums in a dict), before the float32 rounding."""
    p = q_rows(q, **kw)
    value, stats, sums = _finish(p, ("term", "am", "qm", "y", "gap"), p["ae"], p["qd"], p["qd"])
    return value, stats, p["far"], sums


def q_loss_f32(q, **kw):
    """-> (loss, stats, td_error) as the device writes them: float32, NaNs canonical."""
    value, stats, far, _ = q_loss(q, **kw)
    return to_f32(np.array([value]))[0], to_f32(stats), to_f32(far)      # td_error[i] = float32(far)


def q_backward(q, grad_loss, **kw):
    """-> grad_q float64 [M, C], before the float32 rounding; grad_loss: the float32 incoming gradient of the loss."""
    p = q_rows(q, **kw)
    with np.errstate(all="ignore"):
        gs = np.float64(np.float32(grad_loss)) / np.float64(p["e"].shape[0])
        return gs * (p["dH"] if p["w"] is None else p["w"][:, None] * p["dH"])      # grad_q[i, c] = float32(gs * (weights ? w_i * dH(e_c) : dH(e_c)))


def pi_rows(log_prob, q, *, alpha, weights=None):
    """The per-row quantities of the actor's rule -> dict."""
    m = ends(q)
    lp, w, al = _f64(log_prob), _f64(weights), np.float64(alpha)
    with np.errstate(all="ignore"):
        qp = np.where(m["bad"], np.nan, m["mn"])      # qp = bad ? NaN : (double)mn
        t = al * lp - qp                              # t  = al * (double)log_prob[i] - qp
        term = t if w is None else w * t              # term_i = weights ? w_i * t : t
        later = np.where(m["jmin"] != 0, 1.0, 0.0)    # later = jmin != 0 ? 1.0 : 0.0
    return dict(lp=lp, qp=qp, term=term, later=later, gap=m["gap"], jmin=m["jmin"], bad=m["bad"], w=w, al=al, C=np.asarray(q).shape[1])


def pi_loss(log_prob, q, **kw):
    """-> (loss float64, stats float64 [8], the sums in a dict), before the float32 rounding."""
    p = pi_rows(log_prob, q, **kw)
    return _finish(p, ("term", "lp", "qp", "gap", "later"), p["lp"], p["qp"], p["qp"])


def pi_loss_f32(log_prob, q, **kw):
    value, stats, _ = pi_loss(log_prob, q, **kw)
    return to_f32(np.array([value]))[0], to_f32(stats)


def pi_backward(log_prob, q, grad_loss, **kw):
    """-> (grad_log_prob float64 [M], grad_q float32-valued float64 [M, C]); grad_loss: the float32 incoming gradient of the loss."""
    p = pi_rows(log_prob, q, **kw)
    M, C, w = p["lp"].shape[0], p["C"], p["w"]
    with np.errstate(all="ignore"):
        gs = np.float64(np.float32(grad_loss)) / np.float64(M)
        g_lp = np.full(M, gs * p["al"]) if w is None else gs * (w * p["al"])      # grad_log_prob[i] = float32(gs * (weights ? w_i * al : al))
        val = -(np.full(M, gs) if w is None else gs * w)
        g_q = np.where(np.arange(C)[None, :] == p["jmin"][:, None], val[:, None], 0.0)      # grad_q[i, c]     = bad ? NaN : (c == jmin ? float32(-(weights ? gs * w_i : gs)) : +0.0)
        g_q = np.where(p["bad"][:, None], np.nan, g_q)
    return g_lp, g_q
