"""NumPy float64 twin of the rule in include/mxv_gae.h: GAE(lambda) advantages and discounted returns-to-go over
[K, N] arrays.  Every operation below is one IEEE float64 operation on whole rows (NumPy neither fuses nor re-associates them), in the
order the rule states; the device must produce the same bits (tests/test_gpu_gae.py), and tests/test_gae_host.py holds this file to
exact rational arithmetic and to an independent scalar loop."""
import numpy as np

CANONICAL_NAN = np.uint32(0x7FC00000)


def to_f32(x):
    """float32(x): round to nearest even, subnormal results kept; every NaN becomes the one pattern 0x7FC00000."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        y = np.asarray(x, dtype=np.float64).astype(np.float32)
    bits = y.view(np.uint32).copy()
    bits[np.isnan(y)] = CANONICAL_NAN
    return bits.view(np.float32)


def _inputs(reward, terminated, truncated, last_value, final_values):
    r = np.asarray(reward)
    assert r.ndim == 2 and r.dtype in (np.float32, np.float64)
    K, N = r.shape
    term = np.asarray(terminated).reshape(K, N) != 0
    trunc = np.asarray(truncated).reshape(K, N) != 0
    lv = np.zeros(N, np.float64) if last_value is None else np.asarray(last_value, np.float32).reshape(N).astype(np.float64)
    fv = None if final_values is None else np.asarray(final_values, np.float32).reshape(K, N).astype(np.float64)
    return r.astype(np.float64), term, trunc, lv, fv, K, N


def _cut(term, trunc, fv, t, N):
    """The bootstrap of a step that ends its episode: 0 where terminated, final_values (or 0) where only truncated."""
    boot = np.zeros(N, np.float64) if fv is None else np.where(trunc[t] & ~term[t], fv[t], 0.0)
    return np.where(term[t], 0.0, boot)


def gae(reward, terminated, truncated, values, last_value=None, *, gamma=0.99, lam=0.95, final_values=None):
    """-> (advantages, returns), float32 [K, N]."""
    r, term, trunc, nv, fv, K, N = _inputs(reward, terminated, truncated, last_value, final_values)
    v = np.asarray(values, np.float32).reshape(K, N).astype(np.float64)
    gamma, c = np.float64(gamma), np.float64(gamma) * np.float64(lam)
    A = np.zeros(N, np.float64)
    adv, ret = np.empty((K, N), np.float32), np.empty((K, N), np.float32)
    with np.errstate(all="ignore"):
        for t in range(K - 1, -1, -1):
            done = term[t] | trunc[t]
            nxt = np.where(done, _cut(term, trunc, fv, t, N), nv)
            delta = (r[t] + gamma * nxt) - v[t]
            A = np.where(done, delta, delta + c * A)
            adv[t] = to_f32(A)
            ret[t] = to_f32(A + v[t])
            nv = v[t]
    return adv, ret


def discounted_returns(reward, terminated, truncated, *, gamma=0.99, last_value=None, final_values=None):
    """-> returns, float32 [K, N]."""
    r, term, trunc, G, fv, K, N = _inputs(reward, terminated, truncated, last_value, final_values)
    gamma = np.float64(gamma)
    ret = np.empty((K, N), np.float32)
    with np.errstate(all="ignore"):
        for t in range(K - 1, -1, -1):
            done = term[t] | trunc[t]
            nxt = np.where(done, _cut(term, trunc, fv, t, N), G)
            G = r[t] + gamma * nxt
            ret[t] = to_f32(G)
    return ret


def bits(x):
    """The uint32 patterns of a float32 array (comparisons that count NaNs and the sign of zero)."""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
