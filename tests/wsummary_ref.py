"""NumPy / Python-int references of the weighted bands, intervals and densities, given the fixed-point
weights q.  No device code.

Every weight is an integer and every row sum Q is below 2^53: the cumulative weights are exact as Python ints, so the
interval reference is the definition itself; moments and densities are np.longdouble sums."""
import bisect
import math

import numpy as np

import reweight_ref as RR

WS_SUM = 4096          # samples per partial sum of the weighted row reduction (csrc/rows_dev.h)
U = 2.0 ** -53


# ---- highest-density intervals ---------------------------------------------------------------------------------------
def _distinct(x, q):
    """the distinct values of x, ascending (a zero as +0), and the exact cumulative weight at each as Python ints"""
    x = np.asarray(x, dtype=np.float64) + 0.0
    order = np.argsort(x, kind="stable")
    xs, qs = x[order], [int(v) for v in np.asarray(q, dtype=np.uint64)[order]]
    vals, cum, run = [], [], 0
    for i, v in enumerate(xs):
        run += qs[i]
        if i + 1 == len(xs) or xs[i + 1] != v:
            vals.append(float(v))
            cum.append(run)
    return vals, cum


def hpd(x, q, t):
    """The definition: over every sample value a, with b(a) the smallest sample value >= a whose closed interval [a, b]
    holds weight >= t, the (a, b(a)) of the smallest double width b - a, equal widths to the smaller a.  (NaN, NaN) where
    t exceeds the total weight, for a sample with a NaN and for one with an infinite extreme."""
    x = np.asarray(x, dtype=np.float64)
    if np.any(np.isnan(x)) or np.isinf(x.min()) or np.isinf(x.max()):
        return np.nan, np.nan
    vals, cum = _distinct(x, q)
    best = None
    for i, a in enumerate(vals):
        need = (cum[i - 1] if i else 0) + int(t)
        j = bisect.bisect_left(cum, need, i)
        if j == len(vals):
            break                      # later starts hold less
        w = vals[j] - a
        if best is None or w < best[0]:
            best = (w, a, vals[j])
    return (np.nan, np.nan) if best is None else (best[1], best[2])


def hpd_brute(x, q, t):
    """the same by brute force over all pairs of sample values"""
    x = np.asarray(x, dtype=np.float64) + 0.0
    if np.any(np.isnan(x)) or np.isinf(x.min()) or np.isinf(x.max()):
        return np.nan, np.nan
    qs = [int(v) for v in np.asarray(q, dtype=np.uint64)]
    vals = sorted(set(float(v) for v in x))
    best = None
    for a in vals:
        for b in vals:
            if b < a:
                continue
            if sum(w for v, w in zip(x, qs) if a <= v <= b) >= int(t):
                if best is None or (b - a) < best[0]:
                    best = (b - a, a, b)
                break                  # b(a) is the smallest such b
    return (np.nan, np.nan) if best is None else (best[1], best[2])


# ---- densities -------------------------------------------------------------------------------------------------------
def kde(x, q, grid, h, dtype=np.longdouble):
    """1 / (Q h sqrt(2 pi)) sum_s q_s exp(-(g - x_s)^2 / (2 h^2)) in ``dtype`` for every grid point"""
    x, g = np.asarray(x, dtype=dtype), np.asarray(grid, dtype=dtype)
    w = np.asarray(q, dtype=np.uint64).astype(dtype)
    h = dtype(h)
    out = np.empty(g.shape, dtype=dtype)
    block = max(1, (1 << 20) // x.size)
    for g0 in range(0, g.size, block):
        u = (g[g0:g0 + block, None] - x[None, :]) / h
        out[g0:g0 + block] = (w[None, :] * np.exp(-(u * u) / dtype(2))).sum(axis=1)
    return out / (w.sum() * h * np.sqrt(dtype(2) * dtype(np.pi)))


def scipy_bandwidth(x, w):
    """what scipy.stats.gaussian_kde(x, weights=w) uses as the kernel's standard deviation"""
    from scipy.stats import gaussian_kde
    k = gaussian_kde(x, weights=w)
    return float(np.sqrt(k.covariance[0, 0]))


# ---- weighted sums of rows -------------------------------------------------------------------------------------------
def tree_depth(S):
    """D: the additions on the longest path of the weighted row reduction's tree (csrc/k_wsummary.hip): a lane's 16 terms
    (one fused multiply-add each), 6 levels of the wave butterfly, 3 additions over the 4 waves, and the chunks in order"""
    return 16 + 6 + 3 + -(-int(S) // WS_SUM)


def weighted_sums(x, q):
    """(mean, sum q |x| / Q) of the columns of x (S, F) under q (S,), in longdouble"""
    w = np.asarray(q, dtype=np.uint64).astype(np.longdouble)
    x = np.asarray(x, dtype=np.longdouble)
    Q = w.sum()
    return (w[:, None] * x).sum(0) / Q, (w[:, None] * np.abs(x)).sum(0) / Q


def weighted_quantiles(x, q, probabilities):
    """(nq, F): reweight_ref.weighted_quantile of every column"""
    return np.stack([RR.weighted_quantile(x[:, f], q, probabilities) for f in range(x.shape[1])], axis=1)
