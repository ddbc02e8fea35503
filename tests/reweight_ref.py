"""NumPy / Python-int reference of the reweighting definitions, given the fixed-point weights q.

Every weight is an integer and every row sum Q is below 2^53, so the cumulative sums are exact as Python ints (object
dtype) and np.histogram(weights=q.astype(float64)) adds exact integers in float64: both are exact references."""
import math
from fractions import Fraction

import numpy as np

ONE = 1 << 52


def quantise(lw):
    """q = rint(exp(lw) 2^52) from an extended-precision exp: what the device may miss by one unit"""
    e = np.exp(np.asarray(lw, dtype=np.longdouble)) * np.longdouble(ONE)
    return np.rint(e).astype(np.uint64)


def target(p, Q):
    return max(1, math.ceil(Fraction(float(p)) * int(Q)))


def weighted_select(x, q, t):
    """the smallest element v of x with sum_{x_s <= v} q_s >= t; NaN where t exceeds the total weight"""
    x, q = np.asarray(x, dtype=np.float64), np.asarray(q, dtype=np.uint64)
    order = np.argsort(x, kind="stable")
    xs = x[order]
    cum = np.cumsum(q[order].astype(object))
    # ties: the cumulative weight AT a value is that of its last copy
    last = np.append(xs[1:] != xs[:-1], True)
    for i in np.nonzero(last)[0]:
        if cum[i] >= int(t):
            return xs[i]
    return np.nan


def weighted_select_fast(x, q, targets):
    """weighted_select for many targets: searchsorted on the exact cumulative weights (float64 holds them: Q < 2^53)"""
    x, q = np.asarray(x, dtype=np.float64), np.asarray(q, dtype=np.uint64)
    order = np.argsort(x, kind="stable")
    xs = x[order]
    cum = np.cumsum(q[order], dtype=np.uint64)
    last = np.append(xs[1:] != xs[:-1], True)
    vals, cw = xs[last], cum[last]
    idx = np.searchsorted(cw, np.asarray(targets, dtype=np.uint64), side="left")
    out = np.full(len(targets), np.nan)
    ok = idx < vals.size
    out[ok] = vals[idx[ok]]
    return out


def weighted_quantile(x, q, probabilities):
    """(nq,) for one column x (S,) and one weight row q (S,)"""
    Q = int(np.sum(np.asarray(q, dtype=np.uint64).astype(object)))
    return weighted_select_fast(x, q, [target(p, Q) for p in np.atleast_1d(probabilities)])


def hist_ref(x, q, e1, e2):
    """(hist1 (d, nb1), hist2 (n_pairs, nb2, nb2), w_inside (d,)) as uint64 for one weight row"""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(q, dtype=np.uint64).astype(np.float64)
    d = x.shape[1]
    h1 = np.stack([np.histogram(x[:, j], bins=e1[j], weights=w)[0] for j in range(d)])
    pairs = [(i, j) for i in range(d) for j in range(i + 1, d)]
    nb2 = e2.shape[1] - 1
    h2 = np.zeros((len(pairs), nb2, nb2))
    for p, (i, j) in enumerate(pairs):
        h2[p] = np.histogram2d(x[:, i], x[:, j], bins=[e2[i], e2[j]], weights=w)[0]
    assert np.all(h1 == np.rint(h1)) and np.all(h2 == np.rint(h2))
    h1 = h1.astype(np.uint64)
    return h1, h2.astype(np.uint64), h1.sum(axis=1, dtype=np.uint64)


def log_prior(x, kind, a, b):
    """(L (R, S), A (R, S) = sum_i |f_i|) in np.longdouble"""
    x = np.asarray(x, dtype=np.longdouble)
    R, d = kind.shape
    L = np.zeros((R, x.shape[0]), dtype=np.longdouble)
    A = np.zeros_like(L)
    for r in range(R):
        for i in range(d):
            k, ai, bi = int(kind[r, i]), np.longdouble(a[r, i]), np.longdouble(b[r, i])
            if k == 0:
                continue
            if k == 1:
                f = -np.log(x[:, i])
            elif k == 2:
                f = -(x[:, i] - ai) ** 2 / (2 * bi * bi)
            else:
                lx = np.log(x[:, i])
                f = -lx - (lx - ai) ** 2 / (2 * bi * bi)
            L[r] += f
            A[r] += np.abs(f)
    return L, A


def moments(x, q):
    """weighted mean and variance (divisor Q) of the columns of x under the integer weights q, in longdouble"""
    w = np.asarray(q, dtype=np.uint64).astype(np.longdouble)
    x = np.asarray(x, dtype=np.longdouble)
    m = (w[:, None] * x).sum(0) / w.sum()
    v = (w[:, None] * (x - m) ** 2).sum(0) / w.sum()
    return m.astype(np.float64), v.astype(np.float64)
