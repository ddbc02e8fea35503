"""numpy reference of gpemu.information: the unit-box rows, brute-force squared distances with the
per-coordinate differences in float64 accumulated in np.longdouble, the zero-distance rule, the k-th distance, the sums,
the Kozachenko-Leonenko and Wang-Kulkarni-Verdu estimators and the drop-in's settings.  Nothing here calls the library."""
import math

import numpy as np
from scipy.special import digamma, gammaln

LD = np.longdouble


def pair_indices(d):
    return [(i, j) for i in range(d) for j in range(i + 1, d)]


def default_subsets(d):
    return [(j,) for j in range(d)] + pair_indices(d) + ([tuple(range(d))] if d > 2 else [])


def selected_rows(S, max_points):
    n = min(int(S), int(max_points))
    return np.array([(i * int(S)) // n for i in range(n)], dtype=np.int64)


def unit_rows(x, lower, upper, max_points=None):
    """``(u, n_skipped)``: ``(x - lo) * (1 / (hi - lo))``, two roundings per coordinate; a row with a non-finite
    coordinate becomes a row of NaN and is counted."""
    x = np.asarray(x, dtype=np.float64)
    if max_points is not None:
        x = x[selected_rows(x.shape[0], max_points)]
    lo, hi = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    iw = 1.0 / (hi - lo)
    u = (x - lo[None, :]) * iw[None, :]
    bad = ~np.isfinite(x).all(axis=1)
    u[bad] = np.nan
    return u, int(bad.sum())


def sq_distances(uq, ur, cols):
    """``(nq, nr)`` longdouble: float64 differences, squared and added in longdouble"""
    out = np.zeros((uq.shape[0], ur.shape[0]), dtype=LD)
    for j in cols:
        diff = uq[:, j][:, None] - ur[:, j][None, :]          # float64: one rounding per difference
        out += diff.astype(LD) ** 2
    return out


def knn(uq, ur, k, subsets):
    """``(r2 (P, nq) longdouble, zeros (P, nq) int64)`` under the zero-distance rule: a reference at squared distance
    exactly 0 is a copy -- counted, no neighbour; fewer than k others: +inf; a non-finite reference is passed over, a
    non-finite query gives NaN and 0."""
    uq = np.asarray(uq, dtype=np.float64)
    ur = uq if ur is None else np.asarray(ur, dtype=np.float64)
    P, nq = len(subsets), uq.shape[0]
    r2, zeros = np.full((P, nq), np.inf, dtype=LD), np.zeros((P, nq), dtype=np.int64)
    for p, cols in enumerate(subsets):
        cols = sorted(cols)
        refs = ur[np.isfinite(ur[:, cols]).all(axis=1)]
        q_ok = np.isfinite(uq[:, cols]).all(axis=1)
        r2[p, ~q_ok] = np.nan
        for i0 in range(0, nq, 512):                              # queries in chunks: the matrix stays small
            rows = np.arange(i0, min(nq, i0 + 512))[q_ok[i0:i0 + 512]]
            if rows.size == 0 or refs.shape[0] == 0:
                continue
            D = sq_distances(uq[rows], refs, cols)
            copy = D == 0
            zeros[p, rows] = copy.sum(axis=1)
            D[copy] = np.inf
            if refs.shape[0] >= k:
                r2[p, rows] = np.partition(D, k - 1, axis=1)[:, k - 1]
    return r2, zeros


def log_sums(r2, zeros=None, nu2=None):
    """``(counts (P, 3): n_used, n_short, copies; sums (P, 2) longdouble; abs (P,): sum |log r2| (+ |log nu2|))``"""
    P = r2.shape[0]
    counts, sums, sabs = np.zeros((P, 3), dtype=np.int64), np.zeros((P, 2), dtype=LD), np.zeros(P, dtype=LD)
    for p in range(P):
        a = r2[p]
        c = np.ones_like(a) if nu2 is None else nu2[p]
        nan = np.isnan(a) | np.isnan(c)
        short = ~nan & (np.isinf(a) | np.isinf(c))
        used = ~nan & ~short
        la = np.log(a[used].astype(LD))
        v = la if nu2 is None else np.log(c[used].astype(LD)) - la
        counts[p] = (used.sum(), short.sum(), 0 if zeros is None else zeros[p].sum())
        sums[p] = (v.sum(), (v * v).sum())
        sabs[p] = np.abs(la).sum() + (0 if nu2 is None else np.abs(np.log(c[used].astype(LD))).sum())
    return counts, sums, sabs


def log_unit_ball(d):
    return 0.5 * d * math.log(math.pi) - float(gammaln(0.5 * d + 1.0))


def _moments(counts, sums):
    n = counts[:, 0].astype(np.float64)
    mean = (sums[:, 0] / n).astype(np.float64)
    var = np.where(n > 1, ((sums[:, 1] - n * (sums[:, 0] / n) ** 2) / np.maximum(n - 1, 1)).astype(np.float64), 0.0)
    return mean, np.sqrt(np.maximum(var, 0.0) / n)


def entropy_from(r2, subsets, k, n_points):
    """Kozachenko-Leonenko from the k-th squared distances: ``(H (P,), se (P,))``"""
    counts, sums, _ = log_sums(r2)
    mean, sem = _moments(counts, sums)
    dims = np.array([len(s) for s in subsets], dtype=np.float64)
    lc = np.array([log_unit_ball(len(s)) for s in subsets])
    return float(digamma(n_points)) - float(digamma(k)) + lc + 0.5 * dims * mean, 0.5 * dims * sem


def information_gain(x, lower, upper, k=4, subsets=None, max_points=65536):
    u, skipped = unit_rows(x, lower, upper, max_points)
    subsets = default_subsets(u.shape[1]) if subsets is None else [tuple(sorted(s)) for s in subsets]
    r2, zeros = knn(u, None, k, subsets)
    n = u.shape[0] - skipped
    H, se = entropy_from(r2, subsets, k, n)
    return {"subsets": subsets, "nats": -H, "se": se, "n_points": n, "copies": zeros.sum(axis=1) - n, "r2": r2,
            "zeros": zeros}


def divergence_from(rho2, nu2, subsets, n, m):
    counts, sums, _ = log_sums(rho2, None, nu2)
    mean, sem = _moments(counts, sums)
    dims = np.array([len(s) for s in subsets], dtype=np.float64)
    return 0.5 * dims * mean + math.log(m / (n - 1.0)), 0.5 * dims * sem


def kl_divergence(x, y, lower, upper, k=4, subsets=None, max_points=65536):
    ux, sx = unit_rows(x, lower, upper, max_points)
    uy, sy = unit_rows(y, lower, upper, max_points)
    subsets = default_subsets(ux.shape[1]) if subsets is None else [tuple(sorted(s)) for s in subsets]
    rho2, _ = knn(ux, None, k, subsets)
    nu2, _ = knn(ux, uy, k, subsets)
    nats, se = divergence_from(rho2, nu2, subsets, ux.shape[0] - sx, uy.shape[0] - sy)
    return {"subsets": subsets, "nats": nats, "se": se, "rho2": rho2, "nu2": nu2}


# -- the k-th distances of copy-free data by a tree (what the host tests check the brute force against) -------------
def tree_kth_sq(uq, ur, k, cols):
    from scipy.spatial import cKDTree
    cols = sorted(cols)
    if ur is None:
        dist, _ = cKDTree(uq[:, cols]).query(uq[:, cols], k=k + 1)
        return dist[:, k] ** 2
    dist, _ = cKDTree(ur[:, cols]).query(uq[:, cols], k=k)
    return (dist if k == 1 else dist[:, k - 1]) ** 2


def tree_information_gain(x, k=4):
    """(estimate, se) of the joint gain of rows inside the unit box, the neighbours by scipy's tree"""
    n, d = x.shape
    r2 = tree_kth_sq(x, None, k, range(d))[None, :]
    H, se = entropy_from(r2.astype(LD), [tuple(range(d))], k, n)
    return -float(H[0]), float(se[0])


def tree_kl_divergence(x, y, k=4):
    n, d = x.shape
    rho2 = tree_kth_sq(x, None, k, range(d))[None, :].astype(LD)
    nu2 = tree_kth_sq(x, y, k, range(d))[None, :].astype(LD)
    nats, se = divergence_from(rho2, nu2, [tuple(range(d))], n, y.shape[0])
    return float(nats[0]), float(se[0])


def gaussian_gain(d, sigma):
    """the information gain of N(mu, sigma^2 I) inside the unit box over the uniform prior (no mass outside)"""
    return -0.5 * d * math.log(2.0 * math.pi * math.e * sigma * sigma)


def gaussian_kl(d, s0, s1, shift):
    """KL(N(mu0, s0^2 I) || N(mu1, s1^2 I)), |mu0 - mu1|^2 = d shift^2"""
    return d * (math.log(s1 / s0) + (s0 * s0 + shift * shift) / (2.0 * s1 * s1) - 0.5)
