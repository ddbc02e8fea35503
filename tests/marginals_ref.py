"""numpy references of the marginal summaries (gpemu.marginals), shared by the host and the GPU tests."""
import math

import numpy as np

KD_CHUNK = 8192      # samples per partial sum of the density kernel (csrc/k_marginal.hip)


def hist_ref(x, edges1, edges2):
    """``(hist_1d, hist_2d, n_inside)`` by np.histogram / np.histogram2d on the given edges, as int64."""
    S, d = x.shape
    h1 = np.stack([np.histogram(x[:, j], bins=edges1[j])[0] for j in range(d)]).astype(np.int64)
    pairs = [(i, j) for i in range(d) for j in range(i + 1, d)]
    nb2 = edges2.shape[1] - 1
    h2 = np.zeros((len(pairs), nb2, nb2), dtype=np.int64)
    for p, (i, j) in enumerate(pairs):
        h2[p] = np.histogram2d(x[:, i], x[:, j], bins=[edges2[i], edges2[j]])[0].astype(np.int64)
    return h1, h2, h1.sum(axis=1)


def hpd_ref(x, n_out):
    """The narrowest-window rule restated: with s the sorted sample, the window i in [0, n_out) that minimises
    s[S - n_out + i] - s[i], the smallest such i; ``(s[i], s[S - n_out + i])``.  NaN for a sample with a NaN or an
    infinite extreme (the library's convention)."""
    x = np.asarray(x, dtype=np.float64)
    S = x.size
    if np.any(np.isnan(x)) or np.isinf(x.min()) or np.isinf(x.max()):
        return np.nan, np.nan
    s = np.sort(x)
    with np.errstate(over="ignore"):
        width = s[S - n_out:] - s[:n_out]
    i = int(np.argmin(width))
    return s[i], s[S - n_out + i]


def kde_ref(x, grid, h, dtype=np.longdouble):
    """The direct sum 1 / (S h sqrt(2 pi)) sum_j exp(-(g - x_j)^2 / (2 h^2)) in ``dtype`` for every grid point."""
    x = np.asarray(x, dtype=dtype)
    g = np.asarray(grid, dtype=dtype)
    h = dtype(h)
    out = np.empty(g.shape, dtype=dtype)
    two = dtype(2)
    block = max(1, (1 << 20) // x.size)      # grid points at a time
    for a in range(0, g.size, block):
        u = (g[a:a + block, None] - x[None, :]) / h
        out[a:a + block] = np.exp(-(u * u) / two).sum(axis=1)
    pi = np.arctan(dtype(1)) * dtype(4)
    return out / (dtype(x.size) * h * np.sqrt(two * pi))


def kde_bound_factor(S):
    """c of |got - ref| <= c eps (ref + 1 / (sqrt(2 pi) h)), eps = 2^-52, from the density kernel's operations (the
    derivation is in tests/test_gpu_marginals.py: test_kde_within_the_error_bound)."""
    nchunk = -(-S // KD_CHUNK)
    depth = -(-min(S, KD_CHUNK) // 4) + 2 + -(-nchunk // 256) + 6 + 3
    return 0.55 * (depth + 8)


def kde_tolerance(S, h, ref):
    eps = np.finfo(np.float64).eps
    return kde_bound_factor(S) * eps * (np.asarray(ref, dtype=np.longdouble) + 1.0 / (math.sqrt(2.0 * math.pi) * h))
