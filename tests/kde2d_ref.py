"""Reference of the 2-D kernel densities (gpemu.marginals.kde_2d): the sheared product sum in
np.longdouble, and the error bound of the device kernel from its own operations."""
import math

import numpy as np

K2_CHUNK = 8192        # samples per partial tile of csrc/k_kde2d.hip


def kde2d_ref(x, y, shear, h_a, h_b, grid_a, grid_b, dtype=np.longdouble, block=2048):
    """``Z[a][b] = 1 / (S 2 pi h_a h_b) sum_s exp(-((g_a[a] - x_s) / h_a)^2 / 2) exp(-((g_b[b] - v_s) / h_b)^2 / 2)``,
    ``v_s = y_s - shear x_s``, every operation in ``dtype``: the density of the pair (x, y) at the points
    ``(g_a[a], g_b[b] + shear g_a[a])``."""
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    ga, gb = np.asarray(grid_a, dtype=dtype), np.asarray(grid_b, dtype=dtype)
    beta, ha, hb, two = dtype(shear), dtype(h_a), dtype(h_b), dtype(2)
    v = y - beta * x
    out = np.zeros((ga.size, gb.size), dtype=dtype)
    for s0 in range(0, x.size, block):
        ta = (ga[:, None] - x[None, s0:s0 + block]) / ha
        tb = (gb[:, None] - v[None, s0:s0 + block]) / hb
        out += np.exp(-(ta * ta) / two) @ np.exp(-(tb * tb) / two).T
    pi = np.arctan(dtype(1)) * dtype(4)
    return out / (dtype(x.size) * two * pi * ha * hb)


def kde2d_bound_factor(S):
    """c of |got - ref| <= c eps (ref + 1 / (2 pi h_a h_b)) + DBL_MIN / (2 pi h_a h_b), eps = 2^-52 (the derivation is
    in tests/test_gpu_kde2d.py: test_kde2d_within_the_error_bound)."""
    nchunk = -(-S // K2_CHUNK)
    depth = min(S, K2_CHUNK) + nchunk
    c = 0.55 * (depth + 11)
    assert c <= 0.55 * (S + 16)        # what any summation order of S positive terms needs
    return c


def kde2d_tolerance(S, h_a, h_b, ref):
    eps, tiny = np.finfo(np.float64).eps, np.finfo(np.float64).tiny
    peak = 1.0 / (2.0 * math.pi * h_a * h_b)
    return kde2d_bound_factor(S) * eps * (np.asarray(ref, dtype=np.longdouble) + peak) + S * tiny * peak / S


def correlated_pair(S, rho=0.9, scales=(2.0, 0.01), seed=0, mean=(0.3, -0.2)):
    """``(S, 2)`` normal samples with correlation rho and the given scales."""
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(S, 2))
    x = z[:, 0]
    y = rho * z[:, 0] + math.sqrt(1.0 - rho * rho) * z[:, 1]
    return np.stack([mean[0] + scales[0] * x, mean[1] + scales[1] * y], axis=1)
