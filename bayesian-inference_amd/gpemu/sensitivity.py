"""Global (variance-based) sensitivity of the emulated observables over a parameter box: first-order and total-effect
Sobol' indices from the device's pick-freeze moments.

Base matrices A, B (n, d) with independent rows in the box; AB_i is A with column i from B.  With z(x) the PC means of
a group and y_f = s_f sum_p c_pf z_p + m_f an observable, the centred estimators (Saltelli et al., Comput. Phys. Commun.
181 (2010) 259 for the first-order index; Jansen, Comput. Phys. Commun. 117 (1999) 35 for the total effect) are

    z0 = mean of z over the 2 n rows of A and B            C   = mean over them of (z - z0)(z - z0)^T
    D_i = z(AB_i) - z(A)                                   M_i = 1/n sum (z(B) - z0) D_i^T,   DD_i = 1/n sum D_i D_i^T
    V_f = s_f^2 c_f^T C c_f       S_if = s_f^2 c_f^T M_i c_f / V_f       T_if = s_f^2 c_f^T DD_i c_f / (2 V_f)

The back-projection is linear, so everything per feature is a k x k quadratic form of moments the device accumulates
(``DeviceModel.sobol_moments``): no n x F array exists.  Standard errors are batch means: the same estimators from each
batch's own moments (its own centre), their sample standard deviation over the T batches divided by sqrt(T).

Second order.  For a pair i < j, AB_ij is A with columns i and j from B and D_ij = z(AB_ij) - z(A);
``DeviceModel.sobol_moments_pairs`` adds sumD2, M2 and D2 per pair, re-centred exactly as M_i and DD_i:

    closed pair index  Sc_ijf = s_f^2 c_f^T M_ij c_f / V_f             (Saltelli et al. 2010, applied to the pair row)
    interaction index  S_ijf  = Sc_ijf - S_if - S_jf
    total of the pair  T_ijf  = s_f^2 c_f^T DD_ij c_f / (2 V_f)        (Jansen 1999)

with batch-means standard errors; the interaction's from the per-batch values of the difference itself.
"""
from __future__ import annotations

import warnings

import numpy as np

MAX_D = 16


def base_samples(n, lo, hi, seed=0, method="sobol"):
    """The base matrices ``(A, B)``, each (n, d), with rows in the box ``[lo, hi]``.

    ``'sobol'``: one scrambled ``scipy.stats.qmc.Sobol`` sequence of dimension 2 d; its first d columns scaled to the
    box are A, its last d are B (two halves of one point set, so A and B are jointly equidistributed).
    ``'random'``: both drawn from ``numpy.random.default_rng(seed)``, A first."""
    lo = np.asarray(lo, dtype=np.float64).reshape(-1)
    hi = np.asarray(hi, dtype=np.float64).reshape(-1)
    n = int(n)
    if n < 1:
        raise ValueError(f"n must be >= 1, got {n}")
    if lo.shape != hi.shape or lo.size < 1:
        raise ValueError(f"lo and hi must be vectors of one length >= 1, got {lo.shape} and {hi.shape}")
    d = lo.size
    if d > MAX_D:
        raise ValueError(f"at most {MAX_D} parameters, got {d}")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
        raise ValueError("the box needs finite lo <= hi")
    if method == "sobol":
        from scipy.stats import qmc
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)     # n need not be a power of two
            u = qmc.Sobol(d=2 * d, scramble=True, seed=seed).random(n)
    elif method == "random":
        u = np.random.default_rng(seed).random((2, n, d)).transpose(1, 0, 2).reshape(n, 2 * d)
    else:
        raise ValueError(f"method must be 'sobol' or 'random', got {method!r}")
    A = lo + (hi - lo) * u[:, :d]
    B = lo + (hi - lo) * u[:, d:]
    return np.ascontiguousarray(A), np.ascontiguousarray(B)


def _quad(X, comp, s2):
    """s_f^2 c_f^T X c_f for every feature: X (..., k, k), comp (k, F) -> (..., F)"""
    return np.einsum("pf,...pq,qf->...f", comp, X, comp) * s2


def _estimates(count, sumA, sumB, C2, sumD, M, D, pivot, comp, scale, smean):
    """(V, V_i, VT_i, mean) per feature from moments about ``pivot`` over ``count`` rows (leading axes broadcast)"""
    n = np.asarray(count, dtype=np.float64)[..., None]
    a = (sumA + sumB) / (2 * n)                                        # z0 - pivot
    C = C2 / (2 * n[..., None]) - a[..., :, None] * a[..., None, :]
    Mi = (M - a[..., None, :, None] * sumD[..., :, None, :]) / n[..., None, None]
    Di = D / n[..., None, None]
    s2 = scale * scale
    V = _quad(C, comp, s2)
    Vi = _quad(Mi, comp, s2)
    VTi = 0.5 * _quad(Di, comp, s2)
    mean = ((pivot + a) @ comp) * scale + smean
    return V, Vi, VTi, mean


def _ratio(num, V):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(V == 0.0, np.nan, num / V)


def indices_from_moments(moments, components, scaler_scale, scaler_mean):
    """The indices of every feature from ``DeviceModel.sobol_moments``' dict: ``first_order``, ``total`` (d, F), their
    batch-means standard errors ``first_order_se``, ``total_se`` (d, F; NaN for one batch), ``variance`` and ``mean``
    (F,) of the emulated observable over the 2 n base rows, ``n`` and ``n_batches``.  A feature of zero variance has
    NaN indices; nothing is clipped."""
    comp = np.asarray(components, dtype=np.float64)
    scale = np.asarray(scaler_scale, dtype=np.float64)
    smean = np.asarray(scaler_mean, dtype=np.float64)
    m = {key: np.asarray(moments[key], dtype=np.float64) for key in ("sumA", "sumB", "C2", "sumD", "M", "D", "pivot")}
    count = np.asarray(moments["count"], dtype=np.int64)
    T = count.size
    tot = lambda key: m[key].sum(axis=0)
    V, Vi, VTi, mean = _estimates(count.sum(), tot("sumA"), tot("sumB"), tot("C2"), tot("sumD"), tot("M"), tot("D"),
                                  m["pivot"], comp, scale, smean)
    out = {"first_order": _ratio(Vi, V), "total": _ratio(VTi, V), "variance": V, "mean": mean,
           "n": int(count.sum()), "n_batches": int(T)}
    if T > 1:
        Vb, Vib, VTib, _ = _estimates(count, m["sumA"], m["sumB"], m["C2"], m["sumD"], m["M"], m["D"], m["pivot"], comp,
                                      scale, smean)
        with np.errstate(invalid="ignore"):
            out["first_order_se"] = np.std(_ratio(Vib, Vb[:, None, :]), axis=0, ddof=1) / np.sqrt(T)
            out["total_se"] = np.std(_ratio(VTib, Vb[:, None, :]), axis=0, ddof=1) / np.sqrt(T)
    else:
        out["first_order_se"] = np.full_like(out["first_order"], np.nan)
        out["total_se"] = np.full_like(out["total"], np.nan)
    return out


def check_pairs(pairs, d):
    """``pairs`` as a (P, 2) int64 array of distinct i < j < d; None: all of them (``gpemu.marginals.pair_indices``)."""
    d = int(d)
    if d < 2:
        raise ValueError(f"a pair needs d >= 2 parameters, got {d}")
    if pairs is None:
        from .marginals import pair_indices
        return pair_indices(d)
    raw = np.asarray(pairs)
    if raw.ndim != 2 or raw.shape[1] != 2 or raw.shape[0] < 1:
        raise ValueError(f"pairs must have shape (P, 2) with P >= 1, got {raw.shape}")
    out = raw.astype(np.int64)
    if not np.array_equal(out, raw):
        raise ValueError("pairs must be integers")
    if out.min() < 0 or out.max() >= d:
        raise ValueError(f"a pair's index is outside 0 .. {d - 1}")
    if not np.all(out[:, 0] < out[:, 1]):
        raise ValueError("every pair must be given as i < j")
    if len({(int(i), int(j)) for i, j in out}) != out.shape[0]:
        raise ValueError("a pair is repeated")
    return np.ascontiguousarray(out)


def _se(values, T):
    """batch-means standard error of per-batch ``values`` (T, ...)"""
    with np.errstate(invalid="ignore"):
        return np.std(values, axis=0, ddof=1) / np.sqrt(T)


def pair_indices_from_moments(moments, components, scaler_scale, scaler_mean):
    """The second-order indices of every feature from ``DeviceModel.sobol_moments_pairs``' dict: ``closed_pair`` (the
    share of the variance that parameters i and j explain together), ``interaction`` (= closed_pair - S_i - S_j: what
    they explain only jointly) and ``total_pair`` (the share that involves i or j at all), each (P, F) in the order of
    ``pairs`` (P, 2), and their batch-means standard errors ``closed_pair_se``, ``interaction_se`` (from the
    per-batch values of the difference itself), ``total_pair_se`` (NaN for one batch).  A feature of zero variance has
    NaN indices; nothing is clipped.  The quadratic forms are evaluated as matrix products here (at P (d - 1) / 2 pairs
    they are most of the call's host time), so S_i inside ``interaction`` equals ``first_order`` to rounding, not to
    the bit."""
    comp = np.asarray(components, dtype=np.float64)
    scale = np.asarray(scaler_scale, dtype=np.float64)
    smean = np.asarray(scaler_mean, dtype=np.float64)
    m = {key: np.asarray(moments[key], dtype=np.float64)
         for key in ("sumA", "sumB", "C2", "sumD", "M", "D", "sumD2", "M2", "D2", "pivot")}
    pairs = np.asarray(moments["pairs"], dtype=np.int64).reshape(-1, 2)
    count = np.asarray(moments["count"], dtype=np.int64)
    T = count.size
    pi, pj = pairs[:, 0], pairs[:, 1]

    s2 = scale * scale

    def quad(X):
        """``_quad`` as a matrix product (X c_f first): the same forms, another summation order"""
        return (comp * (X @ comp)).sum(axis=-2) * s2

    def est(cnt, get):
        n = np.asarray(cnt, dtype=np.float64)[..., None]
        a = (get("sumA") + get("sumB")) / (2 * n)                      # z0 - pivot
        V = quad(get("C2") / (2 * n[..., None]) - a[..., :, None] * a[..., None, :])[..., None, :]
        recentred = lambda M, sD: (M - a[..., None, :, None] * sD[..., :, None, :]) / n[..., None, None]
        S = _ratio(quad(recentred(get("M"), get("sumD"))), V)
        closed = _ratio(quad(recentred(get("M2"), get("sumD2"))), V)
        total = _ratio(0.5 * quad(get("D2") / n[..., None, None]), V)
        return closed, closed - S[..., pi, :] - S[..., pj, :], total

    closed, inter, total = est(count.sum(), lambda key: m[key].sum(axis=0))
    out = {"pairs": pairs, "closed_pair": closed, "interaction": inter, "total_pair": total}
    if T > 1:
        cb, ib, tb = est(count, lambda key: m[key])
        out["closed_pair_se"], out["interaction_se"], out["total_pair_se"] = _se(cb, T), _se(ib, T), _se(tb, T)
    else:
        for key in ("closed_pair", "interaction", "total_pair"):
            out[key + "_se"] = np.full_like(out[key], np.nan)
    return out


def interacting_pairs(result, n_sigma=3):
    """The pairs (P, 2), in the order of ``gpemu.marginals.pair_indices``, among the parameters that act through
    interactions: those whose ``total - first_order`` exceeds ``n_sigma`` of its error in at least one feature -- the
    pairs worth asking ``sobol_indices(second_order=True, pairs=...)`` for, instead of all d (d - 1) / 2.  ``result`` is
    a first-order result (``sobol_indices`` or ``global_sensitivity``); the error of the difference is taken as
    ``total_se + first_order_se``, which bounds the batch-means error of the difference from above (the standard
    deviation of a difference is at most the sum of the two), so nothing is flagged that the difference's own error
    would not flag.  NaN entries (zero variance, one batch) flag nothing.  Pure host code."""
    S, Tt = np.asarray(result["first_order"], dtype=np.float64), np.asarray(result["total"], dtype=np.float64)
    se = np.asarray(result["first_order_se"], dtype=np.float64) + np.asarray(result["total_se"], dtype=np.float64)
    if not float(n_sigma) >= 0:
        raise ValueError(f"n_sigma must be >= 0, got {n_sigma}")
    with np.errstate(invalid="ignore"):
        acts = np.any((Tt - S) > float(n_sigma) * se, axis=1)
    idx = np.flatnonzero(acts)
    return np.array([(i, j) for a, i in enumerate(idx) for j in idx[a + 1:]], dtype=np.int64).reshape(-1, 2)


def sobol_indices(model_or_models, A, B, n_batches=16, workspace_bytes=0, second_order=False, pairs=None):
    """``DeviceModel.sobol_indices`` of one model, or of every model of a dict (one result per key), on the shared
    base matrices ``A``, ``B``; ``second_order`` and ``pairs`` as there."""
    kw = dict(n_batches=n_batches, workspace_bytes=workspace_bytes)
    if second_order or pairs is not None:
        kw.update(second_order=second_order, pairs=pairs)
    if isinstance(model_or_models, dict):
        return {name: dm.sobol_indices(A, B, **kw) for name, dm in model_or_models.items()}
    return model_or_models.sobol_indices(A, B, **kw)


SOBOL_PATHS = ("call", "chunk", "whole", "dp8", "dp16", "kind0", "kind1", "kind2", "kind3", "kind4")   # enum gpemu_sobol_path


def sobol_path_counts():
    """Counters of enum gpemu_sobol_path, as an int64 array."""
    import ctypes as C

    from . import _lib
    out = np.zeros(16, dtype=np.int64)
    n = _lib.lib().gpemu_sobol_path_counts(out.ctypes.data_as(C.POINTER(C.c_int64)), out.size)
    return out[:n].copy()


def sobol_workspace_bytes(rows, d, k):
    """``workspace_bytes`` with which ``sobol_moments`` holds the PC means of ``rows`` base rows at a time: 8 (d + 2) k
    bytes per row (include/gpemu.h).  Chunks are whole slices of at most 256 rows."""
    return 8 * int(rows) * (int(d) + 2) * int(k)


SOBOL_PAIRS_PATHS = SOBOL_PATHS                                      # enum gpemu_sobol_pairs_path: the same names


def sobol_pairs_path_counts():
    """Counters of enum gpemu_sobol_pairs_path (``DeviceModel.sobol_moments_pairs``), as an int64 array."""
    import ctypes as C

    from . import _lib
    out = np.zeros(16, dtype=np.int64)
    n = _lib.lib().gpemu_sobol_pairs_path_counts(out.ctypes.data_as(C.POINTER(C.c_int64)), out.size)
    return out[:n].copy()


def sobol_pairs_workspace_bytes(rows, d, k, n_pairs):
    """``workspace_bytes`` with which ``sobol_moments_pairs`` holds the PC means of ``rows`` base rows at a time:
    8 (d + 2 + n_pairs) k bytes per row (include/gpemu.h).  Chunks are whole slices of at most 256 rows."""
    return 8 * int(rows) * (int(d) + 2 + int(n_pairs)) * int(k)
