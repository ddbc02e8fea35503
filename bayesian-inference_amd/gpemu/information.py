"""Information gain and Kullback-Leibler divergence of chains by k-th nearest neighbours on the device.

How many nats did the data teach about each parameter, about each pair and about all of them jointly, and how far apart
are two posteriors -- what the reference leaves open twice as "some type of information gain metric, e.g. KL divergence"
(ref: plot_qhat.py:116, plot_analyses.py:144):

* ``information_gain``: ``KL(posterior || prior)`` under the uniform prior on the box.  KL is invariant under
  reparametrisation, so in unit-box coordinates ``u = (x - lower) / (upper - lower)`` it is minus the differential entropy
  of ``u``, estimated by Kozachenko and Leonenko's k-th neighbour estimator (``entropy``);
* ``kl_divergence``: ``D(P || Q)`` between two samples (Wang, Kulkarni, Verdu 2009; Perez-Cruz 2008) -- two
  parameterisations, two closure chains, the stretch chain against the HMC chain, or a derived quantity against samples
  of its prior as 1-column arrays;
* ``knn_distances``: the squared distances to the k-th neighbour that both are made of.

Zero-distance rule: a reference at squared distance exactly 0 is a copy of the query, not a neighbour.  That excludes the
query itself in a self search and the repeated states of an ensemble chain (a rejected move keeps the walker where it
was); the copies are counted.  A chain with many of them should be thinned by its autocorrelation time first.

Subsets of the coordinates are tuples of indices; ``default_subsets(d)`` is every parameter, every pair and the joint.
Rows are ``(n, d)``: numpy arrays go through the host entry, contiguous float64 device tensors are read in place.
There is no CPU implementation."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check, ptr
from .rows import DeviceRows

PATHS = ("UNIT_ROWS", "SEARCH", "MERGE", "SUBSET_BATCH", "LOGSUM")
MAX_D = 16
MAX_K = 16
REF_TILE = 256            # GPEMU_KNN_REF_TILE: references in LDS at a time
MAX_COPIES = 0.1          # the largest share of copies the estimators are used at: a condition of use, not a measurement
LOG2 = math.log(2.0)


def path_counts():
    """The library's counters of these launches since the process started, by name."""
    out = (C.c_int64 * len(PATHS))()
    n = _lib.lib().gpemu_knn_path_counts(out, len(PATHS))
    if n < 0:
        check(n)
    return {k: int(out[i]) for i, k in enumerate(PATHS)}


# -- host-side rules --------------------------------------------------------------------------------------------------
def default_subsets(d):
    """Every parameter ``(j,)``, every pair ``(i, j)`` in ``marginals.pair_indices`` order and, for ``d > 2``, the joint
    ``(0, ..., d - 1)``: a list of tuples."""
    from .marginals import pair_indices
    d = int(d)
    if not 1 <= d <= MAX_D:
        raise ValueError(f"d must be in [1, {MAX_D}], got {d}")
    out = [(j,) for j in range(d)] + [(int(i), int(j)) for i, j in pair_indices(d)]
    return out + ([tuple(range(d))] if d > 2 else [])


def check_subsets(subsets, d):
    """``(list of sorted tuples, masks (P,) uint32)``; ``None``: ``default_subsets(d)``."""
    if not 1 <= int(d) <= MAX_D:
        raise ValueError(f"d must be in [1, {MAX_D}], got {d}")
    subsets = default_subsets(d) if subsets is None else list(subsets)
    if len(subsets) == 0:
        raise ValueError("subsets must name at least one subset")
    out, masks = [], []
    for s in subsets:
        s = (s,) if np.ndim(s) == 0 else tuple(s)
        if len(s) == 0:
            raise ValueError("every subset must name a coordinate")
        for j in s:
            if int(j) != j or not 0 <= int(j) < d:
                raise IndexError(f"a subset names coordinate {j}, outside [0, {d})")
        t = tuple(sorted(int(j) for j in s))
        if len(set(t)) != len(t):
            raise ValueError(f"subset {s} names a coordinate twice")
        out.append(t)
        masks.append(sum(1 << j for j in t))
    return out, np.array(masks, dtype=np.uint32)


def check_k(k):
    if int(k) != k or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must be an integer in [1, {MAX_K}], got {k!r}")
    return int(k)


def digamma_int(n):
    """``psi(n)`` of a positive integer: the harmonic sum below 64, the asymptotic series from there (below 1e-16)."""
    n = int(n)
    if n < 1:
        raise ValueError("digamma_int needs n >= 1")
    if n < 64:
        return -np.euler_gamma + math.fsum(1.0 / j for j in range(1, n))
    x = 1.0 / (n * n)
    return math.log(n) - 0.5 / n - x * (1.0 / 12.0 - x * (1.0 / 120.0 - x * (1.0 / 252.0)))


def log_unit_ball(d):
    """``log`` of the volume of the unit ball in ``d`` dimensions: ``(d / 2) log pi - lgamma(d / 2 + 1)``."""
    return 0.5 * d * math.log(math.pi) - math.lgamma(0.5 * d + 1.0)


def selected_rows(S, max_points):
    """The logical rows ``floor(i S / n)``, ``i < n = min(S, max_points)``, that a summary of ``S`` rows is taken over."""
    n = min(int(S), int(max_points))
    if n < 1:
        raise ValueError("max_points must be >= 1 and the chain must hold a row")
    return (np.arange(n, dtype=np.int64) * int(S)) // n


def unit_rows(x, lower, upper, max_points=None):
    """``(u (n, d), n_skipped)`` on the host: ``(x - lower) * (1 / (upper - lower))`` of the selected rows -- the library's
    two roundings --, a row with a non-finite coordinate as a row of NaN."""
    x = np.asarray(x, dtype=np.float64)
    lo, iw = _box(lower, upper, x.shape[1])
    if max_points is not None:
        x = x[selected_rows(x.shape[0], max_points)]
    u = (x - lo[None, :]) * iw[None, :]
    bad = ~np.all(np.isfinite(x), axis=1)
    u[bad] = np.nan
    return np.ascontiguousarray(u), int(bad.sum())


def _box(lower, upper, d):
    """``(lower, 1 / (upper - lower))``; both ``None``: the identity."""
    if lower is None and upper is None:
        return np.zeros(d), np.ones(d)
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lower, dtype=np.float64), (d,)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(upper, dtype=np.float64), (d,)))
    if not np.all(np.isfinite(lo) & np.isfinite(hi) & (lo < hi)):
        raise ValueError("the box must be finite with lower < upper")
    return lo, 1.0 / (hi - lo)


def _rows(x, what="x"):
    """``(rows (n, d), on_device)``; a vector is one column; ``(steps, walkers, d)`` is flattened."""
    if _lib.is_device_tensor(x):
        import torch
        if x.dtype != torch.float64 or x.dim() not in (1, 2, 3):
            raise TypeError(f"a device {what} must be a float64 tensor (n, d)")
        x = x.reshape(-1, 1) if x.dim() == 1 else x.reshape(-1, x.shape[-1])
        return x.contiguous(), True
    a = np.asarray(x, dtype=np.float64)
    if a.ndim == 1:
        a = a[:, None]
    if a.ndim == 3:
        a = a.reshape(-1, a.shape[-1])
    if a.ndim != 2 or a.shape[0] < 1 or not 1 <= a.shape[1] <= MAX_D:
        raise ValueError(f"{what} must be (n, d) with n >= 1 and d in [1, {MAX_D}]")
    return np.ascontiguousarray(a), False


# -- device calls -----------------------------------------------------------------------------------------------------
def unit_rows_dev(device, base, n_blocks, block_rows, block_stride_rows, d, lower, upper, max_points, block_stride=None):
    """``(U, n_skipped)``: the unit-box rows of the selected rows of device rows in the block layout of
    ``posterior_predictive_dev`` as a device tensor ``(n, d)``.  ``block_stride``: the stride between blocks in elements,
    where it is no multiple of ``d``."""
    import torch
    lo, iw = _box(lower, upper, int(d))
    hi = lo + 1.0 if lower is None and upper is None else np.ascontiguousarray(
        np.broadcast_to(np.asarray(upper, dtype=np.float64), (int(d),)))
    n = selected_rows(int(n_blocks) * int(block_rows), max_points).size
    U = torch.empty((n, int(d)), dtype=torch.float64, device=torch.device("cuda", int(device)))
    skipped = C.c_int64(0)
    check(_lib.lib().gpemu_unit_rows_dev(int(device), C.c_void_p(base), int(n_blocks), int(block_rows),
                                         int(block_stride_rows) * int(d) if block_stride is None else int(block_stride),
                                         int(d), ptr(lo), ptr(hi), n, C.c_void_p(U.data_ptr()),
                                         C.byref(skipped), _lib.current_stream(device)))
    return U, int(skipped.value)


def knn_dist_dev(device, UQ, UR, masks, k, splits=0, workspace_bytes=0):
    """``(r2, zeros)``, device tensors ``(P, nq)`` float64 and int32, of the dense device tensors ``UQ (nq, d)`` and
    ``UR (nr, d)`` (``None``: a self search)."""
    import torch
    nq, d = int(UQ.shape[0]), int(UQ.shape[1])
    nr = nq if UR is None else int(UR.shape[0])
    P = int(masks.size)
    r2 = torch.empty((P, nq), dtype=torch.float64, device=UQ.device)
    zeros = torch.empty((P, nq), dtype=torch.int32, device=UQ.device)
    check(_lib.lib().gpemu_knn_dist_dev(int(device), nq, nr, d, C.c_void_p(UQ.data_ptr()),
                                        None if UR is None else C.c_void_p(UR.data_ptr()), P, ptr(masks), int(k), int(splits),
                                        int(workspace_bytes), C.c_void_p(r2.data_ptr()), C.c_void_p(zeros.data_ptr()),
                                        _lib.current_stream(device)))
    return r2, zeros


def logsum_dev(device, r2, zeros=None, nu2=None):
    """``(counts (P, 3) int64: n_used, n_short, copies; sums (P, 2): the sum of v and of v^2)`` of the device tensors
    ``r2 (P, n)``, ``zeros`` and, for ``v = log nu2 - log r2`` instead of ``log r2``, ``nu2``."""
    P, n = int(r2.shape[0]), int(r2.shape[1])
    counts, sums = np.zeros((P, 3), dtype=np.int64), np.zeros((P, 2))
    check(_lib.lib().gpemu_knn_logsum_dev(int(device), P, n, C.c_void_p(r2.data_ptr()),
                                          None if zeros is None else C.c_void_p(zeros.data_ptr()),
                                          None if nu2 is None else C.c_void_p(nu2.data_ptr()), ptr(counts), ptr(sums),
                                          _lib.current_stream(device)))
    return counts, sums


def _search(U, V, masks, k, splits, device, workspace_bytes):
    """``(device index, r2, zeros)`` as device tensors: host rows through ``gpemu_knn_dist``, device rows in place."""
    import torch
    if _lib.is_device_tensor(U):
        dev = U.device.index or 0
        return (dev,) + knn_dist_dev(dev, U, V, masks, k, splits, workspace_bytes)
    _lib.require_device()
    dev = int(_lib.resolve_device(device))
    nq, d = U.shape
    nr = nq if V is None else V.shape[0]
    r2, zeros = np.empty((masks.size, nq)), np.empty((masks.size, nq), dtype=np.int32)
    check(_lib.lib().gpemu_knn_dist(dev, nq, nr, d, ptr(U), ptr(V), int(masks.size), ptr(masks), int(k), int(splits),
                                    int(workspace_bytes), ptr(r2), ptr(zeros)))
    td = torch.device("cuda", dev)
    return dev, torch.from_numpy(r2).to(td), torch.from_numpy(zeros).to(td)


# -- public functions -------------------------------------------------------------------------------------------------
def knn_distances(uq, ur=None, k=4, subsets=None, splits=0, device=None, workspace_bytes=0):
    """``(r2, zeros)``, each ``(P, nq)``: the squared Euclidean distance of every row of ``uq (nq, d)`` to its ``k``-th
    nearest row of ``ur (nr, d)`` (``None``: of ``uq`` itself) in the coordinates of every subset, and the number of rows
    of ``ur`` at squared distance exactly 0, which are copies and no neighbours (``+inf`` where fewer than ``k`` others
    remain; NaN for a query with a non-finite coordinate).  Device tensors for device rows.  The bits depend neither on
    ``splits`` (0: chosen by the library; 1 to 64: that many splits of the references) nor on ``workspace_bytes``."""
    U, on_device = _rows(uq, "uq")
    V = None
    if ur is not None:
        V, v_dev = _rows(ur, "ur")
        if v_dev != on_device or V.shape[1] != U.shape[1]:
            raise ValueError("uq and ur must both be host arrays or device tensors with the same columns")
    _, masks = check_subsets(subsets, U.shape[1])
    _, r2, zeros = _search(U, V, masks, check_k(k), splits, device, workspace_bytes)
    if on_device:
        return r2, zeros
    return r2.cpu().numpy(), zeros.cpu().numpy()


def _tables(out, d):
    """``joint``, ``per_parameter``, ``pairs`` and ``per_pair`` of a result, by the subsets it holds (NaN where absent)"""
    by = {s: float(v) for s, v in zip(out["subsets"], out["nats"])}
    out["joint"] = by.get(tuple(range(d)), math.nan)
    out["per_parameter"] = np.array([by.get((j,), math.nan) for j in range(d)])
    pairs = [s for s in out["subsets"] if len(s) == 2]
    out["pairs"] = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    out["per_pair"] = np.array([by[s] for s in pairs])
    return out


def _finish(subs, d, k, counts, sums, n_points, self_copies, allow_copies, what):
    """the rules of use and the moments of v: ``(mean, se factor sd / sqrt(n_used), n_used, copies)``"""
    n_used, n_short = counts[:, 0], counts[:, 1]
    copies = counts[:, 2] - (n_points if self_copies else 0)
    if np.any(n_short > 0):
        p = int(np.argmax(n_short > 0))
        raise ValueError(f"{what}: {int(n_short[p])} rows of subset {subs[p]} have fewer than k = {k} distinct neighbours")
    if np.any(n_used < 1):
        raise ValueError(f"{what}: no row with finite coordinates")
    if not allow_copies and np.any(copies > MAX_COPIES * n_points):
        p = int(np.argmax(copies))
        raise ValueError(f"{what}: {int(copies[p])} copies among {n_points} rows in subset {subs[p]} (more than "
                         f"{MAX_COPIES:g} of them): thin the chain by its autocorrelation time, or pass allow_copies=True")
    mean = sums[:, 0] / n_used
    var = np.where(n_used > 1, (sums[:, 1] - n_used * mean * mean) / np.maximum(n_used - 1, 1), 0.0)
    return mean, np.sqrt(np.maximum(var, 0.0) / n_used), n_used.copy(), copies


def entropy_from_sums(subs, k, n_points, mean_log_r2):
    """Kozachenko-Leonenko: ``H_p = psi(N) - psi(k) + log c_dp + (d_p / 2) mean(log r2)``."""
    dims = np.array([len(s) for s in subs], dtype=np.float64)
    lc = np.array([log_unit_ball(len(s)) for s in subs])
    return digamma_int(n_points) - digamma_int(k) + lc + 0.5 * dims * mean_log_r2


def _entropy(U, n_skipped, k, subsets, allow_copies, splits, device, workspace_bytes, what):
    d = int(U.shape[1])
    subs, masks = check_subsets(subsets, d)
    k = check_k(k)
    dev, r2, zeros = _search(U, None, masks, k, splits, device, workspace_bytes)
    counts, sums = logsum_dev(dev, r2, zeros)
    n_points = int(U.shape[0]) - int(n_skipped)
    mean, sem, n_used, copies = _finish(subs, d, k, counts, sums, n_points, True, allow_copies, what)
    dims = np.array([len(s) for s in subs], dtype=np.int64)
    return {"subsets": subs, "dims": dims, "entropy": entropy_from_sums(subs, k, n_points, mean), "se": 0.5 * dims * sem,
            "n_points": n_points, "n_used": n_used, "copies": copies, "k": k}


def _n_nan_rows(U):
    if _lib.is_device_tensor(U):
        import torch
        return int(torch.isnan(U).any(dim=1).sum().item())
    return int(np.isnan(U).any(axis=1).sum())


def entropy(u, k=4, subsets=None, allow_copies=True, splits=0, device=None, workspace_bytes=0):
    """The differential entropy, in nats, of the rows ``u (n, d)`` in every subset of the coordinates: a dict with
    ``subsets``, ``dims``, ``entropy`` ``(P,)``, ``se`` (see ``information_gain``), ``n_points``, ``n_used``, ``copies``
    and ``k``.  ``H_p = psi(N) - psi(k) + log c_dp + (d_p / 2) mean(log r2)`` with ``c_dp`` the volume of the unit ball and
    ``N`` the number of rows with finite coordinates."""
    U, _ = _rows(u, "u")
    return _entropy(U, _n_nan_rows(U), k, subsets, allow_copies, splits, device, workspace_bytes, "entropy")


def _gain(U, n_skipped, k, subsets, allow_copies, splits, device, workspace_bytes):
    out = _entropy(U, n_skipped, k, subsets, allow_copies, splits, device, workspace_bytes, "information_gain")
    out["nats"] = -out.pop("entropy")
    out["bits"] = out["nats"] / LOG2
    return _tables(out, int(U.shape[1]))


def information_gain(x, lower, upper, k=4, subsets=None, max_points=65536, allow_copies=False, splits=0, device=None,
                     workspace_bytes=0):
    """``KL(posterior || prior)`` of the rows ``x (S, d)`` under the uniform prior on the box ``[lower, upper]``, for
    every subset of the parameters (default: every parameter, every pair, the joint): minus the Kozachenko-Leonenko
    entropy of the unit-box rows of ``n = min(S, max_points)`` evenly spaced rows ``floor(i S / n)``.  A dict with

    * ``subsets`` (tuples), ``dims``, ``nats``, ``bits`` and ``se`` ``(P,)``;
    * ``n_points`` (the rows with finite coordinates), ``n_used`` ``(P,)``, ``copies`` ``(P,)`` (the pairs (row, other row
      at distance 0 in the subset)) and ``k``;
    * ``joint``, ``per_parameter (d,)``, ``pairs (n_pairs, 2)`` and ``per_pair``: the same numbers by what they are of (NaN
      where ``subsets`` holds none).

    ``se = (d_p / 2) sd(log r2) / sqrt(n_used)`` is a LOWER bound of the standard error: it ignores the chain's
    autocorrelation and the dependence between neighbours.  The estimate is biased low near the faces of the box (no
    boundary correction).  ``ValueError`` where a row has fewer than ``k`` distinct neighbours, and where the copies
    exceed 0.1 of the rows unless ``allow_copies``: thin the chain by its autocorrelation time."""
    X, on_device = _rows(x)
    if on_device:
        return gain_of_view(DeviceRows.of_tensor(X), lower, upper, k, subsets, max_points, allow_copies, splits,
                            workspace_bytes)
    U, skipped = unit_rows(X, lower, upper, max_points)
    return _gain(U, skipped, k, subsets, allow_copies, splits, device, workspace_bytes)


def _divergence(Ux, skipped_x, Uy, skipped_y, k, subsets, allow_copies, splits, device, workspace_bytes):
    d = int(Ux.shape[1])
    if int(Uy.shape[1]) != d:
        raise ValueError(f"x has {d} columns, y {int(Uy.shape[1])}")
    subs, masks = check_subsets(subsets, d)
    k = check_k(k)
    dev, rho2, zeros = _search(Ux, None, masks, k, splits, device, workspace_bytes)
    _, nu2, _ = _search(Ux, Uy, masks, k, splits, device, workspace_bytes)
    counts, sums = logsum_dev(dev, rho2, zeros, nu2)
    n, m = int(Ux.shape[0]) - int(skipped_x), int(Uy.shape[0]) - int(skipped_y)
    if n < 2 or m < 1:
        raise ValueError("kl_divergence needs at least two rows of x and one of y with finite coordinates")
    mean, sem, n_used, copies = _finish(subs, d, k, counts, sums, n, True, allow_copies, "kl_divergence")
    dims = np.array([len(s) for s in subs], dtype=np.int64)
    nats = 0.5 * dims * mean + math.log(m / (n - 1.0))
    out = {"subsets": subs, "dims": dims, "nats": nats, "bits": nats / LOG2, "se": 0.5 * dims * sem, "n_points": n,
           "m_points": m, "n_used": n_used, "copies": copies, "k": k}
    return _tables(out, d)


def kl_divergence(x, y, lower=None, upper=None, k=4, subsets=None, max_points=65536, allow_copies=False, splits=0,
                  device=None, workspace_bytes=0):
    """``D(P || Q)`` in nats between the samples ``x (n, d)`` of P and ``y (m, d)`` of Q, for every subset of the
    coordinates: ``(d_p / n) sum_i log(nu_i / rho_i) + log(m / (n - 1))`` with ``rho_i`` the distance of row i of x to its
    k-th neighbour in x and ``nu_i`` to its k-th neighbour in y (Wang, Kulkarni, Verdu 2009), in the box's unit coordinates
    (``lower = upper = None``: as given).  At most ``max_points`` evenly spaced rows of each.  The dict of
    ``information_gain`` plus ``m_points``; ``copies`` are those within x.  The same call serves a derived quantity with a
    prior that is not uniform: samples of its posterior against samples of its prior as 1-column arrays."""
    X, x_dev = _rows(x, "x")
    Y, y_dev = _rows(y, "y")
    if x_dev != y_dev:
        raise ValueError("x and y must both be host arrays or both device tensors")
    if X.shape[1] != Y.shape[1]:
        raise ValueError(f"x has {X.shape[1]} columns, y {Y.shape[1]}")
    if x_dev:
        return divergence_of_views(DeviceRows.of_tensor(X), DeviceRows.of_tensor(Y), lower, upper, k, subsets, max_points,
                                   allow_copies, splits, workspace_bytes)
    Ux, sx = unit_rows(X, lower, upper, max_points)
    Uy, sy = unit_rows(Y, lower, upper, max_points)
    return _divergence(Ux, sx, Uy, sy, k, subsets, allow_copies, splits, device, workspace_bytes)


def gain_of_view(rows, lower, upper, k=4, subsets=None, max_points=65536, allow_copies=False, splits=0, workspace_bytes=0):
    """``information_gain`` of the ``DeviceRows`` ``rows`` read in place."""
    U, skipped = unit_rows_dev(rows.device, *rows.layout, rows.d, lower, upper, max_points)
    return _gain(U, skipped, k, subsets, allow_copies, splits, rows.device, workspace_bytes)


def divergence_of_views(rows_x, other, lower, upper, k=4, subsets=None, max_points=65536, allow_copies=False, splits=0,
                        workspace_bytes=0):
    """``kl_divergence`` of ``DeviceRows`` against ``other``: ``DeviceRows``, a host array or a device tensor ``(m, d)``."""
    device, d = rows_x.device, rows_x.d
    Ux, sx = unit_rows_dev(device, *rows_x.layout, d, lower, upper, max_points)
    if not isinstance(other, DeviceRows):
        import torch
        Y, on_device = _rows(other, "other")
        if not on_device:
            Y = torch.from_numpy(Y).to(torch.device("cuda", int(device)))
        if int(Y.shape[1]) != int(d):
            raise ValueError(f"the chain has {d} parameters, other {int(Y.shape[1])} columns")
        other = DeviceRows.of_tensor(Y)
    Uy, sy = unit_rows_dev(device, *other.layout, d, lower, upper, max_points)
    return _divergence(Ux, sx, Uy, sy, k, subsets, allow_copies, splits, device, workspace_bytes)
