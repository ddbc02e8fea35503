"""Marginal posteriors on the device: histograms, highest-density intervals, kernel densities.

The data of a corner plot from EVERY sample of a chain -- what the reference draws from a subsample (ref: plot_mcmc.py
_plot_posterior_pairplot: a Gaussian KDE of each parameter on the diagonal, each pair off it, the shaded
highest-density interval) and the narrowest-window rule of its ``credible_interval(..., 'hpd')``:

* ``histograms``: exact 1-D and 2-D counts, equal as integers to ``np.histogram`` / ``np.histogram2d`` on the same edges;
* ``hpd_intervals``: the narrowest window that leaves ``n_out = int((1 - confidence) * S)`` samples outside, both ends
  elements of the input, ties to the lowest window (``np.argmin``);
* ``kde_1d``: the direct-sum Gaussian kernel density of each parameter (no binning, no truncation), bandwidth and grid by
  scipy's Scott factor and seaborn's ``cut`` rule unless given;
* ``credible_levels``: the contour levels of a 2-D histogram (host numpy);
* ``kde_2d``: the direct-sum Gaussian kernel density of each PAIR of parameters on a product grid, a matrix product on
  the fp64 matrix cores -- scipy's full-covariance ``gaussian_kde`` on a sheared grid, or the
  axis-aligned product kernel -- with ``kde_2d_mesh`` and ``density_levels`` (host numpy) for the contours.

Samples are ``(S, d)`` (or ``(S,)``): numpy arrays go through the host entries, contiguous float64 device tensors are read
in place.  ``summary`` takes all three at once; ``DeviceSampler.marginals`` is the same over the stored chain where it
lies.  There is no CPU implementation."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr
from .rows import DeviceRows

PATHS = ("HIST_SWEEP", "PAIR_GROUP", "SORT_BATCH", "WINDOW_SEARCH", "KDE")
PATHS_KDE2D = ("DENSITY", "PAIR_BATCH", "PARTIAL_SUM", "MOMENTS", "EXTENTS")
MAX_D, MAX_BINS_1D, MAX_BINS_2D, MAX_GRID_2D = 16, 4096, 256, 512


def path_counts():
    """The library's counters of the marginals' launches since the process started, by name."""
    out = (C.c_int64 * len(PATHS))()
    n = _lib.lib().gpemu_marginal_path_counts(out, len(PATHS))
    if n < 0:
        check(n)
    return {k: int(out[i]) for i, k in enumerate(PATHS)}


def kde2d_path_counts():
    """The library's counters of the 2-D densities' launches since the process started, by name (a family of its own:
    ``path_counts`` does not move)."""
    out = (C.c_int64 * len(PATHS_KDE2D))()
    n = _lib.lib().gpemu_kde2d_path_counts(out, len(PATHS_KDE2D))
    if n < 0:
        check(n)
    return {k: int(out[i]) for i, k in enumerate(PATHS_KDE2D)}


# -- host-side rules ------------------------------------------------------------------------------------------------
def pair_indices(d):
    """The pairs (i, j), i < j, in row-major order: ``(d (d - 1) / 2, 2)`` int64."""
    return np.array([(i, j) for i in range(d) for j in range(i + 1, d)], dtype=np.int64).reshape(-1, 2)


def bin_edges(lower, upper, bins):
    """``np.linspace(lower[j], upper[j], bins + 1)`` per parameter: ``(d, bins + 1)``."""
    lo, hi = np.atleast_1d(np.asarray(lower, dtype=np.float64)), np.atleast_1d(np.asarray(upper, dtype=np.float64))
    if lo.shape != hi.shape or lo.ndim != 1:
        raise ValueError("lower and upper must be vectors of one length")
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(hi > lo)):
        raise ValueError("the box must be finite with upper > lower")
    if int(bins) < 1:
        raise ValueError("bins must be >= 1")
    return np.stack([np.linspace(a, b, int(bins) + 1) for a, b in zip(lo, hi)])


def n_outside(confidence, S):
    """Samples left outside the interval, as the reference computes it (ref: mcmc.py:150): ``int((1 - confidence) *
    S)`` per level, an int64 vector.  ValueError where it is 0 (no window to choose from) or exceeds S."""
    conf = np.atleast_1d(np.asarray(confidence, dtype=np.float64))
    if conf.ndim != 1 or conf.size == 0:
        raise ValueError("confidence must be a number or a non-empty sequence")
    out = np.array([int((1 - float(c)) * int(S)) for c in conf], dtype=np.int64)
    for c, n in zip(conf, out):
        if not 1 <= n <= S:
            raise ValueError(f"confidence {c}: n_out = int((1 - confidence) * {S}) = {n} is outside [1, {S}]")
    return out


def scott_bandwidth(S, std_ddof1):
    """scipy.stats.gaussian_kde's default for 1-D data: ``S ** (-1 / 5) * std(ddof=1)``."""
    return np.power(float(S), -1.0 / 5.0) * np.asarray(std_ddof1, dtype=np.float64)


def default_grid(xmin, xmax, bandwidth, n_grid=200, cut=3.0):
    """seaborn's support: ``linspace(min - cut h, max + cut h, n_grid)`` per parameter, ``(d, n_grid)``."""
    xmin, xmax, h = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (xmin, xmax, bandwidth))
    return np.stack([np.linspace(a - cut * w, b + cut * w, int(n_grid)) for a, b, w in zip(xmin, xmax, h)])


def credible_levels(hist_2d, probabilities):
    """For each 2-D histogram ``(..., nb, nb)`` and probability p: the largest count c such that the bins with count
    >= c hold at least p of the counted mass -- the contour levels of a corner plot.  ``(..., len(probabilities))``
    int64 (a scalar p drops the last axis); an empty histogram gives 0."""
    h = np.asarray(hist_2d)
    if h.ndim < 2:
        raise ValueError("hist_2d must have at least two axes")
    p = np.atleast_1d(np.asarray(probabilities, dtype=np.float64))
    if not np.all((p >= 0.0) & (p <= 1.0)):
        raise ValueError("probabilities must be in [0, 1]")
    lead = h.shape[:-2]
    flat = h.reshape((-1, h.shape[-2] * h.shape[-1])).astype(np.int64)
    out = np.zeros((flat.shape[0], p.size), dtype=np.int64)
    for r, row in enumerate(flat):
        total = int(row.sum())
        if total == 0:
            continue
        counts = np.sort(row)[::-1]
        mass = np.cumsum(counts)
        for q, prob in enumerate(p):
            # the first position at which the bins so far hold p of the mass: its count is the level (the bins tied
            # with it come along); exact integer comparison, mass >= ceil(p total) up to the product's rounding
            need = prob * total
            k = int(np.searchsorted(mass, need, side="left"))
            out[r, q] = counts[min(k, counts.size - 1)]
    out = out.reshape(lead + (p.size,))
    return out[..., 0] if np.ndim(probabilities) == 0 else out


def density_levels(density, probabilities):
    """The float twin of ``credible_levels``: for each panel ``(..., G, G)`` of density values on cells of equal area
    and each probability p, the largest density value t such that the cells with value >= t hold at least p of the
    panel's summed mass -- the contour levels of the 68 % / 95 % regions.  ``(..., len(probabilities))`` float64 (a
    scalar p drops the last axis); an all-zero panel gives 0."""
    z = np.asarray(density, dtype=np.float64)
    if z.ndim < 2:
        raise ValueError("density must have at least two axes")
    p = np.atleast_1d(np.asarray(probabilities, dtype=np.float64))
    if not np.all((p >= 0.0) & (p <= 1.0)):
        raise ValueError("probabilities must be in [0, 1]")
    lead = z.shape[:-2]
    flat = z.reshape((-1, z.shape[-2] * z.shape[-1]))
    out = np.zeros((flat.shape[0], p.size))
    for r, row in enumerate(flat):
        vals = np.sort(row)[::-1]
        mass = np.cumsum(vals)
        total = mass[-1]                 # the running sum's own end: p = 1 is reached where the sum stops growing
        if not total > 0.0:
            out[r] = total               # 0 for an all-zero panel, NaN for a NaN one
            continue
        for q, prob in enumerate(p):
            k = int(np.searchsorted(mass, prob * total, side="left"))
            out[r, q] = vals[min(k, vals.size - 1)]
    out = out.reshape(lead + (p.size,))
    return out[..., 0] if np.ndim(probabilities) == 0 else out


def scott_factor_2d(S, bw_adjust=1.0):
    """scipy.stats.gaussian_kde's Scott factor for two dimensions, ``S ** (-1 / 6)``, times ``bw_adjust``."""
    return float(bw_adjust) * np.power(float(S), -1.0 / 6.0)


def _pair_list(pairs, d):
    if pairs is None:
        return pair_indices(d)
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if pr.shape[0] < 1:
        raise ValueError("pairs must hold at least one pair")
    if np.any(pr < 0) or np.any(pr >= d) or np.any(pr[:, 0] == pr[:, 1]):
        raise ValueError(f"every pair must be two different parameters in [0, {d})")
    return np.ascontiguousarray(pr)


def kde2d_plan(S, d, pairs=None, covariance="full", bandwidth=None, shear=None, grid_a=None, grid_b=None, n_grid=100,
               cut=3.0, bw_adjust=1.0, cov=None, extents=None):
    """The plan of ``kde_2d`` -- ``pairs (P, 2)``, ``shear (P,)``, ``bandwidth (P, 2)``, ``grid_a``, ``grid_b (P, G)``
    -- from what is given and, for the rest, from ``cov() -> (d, d)`` (the ``ddof=1`` covariance of the samples) and
    ``extents(pairs (n, 2), shear (n,)) -> (n, 2)`` (the minimum and maximum of ``x_j - shear x_i``), which are only
    called where something is missing.  A pure host function.

    For pair (i, j) and the factor ``f = bw_adjust S ** (-1 / 6)``: with ``"full"`` the shear is ``C_ij / C_ii``, with
    ``"diagonal"`` 0; ``h_a = f sqrt(C_ii)`` and ``h_b = f sqrt(var(v))``, ``var(v) = C_jj - shear (2 C_ij - shear C_ii)``
    the variance of the sheared coordinate ``v = x_j - shear x_i`` -- the conditional variance ``C_jj - C_ij^2 / C_ii``
    under ``"full"`` (x and v are then uncorrelated and ``f^2 C`` is diagonal in them: scipy's bandwidth matrix), ``C_jj``
    under ``"diagonal"``.  The grids are ``linspace(min - cut h, max + cut h, n_grid)`` of x_i and of v."""
    if covariance not in ("full", "diagonal"):
        raise ValueError(f"covariance must be 'full' or 'diagonal', got {covariance!r}")
    pr = _pair_list(pairs, d)
    P = pr.shape[0]
    beta = None if shear is None else np.broadcast_to(np.asarray(shear, dtype=np.float64), (P,)).copy()
    h = None if bandwidth is None else np.broadcast_to(np.asarray(bandwidth, dtype=np.float64), (P, 2)).copy()
    if h is None or (beta is None and covariance == "full"):
        if S < 3:
            raise ValueError(f"pair ({pr[0, 0]}, {pr[0, 1]}): the default bandwidth needs at least 3 samples, got {S}")
        c = np.asarray(cov(), dtype=np.float64).reshape(d, d)
        cii, cjj, cij = c[pr[:, 0], pr[:, 0]], c[pr[:, 1], pr[:, 1]], c[pr[:, 0], pr[:, 1]]
        for (i, j), a, b in zip(pr, cii, cjj):
            if not (a > 0.0 and b > 0.0 and np.isfinite(a) and np.isfinite(b)):
                raise ValueError(f"pair ({i}, {j}): the variances {a}, {b} must be finite and > 0")
        if beta is None:
            beta = cij / cii if covariance == "full" else np.zeros(P)
        if h is None:
            var_v = cjj - beta * (2.0 * cij - beta * cii)
            for (i, j), v, b in zip(pr, var_v, cjj):
                # (a variance of v within the rounding of C_jj is no variance: scipy raises for a singular covariance)
                if not v > 64.0 * np.finfo(np.float64).eps * b:
                    raise ValueError(f"pair ({i}, {j}): the conditional variance {v} is not > 0 (the two parameters "
                                     "are linearly dependent); use covariance='diagonal' or give the bandwidth")
            h = scott_factor_2d(S, bw_adjust) * np.sqrt(np.stack([cii, var_v], axis=1))
    if beta is None:
        beta = np.zeros(P)
    if not np.all(np.isfinite(beta)):
        raise ValueError(f"every shear must be finite, got {beta}")
    if not np.all(np.isfinite(h) & (h > 0.0)):
        raise ValueError(f"every bandwidth must be finite and > 0, got {h}")

    def given(g, name):
        g = np.asarray(g, dtype=np.float64)
        g = np.broadcast_to(g, (P, g.shape[-1])).copy() if g.ndim == 1 else np.ascontiguousarray(g)
        if g.ndim != 2 or g.shape[0] != P or g.shape[1] < 1:
            raise ValueError(f"{name} must be (G,) or ({P}, G)")
        return g
    ga = None if grid_a is None else given(grid_a, "grid_a")
    gb = None if grid_b is None else given(grid_b, "grid_b")
    G = ga.shape[1] if ga is not None else (gb.shape[1] if gb is not None else int(n_grid))
    if ga is not None and gb is not None and ga.shape[1] != gb.shape[1]:
        raise ValueError("grid_a and grid_b must have one length")
    if not 1 <= G <= MAX_GRID_2D:
        raise ValueError(f"the grid must have 1 to {MAX_GRID_2D} points per axis, got {G}")
    if ga is None or gb is None:
        # one pass for both: the extents of x_i are those of the pair (j, i) without shear
        ends = np.asarray(extents(np.concatenate([pr[:, ::-1], pr]), np.concatenate([np.zeros(P), beta])))
        if not np.all(np.isfinite(ends)):
            raise ValueError("the default grid needs finite samples")
        if ga is None:
            ga = default_grid(ends[:P, 0], ends[:P, 1], h[:, 0], G, cut)
        if gb is None:
            gb = default_grid(ends[P:, 0], ends[P:, 1], h[:, 1], G, cut)
    return {"pairs": pr, "shear": np.ascontiguousarray(beta), "bandwidth": np.ascontiguousarray(h),
            "grid_a": np.ascontiguousarray(ga), "grid_b": np.ascontiguousarray(gb)}


def kde2d_plan_host(x, **kw):
    """``kde2d_plan`` of host samples ``x (S, d)``, moments and extents by numpy."""
    x = np.asarray(x, dtype=np.float64)
    S, d = x.shape

    def extents(pr, beta):
        v = x[:, pr[:, 1]] - beta[None, :] * x[:, pr[:, 0]]
        return np.stack([v.min(axis=0), v.max(axis=0)], axis=1)
    return kde2d_plan(S, d, cov=lambda: np.atleast_2d(np.cov(x, rowvar=False, ddof=1)), extents=extents, **kw)


def kde_2d_mesh(result, p):
    """``(X, Y)``, the ``(G, G)`` meshes of panel ``p`` of a ``kde_2d`` result in parameter coordinates -- what contour
    routines take beside ``density[p]``: ``X = grid_a[p][:, None]``, ``Y = grid_b[p][None, :] + shear[p] X`` (a
    parallelogram where the shear is not 0)."""
    ga, gb = np.asarray(result["grid_a"])[p], np.asarray(result["grid_b"])[p]
    X = np.broadcast_to(ga[:, None], (ga.size, gb.size)).copy()
    return X, gb[None, :] + float(np.asarray(result["shear"])[p]) * X


# -- device plumbing ------------------------------------------------------------------------------------------------
def _samples(samples):
    """``(array or tensor (S, d), on_device)``; a vector is one parameter."""
    if _lib.is_device_tensor(samples):
        import torch
        if samples.dtype != torch.float64 or samples.dim() not in (1, 2):
            raise TypeError("device samples must be a float64 tensor (S, d)")
        x = samples.reshape(samples.shape[0], -1).contiguous()
        return x, True
    x = np.asarray(samples, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    if x.ndim != 2:
        raise ValueError("samples must be (S, d)")
    return np.ascontiguousarray(x), False


def _check_shape(S, d):
    if S < 1:
        raise ValueError("no samples")
    if not 1 <= d <= MAX_D:
        raise ValueError(f"d must be in [1, {MAX_D}], got {d}")


def _hist_dev(device, base, n_blocks, block_rows, block_stride_rows, d, e1, e2, group_counters=0):
    """The histograms of device rows in the block layout: ``(hist_1d, hist_2d, n_inside)`` as numpy int64."""
    import torch
    nb1, nb2, npairs = e1.shape[1] - 1, e2.shape[1] - 1, d * (d - 1) // 2
    dev = torch.device("cuda", int(device))
    h1 = torch.empty((d, nb1), dtype=torch.int64, device=dev)
    h2 = torch.empty((max(npairs, 1), nb2, nb2), dtype=torch.int64, device=dev)
    ni = torch.empty((d,), dtype=torch.int64, device=dev)
    check(_lib.lib().gpemu_marginal_hist_dev(int(device), C.c_void_p(base), int(n_blocks), int(block_rows),
                                             int(block_stride_rows), int(d), int(nb1), ptr(e1), int(nb2), ptr(e2),
                                             int(group_counters), C.c_void_p(h1.data_ptr()), C.c_void_p(h2.data_ptr()),
                                             C.c_void_p(ni.data_ptr()), _lib.current_stream(device)))
    return h1.cpu().numpy(), h2[:npairs].cpu().numpy(), ni.cpu().numpy()


def _hpd_dev(device, base, S, d, n_out, workspace_bytes=0):
    """The intervals of the d parameters of a dense device matrix ``[S][d]``: ``(n_levels, d, 2)``."""
    import torch
    n_out = np.ascontiguousarray(n_out, dtype=np.int64)
    out = torch.empty((d, n_out.size, 2), dtype=torch.float64, device=torch.device("cuda", int(device)))
    check(_lib.lib().gpemu_hpd_dev(int(device), int(d), int(S), C.c_void_p(base), 1, int(d), int(n_out.size), ptr(n_out),
                                   C.c_void_p(out.data_ptr()), int(workspace_bytes), _lib.current_stream(device)))
    return np.ascontiguousarray(out.cpu().numpy().transpose(1, 0, 2))


def _kde_dev(device, base, S, d, grid, h):
    """The densities of the d parameters of a dense device matrix ``[S][d]`` on ``grid (d, G)``: ``(d, G)``."""
    import torch
    out = torch.empty(grid.shape, dtype=torch.float64, device=torch.device("cuda", int(device)))
    check(_lib.lib().gpemu_kde1d_dev(int(device), int(d), int(S), C.c_void_p(base), 1, int(d), int(grid.shape[1]),
                                     ptr(grid), ptr(h), C.c_void_p(out.data_ptr()), _lib.current_stream(device)))
    return out.cpu().numpy()


def _moments_dev(device, base, S, d):
    """``(mean, var with divisor S)`` of a dense device matrix ``[S][d]``."""
    mean, var = np.empty(d), np.empty(d)
    check(_lib.lib().gpemu_marginal_moments_dev(int(device), C.c_void_p(base), int(S), int(d), ptr(mean), ptr(var),
                                                _lib.current_stream(device)))
    return mean, var


def _pair_moments_dev(device, base, n_blocks, block_rows, block_stride_rows, d, pairs=None, shear=None, moments=True):
    """``(mean, cov with divisor S, extents (n, 2))`` of device rows in the block layout (what is not asked: None)."""
    mean, cov = (np.empty(d), np.empty((d, d))) if moments else (None, None)
    n = 0 if pairs is None else int(np.asarray(pairs).shape[0])
    pr = None if n == 0 else np.ascontiguousarray(pairs, dtype=np.int64)
    sh = None if n == 0 else np.ascontiguousarray(shear, dtype=np.float64)
    ext = None if n == 0 else np.empty((n, 2))
    check(_lib.lib().gpemu_pair_moments_dev(int(device), C.c_void_p(base), int(n_blocks), int(block_rows),
                                            int(block_stride_rows), int(d), ptr(mean), ptr(cov), n, ptr(pr), ptr(sh),
                                            ptr(ext), _lib.current_stream(device)))
    return mean, cov, ext


def _kde2d_dev(device, base, n_blocks, block_rows, block_stride_rows, d, plan, workspace_bytes=0):
    """The panels of ``plan`` from device rows in the block layout, read in place: ``(P, G, G)``."""
    import torch
    P, G = plan["grid_a"].shape
    out = torch.empty((P, G, G), dtype=torch.float64, device=torch.device("cuda", int(device)))
    check(_lib.lib().gpemu_kde2d_dev(int(device), C.c_void_p(base), int(n_blocks), int(block_rows),
                                     int(block_stride_rows), int(d), P, ptr(plan["pairs"]), ptr(plan["shear"]),
                                     ptr(plan["bandwidth"]), G, ptr(plan["grid_a"]), ptr(plan["grid_b"]),
                                     C.c_void_p(out.data_ptr()), int(workspace_bytes), _lib.current_stream(device)))
    return out.cpu().numpy()


def _kde2d_view(rows, workspace_bytes=0, **plan_kw):
    """``kde_2d`` of ``DeviceRows`` read in place: the plan from the device moments and extents, then the panels."""
    S, at = rows.rows, (rows.device, *rows.layout, rows.d)

    def cov():
        return _pair_moments_dev(*at)[1] * (S / (S - 1.0))
    plan = kde2d_plan(S, rows.d, cov=cov, extents=lambda pr, beta: _pair_moments_dev(*at, pr, beta, moments=False)[2],
                      **plan_kw)
    plan["density"] = _kde2d_dev(*at, plan, workspace_bytes)
    return plan


def _kde_plan(S, d, grid, bandwidth, n_grid, cut, spread):
    """Bandwidth ``(d,)`` and grid ``(d, G)`` of a density: as given, else Scott's rule and seaborn's support from
    ``spread() -> (std with ddof 1, min, max)``, which is only called where something is missing."""
    h = None if bandwidth is None else np.broadcast_to(np.asarray(bandwidth, dtype=np.float64), (d,)).copy()
    if h is None or grid is None:
        sd, xmin, xmax = spread()
        if h is None:
            if S < 2:
                raise ValueError("the default bandwidth needs at least two samples")
            h = scott_bandwidth(S, sd)
    if not np.all(np.isfinite(h) & (h > 0.0)):
        raise ValueError(f"every bandwidth must be finite and > 0, got {h}")
    if grid is None:
        if int(n_grid) < 1:
            raise ValueError("n_grid must be >= 1")
        if not (np.all(np.isfinite(xmin)) and np.all(np.isfinite(xmax))):
            raise ValueError("the default grid needs finite samples")
        g = default_grid(xmin, xmax, h, n_grid, cut)
    else:
        g = np.asarray(grid, dtype=np.float64)
        g = np.broadcast_to(g, (d, g.shape[-1])).copy() if g.ndim == 1 else np.ascontiguousarray(g)
        if g.ndim != 2 or g.shape[0] != d or g.shape[1] < 1:
            raise ValueError(f"grid must be (G,) or ({d}, G)")
    return np.ascontiguousarray(h), np.ascontiguousarray(g)


# -- public functions ---------------------------------------------------------------------------------------------
def histograms(samples, lower, upper, bins_1d=100, bins_2d=50, device=None, group_counters=0):
    """Exact marginal histograms of ``samples (S, d)`` over the box ``[lower, upper]``: a dict of ``edges_1d (d, nb1 +
    1)``, ``edges_2d (d, nb2 + 1)``, ``hist_1d (d, nb1)``, ``pairs (n_pairs, 2)``, ``hist_2d (n_pairs, nb2, nb2)``
    (first axis: the pair's first parameter, as ``np.histogram2d``) and ``n_inside (d,)``, counts as int64, equal to
    numpy's on the same edges.  Samples outside the box and NaN are not counted.  ``group_counters`` bounds the
    counters of one sweep over the samples (0: the default); the counts do not depend on it."""
    x, on_device = _samples(samples)
    S, d = int(x.shape[0]), int(x.shape[1])
    _check_shape(S, d)
    if not (1 <= int(bins_1d) <= MAX_BINS_1D and 1 <= int(bins_2d) <= MAX_BINS_2D):
        raise ValueError(f"bins_1d must be in [1, {MAX_BINS_1D}] and bins_2d in [1, {MAX_BINS_2D}]")
    e1, e2 = bin_edges(lower, upper, bins_1d), bin_edges(lower, upper, bins_2d)
    if e1.shape[0] != d:
        raise ValueError(f"the box has {e1.shape[0]} parameters, the samples {d}")
    pairs = pair_indices(d)
    if on_device:
        h1, h2, ni = _hist_dev(x.device.index or 0, x.data_ptr(), 1, S, S, d, e1, e2, group_counters)
    else:
        _lib.require_device()
        h1 = np.empty((d, int(bins_1d)), dtype=np.int64)
        h2 = np.empty((pairs.shape[0], int(bins_2d), int(bins_2d)), dtype=np.int64)
        ni = np.empty(d, dtype=np.int64)
        check(_lib.lib().gpemu_marginal_hist(int(_lib.resolve_device(device)), S, d, ptr(x), int(bins_1d), ptr(e1),
                                             int(bins_2d), ptr(e2), int(group_counters), ptr(h1),
                                             ptr(h2) if pairs.shape[0] else None, ptr(ni)))
    return {"edges_1d": e1, "edges_2d": e2, "hist_1d": h1, "pairs": pairs, "hist_2d": h2, "n_inside": ni}


def hpd_intervals(samples, confidence=0.9, axis=0, device=None, workspace_bytes=0):
    """Highest-posterior-density intervals by the reference's rule (``credible_interval(x, confidence, 'hpd')`` per
    parameter): ``(n_levels, d, 2)``, or ``(d, 2)`` for a scalar confidence, ``[..., 0]`` the lower end.  Both ends
    are elements of the input.  A parameter with a NaN or an infinite extreme gives NaN."""
    if _lib.is_device_tensor(samples):
        x, _ = _samples(samples if axis in (0, -samples.dim()) else samples.movedim(axis, 0))
        S, d = int(x.shape[0]), int(x.shape[1])
        _check_shape(S, 1)
        n_out = n_outside(confidence, S)
        out = _hpd_dev(x.device.index or 0, x.data_ptr(), S, d, n_out, workspace_bytes)
    else:
        x = np.asarray(samples, dtype=np.float64)
        if x.ndim == 1:
            x = x[:, None]
        x = np.moveaxis(x, axis, 0)
        if x.ndim != 2:
            raise ValueError("samples must be (S, d)")
        S, d = x.shape
        _check_shape(S, 1)
        n_out = n_outside(confidence, S)
        _lib.require_device()
        rows = np.ascontiguousarray(x.T)
        res = np.empty((d, n_out.size, 2))
        check(_lib.lib().gpemu_hpd(int(_lib.resolve_device(device)), d, S, ptr(rows), int(n_out.size), ptr(n_out),
                                   ptr(res)))
        out = np.ascontiguousarray(res.transpose(1, 0, 2))
    return out[0] if np.ndim(confidence) == 0 else out


def kde_1d(samples, grid=None, bandwidth=None, n_grid=200, cut=3.0, device=None):
    """Gaussian kernel density of every parameter of ``samples (S, d)``, the direct sum over all samples: a dict of
    ``grid (d, G)``, ``density (d, G)`` and ``bandwidth (d,)``.  ``bandwidth``: a number or ``(d,)`` (the standard
    deviation of the kernel), default Scott's rule ``S ** (-1/5) * std(ddof=1)`` as scipy's ``gaussian_kde``; ``grid``:
    ``(G,)`` or ``(d, G)``, default ``linspace(min - cut h, max + cut h, n_grid)`` as seaborn's ``kdeplot``."""
    x, on_device = _samples(samples)
    S, d = int(x.shape[0]), int(x.shape[1])
    _check_shape(S, 1)
    if on_device:
        dev, base = x.device.index or 0, x.data_ptr()

        def spread():
            _, var = _moments_dev(dev, base, S, d)
            ends = _hpd_dev(dev, base, S, d, [1])[0]         # n_out = 1, window 0: (smallest, largest)
            return np.sqrt(var * (S / max(S - 1.0, 1.0))), ends[:, 0], ends[:, 1]
        h, g = _kde_plan(S, d, grid, bandwidth, n_grid, cut, spread)
        dens = _kde_dev(dev, base, S, d, g, h)
    else:
        h, g = _kde_plan(S, d, grid, bandwidth, n_grid, cut,
                         lambda: (x.std(axis=0, ddof=1) if S > 1 else np.full(d, np.nan), x.min(axis=0), x.max(axis=0)))
        _lib.require_device()
        rows = np.ascontiguousarray(x.T)
        dens = np.empty(g.shape)
        check(_lib.lib().gpemu_kde1d(int(_lib.resolve_device(device)), d, S, ptr(rows), int(g.shape[1]), ptr(g), ptr(h),
                                     ptr(dens)))
    return {"grid": g, "density": dens, "bandwidth": h}


def kde_2d(samples, pairs=None, covariance="full", bandwidth=None, shear=None, grid_a=None, grid_b=None, n_grid=100,
           cut=3.0, bw_adjust=1.0, device=None, workspace_bytes=0):
    """Gaussian kernel density of pairs of parameters of ``samples (S, d)``, the direct sum over all samples computed
    as a matrix product on the fp64 matrix cores: a dict of ``pairs (P, 2)``, ``shear (P,)``,
    ``bandwidth (P, 2)``, ``grid_a (P, G)``, ``grid_b (P, G)`` and ``density (P, G, G)`` (first axis: the pair's first
    parameter, as ``hist_2d``).  ``density[p][a][b]`` is the density at ``x_i = grid_a[p][a]``, ``x_j = grid_b[p][b] +
    shear[p] grid_a[p][a]`` (``kde_2d_mesh``).

    Defaults (``kde2d_plan``): all pairs ``i < j`` in ``pair_indices`` order; ``covariance="full"`` is
    ``scipy.stats.gaussian_kde`` of the pair (Scott's factor ``S ** (-1 / 6)`` times ``bw_adjust``, the full sample
    covariance) evaluated on the sheared grid; ``"diagonal"`` the axis-aligned product kernel with ``h = f std(ddof=1)``;
    the grids are ``linspace(min - cut h, max + cut h, n_grid)`` of x_i and of ``v = x_j - shear x_i``.  What is given
    is used as given: ``bandwidth`` ``(2,)`` or ``(P, 2)``, ``shear`` a number or ``(P,)``, the grids ``(G,)`` or ``(P,
    G)``, at most 512 points.  ``workspace_bytes`` bounds the partial tiles of a batch of pairs (0: half of the free
    device memory); the bits of the result do not depend on it.  A NaN sample makes the panels of its pairs NaN."""
    x, on_device = _samples(samples)
    S, d = int(x.shape[0]), int(x.shape[1])
    _check_shape(S, d)
    if d < 2:
        raise ValueError("a pair needs at least two parameters")
    kw = dict(pairs=pairs, covariance=covariance, bandwidth=bandwidth, shear=shear, grid_a=grid_a, grid_b=grid_b,
              n_grid=n_grid, cut=cut, bw_adjust=bw_adjust)
    if on_device:
        return _kde2d_view(DeviceRows.of_tensor(x), workspace_bytes, **kw)
    plan = kde2d_plan_host(x, **kw)
    _lib.require_device()
    P, G = plan["grid_a"].shape
    dens = np.empty((P, G, G))
    check(_lib.lib().gpemu_kde2d(int(_lib.resolve_device(device)), S, d, ptr(x), P, ptr(plan["pairs"]),
                                 ptr(plan["shear"]), ptr(plan["bandwidth"]), G, ptr(plan["grid_a"]),
                                 ptr(plan["grid_b"]), ptr(dens), int(workspace_bytes)))
    plan["density"] = dens
    return plan


KEYS = ("edges_1d", "edges_2d", "hist_1d", "pairs", "hist_2d", "n_inside", "confidence", "hpd", "kde_grid", "kde_density",
        "kde_bandwidth")
KEYS_KDE2D = ("kde2d_pairs", "kde2d_shear", "kde2d_bandwidth", "kde2d_grid_a", "kde2d_grid_b", "kde2d_density")


def assemble(hist, confidence, hpd, kde, kde2d=None):
    """The one dict of ``summary`` / ``DeviceSampler.marginals`` from its parts (``kde`` None: no ``kde_*`` keys;
    ``kde2d`` None: no ``kde2d_*`` keys)."""
    out = dict(hist)
    out["confidence"] = np.atleast_1d(np.asarray(confidence, dtype=np.float64))
    out["hpd"] = hpd
    if kde is not None:
        out["kde_grid"], out["kde_density"], out["kde_bandwidth"] = kde["grid"], kde["density"], kde["bandwidth"]
    if kde2d is not None:
        for key in KEYS_KDE2D:
            out[key] = kde2d[key[len("kde2d_"):]]
    return out


def summary(samples, lower, upper, bins_1d=100, bins_2d=50, confidence=(0.9,), kde=True, n_grid=200, device=None,
            kde2d=False, n_grid_2d=100, covariance_2d="full"):
    """``histograms``, ``hpd_intervals`` (``hpd (n_levels, d, 2)`` for ``confidence (n_levels,)``), with ``kde``
    ``kde_1d`` (``kde_grid``, ``kde_density``, ``kde_bandwidth``) and, with ``kde2d``, ``kde_2d`` of all pairs on
    ``n_grid_2d`` points per axis (``KEYS_KDE2D``: ``kde2d_pairs``, ``kde2d_shear``, ``kde2d_bandwidth``,
    ``kde2d_grid_a``, ``kde2d_grid_b``, ``kde2d_density``) of ``samples (S, d)`` in one dict."""
    conf = np.atleast_1d(np.asarray(confidence, dtype=np.float64))
    hist = histograms(samples, lower, upper, bins_1d, bins_2d, device=device)
    hpd = hpd_intervals(samples, conf, device=device)
    dens = kde_1d(samples, n_grid=n_grid, device=device) if kde else None
    dens2 = kde_2d(samples, covariance=covariance_2d, n_grid=n_grid_2d, device=device) if kde2d else None
    return assemble(hist, conf, hpd, dens, dens2)


def summary_view(rows, lower, upper, bins_1d=100, bins_2d=50, confidence=(0.9,), kde=True, n_grid=200, kde2d=False,
                 n_grid_2d=100, covariance_2d="full"):
    """``summary`` of ``DeviceRows`` where they lie (``DeviceSampler.marginals``): the histograms and the 2-D densities
    read them in place, the sort and the 1-D density ``rows.columns()``, which is released before the 2-D densities run."""
    device, d, S = rows.device, rows.d, rows.rows
    if not (1 <= int(bins_1d) <= MAX_BINS_1D and 1 <= int(bins_2d) <= MAX_BINS_2D):
        raise ValueError(f"bins_1d must be in [1, {MAX_BINS_1D}] and bins_2d in [1, {MAX_BINS_2D}]")
    e1, e2 = bin_edges(lower, upper, bins_1d), bin_edges(lower, upper, bins_2d)
    if e1.shape[0] != d:
        raise ValueError(f"the box has {e1.shape[0]} parameters, the sampler {d}")
    conf = np.atleast_1d(np.asarray(confidence, dtype=np.float64))
    n_out = n_outside(conf, S)
    h1, h2, ni = _hist_dev(device, *rows.layout, d, e1, e2)
    hist = {"edges_1d": e1, "edges_2d": e2, "hist_1d": h1, "pairs": pair_indices(d), "hist_2d": h2, "n_inside": ni}
    cols = rows.columns()
    # one sort serves the intervals and, as the level n_out = 1 (window 0: smallest, largest), the density's support
    ends = _hpd_dev(device, cols.address, S, d, np.append(n_out, 1) if kde else n_out)
    dens = None
    if kde:
        def spread():
            _, var = _moments_dev(device, cols.address, S, d)
            return np.sqrt(var * (S / max(S - 1.0, 1.0))), ends[-1, :, 0], ends[-1, :, 1]
        h, g = _kde_plan(S, d, None, None, n_grid, 3.0, spread)
        dens = {"grid": g, "density": _kde_dev(device, cols.address, S, d, g, h), "bandwidth": h}
    del cols        # (the dense copy, where one was made)
    if kde2d and d < 2:
        raise ValueError("kde2d needs at least two parameters")
    dens2 = _kde2d_view(rows, covariance=covariance_2d, n_grid=n_grid_2d) if kde2d else None
    return assemble(hist, conf, ends[:n_out.size], dens, dens2)
