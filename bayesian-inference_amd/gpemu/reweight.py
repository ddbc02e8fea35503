"""Importance reweighting of a stored chain and weighted summaries on the device.

The log-posterior takes constant priors inside a box (ref: log_posterior.py:97), while the reference's own prior sampler
draws ``c_1, c_2, c_3`` with a uniform logarithm (ref: plot_qhat.py:298-326).  What does the posterior look like under
the prior one believes, or under an updated measurement?  The stored chain answers without a second run: its samples
are importance-reweighted to the new target, Pareto smoothing (``gpemu.loo``) stabilises the ratios and its k-hat says
when the answer cannot be trusted, and every chain summary has a weighted form:

* ``log_ratio``: the log of the new target over the old for every sample and scenario -- a prior scenario (kinds
  ``flat``, ``log_uniform``, ``normal``, ``log_normal`` per parameter, inside the sampler's box), a data scenario (the
  sampler's models against models with another ``likelihood_setup``), or their sum;
* ``weights``: normalised log-weights (PSIS, or raw with ``smooth=False``), ``pareto_k``, ``ess_w``, ``log_mean_ratio``;
* ``fixed_weights``: the weights as integers ``q = rint(w 2^52)``, so that every weighted sum is exact;
* ``weighted_quantile``, ``weighted_histograms``: the inverted weighted ECDF and ``np.histogram(weights=q)``, exact;
* ``weighted_hpd``, ``weighted_kde_1d``: the highest-density intervals by value under the weights,
  exact, and the Gaussian kernel density with ``scipy.stats.gaussian_kde(x, weights=w)``'s bandwidth;
* ``summary``: one dict per scenario (``hpd=``, ``kde=`` add the two above).

Samples are ``(S, d)``: numpy arrays go through the host entries, contiguous float64 device tensors are read in place.
There is no CPU implementation."""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction

import numpy as np

from . import _lib
from ._lib import check, ptr
from .rows import DeviceRows

PATHS = ("LOGPRIOR", "QUANTISE", "LOGSUMEXP", "WSEL_HIST_PASS", "WSEL_SCAN", "WHIST_SWEEP", "WHIST_PAIR_GROUP")
KINDS = {"flat": 0, "log_uniform": 1, "normal": 2, "log_normal": 3}
MAX_D, MAX_SCENARIOS = 16, 64
MAX_BINS_1D, MAX_BINS_2D = 4096, 256
ONE = 1 << 52   # the fixed-point unit of the weights
# enum gpemu_wsummary_path
WSUMMARY_PATHS = ("BANDS_WHOLE", "BANDS_FEATURE_BLOCKED", "ROW_REDUCE", "SELECT_PASS", "HPD_SORT_BATCH", "HPD_PLACE",
                  "HPD_SCAN", "HPD_WINDOW", "KDE")


def path_counts():
    """The library's counters of these launches since the process started, by name."""
    out = (C.c_int64 * len(PATHS))()
    n = _lib.lib().gpemu_reweight_path_counts(out, len(PATHS))
    if n < 0:
        check(n)
    return {k: int(out[i]) for i, k in enumerate(PATHS)}


def wsummary_path_counts():
    """The library's counters of the weighted bands, intervals and densities since the process started, by name."""
    out = (C.c_int64 * len(WSUMMARY_PATHS))()
    n = _lib.lib().gpemu_wsummary_path_counts(out, len(WSUMMARY_PATHS))
    if n < 0:
        check(n)
    return {k: int(out[i]) for i, k in enumerate(WSUMMARY_PATHS)}


# -- host-side rules --------------------------------------------------------------------------------------------------
def _entry(e):
    """One parameter's prior as ``(kind, a, b)``: ``None``, a kind (number or name), ``(kind, a, b)`` or a dict with
    ``kind`` and, for kinds 2 / 3, ``a``, ``b``."""
    if e is None:
        return 0, 0.0, 1.0
    if isinstance(e, dict):
        extra = set(e) - {"kind", "a", "b"}
        if extra:
            raise ValueError(f"a prior takes kind, a and b; {sorted(extra)} is not supported (the new prior keeps the "
                             "sampler's box: a narrower box or a truncation needs its own run)")
        if "kind" not in e:
            raise ValueError("a prior needs a kind")
        e = (e["kind"], e.get("a"), e.get("b"))
    if isinstance(e, (str, int, np.integer)):
        e = (e, None, None)
    if not isinstance(e, (tuple, list)) or len(e) != 3:
        raise ValueError(f"cannot read the prior {e!r}")
    kind, a, b = e
    if isinstance(kind, str):
        if kind not in KINDS:
            raise ValueError(f"unknown prior kind {kind!r}: one of {sorted(KINDS)}")
        kind = KINDS[kind]
    if isinstance(kind, bool) or int(kind) != kind or not 0 <= int(kind) <= 3:
        raise ValueError(f"unknown prior kind {kind!r}")
    kind = int(kind)
    if kind < 2:
        return kind, 0.0, 1.0
    if a is None or b is None:
        raise ValueError("a normal or log-normal prior needs a and b")
    a, b = float(a), float(b)
    if not (math.isfinite(a) and math.isfinite(b) and b > 0.0):
        raise ValueError("a must be finite, b finite and > 0")
    return kind, a, b


def check_priors(spec, d, lower, upper):
    """The scenario tables ``(kind (R, d) int32, a (R, d), b (R, d))`` of ``spec``: a list of scenarios, each a list of
    ``d`` priors (see ``_entry``) or a dict ``{parameter index: prior}`` whose other parameters stay flat.  ValueError
    for ``b <= 0``, a non-finite parameter, a log prior on a parameter whose lower bound is not > 0, more than 64
    scenarios, and for anything that narrows the box."""
    lo, hi = np.atleast_1d(np.asarray(lower, dtype=np.float64)), np.atleast_1d(np.asarray(upper, dtype=np.float64))
    d = int(d)
    if not 1 <= d <= MAX_D:
        raise ValueError(f"d must be in [1, {MAX_D}], got {d}")
    if lo.shape != (d,) or hi.shape != (d,) or not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(hi > lo)):
        raise ValueError(f"the box must be two finite vectors of length {d} with upper > lower")
    if isinstance(spec, (str, bytes)) or not hasattr(spec, "__len__") or len(spec) == 0:
        raise ValueError("priors must be a non-empty list of scenarios")
    if len(spec) > MAX_SCENARIOS:
        raise ValueError(f"at most {MAX_SCENARIOS} scenarios per call, got {len(spec)}")
    R = len(spec)
    kind, a, b = np.zeros((R, d), dtype=np.int32), np.zeros((R, d)), np.ones((R, d))
    for r, sc in enumerate(spec):
        if isinstance(sc, dict):
            row = [None] * d
            for i, e in sc.items():
                if isinstance(i, bool) or int(i) != i or not 0 <= int(i) < d:
                    raise IndexError(f"scenario {r} names parameter {i!r}, outside [0, {d})")
                row[int(i)] = e
        else:
            row = list(sc)
            if len(row) != d:
                raise ValueError(f"scenario {r} has {len(row)} priors for {d} parameters")
        for i, e in enumerate(row):
            kind[r, i], a[r, i], b[r, i] = _entry(e)
            if kind[r, i] in (1, 3) and not lo[i] > 0.0:
                raise ValueError(f"scenario {r}: a log-uniform or log-normal prior on parameter {i} needs a lower bound "
                                 f"> 0, the box has {lo[i]}")
    return kind, a, b


def reference_prior(names):
    """One scenario: log-uniform (kind 1) for every parameter whose name contains ``c_``, flat otherwise -- the rule of
    the reference's prior sampler (ref: plot_qhat.py:313-316)."""
    return [1 if "c_" in str(n) else 0 for n in names]


def targets(p, Q):
    """The integer targets ``t = max(1, ceil(p Q))`` of probabilities ``p (nq,)`` for total weights ``Q (R,)``, in exact
    rational arithmetic: ``(R, nq)`` uint64."""
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    if p.ndim != 1 or p.size == 0 or not np.all((p >= 0.0) & (p <= 1.0)):
        raise ValueError("probabilities must be a non-empty vector in [0, 1]")
    Qs = [int(v) for v in np.atleast_1d(Q)]
    if any(v < 1 for v in Qs):
        raise ValueError("every total weight must be >= 1")
    out = np.empty((len(Qs), p.size), dtype=np.uint64)
    for r, Qr in enumerate(Qs):
        for i, pi in enumerate(p):
            out[r, i] = max(1, math.ceil(Fraction(float(pi)) * Qr))
    return out


def weighted_bandwidth(var_w, n_eff):
    """``scipy.stats.gaussian_kde(x, weights=w)``'s default bandwidth for 1-D data: ``n_eff ** (-1 / 5)`` times the square
    root of the unbiased weighted variance ``var_w / (1 - sum w^2)``, with ``var_w = sum_s w_s (x_s - mean_w)^2`` for
    normalised weights and ``n_eff = 1 / sum w^2`` (``ess_w``).  Broadcasts; ``n_eff <= 1`` (one sample carries all the
    weight) gives NaN."""
    var_w, n_eff = np.asarray(var_w, dtype=np.float64), np.asarray(n_eff, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        unbiased = var_w / (1.0 - 1.0 / n_eff)
        h = np.power(n_eff, -1.0 / 5.0) * np.sqrt(unbiased)
    return np.where(n_eff > 1.0, h, np.nan)


def _log_diff_ndtr(zl, zu):
    """``log(Phi(zu) - Phi(zl))``, zl < zu, from ``log_ndtr`` differences taken in the tail where they are accurate."""
    from scipy.special import log_ndtr
    if zl > 0.0:
        zl, zu = -zu, -zl
    hi, lo = float(log_ndtr(zu)), float(log_ndtr(zl))
    return hi + math.log1p(-math.exp(lo - hi))


def log_prior_norm(kind, a, b, lower, upper):
    """``log`` of the integral over the box of the unnormalised new prior ``exp(sum_i f_i)`` per scenario, ``(R,)``:
    closed form for kinds 0 and 1, ``scipy.special.log_ndtr`` differences for kinds 2 and 3.  With the volume of the
    box, ``log_mean_ratio + log V - log_prior_norm`` is the log Bayes factor between the two normalised priors."""
    kind, a, b = np.atleast_2d(kind), np.atleast_2d(a), np.atleast_2d(b)
    lo, hi = np.atleast_1d(np.asarray(lower, dtype=np.float64)), np.atleast_1d(np.asarray(upper, dtype=np.float64))
    out = np.zeros(kind.shape[0])
    for r in range(kind.shape[0]):
        for i in range(kind.shape[1]):
            k, ai, bi, l, u = int(kind[r, i]), float(a[r, i]), float(b[r, i]), float(lo[i]), float(hi[i])
            if k == 0:
                out[r] += math.log(u - l)
            elif k == 1:
                out[r] += math.log(math.log(u / l))
            elif k == 2:
                out[r] += math.log(bi) + 0.5 * math.log(2.0 * math.pi) + _log_diff_ndtr((l - ai) / bi, (u - ai) / bi)
            else:
                out[r] += (math.log(bi) + 0.5 * math.log(2.0 * math.pi)
                           + _log_diff_ndtr((math.log(l) - ai) / bi, (math.log(u) - ai) / bi))
    return out


# -- device wrappers --------------------------------------------------------------------------------------------------
def _samples(samples):
    """``(array or tensor (S, d), on_device)``; a vector is one parameter."""
    if _lib.is_device_tensor(samples):
        import torch
        if samples.dtype != torch.float64 or samples.dim() not in (1, 2):
            raise TypeError("device samples must be a float64 tensor (S, d)")
        return samples.reshape(samples.shape[0], -1).contiguous(), True
    x = np.asarray(samples, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    if x.ndim != 2 or x.shape[0] < 1 or not 1 <= x.shape[1] <= MAX_D:
        raise ValueError(f"samples must be (S, d) with S >= 1 and d in [1, {MAX_D}]")
    return np.ascontiguousarray(x), False


def _rows(L):
    """``(matrix (R, S), on_device)``; a vector is one row."""
    if _lib.is_device_tensor(L):
        return L.reshape(-1, L.shape[-1]).contiguous(), True
    t = np.asarray(L)
    if t.ndim == 1:
        t = t[None, :]
    if t.ndim != 2 or t.shape[1] < 1:
        raise ValueError("expected a matrix (R, S) with S >= 1")
    return np.ascontiguousarray(t), False


def _to_device(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", int(device)))


def _q_tensor(q, device):
    """The weights as an int64 device tensor (the bits of the uint64 values, all below 2^53)."""
    if _lib.is_device_tensor(q):
        return q.reshape(-1, q.shape[-1]).contiguous()
    return _to_device(np.ascontiguousarray(np.atleast_2d(q), dtype=np.uint64).view(np.int64), device)


def log_prior_dev(device, base, n_blocks, block_rows, block_stride_rows, d, tables, lower):
    """The log-ratios of the prior scenarios ``tables = (kind, a, b)`` for device rows in the block layout: a device
    tensor ``(R, S)``."""
    import torch
    kind, a, b = (np.ascontiguousarray(t) for t in tables)
    R, S = int(kind.shape[0]), int(n_blocks) * int(block_rows)
    lo = np.ascontiguousarray(lower, dtype=np.float64)
    out = torch.empty((R, S), dtype=torch.float64, device=torch.device("cuda", int(device)))
    check(_lib.lib().gpemu_logprior_dev(int(device), C.c_void_p(base), int(n_blocks), int(block_rows),
                                        int(block_stride_rows), int(d), R, ptr(kind.astype(np.int32)), ptr(a), ptr(b),
                                        ptr(lo), C.c_void_p(out.data_ptr()), S, _lib.current_stream(device)))
    return out


def logmeanexp_dev(L, normalise=False):
    """``log mean exp`` of every row of the device tensor ``L (R, S)``, ``(R,)`` numpy, from the fixed-tree log-sum-exp;
    with ``normalise`` also ``L - logsumexp(L)`` as a device tensor."""
    import torch
    L, _ = _rows(L)
    R, S = int(L.shape[0]), int(L.shape[1])
    device = L.device.index or 0
    lme = torch.empty((R,), dtype=torch.float64, device=L.device)
    lw = torch.empty((R, S), dtype=torch.float64, device=L.device) if normalise else None
    check(_lib.lib().gpemu_logmeanexp_dev(device, R, S, C.c_void_p(L.data_ptr()), S, C.c_void_p(lme.data_ptr()),
                                          C.c_void_p(lw.data_ptr()) if normalise else None, _lib.current_stream(device)))
    return (lme.cpu().numpy(), lw) if normalise else lme.cpu().numpy()


def fixed_weights_dev(log_weights):
    """``(q, Q)`` of the device tensor ``log_weights (R, S)``: ``q = rint(exp(lw) 2^52)`` as an int64 device tensor (the
    values are below 2^53) and the exact row sums ``Q (R,)`` as numpy uint64."""
    import torch
    lw, _ = _rows(log_weights)
    R, S = int(lw.shape[0]), int(lw.shape[1])
    device = lw.device.index or 0
    q = torch.empty((R, S), dtype=torch.int64, device=lw.device)
    Q = torch.empty((R,), dtype=torch.int64, device=lw.device)
    check(_lib.lib().gpemu_weights_fixed_dev(device, R, S, C.c_void_p(lw.data_ptr()), S, C.c_void_p(q.data_ptr()), S,
                                             C.c_void_p(Q.data_ptr()), _lib.current_stream(device)))
    return q, Q.cpu().numpy().view(np.uint64)


def weighted_quantile_dev(device, base, R_v, S, row_stride, elem_stride, q, tgt, workspace_bytes=0):
    """The elements that answer the targets ``tgt (R_w, nt)`` uint64 in the ``R_v`` device rows (element j of row v at
    ``base + 8 (v row_stride + j elem_stride)``) under the int64 device tensor ``q (R_w, S)``: numpy ``(R_w, R_v, nt)``."""
    import torch
    tgt = np.ascontiguousarray(tgt, dtype=np.uint64)
    R_w, nt = int(q.shape[0]), int(tgt.shape[1])
    if tgt.shape[0] != R_w or int(q.shape[1]) != int(S):
        raise ValueError("the targets and the weights must have one row per weight row, the weights S columns")
    out = torch.empty((R_w, int(R_v), nt), dtype=torch.float64, device=q.device)
    check(_lib.lib().gpemu_weighted_select_dev(int(device), int(R_v), int(S), C.c_void_p(base), int(row_stride),
                                               int(elem_stride), R_w, C.c_void_p(q.data_ptr()), int(S), nt, ptr(tgt),
                                               C.c_void_p(out.data_ptr()), int(workspace_bytes),
                                               _lib.current_stream(device)))
    return out.cpu().numpy()


def weighted_hist_dev(device, base, n_blocks, block_rows, block_stride_rows, d, q, e1, e2, group_bins=0):
    """The weighted histograms of device rows in the block layout under ``q (R_w, S)``: ``(hist_1d (R_w, d, nb1),
    hist_2d (R_w, n_pairs, nb2, nb2), w_inside (R_w, d))`` as numpy uint64."""
    import torch
    nb1, nb2, npairs, R_w = e1.shape[1] - 1, e2.shape[1] - 1, d * (d - 1) // 2, int(q.shape[0])
    S = int(n_blocks) * int(block_rows)
    if int(q.shape[1]) != S:
        raise ValueError(f"the weights have {int(q.shape[1])} columns, the rows are {S}")
    h1 = torch.empty((R_w, d, nb1), dtype=torch.int64, device=q.device)
    h2 = torch.empty((R_w, max(npairs, 1), nb2, nb2), dtype=torch.int64, device=q.device)
    wi = torch.empty((R_w, d), dtype=torch.int64, device=q.device)
    check(_lib.lib().gpemu_weighted_hist_dev(int(device), C.c_void_p(base), int(n_blocks), int(block_rows),
                                             int(block_stride_rows), int(d), R_w, C.c_void_p(q.data_ptr()), S, int(nb1),
                                             ptr(e1), int(nb2), ptr(e2), int(group_bins), C.c_void_p(h1.data_ptr()),
                                             C.c_void_p(h2.data_ptr()) if npairs else None, C.c_void_p(wi.data_ptr()),
                                             _lib.current_stream(device)))
    u = lambda t: t.cpu().numpy().view(np.uint64)
    return u(h1), u(h2[:, :npairs].contiguous()), u(wi)


def weighted_hpd_dev(device, base, R_v, S, row_stride, elem_stride, q, tgt, workspace_bytes=0):
    """The highest-density intervals of target masses ``tgt (R_w, n_levels)`` uint64 of the ``R_v`` device rows (addressed
    as ``weighted_quantile_dev``'s) under the int64 device tensor ``q (R_w, S)``: numpy ``(R_w, R_v, n_levels, 2)``."""
    import torch
    tgt = np.ascontiguousarray(tgt, dtype=np.uint64)
    R_w, nl = int(q.shape[0]), int(tgt.shape[1])
    if tgt.shape[0] != R_w or int(q.shape[1]) != int(S):
        raise ValueError("the targets and the weights must have one row per weight row, the weights S columns")
    out = torch.empty((R_w, int(R_v), nl, 2), dtype=torch.float64, device=q.device)
    ctx = _lib.call_ctx(device, workspace_bytes)
    check(_lib.lib().gpemu_weighted_hpd_dev(int(device), int(R_v), int(S), C.c_void_p(base), int(row_stride),
                                            int(elem_stride), R_w, C.c_void_p(q.data_ptr()), int(S), nl, ptr(tgt),
                                            C.c_void_p(out.data_ptr()), C.byref(ctx)))
    return out.cpu().numpy()


def weighted_kde_dev(device, base, R_v, S, row_stride, elem_stride, q, grid, h):
    """The weighted densities of the ``R_v`` device rows under ``q (R_w, S)`` on ``grid (R_w, R_v, G)`` with bandwidths
    ``h (R_w, R_v)``: numpy ``(R_w, R_v, G)``."""
    import torch
    grid, h = np.ascontiguousarray(grid, dtype=np.float64), np.ascontiguousarray(h, dtype=np.float64)
    R_w, G = int(q.shape[0]), int(grid.shape[-1])
    if grid.shape != (R_w, int(R_v), G) or h.shape != (R_w, int(R_v)) or int(q.shape[1]) != int(S):
        raise ValueError("grid must be (R_w, R_v, G), h (R_w, R_v) and the weights (R_w, S)")
    out = torch.empty((R_w, int(R_v), G), dtype=torch.float64, device=q.device)
    ctx = _lib.call_ctx(device)
    check(_lib.lib().gpemu_weighted_kde1d_dev(int(device), int(R_v), int(S), C.c_void_p(base), int(row_stride),
                                              int(elem_stride), R_w, C.c_void_p(q.data_ptr()), int(S), G, ptr(grid), ptr(h),
                                              C.c_void_p(out.data_ptr()), C.byref(ctx)))
    return out.cpu().numpy()


# -- public functions -------------------------------------------------------------------------------------------------
def _box(lower, upper, d):
    lo, hi = np.atleast_1d(np.asarray(lower, dtype=np.float64)), np.atleast_1d(np.asarray(upper, dtype=np.float64))
    if lo.shape != (d,) or hi.shape != (d,):
        raise ValueError(f"the box must be two vectors of length {d}")
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


def data_log_ratio_dev(models_old, models_new, rows, chain=0):
    """The data scenario's log-ratio of the ``DeviceRows`` ``rows``, a device tensor ``(1, S)``: the pointwise terms of
    both lists of models (``gpemu.loo.pointwise_dev``), each summed in row order on the device, then subtracted once."""
    from . import loo as LO
    S, sums = rows.rows, []
    for models in (models_new, models_old):
        T = LO.pointwise_dev(models, rows, chain)
        sums.append(LO.group_rows_dev(rows.device, T.data_ptr(), int(T.shape[0]), S, S, [list(range(int(T.shape[0])))]))
    return sums[0] - sums[1]


def log_ratio(samples, priors=None, lower=None, upper=None, models_old=None, models_new=None, chain=0, device=None):
    """``(R, S)``: the log of the new target over the old for the rows of ``samples (S, d)``.  ``priors``: a list of
    scenarios (``check_priors``) inside the box ``lower``, ``upper``; ``models_old`` / ``models_new``: the sampler's
    models and the same emulators with another ``likelihood_setup`` -- one row, or with ``priors`` added to every prior
    scenario.  A numpy array for numpy samples, a device tensor for a device tensor."""
    x, on_device = _samples(samples)
    S, d = int(x.shape[0]), int(x.shape[1])
    if priors is None and models_new is None:
        raise ValueError("pass priors, models_new or both")
    if (models_new is None) != (models_old is None):
        raise ValueError("a data scenario needs models_old and models_new")
    L = None
    if priors is not None:
        if lower is None or upper is None:
            raise ValueError("a prior scenario needs the sampler's box: pass lower and upper")
        lo, hi = _box(lower, upper, d)
        kind, a, b = check_priors(priors, d, lo, hi)
        if on_device:
            L = log_prior_dev(x.device.index or 0, x.data_ptr(), 1, S, S, d, (kind, a, b), lo)
        else:
            _lib.require_device()
            L = np.empty((kind.shape[0], S))
            check(_lib.lib().gpemu_logprior(int(_lib.resolve_device(device)), S, d, ptr(x), int(kind.shape[0]), ptr(kind),
                                            ptr(a), ptr(b), ptr(lo), ptr(L)))
    if models_new is not None:
        first = models_old[0] if isinstance(models_old, (list, tuple)) else models_old
        dx = x if on_device else _to_device(x, first.device)
        D = data_log_ratio_dev(models_old, models_new, DeviceRows.of_tensor(dx), chain)
        if L is None:
            L = D if on_device else D.cpu().numpy()
        else:
            L = L + D if on_device else L + D.cpu().numpy()
    return L


def weights(log_ratio, smooth=True, r_eff=None, device=None, workspace_bytes=0):
    """The importance weights of ``log_ratio (R, S)``: a dict of ``log_weights (R, S)`` (normalised; numpy or a device
    tensor as the input), ``pareto_k``, ``ess_w = 1 / sum w^2`` and ``log_mean_ratio = logsumexp(l) - log S`` (raw), each
    ``(R,)``.  ``smooth``: Pareto-smoothed by ``gpemu.loo.psis`` on ``V = -l``; else ``l - logsumexp(l)`` and ``pareto_k``
    NaN.  A row with a NaN or an infinity gives NaN."""
    from . import loo as LO
    L, on_device = _rows(log_ratio)
    R = int(L.shape[0])
    if not on_device:
        _lib.require_device()
        L = np.ascontiguousarray(L, dtype=np.float64)
    dL = L if on_device else _to_device(L, _lib.resolve_device(device))
    if smooth:
        st = LO.psis(-L, r_eff=r_eff, return_weights=True, device=device, workspace_bytes=workspace_bytes)
        lw, k, ess = st["log_weights"], st["pareto_k"], st["ess_w"]
        lme = logmeanexp_dev(dL)
    else:
        lme, dlw = logmeanexp_dev(dL, normalise=True)
        ess = np.exp(-(logmeanexp_dev(dlw * 2.0) + math.log(int(L.shape[1]))))
        lw, k = (dlw if on_device else dlw.cpu().numpy()), np.full(R, np.nan)
    return {"log_weights": lw, "pareto_k": np.asarray(k), "ess_w": np.asarray(ess), "log_mean_ratio": lme}


def fixed_weights(log_weights, device=None):
    """``(q (R, S), Q (R,))``: the weights as integers ``rint(exp(lw) 2^52)`` and their exact row sums, uint64 numpy
    arrays for numpy input; for a device tensor ``q`` is an int64 device tensor (the same bits)."""
    lw, on_device = _rows(log_weights)
    if on_device:
        return fixed_weights_dev(lw)
    _lib.require_device()
    q, Q = fixed_weights_dev(_to_device(np.ascontiguousarray(lw, dtype=np.float64), _lib.resolve_device(device)))
    return q.cpu().numpy().view(np.uint64), Q


def _totals(q):
    if _lib.is_device_tensor(q):
        return q.sum(dim=-1).cpu().numpy().view(np.uint64)
    return np.atleast_2d(q).astype(np.uint64).sum(axis=-1, dtype=np.uint64)


def weighted_quantile(values, probabilities, q, Q=None, device=None, workspace_bytes=0):
    """The weighted quantiles of every column of ``values (S, d)`` under every row of the fixed-point weights
    ``q (R_w, S)``: ``(R_w, nq, d)``, for probability ``p`` the smallest sample value ``v`` with ``sum_{x_s <= v} q_s >=
    max(1, ceil(p Q))`` -- the inverted weighted ECDF, always an element of the input.  ``Q``: the row sums of ``q`` (from
    ``fixed_weights``; recomputed when not given)."""
    x, on_device = _samples(values)
    S, d = int(x.shape[0]), int(x.shape[1])
    tgt = targets(probabilities, _totals(q) if Q is None else Q)
    if on_device:
        dq = _q_tensor(q, x.device.index or 0)
        out = weighted_quantile_dev(x.device.index or 0, x.data_ptr(), d, S, 1, d, dq, tgt, workspace_bytes)
    else:
        _lib.require_device()
        qh = np.ascontiguousarray(np.atleast_2d(q), dtype=np.uint64)
        if qh.shape[1] != S or tgt.shape[0] != qh.shape[0]:
            raise ValueError(f"the weights must be (R_w, {S})")
        out = np.empty((qh.shape[0], d, tgt.shape[1]))
        check(_lib.lib().gpemu_weighted_select(int(_lib.resolve_device(device)), d, S, ptr(np.ascontiguousarray(x.T)),
                                               int(qh.shape[0]), ptr(qh), int(tgt.shape[1]), ptr(tgt), ptr(out)))
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def weighted_histograms(samples, lower, upper, q, bins_1d=100, bins_2d=50, device=None, group_bins=0):
    """``gpemu.marginals.histograms`` with the fixed-point weights ``q (R_w, S)`` added where it counts one: a dict of
    ``edges_1d``, ``edges_2d``, ``pairs``, ``hist_1d_q (R_w, d, bins_1d)``, ``hist_2d_q (R_w, n_pairs, bins_2d, bins_2d)``
    and ``w_inside (R_w, d)``, uint64: ``np.histogram(x[:, j], bins=edges_1d[j], weights=q[w])`` exactly."""
    from . import marginals as M
    x, on_device = _samples(samples)
    S, d = int(x.shape[0]), int(x.shape[1])
    if not (1 <= int(bins_1d) <= MAX_BINS_1D and 1 <= int(bins_2d) <= MAX_BINS_2D):
        raise ValueError(f"bins_1d must be in [1, {MAX_BINS_1D}] and bins_2d in [1, {MAX_BINS_2D}]")
    e1, e2 = M.bin_edges(lower, upper, bins_1d), M.bin_edges(lower, upper, bins_2d)
    if e1.shape[0] != d:
        raise ValueError(f"the box has {e1.shape[0]} parameters, the samples {d}")
    if on_device:
        dq = _q_tensor(q, x.device.index or 0)
        h1, h2, wi = weighted_hist_dev(x.device.index or 0, x.data_ptr(), 1, S, S, d, dq, e1, e2, group_bins)
    else:
        _lib.require_device()
        qh = np.ascontiguousarray(np.atleast_2d(q), dtype=np.uint64)
        if qh.shape[1] != S:
            raise ValueError(f"the weights must be (R_w, {S})")
        R_w, npairs = int(qh.shape[0]), d * (d - 1) // 2
        h1 = np.empty((R_w, d, int(bins_1d)), dtype=np.uint64)
        h2 = np.empty((R_w, npairs, int(bins_2d), int(bins_2d)), dtype=np.uint64)
        wi = np.empty((R_w, d), dtype=np.uint64)
        check(_lib.lib().gpemu_weighted_hist(int(_lib.resolve_device(device)), S, d, ptr(x), R_w, ptr(qh), int(bins_1d),
                                             ptr(e1), int(bins_2d), ptr(e2), int(group_bins), ptr(h1),
                                             ptr(h2) if npairs else None, ptr(wi)))
    return {"edges_1d": e1, "edges_2d": e2, "pairs": M.pair_indices(d), "hist_1d_q": h1, "hist_2d_q": h2, "w_inside": wi}


def weighted_hpd(values, confidence, q, Q=None, device=None, workspace_bytes=0):
    """The highest-density intervals by value of every column of ``values (S, d)`` under every row of the fixed-point
    weights ``q (R_w, S)``: ``(R_w, n_levels, d, 2)``.  For confidence ``c`` the target mass is ``t = max(1, ceil(c Q))``
    (``targets``); over every sample value ``a``, with ``b(a)`` the smallest sample value ``>= a`` whose closed interval
    holds weight ``>= t``, the ``(a, b(a))`` of the smallest width ``b - a``, equal widths to the smaller ``a``.  Both
    ends are elements of the input.  NaN for a column with a NaN or an infinite extreme."""
    x, on_device = _samples(values)
    S, d = int(x.shape[0]), int(x.shape[1])
    tgt = targets(confidence, _totals(q) if Q is None else Q)
    if on_device:
        dq = _q_tensor(q, x.device.index or 0)
        out = weighted_hpd_dev(x.device.index or 0, x.data_ptr(), d, S, 1, d, dq, tgt, workspace_bytes)
    else:
        _lib.require_device()
        qh = np.ascontiguousarray(np.atleast_2d(q), dtype=np.uint64)
        if qh.shape[1] != S or tgt.shape[0] != qh.shape[0]:
            raise ValueError(f"the weights must be (R_w, {S})")
        out = np.empty((qh.shape[0], d, tgt.shape[1], 2))
        check(_lib.lib().gpemu_weighted_hpd(int(_lib.resolve_device(device)), d, S, ptr(np.ascontiguousarray(x.T)),
                                            int(qh.shape[0]), ptr(qh), int(tgt.shape[1]), ptr(tgt), ptr(out)))
    return np.ascontiguousarray(out.transpose(0, 2, 1, 3))


def _kde_plan(var_w, n_eff, xmin, xmax, R_w, d, grid, bandwidth, n_grid, cut):
    """Bandwidths ``(R_w, d)`` and grids ``(R_w, d, G)`` of the weighted densities: as given (a number, ``(d,)`` or
    ``(R_w, d)``; ``(G,)``, ``(d, G)`` or ``(R_w, d, G)``), else ``weighted_bandwidth`` and seaborn's support."""
    from . import marginals as M
    if bandwidth is None:
        h = weighted_bandwidth(var_w, np.asarray(n_eff, dtype=np.float64).reshape(-1, 1))
    else:
        h = np.broadcast_to(np.asarray(bandwidth, dtype=np.float64), (R_w, d)).copy()
    if not np.all(np.isfinite(h) & (h > 0.0)):
        raise ValueError(f"every bandwidth must be finite and > 0, got {h} (the default needs an effective sample size "
                         "above 1 and a positive weighted variance)")
    if grid is None:
        if int(n_grid) < 1:
            raise ValueError("n_grid must be >= 1")
        if not (np.all(np.isfinite(xmin)) and np.all(np.isfinite(xmax))):
            raise ValueError("the default grid needs finite samples")
        g = np.stack([M.default_grid(xmin, xmax, h[w], n_grid, cut) for w in range(R_w)])
    else:
        g = np.asarray(grid, dtype=np.float64)
        if g.ndim < 1 or g.ndim > 3 or g.shape[-1] < 1:
            raise ValueError(f"grid must be (G,), ({d}, G) or ({R_w}, {d}, G)")
        g = np.broadcast_to(g, (R_w, d, g.shape[-1])).copy()
    return np.ascontiguousarray(h), np.ascontiguousarray(g)


def weighted_kde_1d(values, q, log_weights=None, grid=None, bandwidth=None, n_grid=200, cut=3.0, Q=None, device=None):
    """The Gaussian kernel density of every column of ``values (S, d)`` under every row of the fixed-point weights
    ``q (R_w, S)``, ``1 / (Q h sqrt(2 pi)) sum_s q_s exp(-(grid - x_s)^2 / (2 h^2))`` as a direct sum: a dict of ``grid
    (R_w, d, G)``, ``density (R_w, d, G)`` and ``bandwidth (R_w, d)``.  ``bandwidth``: default ``weighted_bandwidth``,
    ``scipy.stats.gaussian_kde(x, weights=w)``'s rule, from the weighted variance of ``gpemu.loo.weighted_moments_dev``
    under ``log_weights (R_w, S)`` (the normalised log-weights ``q`` was made from; default ``log(q / Q)``) and ``n_eff =
    1 / sum w^2``; ``grid``: default ``linspace(min - cut h, max + cut h, n_grid)`` over all samples."""
    import torch
    from . import loo as LO
    x, on_device = _samples(values)
    S, d = int(x.shape[0]), int(x.shape[1])
    Q = _totals(q) if Q is None else np.atleast_1d(Q)
    if np.any(np.asarray(Q) == 0):
        raise ValueError("a weight row is all zero")
    dev = (x.device.index or 0) if on_device else int(_lib.resolve_device(device))
    if not on_device:
        _lib.require_device()
    R_w = len(Q)
    var_w = n_eff = xmin = xmax = None
    if bandwidth is None:
        dx = x if on_device else _to_device(x, dev)
        if log_weights is None:
            dq = _q_tensor(q, dev).to(torch.float64)
            lw = torch.log(dq) - torch.log(torch.from_numpy(np.asarray(Q).astype(np.float64)).to(dq.device))[:, None]
        else:
            lw, lw_dev = _rows(log_weights)
            lw = lw if lw_dev else _to_device(np.ascontiguousarray(lw, dtype=np.float64), dev)
        _, var_w = LO.weighted_moments_dev(dev, dx.data_ptr(), 1, S, S, d, lw)
        n_eff = np.exp(-(logmeanexp_dev(lw * 2.0) + math.log(S)))
    if grid is None:
        xmin = x.amin(dim=0).cpu().numpy() if on_device else x.min(axis=0)
        xmax = x.amax(dim=0).cpu().numpy() if on_device else x.max(axis=0)
    h, g = _kde_plan(var_w, n_eff, xmin, xmax, R_w, d, grid, bandwidth, n_grid, cut)
    if on_device:
        dens = weighted_kde_dev(dev, x.data_ptr(), d, S, 1, d, _q_tensor(q, dev), g, h)
    else:
        qh = np.ascontiguousarray(np.atleast_2d(q), dtype=np.uint64)
        if qh.shape != (R_w, S):
            raise ValueError(f"the weights must be (R_w, {S})")
        dens = np.empty(g.shape)
        check(_lib.lib().gpemu_weighted_kde1d(dev, d, S, ptr(np.ascontiguousarray(x.T)), R_w, ptr(qh), int(g.shape[-1]),
                                              ptr(g), ptr(h), ptr(dens)))
    return {"grid": g, "density": dens, "bandwidth": h}


def bands_of_view(models, rows, q, Q, probabilities=(0.05, 0.5, 0.95), workspace_bytes=0):
    """The weighted posterior-predictive bands of the ``DeviceRows`` ``rows`` under the int64 device tensor ``q (R_w,
    S)`` with totals ``Q``: a list over the weight rows of ``{"posterior_predictive": [one dict per model]}``
    (``DeviceModel.posterior_predictive_weighted``'s dicts)."""
    import torch
    from .model import weighted_postpred_result
    p = np.zeros(0) if probabilities is None else np.asarray(probabilities, dtype=np.float64).reshape(-1)
    R_w = int(q.shape[0])
    tgt = targets(p, Q) if p.size else np.zeros((R_w, 0), dtype=np.uint64)
    per_model = []
    for m in models:
        mean, vp, ve = (torch.empty((R_w, m.F), dtype=torch.float64, device=q.device) for _ in range(3))
        qt = torch.empty((R_w, m.F, max(p.size, 1)), dtype=torch.float64, device=q.device)
        m.posterior_predictive_weighted_dev(*rows.layout, q, tgt, mean.data_ptr(), vp.data_ptr(), ve.data_ptr(),
                                            qt.data_ptr() if p.size else 0, workspace_bytes)
        per_model.append(weighted_postpred_result(mean.cpu().numpy(), vp.cpu().numpy(), ve.cpu().numpy(),
                                                  qt.cpu().numpy(), p, Q))
    return [{"posterior_predictive": [pm[w] for pm in per_model]} for w in range(R_w)]


def add_hpd_kde(out, hpd_conf, hpd, kde):
    """``summary``'s optional entries into its list of dicts: ``hpd_confidence``, ``hpd (n_levels, d, 2)`` where ``hpd``
    ``(R_w, n_levels, d, 2)`` is given; ``kde_grid``, ``kde_density`` ``(d, G)``, ``kde_bandwidth (d,)`` where ``kde`` is."""
    for r, res in enumerate(out):
        if hpd is not None:
            res["hpd_confidence"] = np.atleast_1d(np.asarray(hpd_conf, dtype=np.float64)).copy()
            res["hpd"] = hpd[r]
        if kde is not None:
            res["kde_grid"], res["kde_density"], res["kde_bandwidth"] = kde["grid"][r], kde["density"][r], kde["bandwidth"][r]
    return out


def assemble(stats, S, Q, mean, var, mean0, var0, quantiles, hist, probabilities, log_norm=None, log_volume=None):
    """One dict per scenario from the pieces: see ``summary``."""
    from . import loo as LO
    thr = LO.k_threshold(S)
    out = []
    for r in range(len(Q)):
        Qr = int(Q[r])
        k = float(stats["pareto_k"][r])
        res = {"pareto_k": k, "k_threshold": thr, "ess_w": float(stats["ess_w"][r]), "reliable": bool(k <= thr),
               "log_mean_ratio": float(stats["log_mean_ratio"][r]),
               "log_evidence_ratio": (None if log_norm is None or log_norm[r] is None
                                      else float(stats["log_mean_ratio"][r] + log_volume - log_norm[r])),
               "mean": mean[r], "sd": np.sqrt(var[r]), "shift": (mean[r] - mean0) / np.sqrt(var0),
               "probabilities": np.asarray(probabilities, dtype=np.float64), "quantiles": quantiles[r],
               "hist_1d_q": hist["hist_1d_q"][r], "hist_2d_q": hist["hist_2d_q"][r],
               "hist_1d": hist["hist_1d_q"][r].astype(np.float64) / Qr, "hist_2d": hist["hist_2d_q"][r].astype(np.float64) / Qr,
               "Q": Qr, "edges_1d": hist["edges_1d"], "edges_2d": hist["edges_2d"], "pairs": hist["pairs"]}
        out.append(res)
    return out


def summary_view(rows, log_ratio_dev, lower, upper, probabilities=(0.05, 0.5, 0.95), bins_1d=100, bins_2d=50,
                 smooth=True, r_eff=None, log_norm=None, baseline=None, workspace_bytes=0, hpd=None, kde=False, n_grid=200,
                 extra=None):
    """``summary`` of the ``DeviceRows`` ``rows`` under the device tensor ``log_ratio_dev (R, S)``.  The moments and the
    histograms read the rows as they lie; the quantiles, intervals and densities read ``rows.columns()``.  ``baseline()``:
    the unweighted ``(mean, var)`` where the caller has them, else the same reduction under uniform weights.  ``hpd``
    (confidence levels), ``kde``: see ``summary``; ``extra(q, Q)``: further entries per scenario, a list of dicts to merge in."""
    from . import loo as LO
    from . import marginals as M
    device, d, S = rows.device, rows.d, rows.rows
    lo, hi = _box(lower, upper, d)
    if not (1 <= int(bins_1d) <= MAX_BINS_1D and 1 <= int(bins_2d) <= MAX_BINS_2D):
        raise ValueError(f"bins_1d must be in [1, {MAX_BINS_1D}] and bins_2d in [1, {MAX_BINS_2D}]")
    e1, e2 = M.bin_edges(lo, hi, bins_1d), M.bin_edges(lo, hi, bins_2d)
    st = weights(log_ratio_dev, smooth=smooth, r_eff=r_eff, workspace_bytes=workspace_bytes)
    lw = st["log_weights"]
    q, Q = fixed_weights_dev(lw)
    if np.any(Q == 0):
        raise ValueError("a scenario's weights are all zero or not finite: its log-ratio holds a NaN or an infinity")
    mean, var = LO.weighted_moments_dev(device, *rows.layout, d, lw)
    mean0, var0 = LO.plain_moments_dev(rows, baseline)
    tgt = targets(probabilities, Q)
    cols = rows.columns()
    quant = weighted_quantile_dev(device, cols.address, d, S, 1, d, q, tgt, workspace_bytes).transpose(0, 2, 1)
    h1, h2, wi = weighted_hist_dev(device, *rows.layout, d, q, e1, e2)
    hist = {"edges_1d": e1, "edges_2d": e2, "pairs": M.pair_indices(d), "hist_1d_q": h1, "hist_2d_q": h2, "w_inside": wi}
    out = assemble(st, S, Q, mean, var, np.asarray(mean0), np.asarray(var0), np.ascontiguousarray(quant), hist,
                   probabilities, log_norm, float(np.sum(np.log(hi - lo))))
    iv = dens = None
    if hpd is not None:
        iv = weighted_hpd_dev(device, cols.address, d, S, 1, d, q, targets(hpd, Q), workspace_bytes).transpose(0, 2, 1, 3)
        iv = np.ascontiguousarray(iv)
    if kde:
        ends = M._hpd_dev(device, cols.address, S, d, [1])[0]         # n_out = 1, window 0: (smallest, largest)
        h, g = _kde_plan(var, st["ess_w"], ends[:, 0], ends[:, 1], len(Q), d, None, None, n_grid, 3.0)
        dens = {"grid": g, "density": weighted_kde_dev(device, cols.address, d, S, 1, d, q, g, h), "bandwidth": h}
    add_hpd_kde(out, hpd, iv, dens)
    if extra is not None:
        for res, more in zip(out, extra(q, Q)):
            res.update(more)
    return out


def summary(samples, log_ratio, lower, upper, probabilities=(0.05, 0.5, 0.95), bins_1d=100, bins_2d=50, smooth=True,
            r_eff=None, log_norm=None, device=None, hpd=None, kde=False, n_grid=200, extra=None):
    """The reweighted posterior of ``samples (S, d)`` under every row of ``log_ratio (R, S)``: a list with one dict per
    scenario -- ``pareto_k``, ``k_threshold`` (``gpemu.loo.k_threshold``), ``ess_w``, ``reliable = pareto_k <=
    k_threshold``, ``log_mean_ratio``, ``log_evidence_ratio`` (with ``log_norm`` from ``log_prior_norm``: the log Bayes
    factor between the normalised priors; else ``None``), ``mean``, ``sd`` ``(d,)`` under the weights, ``shift = (mean -
    mean_old) / sd_old``, ``quantiles (nq, d)``, the histograms of ``gpemu.marginals.histograms``' edges as exact integers
    ``hist_1d_q``, ``hist_2d_q`` and as densities ``hist_1d``, ``hist_2d`` ``= hist_q / Q``, ``Q``, ``edges_1d``,
    ``edges_2d``, ``pairs``.  ``hpd``: confidence levels, adds ``hpd_confidence`` and ``hpd (n_levels, d, 2)``
    (``weighted_hpd``); ``kde=True`` adds ``kde_grid``, ``kde_density`` ``(d, n_grid)`` and ``kde_bandwidth (d,)``
    (``weighted_kde_1d`` with its defaults, the weighted variance and ``ess_w`` of this summary); ``extra(q, Q)``:
    further entries per scenario, a list of dicts to merge in (``q`` as the samples are: numpy or device).  numpy samples go
    through the host entries, a float64 device tensor is read in place; the results are the same bits."""
    import torch
    from . import loo as LO
    x, on_device = _samples(samples)
    S, d = int(x.shape[0]), int(x.shape[1])
    L, l_dev = _rows(log_ratio)
    if int(L.shape[1]) != S:
        raise ValueError(f"log_ratio has {int(L.shape[1])} columns, the samples are {S}")
    if on_device:
        dL = L if l_dev else _to_device(np.ascontiguousarray(L, dtype=np.float64), x.device.index or 0)
        return summary_view(DeviceRows.of_tensor(x), dL, lower, upper, probabilities, bins_1d, bins_2d, smooth, r_eff,
                            log_norm, hpd=hpd, kde=kde, n_grid=n_grid, extra=extra)
    _lib.require_device()
    dev = int(_lib.resolve_device(device))
    lo, hi = _box(lower, upper, d)
    L = L.cpu().numpy() if l_dev else np.ascontiguousarray(L, dtype=np.float64)
    st = weights(L, smooth=smooth, r_eff=r_eff, device=dev)
    q, Q = fixed_weights(st["log_weights"], device=dev)
    if np.any(Q == 0):
        raise ValueError("a scenario's weights are all zero or not finite: its log-ratio holds a NaN or an infinity")
    dx, dlw = _to_device(x, dev), _to_device(st["log_weights"], dev)
    mean, var = LO.weighted_moments_dev(dev, dx.data_ptr(), 1, S, S, d, dlw)
    m0, v0 = LO.weighted_moments_dev(dev, dx.data_ptr(), 1, S, S, d,
                                     torch.zeros((1, S), dtype=torch.float64, device=dx.device))
    quant = weighted_quantile(x, probabilities, q, Q, device=dev)
    hist = weighted_histograms(x, lo, hi, q, bins_1d, bins_2d, device=dev)
    out = assemble(st, S, Q, mean, var, m0[0], v0[0], quant, hist, probabilities, log_norm,
                   float(np.sum(np.log(hi - lo))))
    iv = dens = None
    if hpd is not None:
        iv = weighted_hpd(x, hpd, q, Q, device=dev)
    if kde:
        h, g = _kde_plan(var, st["ess_w"], x.min(axis=0), x.max(axis=0), len(Q), d, None, None, n_grid, 3.0)
        dens = weighted_kde_1d(x, q, grid=g, bandwidth=h, Q=Q, device=dev)
    add_hpd_kde(out, hpd, iv, dens)
    if extra is not None:
        for res, more in zip(out, extra(q, Q)):
            res.update(more)
    return out


def chain_reweight(models, X, priors=None, models_new=None, lower=None, upper=None, chain=0, posterior_predictive=False,
                   **summary_kw):
    """``DeviceSampler.reweight`` for a chain on the host: ``X (S, d)``, the flattened rows, of a sampler over ``models``
    (whose bands ``posterior_predictive`` adds)."""
    from .sampler import DeviceSampler
    models = list(models) if isinstance(models, (list, tuple)) else [models]
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] != models[0].d:
        raise ValueError(f"X must be (S, {models[0].d})")
    lower, upper = DeviceSampler._box_or_prior(models, lower, upper)
    L = log_ratio(X, priors=priors, lower=lower, upper=upper, models_old=models if models_new is not None else None,
                  models_new=models_new, chain=chain, device=models[0].device)
    log_norm = None
    if priors is not None and models_new is None:
        log_norm = log_prior_norm(*check_priors(priors, X.shape[1], lower, upper), lower, upper)
    extra = None
    if posterior_predictive:
        probs = summary_kw.get("probabilities", (0.05, 0.5, 0.95))

        def extra(q, Q):
            per_model = [m.posterior_predictive_weighted(X, q, probs) for m in models]
            return [{"posterior_predictive": [pm[w] for pm in per_model]} for w in range(len(Q))]
    return summary(X, L, lower, upper, log_norm=log_norm, device=models[0].device, extra=extra, **summary_kw)
