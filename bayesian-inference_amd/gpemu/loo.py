"""Per-observable log-likelihoods, PSIS-LOO and WAIC on the device.

Which observable does what to the posterior, and how well is each observable predicted by all the others -- what the
reference answers only by a second analysis on a subset of the observables (ref: plot_analyses.py) and leaves open as
"some type of information gain metric" (ref: plot_qhat.py:116, plot_analyses.py:144):

* ``pointwise``: ``T (n_obs, S)``, the log-likelihood term of every observable block for every row of a chain;
* ``psis``: the Pareto-smoothed importance-sampling leave-one-out expected log predictive density of every row of ``T``
  (Vehtari, Gelman, Gabry 2017; Vehtari, Simpson, Gelman, Yao, Gabry 2024), the Pareto k-hat diagnostic and WAIC;
* ``weighted_moments``: the leave-one-observable-out posterior mean and variance of the parameters;
* ``summary`` / ``compare``: the tables ArviZ prints (``loo``, ``compare``) from those.

``p_waic`` is the sample variance of the pointwise log-likelihood with divisor ``S - 1``, as Vehtari, Gelman and Gabry
(2017) define it; ArviZ divides by ``S``.

Matrices are ``(R, S)``: numpy arrays go through the host entries, contiguous float64 device tensors are read in place.
There is no CPU implementation."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check, ptr
from .rows import DeviceRows

PATHS = ("SORT_PASS", "ROW_SMOOTHED", "ROW_RAW", "CHUNK", "ROW_BATCH")
FIELDS = ("elpd_loo", "lppd", "p_loo", "pareto_k", "n_tail", "ess_w", "p_waic", "elpd_waic", "cutoff")
SUMMARY_KEYS = ("elpd_loo", "p_loo", "pareto_k", "k_threshold", "ess_w", "elpd_waic", "p_waic", "lppd")
LOG_2PI = math.log(2.0 * math.pi)


def path_counts():
    """The library's counters of these launches since the process started, by name."""
    out = (C.c_int64 * len(PATHS))()
    n = _lib.lib().gpemu_loo_path_counts(out, len(PATHS))
    if n < 0:
        check(n)
    return {k: int(out[i]) for i, k in enumerate(PATHS)}


# -- host-side rules --------------------------------------------------------------------------------------------------
def tail_size(S, r_eff=1.0):
    """``ceil(min(S / 5, 3 sqrt(S / r_eff)))``: the tail the smoothing asks for."""
    return int(math.ceil(min(S / 5.0, 3.0 * math.sqrt(S / float(r_eff)))))


def k_threshold(S):
    """``min(1 - 1 / log10(S), 0.7)``: the sample-size dependent limit of a reliable k-hat (Vehtari et al. 2024)."""
    return min(1.0 - 1.0 / math.log10(S), 0.7) if S > 1 else -math.inf


def check_leave_out(leave_out, n_obs):
    """``leave_out`` as ``(group_start (G + 1,), rows (n,))`` int64: a list of non-empty lists of rows of ``T``."""
    if isinstance(leave_out, (str, bytes)) or not hasattr(leave_out, "__len__") or len(leave_out) == 0:
        raise ValueError("leave_out must be a non-empty list of lists of observable indices")
    start, rows = [0], []
    for g in leave_out:
        g = [g] if np.ndim(g) == 0 else list(g)
        if len(g) == 0:
            raise ValueError("every leave_out group must name an observable")
        for o in g:
            if int(o) != o or not 0 <= int(o) < n_obs:
                raise IndexError(f"leave_out names observable {o}, outside [0, {n_obs})")
            rows.append(int(o))
        start.append(len(rows))
    return np.array(start, dtype=np.int64), np.array(rows, dtype=np.int64)


def _r_eff(r_eff, R):
    if r_eff is None:
        return None
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(r_eff, dtype=np.float64), (R,)))
    if not np.all(np.isfinite(r) & (r > 0.0)):
        raise ValueError("every r_eff must be finite and > 0")
    return r


def _rows(T):
    """``(matrix (R, S), on_device)``; a vector is one row."""
    if _lib.is_device_tensor(T):
        import torch
        if T.dtype != torch.float64 or T.dim() not in (1, 2):
            raise TypeError("a device matrix must be a float64 tensor (R, S)")
        return T.reshape(-1, T.shape[-1]).contiguous(), True
    t = np.asarray(T, dtype=np.float64)
    if t.ndim == 1:
        t = t[None, :]
    if t.ndim != 2 or t.shape[1] < 1:
        raise ValueError("T must be (R, S) with S >= 1")
    return np.ascontiguousarray(t), False


def _unpack(out):
    res = {k: np.ascontiguousarray(out[:, i]) for i, k in enumerate(FIELDS)}
    res["n_tail"] = np.where(np.isnan(res["n_tail"]), -1, res["n_tail"]).astype(np.int64)
    return res


# -- device calls -----------------------------------------------------------------------------------------------------
def psis_dev(device, base, R, S, row_stride, elem_stride=1, r_eff=None, return_weights=False, workspace_bytes=0):
    """``psis`` of ``R`` device rows (element j of row r at ``base + 8 (r row_stride + j elem_stride)``): the dict of
    numpy arrays and, with ``return_weights``, ``log_weights`` as a device tensor ``(R, S)``."""
    import torch
    dev = torch.device("cuda", int(device))
    r = _r_eff(r_eff, R)
    out = torch.empty((R, len(FIELDS)), dtype=torch.float64, device=dev)
    lw = torch.empty((R, S), dtype=torch.float64, device=dev) if return_weights else None
    check(_lib.lib().gpemu_psis_dev(int(device), int(R), int(S), C.c_void_p(base), int(row_stride), int(elem_stride), ptr(r),
                                    C.c_void_p(out.data_ptr()), C.c_void_p(lw.data_ptr()) if return_weights else None,
                                    int(workspace_bytes), _lib.current_stream(device)))
    res = _unpack(out.cpu().numpy())
    if return_weights:
        res["log_weights"] = lw
    return res


def group_rows_dev(device, base, R, S, ldt, leave_out):
    """The rows of a device matrix ``[R][ldt]`` summed per ``leave_out`` group, in the given order: a device tensor
    ``(G, S)``."""
    import torch
    start, rows = check_leave_out(leave_out, R)
    out = torch.empty((start.size - 1, S), dtype=torch.float64, device=torch.device("cuda", int(device)))
    check(_lib.lib().gpemu_loo_group_rows_dev(int(device), int(R), int(S), C.c_void_p(base), int(ldt), int(start.size - 1),
                                              ptr(start), ptr(rows), C.c_void_p(out.data_ptr()), int(S),
                                              _lib.current_stream(device)))
    return out


def _left_out(device, T, labels, leave_out):
    """``(the rows of the device tensor T summed per leave_out group, the groups' labels "a+b")``"""
    groups = [[g] if np.ndim(g) == 0 else list(g) for g in leave_out]
    names = [str(v) for v in labels]
    out = group_rows_dev(device, T.data_ptr(), int(T.shape[0]), int(T.shape[1]), int(T.shape[1]), groups)
    return out, ["+".join(names[int(o)] for o in g) for g in groups]


def weighted_moments_dev(device, base, n_blocks, block_rows, block_stride_rows, d, log_weights):
    """``(mean, var)``, each ``(R, d)``, of the device rows in the block layout of ``posterior_predictive_dev`` under the
    ``R`` rows of log-weights of the device tensor ``log_weights (R, S)``."""
    import torch
    lw = log_weights.contiguous()
    R, S = int(lw.shape[0]), int(lw.shape[1])
    if S != int(n_blocks) * int(block_rows):
        raise ValueError(f"log_weights has {S} columns, the rows are {int(n_blocks) * int(block_rows)}")
    out = torch.empty((2, R, int(d)), dtype=torch.float64, device=lw.device)
    check(_lib.lib().gpemu_weighted_moments_dev(int(device), C.c_void_p(base), int(n_blocks), int(block_rows),
                                                int(block_stride_rows), int(d), R, C.c_void_p(lw.data_ptr()), S,
                                                C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()),
                                                _lib.current_stream(device)))
    h = out.cpu().numpy()
    return h[0].copy(), h[1].copy()


def pointwise_dev(model_or_models, rows, chain=0):
    """``pointwise`` of the ``DeviceRows`` ``rows``, read in place: a device tensor ``(n_obs, S)``."""
    import torch
    models = list(model_or_models) if isinstance(model_or_models, (list, tuple)) else [model_or_models]
    nobs = [m.n_observable_blocks for m in models]
    T = torch.empty((sum(nobs), rows.rows), dtype=torch.float64, device=torch.device("cuda", rows.device))
    o0 = 0
    for m, nb in zip(models, nobs):
        m.loglik_pointwise_dev(*rows.layout, T[o0].data_ptr(), rows.rows, chain=chain)
        o0 += nb
    return T


def plain_moments_dev(rows, baseline=None):
    """The unweighted ``(mean, var)`` ``(d,)`` of ``DeviceRows``: ``baseline()``, else ``weighted_moments_dev``, uniform."""
    if baseline is not None:
        return baseline()
    import torch
    uniform = torch.zeros((1, rows.rows), dtype=torch.float64, device=torch.device("cuda", rows.device))
    mean, var = weighted_moments_dev(rows.device, *rows.layout, rows.d, uniform)
    return mean[0], var[0]


# -- public functions -------------------------------------------------------------------------------------------------
def pointwise(model_or_models, X, normalised=False, chain=0):
    """``T (n_obs, S)``: the log-likelihood term of every observable block of the model -- or of every model of a list,
    concatenated in the list's order, the order of ``predict``'s observables -- for the rows of ``X (S, d)``, in the
    log-posterior's normalisation (the reference's form carries no 2 pi constant); ``normalised`` adds ``-(F_o / 2) log
    2 pi`` per block.  A likelihood: no prior box.  ``chain`` selects the data vector of a setup with several."""
    models = list(model_or_models) if isinstance(model_or_models, (list, tuple)) else [model_or_models]
    return np.concatenate([m.loglik_pointwise(X, normalised=normalised, chain=chain) for m in models], axis=0)


def psis(T, r_eff=None, return_weights=False, device=None, workspace_bytes=0):
    """PSIS-LOO and WAIC of every row of ``T (R, S)`` (one observable each, or a sum of several): a dict of ``(R,)``
    arrays ``elpd_loo``, ``lppd``, ``p_loo = lppd - elpd_loo``, ``pareto_k`` (``inf``: the tail had at most 4 elements and
    the weights stayed raw), ``n_tail``, ``ess_w = 1 / sum w^2``, ``p_waic`` (divisor ``S - 1``; ArviZ: ``S``),
    ``elpd_waic = lppd - p_waic`` and ``cutoff``; with ``return_weights``, ``log_weights (R, S)``, normalised, in the
    input's order (a device tensor for a device ``T``).  ``r_eff``: a number or ``(R,)``, the relative efficiency of the
    chain for ``exp(T)`` (default 1).  A row with a NaN or an infinity gives NaN.  The result, bit for bit, does not depend on
    ``workspace_bytes``."""
    t, on_device = _rows(T)
    R, S = int(t.shape[0]), int(t.shape[1])
    if on_device:
        return psis_dev(t.device.index or 0, t.data_ptr(), R, S, S, 1, r_eff, return_weights, workspace_bytes)
    _lib.require_device()
    r = _r_eff(r_eff, R)
    out = np.empty((R, len(FIELDS)))
    lw = np.empty((R, S)) if return_weights else None
    check(_lib.lib().gpemu_psis(int(_lib.resolve_device(device)), R, S, ptr(t), ptr(r), int(workspace_bytes), ptr(out),
                                ptr(lw)))
    res = _unpack(out)
    if return_weights:
        res["log_weights"] = lw
    return res


def waic(T, device=None):
    """``lppd``, ``p_waic`` and ``elpd_waic`` of every row of ``T (R, S)`` (``psis`` computes them beside the rest)."""
    res = psis(T, device=device)
    return {k: res[k] for k in ("lppd", "p_waic", "elpd_waic")}


def assemble(stats, S, labels=None):
    """The summary dict from ``psis``'s per-row arrays: the ``SUMMARY_KEYS`` per observable, ``n_obs``, ``n_samples``,
    ``labels``, the totals ``elpd_loo_total`` ... ``lppd_total``, ``se = sqrt(n_obs var_ddof0(elpd_loo_i))`` (``se_waic``
    likewise) and ``warning``, true where ``pareto_k > k_threshold``."""
    n_obs = int(np.asarray(stats["elpd_loo"]).size)
    out = {k: np.asarray(stats[k]) for k in SUMMARY_KEYS if k != "k_threshold"}
    out["k_threshold"] = np.full(n_obs, k_threshold(S))
    out["n_tail"] = np.asarray(stats["n_tail"])
    out["n_obs"], out["n_samples"] = n_obs, int(S)
    out["labels"] = [str(i) for i in range(n_obs)] if labels is None else [str(v) for v in labels]
    if len(out["labels"]) != n_obs:
        raise ValueError(f"{len(out['labels'])} labels for {n_obs} rows")
    for k in ("elpd_loo", "p_loo", "elpd_waic", "p_waic", "lppd"):
        out[k + "_total"] = float(np.sum(out[k]))
    out["se"] = float(np.sqrt(n_obs * np.var(out["elpd_loo"])))
    out["se_waic"] = float(np.sqrt(n_obs * np.var(out["elpd_waic"])))
    out["warning"] = out["pareto_k"] > out["k_threshold"]
    return out


def summary(T, labels=None, leave_out=None, r_eff=None, device=None):
    """The LOO / WAIC table of ``T (n_obs, S)``: see ``assemble``.  ``leave_out=[[0, 1], [2]]`` first sums the named rows
    of ``T`` on the device, in the given order: a class of observables left out together (the reference's two-analysis
    comparison without a second MCMC); the table then has one row per group, labelled by its members."""
    t, on_device = _rows(T)
    R, S = int(t.shape[0]), int(t.shape[1])
    if leave_out is not None:
        import torch
        if not on_device:
            _lib.require_device()
            t = torch.from_numpy(t).to(torch.device("cuda", int(_lib.resolve_device(device))))
        t, labels = _left_out(t.device.index or 0, t, [str(i) for i in range(R)] if labels is None else labels, leave_out)
    return assemble(psis(t, r_eff=r_eff, device=device), S, labels)


def compare(summary_a, summary_b):
    """Two parameterisations on the same data: ``elpd_diff = elpd_loo_total(a) - elpd_loo_total(b)``, ``se_diff = sqrt(n_obs
    var_ddof0(elpd_loo_i(a) - elpd_loo_i(b)))``, the pointwise differences and the same for WAIC."""
    a, b = summary_a, summary_b
    if a["n_obs"] != b["n_obs"] or list(a["labels"]) != list(b["labels"]):
        raise ValueError("the two summaries must be over the same observables")
    diff = np.asarray(a["elpd_loo"]) - np.asarray(b["elpd_loo"])
    dw = np.asarray(a["elpd_waic"]) - np.asarray(b["elpd_waic"])
    n = a["n_obs"]
    return {"elpd_diff": float(np.sum(diff)), "se_diff": float(np.sqrt(n * np.var(diff))), "pointwise_diff": diff,
            "elpd_waic_diff": float(np.sum(dw)), "se_waic_diff": float(np.sqrt(n * np.var(dw))),
            "warning": bool(np.any(a["warning"]) or np.any(b["warning"]))}


def from_terms(T, labels, rows, leave_out=None, shifts=True, r_eff=None, workspace_bytes=0, baseline=None):
    """The table of ``DeviceSampler.loo`` from the device tensor ``T (n_obs, S)`` of the terms of the ``DeviceRows``
    ``rows``: ``assemble`` of ``psis`` and, with ``shifts``, ``mean``, ``sd`` ``(d,)`` (``baseline()``, or the same
    reduction under uniform weights), ``loo_mean``, ``loo_sd`` ``(n_obs, d)`` and ``shift = (loo_mean - mean) / sd``."""
    labels = [str(v) for v in labels]
    if leave_out is not None:
        T, labels = _left_out(rows.device, T, labels, leave_out)
    R, S = int(T.shape[0]), int(T.shape[1])
    stats = psis_dev(rows.device, T.data_ptr(), R, S, S, 1, r_eff, bool(shifts), workspace_bytes)
    out = assemble(stats, S, labels)
    if shifts:
        out["loo_mean"], var = weighted_moments_dev(rows.device, *rows.layout, rows.d, stats["log_weights"])
        out["loo_sd"] = np.sqrt(var)
        mean, v0 = plain_moments_dev(rows, baseline)
        out["mean"], out["sd"] = np.asarray(mean), np.sqrt(v0)
        out["shift"] = (out["loo_mean"] - out["mean"][None, :]) / out["sd"][None, :]
    return out


def default_labels(models):
    """``g<group>o<block>`` for every observable block of every model, in ``pointwise``'s order."""
    return [f"g{g}o{o}" for g, m in enumerate(models) for o in range(m.n_observable_blocks)]


def chain_loo(models, X, leave_out=None, shifts=True, r_eff=None, chain=0, labels=None, workspace_bytes=0):
    """``DeviceSampler.loo`` for a chain on the host: ``X (S, d)``, the flattened rows, against data vector ``chain`` of
    the models' likelihood setup."""
    import torch
    models = list(models) if isinstance(models, (list, tuple)) else [models]
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] != models[0].d:
        raise ValueError(f"X must be (S, {models[0].d})")
    dev = torch.device("cuda", int(models[0].device))
    T = torch.from_numpy(pointwise(models, X, chain=chain)).to(dev)
    rows = DeviceRows.of_tensor(torch.from_numpy(X).to(dev))
    return from_terms(T, default_labels(models) if labels is None else labels, rows, leave_out, shifts, r_eff,
                      workspace_bytes)
