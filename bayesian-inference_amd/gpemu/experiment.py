"""Expected information gain of candidate measurements on the device.

Which *measurement* would constrain the parameters most -- a repeat of an observable, the same observable with half the
uncertainty, a new bin range?  The expected information gain (EIG) of an experiment is the mutual information between
the parameters and its not-yet-seen outcome, the expectation taken under the current posterior (a follow-up measurement)
or under the prior (a first one).  With a Gaussian likelihood of constant covariance ``Sigma = L L^T`` the nested Monte
Carlo estimator that reuses the inner sample (Ryan 2003; Huan and Marzouk 2013) is

    EIG ~ (1/n) sum_i [ log p(y_i | theta_i) - log (1/S') sum_j p(y_i | theta_j) ],    y_i = m(theta_i) + L eps_i.

Whitened, ``log p(y_i | theta_j) = -|yh_i - z_j|^2 / 2 + const`` with ``z_j = L^-1 m(theta_j)``, the constant cancels,
and the hot path is a row-wise log-sum-exp of pairwise squared distances: ``pair_lse``.

* ``pair_lse``: ``lse_i = log sum_j exp(-|y_i - z_j|^2 / 2)`` and the effective number of columns that carry row i;
* ``expected_information_gain``: the estimator for one candidate, from the model's predictions at the parameter samples;
* ``rank_measurements``: several candidates on common random numbers, sorted.

The estimator is biased: it cannot report more than ``log n_inner`` nats, and with the outer rows among the inner ones
(the default, ``exclude_self=False``) it is biased LOW by the row's own weight (Ryan's reuse; of order 1 / ess), with
``exclude_self=True`` HIGH like the plain nested estimator.  ``saturated`` marks results that are at the cap.  The
likelihood covariance must not depend on theta; noise that is not Gaussian is not covered.

numpy arrays go through the host entry, float64 device tensors are read in place.  There is no CPU implementation."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check, ptr
from .information import selected_rows

PATHS = ("CENTRE", "PARTIAL", "MERGE", "ROW_BATCH")
CHUNK = 2048              # GPEMU_PAIRLSE_CHUNK: columns per partial triple
TILE_ROWS = 64            # GPEMU_PAIRLSE_TILE_ROWS: rows per workgroup
MAX_F = 65536
# conditions of use, not measurements: the estimate is flagged where it comes within 3 nats of its cap log n_inner, or
# where fewer than 16 inner samples carry a typical outer row
SATURATION_MARGIN = 3.0
MIN_ESS = 16.0
LOG2 = math.log(2.0)


def path_counts():
    """The library's counters of these launches since the process started, by name."""
    out = (C.c_int64 * len(PATHS))()
    n = _lib.lib().gpemu_pairlse_path_counts(out, len(PATHS))
    if n < 0:
        check(n)
    return {k: int(out[i]) for i, k in enumerate(PATHS)}


def block_bytes(S, F):
    """GPEMU_PAIRLSE_BLOCK_BYTES: the workspace of one block of ``TILE_ROWS`` rows; ``workspace_bytes`` holds whole blocks."""
    return 8 * TILE_ROWS * (((int(F) + 15) // 16 * 16 + 1) + 3 * ((int(S) + CHUNK - 1) // CHUNK))


# -- host-side rules --------------------------------------------------------------------------------------------------
def check_shapes(n, S, F):
    if n < 1 or S < 1 or F < 1:
        raise ValueError(f"Y (n, F) and Z (S, F) need n, S, F >= 1, got n = {n}, S = {S}, F = {F}")
    if n >= 2 ** 31 or S >= 2 ** 31 or F > MAX_F:
        raise ValueError(f"n and S must be below 2^31 and F at most {MAX_F}, got n = {n}, S = {S}, F = {F}")


def check_self_index(self_index, n, S):
    """``self_index`` as a contiguous int64 array ``(n,)`` with every entry in ``[-1, S)``, or ``None``."""
    if self_index is None:
        return None
    s = np.asarray(self_index)
    if s.shape != (n,) or not np.issubdtype(s.dtype, np.integer):
        raise ValueError(f"self_index must be {n} integers")
    s = np.ascontiguousarray(s, dtype=np.int64)
    if np.any(s < -1) or np.any(s >= S):
        raise IndexError(f"every self index must be in [-1, {S})")
    return s


def whitening_factor(F, cov=None, y_err=None):
    """``L = chol(Sigma)`` (lower) of the candidate's covariance: ``cov (F, F)`` or ``diag(y_err^2)``, exactly one."""
    if (cov is None) == (y_err is None):
        raise ValueError("give exactly one of cov and y_err")
    if cov is None:
        e = np.ascontiguousarray(np.broadcast_to(np.asarray(y_err, dtype=np.float64), (F,)))
        if not np.all(np.isfinite(e) & (e > 0.0)):
            raise ValueError("every y_err must be finite and > 0")
        return np.diag(e)
    c = np.asarray(cov, dtype=np.float64)
    if c.shape != (F, F) or not np.all(np.isfinite(c)) or not np.allclose(c, c.T, rtol=1e-12, atol=0.0):
        raise ValueError(f"cov must be a finite symmetric ({F}, {F}) matrix")
    try:
        return np.linalg.cholesky(0.5 * (c + c.T))
    except np.linalg.LinAlgError:
        raise ValueError("cov must be positive definite") from None


def whiten(means, L):
    """``z_j = L^-1 m_j`` for the rows of ``means (S, F)``, on the host (F is small)."""
    if np.count_nonzero(L - np.diag(np.diagonal(L))) == 0:
        return np.ascontiguousarray(means / np.diagonal(L)[None, :])
    from scipy.linalg import solve_triangular
    return np.ascontiguousarray(solve_triangular(L, means.T, lower=True).T)


def check_n_outer(n_outer):
    if int(n_outer) != n_outer or not 1 <= int(n_outer) < 2 ** 31:
        raise ValueError(f"n_outer must be an integer in [1, 2^31), got {n_outer!r}")
    return int(n_outer)


def outer_noise(n, F, seed=0, noise=None):
    """``eps (n, F)``: ``np.random.default_rng(seed).standard_normal((n, F))``, or the first F columns of ``noise``."""
    if noise is None:
        return np.random.default_rng(seed).standard_normal((n, F))
    e = np.asarray(noise, dtype=np.float64)
    if e.ndim != 2 or e.shape[0] != n or e.shape[1] < F or not np.all(np.isfinite(e)):
        raise ValueError(f"noise must be a finite array ({n}, >= {F}), got {e.shape}")
    return np.ascontiguousarray(e[:, :F])


def estimate(lse, ess, eps, n_inner):
    """The estimator's result from the inner sums: term i is ``-|eps_i|^2 / 2 - lse_i + log n_inner`` (the whitened
    outcome is ``z_i + eps_i``, so the first term of the estimator needs no distance)."""
    n = lse.shape[0]
    log_inner = math.log(n_inner)
    terms = -0.5 * np.einsum("ij,ij->i", eps, eps) - lse + log_inner
    eig = float(np.mean(terms))
    se = float(np.std(terms, ddof=1) / math.sqrt(n)) if n > 1 else math.nan
    ess_mean, ess_min = float(np.mean(ess)), float(np.min(ess))
    return {"eig_nats": eig, "eig_bits": eig / LOG2, "se": se, "terms": terms, "ess_mean": ess_mean, "ess_min": ess_min,
            "n_outer": int(n), "n_inner": int(n_inner), "log_n_inner": log_inner,
            "saturated": bool(eig > log_inner - SATURATION_MARGIN or ess_mean < MIN_ESS)}


# -- device calls -----------------------------------------------------------------------------------------------------
def centre_dev(Z):
    """The column means of the device tensor ``Z (S, F)`` (any row stride) as ``pair_lse`` computes them: a device
    tensor ``(F,)``."""
    import torch
    dev = Z.device.index or 0
    S, F = int(Z.shape[0]), int(Z.shape[1])
    out = torch.empty((F,), dtype=torch.float64, device=Z.device)
    check(_lib.lib().gpemu_pairlse_centre_dev(dev, S, F, C.c_void_p(Z.data_ptr()), int(Z.stride(0)),
                                              C.c_void_p(out.data_ptr()), _lib.current_stream(Z.device)))
    return out


def _device_rows(x, what):
    import torch
    if x.dtype != torch.float64 or x.dim() != 2:
        raise TypeError(f"a device {what} must be a float64 tensor (rows, F)")
    if x.shape[1] > 1 and x.stride(1) != 1 or x.shape[0] > 1 and x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x


def pair_lse(Y, Z, self_index=None, centre=None, device=None, workspace_bytes=0):
    """``(lse, ess)``, each ``(n,)``, of the rows ``Y (n, F)`` against ``Z (S, F)``:

        a_ij = -|y_i - z_j|^2 / 2,   lse_i = log sum_j exp(a_ij),   ess_i = (sum_j w_ij)^2 / sum_j w_ij^2,  w = exp(a)

    ``self_index (n,)`` leaves pair ``(i, self_index[i])`` out of row i (-1: nothing); a row with every pair left out gives
    ``-inf`` and 0.  ``centre (F,)`` is subtracted from both sets of rows before the distances are formed (default: the
    column means of Z, computed on the device).  numpy arrays go through the host entry; float64 device tensors are read
    in place, with their row strides, and device tensors are returned.  The bits depend neither on ``workspace_bytes``
    (0: half of the free device memory; else at least ``block_bytes(S, F)``) nor on the run."""
    lib = _lib.lib()
    if _lib.is_device_tensor(Y) != _lib.is_device_tensor(Z):
        raise ValueError("Y and Z must both be host arrays or both device tensors")
    if _lib.is_device_tensor(Y):
        import torch
        Y, Z = _device_rows(Y, "Y"), _device_rows(Z, "Z")
        if Y.device != Z.device or Y.shape[1] != Z.shape[1]:
            raise ValueError("Y and Z must lie on one device and have the same columns")
        n, S, F = int(Y.shape[0]), int(Z.shape[0]), int(Y.shape[1])
        check_shapes(n, S, F)
        dev = Y.device.index or 0
        ds = None
        if self_index is not None:
            if _lib.is_device_tensor(self_index):
                if self_index.dtype != torch.int64 or tuple(self_index.shape) != (n,):
                    raise ValueError(f"a device self_index must be {n} int64")
                ds = self_index.contiguous()
            else:
                ds = torch.from_numpy(check_self_index(self_index, n, S)).to(Y.device)
        dc = None
        if centre is not None:
            dc = centre if _lib.is_device_tensor(centre) else torch.from_numpy(_lib.as_f64(centre, (F,))).to(Y.device)
            if dc.dtype != torch.float64 or tuple(dc.shape) != (F,):
                raise ValueError(f"centre must be {F} float64")
            dc = dc.contiguous()
        lse = torch.empty((n,), dtype=torch.float64, device=Y.device)
        ess = torch.empty((n,), dtype=torch.float64, device=Y.device)
        check(lib.gpemu_pair_lse_dev(dev, n, S, F, C.c_void_p(Y.data_ptr()), int(Y.stride(0)) if n > 1 else F,
                                     C.c_void_p(Z.data_ptr()), int(Z.stride(0)) if S > 1 else F,
                                     None if ds is None else C.c_void_p(ds.data_ptr()),
                                     None if dc is None else C.c_void_p(dc.data_ptr()), int(workspace_bytes),
                                     C.c_void_p(lse.data_ptr()), C.c_void_p(ess.data_ptr()), _lib.current_stream(Y.device)))
        return lse, ess
    Y, Z = np.asarray(Y, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    if Y.ndim != 2 or Z.ndim != 2 or Y.shape[1] != Z.shape[1]:
        raise ValueError(f"Y (n, F) and Z (S, F) must have the same columns, got {Y.shape} and {Z.shape}")
    n, S, F = Y.shape[0], Z.shape[0], Y.shape[1]
    check_shapes(n, S, F)
    s = check_self_index(self_index, n, S)
    c = None if centre is None else _lib.as_f64(centre, (F,))
    _lib.require_device()
    Y, Z = np.ascontiguousarray(Y), np.ascontiguousarray(Z)
    lse, ess = np.empty(n), np.empty(n)
    check(lib.gpemu_pair_lse(int(_lib.resolve_device(device)), n, S, F, ptr(Y), ptr(Z), ptr(s), ptr(c), int(workspace_bytes),
                             ptr(lse), ptr(ess)))
    return lse, ess


# -- public functions -------------------------------------------------------------------------------------------------
def _prepare(means, cov, y_err, n_outer, seed, noise, exclude_self):
    """the whitened predictions, the outer rows' indices, their noise and the self indices of one candidate"""
    m = np.asarray(means, dtype=np.float64)
    if m.ndim == 1:
        m = m[:, None]
    if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1 or not np.all(np.isfinite(m)):
        raise ValueError("means must be a finite array (S, F) with S, F >= 1")
    S, F = m.shape
    if exclude_self and S < 2:
        raise ValueError("exclude_self needs at least two parameter samples")
    Z = whiten(m, whitening_factor(F, cov, y_err))
    rows = selected_rows(S, check_n_outer(n_outer))
    eps = outer_noise(rows.size, F, seed, noise)
    return Z, rows, eps, (rows if exclude_self else None)


def expected_information_gain(means, cov=None, y_err=None, n_outer=4096, seed=0, noise=None, exclude_self=False,
                              device=None, workspace_bytes=0):
    """The expected information gain of a measurement with Gaussian uncertainty ``cov (F, F)`` or ``diag(y_err^2)``, given
    ``means (S, F)``: the model's predictions of the candidate's F features at S samples of the parameters (of the
    posterior for a follow-up measurement, of the prior for a first one).  The covariance must not depend on theta.

    The predictions are whitened with ``L = chol(Sigma)`` on the host; the outer rows are the ``n = min(S, n_outer)``
    evenly spaced rows ``information.selected_rows(S, n_outer)``; their outcomes are ``z_i + eps_i`` with ``eps`` drawn from
    ``np.random.default_rng(seed)`` or taken from ``noise (n, >= F)``; the inner sums are one ``pair_lse`` call.  A dict with

    * ``eig_nats``, ``eig_bits``;
    * ``se``: the standard deviation of the n terms over sqrt(n) -- a LOWER bound of the standard error: it ignores the
      autocorrelation of a chain's rows and the error of the inner sums, which the outer rows share;
    * ``terms (n,)``, ``ess_mean``, ``ess_min`` (the effective number of inner samples that carry an outer row);
    * ``n_outer``, ``n_inner`` and ``log_n_inner``: the estimator cannot report more than ``log n_inner`` nats;
    * ``saturated``: ``eig_nats > log_n_inner - 3`` or ``ess_mean < 16`` -- conditions of use, not measurements: such a
      result is a lower bound at best, and more inner samples are needed.

    ``exclude_self=True`` leaves pair (i, i) out of the inner sum and uses ``S' = S - 1``."""
    Z, rows, eps, self_index = _prepare(means, cov, y_err, n_outer, seed, noise, exclude_self)
    lse, ess = pair_lse(np.ascontiguousarray(Z[rows] + eps), Z, self_index=self_index, device=device,
                        workspace_bytes=workspace_bytes)
    return estimate(lse, ess, eps, Z.shape[0] - (1 if exclude_self else 0))


def check_candidates(candidates, F_all):
    """``[(features int64, y_err or None, cov or None, label)]``; every candidate names features in ``[0, F_all)``, each
    once, and exactly one of ``y_err`` and ``cov``."""
    cands = list(candidates)
    if len(cands) == 0:
        raise ValueError("candidates must name at least one measurement")
    out = []
    for c, cand in enumerate(cands):
        if not isinstance(cand, dict) or "features" not in cand:
            raise ValueError(f"candidate {c} must be a dict with 'features'")
        unknown = set(cand) - {"features", "y_err", "cov", "label"}
        if unknown:
            raise ValueError(f"candidate {c} has unknown keys {sorted(unknown)}")
        f = np.atleast_1d(np.asarray(cand["features"]))
        if f.ndim != 1 or f.size == 0 or not np.issubdtype(f.dtype, np.integer):
            raise ValueError(f"candidate {c}: features must be a non-empty list of integers")
        if np.any(f < 0) or np.any(f >= F_all):
            raise IndexError(f"candidate {c} names a feature outside [0, {F_all})")
        if np.unique(f).size != f.size:
            raise ValueError(f"candidate {c} names a feature twice")
        if (cand.get("y_err") is None) == (cand.get("cov") is None):
            raise ValueError(f"candidate {c}: give exactly one of y_err and cov")
        out.append((f.astype(np.int64), cand.get("y_err"), cand.get("cov"), str(cand.get("label", f"candidate {c}"))))
    return out


def rank_measurements(means, candidates, n_outer=4096, seed=0, exclude_self=False, device=None, workspace_bytes=0):
    """The expected information gain of every candidate measurement, compared on common random numbers.  ``means (S,
    F_all)``; ``candidates``: dicts with ``features`` (indices into the columns of ``means``), ``y_err`` or ``cov`` and
    an optional ``label``.  One normal array ``(n, F_max)`` is drawn from ``seed``; candidate c uses its first ``F_c``
    columns.  A dict with ``labels``, ``eig_nats``, ``eig_bits``, ``se``, ``ess_mean``, ``saturated`` (arrays in the order
    given), ``order`` (the candidates' indices sorted by ``eig_nats``, largest first), ``table`` (the results in that
    order, each a dict of ``expected_information_gain`` plus ``label`` and ``index``) and ``results`` (in the order given)."""
    m = np.asarray(means, dtype=np.float64)
    if m.ndim != 2:
        raise ValueError("means must be (S, F_all)")
    cands = check_candidates(candidates, m.shape[1])
    n = selected_rows(m.shape[0], check_n_outer(n_outer)).size
    noise = outer_noise(n, max(f.size for f, _, _, _ in cands), seed)
    results = []
    for c, (f, y_err, cov, label) in enumerate(cands):
        r = expected_information_gain(m[:, f], cov=cov, y_err=y_err, n_outer=n_outer, noise=noise,
                                      exclude_self=exclude_self, device=device, workspace_bytes=workspace_bytes)
        r["label"], r["index"] = label, c
        results.append(r)
    eig = np.array([r["eig_nats"] for r in results])
    order = np.argsort(-eig, kind="stable")
    return {"labels": [r["label"] for r in results], "eig_nats": eig, "eig_bits": eig / LOG2,
            "se": np.array([r["se"] for r in results]), "ess_mean": np.array([r["ess_mean"] for r in results]),
            "saturated": np.array([r["saturated"] for r in results], dtype=bool), "order": order,
            "table": [results[i] for i in order], "results": results}


# -- emulators and chains ---------------------------------------------------------------------------------------------
EMULATOR_COV = ("mean", "none")


def model_predictions(models, X, batch=4096):
    """``(means (S, F_total), emulator_cov (F_total, F_total))`` of the emulation groups ``models`` at the rows ``X (S, d)``:
    the central values of ``DeviceModel.predict_full(n_div=1)`` with the groups' features concatenated in the order given
    (the order ``emulation.predict`` returns), and the average over the rows of the emulators' feature-space covariance
    (truncation term included), block diagonal over the groups.  The rows go through the library in batches of at most
    ``batch`` (fewer where a batch's covariances would exceed 128 MiB)."""
    models = list(models)
    if not models:
        raise ValueError("model_predictions needs at least one model")
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1:
        raise ValueError("X must be (S, d) with S >= 1")
    S, Ft = X.shape[0], sum(int(m.F) for m in models)
    means, emu, f0 = np.empty((S, Ft)), np.zeros((Ft, Ft)), 0
    for m in models:
        F = int(m.F)
        step = max(1, min(int(batch), (1 << 24) // (F * F)))
        acc = np.zeros((F, F))
        for b0 in range(0, S, step):
            cv, cov = m.predict_full(X[b0:b0 + step], n_div=1.0)
            means[b0:b0 + step, f0:f0 + F] = cv
            acc += cov.sum(axis=0)
        emu[f0:f0 + F, f0:f0 + F] = acc / S
        f0 += F
    return means, emu


def chain_expected_information_gain(models, X, candidates, n_outer=4096, seed=0, emulator_cov="mean", exclude_self=False,
                                    batch=4096, workspace_bytes=0):
    """``rank_measurements`` of candidate measurements given samples ``X (S, d)`` of the parameters and the emulators
    ``models`` that predict the observables: ``means`` are the emulators' central values at X, the candidates' features
    index the groups' features concatenated in the order of ``models``.  ``emulator_cov='mean'`` adds the average over the
    rows of the emulators' covariance (truncation term included) to every candidate's covariance -- a constant matrix, as
    the estimator requires; ``'none'`` uses the candidates' covariance alone.  A covariance that depends on theta (the
    emulator's own, row by row) is out of scope."""
    if emulator_cov not in EMULATOR_COV:
        raise ValueError(f"emulator_cov must be one of {EMULATOR_COV}, got {emulator_cov!r}")
    models = list(models)
    means, emu = model_predictions(models, X, batch)
    cands = []
    for f, y_err, cov, label in check_candidates(candidates, means.shape[1]):
        if emulator_cov == "mean":
            L = whitening_factor(f.size, cov, y_err)
            cov, y_err = L @ L.T + emu[np.ix_(f, f)], None
        cands.append(dict(features=f, y_err=y_err, cov=cov, label=label))
    return rank_measurements(means, cands, n_outer=n_outer, seed=seed, exclude_self=exclude_self,
                             device=models[0].device, workspace_bytes=workspace_bytes)
