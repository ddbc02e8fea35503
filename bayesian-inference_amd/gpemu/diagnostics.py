"""Rank-normalised split-R-hat, bulk / tail ESS and the ESS of the mean, computed where the chain lies.

The definitions are those of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021), as Stan, ``posterior`` and ArviZ
print them: for a segment ``x[n][M]`` of one parameter (n stored steps, M chains), split every chain in halves
(``N = n // 2`` rows each, an odd n drops the middle row), and with ``z(y)`` the normal scores of the pooled average ranks

    rhat      = max(Rhat(z(split x)), Rhat(z(split |x - median x|)))
    ess_bulk  = ESS(z(split x))
    ess_tail  = min(ESS(split 1[x <= q05]), ESS(split 1[x <= q95]))
    ess_mean  = ESS(split x)
    mcse_mean = sd(x, ddof 1) / sqrt(ess_mean)

The device ranks, transforms and forms the chain-averaged autocovariances (``gpemu_diag_*``); the host pulls them in
blocks of 64 lags and runs Geyer's scan (``geyer_ess``) until its first loop has ended for every parameter -- the
division of labour of ``DeviceSampler.integrated_time``.  A parameter with a non-finite value has every diagnostic NaN;
a transformed series that is constant (max - min < 1e-15) has ESS = N K and R-hat NaN, and ``rhat`` is NaN if either of
its two forms is.  There is no CPU implementation."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check, ptr

IDENTITY, RANK_Z, FOLDED_RANK_Z, INDICATOR_LE = 0, 1, 2, 3
PATHS = ("SORT_PASS", "RANK_LOOKUP", "TRANSFORM", "ACOV_BLOCK", "ROW_BATCH")
LAG_BLOCK = 64
KEYS = ("rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean")


def path_counts():
    """The library's counters of the diagnostics' launches since the process started, by name."""
    out = (C.c_int64 * len(PATHS))()
    n = _lib.lib().gpemu_diag_path_counts(out, len(PATHS))
    if n < 0:
        check(n)
    return {k: int(out[i]) for i, k in enumerate(PATHS)}


def plain_rhat(N, mean_var, b):
    """sqrt(((N - 1) / N W + b) / W) from the split chains' moments (W = ``mean_var``)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(((N - 1.0) / N * mean_var + b) / mean_var)


def geyer_ess(N, K, g, mean_var, b):
    """ESS of K chains of N draws from the chain-averaged biased autocovariances ``g[0 .. L)``, ``mean_var`` (the mean
    ddof-1 chain variance, ``g[0] N / (N - 1)``) and ``b`` (the ddof-1 variance of the chain means; not read for K = 1):
    Geyer's initial positive and monotone sequences as Stan and ArviZ run them.  Returns None where the first loop
    needs a lag beyond ``L`` (and L < N): the caller fetches another block."""
    g = np.asarray(g, dtype=np.float64)
    L = g.shape[0]
    var_plus = mean_var * (N - 1.0) / N
    if K > 1:
        var_plus = var_plus + b

    def rho_at(t):
        return 1.0 - (mean_var - g[t]) / var_plus

    if L < min(2, N):
        return None
    rho = np.zeros(N)
    even = 1.0
    rho[0] = even
    odd = rho_at(1)
    rho[1] = odd
    t = 1
    while t < N - 3 and even + odd > 0.0:
        if t + 2 >= L:
            return None
        even, odd = rho_at(t + 1), rho_at(t + 2)
        if even + odd >= 0.0:
            rho[t + 1], rho[t + 2] = even, odd
        t += 2
    max_t = t - 2
    if even > 0.0:
        rho[max_t + 1] = even
    t = 1
    while t <= max_t - 2:
        if rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]:
            rho[t + 1] = (rho[t - 1] + rho[t]) / 2.0
            rho[t + 2] = rho[t + 1]
        t += 2
    tau = -1.0 + 2.0 * np.sum(rho[:max_t + 1]) + rho[max_t + 1]
    tau = max(tau, 1.0 / math.log10(N * K))
    return N * K / tau


class Diag:
    """A segment ``[n][M][d]`` of a chain on the device (``gpemu_diag``): a host array is copied there, a float64
    device tensor ``[n][M][d]`` is read in place (and must outlive the handle).  ``from_sampler`` borrows the stored
    chain of a sampler handle: the library refuses it once the sampler has run, reserved, reset or restored."""

    def __init__(self, chain=None, device=None, workspace_bytes=0, _handle=None, _shape=None, _keep=None):
        self._h = C.c_void_p()
        self._keep = _keep
        if _handle is not None:
            self._h, (self.n, self.M, self.d) = _handle, _shape
            return
        if _lib.is_device_tensor(chain):
            import torch
            if chain.dtype != torch.float64 or chain.dim() != 3:
                raise TypeError("a device chain must be a float64 tensor [n][M][d]")
            chain = chain.contiguous()
            self._keep = chain
            n, M, d = (int(v) for v in chain.shape)
            check(_lib.lib().gpemu_diag_create_dev(C.byref(self._h), int(chain.device.index or 0),
                                                   C.c_void_p(chain.data_ptr()), n, M * d, 0, M, d, int(workspace_bytes),
                                                   _lib.current_stream(chain.device)))
        else:
            x = np.asarray(chain, dtype=np.float64)
            if x.ndim == 2:
                x = x[:, :, None]
            if x.ndim != 3:
                raise ValueError("chain must be [n][M] or [n][M][d]")
            x = np.ascontiguousarray(x)
            n, M, d = x.shape
            _lib.require_device()
            check(_lib.lib().gpemu_diag_create(C.byref(self._h), int(_lib.resolve_device(device)), ptr(x), n, M, d))
        self.n, self.M, self.d = n, M, d

    @classmethod
    def from_sampler(cls, handle, first, n, thin, w0, nw, d):
        h = C.c_void_p()
        check(_lib.lib().gpemu_sampler_diag_create(C.byref(h), handle, int(first), int(n), int(thin), int(w0), int(nw)))
        return cls(_handle=h, _shape=(int(n), int(nw), int(d)))

    @property
    def N(self):
        return self.n // 2

    @property
    def K(self):
        return 2 * self.M

    def close(self):
        if self._h:
            _lib.lib().gpemu_diag_destroy(self._h)
            self._h = C.c_void_p()
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def transform(self, kind, prob=0.0):
        """Writes the transformed split series and returns ``(grand_mean, mean_var, var_of_means)``, ``(d,)`` each."""
        gm, w, b = np.empty(self.d), np.empty(self.d), np.empty(self.d)
        check(_lib.lib().gpemu_diag_transform(self._h, int(kind), float(prob), ptr(gm), ptr(w), ptr(b)))
        return gm, w, b

    def value_range(self):
        lo, hi = np.empty(self.d), np.empty(self.d)
        check(_lib.lib().gpemu_diag_range(self._h, ptr(lo), ptr(hi)))
        return lo, hi

    def series(self):
        """The transformed split series as the device holds them: ``(N, 2 M, d)``, split chain h M + m."""
        y = np.empty((self.N, self.K, self.d))
        check(_lib.lib().gpemu_diag_series(self._h, ptr(y)))
        return y

    def acov(self, lag0, n_lags):
        g = np.empty((int(n_lags), self.d))
        check(_lib.lib().gpemu_diag_acov(self._h, int(lag0), int(n_lags), ptr(g)))
        return g

    def pooled(self):
        """``dict(mean, sd, median, min, max)`` of the pooled unsplit segment, ``(d,)`` each."""
        out = {k: np.empty(self.d) for k in ("mean", "sd", "median", "min", "max")}
        check(_lib.lib().gpemu_diag_pooled(self._h, *(ptr(out[k]) for k in ("mean", "sd", "median", "min", "max"))))
        return out

    # -- the two plain statistics of the current transform ------------------------------------------------------------
    def _rhat(self, kind):
        _, w, b = self.transform(kind)
        lo, hi = self.value_range()
        r = plain_rhat(self.N, w, b)
        r[~(hi - lo >= 1e-15)] = np.nan
        return r

    def _ess(self, kind, prob=0.0, moments=None):
        """ESS of every parameter for ``kind`` (transformed here unless its ``moments`` are passed: Y is current)."""
        N, K, d = self.N, self.K, self.d
        _, w, b = self.transform(kind, prob) if moments is None else moments
        lo, hi = self.value_range()
        ess = np.full(d, np.nan)
        todo = np.ones(d, dtype=bool)
        const = ~(hi - lo >= 1e-15)
        ess[const] = N * K
        todo[const] = False
        g = np.empty((0, d))
        while np.any(todo) and g.shape[0] < N:
            nl = min(LAG_BLOCK, N - g.shape[0])
            g = np.concatenate([g, self.acov(g.shape[0], nl)], axis=0)
            for dd in np.nonzero(todo)[0]:
                e = geyer_ess(N, K, g[:, dd], w[dd], b[dd])
                if e is not None:
                    ess[dd] = e
                    todo[dd] = False
        return ess

    def summary(self):
        """``dict`` of ``rhat, ess_bulk, ess_tail, ess_mean, mcse_mean`` (``(d,)`` each) plus ``n_chains`` (the 2 M
        split chains) and ``n_draws`` (N per split chain)."""
        N, d = self.N, self.d
        pooled = self.pooled()
        bad = ~(np.isfinite(pooled["min"]) & np.isfinite(pooled["max"]))
        mom = self.transform(RANK_Z)
        lo, hi = self.value_range()
        rhat_bulk = plain_rhat(N, mom[1], mom[2])
        rhat_bulk[~(hi - lo >= 1e-15)] = np.nan
        ess_bulk = self._ess(RANK_Z, moments=mom)
        rhat_fold = self._rhat(FOLDED_RANK_Z)
        ess_tail = np.minimum(self._ess(INDICATOR_LE, 0.05), self._ess(INDICATOR_LE, 0.95))
        ess_mean = self._ess(IDENTITY)
        out = {"rhat": np.maximum(rhat_bulk, rhat_fold), "ess_bulk": ess_bulk, "ess_tail": ess_tail, "ess_mean": ess_mean}
        with np.errstate(invalid="ignore", divide="ignore"):
            out["mcse_mean"] = pooled["sd"] / np.sqrt(ess_mean)
        for k in KEYS:
            out[k] = np.where(bad, np.nan, out[k])
        out["n_chains"] = self.K
        out["n_draws"] = N
        return out


def _with(chain_or_handle, fn, **kw):
    if isinstance(chain_or_handle, Diag):
        return fn(chain_or_handle)
    with Diag(chain_or_handle, **kw) as h:
        return fn(h)


def summary(chain_or_handle, device=None, workspace_bytes=0):
    """All five diagnostics of a chain ``[n][M][d]`` (host array or float64 device tensor) or of a ``Diag``."""
    return _with(chain_or_handle, lambda h: h.summary(), device=device, workspace_bytes=workspace_bytes)


def _masked(h, v):
    p = h.pooled()
    return np.where(np.isfinite(p["min"]) & np.isfinite(p["max"]), v, np.nan)


def rhat(chain_or_handle, **kw):
    return _with(chain_or_handle, lambda h: _masked(h, np.maximum(h._rhat(RANK_Z), h._rhat(FOLDED_RANK_Z))), **kw)


def ess_bulk(chain_or_handle, **kw):
    return _with(chain_or_handle, lambda h: _masked(h, h._ess(RANK_Z)), **kw)


def ess_tail(chain_or_handle, **kw):
    return _with(chain_or_handle,
                 lambda h: _masked(h, np.minimum(h._ess(INDICATOR_LE, 0.05), h._ess(INDICATOR_LE, 0.95))), **kw)


def ess_mean(chain_or_handle, **kw):
    return _with(chain_or_handle, lambda h: _masked(h, h._ess(IDENTITY)), **kw)


def mcse_mean(chain_or_handle, **kw):
    def f(h):
        with np.errstate(invalid="ignore", divide="ignore"):
            return _masked(h, h.pooled()["sd"] / np.sqrt(h._ess(IDENTITY)))
    return _with(chain_or_handle, f, **kw)


def log_line(diag, label="chain"):
    """One line for a run's log, and whether max R-hat exceeds the paper's threshold of 1.01."""
    r = np.asarray(diag["rhat"], dtype=np.float64)
    worst = float(np.nanmax(r)) if np.any(np.isfinite(r)) else float("nan")
    line = (f"{label}: max rhat {worst:.4f}, min ess_bulk {np.nanmin(diag['ess_bulk']):.0f}, "
            f"min ess_tail {np.nanmin(diag['ess_tail']):.0f}, min ess_mean {np.nanmin(diag['ess_mean']):.0f}")
    return line, bool(worst > 1.01)
