"""Host-side pieces of parallel tempering: the temperature ladder and the thermodynamic-integration
log-evidence.  The tempered sampler itself is ``gpemu.sampler.TemperedSampler``."""
from __future__ import annotations

import math

import numpy as np


def geometric_ladder(n_temps, t_max, prior_rung=True):
    """Inverse temperatures ``beta_t = t_max ** (-t / (m - 1))`` for ``t < m``, from 1 down to ``1 / t_max``.
    ``prior_rung``: ``m = n_temps - 1`` and ``beta = 0`` (the prior) is appended as the last rung; otherwise
    ``m = n_temps``.  ``2 <= n_temps <= 64``, ``t_max >= 1`` finite."""
    if isinstance(n_temps, bool) or int(n_temps) != n_temps:
        raise ValueError(f"n_temps must be an integer, got {n_temps!r}")
    n_temps = int(n_temps)
    if not 2 <= n_temps <= 64:
        raise ValueError(f"n_temps must be in [2, 64], got {n_temps}")
    t_max = float(t_max)
    if not (math.isfinite(t_max) and t_max >= 1.0):
        raise ValueError(f"t_max must be finite and >= 1, got {t_max}")
    m = n_temps - 1 if prior_rung else n_temps
    if m == 1:
        betas = np.ones(1)
    else:
        betas = t_max ** (-np.arange(m) / (m - 1.0))
    if prior_rung:
        betas = np.concatenate([betas, [0.0]])
    return betas


def _trapz(y, x):
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return float(np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(x)))


def thermodynamic_integration_log_evidence(betas, logls):
    """log Z = int_0^1 <log L>_beta d beta by the trapezoid rule over the ladder, and the error estimate
    |log Z - log Z'| with log Z' from every other rung (emcee 2's ``PTSampler.thermodynamic_integration_log_evidence``).
    Without a beta = 0 rung the hottest rung's mean stands in for it.  Returns ``(logZ, dlogZ)``."""
    betas = np.asarray(betas, dtype=np.float64)
    logls = np.asarray(logls, dtype=np.float64)
    if betas.shape != logls.shape or betas.ndim != 1 or betas.size < 1:
        raise ValueError("need one mean log-likelihood per temperature")
    order = np.argsort(betas, kind="stable")[::-1]
    betas, logls = betas[order], logls[order]
    if betas[-1] != 0:
        b = np.concatenate([betas, [0.0]])
        l = np.concatenate([logls, [logls[-1]]])
        b2 = np.concatenate([betas[::2], [0.0]])
        l2 = np.concatenate([logls[::2], [logls[-1]]])
    else:
        b, l = betas, logls
        b2 = np.concatenate([betas[:-1:2], [0.0]])
        l2 = np.concatenate([logls[:-1:2], [logls[-1]]])
    logz = -_trapz(l, b)
    logz2 = -_trapz(l2, b2)
    return logz, abs(logz - logz2)
