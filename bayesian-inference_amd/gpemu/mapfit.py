"""Maximum of a log-posterior in a box from many starts at once.

The starts advance in lock step through ``estimators._LbfgsbRun`` -- scipy's L-BFGS-B with its default options, cut
where it asks for a value -- so that every round is ONE batched evaluation of ``value_and_grad``: on the device, the
rows of all starts in one call of the analytic gradient.  Each start ends where
``scipy.optimize.minimize(method="L-BFGS-B", jac=True)`` ends from it.  The driver knows nothing of the device: any
callable ``value_and_grad(X (n, d)) -> (lp (n,), grad (n, d))`` of a function to MAXIMISE will do.
"""
from __future__ import annotations

import numpy as np

from .estimators import _LbfgsbRun


def open_box_bounds(lo, hi):
    """(d, 2) bounds one float inside the box: the prior is strict (-inf ON the edge), L-BFGS-B's bounds are closed"""
    lo = np.asarray(lo, dtype=np.float64)
    hi = np.asarray(hi, dtype=np.float64)
    return np.stack([np.nextafter(lo, hi), np.nextafter(hi, lo)], axis=1)


def minimise_lockstep(neg_value_and_grad, starts, bounds):
    """L-BFGS-B from every row of ``starts`` (n, d) inside ``bounds`` (d, 2), all runs advanced together:
    ``neg_value_and_grad(X (m, d)) -> (f (m,), g (m, d))`` of the function to minimise is called once per round with
    the points the unfinished runs ask for.  A non-finite value is handed to the routine as +inf with a zero gradient
    (its line search backs off).  Returns ``x (n, d), f (n,), status (n,), nfev (n,), nit (n,)``; status as scipy's
    (0 converged, 1 iteration / evaluation limit, 2 abnormal termination)."""
    starts = np.array(starts, ndmin=2, dtype=np.float64)
    runs = [_LbfgsbRun(x0, bounds) for x0 in starts]
    while True:
        ask = []
        for idx, run in enumerate(runs):
            if run.done:
                continue
            x = run.advance()
            if x is not None:
                ask.append((idx, x))
        if not ask:
            break
        f, g = neg_value_and_grad(np.stack([x for _, x in ask]))
        f = np.asarray(f, dtype=np.float64)
        g = np.asarray(g, dtype=np.float64)
        for j, (idx, x) in enumerate(ask):
            if np.isfinite(f[j]) and np.all(np.isfinite(g[j])):
                runs[idx].supply(x, f[j], g[j].copy())
            else:
                runs[idx].supply(x, np.inf, np.zeros_like(x))
    return (np.stack([r.x for r in runs]), np.array([r.f for r in runs]), np.array([r.status for r in runs]),
            np.array([r.nfev for r in runs]), np.array([r.nit for r in runs]))


def hessian_steps(lo, hi, rel_step=1e-4):
    return rel_step * (np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64))


def central_hessian(value_and_grad, x, lo, hi, rel_step=1e-4):
    """(d, d) Hessian of the function at ``x`` from central differences of its analytic gradient: 2 d rows in one
    batch, ``H[:, i] = (grad(x + h_i e_i) - grad(x - h_i e_i)) / (2 h_i)``, ``h_i = rel_step (hi_i - lo_i)``, then
    symmetrised.  The scheme's error is ``h_i^2 / 6`` times the third derivative.  Where ``x`` is closer than ``2 h_i``
    to a face, the pair of coordinate i is centred ``2 h_i`` inside that face instead (both points stay at least
    ``h_i`` inside the open box); the column is then the derivative at that shifted point, off by the shift (at most
    ``2 h_i``) times the third derivative."""
    x = np.asarray(x, dtype=np.float64)
    d = x.size
    h = hessian_steps(lo, hi, rel_step)
    pts = np.empty((2 * d, d))
    for i in range(d):
        c = x.copy()
        c[i] = min(max(x[i], lo[i] + 2 * h[i]), hi[i] - 2 * h[i])
        pts[2 * i] = c
        pts[2 * i + 1] = c
        pts[2 * i, i] += h[i]
        pts[2 * i + 1, i] -= h[i]
    _, g = value_and_grad(pts)
    g = np.asarray(g, dtype=np.float64)
    H = np.stack([(g[2 * i] - g[2 * i + 1]) / (pts[2 * i, i] - pts[2 * i + 1, i]) for i in range(d)], axis=1)
    return 0.5 * (H + H.T)


def uniform_starts(lo, hi, n_starts, rng=None):
    rng = np.random.default_rng() if rng is None else rng
    return rng.uniform(lo, hi, (int(n_starts), len(lo)))


def best_distinct(chain, log_prob, count):
    """Positions of the ``count`` highest distinct log-probabilities of a stored chain (steps, walkers, d) /
    log_prob (steps, walkers): the rule of ``mcmc._best_distinct`` on the arrays of ``mcmc.h5``."""
    chain = np.asarray(chain, dtype=np.float64)
    flat = chain.reshape(-1, chain.shape[-1])
    _, first_seen = np.unique(np.asarray(log_prob, dtype=np.float64).reshape(-1), return_index=True)
    return flat[first_seen[-int(count):]]


def find_map(value_and_grad, starts, lo, hi, hessian=True):
    """The maximum of ``value_and_grad`` in the open box (lo, hi) from ``starts`` (n, d).  Returns a dict:
    ``map_parameters`` (d,), ``map_log_prob``, ``all_parameters`` (n, d), ``all_log_prob`` (n,), ``status`` (n,),
    ``nfev`` (n,), ``nit`` (n,) per start, and ``hessian`` (d, d) of the log-probability at the maximum
    (``central_hessian``; None without ``hessian``)."""
    lo = np.asarray(lo, dtype=np.float64)
    hi = np.asarray(hi, dtype=np.float64)

    def neg(X):
        lp, grad = value_and_grad(X)
        return -np.asarray(lp, dtype=np.float64), -np.asarray(grad, dtype=np.float64)

    x, f, status, nfev, nit = minimise_lockstep(neg, starts, open_box_bounds(lo, hi))
    best = int(np.argmin(f))
    return {
        'map_parameters': x[best].copy(), 'map_log_prob': float(-f[best]), 'all_parameters': x, 'all_log_prob': -f,
        'status': status, 'nfev': nfev, 'nit': nit,
        'hessian': central_hessian(value_and_grad, x[best], lo, hi) if hessian else None,
    }
