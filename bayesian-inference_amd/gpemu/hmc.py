"""Warm-up schedule and dual-averaging constants of the device HMC sampler (csrc/k_hmc.hip).

The step size adapts on the device after every iteration (``gpemu_sampler_hmc_adapt``); this module only decides when
the averaging restarts and when the metric is set: the Stan-like three-stage warm-up

    first 15 %   step size only
    next 75 %    doubling windows; at the end of each the inverse metric becomes the pooled variance of that window's
                 draws (``gpemu_sampler_chain_moments``, on the device) and the averaging restarts
    last 10 %    step size only; at its end the step size freezes at the averaged one
"""
from __future__ import annotations

import numpy as np

# dual averaging (Hoffman & Gelman 2014, algorithm 5); k_hmc.hip holds the same numbers
GAMMA = 0.05
T0 = 10.0
KAPPA = 0.75
MU_FACTOR = 10.0          # mu = log(MU_FACTOR * eps) at every (re)start
DEFAULT_TARGET_ACCEPT = 0.8
DEFAULT_JITTER = 0.1
DIVERGENCE_THRESHOLD = 1000.0

INITIAL_FRACTION = 0.15
FINAL_FRACTION = 0.10
FIRST_WINDOW = 25
# regularisation of a window's variance towards a small fraction of the prior's, as Stan shrinks towards 1e-3:
# var * n / (n + 5) + 1e-3 * prior_var * 5 / (n + 5), n = the window's iterations
SHRINK_WEIGHT = 5.0
SHRINK_SCALE = 1e-3


def dual_averaging_update(state, accept_prob, target):
    """One update of ``state = (eps, log_eps_bar, h_bar, m, mu)`` with an iteration's mean accept probability; returns
    the new state.  The recurrence of the device's hmc_adapt_kernel."""
    eps, log_eps_bar, h_bar, m, mu = state
    m = m + 1.0
    w = 1.0 / (m + T0)
    h_bar = (1.0 - w) * h_bar + w * (target - accept_prob)
    log_eps = mu - np.sqrt(m) / GAMMA * h_bar
    eta = m ** -KAPPA
    log_eps_bar = eta * log_eps + (1.0 - eta) * log_eps_bar
    return (float(np.exp(log_eps)), float(log_eps_bar), float(h_bar), m, mu)


def dual_averaging_start(eps):
    return (float(eps), 0.0, 0.0, 0.0, float(np.log(MU_FACTOR * eps)))


def warmup_schedule(n_warmup):
    """``[(iterations, set_metric_after)]``: the blocks of an ``n_warmup``-iteration warm-up, in order.  Below 20
    iterations: one block, step size only.  Windows double from FIRST_WINDOW (shorter if the middle stage is); the last
    window takes what remains when the next doubling would not fit."""
    n = int(n_warmup)
    if n <= 0:
        return []
    if n < 20:
        return [(n, False)]
    first = int(round(INITIAL_FRACTION * n))
    last = int(round(FINAL_FRACTION * n))
    middle = n - first - last
    blocks = [(first, False)]
    size = min(FIRST_WINDOW, middle)
    left = middle
    while left > 0:
        if left < 3 * size:            # the next (doubled) window would not fit after this one: this one takes the rest
            size = left
        blocks.append((size, True))
        left -= size
        size *= 2
    blocks.append((last, False))
    assert sum(b for b, _ in blocks) == n
    return [(b, m) for b, m in blocks if b > 0]


def regularised_metric(var, n_iterations, prior_var):
    """The inverse metric from a window's pooled variance (module constants)."""
    var = np.asarray(var, dtype=np.float64)
    n = float(n_iterations)
    return var * n / (n + SHRINK_WEIGHT) + SHRINK_SCALE * np.asarray(prior_var, dtype=np.float64) * SHRINK_WEIGHT / (n + SHRINK_WEIGHT)
