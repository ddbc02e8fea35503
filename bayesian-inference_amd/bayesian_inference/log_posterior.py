"""Drop-in replacement of ``bayesian_inference.log_posterior`` (ref: src/bayesian_inference/log_posterior.py).

``initialize_pool_variables`` keeps the reference's module-global calling convention; ``log_posterior(X)``
returns an ndarray of shape (n_samples,), ``-inf`` outside the open parameter box, evaluated by
libgpemu on the device.  The reference's batch semantics are kept: the truncation covariance is
divided by the number of IN-BOUNDS rows of the call (ref: log_posterior.py:67,80 ->
emulation.py:493,531-532), so one call with B rows differs from B single-row calls exactly as it
does upstream; emcee calls it with one walker at a time.  The ensemble sampler's fused device path
(``gpemu.sampler.DeviceSampler``) uses the single-walker semantics (n = 1).

A covariance that is not positive definite yields NaN (the reference's dpotrf error branch is dead
code, ref: log_posterior.py:125-135, and it would also compute with an invalid factor).

Correlated experimental uncertainties (the reference's TODO at log_posterior.py:90-94 resolved):
``experimental_results['cov']`` (F, F), in the merged observable order, replaces ``diag(y_err**2)`` inside each
observable and must be zero across observables; ``experimental_results['sys_sources']`` (S, F), S <= 16, adds
``sum_s b_s b_s^T``, spanning any observables and groups.  Without either key nothing changes.
"""
from __future__ import annotations

import logging

import numpy as np

from bayesian_inference import emulation

logger = logging.getLogger(__name__)

min = None
max = None
emulation_config = None
emulation_results = None
experimental_results = None
emulator_cov_unexplained = None

_state = {"models": None, "n_div": None, "data_cov": None}


def initialize_pool_variables(local_min, local_max, local_emulation_config, local_emulation_results,
                              local_experimental_results, local_emulator_cov_unexplained) -> None:
    """Same signature as the reference (ref: log_posterior.py:26-38); also drops cached device state."""
    global min, max, emulation_config, emulation_results, experimental_results, emulator_cov_unexplained
    min = local_min
    max = local_max
    emulation_config = local_emulation_config
    emulation_results = local_emulation_results
    experimental_results = local_experimental_results
    emulator_cov_unexplained = local_emulator_cov_unexplained
    _state["models"] = None
    _state["n_div"] = None
    _state["data_cov"] = None
    # the previous run's device models (k N^2 doubles each) are not needed any more
    emulation.release_device_models()


def _group_layouts():
    """[(group name, group config, columns in the merged observable order, observable block starts)]."""
    groups = list(emulation_config.emulation_groups_config.items())
    sorter = getattr(emulation_config, "sort_observables_in_matrix", None)
    out = []
    for name, cfg in groups:
        if hasattr(sorter, "group_layout"):
            cols, starts = sorter.group_layout(name)
        elif len(groups) == 1:     # single group whose matrix already is the merged matrix
            F = experimental_results['y'].shape[0]
            cols, starts = np.arange(F), np.array([0, F], dtype=np.int64)
        else:
            raise ValueError("multiple emulation groups need emulation_config.sort_observables_in_matrix "
                             "with a group_layout() (bayesian_inference.emulation.SortEmulationGroupObservables)")
        out.append((name, cfg, cols, starts))
    return out


def _observable_of_columns(F):
    """(observable index of every merged column, observable names): one observable without a sorter."""
    sorter = getattr(emulation_config, "sort_observables_in_matrix", None)
    mapping = getattr(sorter, "emulation_group_to_observable_matrix", None)
    if not mapping:
        return np.zeros(F, dtype=np.int64), ["all observables"]
    obs = np.full(F, -1, dtype=np.int64)
    names = []
    for i, (name, (_, slice_out, _)) in enumerate(sorted(mapping.items(), key=lambda e: e[1][1].start)):
        obs[slice_out] = i
        names.append(str(name))
    return obs, names


def data_covariance():
    """(cov or None, sys_sources or None) of ``experimental_results``, in the merged observable order, checked
    (once per ``initialize_pool_variables``)."""
    if _state["data_cov"] is None:
        _state["data_cov"] = _read_data_covariance()
    return _state["data_cov"]


def _read_data_covariance():
    er = experimental_results
    get = er.get if hasattr(er, "get") else (lambda key: er[key] if key in er else None)
    cov, src = get('cov'), get('sys_sources')
    F = np.asarray(er['y']).shape[0]
    if cov is not None:
        cov = np.ascontiguousarray(cov, dtype=np.float64)
        if cov.shape != (F, F):
            raise ValueError(f"experimental_results['cov'] must have shape ({F}, {F}), got {cov.shape}")
        if not np.all(np.isfinite(cov)) or not np.array_equal(cov, cov.T):
            raise ValueError("experimental_results['cov'] must be finite and symmetric")
        obs, names = _observable_of_columns(F)
        cross = (obs[:, None] != obs[None, :]) & (cov != 0.0)
        if np.any(cross):
            i, j = (int(v) for v in np.argwhere(cross)[0])
            raise ValueError(
                f"experimental_results['cov'][{i}, {j}] = {cov[i, j]:g} couples observables {names[obs[i]]!r} and "
                f"{names[obs[j]]!r}: only the covariance inside an observable may be dense; give correlations across "
                "observables as fully correlated sources, experimental_results['sys_sources'] (S, F)")
    if src is not None:
        src = np.ascontiguousarray(src, dtype=np.float64)
        if src.ndim != 2 or src.shape[1] != F:
            raise ValueError(f"experimental_results['sys_sources'] must have shape (S, {F}), got {src.shape}")
        if src.shape[0] > 16:
            raise ValueError(f"experimental_results['sys_sources'] holds {src.shape[0]} sources: at most 16 are supported")
        if not np.all(np.isfinite(src)):
            raise ValueError("experimental_results['sys_sources'] must be finite")
        if src.shape[0] == 0:
            src = None
    return cov, src


def _setup_group(dm, y, cols, starts, lo, hi, n_div, cov, src):
    """One group's likelihood setup: today's call without correlated uncertainties, else with its slices."""
    y_err = experimental_results['y_err']
    if cov is None and src is None:
        dm.likelihood_setup(y, y_err[cols], lo, hi, n_div=n_div, block_start=starts)
    else:
        dm.likelihood_setup(y, y_err[cols], lo, hi, n_div=n_div, block_start=starts,
                            cov=None if cov is None else cov[np.ix_(cols, cols)],
                            sys_sources=None if src is None else src[:, cols])


def device_models(n_div: float = 1.0):
    """Device models of all groups with the likelihood set up for ``n_div`` (cached)."""
    if _state["models"] is None:
        results = emulation_results or emulation_config.read_all_emulator_groups()
        models = []
        for name, cfg, cols, starts in _group_layouts():
            cov_un = emulator_cov_unexplained[name] if emulator_cov_unexplained else None
            models.append((emulation.device_model_for(results[name], cfg.n_pc, cov_un), cols, starts))
        _state["models"] = models
        _state["n_div"] = None
    if _state["n_div"] != float(n_div):
        lo = np.asarray(min, dtype=np.float64)
        hi = np.asarray(max, dtype=np.float64)
        y = experimental_results['y']
        cov, src = data_covariance()
        for dm, cols, starts in _state["models"]:
            _setup_group(dm, y[cols], cols, starts, lo, hi, float(n_div), cov, src)
        _state["n_div"] = float(n_div)
    return [m for m, _, _ in _state["models"]]


def chains_can_stack(config) -> bool:
    """Closure chains share one multi-chain device sampler for every configuration the device models support (any
    number of emulation groups, up to 64 PCs each: ``tests/test_gpu_shipped.py`` stacks the shipped three-group shape);
    what bounds a stacked run is chain memory, which ``mcmc._closure_sub_batches`` handles.  False only for a config
    without an ``emulators`` block (then there is nothing to run either way)."""
    try:
        groups = config.analysis_config['parameters']['emulators']
    except (KeyError, TypeError):
        return False
    return len(groups) >= 1


def device_models_for_chains(y_chains):
    """Device models (n_div = 1) with ONE DATA VECTOR PER CHAIN: ``y_chains`` (C, F) in the merged observable
    order; the uncertainties are those of ``experimental_results``."""
    y_chains = np.asarray(y_chains, dtype=np.float64)
    models = device_models(n_div=1.0)               # builds / caches the models
    lo = np.asarray(min, dtype=np.float64)
    hi = np.asarray(max, dtype=np.float64)
    cov, src = data_covariance()
    for dm, cols, starts in _state["models"]:
        _setup_group(dm, y_chains[:, cols], cols, starts, lo, hi, 1.0, cov, src)
    _state["n_div"] = None                          # the single-vector constants are gone
    return models


def log_posterior(X):
    """log-posterior of each row of X; shape (n_samples,) (ref: log_posterior.py:42-101)."""
    X = np.array(X, ndmin=2, dtype=np.float64)
    log_post = np.zeros(X.shape[0])
    inside = np.all((X > min) & (X < max), axis=1)
    log_post[~inside] = -np.inf
    n_samples = int(np.count_nonzero(inside))
    if n_samples > 0:
        models = device_models(n_div=n_samples)
        if data_covariance()[1] is not None:
            # sources span the groups: their term needs every group at once
            from gpemu.model import logpost_groups
            total = logpost_groups(models, X)
        else:
            total = np.zeros(X.shape[0])
            for dm in models:
                total += dm.logpost(X)          # rows outside the box come back as -inf
        log_post[inside] = total[inside]
    return log_post


def observable_labels():
    """The observable of every block of every group, in the order of ``log_likelihood_pointwise``'s rows (the groups'
    order, each group's blocks in turn): the sorter's observable names, ``<group>`` for a group of one block without
    a sorter."""
    F = np.asarray(experimental_results['y']).shape[0]
    obs, names = _observable_of_columns(F)
    labels = []
    for name, _, cols, starts in _group_layouts():
        for o in range(len(starts) - 1):
            i = obs[np.asarray(cols)[int(starts[o])]]
            labels.append(str(names[i]) if len(names) > 1 or i < 0 else str(name))
    return labels


def measurement_candidates(scale=1.0, observables=None):
    """The candidate measurements of ``gpemu.experiment`` that repeat the observables of this analysis
    independently with ``scale`` times their present uncertainties: one dict per observable label
    (``observable_labels()``: the blocks ``loo`` uses), or per entry of ``observables`` -- a label, or a list of labels
    measured together.  ``features`` index the groups' features concatenated in the order of ``device_models()``;
    ``y_err`` is ``scale * y_err`` of the data, or, where the data has a covariance, ``cov`` is ``scale^2`` times its
    block (blocks of different observables are independent).  Fully correlated sources are not part of a repeat's own
    uncertainty and are left out."""
    scale = float(scale)
    if not (np.isfinite(scale) and scale > 0.0):
        raise ValueError(f"scale must be finite and > 0, got {scale!r}")
    labels = observable_labels()
    y_err = np.asarray(experimental_results['y_err'], dtype=np.float64)
    cov = data_covariance()[0]
    blocks, off = [], 0          # per block: (features in the concatenated order, columns in the merged order)
    for _, _, cols, starts in _group_layouts():
        cols = np.asarray(cols)
        for o in range(len(starts) - 1):
            a, b = int(starts[o]), int(starts[o + 1])
            blocks.append((off + np.arange(a, b, dtype=np.int64), cols[a:b]))
        off += len(cols)
    if observables is None:
        classes = [[name] for name in labels]
    else:
        classes = [[c] if isinstance(c, str) else list(c) for c in observables]
        if len(classes) == 0 or any(len(c) == 0 for c in classes):
            raise ValueError("observables must be a non-empty list of labels or non-empty lists of labels")
    out = []
    for names in classes:
        for name in names:
            if labels.count(name) != 1:
                raise ValueError(f"observables names {name!r}; the observables are {labels}")
        feats = np.concatenate([blocks[labels.index(name)][0] for name in names])
        cols = np.concatenate([blocks[labels.index(name)][1] for name in names])
        cand = {'features': feats, 'label': '+'.join(names)}
        if cov is None:
            cand['y_err'] = scale * y_err[cols]
        else:
            cand['cov'] = (scale * scale) * cov[np.ix_(cols, cols)]
        out.append(cand)
    return out


def log_likelihood_pointwise(X):
    """``(labels, T)``: ``T (n_obs, n_samples)``, the log-likelihood term of every observable for each row of X -- the
    terms whose sum over the observables is ``log_posterior`` of a single row inside the box (n_div =
    1: every row on its own, as the sampler evaluates a walker).  A likelihood: no prior box.  Fully correlated sources
    (``experimental_results['sys_sources']``) span the observables, so the likelihood is no sum of terms: ValueError."""
    X = np.array(X, ndmin=2, dtype=np.float64)
    if data_covariance()[1] is not None:
        raise ValueError("log_likelihood_pointwise does not support experimental_results['sys_sources'] "
                         "(fully correlated sources span the observables)")
    from gpemu import loo
    return observable_labels(), loo.pointwise(device_models(n_div=1.0), X)


def log_posterior_and_gradient(X):
    """``(lp (B,), grad (B, d))``: the log-posterior of each row of X and its gradient with respect to the parameters
    (DESIGN.md §4.24), on the state ``initialize_pool_variables`` set.  Every row is evaluated on its own, as emcee
    evaluates a walker (the truncation covariance is not divided by the batch size: n_div = 1), so a row's value and
    gradient do not depend on the rest of the batch.  Rows outside the open box: ``-inf`` and a zero gradient.
    Fully correlated sources (``experimental_results['sys_sources']``) have no gradient path: ValueError."""
    X = np.array(X, ndmin=2, dtype=np.float64)
    if data_covariance()[1] is not None:
        raise ValueError("log_posterior_and_gradient does not support experimental_results['sys_sources'] "
                         "(fully correlated sources have no gradient path)")
    from gpemu.model import logpost_groups_grad
    return logpost_groups_grad(device_models(n_div=1.0), X)


# the ensemble sampler recognises this function and takes the fused device path (n_div = 1)
log_posterior._gpemu_device_models = lambda: device_models(n_div=1.0)
