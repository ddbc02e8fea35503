"""Host tests of the MAP driver (gpemu.mapfit) on analytic objectives and of the new interfaces that need no device:
the entry points by name, ``return_jacobian``'s merge and shapes, the YAML key's default, the refusals decided on the
host."""
from __future__ import annotations

import inspect
import os
import re

import numpy as np
import pytest
import scipy.optimize
import yaml

D = 5


def gaussian_in_box(seed, on_face):
    """a correlated Gaussian log-density with a small quartic term (so that third derivatives exist) in a box; the
    maximum inside the box, or -- the mean moved beyond the upper face of coordinate 0 -- on that face"""
    rng = np.random.default_rng(seed)
    Q = rng.normal(size=(D, D))
    A = Q @ Q.T + D * np.eye(D)
    lo, hi = -np.ones(D), np.ones(D) * 1.5
    mu = rng.uniform(-0.5, 0.8, D)
    if on_face:
        mu[0] = 2.5

    def value_and_grad(X):
        X = np.array(X, ndmin=2)
        lp, grad = np.empty(len(X)), np.empty(X.shape)
        for b, x in enumerate(X):          # row by row: a row's bits must not depend on the batch it comes in
            r = x - mu
            Ar = A @ r
            lp[b] = -0.5 * (r @ Ar) - 0.1 * np.sum(x ** 4)
            grad[b] = -Ar - 0.4 * x ** 3
        inside = np.all((X > lo) & (X < hi), axis=1)
        return np.where(inside, lp, -np.inf), np.where(inside[:, None], grad, 0.0)

    def hessian(x):
        return -A - 1.2 * np.diag(x ** 2)
    return value_and_grad, hessian, lo, hi


@pytest.mark.parametrize("on_face", [False, True])
def test_every_start_ends_where_scipy_ends(on_face):
    from gpemu import mapfit
    vg, _, lo, hi = gaussian_in_box(11, on_face)
    starts = np.random.default_rng(5).uniform(lo, hi, (9, D))
    batches = []

    def counted(X):
        batches.append(len(X))
        return vg(X)
    out = mapfit.find_map(counted, starts, lo, hi, hessian=False)
    bounds = mapfit.open_box_bounds(lo, hi)
    assert np.all(bounds[:, 0] > lo) and np.all(bounds[:, 1] < hi)
    assert np.array_equal(bounds[:, 0], np.nextafter(lo, hi)) and np.array_equal(bounds[:, 1], np.nextafter(hi, lo))
    for s, x0 in enumerate(starts):
        def neg(x):
            f, g = vg(x[None])
            return -f[0], -g[0]
        ref = scipy.optimize.minimize(neg, x0, method="L-BFGS-B", jac=True, bounds=bounds)
        np.testing.assert_array_equal(out["all_parameters"][s], ref.x)
        assert out["all_log_prob"][s] == -ref.fun
        assert out["status"][s] == ref.status == 0 and out["nfev"][s] == ref.nfev and out["nit"][s] == ref.nit
    assert out["status"].shape == out["nfev"].shape == (9,)
    best = int(np.argmax(out["all_log_prob"]))
    np.testing.assert_array_equal(out["map_parameters"], out["all_parameters"][best])
    assert out["map_log_prob"] == out["all_log_prob"][best]
    assert batches[0] == 9 and max(batches) == 9                  # one batched evaluation per round, all starts in the first
    assert len(batches) == int(out["nfev"].max())                 # ... and as many rounds as the longest run has evaluations
    if on_face:
        assert out["map_parameters"][0] == np.nextafter(hi[0], lo[0])
    else:
        assert np.all(out["map_parameters"] > lo + 1e-3) and np.all(out["map_parameters"] < hi - 1e-3)
    assert out["hessian"] is None


@pytest.mark.parametrize("on_face", [False, True])
def test_central_difference_hessian(on_face):
    """Against the analytic Hessian.  The gradient's only non-quadratic term is -0.4 x_i^3, whose central difference
    errs by exactly 0.4 h_i^2 on the diagonal (the scheme's h^2 / 6 f''' term); on a face the pair is centred up to
    2 h_i inside, which moves the diagonal entry by at most 2.4 |x_i| 2 h_i more.  Plus the rounding of the quotient."""
    from gpemu import mapfit
    vg, hess, lo, hi = gaussian_in_box(12, on_face)
    out = mapfit.find_map(vg, np.random.default_rng(6).uniform(lo, hi, (4, D)), lo, hi)
    x = out["map_parameters"]
    H = out["hessian"]
    assert H.shape == (D, D) and np.array_equal(H, H.T)
    h = mapfit.hessian_steps(lo, hi)
    _, g = vg(x[None])
    floor = 16 * np.finfo(float).eps * (np.abs(hess(x)) @ np.abs(x) + np.abs(g[0]) + 1.0).max() / h.min()
    tol = np.full((D, D), floor)
    tol[np.diag_indices(D)] += 0.4 * h ** 2
    shift = np.abs(x - np.clip(x, lo + 2 * h, hi - 2 * h))
    tol[np.diag_indices(D)] += 2.4 * (np.abs(x) + shift) * shift + 0.4 * shift ** 2 * 3
    assert np.all(np.abs(H - hess(x)) <= tol), (np.abs(H - hess(x)) / tol).max()
    if on_face:
        assert shift[0] > 0
    # teeth: the quartic term is seen (without it the diagonal would be off by 1.2 x_i^2)
    assert np.any(1.2 * x ** 2 > 10 * tol[np.diag_indices(D)])


def test_best_distinct_is_the_samplers_rule_on_stored_arrays():
    from bayesian_inference import mcmc
    from gpemu import mapfit
    rng = np.random.default_rng(0)
    chain = rng.normal(size=(7, 6, 3))
    lp = rng.normal(size=(7, 6))
    chain[3], lp[3] = chain[2], lp[2]                             # rejected moves: repeated points

    class S:
        flatchain = chain.reshape(-1, 3)
        flatlnprobability = lp.reshape(-1)
    np.testing.assert_array_equal(mapfit.best_distinct(chain, lp, 5), mcmc._best_distinct(S, 5))
    assert len(np.unique(mapfit.best_distinct(chain, lp, 5), axis=0)) == 5


def test_new_entry_points_are_declared_bound_and_exported():
    from gpemu import _lib, model
    names = ["gpemu_gp_predict_grad", "gpemu_gp_predict_grad_dev", "gpemu_logpost_grad", "gpemu_logpost_grad_dev",
             "gpemu_logpost_groups_grad", "gpemu_grad_path_counts"]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpemu.h")).read()
    declared = set(re.findall(r"\b(gpemu_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for n in names:
        assert n in declared and n in _lib.exported_symbols() and hasattr(L, n), n
    for n in ("GPEMU_GRAD_PATH_CHUNK", "GPEMU_GRAD_PATH_LOGLIK", "GPEMU_GRAD_PATH_CONTRACT_8", "GPEMU_GRAD_PATH_CONTRACT_16",
              "GPEMU_GRAD_PATH_JACOBIAN_8", "GPEMU_GRAD_PATH_JACOBIAN_16"):
        assert n in hdr
    for n in ("gp_predict_grad", "logpost_grad", "logpost_grad_dev"):
        assert callable(getattr(model.DeviceModel, n))
    assert callable(model.logpost_groups_grad) and callable(model.grad_path_counts)
    # the counters can be read without a device, and there are as many as the enum holds
    out = np.zeros(8, dtype=np.int64)
    import ctypes as C
    assert L.gpemu_grad_path_counts(out.ctypes.data_as(C.POINTER(C.c_int64)), 8) == 6


def test_public_surface_of_the_dropin_modules():
    from bayesian_inference import emulation, log_posterior, mcmc
    assert inspect.signature(emulation.predict).parameters["return_jacobian"].default is False
    assert list(inspect.signature(emulation.sensitivity).parameters) == ["parameters", "emulation_config",
                                                                          "emulation_group_results"]
    assert callable(log_posterior.log_posterior_and_gradient)
    sig = inspect.signature(mcmc.find_map).parameters
    assert sig["closure_index"].default == -1 and sig["n_starts"].default == 32 and sig["starts"].default is None
    # map_parameters keeps its behaviour
    post = np.random.default_rng(1).normal(size=(4000, 2)) * [1.0, 3.0] + [0.5, -2.0]
    est = mcmc.map_parameters(post)
    assert np.all(np.abs(est - np.median(post, axis=0)) < 0.01 * np.array([1.0, 3.0]))
    with pytest.raises(ValueError):
        mcmc.map_parameters(post, method="other")


def test_jacobian_backprojection_merge_and_sensitivity_shapes():
    from bayesian_inference import emulation
    rng = np.random.default_rng(2)
    B, d = 3, 4
    comps = {"a": rng.normal(size=(2, 5)), "b": rng.normal(size=(3, 4))}
    scales = {"a": rng.uniform(1, 2, 5), "b": rng.uniform(1, 2, 4)}
    dmeans = {"a": rng.normal(size=(B, 2, d)), "b": rng.normal(size=(B, 3, d))}
    jac = {n: emulation.backproject_jacobian(dmeans[n], comps[n], scales[n]) for n in comps}
    assert jac["a"].shape == (B, 5, d) and jac["b"].shape == (B, 4, d)
    b, f, i = 1, 3, 2
    assert np.isclose(jac["a"][b, f, i], scales["a"][f] * np.sum(comps["a"][:, f] * dmeans["a"][b, :, i]))
    # two observables per group, interleaved in the merged order
    mapping = {"o1": ("a", slice(0, 2), slice(0, 2)), "o2": ("b", slice(2, 5), slice(0, 3)),
               "o3": ("a", slice(5, 8), slice(2, 5)), "o4": ("b", slice(8, 9), slice(3, 4))}
    sorter = emulation.SortEmulationGroupObservables(mapping, (10, 9))
    J = emulation.merge_jacobians(sorter, jac)
    assert J.shape == (B, 9, d)
    cv = {n: {"central_value": jac[n][:, :, 0].copy()} for n in jac}
    merged = sorter.convert(cv)["central_value"]                     # the same placement as central_value's
    np.testing.assert_array_equal(J[:, :, 0], merged)
    X = rng.uniform(1, 2, (B, d))
    O = rng.uniform(1, 2, (B, 9))
    S = emulation.normalised_sensitivity(J, X, O)
    assert S.shape == (B, 9, d) and np.isclose(S[2, 7, 1], J[2, 7, 1] * X[2, 1] / O[2, 7])


def test_find_map_yaml_key_defaults_to_false(tmp_path):
    from bayesian_inference import mcmc
    top = {"observable_table_dir": "t", "observable_config_dir": "c", "observables_filename": "o",
           "output_dir": str(tmp_path / "out")}
    cfg_file = tmp_path / "config.yaml"
    cfg_file.write_text(yaml.safe_dump(top))
    mc = {"n_walkers": 4, "n_burn_steps": 1, "n_sampling_steps": 1, "n_logging_steps": 1}
    ana = {"parameters": {"mcmc": dict(mc)}, "parameterization": {"p": {"names": ["a"]}}}
    assert mcmc.MCMCConfig("ana", "p", ana, str(cfg_file)).find_map is False
    ana["parameters"]["mcmc"]["find_map"] = True
    assert mcmc.MCMCConfig("ana", "p", ana, str(cfg_file)).find_map is True
    ana["parameters"]["mcmc"]["find_map"] = False
    assert mcmc.MCMCConfig("ana", "p", ana, str(cfg_file)).find_map is False


def test_gradient_with_correlated_sources_is_refused_on_the_host():
    from bayesian_inference import log_posterior
    F = 4
    data = {"y": np.zeros(F), "y_err": np.ones(F), "sys_sources": np.ones((1, F))}
    log_posterior.initialize_pool_variables(np.zeros(2), np.ones(2), None, None, data, None)
    try:
        with pytest.raises(ValueError, match="sys_sources"):
            log_posterior.log_posterior_and_gradient(np.full((1, 2), 0.5))
    finally:
        log_posterior.initialize_pool_variables(None, None, None, None, None, None)


def test_non_finite_queries_are_refused_before_the_device():
    """gp_predict_grad validates like gp_predict (DeviceModel._finite): no handle is needed to get the ValueError"""
    from gpemu.model import DeviceModel
    dm = DeviceModel.__new__(DeviceModel)
    dm._h, dm.d, dm.k = None, 2, 1
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="NaN or infinity"):
            dm.gp_predict_grad(np.array([[0.1, bad]]))


def _fake_pool(kind, nu, sources):
    import types
    from bayesian_inference import log_posterior
    F = 4
    data = {"y": np.zeros(F), "y_err": np.ones(F)}
    if sources:
        data["sys_sources"] = np.ones((1, F))
    log_posterior.initialize_pool_variables(np.zeros(2), np.ones(2), None, None, data, None)
    emu = types.SimpleNamespace(kernel_=types.SimpleNamespace(kind=kind, nu=nu))
    cfg = types.SimpleNamespace(emulation_groups_config={"main": types.SimpleNamespace(n_pc=1)})
    return cfg, {"main": {"emulators": [emu]}}


@pytest.mark.parametrize("kind, nu, sources, word", [(0, np.inf, False, None), (1, 1.5, False, None), (1, 2.5, False, None),
                                                     (1, np.inf, False, None), (1, 0.5, False, "nu = 0.5"),
                                                     (1, 2.0, False, "nu = 2"), (0, np.inf, True, "sys_sources")])
def test_find_map_key_is_refused_before_sampling_where_the_gradient_is_declined(kind, nu, sources, word):
    """what run_mcmc asks before its first step when parameters.mcmc.find_map is set"""
    from bayesian_inference import log_posterior, mcmc
    cfg, res = _fake_pool(kind, nu, sources)
    try:
        reason = mcmc.find_map_unsupported(cfg, res)
        assert (reason is None) if word is None else (word in reason)
    finally:
        log_posterior.initialize_pool_variables(None, None, None, None, None, None)


def test_paths_that_do_not_read_the_find_map_key_say_so(caplog):
    import logging
    import types
    from bayesian_inference import mcmc
    with caplog.at_level(logging.WARNING, logger=mcmc.logger.name):
        mcmc._warn_find_map_not_read(types.SimpleNamespace(find_map=False), "the tempered run")
        assert not caplog.records
        mcmc._warn_find_map_not_read(types.SimpleNamespace(find_map=True), "the tempered run")
        mcmc._warn_find_map_not_read(types.SimpleNamespace(find_map=True), "the stacked closure chains")
    text = " ".join(r.getMessage() for r in caplog.records)
    assert "tempered run" in text and "stacked closure chains" in text and "map_*" in text
    import inspect
    src = inspect.getsource(mcmc.run_mcmc)
    assert src.count("_warn_find_map_not_read(config") == 2, "both paths that skip the key must warn"
