"""Correlated experimental uncertainties, host side: the Woodbury / source algebra of the device in
float64 against the reference's dense formula in extended precision, and the drop-in's validation of ``cov`` /
``sys_sources`` and of ``parameters.mcmc.data_covariance``."""
from types import SimpleNamespace

import numpy as np
import pytest

import srccorr_ref as R
from oracle import gp_oracle as O


def _predict(c, X):
    means, vars_ = [], []
    for model, _, _ in c["groups"]:
        m, v = O.gp_predict_all(X, model)
        means.append(np.asarray(m, dtype=np.float64))
        vars_.append(np.asarray(v, dtype=np.float64))
    return means, vars_


@pytest.mark.parametrize("name", ["G1", "G5", "G7"])
@pytest.mark.parametrize("S", [0, 1, 4, 16])
@pytest.mark.parametrize("correlated", [False, True])
def test_woodbury_sources_equal_dense_formula(name, S, correlated):
    c = R.case(name)
    X = c["Xq"][:5]
    means, vars_ = _predict(c, X)
    Cd, cov, src = R.data_covariance(c, S, seed=7 + S, correlated=correlated)
    ref, *_ = R.dense_logpost(c, X, means, vars_, Cd)
    zero = [np.zeros_like(m) for m in means]
    bnd = R.bound(c, X, means, vars_, zero, zero, Cd, src)
    setups = [R.woodbury_setup(model, cols, bs, c["y"], c["y_err"], cov, src) for model, cols, bs in c["groups"]]
    got = R.woodbury_logpost(setups, means, vars_, S)
    inside = np.isfinite(np.asarray(ref, dtype=np.float64))
    assert inside.any()
    err = np.abs(got[inside] - np.asarray(ref[inside], dtype=np.float64))
    assert np.all(err <= bnd[inside]), (err, bnd[inside])
    if S > 0:       # the sources matter at this size: the test would see a missing or wrong term
        Cd0 = Cd - src.T @ src
        ref0, *_ = R.dense_logpost(c, X, means, vars_, Cd0)
        assert np.all(np.abs(np.asarray(ref0 - ref, dtype=np.float64))[inside] > 1e3 * bnd[inside])


# ---- the drop-in: experimental_results['cov'] / ['sys_sources'] ------------------------------------------------------
@pytest.fixture
def dropin(monkeypatch):
    from bayesian_inference import log_posterior as LP
    F = 10
    mapping = {"obs_a": ("g1", slice(0, 4), slice(0, 4)), "obs_b": ("g1", slice(4, 10), slice(4, 10))}
    cfg = SimpleNamespace(sort_observables_in_matrix=SimpleNamespace(emulation_group_to_observable_matrix=mapping))
    monkeypatch.setattr(LP, "emulation_config", cfg)
    monkeypatch.setitem(LP._state, "data_cov", None)
    y_err = np.linspace(0.5, 1.0, F)

    def set_data(**extra):
        monkeypatch.setattr(LP, "experimental_results", dict(y=np.zeros(F), y_err=y_err, **extra))
        LP._state["data_cov"] = None
    return LP, F, y_err, set_data


def test_dropin_without_keys_changes_nothing(dropin):
    LP, F, y_err, set_data = dropin
    set_data()
    assert LP.data_covariance() == (None, None)


def test_dropin_accepts_within_observable_cov_and_sources(dropin):
    LP, F, y_err, set_data = dropin
    obs = np.array([0] * 4 + [1] * 6)
    cov = R.within_cov(y_err, obs)
    src = R.sources(y_err, 3, seed=1)
    set_data(cov=cov, sys_sources=src)
    got_cov, got_src = LP.data_covariance()
    np.testing.assert_array_equal(got_cov, cov)
    np.testing.assert_array_equal(got_src, src)


def test_dropin_rejects_cross_observable_cov(dropin):
    LP, F, y_err, set_data = dropin
    cov = np.diag(y_err ** 2)
    cov[2, 7] = cov[7, 2] = 0.01
    set_data(cov=cov)
    with pytest.raises(ValueError) as e:
        LP.data_covariance()
    msg = str(e.value)
    assert "obs_a" in msg and "obs_b" in msg and "sys_sources" in msg


@pytest.mark.parametrize("bad", ["asymmetric", "shape", "nan"])
def test_dropin_rejects_malformed_cov(dropin, bad):
    LP, F, y_err, set_data = dropin
    cov = np.diag(y_err ** 2)
    if bad == "asymmetric":
        cov[1, 0] = 0.1
    elif bad == "shape":
        cov = cov[:-1, :-1]
    else:
        cov[3, 3] = np.nan
    set_data(cov=cov)
    with pytest.raises(ValueError):
        LP.data_covariance()


def test_dropin_rejects_more_than_16_sources(dropin):
    LP, F, y_err, set_data = dropin
    set_data(sys_sources=np.ones((17, F)))
    with pytest.raises(ValueError, match="at most 16"):
        LP.data_covariance()
    set_data(sys_sources=np.ones((2, F + 1)))
    with pytest.raises(ValueError, match="shape"):
        LP.data_covariance()


def test_dropin_zero_sources_is_no_sources(dropin):
    LP, F, y_err, set_data = dropin
    set_data(sys_sources=np.zeros((0, F)))
    assert LP.data_covariance() == (None, None)


# ---- parameters.mcmc.data_covariance ---------------------------------------------------------------------------------
def test_data_covariance_key_adds_arrays(tmp_path):
    from bayesian_inference import mcmc
    F = 6
    cov = np.diag(np.arange(1.0, F + 1))
    src = np.ones((2, F))
    path = tmp_path / "dcov.npz"
    np.savez(path, cov=cov, sys_sources=src)
    data = {"y": np.zeros(F), "y_err": np.ones(F)}
    out = mcmc._with_data_covariance(SimpleNamespace(data_covariance=str(path)), data)
    np.testing.assert_array_equal(out["cov"], cov)
    np.testing.assert_array_equal(out["sys_sources"], src)
    assert "cov" not in data                                  # the caller's dict is left alone
    assert mcmc._with_data_covariance(SimpleNamespace(data_covariance=None), data) is data
    assert mcmc._with_data_covariance(SimpleNamespace(), data) is data
    np.savez(tmp_path / "empty.npz", other=np.zeros(1))
    with pytest.raises(ValueError, match="neither"):
        mcmc._with_data_covariance(SimpleNamespace(data_covariance=str(tmp_path / "empty.npz")), data)


def test_data_covariance_key_read_from_config(tmp_path):
    import yaml
    from bayesian_inference import mcmc
    top = {"observable_table_dir": "t", "observable_config_dir": "c", "observables_filename": "o",
           "output_dir": str(tmp_path / "out")}
    cfg_file = tmp_path / "config.yaml"
    cfg_file.write_text(yaml.safe_dump(top))
    mc = {"n_walkers": 4, "n_burn_steps": 1, "n_sampling_steps": 1, "n_logging_steps": 1}
    ana = {"parameters": {"mcmc": dict(mc)}, "parameterization": {"p": {"names": ["a"]}}}
    c0 = mcmc.MCMCConfig("ana", "p", ana, str(cfg_file))
    assert c0.data_covariance is None
    ana["parameters"]["mcmc"]["data_covariance"] = "dcov.npz"
    c1 = mcmc.MCMCConfig("ana", "p", ana, str(cfg_file))
    assert c1.data_covariance == str(tmp_path / "dcov.npz")
