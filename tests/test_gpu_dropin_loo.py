"""-m gpu test of the drop-in's ``parameters.mcmc.loo`` key (bayesian_inference/mcmc.py): with the key
mcmc.h5 gains the documented ``loo_*`` entries, equal to ``mcmc.loo(config)`` recomputed from the file; a stacked closure
run writes them per chain, against each chain's own pseudo-data; without the key the file holds what it held before."""
import numpy as np
import pytest

import dropin_util as DU
import golden_util as GU

pytestmark = pytest.mark.gpu

USUAL = {"chain", "acceptance_fraction", "log_prob", "autocorrelation_time"}
EXACT = ("elpd_loo", "p_loo", "pareto_k", "k_threshold", "ess_w", "elpd_waic", "p_waic", "lppd", "se", "weighted_mean",
         "weighted_sd")


def _analysis(tmp_path, monkeypatch, written=None):
    """The g1 golden fitted through the drop-in's emulation module, behind the fake data layer."""
    from bayesian_inference import emulation
    from gpemu import h5io
    g = GU.load("g1_rbf_noise")
    io = DU.install_fake_data_IO(g["Y"], g["design"], g["y_exp"], g["y_err"], {} if written is None else written)
    io.read_dict_from_h5 = lambda output_dir, filename, verbose=True: h5io.read_dict_from_h5(output_dir, filename)
    path, analysis = DU.write_config(tmp_path, n_pc=5, n_restarts=0)
    ec = emulation.EmulationConfig.from_config_file("test_analysis", "exponential", path, analysis)
    ec._sort_observables_in_matrix = None
    np.random.seed(1)
    emulation.fit_emulators(ec)
    monkeypatch.setattr(emulation.EmulationConfig, "sort_observables_in_matrix",
                        property(lambda self: DU.TrivialSort("main")))
    monkeypatch.setattr(emulation.EmulationConfig, "observable_filter", property(lambda self: None))
    return path, analysis, h5io


def _labels(v):
    return [x.decode() if isinstance(x, bytes) else str(x) for x in np.atleast_1d(np.asarray(v)).tolist()]


def _loo_keys(mcmc):
    return {f"loo_{k}" for k in mcmc.LOO_KEYS} | {"loo_weighted_mean", "loo_weighted_sd", "loo_shift"}


def _check_against_the_file(mcmc, cfg, back, closure_index=-1):
    d = back["chain"].shape[2]
    assert _labels(back["loo_labels"]) == ["main"]
    assert back["loo_elpd_loo"].shape == (1,) and back["loo_shift"].shape == (1, d)
    assert np.all(back["loo_elpd_loo"] <= back["loo_lppd"]) and np.all(np.isfinite(back["loo_shift"]))
    again = mcmc.loo(cfg, closure_index=closure_index)      # from the file, through the host entries
    assert set(again) == _loo_keys(mcmc)
    for k in EXACT:
        assert np.asarray(back[f"loo_{k}"]).tobytes() == np.asarray(again[f"loo_{k}"]).tobytes(), k
    # the shift's baseline: the sampler's pooled chain moments in place, the same reduction under uniform weights from
    # the file -- two fixed trees
    assert np.allclose(back["loo_shift"], again["loo_shift"], rtol=0, atol=1e-10)


def test_dropin_loo_key(tmp_path, monkeypatch):
    from bayesian_inference import log_posterior, mcmc
    path, analysis, h5io = _analysis(tmp_path, monkeypatch)
    mc = analysis["parameters"]["mcmc"]
    mc.update(n_burn_steps=20, n_sampling_steps=40)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.loo is False and cfg.loo_leave_out is None
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    plain = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(plain) == USUAL, set(plain)

    mc.update(loo=True)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.loo is True
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(back) == USUAL | _loo_keys(mcmc), set(back)
    assert np.array_equal(back["chain"], plain["chain"])           # the run itself is untouched
    _check_against_the_file(mcmc, cfg, back)
    # the terms of the drop-in: one observable, whose term is the log-posterior of a row inside the box
    rows = back["chain"][-1][:6]
    labels, T = log_posterior.log_likelihood_pointwise(rows)
    assert labels == ["main"] and T.shape == (1, 6)
    lp = np.array([log_posterior.log_posterior(x)[0] for x in rows])
    assert np.allclose(T[0], lp, rtol=1e-10)
    # a class of observables by name; an unknown name is a warning and a file without the entries
    mc.update(loo_leave_out=[["main"]])
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    grouped = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert np.asarray(grouped["loo_elpd_loo"]).tobytes() == np.asarray(back["loo_elpd_loo"]).tobytes()
    mc.update(loo_leave_out=[["no such observable"]])
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    assert set(h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)) == USUAL


def test_stacked_closure_chains_write_their_own_loo(tmp_path, monkeypatch):
    from bayesian_inference import mcmc
    written = {}
    path, analysis, h5io = _analysis(tmp_path, monkeypatch, written)
    analysis["validation_indices"] = [0, 2]
    analysis["parameters"]["mcmc"].update(n_burn_steps=20, n_sampling_steps=40, loo=True)
    mcmc._closure_done.clear()
    cfgs = [mcmc.MCMCConfig("test_analysis", "exponential", analysis, path, closure_index=j) for j in range(2)]
    np.random.seed(11)
    mcmc.run_mcmc(cfgs[0], closure_index=0)                      # runs both chains, stacked
    assert all(c.mcmc_outputfile in written for c in cfgs)
    elpd = []
    for j, c in enumerate(cfgs):
        back = h5io.read_dict_from_h5(c.mcmc_output_dir, "mcmc.h5")
        assert _loo_keys(mcmc) <= set(back)
        _check_against_the_file(mcmc, cfgs[0], back, closure_index=j)
        elpd.append(float(back["loo_elpd_loo"][0]))
    assert elpd[0] != elpd[1]                                    # each against its own pseudo-data
    mcmc._closure_done.clear()
