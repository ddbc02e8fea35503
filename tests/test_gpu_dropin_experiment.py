"""-m gpu test of the drop-in's ``parameters.mcmc.expected_information_gain`` keys (bayesian_inference/mcmc.py;
DESIGN.md §4.38): with the key mcmc.h5 gains the documented ``eig_*`` entries, equal to
``mcmc.expected_information_gain(config)`` recomputed from the file, bit for bit; the tempered, HMC and closure-batch
runs write them too; without the key the file holds exactly its former keys."""
import numpy as np
import pytest

from test_gpu_dropin_loo import USUAL, _analysis, _labels

pytestmark = pytest.mark.gpu

EIG = {"eig_labels", "eig_nats", "eig_se", "eig_ess_mean", "eig_saturated"}


def _check_against_the_file(mcmc, cfg, back, closure_index=-1):
    """the entries' shapes, and the same entries from the stored chain, bit for bit"""
    assert _labels(back["eig_labels"]) == ["main"]
    for key in EIG - {"eig_labels"}:
        assert np.asarray(back[key]).shape == (1,), key
    assert np.isfinite(back["eig_nats"][0]) and back["eig_se"][0] > 0 and back["eig_ess_mean"][0] >= 1.0
    assert back["eig_saturated"][0] in (0, 1)
    again = mcmc.expected_information_gain(cfg, closure_index=closure_index)
    assert set(again) == EIG
    assert _labels(again["eig_labels"]) == ["main"]
    for key in EIG - {"eig_labels"}:
        assert np.asarray(back[key]).tobytes() == np.asarray(again[key]).tobytes(), key
    return again


def test_dropin_expected_information_gain_key(tmp_path, monkeypatch):
    from bayesian_inference import log_posterior, mcmc
    from gpemu import experiment as E, information as I
    path, analysis, h5io = _analysis(tmp_path, monkeypatch)
    mc = analysis["parameters"]["mcmc"]
    mc.update(n_burn_steps=20, n_sampling_steps=40)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert (cfg.expected_information_gain, cfg.eig_scale, cfg.eig_n_outer, cfg.eig_n_inner) == (False, 1.0, 4096, 16384)
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    plain = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(plain) == USUAL, set(plain)

    mc.update(expected_information_gain=True, eig_n_outer=256, eig_n_inner=500)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.expected_information_gain is True
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(back) == USUAL | EIG, set(back)
    assert np.array_equal(back["chain"], plain["chain"])           # the run itself is untouched
    _check_against_the_file(mcmc, cfg, back)
    # the module function on the chain: the repeat of the whole data vector with the emulator's mean covariance
    d = back["chain"].shape[2]
    rows = back["chain"].reshape(-1, d)
    X = np.ascontiguousarray(rows[I.selected_rows(rows.shape[0], 500)])
    cands = log_posterior.measurement_candidates()
    assert len(cands) == 1 and cands[0]["label"] == "main"
    out = E.chain_expected_information_gain(log_posterior.device_models(n_div=1.0), X, cands, n_outer=256)
    assert out["eig_nats"].tobytes() == np.asarray(back["eig_nats"]).tobytes()
    assert out["results"][0]["n_inner"] == 500 and out["results"][0]["n_outer"] == 256

    # half the uncertainty teaches more, and the setting reaches the file
    half = mcmc.expected_information_gain(cfg, scale=0.5)
    assert half["eig_nats"][0] > back["eig_nats"][0]
    mc.update(eig_scale=0.5)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    few = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert np.asarray(few["eig_nats"]).tobytes() == half["eig_nats"].tobytes()
    with pytest.raises(ValueError, match="observables"):
        mcmc.expected_information_gain(cfg, observables=["no such observable"])


def test_tempered_hmc_and_closure_runs_write_the_entries(tmp_path, monkeypatch):
    from bayesian_inference import mcmc
    written = {}
    path, analysis, h5io = _analysis(tmp_path, monkeypatch, written)
    mc = analysis["parameters"]["mcmc"]
    mc.update(n_burn_steps=20, n_sampling_steps=40, expected_information_gain=True, eig_n_outer=128, eig_n_inner=512)

    mc.update(n_temperatures=3)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    np.random.seed(5)
    mcmc.run_mcmc(cfg)
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert EIG <= set(back) and "betas" in back
    _check_against_the_file(mcmc, cfg, back)
    mc.pop("n_temperatures")

    mc.update(sampler="hmc", hmc_n_leapfrog=4, hmc_step_size=0.2)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    np.random.seed(5)
    mcmc.run_mcmc(cfg)
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert EIG <= set(back)
    _check_against_the_file(mcmc, cfg, back)
    for key in ("sampler", "hmc_n_leapfrog", "hmc_step_size"):
        mc.pop(key)

    analysis["validation_indices"] = [0, 2]
    mcmc._closure_done.clear()
    cfgs = [mcmc.MCMCConfig("test_analysis", "exponential", analysis, path, closure_index=j) for j in range(2)]
    np.random.seed(11)
    mcmc.run_mcmc(cfgs[0], closure_index=0)                      # runs both chains, stacked
    nats = []
    for j, c in enumerate(cfgs):
        back = h5io.read_dict_from_h5(c.mcmc_output_dir, "mcmc.h5")
        assert EIG <= set(back)
        _check_against_the_file(mcmc, cfgs[0], back, closure_index=j)
        nats.append(float(back["eig_nats"][0]))
    assert nats[0] != nats[1]                                    # each chain its own
    mcmc._closure_done.clear()
