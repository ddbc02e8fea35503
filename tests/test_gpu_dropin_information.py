"""-m gpu test of the drop-in's ``parameters.mcmc.information_gain`` keys (bayesian_inference/mcmc.py):
with the key mcmc.h5 gains the documented ``information_gain_*`` entries, equal to ``mcmc.information_gain(config)``
recomputed from the file and to the module function on the chain; the tempered, HMC and closure-batch runs write them
too; without the key the file holds what it held before."""
import numpy as np
import pytest

from test_gpu_dropin_loo import USUAL, _analysis

pytestmark = pytest.mark.gpu


def _keys(mcmc):
    return {f"information_gain_{k}" for k in mcmc.INFORMATION_GAIN_KEYS}


def _check_against_the_file(mcmc, cfg, back, closure_index=-1, k=4):
    """the entries' shapes, and the same entries from the stored chain through the host entry, bit for bit"""
    from gpemu import information as I
    d = back["chain"].shape[2]
    S = back["chain"].shape[0] * back["chain"].shape[1]
    subs = I.default_subsets(d)
    P = len(subs)
    assert back["information_gain_masks"].tolist() == [sum(1 << j for j in s) for s in subs]
    assert back["information_gain_dims"].tolist() == [len(s) for s in subs]
    for key in ("nats", "bits", "se", "n_used", "copies"):
        assert back[f"information_gain_{key}"].shape == (P,), key
    assert back["information_gain_per_parameter"].shape == (d,)
    assert back["information_gain_pairs"].shape == (d * (d - 1) // 2, 2) == back["information_gain_per_pair"].shape + (2,)
    assert int(back["information_gain_n_points"]) == S and int(back["information_gain_k"]) == k
    assert np.all(back["information_gain_n_used"] == S) and np.all(np.isfinite(back["information_gain_nats"]))
    assert float(back["information_gain_joint"]) == back["information_gain_nats"][-1]
    assert np.array_equal(back["information_gain_per_parameter"], back["information_gain_nats"][:d])
    assert float(back["information_gain_joint"]) > 0.0             # the data taught something
    again = mcmc.information_gain(cfg, closure_index=closure_index)
    assert set(again) == _keys(mcmc)
    for key in again:
        assert np.asarray(back[key]).tobytes() == np.asarray(again[key]).tobytes(), key
    return again


def test_dropin_information_gain_key(tmp_path, monkeypatch):
    from bayesian_inference import mcmc
    from gpemu import information as I
    path, analysis, h5io = _analysis(tmp_path, monkeypatch)
    mc = analysis["parameters"]["mcmc"]
    mc.update(n_burn_steps=20, n_sampling_steps=40)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert (cfg.information_gain, cfg.information_gain_k, cfg.information_gain_max_points) == (False, 4, 65536)
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    plain = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(plain) == USUAL, set(plain)

    mc.update(information_gain=True)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.information_gain is True
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(back) == USUAL | _keys(mcmc), set(back)
    assert np.array_equal(back["chain"], plain["chain"])           # the run itself is untouched
    _check_against_the_file(mcmc, cfg, back)
    # the module function on the chain, with the configuration's box
    box = analysis["parameterization"]["exponential"]
    d = back["chain"].shape[2]
    out = I.information_gain(back["chain"].reshape(-1, d), np.asarray(box["min"], dtype=np.float64),
                             np.asarray(box["max"], dtype=np.float64), allow_copies=True)
    assert out["nats"].tobytes() == back["information_gain_nats"].tobytes()
    assert out["se"].tobytes() == back["information_gain_se"].tobytes()
    assert np.array_equal(out["copies"], back["information_gain_copies"])

    # the two settings: another neighbour, fewer rows
    mc.update(information_gain_k=2, information_gain_max_points=100)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    few = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert int(few["information_gain_k"]) == 2 and int(few["information_gain_n_points"]) == 100
    sel = I.selected_rows(back["chain"].shape[0] * back["chain"].shape[1], 100)
    out = I.information_gain(back["chain"].reshape(-1, d)[sel], np.asarray(box["min"], dtype=np.float64),
                             np.asarray(box["max"], dtype=np.float64), k=2, allow_copies=True)
    assert out["nats"].tobytes() == few["information_gain_nats"].tobytes()


def test_the_sampler_method_is_the_module_function_on_get_chain():
    from test_gpu_row_views import _stacked
    from gpemu import information as I
    s, dm, full, lo, hi = _stacked()
    W = full.shape[1] // 2
    for chain in (0, 1):
        got = s.information_gain(chain=chain, k=3, allow_copies=True)
        rows = np.ascontiguousarray(s.get_chain()[0][:, chain * W:(chain + 1) * W]).reshape(-1, lo.size)
        want = I.information_gain(rows, lo, hi, k=3, allow_copies=True)
        assert got["subsets"] == want["subsets"] == I.default_subsets(lo.size)
        for key in ("nats", "bits", "se", "n_used", "copies", "per_parameter", "per_pair"):
            assert np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), key


def test_tempered_hmc_and_closure_runs_write_the_entries(tmp_path, monkeypatch):
    from bayesian_inference import mcmc
    written = {}
    path, analysis, h5io = _analysis(tmp_path, monkeypatch, written)
    mc = analysis["parameters"]["mcmc"]
    mc.update(n_burn_steps=20, n_sampling_steps=40, information_gain=True)

    mc.update(n_temperatures=3)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    np.random.seed(5)
    mcmc.run_mcmc(cfg)
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert _keys(mcmc) <= set(back) and "betas" in back
    _check_against_the_file(mcmc, cfg, back)
    mc.pop("n_temperatures")

    mc.update(sampler="hmc", hmc_n_leapfrog=4, hmc_step_size=0.2)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    np.random.seed(5)
    mcmc.run_mcmc(cfg)
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert _keys(mcmc) <= set(back)
    _check_against_the_file(mcmc, cfg, back)
    for key in ("sampler", "hmc_n_leapfrog", "hmc_step_size"):
        mc.pop(key)

    analysis["validation_indices"] = [0, 2]
    mcmc._closure_done.clear()
    cfgs = [mcmc.MCMCConfig("test_analysis", "exponential", analysis, path, closure_index=j) for j in range(2)]
    np.random.seed(11)
    mcmc.run_mcmc(cfgs[0], closure_index=0)                      # runs both chains, stacked
    joint = []
    for j, c in enumerate(cfgs):
        back = h5io.read_dict_from_h5(c.mcmc_output_dir, "mcmc.h5")
        assert _keys(mcmc) <= set(back)
        _check_against_the_file(mcmc, cfgs[0], back, closure_index=j)
        joint.append(float(back["information_gain_joint"]))
    assert joint[0] != joint[1]                                  # each chain its own
    mcmc._closure_done.clear()
