"""-m gpu test of the drop-in's ``parameters.mcmc.marginals`` key (bayesian_inference/mcmc.py): with
the key mcmc.h5 gains exactly the documented ``marginal_*`` arrays, equal to ``mcmc.marginals(config)`` recomputed from
the file; without it the file holds what it held before."""
import numpy as np
import pytest

import dropin_util as DU
import golden_util as GU

pytestmark = pytest.mark.gpu

USUAL = {"chain", "acceptance_fraction", "log_prob", "autocorrelation_time"}


def _analysis(tmp_path, monkeypatch):
    """The g1 golden fitted through the drop-in's emulation module, behind the fake data layer."""
    from bayesian_inference import emulation
    from gpemu import h5io
    g = GU.load("g1_rbf_noise")
    io = DU.install_fake_data_IO(g["Y"], g["design"], g["y_exp"], g["y_err"], {})
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


def test_dropin_marginals_key(tmp_path, monkeypatch):
    from bayesian_inference import mcmc
    from gpemu import marginals as M
    path, analysis, h5io = _analysis(tmp_path, monkeypatch)
    mc = analysis["parameters"]["mcmc"]
    mc.update(n_burn_steps=20, n_sampling_steps=40)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.marginals is False
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    plain = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(plain) == USUAL, set(plain)

    mc.update(marginals=True, marginals_bins=[24, 12], marginals_confidence=[0.68, 0.9])
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert (cfg.marginals, cfg.marginals_bins, cfg.marginals_confidence, cfg.marginals_kde) == (True, (24, 12), (0.68, 0.9), True)
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    keys = mcmc.MARGINALS_KEYS + mcmc.MARGINALS_KDE_KEYS
    assert set(keys) == set(M.KEYS)
    assert set(back) == USUAL | {f"marginal_{k}" for k in keys}, set(back)
    assert np.array_equal(back["chain"], plain["chain"])           # the run itself is untouched
    d = back["chain"].shape[2]
    S = back["chain"].shape[0] * back["chain"].shape[1]
    npairs = d * (d - 1) // 2
    shapes = {"edges_1d": (d, 25), "edges_2d": (d, 13), "hist_1d": (d, 24), "pairs": (npairs, 2),
              "hist_2d": (npairs, 12, 12), "n_inside": (d,), "confidence": (2,), "hpd": (2, d, 2), "kde_grid": (d, 200),
              "kde_density": (d, 200), "kde_bandwidth": (d,)}
    for k, shape in shapes.items():
        assert back[f"marginal_{k}"].shape == shape, k
    for k in ("hist_1d", "hist_2d", "n_inside", "pairs"):
        assert back[f"marginal_{k}"].dtype == np.int64, k
    assert np.all(back["marginal_n_inside"] == S)                  # the box is the prior box: every sample lies inside
    assert np.all(back["marginal_hist_2d"].sum(axis=(1, 2)) == S)
    box = analysis["parameterization"]["exponential"]
    assert np.array_equal(back["marginal_edges_1d"][:, 0], np.asarray(box["min"], dtype=np.float64))
    assert np.array_equal(back["marginal_edges_1d"][:, -1], np.asarray(box["max"], dtype=np.float64))

    again = mcmc.marginals(cfg)                                    # from the file, through the host entries
    flat = back["chain"].reshape(-1, d)
    for k in ("edges_1d", "edges_2d", "hist_1d", "pairs", "hist_2d", "n_inside", "confidence", "hpd"):
        assert np.array_equal(back[f"marginal_{k}"], again[k]), k
    for j in range(d):                                             # the interval is the drop-in's own, per parameter
        lo, hi = mcmc.credible_interval(flat[:, j], 0.68, "hpd")
        assert (back["marginal_hpd"][0, j, 0], back["marginal_hpd"][0, j, 1]) == (lo, hi)
    # the stored bandwidth and support come from device moments (Scott's rule up to their rounding); on them the
    # density is the module function's, bit for bit
    assert np.allclose(back["marginal_kde_bandwidth"], again["kde_bandwidth"], rtol=1e-12, atol=0.0)
    dens = M.kde_1d(flat, grid=back["marginal_kde_grid"], bandwidth=back["marginal_kde_bandwidth"])["density"]
    assert back["marginal_kde_density"].tobytes() == dens.tobytes()
    thinned = mcmc.marginals(cfg, discard=4, thin=2)
    assert np.all(thinned["n_inside"] == 18 * back["chain"].shape[1])

    mc.update(marginals_kde=False)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    lean = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(lean) == USUAL | {f"marginal_{k}" for k in mcmc.MARGINALS_KEYS}, set(lean)
    assert np.array_equal(lean["marginal_hist_2d"], back["marginal_hist_2d"])
