"""-m gpu test of the drop-in's ``parameters.mcmc.marginals_kde2d`` keys (bayesian_inference/mcmc.py):
with the key mcmc.h5 gains the six ``marginal_kde2d_*`` arrays with the documented shapes, ``mcmc.marginals(config)``
reproduces them from the file, and without the key the file holds exactly what it held before."""
import numpy as np
import pytest

from test_gpu_dropin_marginals import USUAL, _analysis

pytestmark = pytest.mark.gpu


def test_dropin_marginals_kde2d_key(tmp_path, monkeypatch):
    from bayesian_inference import mcmc
    from gpemu import marginals as M
    path, analysis, h5io = _analysis(tmp_path, monkeypatch)
    mc = analysis["parameters"]["mcmc"]
    mc.update(n_burn_steps=20, n_sampling_steps=40, marginals=True, marginals_bins=[24, 12])
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert (cfg.marginals_kde2d, cfg.marginals_kde2d_grid, cfg.marginals_kde2d_covariance) == (False, 100, "full")
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    before = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    today = USUAL | {f"marginal_{k}" for k in mcmc.MARGINALS_KEYS + mcmc.MARGINALS_KDE_KEYS}
    assert set(before) == today, set(before)

    G = 24
    mc.update(marginals_kde2d=True, marginals_kde2d_grid=G)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert (cfg.marginals_kde2d, cfg.marginals_kde2d_grid, cfg.marginals_kde2d_covariance) == (True, G, "full")
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(mcmc.MARGINALS_KDE2D_KEYS) == set(M.KEYS_KDE2D)
    assert set(back) == today | {f"marginal_{k}" for k in mcmc.MARGINALS_KDE2D_KEYS}, set(back)
    for k in before:                                                # the run and the other marginals are untouched
        assert np.array_equal(back[k], before[k]), k
    d = back["chain"].shape[2]
    P = d * (d - 1) // 2
    shapes = {"kde2d_pairs": (P, 2), "kde2d_shear": (P,), "kde2d_bandwidth": (P, 2), "kde2d_grid_a": (P, G),
              "kde2d_grid_b": (P, G), "kde2d_density": (P, G, G)}
    for k, shape in shapes.items():
        assert back[f"marginal_{k}"].shape == shape, k
    assert back["marginal_kde2d_pairs"].dtype == np.int64
    assert np.array_equal(back["marginal_kde2d_pairs"], back["marginal_pairs"])
    flat = back["chain"].reshape(-1, d)
    S = flat.shape[0]
    c = np.cov(flat, rowvar=False, ddof=1)
    for p, (i, j) in enumerate(back["marginal_kde2d_pairs"]):
        assert np.isclose(back["marginal_kde2d_shear"][p], c[i, j] / c[i, i], rtol=1e-9, atol=1e-12)
        assert np.isclose(back["marginal_kde2d_bandwidth"][p, 0], S ** (-1 / 6) * np.sqrt(c[i, i]), rtol=1e-10, atol=0.0)
    # a density over its support (the tails beyond 3 h hold ~1e-3; the short chain is lumpy, the sum is not)
    cell = np.diff(back["marginal_kde2d_grid_a"], axis=1)[:, 0] * np.diff(back["marginal_kde2d_grid_b"], axis=1)[:, 0]
    area = back["marginal_kde2d_density"].sum(axis=(1, 2)) * cell
    assert np.all(np.abs(area - 1.0) < 2e-2), area

    again = mcmc.marginals(cfg)                                    # from the file, through the host entry
    assert set(again) == set(M.KEYS) | set(M.KEYS_KDE2D)
    assert np.array_equal(again["kde2d_pairs"], back["marginal_kde2d_pairs"])
    assert np.allclose(again["kde2d_shear"], back["marginal_kde2d_shear"], rtol=1e-10, atol=1e-13)
    assert np.allclose(again["kde2d_bandwidth"], back["marginal_kde2d_bandwidth"], rtol=1e-10, atol=0.0)
    for k in ("grid_a", "grid_b"):
        assert np.allclose(again["kde2d_" + k], back["marginal_kde2d_" + k], rtol=0.0,
                           atol=1e-10 * np.abs(again["kde2d_" + k]).max()), k
    # on the stored plan the density is the module function's, bit for bit
    given = {k: back["marginal_kde2d_" + k] for k in ("pairs", "shear", "bandwidth", "grid_a", "grid_b")}
    dens = M.kde_2d(flat, **given)["density"]
    assert back["marginal_kde2d_density"].tobytes() == dens.tobytes()
    levels = M.density_levels(back["marginal_kde2d_density"], [0.68, 0.95])
    assert levels.shape == (P, 2) and np.all(levels[:, 0] > levels[:, 1]) and np.all(levels[:, 1] > 0.0)

    mc.update(marginals_kde2d_covariance="diagonal", marginals_kde=False)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    lean = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(lean) == USUAL | {f"marginal_{k}" for k in mcmc.MARGINALS_KEYS + mcmc.MARGINALS_KDE2D_KEYS}, set(lean)
    assert np.all(lean["marginal_kde2d_shear"] == 0.0)

    mc.update(marginals=False)                                     # the 2-D densities go with the marginals
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    assert set(h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)) == USUAL
