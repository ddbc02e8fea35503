"""-m gpu tests of 9 to 16 parameters against the goldens the reference made (tests/golden/make_goldens_wide_d.py):
kernel matrix, LML and gradient at the reference's theta, predictions, full predictions and the log-posterior (both
modes, batches on both cross-kernel forms), three emulation groups at d = 9 (the several-group launches), cross-
validation at d = 10, a two-rank sharded run on one card, and the drop-in modules end to end with a 10-name
parameterization (whole-fit certificate, fit_emulators, run_mcmc)."""
import os

import numpy as np
import pytest
import yaml

import cv_ref as CV
import dropin_util as DU
import golden_util as GU
import matern_nu_ref as R
from oracle import gp_oracle as O
from oracle import sampler_oracle as SO

pytestmark = pytest.mark.gpu

TOL = 1e-8
SINGLE = ["g10_wide_d_rbf_const_noise_d10", "g10_wide_d_matern25_d16", "g10_wide_d_nu0p75_d12"]
MAPPING3 = {"A": ("g1", slice(0, 10), slice(0, 10)), "B": ("g2", slice(10, 18), slice(0, 8)),
            "C": ("g3", slice(18, 30), slice(0, 12))}


def relerr(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _setup(name):
    g = GU.load(name)
    with R.general_nu():
        model = GU.group_model(g)
    return g, model, GU.device_model(model)


@pytest.mark.parametrize("name", SINGLE)
def test_fit_at_reference_theta(name):
    from gpemu import fit as _fit
    g = GU.load(name)
    spec = GU.spec_of(g)
    X = g["design"]
    K = _fit.kernel_matrix(X, g["theta"][0], spec.kind, spec.nu, spec.has_const, spec.has_noise)
    assert relerr(K, g["kernel_matrix_pc0"]) < 1e-12
    df = _fit.DeviceFit(X, spec.kind, spec.nu, spec.has_const, spec.has_noise, float(g["gpr_alpha"]))
    ytr = g["Y_pca_truncated"]
    for i in range(int(g["n_pc"])):
        for th, lml, grad in ((g["theta"][i], g["lml_at_theta"][i], g["grad_at_theta"][i]),
                              (g["theta2"][i], g["lml_at_theta2"][i], g["grad_at_theta2"][i])):
            val, gr = df.lml(ytr[:, i], th)
            assert abs(val - lml) < 1e-9 * abs(lml)
            if spec.nu in (0.5, 1.5, 2.5, np.inf):
                assert np.max(np.abs(gr - grad)) < 1e-8 * max(1.0, np.max(np.abs(grad))), (gr, grad)
            else:
                # sklearn's general-nu gradient is a forward difference with step 1e-10 (kernels.py:1767-1774): ~1e-3
                # off; the device's analytic one is held to central differences of the restated LML, as
                # test_gpu_matern_nu.py does
                gc = R.lml_grad_central(X, ytr[:, i], th, spec)
                assert np.max(np.abs(gr - gc)) < 1e-6 * max(1.0, np.max(np.abs(gc))), (gr, gc)
    df.close()


@pytest.mark.parametrize("name", SINGLE)
def test_predict_and_logpost_vs_golden(name):
    g, model, dm = _setup(name)
    Xq = g["Xq"]                       # in the box, six training points, two rows far outside the design
    big = np.concatenate([Xq] * 10)    # 320 rows: the > 256-column cross-kernel
    for Q, reps in ((Xq, 1), (big, 10)):
        m, v = dm.gp_predict(Q)
        assert relerr(m, np.tile(g["gp_mean"], (reps, 1))) < TOL
        assert np.max(np.abs(v - np.tile(g["gp_var"], (reps, 1)))) < TOL * max(1.0, np.max(g["gp_var"]))
        with R.general_nu():
            mo, vo = O.gp_predict_all(Q, model)
        assert relerr(m, mo) < TOL and np.max(np.abs(v - vo)) < TOL * max(1.0, np.max(vo))
    cv, cov = dm.predict_full(Xq)
    assert relerr(cv, g["batch_central_value"]) < TOL
    nh = g["batch_cov_head"].shape[0]
    assert relerr(cov[:nh], g["batch_cov_head"]) < TOL
    for i in range(g["single_cov_head"].shape[0]):
        cv1, cov1 = dm.predict_full(Xq[i:i + 1])
        assert relerr(cv1[0], g["single_central_value"][i]) < TOL
        assert relerr(cov1[0], g["single_cov_head"][i]) < TOL
    for mode in (0, 1):
        dm.likelihood_setup(g["y_exp"], g["y_err"], g["lo"], g["hi"], 1.0)
        lp1 = np.array([dm.logpost(x[None, :], mode=mode)[0] for x in g["Xw"]])
        assert relerr(lp1, g["logpost_per_walker"]) < TOL
        n = g["Xw"].shape[0]
        dm.likelihood_setup(g["y_exp"], g["y_err"], g["lo"], g["hi"], float(n))     # the reference's /n_samples
        assert relerr(dm.logpost(g["Xw"], mode=mode), g["logpost_batched"]) < TOL
        inside = np.all((g["X_mixed"] > g["lo"]) & (g["X_mixed"] < g["hi"]), axis=1)
        dm.likelihood_setup(g["y_exp"], g["y_err"], g["lo"], g["hi"], float(inside.sum()))
        lpm = dm.logpost(g["X_mixed"], mode=mode)
        assert np.array_equal(np.isneginf(lpm), np.isneginf(g["logpost_mixed"]))
        fin = np.isfinite(g["logpost_mixed"])
        assert relerr(lpm[fin], g["logpost_mixed"][fin]) < TOL
        # a batch of > 256 rows, rows outside the box included
        rows = np.concatenate([g["Xw"]] * 12 + [g["X_mixed"]])
        dm.likelihood_setup(g["y_exp"], g["y_err"], g["lo"], g["hi"], 1.0)
        lpb = dm.logpost(rows, mode=mode)
        assert relerr(lpb[:n], g["logpost_per_walker"]) < TOL and relerr(lpb[n:2 * n], g["logpost_per_walker"]) < TOL
        assert np.array_equal(np.isneginf(lpb[-8:]), ~inside)
    dm.close()


def _three_groups():
    g = GU.load("g10_wide_d_3groups_d9")
    models = {n: GU.group_model(g, prefix=n + "_") for n in ("g1", "g2", "g3")}
    dms = []
    for n in ("g1", "g2", "g3"):
        cols = g[f"cols_{n}"]
        dm = GU.device_model(models[n])
        dm.likelihood_setup(g["y_exp"][cols], g["y_err"][cols], g["lo"], g["hi"], 1.0)
        dms.append(dm)
    return g, models, dms


def test_three_groups_d9():
    """Three groups: the several-group cross-kernel and likelihood launches at the wide padding, against the reference's
    merged log-posterior and the oracle's chain."""
    from gpemu.sampler import DeviceSampler
    g, models, dms = _three_groups()
    for dm, n in zip(dms, ("g1", "g2", "g3")):
        m, v = dm.gp_predict(g["Xq"])
        mo, vo = O.gp_predict_all(g["Xq"], models[n])
        assert relerr(m, mo) < TOL and np.max(np.abs(v - vo)) < TOL
    W = 24
    ds = DeviceSampler(dms, W, seed=7)
    ds.set_state(g["Xw"])
    _, lp0 = ds.get_state()
    assert relerr(lp0, g["logpost_per_walker"]) < TOL

    def oracle_lp(X):
        return np.array([O.log_posterior(x, models, g["lo"], g["hi"], g["y_exp"], g["y_err"], MAPPING3)[0]
                         for x in np.atleast_2d(X)])
    ds.run(5)
    chain, lps = ds.get_chain()
    ochain, olps, _ = SO.run(g["Xw"], oracle_lp, SO.PhiloxStream(7), 5)
    np.testing.assert_allclose(chain, ochain, rtol=1e-12, atol=1e-12)
    fin = np.isfinite(olps)
    assert np.array_equal(fin, np.isfinite(lps))
    np.testing.assert_allclose(lps[fin], olps[fin], rtol=TOL)
    ds.close()
    for dm in dms:
        dm.close()


def test_cross_validation_d10():
    from bayesian_inference import emulation
    g, model, dm = _setup("g10_wide_d_rbf_const_noise_d10")
    y = g["Y_pca_truncated"]
    N = y.shape[0]
    for fold in (emulation.kfold_labels(N, 5), np.arange(N)):
        m, v, cv, var = dm.cross_validate(y, fold)
        bm, bv = CV.brute_force_group(model, y, fold, float(g["gpr_alpha"]))
        assert np.max(np.abs(m - bm)) <= 1e-9 * np.max(np.abs(y))
        assert np.all(np.abs(v - bv) <= 1e-9 * np.abs(bv) + 1e-14)
        rcv, rvar = CV.back_project(model, bm, bv, O.cov_unexplained(model))
        assert np.max(np.abs(cv - rcv)) <= 1e-9 * np.max(np.abs(rcv))
        assert np.all(np.abs(var - rvar) <= 1e-9 * np.abs(rvar) + 1e-14)
    dm.close()


# ---- two ranks on the one GPU: the fused front kernel has no wide instance, so the run falls back -------------------
def _sharded_worker(rank, world, port, out_dir, W=26):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gpemu.sampler import DeviceSampler
    g = GU.load("g10_wide_d_rbf_const_noise_d10")
    dm = GU.device_model(GU.group_model(g))
    dm.likelihood_setup(g["y_exp"], g["y_err"], g["lo"], g["hi"], 1.0)
    ds = DeviceSampler([dm], W, seed=99)
    ds.set_state(np.random.default_rng(3).uniform(g["lo"], g["hi"], (W, 10)))
    for n_steps in (2, 1, 3):
        ds.run_sharded(n_steps, transport="peer")
    np.save(os.path.join(out_dir, f"transport_{rank}.npy"),
            np.array([ds.last_transport == "torch", bool(ds.transport_info.get("fallback_from_peer"))]))
    chain, lps = ds.get_chain()
    np.save(os.path.join(out_dir, f"chain_{rank}.npy"), chain)
    np.save(os.path.join(out_dir, f"lp_{rank}.npy"), lps)
    dist.barrier()
    dist.destroy_process_group()
    ds.close()
    dm.close()


def test_sharded_two_ranks_equals_single_d10(tmp_path):
    import torch.multiprocessing as mp
    from gpemu.sampler import DeviceSampler
    port = 29400 + (os.getpid() % 2000)
    mp.spawn(_sharded_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for r in (0, 1):      # the peer transport was requested, declined before any launch, and the collective one ran
        assert np.load(tmp_path / f"transport_{r}.npy").all()
    c0 = np.load(tmp_path / "chain_0.npy")
    np.testing.assert_array_equal(c0, np.load(tmp_path / "chain_1.npy"))
    g = GU.load("g10_wide_d_rbf_const_noise_d10")
    dm = GU.device_model(GU.group_model(g))
    dm.likelihood_setup(g["y_exp"], g["y_err"], g["lo"], g["hi"], 1.0)
    W = 26
    ds = DeviceSampler([dm], W, seed=99)
    ds.set_state(np.random.default_rng(3).uniform(g["lo"], g["hi"], (W, 10)))
    ds.run(6)
    chain, lps = ds.get_chain()
    np.testing.assert_array_equal(chain, c0)
    np.testing.assert_array_equal(lps, np.load(tmp_path / "lp_0.npy"))
    ds.close()
    dm.close()


# ---- drop-in modules, 10 parameters -----------------------------------------------------------------------------
def _write_config(tmp_path, g, n_restarts, n_pc=4):
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "analysis.yaml")))
    cfg["output_dir"] = str(tmp_path / "out")
    an = cfg["test_analysis"]
    an["parameterization"]["exponential"] = {"names": [f"$p_{{{i}}}$" for i in range(10)],
                                             "min": [float(v) for v in g["lo"]], "max": [float(v) for v in g["hi"]]}
    em = an["parameters"]["emulators"]["main"]
    em["kernels"]["active"] = ["rbf", "constant", "noise"]
    em["kernels"]["constant"] = {"constant_value": 1.0, "constant_value_bounds": [1e-3, 1e3]}
    em["n_pc"] = n_pc
    em["GPR"]["n_restarts"] = n_restarts
    an["parameters"]["mcmc"].update(n_walkers=24, n_burn_steps=50, n_sampling_steps=250)
    path = tmp_path / "analysis.yaml"
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return str(path), an


def test_dropin_fit_and_mcmc_d10(tmp_path, monkeypatch):
    from bayesian_inference import emulation, mcmc
    g = GU.load("g10_wide_d_rbf_const_noise_d10")
    written = {}
    DU.install_fake_data_IO(g["Y"], g["design"], g["y_exp"], g["y_err"], written)
    path, analysis = _write_config(tmp_path, g, n_restarts=int(g["n_restarts"]))
    ec = emulation.EmulationConfig.from_config_file("test_analysis", "exponential", path, analysis)
    ec._sort_observables_in_matrix = None
    np.random.seed(2468)       # the golden's restart seed
    emulation.fit_emulators(ec)
    res = emulation.read_emulators(ec.emulation_groups_config["main"])
    assert relerr(res["PCA"]["Y_pca_truncated"], g["Y_pca_truncated"]) < 1e-9
    DU.certify_fit_against_reference(res["emulators"], g["theta"], g["lml_value"], "d=10 fit", g["design"],
                                     g["Y_pca_truncated"], float(g["gpr_alpha"]))
    monkeypatch.setattr(emulation.EmulationConfig, "sort_observables_in_matrix",
                        property(lambda self: DU.TrivialSort("main")))
    monkeypatch.setattr(emulation.EmulationConfig, "observable_filter", property(lambda self: None))
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    mcmc.run_mcmc(cfg)
    out = written[cfg.mcmc_outputfile]
    assert out["chain"].shape == (250, 24, 10) and out["log_prob"].shape == (250, 24)
    assert np.all(out["chain"] > g["lo"]) and np.all(out["chain"] < g["hi"]) and np.all(np.isfinite(out["log_prob"]))
    from bayesian_inference import log_posterior
    lp = np.array([log_posterior.log_posterior(x)[0] for x in out["chain"][-1][:5]])
    np.testing.assert_allclose(lp, out["log_prob"][-1][:5], rtol=1e-10)
    from gpemu import h5io
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert back["chain"].shape == (250, 24, 10)
    np.testing.assert_array_equal(back["chain"], out["chain"])
