"""-m gpu tests of the Matern kernel of general smoothness nu (csrc/matern_dev.h: kind 4; nu = inf: the RBF kind) against
the restatement (tests/matern_nu_ref.py) and the goldens the reference made (tests/golden/make_goldens_matern_nu.py):
fit-side kernel matrix / LML / gradient, predictions, log-posterior, whole fit, sampler chains."""
import numpy as np
import pytest

import golden_util as GU
import matern_nu_ref as R
from oracle import gp_oracle as O
from oracle import sampler_oracle as SO

pytestmark = pytest.mark.gpu

TOL = 1e-8
SINGLE = ["g8_matern_nu_0p75", "g8_matern_nu_2p0", "g8_matern_nu_3p5", "g8_matern_nu_inf"]
MAPPING3 = {"A": ("g1", slice(0, 10), slice(0, 10)), "B": ("g2", slice(10, 18), slice(0, 8)),
            "C": ("g3", slice(18, 30), slice(0, 12))}


def relerr(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _setup(name):
    g = GU.load(name)
    with R.general_nu():
        model = GU.group_model(g)
    dm = GU.device_model(model)
    return g, model, dm


@pytest.mark.parametrize("name", SINGLE)
def test_kernel_matrix_lml_and_gradient(name):
    from gpemu import fit as _fit
    g = GU.load(name)
    spec = GU.spec_of(g)
    X = g["design"]
    for i in range(int(g["n_pc"])):
        th = g["theta"][i]
        K = _fit.kernel_matrix(X, th, spec.kind, spec.nu, spec.has_const, spec.has_noise)
        Kr = R.kernel_matrix(X, th, spec)
        assert np.max(np.abs(K - Kr) / np.abs(Kr)) < 1e-12
    df = _fit.DeviceFit(X, spec.kind, spec.nu, spec.has_const, spec.has_noise, float(g["gpr_alpha"]))
    ytr = g["Y_pca_truncated"]
    for i in range(int(g["n_pc"])):
        for th in (g["theta"][i], g["theta2"][i]):
            val, grad = df.lml(ytr[:, i], th)
            ref = R.lml(X, ytr[:, i], th, spec)
            assert abs(val - ref) < 1e-10 * abs(ref)
            gc = R.lml_grad_central(X, ytr[:, i], th, spec)
            assert np.max(np.abs(grad - gc)) < 1e-6 * max(1.0, np.max(np.abs(gc))), (grad, gc)
        assert abs(df.lml(ytr[:, i], g["theta"][i], eval_gradient=False) - g["lml_at_theta"][i]) \
            < 1e-10 * abs(g["lml_at_theta"][i])
    # the batched evaluation: the same numbers
    n = int(g["n_pc"])
    lml_b, grad_b, info = df.lml_batch(ytr[:, :n].T.copy(), g["theta"][:n])
    assert np.all(info == 0)
    for i in range(n):
        v, gr = df.lml(ytr[:, i], g["theta"][i])
        assert lml_b[i] == v and np.array_equal(grad_b[i], gr)
    df.close()


@pytest.mark.parametrize("name", SINGLE)
def test_predict_vs_golden(name):
    g, model, dm = _setup(name)
    Xq = g["Xq"]                         # in the box, six training points, two rows far outside
    m, v = dm.gp_predict(Xq)
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(v))
    assert relerr(m, g["gp_mean"]) < TOL
    vscale = max(1.0, np.max(g["gp_var"]))
    assert np.max(np.abs(v - g["gp_var"])) < TOL * vscale
    cv, cov = dm.predict_full(Xq)
    assert np.all(np.isfinite(cv)) and np.all(np.isfinite(cov))
    assert relerr(cv, g["batch_central_value"]) < TOL
    nh = g["batch_cov_head"].shape[0]
    assert relerr(cov[:nh], g["batch_cov_head"]) < TOL
    for i in range(g["single_cov_head"].shape[0]):
        cv1, cov1 = dm.predict_full(Xq[i:i + 1])
        assert relerr(cv1[0], g["single_central_value"][i]) < TOL
        assert relerr(cov1[0], g["single_cov_head"][i]) < TOL
    dm.close()


@pytest.mark.parametrize("name", SINGLE)
def test_log_posterior_vs_golden(name):
    g, model, dm = _setup(name)
    dm.likelihood_setup(g["y_exp"], g["y_err"], g["lo"], g["hi"], 1.0)
    lp1 = np.array([dm.logpost(x[None, :])[0] for x in g["Xw"]])
    assert relerr(lp1, g["logpost_per_walker"]) < TOL
    n = g["Xw"].shape[0]
    dm.likelihood_setup(g["y_exp"], g["y_err"], g["lo"], g["hi"], float(n))     # the reference's /n_samples
    assert relerr(dm.logpost(g["Xw"]), g["logpost_batched"]) < TOL
    dm.close()


@pytest.mark.parametrize("name", SINGLE)
def test_whole_fit_certificate(name):
    """Per GP: the device's optimum, in the restatement's arithmetic, is no worse than the reference's, and L-BFGS-B with
    sklearn's settings (restated LML, sklearn's forward-difference gradient) started there stops within one iteration."""
    import scipy.optimize
    from gpemu import estimators as E
    g = GU.load(name)
    spec = GU.spec_of(g)
    X, lo, hi = g["design"], g["lo"], g["hi"]
    ytr = g["Y_pca_truncated"]
    ls = hi - lo
    kern = E.ARDKernel(E.MATERN_KIND, ls, np.outer(ls, (0.01, 100)), nu=spec.nu, constant_value=1.0,
                       constant_value_bounds=(1e-3, 1e3), noise_level=0.1, noise_level_bounds=(1e-3, 1e1))
    np.random.seed(2468)
    for i in range(int(g["n_pc"])):
        gp = E.GaussianProcessRegressor(kernel=kern, alpha=float(g["gpr_alpha"]),
                                        n_restarts_optimizer=int(g["n_restarts"])).fit(X, ytr[:, i])
        assert gp.kernel_.nu == spec.nu
        th = np.asarray(gp.kernel_.theta)
        mine = R.lml(X, ytr[:, i], th, spec)
        assert mine >= g["lml_value"][i] - 1e-8 * abs(g["lml_value"][i]), (i, mine, g["lml_value"][i])

        def neg(t, y=ytr[:, i]):
            return -R.lml(X, y, t, spec), -R.lml_grad_fd(X, y, t, spec)
        res = scipy.optimize.minimize(neg, th, method="L-BFGS-B", jac=True, bounds=gp.kernel_.bounds)
        assert res.nit <= 1, (i, res.nit, res.message)


def _oracle_lp(models, g, mapping=None):
    def lp(X):
        with R.general_nu():
            return np.array([O.log_posterior(x, models, g["lo"], g["hi"], g["y_exp"], g["y_err"], mapping)[0]
                             for x in np.atleast_2d(X)])
    return lp


@pytest.mark.parametrize("name", ["g8_matern_nu_2p0", "g8_matern_nu_inf"])
@pytest.mark.parametrize("W", [24, 200])
def test_sampler_chain_equals_oracle(name, W):
    from gpemu import synthetic
    from gpemu.sampler import DeviceSampler
    g, model, dm = _setup(name)
    dm.likelihood_setup(g["y_exp"], g["y_err"], g["lo"], g["hi"], 1.0)
    X0 = synthetic.make_walkers(W, seed=3, lo=g["lo"], hi=g["hi"])
    ds = DeviceSampler([dm], W, seed=0xABCDEF)
    ds.set_state(X0)
    steps = 6
    ds.run(steps)
    chain, lps = ds.get_chain()
    ochain, olps, onacc = SO.run(X0, _oracle_lp({"g": model}, g), SO.PhiloxStream(0xABCDEF), steps)
    np.testing.assert_allclose(chain, ochain, rtol=1e-12, atol=1e-12)
    fin = np.isfinite(olps)
    assert np.array_equal(fin, np.isfinite(lps))
    np.testing.assert_allclose(lps[fin], olps[fin], rtol=1e-8)
    np.testing.assert_array_equal(ds.counts()[0], onacc)
    ds.close()
    dm.close()


def _three_groups():
    g = GU.load("g8_matern_nu_3groups")
    with R.general_nu():
        models = {n: GU.group_model(g, prefix=n + "_") for n in ("g1", "g2", "g3")}
    dms = []
    for n in ("g1", "g2", "g3"):
        cols = g[f"cols_{n}"]
        dm = GU.device_model(models[n])
        dm.likelihood_setup(g["y_exp"][cols], g["y_err"][cols], g["lo"], g["hi"], 1.0)
        dms.append(dm)
    return g, models, dms


def test_three_groups_small_emulator_launch_equals_general_launches(monkeypatch):
    from gpemu import _lib, synthetic
    from gpemu.sampler import DeviceSampler
    L = _lib.lib()
    g, models, dms = _three_groups()
    W = 40
    X0 = synthetic.make_walkers(W, seed=5, lo=g["lo"], hi=g["hi"])
    monkeypatch.setenv("GPEMU_HALFSTEP_MIN_PAIRS", "0")
    out, launches = {}, {}
    for form in ("small", "general"):
        monkeypatch.delenv("GPEMU_NO_HALFSTEP", raising=False)
        if form == "general":
            monkeypatch.setenv("GPEMU_NO_HALFSTEP", "1")
        n0 = L.gpemu_halfstep_small_launches()
        ds = DeviceSampler(dms, W, seed=12)
        ds.set_state(X0)
        ds.run(6)
        out[form] = ds.get_chain() + (ds.counts()[0],)
        launches[form] = L.gpemu_halfstep_small_launches() - n0
        ds.close()
    monkeypatch.delenv("GPEMU_NO_HALFSTEP", raising=False)
    assert launches["small"] >= 12 and launches["general"] == 0, launches
    for a, b in zip(out["small"], out["general"]):
        np.testing.assert_array_equal(a, b)
    chain, lps = out["small"][0], out["small"][1]
    ref = _oracle_lp(models, g, MAPPING3)(chain[-1, :4])
    np.testing.assert_allclose(lps[-1, :4], ref, rtol=1e-8)
    # the reference's merged log-posterior at its walkers
    ds = DeviceSampler(dms, g["Xw"].shape[0], seed=1)
    ds.set_state(g["Xw"])
    np.testing.assert_allclose(ds.get_state()[1], g["logpost_per_walker"], rtol=1e-8)
    ds.close()
    for dm in dms:
        dm.close()


def test_fused_run_world1_equals_three_launch_run():
    """the fused front kernel (its general-nu instances) against the three-launch half-step, three groups at nu = 2"""
    import ctypes as C
    from gpemu import _lib, synthetic
    from gpemu.sampler import DeviceSampler
    L = _lib.lib()
    g, models, dms = _three_groups()
    for W in (24, 200):
        X0 = synthetic.make_walkers(W, seed=3, lo=g["lo"], hi=g["hi"])
        a = DeviceSampler(dms, W, seed=7)
        a.set_state(X0)
        a.run(5)
        b = DeviceSampler(dms, W, seed=7)
        b.set_state(X0)
        h = (C.c_char * 64)()
        _lib.check(L.gpemu_sampler_peer_export(b._h, C.cast(h, C.c_void_p)))
        _lib.check(L.gpemu_sampler_peer_import(b._h, 1, 0, C.cast(h, C.c_void_p)))
        _lib.check(L.gpemu_sampler_run_peer(b._h, 5, 1))
        np.testing.assert_array_equal(a.get_chain()[0], b.get_chain()[0])
        np.testing.assert_array_equal(a.get_chain()[1], b.get_chain()[1])
        np.testing.assert_array_equal(a.counts()[0], b.counts()[0])
        a.close()
        b.close()
    for dm in dms:
        dm.close()


def test_nu_2_never_runs_the_nu_2p5_kernel():
    """the dispatch trap: every kind is named, nu = 2.0 is not the closed form of 2.5"""
    from gpemu import fit as _fit
    g, model, dm = _setup("g8_matern_nu_2p0")
    X = g["design"]
    th = g["theta"][0]
    spec = GU.spec_of(g)
    K20 = _fit.kernel_matrix(X, th, 1, 2.0, spec.has_const, spec.has_noise)
    K25 = _fit.kernel_matrix(X, th, 1, 2.5, spec.has_const, spec.has_noise)
    off = ~np.eye(X.shape[0], dtype=bool)
    assert np.min(np.abs(K20 - K25)[off]) > 0.0
    assert np.max(np.abs(K20 - R.kernel_matrix(X, th, spec)) / np.abs(K20)) < 1e-12
    # the cross-kernel: predictions of the nu = 2.0 model are the restated nu = 2.0 ones, not the 2.5 ones
    Xq = g["Xq"][:24]
    m, _ = dm.gp_predict(Xq)
    with R.general_nu():
        mo, _ = O.gp_predict_all(Xq, model)
    spec25 = O.KernelSpec(O.MATERN, 2.5, spec.has_const, spec.has_noise)
    m25, _ = O.gp_predict_all(Xq, O.GroupModel(model.X_train, spec25, model.gps, model.components,
                                                model.explained_variance, model.scaler_mean, model.scaler_scale,
                                                model.n_pc))
    assert relerr(m, mo) < TOL and relerr(m, m25) > 1e-4
    dm.close()



@pytest.mark.parametrize("nu", [2.0, np.inf])
def test_dropin_config_with_general_nu_fits_predicts_and_samples(tmp_path, monkeypatch, nu):
    """The route a user takes: the analysis YAML (a copy of tests/fixtures/analysis.yaml) with the emulator's Matern
    ``nu`` set to 2.0 / .inf -> fit_emulators (device PCA, the batched multi-handle L-BFGS-B fit), the emulator's
    predict, predict_emulation_group and run_mcmc.  Predictions are the restatement's at the device's theta."""
    import pickle

    import yaml

    import dropin_util as DU
    from bayesian_inference import emulation, log_posterior, mcmc
    g = GU.load("g8_matern_nu_2p0")
    written = {}
    DU.install_fake_data_IO(g["Y"], g["design"], g["y_exp"], g["y_err"], written)
    path, analysis = DU.write_config(tmp_path, kernels_active=("matern", "noise"), n_pc=4, n_restarts=1)
    cfg = yaml.safe_load(open(path))
    cfg["test_analysis"]["parameters"]["emulators"]["main"]["kernels"]["matern"]["nu"] = float(nu)
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    assert ("nu: .inf" if np.isinf(nu) else "nu: 2.0") in open(path).read()
    analysis = cfg["test_analysis"]
    ec = emulation.EmulationConfig.from_config_file("test_analysis", "exponential", path, analysis)
    ec._sort_observables_in_matrix = None
    np.random.seed(3)
    emulation.fit_emulators(ec)
    gcfg = ec.emulation_groups_config["main"]
    res = emulation.read_emulators(gcfg)
    emus = res["emulators"]
    assert len(emus) == 4 and all(e.kernel_.nu == nu for e in emus)
    assert all(("nu=inf" if np.isinf(nu) else "nu=2") in repr(e.kernel_) for e in emus)
    assert pickle.loads(pickle.dumps(emus[0].kernel_)).nu == nu
    # every GP's optimum is one the restated LML agrees with: the device's LML at its theta is the restatement's
    spec = O.KernelSpec(O.MATERN, nu, False, True)
    ytr = res["PCA"]["Y_pca_truncated"]
    assert relerr(ytr, g["Y_pca_truncated"]) < 1e-9          # the same data as the golden: the reference's PCA
    for i, e in enumerate(emus):
        th = np.asarray(e.kernel_.theta)
        assert abs(R.lml(g["design"], ytr[:, i], th, spec) - e.log_marginal_likelihood_value_) \
            < 1e-8 * max(1.0, abs(e.log_marginal_likelihood_value_))
    # predictions at the device's theta, against the restatement (queries on training points and far outside included)
    Xq = g["Xq"]
    with R.general_nu():
        om = DU.oracle_group_at(emus, g["design"], ytr, g["pca_components"], g["pca_explained_variance"],
                                g["scaler_mean"], g["scaler_scale"], float(g["gpr_alpha"]))
        mo, vo = O.gp_predict_all(Xq, om)
        po = O.predict_group(Xq, om)
    for i, e in enumerate(emus):
        m, sd = e.predict(Xq, return_std=True)
        assert np.all(np.isfinite(m)) and np.all(np.isfinite(sd))
        assert relerr(m, mo[:, i]) < 1e-6
        assert np.max(np.abs(sd ** 2 - vo[:, i])) < 1e-6 * max(1.0, np.max(vo[:, i]))
    p = emulation.predict_emulation_group(Xq, res, gcfg)
    assert relerr(p["central_value"], po["central_value"]) < 1e-6
    assert relerr(p["cov"], po["cov"]) < 1e-6
    # the sampler on the fitted emulators
    monkeypatch.setattr(emulation.EmulationConfig, "sort_observables_in_matrix",
                        property(lambda self: DU.TrivialSort("main")))
    monkeypatch.setattr(emulation.EmulationConfig, "observable_filter", property(lambda self: None))
    mc = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    mcmc.run_mcmc(mc)
    out = written[mc.mcmc_outputfile]
    assert out["chain"].shape == (mc.n_sampling_steps, mc.n_walkers, 6)
    lo, hi = np.array(g["lo"]), np.array(g["hi"])
    assert np.all(out["chain"] > lo) and np.all(out["chain"] < hi) and np.all(np.isfinite(out["log_prob"]))
    assert np.any(out["acceptance_fraction"] > 0)
    lp = np.array([log_posterior.log_posterior(x)[0] for x in out["chain"][-1][:5]])
    np.testing.assert_allclose(lp, out["log_prob"][-1][:5], rtol=1e-10)
    with R.general_nu():
        ref = np.array([O.log_posterior(x, {"main": om}, lo, hi, g["y_exp"], g["y_err"])[0]
                        for x in out["chain"][-1][:5]])
    np.testing.assert_allclose(out["log_prob"][-1][:5], ref, rtol=1e-6)
