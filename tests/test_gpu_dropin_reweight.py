"""-m gpu tests of the reweighting of a sampler's stored chain and of the drop-in's ``parameters.mcmc.reweight`` key
(DeviceSampler.reweight, TemperedSampler.reweight, bayesian_inference/mcmc.py): the in-place forms equal
``gpemu.reweight.summary`` of the downloaded chain through the host entries, the data scenario equals the same composition
of ``gpemu.loo.pointwise`` outputs in numpy, and with the key mcmc.h5 gains the documented ``reweight_*`` entries."""
import numpy as np
import pytest

import dropin_util as DU
import golden_util as GU
import reweight_ref as RR

pytestmark = pytest.mark.gpu

USUAL = {"chain", "acceptance_fraction", "log_prob", "autocorrelation_time"}
NAMES = ["alpha_s", "Q_0", "c_1", "c_2", "tau_0", "c_3"]          # the synthetic problem's box is the reference's
EXACT = ("pareto_k", "ess_w", "log_mean_ratio", "log_evidence_ratio", "Q", "quantiles", "hist_1d_q", "hist_2d_q", "hist_1d",
         "hist_2d", "mean", "sd")


def _same(got, want, whole):
    """quantiles, integer histograms and weighted moments bit for bit; the shift's baseline is the sampler's pooled chain
    moments in place and the same reduction under uniform weights from the host rows -- two fixed trees"""
    assert len(got) == len(want)
    for a, b in zip(got, want):
        for k in EXACT:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
        assert a["reliable"] == b["reliable"] and a["k_threshold"] == b["k_threshold"]
        assert np.allclose(a["shift"], b["shift"], rtol=0, atol=1e-10)
        if not whole:
            assert np.asarray(a["shift"]).tobytes() == np.asarray(b["shift"]).tobytes()


@pytest.fixture(scope="module")
def problem():
    model, prob, _ = GU.fixed_theta_model(200, 100, 5, seed=0)
    dm = GU.device_model(model)
    lo, hi = np.asarray(prob["lo"], dtype=np.float64), np.asarray(prob["hi"], dtype=np.float64)
    dm.likelihood_setup(prob["y_exp"], prob["y_err"], lo, hi, 1.0)
    yield dict(model=model, prob=prob, dm=dm, lo=lo, hi=hi)
    dm.close()


def test_sampler_reweight_equals_the_summary_of_the_downloaded_chain(problem):
    from gpemu import reweight as R
    from gpemu.sampler import DeviceSampler, TemperedSampler
    dm, lo, hi, prob = problem["dm"], problem["lo"], problem["hi"], problem["prob"]
    d, W, steps = lo.size, 64, 200
    rng = np.random.default_rng(3)
    spec = [R.reference_prior(NAMES), {0: ("normal", 0.3, 0.1), 5: ("log_normal", 2.0, 1.5)}]
    assert spec[0] == [0, 0, 1, 1, 0, 1]
    s = DeviceSampler([dm], W, seed=4)
    s.set_state(rng.uniform(lo, hi, (W, d)))
    s.run(steps)
    chain, _ = s.get_chain()
    kw = dict(bins_1d=40, bins_2d=12)
    c0 = R.path_counts()
    got = s.reweight(priors=spec, discard=50, **kw)                     # the prior box by default, the chain in place
    c1 = R.path_counts()
    assert c1["LOGPRIOR"] - c0["LOGPRIOR"] == 1 and c1["WHIST_SWEEP"] - c0["WHIST_SWEEP"] == 1
    rows = np.ascontiguousarray(chain[50:].reshape(-1, d))
    want = R.chain_reweight([dm], rows, priors=spec, **kw)              # through the host entries
    _same(got, want, whole=True)
    for r, res in enumerate(got):
        print(f"scenario {r}: pareto_k {res['pareto_k']:.3f} (threshold {res['k_threshold']:.2f}), ess_w {res['ess_w']:.0f} of "
              f"{rows.shape[0]}, largest |shift| {np.abs(res['shift']).max():.3f}, log_evidence_ratio {res['log_evidence_ratio']:.4f}")
        assert res["quantiles"].shape == (3, d) and res["hist_1d_q"].shape == (d, 40) and res["hist_2d_q"].shape == (15, 12, 12)
        assert np.isfinite(res["log_evidence_ratio"]) and 0 < res["ess_w"] <= rows.shape[0]
    # ... and the host summary equals the reference from the weights the device produced
    st = R.weights(R.log_ratio(rows, priors=spec, lower=lo, upper=hi))
    q, Q = R.fixed_weights(st["log_weights"])
    for r, res in enumerate(got):
        for j in range(d):
            assert np.array_equal(res["quantiles"][:, j], RR.weighted_quantile(rows[:, j], q[r], (0.05, 0.5, 0.95)))
        h1, h2, _ = RR.hist_ref(rows, q[r], res["edges_1d"], res["edges_2d"])
        assert np.array_equal(res["hist_1d_q"], h1) and np.array_equal(res["hist_2d_q"], h2) and res["Q"] == int(Q[r])
    # thinned: a dense copy serves the quantiles, everything else reads the view as it lies
    got = s.reweight(priors=spec, discard=41, thin=3, lower=lo, upper=hi, probabilities=(0.16, 0.84), **kw)
    rows3 = np.ascontiguousarray(chain[41::3].reshape(-1, d))
    _same(got, R.chain_reweight([dm], rows3, priors=spec, probabilities=(0.16, 0.84), **kw), whole=False)
    with pytest.raises(ValueError):
        s.reweight()
    with pytest.raises(ValueError):
        s.reweight(priors=[[1] * d])                                    # tau_0's lower bound is 0
    s.close()

    # chain 1 of a stacked sampler
    dm.likelihood_setup(np.stack([prob["y_exp"], prob["y_exp"] * 1.01]), prob["y_err"], lo, hi, 1.0)
    s2 = DeviceSampler([dm], W, seeds=[3, 4])
    s2.set_state(rng.uniform(lo, hi, (2 * W, d)))
    s2.run(60)
    chain2, _ = s2.get_chain()
    with pytest.raises(ValueError):
        s2.reweight(priors=spec)
    got = s2.reweight(priors=spec, chain=1, discard=10, **kw)
    rows2 = np.ascontiguousarray(chain2[10:, W:2 * W]).reshape(-1, d)
    _same(got, R.chain_reweight([dm], rows2, priors=spec, **kw), whole=False)
    s2.close()

    # rung 0 of a tempered sampler
    dm.likelihood_setup(prob["y_exp"], prob["y_err"], lo, hi, 1.0)
    ts = TemperedSampler([dm], W, [1.0, 0.5, 0.1], seed=5, swap_every=2)
    ts.set_state(rng.uniform(lo, hi, (3 * W, d)))
    ts.run(60)
    got = ts.reweight(priors=spec, discard=10, **kw)
    rows_t = np.ascontiguousarray(ts.get_chain(temp=0, discard=10)[0].reshape(-1, d))
    _same(got, R.chain_reweight([dm], rows_t, priors=spec, **kw), whole=False)
    ts.close()


def test_data_scenario_equals_the_composition_in_numpy(problem):
    from gpemu import loo
    from gpemu import reweight as R
    from gpemu.sampler import DeviceSampler
    dm, lo, hi, prob, model = problem["dm"], problem["lo"], problem["hi"], problem["prob"], problem["model"]
    d, W = lo.size, 64
    bs = np.array([0, 30, 100], dtype=np.int64)                         # two observables
    dm.likelihood_setup(prob["y_exp"], prob["y_err"], lo, hi, 1.0, block_start=bs)
    new = GU.device_model(model)
    new.likelihood_setup(prob["y_exp"], 2.0 * prob["y_err"], lo, hi, 1.0, block_start=bs)      # y_err doubled
    s = DeviceSampler([dm], W, seed=9)
    s.set_state(np.random.default_rng(10).uniform(lo, hi, (W, d)))
    s.run(200)
    rows = np.ascontiguousarray(s.get_chain()[0][50:].reshape(-1, d))
    S = rows.shape[0]
    # the log-ratio: both lists' terms, each summed in row order, then subtracted once
    T_new, T_old = loo.pointwise([new], rows), loo.pointwise([dm], rows)
    want = (T_new[0] + T_new[1]) - (T_old[0] + T_old[1])
    L = R.log_ratio(rows, models_old=[dm], models_new=[new])
    assert L.shape == (1, S) and L[0].tobytes() == want.tobytes()
    got = s.reweight(models_new=[new], discard=50, bins_1d=40, bins_2d=12)
    ref = R.chain_reweight([dm], rows, models_new=[new], bins_1d=40, bins_2d=12)
    _same(got, ref, whole=True)
    res = got[0]
    assert res["log_evidence_ratio"] is None and np.isfinite(res["pareto_k"]) and res["ess_w"] < S
    # the same comparison from the same weights in the reference: what holds there is asserted here, not a physics claim
    st = R.weights(L)
    q, Q = R.fixed_weights(st["log_weights"])
    mean, var = RR.moments(rows, q[0])
    assert np.allclose(res["mean"], mean, rtol=1e-9) and np.allclose(res["sd"], np.sqrt(var), rtol=1e-7)
    sd0 = rows.std(axis=0)
    mc_err = sd0 / np.sqrt(2.0 * res["ess_w"])                          # the Monte Carlo error of a standard deviation
    wider_ref = np.sqrt(var) >= sd0 - mc_err
    print(f"y_err doubled: pareto_k {res['pareto_k']:.3f}, ess_w {res['ess_w']:.0f} of {S}, sd ratio {res['sd'] / sd0}, "
          f"wider within the Monte Carlo error (reference): {wider_ref}")
    assert np.array_equal(res["sd"] >= sd0 - mc_err, wider_ref)
    # both: every prior scenario plus the data scenario
    both = s.reweight(priors=[R.reference_prior(NAMES)], models_new=[new], discard=50, bins_1d=10, bins_2d=4)
    Lp = R.log_ratio(rows, priors=[R.reference_prior(NAMES)], lower=lo, upper=hi)
    assert both[0]["log_mean_ratio"] == R.weights(Lp + L)["log_mean_ratio"][0] and both[0]["log_evidence_ratio"] is None
    s.close()
    new.close()
    dm.likelihood_setup(prob["y_exp"], prob["y_err"], lo, hi, 1.0)


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


def _labels(v):
    return [x.decode() if isinstance(x, bytes) else str(x) for x in np.atleast_1d(np.asarray(v)).tolist()]


def test_dropin_reweight_key(tmp_path, monkeypatch):
    from bayesian_inference import mcmc
    path, analysis, h5io = _analysis(tmp_path, monkeypatch)
    mc = analysis["parameters"]["mcmc"]
    mc.update(n_burn_steps=20, n_sampling_steps=40)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.reweight is None
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    plain = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(plain) == USUAL, set(plain)                       # without the key: what the file held before

    names = analysis["parameterization"]["exponential"]["names"]
    scen = [{"name": "prior_run", "priors": {names[0]: {"kind": "normal", "a": 0.3, "b": 0.1},
                                             names[5]: {"kind": "log_normal", "a": 2.0, "b": 1.5}}},
            {"name": "logc", "priors": {names[2]: {"kind": "log_uniform"}}}]
    for key, labels in (({"reference_prior": True}, ["reference_prior"]), (scen, ["prior_run", "logc"])):
        mc.update(reweight=key)
        cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
        assert [n for n, _ in cfg.reweight] == labels
        np.random.seed(3)
        mcmc.run_mcmc(cfg)
        back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
        want = {"reweight_names"} | {f"reweight_{k}" for k in mcmc.REWEIGHT_SHARED_KEYS} | \
            {f"reweight_{n}_{k}" for n in labels for k in mcmc.REWEIGHT_KEYS}
        assert set(back) == USUAL | want, set(back) ^ (USUAL | want)
        assert np.array_equal(back["chain"], plain["chain"])     # the run itself is untouched
        assert _labels(back["reweight_names"]) == labels
        d = back["chain"].shape[2]
        npair = d * (d - 1) // 2
        assert back["reweight_edges_1d"].shape == (d, 101) and back["reweight_edges_2d"].shape == (d, 51)
        assert back["reweight_pairs"].shape == (npair, 2) and back["reweight_probabilities"].tolist() == [0.05, 0.5, 0.95]
        again = mcmc.reweight(cfg)                               # from the file, through the host entries
        assert set(again) == want
        for n in labels:
            p = f"reweight_{n}_"
            assert back[p + "quantiles"].shape == (3, d) and back[p + "mean"].shape == (d,) and back[p + "shift"].shape == (d,)
            assert back[p + "hist_1d"].shape == (d, 100) and back[p + "hist_2d"].shape == (npair, 50, 50)
            assert back[p + "hist_1d_q"].dtype == np.uint64 and back[p + "hist_2d_q"].dtype == np.uint64
            assert int(back[p + "hist_1d_q"][0].sum()) <= int(back[p + "Q"]) and np.isfinite(back[p + "pareto_k"])
            assert np.isfinite(back[p + "log_evidence_ratio"])
            for k in mcmc.REWEIGHT_KEYS:
                if k != "shift":
                    assert np.asarray(back[p + k]).tobytes() == np.asarray(again[p + k]).tobytes(), k
            assert np.allclose(back[p + "shift"], again[p + "shift"], rtol=0, atol=1e-10)
    # the same scenarios on request, without the key
    mc.pop("reweight")
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    on_request = mcmc.reweight(cfg, priors=scen, bins_1d=20, bins_2d=5)
    assert on_request["reweight_logc_hist_1d_q"].shape == (6, 20) and _labels(on_request["reweight_names"]) == ["prior_run", "logc"]
    ref_only = mcmc.reweight(cfg, reference_prior=True)
    assert _labels(ref_only["reweight_names"]) == ["reference_prior"]
    # a parameter that does not exist, or a log prior on tau_0 (lower bound 0): a warning and a file without the entries
    for bad in ([{"name": "x", "priors": {"no such parameter": {"kind": "log_uniform"}}}],
                [{"name": "x", "priors": {names[4]: {"kind": "log_uniform"}}}]):
        mc.update(reweight=bad)
        cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
        np.random.seed(3)
        mcmc.run_mcmc(cfg)
        assert set(h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)) == USUAL
