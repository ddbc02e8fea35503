"""-m gpu tests of the weighted summaries of a sampler's stored chain and of the drop-in's
``parameters.mcmc.reweight_summaries`` key (DeviceSampler.reweight(hpd=, kde=, posterior_predictive=),
bayesian_inference/mcmc.py): the in-place forms equal the host entries on the downloaded chain, and with
the key mcmc.h5 gains the documented entries -- those of ``DeviceSampler.reweight`` on the chain where it lies, and of
``mcmc.reweight`` recomputed from the file."""
import numpy as np
import pytest

import golden_util as GU
import wsummary_ref as WR
from test_gpu_dropin_reweight import NAMES, USUAL, _analysis, _labels

pytestmark = pytest.mark.gpu

CONF = [0.68, 0.9]
PP = ("mean", "variance_parameters", "variance_emulator", "variance", "quantiles", "probabilities", "total_weight")
NEW = ("hpd_confidence", "hpd", "kde_grid", "kde_density", "kde_bandwidth")


def _same_new(a, b, n_models=0):
    for k in NEW:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    if n_models:
        assert len(a["posterior_predictive"]) == len(b["posterior_predictive"]) == n_models
        for pa, pb in zip(a["posterior_predictive"], b["posterior_predictive"]):
            assert set(pa) == set(pb) == set(PP)
            for k in PP:
                assert np.asarray(pa[k]).tobytes() == np.asarray(pb[k]).tobytes(), k


def test_sampler_reweight_options_equal_the_host_entries_on_the_downloaded_chain():
    from gpemu import reweight as R
    from gpemu.sampler import DeviceSampler, TemperedSampler
    model, prob, _ = GU.fixed_theta_model(200, 100, 5, seed=0)
    dm = GU.device_model(model)
    lo, hi = np.asarray(prob["lo"], dtype=np.float64), np.asarray(prob["hi"], dtype=np.float64)
    dm.likelihood_setup(prob["y_exp"], prob["y_err"], lo, hi, 1.0)
    d, W, steps = lo.size, 64, 120
    rng = np.random.default_rng(3)
    spec = [R.reference_prior(NAMES), {0: ("normal", 0.3, 0.1)}]
    kw = dict(bins_1d=20, bins_2d=6, hpd=CONF, kde=True, n_grid=65)
    s = DeviceSampler([dm], W, seed=4)
    try:
        s.set_state(rng.uniform(lo, hi, (W, d)))
        s.run(steps)
        chain, _ = s.get_chain()
        plain = s.reweight(priors=spec, discard=40, bins_1d=20, bins_2d=6)
        c0 = R.wsummary_path_counts()
        got = s.reweight(priors=spec, discard=40, posterior_predictive=True, **kw)
        c1 = R.wsummary_path_counts()
        assert all(c1[k] > c0[k] for k in ("BANDS_WHOLE", "ROW_REDUCE", "HPD_PLACE", "HPD_WINDOW", "KDE"))
        rows = np.ascontiguousarray(chain[40:].reshape(-1, d))
        want = R.chain_reweight([dm], rows, priors=spec, posterior_predictive=True, **kw)
        for a, b, p in zip(got, want, plain):
            assert set(a) == set(b) == set(p) | set(NEW) | {"posterior_predictive"}       # the default keys are today's
            _same_new(a, b, n_models=1)
            assert a["hpd"].shape == (2, d, 2) and a["kde_density"].shape == (d, 65) and a["kde_bandwidth"].shape == (d,)
            assert a["posterior_predictive"][0]["quantiles"].shape == (3, dm.F)
            for k in ("quantiles", "hist_1d_q", "mean"):
                assert np.asarray(a[k]).tobytes() == np.asarray(p[k]).tobytes(), k
        # ... and the intervals are the definition's, from the weights the device produced
        st = R.weights(R.log_ratio(rows, priors=spec, lower=lo, upper=hi))
        q, Q = R.fixed_weights(st["log_weights"])
        tg = R.targets(CONF, Q)
        for r, res in enumerate(got):
            for j in range(d):
                for l in range(2):
                    assert tuple(res["hpd"][l, j]) == WR.hpd(rows[:, j], q[r], int(tg[r, l]))
        # thinned: a dense copy serves the sort and the density, the bands read the view as it lies
        got = s.reweight(priors=spec, discard=41, thin=3, posterior_predictive=True, **kw)
        rows3 = np.ascontiguousarray(chain[41::3].reshape(-1, d))
        for a, b in zip(got, R.chain_reweight([dm], rows3, priors=spec, posterior_predictive=True, **kw)):
            _same_new(a, b, n_models=1)
    finally:
        s.close()
    ts = TemperedSampler([dm], W, [1.0, 0.5], seed=5, swap_every=2)
    try:
        ts.set_state(rng.uniform(lo, hi, (2 * W, d)))
        ts.run(40)
        got = ts.reweight(priors=spec, discard=10, posterior_predictive=True, **kw)
        rows_t = np.ascontiguousarray(ts.get_chain(temp=0, discard=10)[0].reshape(-1, d))
        for a, b in zip(got, R.chain_reweight([dm], rows_t, priors=spec, posterior_predictive=True, **kw)):
            _same_new(a, b, n_models=1)
    finally:
        ts.close()
        dm.close()


def test_dropin_reweight_summaries_key(tmp_path, monkeypatch):
    from bayesian_inference import mcmc
    from gpemu import reweight as R
    from gpemu.sampler import DeviceSampler
    path, analysis, h5io = _analysis(tmp_path, monkeypatch)
    mc = analysis["parameters"]["mcmc"]
    mc.update(n_burn_steps=20, n_sampling_steps=40, reweight={"reference_prior": True})
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.reweight_summaries is None
    c0 = R.wsummary_path_counts()
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    today = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert R.wsummary_path_counts() == c0                        # without the key: no launch of the new family
    base = {"reweight_names"} | {f"reweight_{k}" for k in mcmc.REWEIGHT_SHARED_KEYS} | \
        {f"reweight_reference_prior_{k}" for k in mcmc.REWEIGHT_KEYS}
    assert set(today) == USUAL | base, set(today) ^ (USUAL | base)

    seen = []
    inner = DeviceSampler.reweight

    def recording(self, *a, **kw):
        out = inner(self, *a, **kw)
        seen.append(out)
        return out
    monkeypatch.setattr(DeviceSampler, "reweight", recording)
    mc.update(reweight_summaries={"hpd": CONF, "kde": True, "posterior_predictive": True})
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.reweight_summaries == {"hpd": CONF, "kde": True, "posterior_predictive": True}
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    p = "reweight_reference_prior_"
    new = {"reweight_hpd_confidence", p + "hpd"} | {p + f"kde_{k}" for k in ("grid", "density", "bandwidth")} | \
        {p + f"pp_{k}" for k in mcmc.REWEIGHT_PP_KEYS}
    assert set(back) == USUAL | base | new, set(back) ^ (USUAL | base | new)
    for k in (USUAL - {"autocorrelation_time"}) | base:          # (no autocorrelation time from so short a chain)
        assert np.asarray(back[k]).tobytes() == np.asarray(today[k]).tobytes(), k           # the rest is untouched
    d = back["chain"].shape[2]
    F = back[p + "pp_mean"].shape[0]
    assert back["reweight_hpd_confidence"].tolist() == CONF and back[p + "hpd"].shape == (2, d, 2)
    assert back[p + "kde_grid"].shape == back[p + "kde_density"].shape == (d, 200) and back[p + "kde_bandwidth"].shape == (d,)
    assert back[p + "pp_quantiles"].shape == (3, F) and back[p + "pp_variance_emulator"].shape == (F,)
    assert np.all(back[p + "hpd"][..., 0] <= back[p + "hpd"][..., 1]) and np.all(back[p + "kde_density"] >= 0)
    # ... DeviceSampler.reweight's, on the chain where it lay
    assert len(seen) == 1 and len(seen[0]) == 1
    res = seen[0][0]
    assert np.asarray(res["hpd"]).tobytes() == back[p + "hpd"].tobytes()
    for k in ("grid", "density", "bandwidth"):
        assert np.asarray(res[f"kde_{k}"]).tobytes() == back[p + f"kde_{k}"].tobytes(), k
    assert len(res["posterior_predictive"]) == 1                 # one group, a trivial sort: the merge is the identity
    for k in mcmc.REWEIGHT_PP_KEYS:
        assert np.asarray(res["posterior_predictive"][0][k]).tobytes() == back[p + f"pp_{k}"].tobytes(), k
    # ... and mcmc.reweight's, recomputed from the file through the host entries
    monkeypatch.setattr(DeviceSampler, "reweight", inner)
    again = mcmc.reweight(cfg)
    assert set(again) == base | new
    for k in new:
        assert np.asarray(again[k]).tobytes() == np.asarray(back[k]).tobytes(), k
    only = mcmc.reweight(cfg, kde=False, posterior_predictive=False)
    assert set(only) == base | {"reweight_hpd_confidence", p + "hpd"}
    # a failure of the new entries is logged and the chain is written with today's entries
    mc.update(reweight_summaries={"hpd": [0.5], "kde": True})
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)

    def failing(*a, **kw):
        raise RuntimeError("no intervals today")
    monkeypatch.setattr(R, "weighted_hpd_dev", failing)
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    assert set(h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)) == USUAL | base
