"""-m gpu tests of the posterior-predictive reduction (gpemu_posterior_predictive*, DeviceModel / DeviceSampler
.posterior_predictive) against tests/pp_ref.py: the extended-precision per-sample reference of
tests/hp_ref.py, back-projected and summarised in longdouble, with the tolerances that follow from its bound delta.

Figures measured on an MI355X are printed by every test before it asserts (run with -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

import pp_ref as P
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.5, 0.95)
SIZES = (1, 2, 257, 4096, 20000)
KINDS = {
    "rbf": dict(d=6, spec=O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=False, has_noise=True)),
    "matern25": dict(d=6, spec=O.KernelSpec(kind=O.MATERN, nu=2.5, has_const=False, has_noise=True)),
    "matern_nu": dict(d=5, spec=O.KernelSpec(kind=O.MATERN, nu=1.2, has_const=False, has_noise=True)),
    "wide_d12": dict(d=12, spec=O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=False, has_noise=True)),
    "const_white": dict(d=6, spec=O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=True, has_noise=True)),
}
N_DESIGN, N_FEAT, N_PC = 100, 40, 3


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(model, device model, pool of 20 000 rows inside the design box, per-sample reference of the pool)"""
    import golden_util as GU
    c = KINDS[kind]
    model, lo, hi = P.problem(N_DESIGN, c["d"], N_FEAT, N_PC, c["spec"], seed=sorted(KINDS).index(kind))
    X = np.random.default_rng(11).uniform(lo, hi, (max(SIZES), c["d"]))
    return model, GU.device_model(model), X, P.per_sample(model, X)


def _fixed_theta_case():
    import golden_util as GU
    model, prob, _ = GU.fixed_theta_model(200, 100, 5, seed=0)
    return model, GU.device_model(model), prob


def _compare(out, mu, sigma2, delta, label):
    ref = P.summaries(mu, sigma2, PROBS)
    tol = P.tolerances(mu, delta, ref["variance_parameters"])
    for key in ("mean", "variance_parameters", "quantiles"):
        err = np.abs(np.asarray(out[key] - ref[key], dtype=np.float64))
        print(f"{label} {key}: max err {err.max():.3e}, max err / tol {np.max(err / tol[key]):.3e}")
        assert np.all(err <= tol[key]), key
    ve = np.asarray(ref["variance_emulator"], dtype=np.float64)
    err = np.abs(out["variance_emulator"] - ve)
    print(f"{label} variance_emulator: max rel err {np.max(err / ve):.3e}")
    assert np.all(err <= P.VAR_EMU_RTOL * ve + P.VAR_EMU_ATOL)
    assert np.array_equal(out["variance"], out["variance_parameters"] + out["variance_emulator"])
    assert np.array_equal(out["probabilities"], np.asarray(PROBS))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_summaries_against_the_extended_precision_reference(kind):
    model, dm, X, (mu, sigma2, delta) = _case(kind)
    for S in SIZES:
        out = dm.posterior_predictive(X[:S], probabilities=PROBS)
        assert out["mean"].shape == (N_FEAT,) and out["quantiles"].shape == (len(PROBS), N_FEAT)
        _compare(out, mu[:S], sigma2[:S], delta[:S], f"{kind} S={S}")


def test_fixed_theta_model_against_the_reference():
    model, dm, prob = _fixed_theta_case()
    X = np.random.default_rng(3).uniform(prob["lo"], prob["hi"], (257, prob["lo"].size))
    mu, sigma2, delta = P.per_sample(model, X)
    _compare(dm.posterior_predictive(X, probabilities=PROBS), mu, sigma2, delta, "fixed_theta S=257")


@pytest.mark.parametrize("kind", ["rbf", "wide_d12"])
def test_quantiles_equal_select_of_the_devices_own_central_values(kind):
    """quantiles = select.quantile of predict_full's central_value, within delta (the projection is cross_validate's)"""
    from gpemu import select
    model, dm, X, (mu, sigma2, delta) = _case(kind)
    S = 257
    cv, _ = dm.predict_full(X[:S], n_div=1.0)
    out = dm.posterior_predictive(X[:S], probabilities=PROBS)
    q = select.quantile(cv, PROBS, axis=0)
    err = np.abs(out["quantiles"] - q)
    d = delta[:S].max(axis=0)
    print(f"{kind}: quantiles vs select.quantile(central_value): max err {err.max():.3e}, max err / delta "
          f"{np.max(err / d):.3e}")
    assert np.all(err <= d)
    assert np.all(np.abs(out["mean"] - cv.mean(axis=0)) <= d + S * 2.0 ** -53 * np.abs(cv).max(axis=0))


def _same(a, b):
    for key in ("mean", "variance_parameters", "variance_emulator", "variance", "quantiles"):
        assert a[key].tobytes() == b[key].tobytes(), key


def test_results_do_not_depend_on_the_workspace_or_the_run():
    from gpemu.model import POSTPRED_PATHS, postpred_path_counts, postpred_workspace_bytes
    model, dm, X, _ = _case("rbf")
    S = 4096 + 33
    whole = dm.posterior_predictive(X[:S], probabilities=PROBS)
    _same(whole, dm.posterior_predictive(X[:S], probabilities=PROBS))
    iw, ib, ik = (POSTPRED_PATHS.index(n) for n in ("whole", "feature_blocked", "feature_block"))
    for per_block, blocks in ((48, 1), (16, 3), (32, 2)):
        c0 = postpred_path_counts()
        out = dm.posterior_predictive(X[:S], probabilities=PROBS,
                                      workspace_bytes=postpred_workspace_bytes(S, N_PC, per_block))
        c1 = postpred_path_counts() - c0
        print(f"workspace for {per_block} features: counters {dict(zip(POSTPRED_PATHS, c1))}")
        assert c1[ik] == blocks and c1[iw] == (blocks == 1) and c1[ib] == (blocks > 1)
        _same(whole, out)
    # many blocks: a model of 100 features, 16 at a time
    model2, dm2, prob = _fixed_theta_case()
    X2 = np.random.default_rng(4).uniform(prob["lo"], prob["hi"], (2049, prob["lo"].size))
    c0 = postpred_path_counts()
    blocked = dm2.posterior_predictive(X2, probabilities=PROBS, workspace_bytes=postpred_workspace_bytes(2049, 5, 16))
    assert (postpred_path_counts() - c0)[ik] == 7
    _same(dm2.posterior_predictive(X2, probabilities=PROBS), blocked)


def test_too_small_a_workspace_is_an_out_of_memory_error_with_sizes():
    from gpemu import _lib
    from gpemu.model import postpred_workspace_bytes
    model, dm, X, _ = _case("rbf")
    with pytest.raises(_lib.GpemuError) as e:
        dm.posterior_predictive(X[:257], workspace_bytes=postpred_workspace_bytes(257, N_PC, 15))
    assert e.value.code == -2 and "out of memory" in str(e.value) and str(16 * 257 * N_PC) in str(e.value)


def test_non_finite_rows_are_refused_and_no_probabilities_skip_the_selection():
    model, dm, X, _ = _case("rbf")
    bad = X[:5].copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        dm.posterior_predictive(bad)
    out = dm.posterior_predictive(X[:300], probabilities=None)
    assert out["quantiles"].shape == (0, N_FEAT) and out["probabilities"].size == 0
    _same_keys = ("mean", "variance_parameters", "variance_emulator")
    ref = dm.posterior_predictive(X[:300], probabilities=PROBS)
    for key in _same_keys:
        assert out[key].tobytes() == ref[key].tobytes()


def _dev_call(dm, dX, n_blocks, block_rows, block_stride_rows, S):
    import torch
    from gpemu.model import QuantilePlan
    plan = QuantilePlan(S, PROBS)
    bufs = torch.empty((3, dm.F), dtype=torch.float64, device="cuda:0")
    order = torch.empty((dm.F, plan.ranks.size), dtype=torch.float64, device="cuda:0")
    dm.posterior_predictive_dev(dX, n_blocks, block_rows, block_stride_rows, plan.ranks, bufs[0].data_ptr(),
                                bufs[1].data_ptr(), bufs[2].data_ptr(), order.data_ptr())
    h = bufs.cpu().numpy()
    return plan.result(h[0].copy(), h[1].copy(), h[2].copy(), order.cpu().numpy())


def test_block_form_equals_the_contiguous_gather():
    import torch
    model, dm, X, _ = _case("rbf")
    d = X.shape[1]
    T, W = 40, 96
    chain = X[:T * W].reshape(T, W, d)
    dchain = torch.as_tensor(chain, device="cuda:0")
    # thin = 3, discard = 5, all walkers
    rows = chain[5::3].reshape(-1, d)
    nb = chain[5::3].shape[0]
    got = _dev_call(dm, dchain.data_ptr() + 8 * 5 * W * d, nb, W, 3 * W, nb * W)
    _same(dm.posterior_predictive(rows, probabilities=PROBS), got)
    # a stacked 3-chain layout, chain 1: walkers [32, 64) of every step
    Wc = W // 3
    rows = chain[:, Wc:2 * Wc].reshape(-1, d)
    got = _dev_call(dm, dchain.data_ptr() + 8 * Wc * d, T, Wc, W, T * Wc)
    _same(dm.posterior_predictive(rows, probabilities=PROBS), got)
    # blocks longer than a predict pass: one rung of 2 with 2500 walkers
    big = X[:3 * 5000].reshape(3, 5000, d)
    got = _dev_call(dm, torch.as_tensor(big, device="cuda:0").data_ptr(), 3, 2500, 5000, 7500)
    _same(dm.posterior_predictive(big[:, :2500].reshape(-1, d), probabilities=PROBS), got)


def _likelihood(dm, prob):
    dm.likelihood_setup(prob["y_exp"], prob["y_err"], prob["lo"], prob["hi"], 1.0)


def _assert_parameter_quantiles(chain2d, got, probs):
    from gpemu import select
    want = np.quantile(chain2d, probs, axis=0, method="linear")
    lo, hi, _ = select.virtual_index(chain2d.shape[0], probs)
    srt = np.sort(chain2d, axis=0)
    tol = 2 * np.spacing(np.maximum(np.abs(srt[lo]), np.abs(srt[hi])))
    assert np.all(np.abs(got - want) <= tol)


def test_sampler_summaries_read_the_device_chain_in_place():
    from gpemu import synthetic
    from gpemu.sampler import DeviceSampler
    model, dm, prob = _fixed_theta_case()
    _likelihood(dm, prob)
    W, d = 64, prob["lo"].size
    s = DeviceSampler([dm], W, seed=5)
    s.set_state(synthetic.make_walkers(W, seed=1))
    s.run(30)
    chain, _ = s.get_chain()
    got = s.posterior_predictive(probabilities=PROBS)
    assert len(got) == 1
    _same(dm.posterior_predictive(chain.reshape(-1, d), probabilities=PROBS), got[0])
    got = s.posterior_predictive(discard=4, thin=3, probabilities=PROBS)[0]
    _same(dm.posterior_predictive(chain[4::3].reshape(-1, d), probabilities=PROBS), got)
    probs = [0.05, 0.16, 0.5, 0.84, 0.95]
    _assert_parameter_quantiles(chain[4:].reshape(-1, d), s.parameter_quantiles(probs, discard=4), probs)
    s.close()


def test_stacked_and_tempered_samplers():
    from gpemu import synthetic
    from gpemu.sampler import DeviceSampler, TemperedSampler
    model, dm, prob = _fixed_theta_case()
    d = prob["lo"].size
    W = 32
    dm.likelihood_setup(np.stack([prob["y_exp"], prob["y_exp"] * 1.01, prob["y_exp"] * 0.99]), prob["y_err"], prob["lo"],
                        prob["hi"], 1.0)
    s = DeviceSampler([dm], W, seeds=[1, 2, 3])
    s.set_state(np.concatenate([synthetic.make_walkers(W, seed=c) for c in range(3)]))
    s.run(12)
    chain, _ = s.get_chain()
    with pytest.raises(ValueError):
        s.posterior_predictive()
    got = s.posterior_predictive(chain=1, discard=2, probabilities=PROBS)[0]
    rows = chain[2:, W:2 * W].reshape(-1, d)
    _same(dm.posterior_predictive(rows, probabilities=PROBS), got)
    _assert_parameter_quantiles(rows, s.parameter_quantiles([0.1, 0.9], discard=2, chain=1), [0.1, 0.9])
    s.close()
    _likelihood(dm, prob)
    t = TemperedSampler([dm], W, betas=[1.0, 0.5, 0.1], seed=3)
    t.set_state(np.concatenate([synthetic.make_walkers(W, seed=c) for c in range(3)]))
    t.run(12)
    rung0, _ = t.get_chain(temp=0)
    _same(dm.posterior_predictive(rung0.reshape(-1, d), probabilities=PROBS), t.posterior_predictive(probabilities=PROBS)[0])
    _assert_parameter_quantiles(rung0.reshape(-1, d), t.parameter_quantiles([0.5]), [0.5])
    t.close()


def test_c3_size_finishes_on_the_whole_path():
    """N = 1000, F = 500, k = 10, S = 1024 x 200: mean and quantiles of 8 features against a host reduction of the
    device's own central values; the path counters show one whole-workspace reduction and 8 select passes."""
    import time

    import golden_util as GU
    from gpemu.model import POSTPRED_PATHS, postpred_path_counts
    model, prob, _ = GU.fixed_theta_model(1000, 500, 10, seed=0)
    dm = GU.device_model(model)
    S, d = 1024 * 200, prob["lo"].size
    X = np.random.default_rng(8).uniform(prob["lo"], prob["hi"], (S, d))
    c0 = postpred_path_counts()
    t0 = time.perf_counter()
    out = dm.posterior_predictive(X, probabilities=PROBS)
    dt = time.perf_counter() - t0
    c1 = dict(zip(POSTPRED_PATHS, postpred_path_counts() - c0))
    print(f"C3 size: S = {S}, {dt:.3f} s host to host, counters {c1}")
    assert c1 == {"whole": 1, "feature_blocked": 0, "feature_block": 1, "select_pass": 8}
    # the device's own central values of 8 features: PC means, projected on the host as the kernel projects them
    feats = np.array([0, 1, 63, 64, 250, 333, 498, 499])
    mean_pc = np.concatenate([dm.gp_predict(X[i:i + 16384])[0] for i in range(0, S, 16384)])
    comp = model.components[:10][:, feats]
    cv = (mean_pc @ comp) * model.scaler_scale[feats] + model.scaler_mean[feats]
    # both projections round k products, k sums, the scaling and the shift, each within (k + 2) u of the sum of the
    # absolute terms; an order statistic moves by at most the largest difference over the samples
    mag = (np.abs(mean_pc) @ np.abs(comp)) * np.abs(model.scaler_scale[feats]) + np.abs(model.scaler_mean[feats])
    tol = 2 * (10 + 2) * 2.0 ** -53 * mag.max(axis=0)
    q = np.quantile(cv, PROBS, axis=0, method="linear")
    print("C3 size: max |quantile - host| / tol", float(np.max(np.abs(out["quantiles"][:, feats] - q) / tol)))
    assert np.all(np.abs(out["quantiles"][:, feats] - q) <= tol)
    assert np.all(np.abs(out["mean"][feats] - cv.mean(axis=0)) <= tol + S * 2.0 ** -53 * mag.max(axis=0))
    assert np.all(out["variance_emulator"] > 0) and np.all(out["variance_parameters"] > 0)
    dm.close()


# ---- the drop-in: merge over the shipped three groups (golden G7), the YAML key of run_mcmc (golden G1) -------------
class _GroupCfg:
    def __init__(self, n_pc):
        self.n_pc = n_pc


class _EmuCfg:
    def __init__(self, groups, sorter):
        self.emulation_groups_config = groups
        self.sort_observables_in_matrix = sorter


def test_dropin_merge_over_the_three_shipped_groups_is_a_scatter():
    import dropin_util as DU
    import golden_util as GU
    from bayesian_inference import emulation
    g = GU.load("g7_shipped_config")
    names, mapping, block_start, cols = GU.g7_groups(g)
    sorter = emulation.SortEmulationGroupObservables(mapping, tuple(int(v) for v in g["map_shape"]))
    res = {}
    for n in names:
        sub = {k[len(n) + 1:]: v for k, v in g.items() if k.startswith(n + "_")}
        sub.update(design=g["design"], gpr_alpha=g["gpr_alpha"])
        res[n] = DU.results_at_golden_theta(sub)
    emu_cfg = _EmuCfg({n: _GroupCfg(int(g[n + "_n_pc"])) for n in names}, sorter)
    X = np.random.default_rng(2).uniform(g["lo"], g["hi"], (700, g["lo"].size))
    merged = emulation.posterior_predictive(X, emu_cfg, emulation_group_results=res, probabilities=(0.16, 0.5, 0.84))
    per_group = emulation.posterior_predictive(X, emu_cfg, emulation_group_results=res, probabilities=(0.16, 0.5, 0.84),
                                               merge_predictions_over_groups=False)
    F = sorter.shape[1]
    assert merged["mean"].shape == (F,) and merged["quantiles"].shape == (3, F)
    covered = np.zeros(F, dtype=bool)
    for _, (grp, so, sg) in mapping.items():
        dm = emulation.device_model_for(res[grp], emu_cfg.emulation_groups_config[grp].n_pc)
        own = dm.posterior_predictive(X, probabilities=(0.16, 0.5, 0.84))
        for key in ("mean", "variance_parameters", "variance_emulator", "variance"):
            assert np.array_equal(merged[key][so], own[key][sg]) and np.array_equal(own[key], per_group[grp][key])
        assert np.array_equal(merged["quantiles"][:, so], own["quantiles"][:, sg])
        covered[so] = True
    assert covered.all()
    # the merged order is predict's: the mean of predict's central values, at the project's parity bound 1e-9 max|y|
    cv = np.concatenate([emulation.predict(X[i:i + 100], emu_cfg, emulation_group_results=res)["central_value"]
                         for i in range(0, 700, 100)])
    assert np.all(np.abs(merged["mean"] - cv.mean(axis=0)) <= 1e-9 * np.abs(cv).max())
    emulation.release_device_models()


USUAL = {"chain", "acceptance_fraction", "log_prob", "autocorrelation_time"}
PP_KEYS = {"posterior_predictive_" + k for k in ("mean", "variance_parameters", "variance_emulator", "quantiles",
                                                 "probabilities")}


def test_run_mcmc_yaml_key_adds_five_datasets_and_nothing_without_it(tmp_path, monkeypatch):
    import dropin_util as DU
    import golden_util as GU
    from bayesian_inference import emulation, log_posterior, mcmc
    from gpemu import h5io
    g = GU.load("g1_rbf_noise")
    written = {}
    io = DU.install_fake_data_IO(g["Y"], g["design"], g["y_exp"], g["y_err"], written)
    io.read_dict_from_h5 = lambda output_dir, filename, verbose=True: h5io.read_dict_from_h5(output_dir, filename)
    path, analysis = DU.write_config(tmp_path, n_pc=5, n_restarts=0)
    ec = emulation.EmulationConfig.from_config_file("test_analysis", "exponential", path, analysis)
    ec._sort_observables_in_matrix = None
    np.random.seed(1)
    emulation.fit_emulators(ec)
    monkeypatch.setattr(emulation.EmulationConfig, "sort_observables_in_matrix",
                        property(lambda self: DU.TrivialSort("main")))
    monkeypatch.setattr(emulation.EmulationConfig, "observable_filter", property(lambda self: None))
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.posterior_predictive is False
    np.random.seed(2)
    mcmc.run_mcmc(cfg)
    assert set(h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)) == USUAL
    analysis["parameters"]["mcmc"]["posterior_predictive"] = True
    analysis["parameters"]["mcmc"]["posterior_predictive_probabilities"] = [0.16, 0.5, 0.84, 0.975]
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.posterior_predictive is True
    np.random.seed(2)
    mcmc.run_mcmc(cfg)
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(back) == USUAL | PP_KEYS
    F = g["Y"].shape[1]
    assert back["posterior_predictive_mean"].shape == (F,) and back["posterior_predictive_quantiles"].shape == (4, F)
    assert np.array_equal(back["posterior_predictive_probabilities"], [0.16, 0.5, 0.84, 0.975])
    # the stored datasets are those of the stored chain, and mcmc.posterior_predictive recomputes them from mcmc.h5
    again = mcmc.posterior_predictive(cfg, probabilities=(0.16, 0.5, 0.84, 0.975))
    for key in ("mean", "variance_parameters", "variance_emulator", "quantiles"):
        assert np.array_equal(again[key], back["posterior_predictive_" + key]), key
    thinned = mcmc.posterior_predictive(cfg, discard=2, thin=2)
    assert thinned["quantiles"].shape == (3, F) and np.all(np.isfinite(thinned["variance"]))
    assert np.all(np.diff(back["posterior_predictive_quantiles"], axis=0) >= 0)
    log_posterior.initialize_pool_variables(None, None, None, None, None, None)
    emulation.release_device_models()
