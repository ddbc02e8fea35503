"""-m gpu: correlated experimental uncertainties on the device.

(a) ``cov = diag(y_err**2)`` without sources gives the bits of today's setup; (b) within-observable correlations and
S in {1, 4, 16} fully correlated sources stay within the bound of the extended-precision reference (tests/srccorr_ref.py)
on the likelihood's launch forms -- every case of tests/path_cases.py, with ``gpemu_path_counts`` naming the form that
ran, plus an observable block over 256 features (the blocked setup) -- and ``gpemu_src_path_counts`` shows that the
sources' launch ran; (c) the documented errors; (d) the host-RNG replay takes the accept decisions of
oracle/sampler_oracle.py driven by the dense reference, stacked chains equal their single-chain runs bit for bit,
tempered rung 0 holds the joint evaluation; (e) the drop-in ``log_posterior`` and ``run_mcmc`` with
``parameters.mcmc.data_covariance``.
"""
import numpy as np
import pytest

import golden_util as GU
import hp_ref as H
import srccorr_ref as R
from gpemu import model as GM
from gpemu._lib import GpemuError
from gpemu.sampler import DeviceSampler

pytestmark = pytest.mark.gpu

CORRECTION, SETUP_COV, SETUP_SOURCES, EXACT_COV, SETUP_BLOCKED, CORRECTION_K64 = range(6)


def _models(c):
    return [GU.device_model(model) for model, _, _ in c["groups"]]


def _setup(dms, c, cov=None, src=None, n_div=1.0, y=None):
    y = c["y"] if y is None else y
    for dm, (_, cols, bs) in zip(dms, c["groups"]):
        kw = {}
        if cov is not None:
            kw["cov"] = cov[np.ix_(cols, cols)]
        if src is not None:
            kw["sys_sources"] = src[:, cols]
        dm.likelihood_setup(y[..., cols], c["y_err"][cols], c["lo"], c["hi"], n_div=n_div, block_start=bs, **kw)


def _close(dms):
    for dm in dms:
        dm.close()


@pytest.mark.parametrize("name", ["G1", "G5", "G7"])
def test_diag_cov_without_sources_same_bits(name):
    c = R.case(name)
    dms = _models(c)
    X = c["Xq"]
    _setup(dms, c)
    today = [dm.logpost(X) for dm in dms]
    today_exact = [dm.logpost(X, mode=GM.EXACT) for dm in dms]
    _setup(dms, c, cov=np.diag(c["y_err"] ** 2), src=np.zeros((0, c["y"].shape[0])))
    for dm, lp, lpx in zip(dms, today, today_exact):
        np.testing.assert_array_equal(dm.logpost(X), lp)
        np.testing.assert_array_equal(dm.logpost(X, mode=GM.EXACT), lpx)
    np.testing.assert_allclose(GM.logpost_groups(dms, X), np.sum(today, axis=0), rtol=1e-13)
    _close(dms)


def _reference(c, X, Cd, src, n_div=1.0, input_rounding=False):
    preds = [H.gp_predict(X, model, input_rounding=input_rounding) for model, _, _ in c["groups"]]
    means = [p[0] for p in preds]
    vars_ = [p[1] for p in preds]
    ref, *_ = R.dense_logpost(c, X, means, vars_, Cd, n_div)
    bnd = R.bound(c, X, [np.asarray(m, dtype=np.float64) for m in means], [np.asarray(v, dtype=np.float64) for v in vars_],
                  [p[2] for p in preds], [p[3] for p in preds], Cd, src, n_div)
    return np.asarray(ref, dtype=np.float64), bnd


def _within(got, ref, bnd):
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(got)), "-inf rows differ"
    assert np.all(got[~fin] == -np.inf)
    err = np.abs(got[fin] - ref[fin])
    assert np.all(err <= bnd[fin]), (err.max(), bnd[fin][np.argmax(err - bnd[fin])])


# launch forms of the likelihood stage (gpemu_api.hip: logpost_eval), chosen by the switches it reads per call
SWITCHES = {"default": {}, "no_tasks": {"GPEMU_NO_LOGLIK_TASKS": "1"}, "per_group": {"GPEMU_NO_GROUP_MERGE": "1"}}


@pytest.mark.parametrize("name", ["G1", "G5", "G7"])
@pytest.mark.parametrize("S", [1, 4, 16])
@pytest.mark.parametrize("form", list(SWITCHES))
def test_sources_within_reference_bound(name, S, form, monkeypatch):
    for key, val in SWITCHES[form].items():
        monkeypatch.setenv(key, val)
    c = R.case(name)
    X = c["Xq"]
    Cd, cov, src = R.data_covariance(c, S, seed=11 + S)
    dms = _models(c)
    _setup(dms, c, cov=cov, src=src)
    n0 = GM.src_path_counts()
    got = GM.logpost_groups(dms, X)
    assert GM.src_path_counts()[CORRECTION] > n0[CORRECTION]
    ref, bnd = _reference(c, X, Cd, src)
    _within(got, ref, bnd)
    # the reference's batch semantics: n_div = number of rows in the box
    n_in = int(np.count_nonzero(np.all((X > c["lo"]) & (X < c["hi"]), axis=1)))
    _setup(dms, c, cov=cov, src=src, n_div=float(n_in))
    ref_b, bnd_b = _reference(c, X, Cd, src, n_div=float(n_in))
    _within(GM.logpost_groups(dms, X), ref_b, bnd_b)
    _close(dms)


@pytest.mark.parametrize("name", ["G1", "G7"])
def test_large_batch_with_sources(name):
    """more than 256 rows (the large-batch variants of every stage): rows equal a small call's to rounding"""
    from gpemu import synthetic
    c = R.case(name)
    Cd, cov, src = R.data_covariance(c, 4, seed=3)
    dms = _models(c)
    _setup(dms, c, cov=cov, src=src)
    X = synthetic.make_walkers(600, seed=5, lo=c["lo"], hi=c["hi"])
    big = GM.logpost_groups(dms, X)
    ref, bnd = _reference(c, X[:6], Cd, src)
    _within(big[:6], ref, bnd)
    np.testing.assert_allclose(big[290:300], GM.logpost_groups(dms, X[290:300]), rtol=1e-11)
    _close(dms)


@pytest.mark.parametrize("name", ["G1", "G5"])
def test_exact_mode_reads_within_observable_cov(name):
    c = R.case(name)
    X = c["Xq"]
    Cd, cov, _ = R.data_covariance(c, 0, seed=0)
    dms = _models(c)
    _setup(dms, c, cov=cov)
    n0 = GM.src_path_counts()
    got_x = GM.logpost_groups(dms, X, mode=GM.EXACT)
    assert GM.src_path_counts()[EXACT_COV] > n0[EXACT_COV]
    got_l = GM.logpost_groups(dms, X)
    ref, bnd = _reference(c, X, Cd, None)
    _within(got_x, ref, bnd)
    _within(got_l, ref, bnd)
    _close(dms)


def test_documented_errors():
    c = R.case("G5")
    dms = _models(c)
    y_err = c["y_err"]
    with pytest.raises(GpemuError) as e:
        _setup(dms, c, src=R.sources(y_err, 17, seed=1))
    assert e.value.code == -1
    # a dense entry across two observables
    cov = np.diag(y_err ** 2)
    i, j = np.flatnonzero(c["obs"] == 0)[0], np.flatnonzero(c["obs"] == 1)[0]
    cov[i, j] = cov[j, i] = 0.1 * y_err[i] * y_err[j]
    with pytest.raises(GpemuError) as e:
        _setup(dms, c, cov=cov)
    assert e.value.code == -1 and "sources" in str(e.value)
    # groups that disagree on S: the sampler refuses them at creation, the joint evaluation at evaluation
    _, _, src = R.data_covariance(c, 2, seed=1)
    _setup(dms, c, src=src)
    (_, cols, bs) = c["groups"][1]
    dms[1].likelihood_setup(c["y"][cols], y_err[cols], c["lo"], c["hi"], block_start=bs, sys_sources=src[:1, cols])
    with pytest.raises(GpemuError) as e:
        DeviceSampler(dms, 16, seed=1)
    assert e.value.code == -1
    with pytest.raises(GpemuError) as e:
        GM.logpost_groups(dms, c["Xq"])
    assert e.value.code == -4
    # the exact form has no sources' term
    _setup(dms, c, src=src)
    with pytest.raises(GpemuError) as e:
        dms[0].logpost(c["Xq"], mode=GM.EXACT)
    assert e.value.code == -5
    _close(dms)


def test_sampler_logprob_is_joint_evaluation():
    """the fused sampler with sources: every stored log-probability is the joint evaluation of the stored position"""
    from gpemu import synthetic
    c = R.case("G7")
    _, cov, src = R.data_covariance(c, 4, seed=9)
    dms = _models(c)
    _setup(dms, c, cov=cov, src=src)
    n0 = GM.src_path_counts()
    s = DeviceSampler(dms, 64, seed=5)
    X0 = synthetic.make_walkers(64, seed=2, lo=c["lo"], hi=c["hi"])
    s.set_state(X0)
    _, lp0 = s.get_state()
    np.testing.assert_allclose(lp0, GM.logpost_groups(dms, X0), rtol=1e-11)
    s.run(6, store=True)
    chain, lp = s.get_chain()
    nacc, _, _ = s.counts()
    assert nacc.sum() > 0
    for t in (0, 5):
        np.testing.assert_allclose(lp[t], GM.logpost_groups(dms, chain[t]), rtol=1e-11)
    assert GM.src_path_counts()[CORRECTION] > n0[CORRECTION]
    s.close()
    _close(dms)


# ---- (b) on every likelihood launch path of tests/path_cases.py ----------------------------------------------------------
import math  # noqa: E402

import path_cases as PC  # noqa: E402
from gpemu import _lib  # noqa: E402

PATH_CASES = PC.cases(256) + [
    # an observable block over 256 features: the blocked setup (lik_z_kernel / lik_gram_kernel) with the source columns
    PC.Case("f300_blocked_setup", 100, 3, 6, 40, PC.O.RBF, np.inf, False, nblk=1, F=300),
    PC.Case("f300_blocked_setup_k40", 100, 3, 40, 24, PC.O.MATERN, 2.5, False, nblk=1, F=300),
]


def _path_counts():
    import ctypes as C
    out = np.zeros(len(PC.PATHS), dtype=np.int64)
    _lib.lib().gpemu_path_counts(out.ctypes.data_as(C.POINTER(C.c_int64)), out.size)
    return out


def _num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _single_case(c, model, lo, hi, y_exp, y_err, bs):
    F = y_exp.shape[0]
    obs = np.zeros(F, dtype=np.int64)
    for o in range(len(bs) - 1):
        obs[bs[o]:bs[o + 1]] = o
    return dict(groups=[(model, np.arange(F), [int(v) for v in bs])], y=y_exp, y_err=y_err, lo=lo, hi=hi, obs=obs)


@pytest.mark.parametrize("S", [1, 16])
@pytest.mark.parametrize("idx", range(len(PATH_CASES)), ids=[c.name for c in PATH_CASES])
def test_path_cases_with_cov_and_sources(idx, S):
    ncu = _num_cu()
    cs = PC.cases(ncu) + PATH_CASES[len(PC.cases(256)):]
    c = cs[idx]
    model, lo, hi, y_exp, y_err, bs, rng = PC.problem(c)
    Xq, _, cols = PC.queries(c, model, lo, hi, rng)
    cc = _single_case(c, model, lo, hi, y_exp, y_err, bs)
    Cd, cov, src = R.data_covariance(cc, S, seed=3 + S)
    dm = GU.device_model(model)
    s0 = GM.src_path_counts()
    dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0, block_start=bs, cov=cov, sys_sources=src)
    p0 = _path_counts()
    out = dm.logpost(Xq)
    dp, ds = _path_counts() - p0, GM.src_path_counts() - s0
    missing = [p for p in sorted(PC.logpost_paths(c, ncu)) if dp[PC.PATH[p]] == 0]
    assert not missing, f"{c.name}: likelihood paths not taken {missing}"
    assert ds[CORRECTION] == math.ceil(c.B / PC.MAX_CHUNK)
    assert ds[SETUP_COV] == 1 and ds[SETUP_SOURCES] == 1
    assert (ds[CORRECTION_K64] > 0) == (c.k > 32)
    assert (ds[SETUP_BLOCKED] > 0) == (int(np.max(np.diff(bs))) > 256)
    # the reference on the special columns (a few rows where the blocks are large: longdouble is slow there)
    X = Xq[cols[:6] if c.F > 256 else cols]
    got = out[cols[:6] if c.F > 256 else cols]
    ref, bnd = _reference(cc, X, Cd, src, input_rounding=c.ls_bounds)
    _within(got, ref, bnd)
    dm.close()


# ---- (d) the samplers ---------------------------------------------------------------------------------------------------
from oracle import gp_oracle as O  # noqa: E402
from oracle import sampler_oracle as SO  # noqa: E402


def _dense_lp_fn(c, Cd):
    def lp(X):
        X = np.atleast_2d(X)
        means, vars_ = [], []
        for model, _, _ in c["groups"]:
            m, v = O.gp_predict_all(X, model)
            means.append(np.asarray(m, dtype=np.float64))
            vars_.append(np.asarray(v, dtype=np.float64))
        return np.asarray(R.dense_logpost(c, X, means, vars_, Cd)[0], dtype=np.float64)
    return lp


def test_host_rng_replay_with_sources_equals_oracle():
    """gpemu_sampler_step_host_rng on two groups with within-observable correlation and 4 sources takes the accept
    decisions of oracle/sampler_oracle.py whose log-probability is the dense reference"""
    from gpemu import synthetic
    c = R.case("G5")
    Cd, cov, src = R.data_covariance(c, 4, seed=21)
    dms = _models(c)
    _setup(dms, c, cov=cov, src=src)
    W, steps = 20, 8
    X0 = synthetic.make_walkers(W, seed=5, lo=c["lo"], hi=c["hi"])
    ds = DeviceSampler(dms, W)
    ds.set_state(X0)
    stream = SO.EmceeStream(2024)
    for _ in range(steps):
        ds.step_host_rng(*stream.draw(W))
    chain, lps = ds.get_chain()
    nacc = ds.counts()[0]
    ochain, olps, onacc = SO.run(X0, _dense_lp_fn(c, Cd), SO.EmceeStream(2024), steps)
    np.testing.assert_allclose(chain, ochain, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(nacc, onacc)
    assert 0 < nacc.sum() < W * steps
    fin = np.isfinite(olps)
    assert np.array_equal(fin, np.isfinite(lps))
    np.testing.assert_allclose(lps[fin], olps[fin], rtol=1e-8)
    # without the sources' term the chain would differ: the test sees a missing or wrong term
    o2, _, _ = SO.run(X0, _dense_lp_fn(c, Cd - src.T @ src), SO.EmceeStream(2024), steps)
    assert not np.allclose(o2, ochain)
    ds.close()
    _close(dms)


@pytest.mark.parametrize("W", [24, 33])
def test_stacked_chains_with_sources_equal_single_chains(W):
    """closure-style stacked chains (one data vector per chain) with sources over two groups: bit for bit the chains
    of separate samplers -- the per-chain offsets into g0 / w0 of the sources' launch"""
    from gpemu import synthetic
    c = R.case("G5")
    _, cov, src = R.data_covariance(c, 4, seed=8)
    C, steps = 3, 5
    rng = np.random.default_rng(17)
    ys = c["y"][None, :] + 0.05 * rng.normal(size=(C, c["y"].size)) * c["y_err"][None, :]
    seeds = [101 + 13 * i for i in range(C)]
    X0 = np.concatenate([synthetic.make_walkers(W, seed=40 + i, lo=c["lo"], hi=c["hi"]) for i in range(C)])
    dms = _models(c)
    _setup(dms, c, cov=cov, src=src, y=ys)
    ms = DeviceSampler(dms, W, seeds=seeds)
    ms.set_state(X0)
    lp0 = ms.get_state()[1]
    ms.run(steps)
    chain, lps = ms.get_chain()
    nacc = ms.counts()[0]
    ms.close()
    for i in range(C):
        _setup(dms, c, cov=cov, src=src, y=ys[i])
        one = DeviceSampler(dms, W, seed=seeds[i])
        one.set_state(X0[i * W:(i + 1) * W])
        np.testing.assert_array_equal(one.get_state()[1], lp0[i * W:(i + 1) * W])
        one.run(steps)
        c1, l1 = one.get_chain()
        np.testing.assert_array_equal(chain[:, i * W:(i + 1) * W], c1)
        np.testing.assert_array_equal(lps[:, i * W:(i + 1) * W], l1)
        np.testing.assert_array_equal(nacc[i * W:(i + 1) * W], one.counts()[0])
        one.close()
    # the chains' data vectors differ, so do their log-probabilities at the same point
    lpa = GM.logpost_groups(dms, X0[:4])
    _setup(dms, c, cov=cov, src=src, y=ys[0])
    assert not np.allclose(lpa, GM.logpost_groups(dms, X0[:4]))
    _close(dms)


def test_tempered_rung0_with_sources_equals_direct_evaluation():
    """the tempered accept inside the sources' launch: rung 0's stored log-probabilities are the joint evaluation of its
    positions, and every rung moves"""
    from gpemu import synthetic
    from gpemu.sampler import TemperedSampler
    from gpemu.tempering import geometric_ladder
    c = R.case("G7")
    _, cov, src = R.data_covariance(c, 4, seed=2)
    dms = _models(c)
    _setup(dms, c, cov=cov, src=src)
    T, W = 4, 32
    ts = TemperedSampler(dms, W, geometric_ladder(T, 50.0), seed=77, swap_every=1)
    ts.set_state(synthetic.make_walkers(T * W, seed=9, lo=c["lo"], hi=c["hi"]))
    ts.run(6, store=True)
    chain, lps = ts.get_chain()                      # (steps, T, W, d), (steps, T, W)
    for step in (0, 5):
        x, lp = chain[step, 0], lps[step, 0]
        assert np.all(np.isfinite(lp))
        np.testing.assert_allclose(lp, GM.logpost_groups(dms, x), rtol=1e-11)
    for t in range(T):
        assert np.any(chain[5, t] != chain[0, t])
    ts.close()
    _close(dms)


# ---- (e) the drop-in modules --------------------------------------------------------------------------------------------
import dropin_util as DU  # noqa: E402


class _GroupCfg:
    def __init__(self, n_pc):
        self.n_pc = n_pc


class _EmuCfg:
    def __init__(self, groups, sorter):
        self.emulation_groups_config = groups
        self.sort_observables_in_matrix = sorter


def test_dropin_log_posterior_with_cov_and_sources():
    """log_posterior(X) with experimental_results['cov'] / ['sys_sources'] on the reference's two-group fixture equals the
    dense formula -- batched (n_div = rows in the box) and one walker at a time -- and a cross-observable cov is refused"""
    from bayesian_inference import emulation, log_posterior
    g = GU.load("g5_multigroup")
    c = R.case("G5")
    mapping = {"A": ("g1", slice(0, 10), slice(0, 10)), "B": ("g2", slice(10, 18), slice(0, 8)),
               "C": ("g1", slice(18, 30), slice(10, 22))}
    sorter = emulation.SortEmulationGroupObservables(mapping, (60, 30))
    for grp, (_, cols, bs) in zip(("g1", "g2"), c["groups"]):
        lay_cols, lay_bs = sorter.group_layout(grp)
        assert np.array_equal(lay_cols, cols) and list(lay_bs) == list(bs)
    res, cfgs = {}, {}
    for grp in ("g1", "g2"):
        sub = {k[len(grp) + 1:]: v for k, v in g.items() if k.startswith(grp + "_")}
        sub.update(design=g["design"], gpr_alpha=g["gpr_alpha"])
        res[grp] = DU.results_at_golden_theta(sub, None)
        cfgs[grp] = _GroupCfg(int(sub["n_pc"]))
    emu_cfg = _EmuCfg(cfgs, sorter)
    Cd, cov, src = R.data_covariance(c, 4, seed=31)
    data = {"y": g["y_exp"], "y_err": g["y_err"], "cov": cov, "sys_sources": src}
    log_posterior.initialize_pool_variables(g["lo"], g["hi"], emu_cfg, res, data, None)
    X = g["Xq"][:8]
    lp_fn = _dense_lp_fn(c, Cd)
    n_in = int(np.count_nonzero(np.all((X > g["lo"]) & (X < g["hi"]), axis=1)))
    means, vars_ = [], []
    for model, _, _ in c["groups"]:
        m, v = O.gp_predict_all(X, model)
        means.append(np.asarray(m, dtype=np.float64))
        vars_.append(np.asarray(v, dtype=np.float64))
    ref_batch = np.asarray(R.dense_logpost(c, X, means, vars_, Cd, n_div=float(n_in))[0], dtype=np.float64)
    np.testing.assert_allclose(log_posterior.log_posterior(X), ref_batch, rtol=1e-8)
    per = np.array([log_posterior.log_posterior(X[i])[0] for i in range(4)])
    np.testing.assert_allclose(per, lp_fn(X[:4]), rtol=1e-8)
    assert not np.allclose(per, _dense_lp_fn(c, Cd - src.T @ src)(X[:4]), rtol=1e-6)
    bad = np.diag(g["y_err"] ** 2)
    bad[0, 12] = bad[12, 0] = 0.01 * g["y_err"][0] * g["y_err"][12]
    log_posterior.initialize_pool_variables(g["lo"], g["hi"], emu_cfg, res, {"y": g["y_exp"], "y_err": g["y_err"],
                                                                            "cov": bad}, None)
    with pytest.raises(ValueError, match="'A' and 'B'"):
        log_posterior.log_posterior(X)


def test_run_mcmc_with_data_covariance_key(tmp_path, monkeypatch):
    """parameters.mcmc.data_covariance: run_mcmc reads the .npz, samples the correlated posterior and writes the usual
    mcmc.h5 schema; the stored log-probabilities are the drop-in's log_posterior with the arrays"""
    from bayesian_inference import emulation, log_posterior, mcmc
    from gpemu import h5io
    g = GU.load("g1_rbf_noise")
    written = {}
    DU.install_fake_data_IO(g["Y"], g["design"], g["y_exp"], g["y_err"], written)
    path, analysis = DU.write_config(tmp_path, n_pc=5, n_restarts=0)
    F = g["y_exp"].shape[0]
    obs = np.zeros(F, dtype=np.int64)
    cov = R.within_cov(g["y_err"], obs)
    src = R.sources(g["y_err"], 2, seed=4)
    np.savez(tmp_path / "dcov.npz", cov=cov, sys_sources=src)
    import os
    assert os.path.dirname(os.path.abspath(path)) == str(tmp_path)
    analysis["parameters"]["mcmc"]["data_covariance"] = "dcov.npz"
    ec = emulation.EmulationConfig.from_config_file("test_analysis", "exponential", path, analysis)
    ec._sort_observables_in_matrix = None
    np.random.seed(1)
    emulation.fit_emulators(ec)
    monkeypatch.setattr(emulation.EmulationConfig, "sort_observables_in_matrix",
                        property(lambda self: DU.TrivialSort("main")))
    monkeypatch.setattr(emulation.EmulationConfig, "observable_filter", property(lambda self: None))
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.data_covariance == str(tmp_path / "dcov.npz")
    mcmc.run_mcmc(cfg)
    out = written[cfg.mcmc_outputfile]
    W, steps, d = cfg.n_walkers, cfg.n_sampling_steps, 6
    assert out["chain"].shape == (steps, W, d) and out["log_prob"].shape == (steps, W)
    assert out["acceptance_fraction"].shape == (W,)
    assert np.all(np.isfinite(out["log_prob"]))
    np.testing.assert_array_equal(log_posterior.experimental_results["cov"], cov)
    np.testing.assert_array_equal(log_posterior.experimental_results["sys_sources"], src)
    lp = np.array([log_posterior.log_posterior(x)[0] for x in out["chain"][-1][:5]])
    np.testing.assert_allclose(lp, out["log_prob"][-1][:5], rtol=1e-10)
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(back) == {"chain", "acceptance_fraction", "log_prob", "autocorrelation_time"}
    np.testing.assert_array_equal(back["chain"], out["chain"])
    np.testing.assert_array_equal(back["log_prob"], out["log_prob"])
