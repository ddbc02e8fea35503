"""-m gpu tests of parallel tempering (gpemu_sampler_create_tempered, gpemu.sampler.TemperedSampler, the drop-in's
n_temperatures): bit equality with the stacked chains where tempering is off, the chain of the CPU reference
(tests/pt_ref.py), the evidence and tempered moments against quadrature, the declines, and the drop-in outputs."""
import ctypes as C
import pickle

import numpy as np
import pytest
from scipy.special import logsumexp

import dropin_util as DU
import golden_util as GU
import pt_ref
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu


def _g1():
    g = GU.load("g1_rbf_noise")
    model = GU.group_model(g)
    dm = GU.device_model(model)
    dm.likelihood_setup(g["y_exp"], g["y_err"], g["lo"], g["hi"], 1.0)

    def oracle_lp(X):
        X = np.atleast_2d(X)
        return np.array([O.log_posterior(x, {"g": model}, g["lo"], g["hi"], g["y_exp"], g["y_err"])[0] for x in X])
    return g, model, dm, oracle_lp


def _starts(g, T, W, seed=40):
    from gpemu import synthetic
    return np.stack([synthetic.make_walkers(W, seed=seed + t, lo=g["lo"], hi=g["hi"]) for t in range(T)])


def _compare_chains(chain, lps, ochain, olps):
    np.testing.assert_allclose(chain, ochain, rtol=1e-12, atol=1e-12)
    fin = np.isfinite(olps)
    assert np.array_equal(fin, np.isfinite(lps))
    np.testing.assert_allclose(lps[fin], olps[fin], rtol=1e-8)


def _rungs_equal_single_chains(g, dm, X0, ts, seeds, steps, check_rungs):
    from gpemu.sampler import DeviceSampler
    T, W = X0.shape[:2]
    ts.set_state(X0)
    lp0 = ts.get_state()[1]
    ts.run(3)
    ts.run(steps - 3)
    chain, lps = ts.get_chain()
    nacc = ts.counts()[0].reshape(T, W)
    for t in check_rungs:
        one = DeviceSampler([dm], W, seed=seeds[t])
        one.set_state(X0[t])
        np.testing.assert_array_equal(one.get_state()[1], lp0[t])
        one.run(steps)
        c1, l1 = one.get_chain()
        np.testing.assert_array_equal(chain[:, t], c1)
        np.testing.assert_array_equal(lps[:, t], l1)
        np.testing.assert_array_equal(nacc[t], one.counts()[0])
        one.close()


@pytest.mark.parametrize("W", [24, 33])
def test_tempering_off_gives_the_stacked_chains(W):
    """betas all 1, no swaps: every rung is, bit for bit, the one-chain sampler with its seed."""
    from gpemu.sampler import TemperedSampler
    g, _, dm, _ = _g1()
    T, steps = 4, 7
    seeds = [101 + 13 * t for t in range(T)]
    ts = TemperedSampler([dm], W, [1.0] * T, seeds=seeds, swap_every=0)
    assert ts.n_temps == T and ts.W == T * W
    _rungs_equal_single_chains(g, dm, _starts(g, T, W), ts, seeds, steps, range(T))
    acc, tried = ts.swap_counts()
    assert not acc.any() and not tried.any()
    ts.close()
    dm.close()


@pytest.mark.parametrize("W", [24, 33])
def test_rung0_untouched_by_hotter_rungs(W):
    from gpemu.sampler import TemperedSampler
    from gpemu.tempering import geometric_ladder
    g, _, dm, _ = _g1()
    T, steps = 5, 8
    ts = TemperedSampler([dm], W, geometric_ladder(T, 50.0), seed=77, swap_every=0)
    seeds = [(77 + t * 0x9E3779B97F4A7C15) % 2 ** 64 for t in range(T)]
    _rungs_equal_single_chains(g, dm, _starts(g, T, W), ts, seeds, steps, [0])
    ts.close()
    dm.close()


@pytest.mark.parametrize("W", [24, 33])
@pytest.mark.parametrize("swap_every", [1, 3])
def test_tempered_chain_equals_host_reference(W, swap_every):
    from gpemu.sampler import TemperedSampler
    g, _, dm, oracle_lp = _g1()
    betas = np.array([1.0, 0.4, 0.1, 0.0])
    T, steps = betas.size, 12
    seeds = [0xC0FFEE12345 + 7 * t for t in range(T)]
    X0 = _starts(g, T, W, seed=3)
    ts = TemperedSampler([dm], W, betas, seeds=seeds, swap_every=swap_every)
    ts.set_state(X0)
    ts.run(steps)
    chain, lps = ts.get_chain()
    nacc = ts.counts()[0].reshape(T, W)
    sacc, stry = ts.swap_counts()
    ochain, olps, onacc, osacc, ostry = pt_ref.run(X0, oracle_lp, betas, seeds, steps, swap_every=swap_every)
    _compare_chains(chain, lps, ochain, olps)
    np.testing.assert_array_equal(nacc, onacc)
    np.testing.assert_array_equal(sacc, osacc)
    np.testing.assert_array_equal(stry, ostry)
    assert stry.sum() == (steps // swap_every) * (T - 1) * W
    np.testing.assert_allclose(ts.tswap_acceptance_fraction, osacc.sum(1) / np.maximum(ostry.sum(1), 1), rtol=1e-15)
    # no walker of any rung leaves the box (the beta = 0 rung proposes outside it all the time)
    lo, hi = np.asarray(g["lo"]), np.asarray(g["hi"])
    assert np.all(chain > lo) and np.all(chain < hi) and np.all(np.isfinite(lps))
    # one rung's walkers alone (a strided copy) are the columns of the whole ladder's chain
    for t in (0, T - 1):
        c_t, l_t = ts.get_chain(temp=t, discard=5)
        np.testing.assert_array_equal(c_t, chain[5:, t])
        np.testing.assert_array_equal(l_t, lps[5:, t])
    # the device mean of the stored log-likelihoods
    np.testing.assert_allclose(ts.mean_log_likelihood(discard=2), olps[2:].mean(axis=(0, 2)), rtol=1e-10)
    # reset clears the swap counters too
    ts.reset()
    assert not any(a.any() for a in ts.swap_counts())
    ts.close()
    dm.close()


def _wide(d=16):
    """a d-parameter model of the path sweep's family, its box and the oracle's log-posterior"""
    import path_cases as PC
    c = PC.Case("wide", 60, d, 3, 64, O.MATERN, 2.5, True)
    model, lo, hi, y_exp, y_err, _, _ = PC.problem(c)
    dm = GU.device_model(model)
    dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0)

    def oracle_lp(X):
        X = np.atleast_2d(X)
        return np.array([O.log_posterior(x, {"g": model}, lo, hi, y_exp, y_err)[0] for x in X])
    return dict(lo=lo, hi=hi), model, dm, oracle_lp


@pytest.mark.parametrize("swap_every", [1, 3])
def test_tempered_chain_equals_host_reference_d16(swap_every):
    """16 parameters, odd W: temper_swap_kernel<16> swaps 16-wide rows of the state and of the stored chain; chain,
    acceptance and swap counts and stored log-probabilities against tests/pt_ref.py"""
    from gpemu.sampler import TemperedSampler
    g, _, dm, oracle_lp = _wide(16)
    betas = np.array([1.0, 0.4, 0.1, 0.0])
    T, W, steps = betas.size, 33, 10
    seeds = [0xBEEF + 7 * t for t in range(T)]
    rng = np.random.default_rng(9)
    lo, hi = g["lo"], g["hi"]
    X0 = rng.uniform(lo + 0.2 * (hi - lo), hi - 0.2 * (hi - lo), (T, W, 16))
    ts = TemperedSampler([dm], W, betas, seeds=seeds, swap_every=swap_every)
    ts.set_state(X0)
    ts.run(steps)
    chain, lps = ts.get_chain()
    nacc = ts.counts()[0].reshape(T, W)
    sacc, stry = ts.swap_counts()
    ochain, olps, onacc, osacc, ostry = pt_ref.run(X0, oracle_lp, betas, seeds, steps, swap_every=swap_every)
    _compare_chains(chain, lps, ochain, olps)
    np.testing.assert_array_equal(nacc, onacc)
    np.testing.assert_array_equal(sacc, osacc)
    np.testing.assert_array_equal(stry, ostry)
    assert stry.sum() == (steps // swap_every) * (T - 1) * W and sacc.sum() > 0
    assert np.all(chain > lo) and np.all(chain < hi) and np.all(np.isfinite(lps))
    ts.close()
    dm.close()


def _model_2d(y_err_scale):
    """A d = 2 emulator from the oracle's pieces (as oracle.workloads.fixed_theta_model, on a 2-D design)."""
    rng = np.random.default_rng(23)
    lo, hi = np.zeros(2), np.ones(2)
    N, F, k = 80, 8, 3
    design = rng.uniform(lo, hi, (N, 2))
    Wm = rng.normal(size=(2, F))
    f = lambda X: np.tanh(X @ Wm)
    Y = f(design) + 0.005 * rng.normal(size=(N, F))
    mean, scale, _ = O.scaler_fit(Y)
    pca = O.pca_fit((Y - mean) / scale)
    spec = O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=False, has_noise=True)
    theta = np.log(np.r_[0.5, 0.5, 0.01])
    gps = [O.gp_fit_at_theta(design, pca["Y_pca"][:, i], theta, spec, 1e-10) for i in range(k)]
    model = O.GroupModel(X_train=design, spec=spec, gps=gps, components=pca["components"],
                         explained_variance=pca["explained_variance"], scaler_mean=mean, scaler_scale=scale, n_pc=k)
    y_exp = f(np.array([[0.4, 0.6]]))[0]
    y_err = np.full(F, y_err_scale)
    return model, lo, hi, y_exp, y_err


def test_evidence_and_tempered_moments_against_quadrature():
    from gpemu.sampler import TemperedSampler
    from gpemu.tempering import geometric_ladder
    model, lo, hi, y_exp, y_err = _model_2d(0.15)
    dm = GU.device_model(model)
    dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0)
    n = 1024
    g1 = lo[0] + (np.arange(n) + 0.5) / n * (hi[0] - lo[0])
    g2 = lo[1] + (np.arange(n) + 0.5) / n * (hi[1] - lo[1])
    grid = np.stack(np.meshgrid(g1, g2, indexing="ij"), axis=-1).reshape(-1, 2)
    ll = np.concatenate([dm.logpost(grid[i:i + 65536]) for i in range(0, grid.shape[0], 65536)])
    assert np.all(np.isfinite(ll))
    log_z_grid = logsumexp(ll) - np.log(ll.size)
    post = np.exp(ll - logsumexp(ll))
    sd = np.sqrt(post @ (grid - post @ grid) ** 2)
    assert np.all(sd < 0.25 * (hi - lo)), sd                 # the posterior is clearly narrower than the box

    betas = geometric_ladder(25, 100.0, prior_rung=True)
    T, Wc, discard, steps = betas.size, 256, 1000, 3000
    ts = TemperedSampler([dm], Wc, betas, seed=2024, swap_every=1)
    rng = np.random.default_rng(8)
    ts.set_state(rng.uniform(lo, hi, (T * Wc, 2)))
    ts.run(discard + steps)
    log_z, dlog_z = ts.log_evidence_estimate(discard=discard)
    print(f"logZ {log_z:.5f} +- {dlog_z:.5f}, grid {log_z_grid:.5f}, swap acceptance "
          f"{np.array2string(ts.tswap_acceptance_fraction, precision=3)}")
    assert dlog_z < 0.2
    assert abs(log_z - log_z_grid) <= 3 * dlog_z + 0.05
    chain, _ = ts.get_chain(discard=discard)
    width = hi - lo
    worst = 0.0
    for t, b in enumerate(betas):
        w = np.exp(b * ll - logsumexp(b * ll))
        mean_grid = w @ grid
        mean_chain = chain[:, t].reshape(-1, 2).mean(axis=0)
        worst = max(worst, float(np.max(np.abs(mean_chain - mean_grid) / width)))
        assert np.all(np.abs(mean_chain - mean_grid) <= 0.02 * width), (t, mean_chain, mean_grid)
    var_prior = chain[:, -1].reshape(-1, 2).var(axis=0)
    print(f"worst rung-mean offset {worst:.4f} box widths; prior-rung variance / (width^2/12) "
          f"{np.array2string(var_prior / (width ** 2 / 12), precision=4)}")
    np.testing.assert_allclose(var_prior, width ** 2 / 12, rtol=0.05)
    ts.close()
    dm.close()


def test_tempered_sampler_declines_the_other_paths():
    from gpemu import _lib
    from gpemu.sampler import DeviceSampler, TemperedSampler
    g, _, dm, _ = _g1()
    ts = TemperedSampler([dm], 24, [1.0, 0.5, 0.0], seed=5)
    ts.set_state(_starts(g, 3, 24))
    L = _lib.lib()
    UNSUPPORTED = -5
    assert L.gpemu_sampler_run_sharded(ts._h, None, 1, 1, 0) == UNSUPPORTED
    assert "tempered" in _lib.last_error()
    assert L.gpemu_sampler_run_sharded(ts._h, None, 1, 1, 2) == UNSUPPORTED
    buf = (C.c_char * 64)()
    assert L.gpemu_sampler_peer_export(ts._h, C.cast(buf, C.c_void_p)) == UNSUPPORTED
    assert "tempered" in _lib.last_error()
    assert L.gpemu_sampler_run_peer(ts._h, 1, 1) == UNSUPPORTED
    W = ts.W
    inds = np.array([0, 1] * (W // 2), dtype=np.int32)
    zz = np.ones(W)
    rint = np.zeros(W, dtype=np.int64)
    logu = np.zeros(W)
    assert L.gpemu_sampler_step_host_rng(ts._h, _lib.ptr(inds), _lib.ptr(zz), _lib.ptr(rint), _lib.ptr(logu), 1) \
        == UNSUPPORTED
    with pytest.raises(_lib.GpemuError, match="tempered"):
        ts.run_emulated(1, 2)
    # the state is untouched by the declined calls
    assert ts.counts()[1:] == (0, 0)
    ts.close()
    # bad ladders
    for bad in ([0.9, 0.5], [1.0, 0.5, 0.7], [1.0, -0.1], [1.0]):
        with pytest.raises(_lib.GpemuError):
            TemperedSampler([dm], 24, bad, seed=5)
    # several data vectors: rejected
    ys = np.stack([g["y_exp"], g["y_exp"] + 0.01])
    dm.likelihood_setup(ys, g["y_err"], g["lo"], g["hi"], 1.0)
    with pytest.raises(_lib.GpemuError, match="data vectors"):
        TemperedSampler([dm], 24, [1.0, 0.5], seed=5)
    DeviceSampler([dm], 24, seeds=[1, 2]).close()       # (the stacked sampler still takes them)
    dm.close()


def test_run_mcmc_tempered_end_to_end(tmp_path, monkeypatch):
    from bayesian_inference import emulation, log_posterior, mcmc
    from gpemu import h5io
    g = GU.load("g1_rbf_noise")
    written = {}
    DU.install_fake_data_IO(g["Y"], g["design"], g["y_exp"], g["y_err"], written)
    path, analysis = DU.write_config(tmp_path, n_pc=5, n_restarts=0)
    analysis["parameters"]["mcmc"]["n_temperatures"] = 4
    ec = emulation.EmulationConfig.from_config_file("test_analysis", "exponential", path, analysis)
    ec._sort_observables_in_matrix = None
    np.random.seed(1)
    emulation.fit_emulators(ec)
    monkeypatch.setattr(emulation.EmulationConfig, "sort_observables_in_matrix",
                        property(lambda self: DU.TrivialSort("main")))
    monkeypatch.setattr(emulation.EmulationConfig, "observable_filter", property(lambda self: None))
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.n_temperatures == 4 and cfg.t_max == 1e5 and cfg.swap_every == 1 and cfg.prior_rung
    mcmc.run_mcmc(cfg)
    out = written[cfg.mcmc_outputfile]
    W, steps, d = cfg.n_walkers, cfg.n_sampling_steps, 6
    assert out["chain"].shape == (steps, W, d) and out["log_prob"].shape == (steps, W)
    assert out["acceptance_fraction"].shape == (W,)
    new = {"betas", "log_evidence", "log_evidence_error", "mean_log_likelihood", "temperature_swap_acceptance_fraction"}
    assert set(out) == {"chain", "acceptance_fraction", "log_prob", "autocorrelation_time"} | new
    assert out["betas"].shape == (4,) and out["betas"][0] == 1.0 and out["betas"][-1] == 0.0
    assert out["mean_log_likelihood"].shape == (4,) and out["temperature_swap_acceptance_fraction"].shape == (3,)
    assert np.isfinite(out["log_evidence"]) and np.isfinite(out["log_evidence_error"])
    lo, hi = np.array(g["lo"]), np.array(g["hi"])
    assert np.all(out["chain"] > lo) and np.all(out["chain"] < hi) and np.all(np.isfinite(out["log_prob"]))
    lp = np.array([log_posterior.log_posterior(x)[0] for x in out["chain"][-1][:5]])
    np.testing.assert_allclose(lp, out["log_prob"][-1][:5], rtol=1e-10)
    sampler = pickle.loads(pickle.dumps(pickle.load(open(cfg.sampler_outputfile, "rb"))))
    np.testing.assert_array_equal(sampler.get_chain(), out["chain"])
    np.testing.assert_array_equal(sampler.get_log_prob(), out["log_prob"])
    np.testing.assert_array_equal(sampler.acceptance_fraction, out["acceptance_fraction"])
    np.testing.assert_array_equal(sampler.betas, out["betas"])
    assert sampler.log_evidence == out["log_evidence"]
    try:
        sampler.get_autocorr_time(quiet=True)
    except Exception as err:          # a 12-step chain: too short (or 0 / 0) is the expected answer
        assert "chain" in str(err).lower() or "autocorr" in type(err).__name__.lower()
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert new <= set(back)
    np.testing.assert_array_equal(back["chain"], out["chain"])
    np.testing.assert_array_equal(back["betas"], out["betas"])


def test_prior_rung_walker_outside_the_box_moves_in():
    """A walker that starts outside the open box (ll = -inf) on the beta = 0 rung takes its first finite proposal, as it
    would on any rung with beta > 0 (no 0 * inf); the chain still equals the reference's."""
    from gpemu.sampler import TemperedSampler
    g, _, dm, oracle_lp = _g1()
    betas = np.array([1.0, 0.3, 0.0])
    T, W, steps = betas.size, 24, 12
    seeds = [91 + t for t in range(T)]
    lo, hi = np.asarray(g["lo"]), np.asarray(g["hi"])
    X0 = _starts(g, T, W, seed=9)
    X0[-1, 0, 0] = lo[0] - 0.1 * (hi[0] - lo[0])             # prior rung, walker 0: outside the box
    X0[1, 3, 1] = hi[1] + 0.05 * (hi[1] - lo[1])             # and one on a beta > 0 rung
    ts = TemperedSampler([dm], W, betas, seeds=seeds, swap_every=1)
    ts.set_state(X0)
    assert ts.get_state()[1][-1, 0] == -np.inf and ts.get_state()[1][1, 3] == -np.inf
    ts.run(steps)
    chain, lps = ts.get_chain()
    ochain, olps, onacc, osacc, ostry = pt_ref.run(X0, oracle_lp, betas, seeds, steps, swap_every=1)
    _compare_chains(chain, lps, ochain, olps)
    np.testing.assert_array_equal(ts.counts()[0].reshape(T, W), onacc)
    np.testing.assert_array_equal(ts.swap_counts()[0], osacc)
    assert onacc[-1, 0] >= 1                     # (0 * inf would have rejected every proposal)
    assert np.all(chain[-1, -1] > lo) and np.all(chain[-1, -1] < hi) and np.all(np.isfinite(lps[-1, -1]))
    assert np.isfinite(ts.mean_log_likelihood(discard=steps - 1)[-1])
    ts.close()
    dm.close()


def test_phase_api_on_one_rank_equals_host_reference():
    """The per-phase calls (begin_step / half_propose_eval / half_accept / end_step) on a tempered sampler: the
    beta-aware accept_kernel and the swap pass in end_step give the reference's chain."""
    import torch
    from gpemu import _lib
    from gpemu.sampler import TemperedSampler
    g, _, dm, oracle_lp = _g1()
    betas = np.array([1.0, 0.4, 0.0])
    T, W, steps = betas.size, 33, 6
    seeds = [501 + 3 * t for t in range(T)]
    X0 = _starts(g, T, W, seed=12)
    ts = TemperedSampler([dm], W, betas, seeds=seeds, swap_every=2)
    ts.set_state(X0)
    L = _lib.lib()
    dev = torch.device("cuda", ts.device)
    buf = [torch.zeros(ts.ns[h], dtype=torch.float64, device=dev) for h in (0, 1)]
    torch.cuda.synchronize(dev)
    _lib.check(L.gpemu_sampler_reserve_chain(ts._h, steps))
    for _ in range(steps):
        _lib.check(L.gpemu_sampler_begin_step(ts._h))
        for h in (0, 1):
            _lib.check(L.gpemu_sampler_half_propose_eval(ts._h, h, 0, ts.ns[h], C.c_void_p(buf[h].data_ptr())))
            _lib.check(L.gpemu_sampler_half_accept(ts._h, h, C.c_void_p(buf[h].data_ptr()), 1))
        _lib.check(L.gpemu_sampler_end_step(ts._h, 1))
    assert L.gpemu_sampler_check(ts._h) == 0
    chain, lps = ts.get_chain()
    ochain, olps, onacc, osacc, ostry = pt_ref.run(X0, oracle_lp, betas, seeds, steps, swap_every=2)
    _compare_chains(chain, lps, ochain, olps)
    np.testing.assert_array_equal(ts.counts()[0].reshape(T, W), onacc)
    np.testing.assert_array_equal(ts.swap_counts()[0], osacc)
    np.testing.assert_array_equal(ts.swap_counts()[1], ostry)
    ts.close()
    dm.close()


def test_snapshot_restore_covers_the_swap_counters():
    """A block rerun after gpemu_sampler_restore gives the state, chain and counters -- swap counters included -- of an
    unbroken run."""
    from gpemu import _lib
    from gpemu.sampler import TemperedSampler
    g, _, dm, _ = _g1()
    betas = [1.0, 0.5, 0.1, 0.0]
    W = 24
    X0 = _starts(g, len(betas), W, seed=21)
    a = TemperedSampler([dm], W, betas, seed=8, swap_every=1)
    b = TemperedSampler([dm], W, betas, seed=8, swap_every=1)
    a.set_state(X0)
    b.set_state(X0)
    a.run(9)
    b.run(4)
    _lib.check(_lib.lib().gpemu_sampler_snapshot(b._h))
    b.run(5)
    assert b.swap_counts()[1].sum() == 9 * (len(betas) - 1) * W
    _lib.check(_lib.lib().gpemu_sampler_restore(b._h))
    b.run(5)
    for x, y in zip(a.swap_counts(), b.swap_counts()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a.counts()[0], b.counts()[0])
    np.testing.assert_array_equal(a.get_chain()[0], b.get_chain()[0])
    np.testing.assert_array_equal(a.get_state()[1], b.get_state()[1])
    with pytest.raises(_lib.GpemuError, match="one GPU"):
        a.run_sharded(1)
    a.close()
    b.close()
    dm.close()
