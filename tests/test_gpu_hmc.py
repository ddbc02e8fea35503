"""-m gpu tests of the device HMC sampler (csrc/k_hmc.hip) against tests/hmc_ref.py: trajectories
through the host-RNG step and through the device's own random stream, determinism and chain independence, the
step-size adaptation, the chain moments, the sampled distribution, the declines and the drop-in route.

Tolerance of the trajectory comparisons.  hmc_ref reruns every case with each gradient component moved by +-grad_bound
(grad_ref's a-priori bound of the device's gradient) under 8 sign patterns; per iteration, the device's positions must
stay within 4 x the largest deviation those runs show from the unperturbed one, in units of the box width.  The
device's gradients sit at <= 0.0013 of the bound, and the 4 covers sign patterns not drawn.
tests/test_hmc_host.py asserts that no accept or divergence decision of any case is within 1e-6 of its threshold and
that no perturbed run decides differently, so the device's decisions must be the reference's."""
from __future__ import annotations

import numpy as np
import pytest

import dropin_util as DU
import golden_util as GU
import hmc_ref as R
import path_cases as PC
from gpemu import _lib
from gpemu import model as M
from gpemu.sampler import DeviceSampler, HMCSampler, integrated_time

pytestmark = pytest.mark.gpu

HMC_PATHS = ["BEGIN", "BEGIN_HOST_RNG", "LEAPFROG", "FINISH", "ADAPT", "ACCEPT_MEAN", "MOMENTS"]
HP = {n: i for i, n in enumerate(HMC_PATHS)}


def hmc_counts():
    c = M.hmc_path_counts()
    assert len(c) == len(HMC_PATHS), "enum gpemu_hmc_path and HMC_PATHS disagree"
    return c


def device_groups(name):
    pr = R.trajectory_problem(name)
    dms = []
    for model, y_exp, y_err, bs in pr["groups"]:
        dm = GU.device_model(model)
        dm.likelihood_setup(y_exp, y_err, pr["lo"], pr["hi"], 1.0, block_start=bs)
        dms.append(dm)
    return dms, pr["lo"], pr["hi"]


def case_model(name, y_err_scale=1.0):
    c = [x for x in PC.cases() if x.name == name][0]
    model, lo, hi, y_exp, y_err, bs, rng = PC.problem(c)
    dm = GU.device_model(model)
    dm.likelihood_setup(y_exp, y_err * y_err_scale, lo, hi, 1.0, block_start=bs)
    return dm, lo, hi, rng


def check_against_reference(what, name, W, sampler, lo, hi):
    """chain, accept and divergence counts of the sampler's N_ITER stored iterations against the reference run"""
    run = R.reference_run(name)
    chain, lp = sampler.get_chain()
    assert chain.shape == (R.N_ITER, W, lo.size)
    tol = R.tolerance(run, W)
    err = np.max(np.abs(chain - run["chain"][:, :W]) / (hi - lo), axis=(1, 2))
    st = sampler.stats()
    print(f"\nHMC {what} {name} W={W}: deviation of the perturbed reference runs per iteration {tol / R.TOL_FACTOR}, device "
          f"error {err}, largest error / tolerance {np.max(err / np.maximum(tol, 1e-300)):.3g}; accepts "
          f"{int(st['accepted'].sum())} of {W * R.N_ITER}, divergences {int(st['divergences'].sum())}")
    assert np.array_equal(st["accepted"], run["accept"][:, :W].sum(axis=0)), "accepts per chain"
    assert np.array_equal(st["divergences"], run["divergent"][:, :W].sum(axis=0)), "divergences per chain"
    assert np.all(err <= tol), (err, tol)
    assert np.all((chain > lo) & (chain < hi)), "every stored point lies strictly inside the box"
    assert np.all(np.isfinite(lp))
    # the stored log-probabilities are those of the stored points: where a chain moved, lp changed with it
    moved = np.any(chain[1:] != chain[:-1], axis=2)
    assert np.array_equal(moved, run["accept"][1:, :W]) and np.array_equal(lp[1:] != lp[:-1], moved)
    nacc, it, cl = sampler.counts()
    assert it == R.N_ITER and cl == R.N_ITER and np.array_equal(nacc, st["accepted"])


# ---- 1. trajectories through the host-RNG step ----------------------------------------------------------------------
@pytest.mark.parametrize("W", [24, R.W_MAX])
@pytest.mark.parametrize("name", list(R.TRAJECTORY_CASES))
def test_trajectory_against_the_reference(name, W):
    dms, lo, hi = device_groups(name)
    cs = R.TRAJECTORY_CASES[name]
    s = HMCSampler(dms, W, n_leapfrog=R.N_LEAPFROG, step_size=cs["eps"], jitter=R.JITTER, seed=cs["seed"])
    assert np.array_equal(s.inverse_metric, (hi - lo) ** 2 / 12.0)
    s.set_state(R.trajectory_start(name)[:W])
    c0 = hmc_counts()
    for it in range(R.N_ITER):
        p0, logu, eps_w = R.trajectory_draws(name, it)
        s.step_host_rng(p0[:W], logu[:W], eps_w[:W])
    dc = hmc_counts() - c0
    assert dc[HP["BEGIN_HOST_RNG"]] == R.N_ITER and dc[HP["BEGIN"]] == 0 and dc[HP["FINISH"]] == R.N_ITER
    assert dc[HP["LEAPFROG"]] == R.N_ITER * (R.N_LEAPFROG - 1) and dc[HP["ACCEPT_MEAN"]] == R.N_ITER
    check_against_reference("host rng", name, W, s, lo, hi)
    s.close()
    for dm in dms:
        dm.close()


# ---- 2. the device's random stream ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n16_d7_m15_const", "n17_d1_m25"])
def test_device_random_stream(name):
    """``run`` draws what hmc_ref draws: the uniforms bit for bit, the normals within 4 ulp of their pair's radius (log,
    sqrt, sincos differ in last bits between the libraries), the chain within the tolerance of the trajectory test"""
    dms, lo, hi = device_groups(name)
    cs = R.TRAJECTORY_CASES[name]
    W, d = R.W_MAX, lo.size
    s = HMCSampler(dms, W, n_leapfrog=R.N_LEAPFROG, step_size=cs["eps"], jitter=R.JITTER, seed=cs["seed"])
    worst = 0.0
    for step in (0, 5, 2 ** 32 + 3):
        z, ua, uj = s.draws(step)
        zr, uar, ujr = R.draws(W, d, cs["seed"], step)
        assert np.array_equal(ua, uar) and np.array_equal(uj, ujr)
        zp = R.draws(W, d + d % 2, cs["seed"], step)[0].reshape(W, -1, 2)       # whole pairs, also for an odd d
        assert np.array_equal(zp.reshape(W, -1)[:, :d], zr)
        rad = np.repeat(np.sqrt(np.sum(zp * zp, axis=2)), 2, axis=1)[:, :d]
        ratio = np.abs(z - zr) / np.spacing(rad)
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 4.0), ratio.max()
    print(f"\nHMC normals {name}: largest |z_dev - z_ref| = {worst:.3g} ulp of the pair's radius")
    s.set_state(R.trajectory_start(name))
    c0 = hmc_counts()
    s.run(R.N_ITER)
    dc = hmc_counts() - c0
    assert dc[HP["BEGIN"]] == R.N_ITER and dc[HP["BEGIN_HOST_RNG"]] == 0
    check_against_reference("device rng", name, W, s, lo, hi)
    s.close()
    for dm in dms:
        dm.close()


# ---- 3. independence and determinism ----------------------------------------------------------------------------------
def test_determinism_chain_independence_and_snapshot():
    dm, lo, hi, rng = case_model("n16_d7_m15_const")
    X0 = rng.uniform(lo, hi, (1030, lo.size))

    def run(W, steps=4):
        s = HMCSampler([dm], W, n_leapfrog=3, step_size=0.3, seed=77)
        s.set_state(X0[:W])
        s.run(steps)
        out = s.get_chain() + (s.stats(),)
        s.close()
        return out
    a, b = run(24), run(24)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "the same seed twice"
    assert np.any(a[0][-1] != X0[:24]), "the chains moved"
    big = run(1030)                       # crosses the gradient's 1024-row pass
    assert np.array_equal(big[0][:, :24], a[0]) and np.array_equal(big[1][:, :24], a[1]), "chains 0..23 of 1030"
    assert np.array_equal(big[2]["accepted"][:24], a[2]["accepted"])
    assert np.any(big[0][-1, 1024:] != X0[1024:]), "the chains of the second pass moved as well"
    # snapshot, run, restore, run: the block again
    s = HMCSampler([dm], 33, n_leapfrog=3, step_size=0.3, seed=5)
    s.set_state(X0[:33])
    s.run(2)
    _lib.check(_lib.lib().gpemu_sampler_snapshot(s._h))
    s.run(3)
    first = s.get_chain() + (s.get_state(), s.stats())
    _lib.check(_lib.lib().gpemu_sampler_restore(s._h))
    assert s.counts()[2] == 2
    s.run(3)
    again = s.get_chain() + (s.get_state(), s.stats())
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    assert np.array_equal(first[2][0], again[2][0]) and np.array_equal(first[2][1], again[2][1])
    assert np.array_equal(first[3]["accepted"], again[3]["accepted"]) and np.array_equal(first[3]["divergences"], again[3]["divergences"])
    s.close()
    dm.close()


# ---- 4. adaptation and chain moments --------------------------------------------------------------------------------
def test_step_size_adaptation_equals_dual_averaging_of_the_devices_accept_probabilities():
    dm, lo, hi, rng = case_model("n16_d7_m15_const")
    W, eps0, target = 48, 0.6, 0.8
    s = HMCSampler([dm], W, n_leapfrog=3, step_size=eps0, seed=9)
    s.set_state(rng.uniform(lo, hi, (W, lo.size)))
    s.adapt(True, target)
    c0 = hmc_counts()
    alphas, eps = [], []
    for _ in range(20):
        s.run(1, store=False)
        alphas.append(s.stats()["last_accept_prob"])
        eps.append(s.step_size)
    dc = hmc_counts() - c0
    assert dc[HP["ADAPT"]] == 20 and dc[HP["ACCEPT_MEAN"]] == 0
    ref, eps_bar = R.dual_averaging(eps0, alphas, target)
    print(f"\nHMC adaptation: accept probabilities {np.round(alphas, 3)}, step sizes {np.round(eps, 4)}")
    assert np.allclose(eps, ref, rtol=1e-12, atol=0), np.max(np.abs(np.array(eps) / ref - 1))
    assert len(set(eps)) == 20 and 0 < min(alphas) and max(alphas) <= 1
    assert abs(s.stats()["mean_accept_prob"] - np.mean(alphas)) <= 1e-13
    s.adapt(False)
    assert abs(s.step_size / eps_bar - 1) <= 1e-12, "the step size freezes at the averaged one"
    s.run(2, store=False)
    assert abs(s.step_size / eps_bar - 1) <= 1e-12
    s.close()
    dm.close()


def _moments_equal(sampler, discard, n):
    chain = sampler.get_chain()[0]
    x = chain[discard:discard + n].reshape(-1, chain.shape[2])
    c0 = hmc_counts()
    mean, var = sampler.chain_moments(discard=discard, n=n)
    assert (hmc_counts() - c0)[HP["MOMENTS"]] == 1
    # a sum's rounding error scales with its summands, not with the result: the mean is held to 1e-12 of the larger of
    # |mean| and the standard deviation
    assert np.all(np.abs(mean - x.mean(axis=0)) <= 1e-12 * np.maximum(np.abs(x.mean(axis=0)), x.std(axis=0)))
    assert np.allclose(var, x.var(axis=0), rtol=1e-12, atol=0)
    assert np.all(var > 0)


def test_chain_moments_equal_numpy_for_an_hmc_chain_and_a_stretch_chain():
    dm, lo, hi, rng = case_model("n16_d7_m15_const")
    s = HMCSampler([dm], 37, n_leapfrog=2, step_size=0.3, seed=3)
    s.set_state(rng.uniform(lo, hi, (37, lo.size)))
    s.run(60)                                   # 2220 rows: three blocks of the partial sums, the last one short
    _moments_equal(s, 0, 60)
    _moments_equal(s, 7, 1)
    _moments_equal(s, 11, 30)
    with pytest.raises(_lib.GpemuError):
        s.chain_moments(discard=50, n=20)
    s.close()
    st = DeviceSampler([dm], 40, seed=4)
    st.set_state(rng.uniform(lo, hi, (40, lo.size)))
    st.run(30)
    _moments_equal(st, 0, 30)
    _moments_equal(st, 5, 20)
    st.close()
    dm.close()


# ---- 5. the sampled distribution ------------------------------------------------------------------------------------
def _quadrature(dm, lo, hi, n):
    """mean and variance per parameter (d = 2) by the midpoint rule on an n x n grid of the value path's logpost, and
    the largest ratio of a marginal's density in a cell at a face to its maximum"""
    g = [lo[j] + (np.arange(n) + 0.5) / n * (hi[j] - lo[j]) for j in range(2)]
    X = np.stack(np.meshgrid(*g, indexing="ij"), axis=-1).reshape(-1, 2)
    lp = dm.logpost(X)
    w = np.exp(lp - lp.max())
    w /= w.sum()
    mu = w @ X
    var = w @ (X - mu) ** 2
    w2 = w.reshape(n, n)
    lean = max(max(m[0], m[-1]) / m.max() for m in (w2.sum(axis=1), w2.sum(axis=0)))
    return mu, var, lean


@pytest.mark.parametrize("y_err_scale", [1.0, 3.0])
def test_samples_the_posterior(y_err_scale):
    """W = 256 independent chains, 100 warm-up + 300 iterations, against quadrature of the value path: mean and
    variance within 5 standard errors, taken from the spread over the chains (of the chain means; of the chains' mean
    squared distance from the quadrature's mean), which must themselves be below 10 % of the posterior's standard
    deviation (variance): noise cannot pass.  y_err x 3 presses the posterior against two faces of the box."""
    dm, lo, hi, rng = case_model("n100_b2049_two_passes", y_err_scale)
    W = 256
    mu, var, lean = _quadrature(dm, lo, hi, 400)
    mu2, var2, _ = _quadrature(dm, lo, hi, 200)
    if y_err_scale > 1.0:
        assert lean > 0.9, "the posterior must lean on a face"
    s = HMCSampler([dm], W, n_leapfrog=8, step_size=0.2, seed=21)
    s.set_state(rng.uniform(lo, hi, (W, 2)))
    warm = s.warmup(100)
    assert s.counts()[1:] == (0, 0), "the warm-up's chain and counters are dropped"
    eps, minv = s.step_size, s.inverse_metric
    assert eps == warm["step_size"] and np.array_equal(minv, warm["inverse_metric"])
    s.run(300)
    assert s.step_size == eps and np.array_equal(s.inverse_metric, minv), "production runs with both fixed"
    chain, _ = s.get_chain()
    assert np.all((chain > lo) & (chain < hi))
    means = chain.mean(axis=0)                                  # [W, 2]
    m2 = ((chain - mu) ** 2).mean(axis=0)
    se_mean = means.std(axis=0, ddof=1) / np.sqrt(W)
    se_var = m2.std(axis=0, ddof=1) / np.sqrt(W)
    st = s.stats()
    print(f"\nHMC distribution y_err x {y_err_scale}: quadrature mean {mu} var {var} (lean {lean:.3g}); chains mean "
          f"{means.mean(axis=0)} +- {se_mean}, var {m2.mean(axis=0)} +- {se_var}; step size {eps:.4g}, inverse metric {minv}, "
          f"accept probability {st['mean_accept_prob']:.3f}, acceptance {s.acceptance_fraction.mean():.3f}, divergences "
          f"{int(st['divergences'].sum())}, warm-up divergences {warm['divergences']}")
    assert np.all(np.abs(mu - mu2) < 0.2 * se_mean) and np.all(np.abs(var - var2) < 0.2 * se_var), "the quadrature has converged"
    assert np.all(se_mean < 0.1 * np.sqrt(var)) and np.all(se_var < 0.1 * var)
    assert np.all(np.abs(means.mean(axis=0) - mu) <= 5 * se_mean), (means.mean(axis=0), mu, se_mean)
    assert np.all(np.abs(m2.mean(axis=0) - var) <= 5 * se_var), (m2.mean(axis=0), var, se_var)
    assert 0.5 < st["mean_accept_prob"] < 0.99
    # the device's pooled moments are those of the chain
    dmean, dvar = s.chain_moments()
    assert np.allclose(dmean, chain.reshape(-1, 2).mean(axis=0), rtol=1e-12) and np.allclose(dvar, chain.reshape(-1, 2).var(axis=0), rtol=1e-12)
    s.close()
    dm.close()


# ---- 6. declines ------------------------------------------------------------------------------------------------------
def _refused(call, word=None):
    c0, g0 = hmc_counts(), M.grad_path_counts()
    with pytest.raises(_lib.GpemuError) as ei:
        call()
    assert ei.value.code == -5, ei.value
    assert np.array_equal(hmc_counts(), c0) and np.array_equal(M.grad_path_counts(), g0), "a refused call must not launch"
    if word:
        assert word in str(ei.value), ei.value
    return str(ei.value)


def test_declines_at_create_before_any_launch():
    by_name = {c.name: c for c in PC.cases()}
    for name, word in (("n15_d8_ksteps3_m05", "nu = 0.5"), ("n63_nu075_direct", "nu = 0.75")):
        c = by_name[name]
        model, lo, hi, y_exp, y_err, bs, rng = PC.problem(c)
        dm = GU.device_model(model)
        dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0, block_start=bs)
        X = rng.uniform(lo, hi, (5, c.d))
        before = dm.logpost(X)
        _refused(lambda: HMCSampler([dm], 8), word)
        assert np.array_equal(dm.logpost(X), before), "logpost after a refused create"
        DeviceSampler([dm], 8).close()            # the stretch sampler takes the model as ever
        dm.close()
    c = by_name["n300_tasks_multi"]
    model, lo, hi, y_exp, y_err, bs, rng = PC.problem(c)
    dm = GU.device_model(model)
    X = rng.uniform(lo, hi, (5, c.d))
    dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0, block_start=bs, sys_sources=0.05 * np.ones((1, len(y_exp))))
    before = M.logpost_groups([dm], X)
    _refused(lambda: HMCSampler([dm], 8), "sources")
    assert np.array_equal(M.logpost_groups([dm], X), before)
    dm.likelihood_setup(np.stack([y_exp, y_exp + 0.01]), y_err, lo, hi, 1.0, block_start=bs)
    _refused(lambda: HMCSampler([dm], 8), "data vectors")
    dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0, block_start=bs)
    before = dm.logpost(X)
    for bad in (dict(n_leapfrog=0), dict(step_size=0.0), dict(step_size=np.nan), dict(jitter=1.0)):
        with pytest.raises(_lib.GpemuError) as ei:
            HMCSampler([dm], 8, **bad)
        assert ei.value.code == -1
    s = HMCSampler([dm], 8, n_leapfrog=2, step_size=0.1, seed=1)      # a single data vector again: it runs
    s.set_state(rng.uniform(lo, hi, (8, c.d)))
    s.run(2)
    assert s.counts()[2] == 2
    s.close()
    assert np.array_equal(dm.logpost(X), before)
    dm.close()


def test_declines_on_an_hmc_sampler():
    import ctypes as C
    dm, lo, hi, rng = case_model("n16_d7_m15_const")
    W, d = 12, lo.size
    s = HMCSampler([dm], W, n_leapfrog=2, step_size=0.2, seed=2)
    X0 = rng.uniform(lo, hi, (W, d))
    s.set_state(X0)
    X = rng.uniform(lo, hi, (5, d))
    before = dm.logpost(X)
    L, h = _lib.lib(), s._h
    buf = np.zeros(2 * W)
    ints = np.zeros(2 * W, dtype=np.int64)
    hb = C.create_string_buffer(128)
    calls = {
        "run_sharded": lambda: L.gpemu_sampler_run_sharded(h, None, 1, 1, 0),
        "run_sharded (emulated)": lambda: L.gpemu_sampler_run_sharded(h, None, 1, 1, 2),
        "run_peer": lambda: L.gpemu_sampler_run_peer(h, 1, 1),
        "peer_export": lambda: L.gpemu_sampler_peer_export(h, C.cast(hb, C.c_void_p)),
        "peer_import": lambda: L.gpemu_sampler_peer_import(h, 1, 0, C.cast(hb, C.c_void_p)),
        "begin_step": lambda: L.gpemu_sampler_begin_step(h),
        "half_propose_eval": lambda: L.gpemu_sampler_half_propose_eval(h, 0, 0, 1, _lib.ptr(buf)),
        "half_accept": lambda: L.gpemu_sampler_half_accept(h, 0, _lib.ptr(buf), 1),
        "end_step": lambda: L.gpemu_sampler_end_step(h, 1),
        "step_host_rng": lambda: L.gpemu_sampler_step_host_rng(h, _lib.ptr(np.zeros(W, dtype=np.int32)), _lib.ptr(buf),
                                                               _lib.ptr(ints), _lib.ptr(buf), 1),
        "set_betas": lambda: L.gpemu_sampler_set_betas(h, _lib.ptr(np.ones(1))),
        "get_swap_counts": lambda: L.gpemu_sampler_get_swap_counts(h, _lib.ptr(ints), _lib.ptr(ints)),
        "mean_loglik": lambda: L.gpemu_sampler_mean_loglik(h, 0, 1, _lib.ptr(buf)),
    }
    for what, call in calls.items():
        _refused(lambda: _lib.check(call()), "HMC")
    _refused(lambda: s.run_sharded(1))
    # and the HMC calls on a stretch sampler: a state error, no launch
    st = DeviceSampler([dm], W, seed=1)
    for call in (lambda: L.gpemu_sampler_hmc_adapt(st._h, 1, 0.8), lambda: L.gpemu_sampler_hmc_set_step_size(st._h, 0.1),
                 lambda: L.gpemu_sampler_hmc_stats(st._h, None, None, None, None)):
        assert call() == -4
    st.close()
    lp0 = s.get_state()[1]
    assert np.array_equal(s.get_state()[0], X0) and np.array_equal(dm.logpost(X), before)
    s.run(3)                                                         # the sampler is as it was: it runs
    assert s.counts()[2] == 3 and np.array_equal(np.isfinite(lp0), np.ones(W, bool))
    s.close()
    dm.close()


def test_set_state_and_reset():
    """set_state takes lp from the gradient path (logp0 is not read); reset drops the chain and the counters"""
    dm, lo, hi, rng = case_model("n16_d7_m15_const")
    W, d = 16, lo.size
    s = HMCSampler([dm], W, n_leapfrog=3, step_size=0.3, seed=8)
    X0 = rng.uniform(lo, hi, (W, d))
    s.set_state(X0, logp0=np.full(W, 123.0))
    X, lp = s.get_state()
    lp_grad, _ = dm.logpost_grad(X0)
    assert np.array_equal(X, X0) and np.array_equal(lp, lp_grad)
    s.run(5)
    assert s.counts()[1:] == (5, 5)
    s.reset()
    st = s.stats()
    assert s.counts()[1:] == (0, 0) and not st["accepted"].any() and not st["divergences"].any() and st["mean_accept_prob"] == 0
    s.run(2, store=False)
    assert s.counts()[1:] == (2, 0)
    s.close()
    dm.close()


# ---- 7. the drop-in route ---------------------------------------------------------------------------------------------
USUAL = {"chain", "acceptance_fraction", "log_prob", "autocorrelation_time"}
HMC_KEYS = {"hmc_step_size", "hmc_inverse_metric", "hmc_divergences"}


def _g1_analysis(tmp_path, monkeypatch):
    from bayesian_inference import emulation
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
    return path, analysis, h5io


def test_dropin_sampler_hmc(tmp_path, monkeypatch):
    import os
    import pickle
    from bayesian_inference import emulation, log_posterior, mcmc
    path, analysis, h5io = _g1_analysis(tmp_path, monkeypatch)
    mc = analysis["parameters"]["mcmc"]
    assert mcmc.MCMCConfig("test_analysis", "exponential", analysis, path).sampler == "stretch"
    mc.update(sampler="hmc", hmc_n_leapfrog=4, hmc_step_size=0.2, n_burn_steps=40, n_sampling_steps=50,
              find_map=True, posterior_predictive=True)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert (cfg.sampler, cfg.hmc_n_leapfrog, cfg.hmc_target_accept, cfg.hmc_step_size) == ("hmc", 4, 0.8, 0.2)
    c0 = hmc_counts()
    np.random.seed(2)
    mcmc.run_mcmc(cfg)
    dc = hmc_counts() - c0
    assert dc[HP["BEGIN"]] == 90 and dc[HP["ADAPT"]] == 40 and dc[HP["ACCEPT_MEAN"]] == 50 and dc[HP["MOMENTS"]] >= 1
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    pp = {f"posterior_predictive_{k}" for k in mcmc.POSTERIOR_PREDICTIVE_KEYS}
    assert set(back) == USUAL | HMC_KEYS | {"map_parameters", "map_log_prob", "map_hessian"} | pp, set(back)
    box = analysis["parameterization"]["exponential"]
    lo, hi = np.asarray(box["min"], float), np.asarray(box["max"], float)
    d, W = lo.size, cfg.n_walkers
    assert back["chain"].shape == (50, W, d) and back["log_prob"].shape == (50, W)
    assert back["acceptance_fraction"].shape == (W,) and np.all((back["acceptance_fraction"] >= 0) & (back["acceptance_fraction"] <= 1))
    assert np.all((back["chain"] > lo) & (back["chain"] < hi)) and np.all(np.isfinite(back["log_prob"]))
    assert back["hmc_inverse_metric"].shape == (d,) and np.all(back["hmc_inverse_metric"] > 0)
    assert float(back["hmc_step_size"]) > 0 and back["hmc_divergences"].shape == (W,)
    assert float(back["map_log_prob"]) >= float(back["log_prob"].max()) - 1e-9 * max(1.0, abs(float(back["log_prob"].max())))
    sd = back["chain"].std(axis=0)                               # [W, d]: how far every chain moved in every parameter
    print(f"\nHMC drop-in: step size {float(back['hmc_step_size']):.4g}, inverse metric {back['hmc_inverse_metric']}, prior variance "
          f"{(hi - lo) ** 2 / 12}, acceptance {back['acceptance_fraction']}, divergences {back['hmc_divergences']}, smallest "
          f"per-chain standard deviation per parameter {sd.min(axis=0)} (chain {sd.argmin(axis=0)}), box {lo} .. {hi}")
    # what reads a chain reads this one
    tau = integrated_time(back["chain"], quiet=True)
    assert tau.shape == (d,) and np.all(np.isfinite(tau))
    out = mcmc.posterior_predictive(cfg, discard=10, thin=2)
    assert np.all(np.isfinite(out["mean"])) and out["quantiles"].shape[0] == 3
    from gpemu import select
    q = select.quantile(back["chain"].reshape(-1, d), (0.05, 0.5, 0.95), axis=0)
    assert np.allclose(q, np.quantile(back["chain"].reshape(-1, d), (0.05, 0.5, 0.95), axis=0), rtol=1e-14)
    with open(cfg.sampler_outputfile, "rb") as fh:
        one = pickle.load(fh)
    assert np.array_equal(one.get_chain(), back["chain"]) and one.hmc_step_size == float(back["hmc_step_size"])

    # the declined combinations raise before any step
    def declined(match, closure_index=-1, world=1, **keys):
        a = {**analysis, "parameters": {**analysis["parameters"], "mcmc": {**mc, **keys}}}
        cfg2 = mcmc.MCMCConfig("test_analysis", "exponential", a, path)
        os.remove(cfg.mcmc_outputfile) if os.path.exists(cfg.mcmc_outputfile) else None
        monkeypatch.setattr(mcmc, "_rank_world", lambda: (0, world))
        c1, g1 = hmc_counts(), M.grad_path_counts()
        with pytest.raises(ValueError, match=match):
            mcmc.run_mcmc(cfg2, closure_index=closure_index)
        assert np.array_equal(hmc_counts(), c1) and np.array_equal(M.grad_path_counts(), g1)
        assert not os.path.exists(cfg2.mcmc_outputfile)
    declined("tempering", n_temperatures=3)
    declined("one GPU", world=2)
    a_cl = dict(analysis)
    a_cl["validation_indices"] = [0, 2]
    cfg3 = mcmc.MCMCConfig("test_analysis", "exponential", a_cl, path, closure_index=0)
    monkeypatch.setattr(mcmc, "_rank_world", lambda: (0, 1))
    with pytest.raises(ValueError, match="stacked"):
        mcmc.run_mcmc(cfg3, closure_index=0)
    with pytest.raises(ValueError, match="sampler"):
        mcmc.MCMCConfig("test_analysis", "exponential",
                        {**analysis, "parameters": {**analysis["parameters"], "mcmc": {**mc, "sampler": "nuts"}}}, path)
    # a kernel without a gradient path: said before the first step
    monkeypatch.setattr(mcmc, "find_map_unsupported", lambda *a: "emulation group 'main' has a Matern kernel of nu = 0.5")
    c1 = hmc_counts()
    with pytest.raises(ValueError, match="nu = 0.5.*no step"):
        mcmc.run_mcmc(cfg)
    assert np.array_equal(hmc_counts(), c1)
    log_posterior.initialize_pool_variables(None, None, None, None, None, None)
    emulation.release_device_models()
