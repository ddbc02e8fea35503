"""-m gpu tests of models, fit handles and samplers with 9 to 16 parameters (the padded width 16 of csrc/internal.h:
DPAD_WIDE): fit-side kernel matrix / LML / gradient, predictions, full predictions and the log-posterior against the CPU
oracle, the d = 8 path against the wide path on the same problem (padding cross-check), sampler chains against the
stretch-move restatement (d = 9, 12, 16; the state's log-probabilities also within the bound of tests/hp_ref.py),
snapshot and restore at d = 16, and the rejection of d > 16."""
import contextlib

import numpy as np
import pytest

import matern_nu_ref as R
from oracle import gp_oracle as O
from oracle import sampler_oracle as SO

pytestmark = pytest.mark.gpu

TOL = 1e-8


def relerr(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _design(N, d, seed):
    rng = np.random.default_rng(seed)
    lo = -1.0 - rng.uniform(0.0, 1.0, d)
    hi = 1.0 + rng.uniform(0.0, 1.0, d)
    X = rng.uniform(lo, hi, (N, d))
    return X, lo, hi, rng


def _problem(N, d, F, k, seed=0, spec=None, X=None, lo=None, hi=None, ls=None, data=None):
    """A synthetic d-parameter emulation group fitted at a fixed theta by the oracle: (GroupModel, problem dict)."""
    if X is None:
        X, lo, hi, rng = _design(N, d, seed)
    else:
        rng = np.random.default_rng(seed)
    spec = spec or O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=False, has_noise=True)
    if data is None:
        Wm = rng.normal(size=(d, F))
        Y = np.sin(X @ Wm) + 0.1 * (X ** 2) @ np.abs(Wm) + 0.01 * rng.normal(size=(X.shape[0], F))
        y_exp = Y[0] + 0.05 * rng.normal(size=F)
        y_err = 0.1 * np.abs(Y[0]) + 0.05
    else:
        Y, y_exp, y_err = data
    mean, scale, _ = O.scaler_fit(Y)
    pca = O.pca_fit((Y - mean) / scale)
    if ls is None:
        ls = (hi - lo) * (0.4 + 0.1 * np.arange(d) / d)
    theta = np.log(np.r_[ls, [0.7] if spec.has_const else [], [0.03] if spec.has_noise else []])
    gps = [O.gp_fit_at_theta(X, pca["Y_pca"][:, i], theta, spec, 1e-10) for i in range(k)]
    model = O.GroupModel(X_train=X, spec=spec, gps=gps, components=pca["components"],
                         explained_variance=pca["explained_variance"], scaler_mean=mean, scaler_scale=scale, n_pc=k)
    return model, dict(X=X, lo=lo, hi=hi, Y=pca["Y_pca"], theta=theta, y_exp=y_exp, y_err=y_err, spec=spec,
                       data=(Y, y_exp, y_err))


def _device(model):
    import golden_util as GU
    return GU.device_model(model)


def _queries(prob, B, seed):
    """B rows: walkers inside the box, training points and (every 7th) rows outside the box."""
    rng = np.random.default_rng(seed)
    lo, hi, X = prob["lo"], prob["hi"], prob["X"]
    Q = rng.uniform(lo, hi, (B, lo.size))
    Q[1::5] = X[rng.integers(0, X.shape[0], Q[1::5].shape[0])]
    out = Q[3::7]
    out[:, rng.integers(0, lo.size)] = hi.max() + 1.0
    Q[3::7] = out
    return Q


CASES = [  # (d, spec): RBF + constant + noise; Matern 0.75 (direct distance of near pairs); Matern 2.5
    (9, O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=True, has_noise=True)),
    (10, O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=True, has_noise=True)),
    (12, O.KernelSpec(kind=O.MATERN, nu=0.75, has_const=False, has_noise=True)),
    (15, O.KernelSpec(kind=O.MATERN, nu=1.5, has_const=False, has_noise=True)),
    (16, O.KernelSpec(kind=O.MATERN, nu=2.5, has_const=False, has_noise=True)),
]


def _oracle_for(spec):
    """the oracle's base kernel extended to every nu where the spec needs it (matern_nu_ref.general_nu)"""
    closed = spec.kind == O.RBF or spec.nu in (0.5, 1.5, 2.5, np.inf)
    return contextlib.nullcontext() if closed else R.general_nu()


def _counts():
    import ctypes as C

    from gpemu import _lib
    out = (C.c_int64 * 16)()
    n = _lib.lib().gpemu_wide_path_counts(out, 16)
    return np.array(out[:n])


@pytest.mark.parametrize("d,spec", CASES, ids=[f"d{c[0]}" for c in CASES])
def test_fit_kernel_matrix_lml_and_gradient(d, spec):
    from gpemu import fit as _fit
    with _oracle_for(spec):
        model, prob = _problem(150, d, 12, 3, seed=d, spec=spec)
    X, th = prob["X"], prob["theta"]
    before = _counts()
    K = _fit.kernel_matrix(X, th, spec.kind, spec.nu, spec.has_const, spec.has_noise)
    assert relerr(K, R.kernel_matrix(X, th, spec)) < 1e-12
    df = _fit.DeviceFit(X, spec.kind, spec.nu, spec.has_const, spec.has_noise, 1e-10)
    Y = prob["Y"]
    for i in range(3):
        val, grad = df.lml(Y[:, i], th)
        if isinstance(_oracle_for(spec), contextlib.nullcontext):
            rv, rg = O.lml_and_grad(X, Y[:, i], th, spec, 1e-10)
            gtol = 1e-7
        else:   # general nu: the oracle has no analytic gradient; central differences (test_gpu_matern_nu.py's bound)
            rv, rg = R.lml(X, Y[:, i], th, spec), R.lml_grad_central(X, Y[:, i], th, spec)
            gtol = 1e-6
        assert abs(val - rv) < 1e-9 * abs(rv)
        assert np.max(np.abs(grad - rg)) < gtol * max(1.0, np.max(np.abs(rg))), (grad, rg)
    thetas = np.stack([th, th + 0.05, th - 0.05])
    lml_b, grad_b, info = df.lml_batch(Y[:, :3].T.copy(), thetas)
    assert np.all(info == 0)
    for i in range(3):
        v, g = df.lml(Y[:, i], thetas[i])
        assert lml_b[i] == v
        np.testing.assert_array_equal(grad_b[i], g)
    df.close()
    after = _counts()
    assert after[3] > before[3] and after[4] > before[4]        # the 16-wide kmat and gradient instances ran


@pytest.mark.parametrize("d,spec", CASES, ids=[f"d{c[0]}" for c in CASES])
def test_predict_and_logpost_against_oracle(d, spec):
    with _oracle_for(spec):
        _predict_and_logpost(d, spec)


def _predict_and_logpost(d, spec):
    model, prob = _problem(200, d, 14, 4, seed=100 + d, spec=spec)
    dm = _device(model)
    dm.likelihood_setup(prob["y_exp"], prob["y_err"], prob["lo"], prob["hi"], 1.0)
    ks = int(np.ceil((d + 1) / 4))
    before = _counts()
    for B in (100, 300):                                          # both cross-kernel forms (<= 128, > 256 columns)
        Q = _queries(prob, B, seed=B + d)
        m, v = dm.gp_predict(Q)
        mo, vo = O.gp_predict_all(Q, model)
        assert np.max(np.abs(m - mo)) < TOL * max(1.0, np.max(np.abs(mo)))
        assert np.max(np.abs(v - vo)) < TOL
        rows = np.r_[np.arange(0, 12), np.arange(B - 8, B)]
        cv, cov = dm.predict_full(Q[rows], n_div=1.0)
        for j, r in enumerate(rows[:6]):
            ref = O.predict_group(Q[r:r + 1], model)
            assert relerr(cv[j], ref["central_value"][0]) < TOL
            assert relerr(cov[j], ref["cov"][0]) < TOL
        inside = np.all((Q > prob["lo"]) & (Q < prob["hi"]), axis=1)
        assert not inside.all()
        for mode in (0, 1):
            lp = dm.logpost(Q, mode=mode)
            assert np.array_equal(np.isneginf(lp), ~inside)
            ref = np.array([O.log_posterior(Q[r], {"g": model}, prob["lo"], prob["hi"], prob["y_exp"],
                                            prob["y_err"])[0] for r in rows])
            fin = np.isfinite(ref)
            assert np.array_equal(fin, np.isfinite(lp[rows]))
            assert np.max(np.abs(lp[rows][fin] - ref[fin]) / np.abs(ref[fin])) < TOL
    after = _counts()
    assert after[ks - 3] > before[ks - 3]                         # the cross-kernel of ceil((d + 1) / 4) k-steps ran
    dm.close()


def test_padding_cross_check_d8_against_d9():
    """The same problem at d = 8 and with a ninth coordinate that is 0 everywhere (box (-1, 1)): the 8-wide and the
    16-wide instances.  The extra terms are exact zeros, so the results agree to rounding (here: bit for bit is
    allowed, 1e-12 is asserted) and the extra length scale's gradient is exactly 0."""
    from gpemu import fit as _fit
    spec = O.KernelSpec(kind=O.MATERN, nu=2.5, has_const=True, has_noise=True)
    X8, lo8, hi8, _ = _design(180, 8, 5)
    m8, p8 = _problem(180, 8, 10, 3, seed=5, spec=spec, X=X8, lo=lo8, hi=hi8)
    X9 = np.c_[X8, np.zeros(X8.shape[0])]
    lo9, hi9 = np.r_[lo8, -1.0], np.r_[hi8, 1.0]
    ls9 = np.r_[np.exp(p8["theta"][:8]), 1.3]
    m9, p9 = _problem(180, 9, 10, 3, seed=5, spec=spec, X=X9, lo=lo9, hi=hi9, ls=ls9, data=p8["data"])
    # fit side
    f8 = _fit.DeviceFit(X8, spec.kind, spec.nu, spec.has_const, spec.has_noise, 1e-10)
    f9 = _fit.DeviceFit(X9, spec.kind, spec.nu, spec.has_const, spec.has_noise, 1e-10)
    for i in range(3):
        v8, g8 = f8.lml(p8["Y"][:, i], p8["theta"])
        v9, g9 = f9.lml(p9["Y"][:, i], p9["theta"])
        assert abs(v9 - v8) <= 1e-12 * abs(v8)
        assert g9[8] == 0.0
        assert np.max(np.abs(np.delete(g9, 8) - g8)) <= 1e-12 * max(1.0, np.max(np.abs(g8)))
    f8.close()
    f9.close()
    # predictions and log-posterior
    d8, d9 = _device(m8), _device(m9)
    for dm, p in ((d8, p8), (d9, p9)):
        dm.likelihood_setup(p["y_exp"], p["y_err"], p["lo"], p["hi"], 1.0)
    for B in (64, 300):
        Q8 = _queries(p8, B, seed=B)
        Q9 = np.c_[Q8, np.zeros(B)]
        a, b = d8.gp_predict(Q8), d9.gp_predict(Q9)
        for x, y in zip(a, b):
            assert np.max(np.abs(x - y)) <= 1e-12 * max(1.0, np.max(np.abs(x)))
        for mode in (0, 1):
            l8, l9 = d8.logpost(Q8, mode=mode), d9.logpost(Q9, mode=mode)
            assert np.array_equal(np.isfinite(l8), np.isfinite(l9))
            fin = np.isfinite(l8)
            assert np.max(np.abs(l9[fin] - l8[fin]) / np.abs(l8[fin])) <= 1e-12
    d8.close()
    d9.close()


def _sampler_setup(d=12, N=150):
    spec = O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=False, has_noise=True)
    model, prob = _problem(N, d, 10, 3, seed=40 + d, spec=spec)
    dm = _device(model)
    dm.likelihood_setup(prob["y_exp"], prob["y_err"], prob["lo"], prob["hi"], 1.0)

    def oracle_lp(X):
        return np.array([O.log_posterior(x, {"g": model}, prob["lo"], prob["hi"], prob["y_exp"], prob["y_err"])[0]
                         for x in np.atleast_2d(X)])
    return model, prob, dm, oracle_lp


@pytest.mark.parametrize("W,steps", [(64, 6), (1024, 2)])
def test_sampler_chain_equals_oracle_d12(W, steps):
    from gpemu.sampler import DeviceSampler
    model, prob, dm, oracle_lp = _sampler_setup()
    rng = np.random.default_rng(W)
    X0 = rng.uniform(prob["lo"], prob["hi"], (W, 12))
    # the device's own (Philox) stream
    ds = DeviceSampler([dm], W, a=2.0, seed=0xABCDEF)
    ds.set_state(X0)
    X, lp0 = ds.get_state()
    np.testing.assert_array_equal(X, X0)
    np.testing.assert_allclose(lp0, oracle_lp(X0), rtol=TOL)
    ds.run(steps)
    chain, lps = ds.get_chain()
    assert chain.shape == (steps, W, 12)
    ochain, olps, onacc = SO.run(X0, oracle_lp, SO.PhiloxStream(0xABCDEF), steps)
    np.testing.assert_allclose(chain, ochain, rtol=1e-12, atol=1e-12)
    fin = np.isfinite(olps)
    assert np.array_equal(fin, np.isfinite(lps))
    np.testing.assert_allclose(lps[fin], olps[fin], rtol=TOL)
    np.testing.assert_array_equal(ds.counts()[0], onacc)
    ds.close()
    # host-RNG replay
    ds = DeviceSampler([dm], W)
    ds.set_state(X0)
    stream = SO.EmceeStream(77)
    for _ in range(steps):
        ds.step_host_rng(*stream.draw(W))
    chain, lps = ds.get_chain()
    ochain, olps, _ = SO.run(X0, oracle_lp, SO.EmceeStream(77), steps)
    np.testing.assert_allclose(chain, ochain, rtol=1e-12, atol=1e-12)
    ds.close()
    dm.close()


def test_stacked_chains_equal_separate_chains_d12():
    from gpemu.sampler import DeviceSampler
    model, prob, dm, _ = _sampler_setup()
    W, steps, seeds = 40, 5, [11, 22, 33]
    rng = np.random.default_rng(3)
    X0 = rng.uniform(prob["lo"], prob["hi"], (len(seeds) * W, 12))
    dm.likelihood_setup(np.tile(prob["y_exp"], (len(seeds), 1)), prob["y_err"], prob["lo"], prob["hi"], 1.0)
    st = DeviceSampler([dm], W, seeds=seeds)
    st.set_state(X0)
    st.run(steps)
    chain_s, lps_s = st.get_chain()
    st.close()
    dm.likelihood_setup(prob["y_exp"], prob["y_err"], prob["lo"], prob["hi"], 1.0)
    for c, sd in enumerate(seeds):
        one = DeviceSampler([dm], W, seed=sd)
        one.set_state(X0[c * W:(c + 1) * W])
        one.run(steps)
        ch, lp = one.get_chain()
        one.close()
        np.testing.assert_array_equal(chain_s[:, c * W:(c + 1) * W], ch)
        np.testing.assert_array_equal(lps_s[:, c * W:(c + 1) * W], lp)
    dm.close()


def _path_model(d, kind, nu):
    import path_cases as PC
    c = PC.Case(f"sampler_d{d}", 70, d, 3, 64, kind, nu, False)
    model, lo, hi, y_exp, y_err, bs, _ = PC.problem(c)
    dm = _device(model)
    dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0)

    def oracle_lp(X):
        return np.array([O.log_posterior(x, {"g": model}, lo, hi, y_exp, y_err)[0] for x in np.atleast_2d(X)])
    return model, lo, hi, y_exp, y_err, bs, dm, oracle_lp


@pytest.mark.parametrize("d", [9, 16])
def test_philox_chain_equals_oracle_and_state_within_bound(d):
    """d = 9 (7 padded lanes) and d = 16 (none): accept_kernel<16> and the 16-wide pad / unpad of the rows against the
    stretch-move restatement on the Philox stream; the state's log-probabilities within the hp_ref bound"""
    import hp_ref as H
    from gpemu.sampler import DeviceSampler
    model, lo, hi, y_exp, y_err, bs, dm, oracle_lp = _path_model(d, O.MATERN, 1.5)
    W, steps = 48, 6
    X0 = np.random.default_rng(d).uniform(lo + 0.2 * (hi - lo), hi - 0.2 * (hi - lo), (W, d))
    ds = DeviceSampler([dm], W, a=2.0, seed=0x5EED + d)
    ds.set_state(X0)
    ds.run(steps)
    chain, lps = ds.get_chain()
    ochain, olps, onacc = SO.run(X0, oracle_lp, SO.PhiloxStream(0x5EED + d), steps)
    np.testing.assert_allclose(chain, ochain, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(ds.counts()[0], onacc)
    assert onacc.sum() > 0
    X, lpd = ds.get_state()
    np.testing.assert_array_equal(X, chain[-1])
    lp, lb, _ = H.log_posterior(X, model, lo, hi, y_exp, y_err, bs)
    err = np.abs(lpd.astype(np.longdouble) - lp).astype(np.float64)
    r = np.where(err == 0, 0.0, err / np.maximum(lb, 1e-300))
    assert r.max() <= 1.0, f"state log-probability: err/bound {r.max():.3g}"
    print(f"\nRATIOS sampler_state_d{d} lp={r.max():.3g}")
    ds.close()
    dm.close()


def test_snapshot_restore_d16():
    """gpemu_sampler_snapshot / _restore at d = 16 (the snapshot's rows are 16 wide): the rerun block equals an
    unbroken run in state, chain and counts"""
    from gpemu import _lib
    from gpemu.sampler import DeviceSampler
    _, lo, hi, _, _, _, dm, _ = _path_model(16, O.RBF, np.inf)
    W = 40
    X0 = np.random.default_rng(4).uniform(lo + 0.2 * (hi - lo), hi - 0.2 * (hi - lo), (W, 16))
    a = DeviceSampler([dm], W, seed=31)
    b = DeviceSampler([dm], W, seed=31)
    a.set_state(X0)
    b.set_state(X0)
    a.run(9)
    b.run(4)
    _lib.check(_lib.lib().gpemu_sampler_snapshot(b._h))
    b.run(5)
    _lib.check(_lib.lib().gpemu_sampler_restore(b._h))
    b.run(5)
    np.testing.assert_array_equal(a.counts()[0], b.counts()[0])
    np.testing.assert_array_equal(a.get_chain()[0], b.get_chain()[0])
    np.testing.assert_array_equal(a.get_chain()[1], b.get_chain()[1])
    np.testing.assert_array_equal(a.get_state()[0], b.get_state()[0])
    np.testing.assert_array_equal(a.get_state()[1], b.get_state()[1])
    a.close()
    b.close()
    dm.close()


def test_d17_is_rejected():
    from gpemu import fit as _fit
    from gpemu._lib import GpemuError
    X, lo, hi, rng = _design(40, 17, 0)
    with pytest.raises(GpemuError, match="16"):
        _fit.DeviceFit(X, O.RBF, np.inf, False, True, 1e-10)
    from gpemu.model import DeviceModel
    k, F = 2, 5
    with pytest.raises(GpemuError, match="16"):
        DeviceModel(X_train=X, ls=np.ones((k, 17)), alpha=np.zeros((k, 40)), L=np.tile(np.eye(40), (k, 1, 1)),
                    components=np.eye(k, F), scaler_mean=np.zeros(F), scaler_scale=np.ones(F), noise=np.full(k, 0.1))
