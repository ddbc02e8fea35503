"""-m gpu: the joint predictive covariance (gpemu_gp_predict_cov) and the draws (gpemu_gp_sample) against the
extended-precision reference of tests/cov_ref.py, element by element within its a-priori bound.

The two-set form is checked on disjoint sets with M1 != M2 (a symmetric output would hide a swapped store).  Where the
reference would be slow (N = 1000, M = 1030) it runs on a subset of rows and columns that holds every edge and special
one: the first and last rows, the 64-column tile edges, the training row, the duplicates and the far query.
"""
import ctypes as C
import math

import numpy as np
import pytest

import cov_ref as CR
import golden_util as GU
import hp_ref as H
import matern_nu_ref as R
from gpemu import _lib
from gpemu import estimators as E
from gpemu.fit import LinAlgError
from gpemu.model import DeviceModel
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

LD = np.longdouble

KERNELS = {"rbf": (O.RBF, math.inf), "m05": (O.MATERN, 0.5), "m15": (O.MATERN, 1.5), "m25": (O.MATERN, 2.5),
           "nu075": (O.MATERN, 0.75), "nuinf": (O.MATERN, math.inf)}


def within(what, dev, ref, bound):
    dev = np.asarray(dev, dtype=np.float64)
    err = np.abs(dev.astype(LD) - ref).astype(np.float64)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio.max() <= 1.0, (f"{what}: max err/bound {ratio.max():.3g} at {worst}: dev {dev[worst]!r} "
                                f"ref {float(ref[worst])!r} bound {bound[worst]:.3g}")
    return float(ratio.max())


def synth(kernel, cn, d, N, k=2, seed=0):
    """a GroupModel fitted at fixed theta on a random design in [0, 1]^d (noise-free forms: jitter 1e-8)"""
    kind, nu = KERNELS[kernel]
    rng = np.random.default_rng(seed + 1000 * d + N)
    X = rng.uniform(0.0, 1.0, (N, d))
    spec = O.KernelSpec(kind=kind, nu=nu, has_const=cn, has_noise=cn)
    gps = []
    for p in range(k):
        ls = 0.35 * math.sqrt(d) * (1.0 + 0.3 * p) * rng.uniform(0.8, 1.25, d)
        y = np.sin(X @ rng.normal(size=d) * 3.0) + 0.1 * p
        theta = np.log(np.r_[ls, [0.7] if cn else [], [0.01] if cn else []])
        with R.general_nu():
            gps.append(O.gp_fit_at_theta(X, y, theta, spec, 1e-10 if cn else 1e-8))
    F = 3
    return O.GroupModel(X_train=X, spec=spec, gps=gps, components=rng.normal(size=(k, F)),
                        explained_variance=np.ones(k), scaler_mean=np.zeros(F), scaler_scale=np.ones(F), n_pc=k)


def queries(model, M, seed, special=True):
    """M rows in and around the design; with `special`: a training row (0), a duplicate pair (1, 2), one far query"""
    d = model.X_train.shape[1]
    X = np.random.default_rng(seed).uniform(-0.1, 1.1, (M, d))
    if special and M >= 4:
        X[0] = model.X_train[3]
        X[2] = X[1]
        X[-1] = 4.0
    return X


def edges(M, rng):
    s = {0, 1, 2, 3, M - 1, M - 2} | {t + o for t in range(64, M, 64) for o in (-1, 0)}
    s |= set(rng.integers(0, M, 8).tolist())
    return np.array(sorted(i for i in s if 0 <= i < M))


def check_two_set(model, dm, X1, X2, rows=None, cols=None, tag=""):
    _, cov = dm.gp_predict_cov(X1, X2)
    assert cov.shape == (model.n_pc, len(X1), len(X2))
    rows = np.arange(len(X1)) if rows is None else rows
    cols = np.arange(len(X2)) if cols is None else cols
    for p, ref in enumerate(CR.predict_cov(X1[rows], X2[cols], model)):
        within(f"{tag} pc {p}", cov[p][np.ix_(rows, cols)], ref.C, ref.bound)
    return cov


@pytest.mark.parametrize("d", [1, 6, 8, 9, 16])
@pytest.mark.parametrize("cn", [False, True], ids=["plain", "const_noise"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_two_set_grid(kernel, cn, d):
    for N, pairs in ((50, [(1, 17), (300, 17)]), (150, [(17, 300)])):
        model = synth(kernel, cn, d, N)
        dm = GU.device_model(model)
        try:
            for i, (M1, M2) in enumerate(pairs):
                X1 = queries(model, M1, 10 * i + 1)
                X2 = queries(model, M2, 10 * i + 2, special=False)
                check_two_set(model, dm, X1, X2, tag=f"{kernel} N={N} {M1}x{M2}")
        finally:
            dm.close()


@pytest.mark.parametrize("kernel,d", [("rbf", 6), ("m05", 9), ("nu075", 6), ("m25", 16)])
def test_two_set_large(kernel, d):
    """N = 1000 and M = 1030: a subset of rows and columns with every edge and special one"""
    rng = np.random.default_rng(5)
    model = synth(kernel, True, d, 1000)
    dm = GU.device_model(model)
    try:
        X1 = queries(model, 1030, 3)
        X2 = queries(model, 300, 4, special=False)
        X2[0] = model.X_train[999]
        check_two_set(model, dm, X1, X2, edges(1030, rng), edges(300, rng), tag=f"{kernel} N=1000")
    finally:
        dm.close()


@pytest.mark.parametrize("kernel,cn,d", [("rbf", True, 6), ("rbf", False, 1), ("m05", True, 8), ("m15", False, 9),
                                         ("m25", True, 16), ("nu075", True, 6), ("nuinf", False, 6)])
def test_symmetric_form(kernel, cn, d):
    model = synth(kernel, cn, d, 150)
    dm = GU.device_model(model)
    try:
        X = queries(model, 300, 7)
        mean, cov = dm.gp_predict_cov(X)
        assert np.array_equal(cov, np.transpose(cov, (0, 2, 1))), "not symmetric bit for bit"
        m, v = dm.gp_predict(X)
        assert np.array_equal(mean, m), "mean differs from gp_predict's"
        _, two = dm.gp_predict_cov(X, X.copy())
        _, _, _, vb, _ = H.gp_predict(X, model, cx=H.C_X8)       # the factor this check was set with
        for p, ref in enumerate(CR.predict_cov(X, None, model)):
            lo = np.tril_indices(len(X))
            within(f"sym pc {p}", cov[p][lo], ref.C[lo], ref.bound[lo])
            noise = model.gps[p].noise if cn else 0.0
            ref2 = CR.PCCov(X, X, model.X_train, model.gps[p], model.spec)
            within(f"sym - noise vs two-set pc {p}", cov[p] - noise * np.eye(len(X)), two[p].astype(LD),
                   ref.bound + ref2.bound + 2 * H.U * noise * np.eye(len(X)))
            dg = np.diag(cov[p])
            vraw = np.asarray(dg, dtype=LD)
            big = v[:, p] > vb[:, p]
            within(f"diag vs var pc {p}", dg[big], np.asarray(v[big, p], dtype=LD),
                   np.diag(ref.bound)[big] + vb[big, p])
            assert np.all(np.isfinite(vraw))
    finally:
        dm.close()


def test_chunking_is_bit_identical():
    model = synth("m25", True, 6, 150, k=3)
    dm = GU.device_model(model)
    try:
        X1 = queries(model, 300, 1)
        X2 = queries(model, 200, 2, special=False)
        N64, M1p, M2p = 192, 320, 256
        one_sym = (2 * N64 * M1p + M1p * 64) * 8
        one_two = (2 * N64 * M1p + (M1p + 2 * N64) * 64) * 8
        for X2_, one in ((None, one_sym), (X2, one_two)):
            m0, c0 = dm.gp_predict_cov(X1, X2_)
            for ws in (one, one + 64 * 8 * (M1p + (0 if X2_ is None else 2 * N64)), 2 * one + 1):
                m1, c1 = dm.gp_predict_cov(X1, X2_, workspace_bytes=ws)
                assert np.array_equal(m0, m1) and np.array_equal(c0, c1), ws
            with pytest.raises(_lib.GpemuError) as e:
                dm.gp_predict_cov(X1, X2_, workspace_bytes=one - 8)
            assert e.value.code == -1 and "workspace_bytes" in str(e.value)
    finally:
        dm.close()


def test_abi_argument_checks():
    model = synth("rbf", True, 6, 50)
    dm = GU.device_model(model)
    try:
        L = _lib.lib()
        X = np.zeros((4, 6))
        out = np.empty(2 * 16)
        assert L.gpemu_gp_predict_cov(dm.handle, 0, _lib.ptr(X), 0, None, 0, None, _lib.ptr(out)) == -1
        assert L.gpemu_gp_predict_cov(dm.handle, 4, None, 0, None, 0, None, _lib.ptr(out)) == -1
        X[1, 2] = np.nan
        assert L.gpemu_gp_predict_cov(dm.handle, 4, _lib.ptr(X), 0, None, 0, None, _lib.ptr(out)) == -1
        z = np.zeros(2 * 4)
        tau = np.empty(2)
        assert L.gpemu_gp_sample(dm.handle, 4, _lib.ptr(X), 1, _lib.ptr(z), _lib.ptr(out), _lib.ptr(tau)) == -1
    finally:
        dm.close()


# ---- the GaussianProcessRegressor interface on the goldens' fitted emulators --------------------------------------
def golden_gprs(name, n=2):
    g = GU.load(name)
    design = GU.load("observables_fixture")["design"] if name.startswith("g3") else None
    model = GU.group_model(g, design=design)
    spec = model.spec
    out = []
    for gp in model.gps[:n]:
        d = model.X_train.shape[1]
        k = E.ARDKernel(spec.kind, gp.ls, [[1e-5, 1e5]] * d, spec.nu,
                        constant_value=gp.const if spec.has_const else None, constant_value_bounds=(1e-5, 1e5),
                        noise_level=gp.noise if spec.has_noise else None, noise_level_bounds=(1e-12, 1e5))
        r = E.GaussianProcessRegressor(kernel=k)
        r.kernel_, r.X_train_, r.L_, r.alpha_ = k, model.X_train, gp.L, gp.alpha
        out.append((r, gp))
    return model, out


GOLDENS = ["g1_rbf_noise", "g1_matern25_const_noise", "g3_realdata_matern15", "g10_wide_d_rbf_const_noise_d10"]


@pytest.mark.parametrize("name", GOLDENS)
def test_gpr_predict_cov_and_sample_y(name):
    model, gprs = golden_gprs(name)
    rng = np.random.default_rng(11)
    lo, hi = model.X_train.min(axis=0), model.X_train.max(axis=0)
    X = rng.uniform(lo, hi, (20, model.X_train.shape[1]))
    X[0] = model.X_train[5]
    for r, gp in gprs:
        mean, cov = r.predict(X, return_cov=True)
        assert mean.shape == (20,) and cov.shape == (20, 20)
        ref = CR.PCCov(X, None, model.X_train, gp, model.spec)
        within(f"{name} predict cov", cov, ref.C, ref.bound)
        pr = H.PCRef(X, model.X_train, gp, model.spec, cx=H.C_X8)
        within(f"{name} predict mean", mean, pr.mean, pr.mean_bound)
        Y = r.sample_y(X, n_samples=5, random_state=7)
        assert Y.shape == (20, 5)
        Z = np.random.RandomState(7).standard_normal((20, 5))
        Yr, yb = CR.draws(ref.C, ref.bound, pr.mean, pr.mean_bound, r.sample_y_jitter_, Z)
        within(f"{name} sample_y", Y, Yr, yb)
        assert np.array_equal(Y, r.sample_y(X, n_samples=5, random_state=np.random.RandomState(7)))
        r._dev.close()


def test_sample_y_statistics():
    model, gprs = golden_gprs("g1_matern25_const_noise", n=1)
    r, gp = gprs[0]
    X = model.X_train[:6] * 0.7 + 0.3 * model.X_train[6:12]
    n = 40000
    Y = r.sample_y(X, n_samples=n, random_state=3)
    mean, cov = r.predict(X, return_cov=True)
    se_m = np.sqrt(np.diag(cov) / n)
    assert np.all(np.abs(Y.mean(axis=1) - mean) <= 5 * se_m)
    emp = np.cov(Y)
    se_c = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov * cov) / n)
    assert np.all(np.abs(emp - cov) <= 5 * se_c)
    r._dev.close()


def test_duplicate_rows_need_jitter():
    """noise-free RBF: far rows repeated -- C has an exact block of ones there (K_* underflows to 0), whose pivots are
    0 -- beside training rows, where the variance is the fit's alpha"""
    g = GU.load("g1_rbf_only")
    model = GU.group_model(g)
    X = np.concatenate([model.X_train[:6], np.full((3, 6), 30.0), np.full((2, 6), -30.0)])
    dm = GU.device_model(model)
    try:
        z = np.random.RandomState(1).standard_normal((model.n_pc, len(X), 4))
        draws, tau = dm.gp_sample(X, z)
        assert np.all(tau > 0), tau
        assert np.all(np.isfinite(draws))
    finally:
        dm.close()


def test_indefinite_covariance_exhausts_the_ladder():
    """an L that is not the factor of its kernel (0.01 I): C = kdiag - 1e4 K*^T K* is strongly indefinite"""
    model = synth("rbf", True, 6, 50, k=3)
    Lbad = np.stack([0.01 * np.eye(50)] * 3)
    Lbad[0] = model.gps[0].L                      # PC 0 stays sound: the first failing PC is 1
    dm = DeviceModel(X_train=model.X_train, ls=np.stack([gp.ls for gp in model.gps]),
                     alpha=np.stack([gp.alpha for gp in model.gps]), L=Lbad, components=model.components,
                     scaler_mean=model.scaler_mean, scaler_scale=model.scaler_scale, kernel_kind=O.RBF,
                     const=np.array([gp.const for gp in model.gps]), noise=np.array([gp.noise for gp in model.gps]))
    try:
        X = queries(model, 12, 3, special=False)
        z = np.random.RandomState(2).standard_normal((3, 12, 2))
        with pytest.raises(LinAlgError):
            dm.gp_sample(X, z)
        out = np.empty(3 * 12 * 2)
        tau = np.empty(3)
        rc = _lib.lib().gpemu_gp_sample(dm.handle, 12, _lib.ptr(X), 2, _lib.ptr(z), _lib.ptr(out), _lib.ptr(tau))
        assert rc == 2, (rc, _lib.last_error())
        assert tau[0] == 0.0 and np.all(np.isnan(tau[1:]))
    finally:
        dm.close()


def test_c3_size():
    """N = 1000, k = 10, M = 2048, all PCs in one call: symmetric; 64 rows of two PCs against the reference"""
    model, _, _ = GU.fixed_theta_model(1000, 40, 10, seed=0)
    dm = GU.device_model(model)
    try:
        from gpemu import synthetic
        X = synthetic.make_walkers(2048, seed=4)
        mean, cov = dm.gp_predict_cov(X)
        assert cov.shape == (10, 2048, 2048)
        assert np.array_equal(cov, np.transpose(cov, (0, 2, 1)))
        rows = np.unique(np.r_[0, 63, 64, 1023, 2047, np.random.default_rng(0).integers(0, 2048, 59)])[:64]
        for p in (0, 9):
            gp = model.gps[p]
            ref = CR.PCCov(X[rows], X, model.X_train, gp, model.spec)
            C = ref.C.copy()
            C[np.arange(len(rows)), rows] += LD(gp.noise)      # the symmetric form's noise on the diagonal
            within(f"C3 pc {p}", cov[p][rows], C, ref.bound + H.U * gp.noise)
    finally:
        dm.close()
