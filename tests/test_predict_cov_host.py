"""CPU: the joint-covariance reference (tests/cov_ref.py) against scikit-learn 1.7.2's predict(X, return_cov=True) on
the goldens, and the GaussianProcessRegressor interface checks that run before any device call."""
import numpy as np
import pytest

import cov_ref as CR
import golden_util as GU
from gpemu import estimators as E
from oracle import gp_oracle as O


def _load(name):
    g = GU.load(name)
    design = GU.load("observables_fixture")["design"] if name.startswith("g3") else None
    return g, GU.group_model(g, design=design)


def _skl_kernel(gp, spec):
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern, WhiteKernel
    ls = np.asarray(gp.ls, dtype=np.float64)
    k = RBF(length_scale=ls) if spec.kind == O.RBF else Matern(length_scale=ls, nu=spec.nu)
    if spec.has_const:
        k = k + ConstantKernel(gp.const)
    if spec.has_noise:
        k = k + WhiteKernel(gp.noise)
    return k


@pytest.mark.parametrize("name", ["g1_rbf_noise", "g1_matern25_const_noise", "g1_rbf_only", "g3_realdata_matern15"])
def test_cov_ref_matches_sklearn(name):
    pytest.importorskip("sklearn")
    from sklearn.gaussian_process import GaussianProcessRegressor
    g, model = _load(name)
    X = model.X_train
    Xq = np.concatenate([g["Xq"][:12], X[:2]])          # two training rows among the queries
    X2 = g["Xq"][12:19]
    for i, gp in enumerate(model.gps[:3]):
        skl = GaussianProcessRegressor(kernel=_skl_kernel(gp, model.spec), optimizer=None,
                                       alpha=float(g["gpr_alpha"])).fit(X, g["Y_pca_truncated"][:, i])
        _, cov = skl.predict(Xq, return_cov=True)
        ref = CR.PCCov(Xq, None, X, gp, model.spec)
        C = np.asarray(ref.C, dtype=np.float64)
        scale = 1.0 + abs(gp.const) + abs(gp.noise)
        # skl factors K + alpha I itself (the golden's L_ to rounding): agreement to the conditioning of L
        assert np.max(np.abs(C - cov)) <= 1e-8 * scale, name
        assert np.array_equal(C, C.T)
        # the two-set form: skl has no such call; it is the off-diagonal block of the symmetric form on [X1; X2]
        both = np.concatenate([Xq, X2])
        _, cov_b = skl.predict(both, return_cov=True)
        two = CR.PCCov(Xq, X2, X, gp, model.spec)
        assert np.max(np.abs(np.asarray(two.C, dtype=np.float64) - cov_b[:len(Xq), len(Xq):])) <= 1e-8 * scale
        assert np.all(ref.bound >= 0) and np.all(np.isfinite(ref.bound))


def _gpr():
    k = E.ARDKernel(E.RBF_KIND, [0.5, 0.5], [[1e-2, 1e2]] * 2, noise_level=1e-3, noise_level_bounds=(1e-8, 1.0))
    gpr = E.GaussianProcessRegressor(kernel=k)
    gpr.kernel_ = k
    gpr.X_train_ = np.zeros((3, 2))
    return gpr


def test_return_std_and_return_cov_rejected_before_the_device():
    gpr = _gpr()
    gpr._device = lambda: pytest.fail("device touched")     # noqa: E731
    with pytest.raises(RuntimeError, match="At most one of return_std or return_cov can be requested."):
        gpr.predict(np.zeros((2, 2)), return_std=True, return_cov=True)


def test_sample_y_interface():
    gpr = _gpr()
    assert callable(getattr(gpr, "sample_y", None))
    gpr._device = lambda: pytest.fail("device touched")     # noqa: E731
    for bad in (0, -3):
        with pytest.raises(ValueError):
            gpr.sample_y(np.zeros((2, 2)), n_samples=bad)
    with pytest.raises(ValueError):
        gpr.sample_y(np.zeros((2, 2)), n_samples=2, random_state="seed")


def test_sample_y_jitter_not_pickled():
    gpr = _gpr()
    gpr.sample_y_jitter_ = 0.0
    assert "sample_y_jitter_" not in gpr.__getstate__()


def test_random_state_like_sklearn():
    pytest.importorskip("sklearn")
    from sklearn.utils import check_random_state
    for seed in (7, np.random.RandomState(3)):
        a = E._check_random_state(seed).standard_normal(5)
        b = check_random_state(seed if isinstance(seed, int) else np.random.RandomState(3)).standard_normal(5)
        assert np.array_equal(a, b)
    assert E._check_random_state(None) is np.random.mtrand._rand


def test_library_declares_the_new_calls():
    from gpemu import _lib
    for name in ("gpemu_gp_predict_cov", "gpemu_gp_predict_cov_dev", "gpemu_gp_sample"):
        assert name in _lib.exported_symbols()
