"""CPU tests of cross-validation at the fitted hyper-parameters: the fold labels, the config keys, the
refusal of bad folds, and the numpy restatement of the closed form against scikit-learn (golden G9) and against
brute-force oracle refits."""
import numpy as np
import pytest
import yaml

import cv_ref as R
import dropin_util as DU
import golden_util as GU
from oracle import gp_oracle as O


def _g9():
    return GU.load("g9_cross_validation")


def test_kfold_labels_match_sklearn_kfold():
    from bayesian_inference import emulation
    g9 = _g9()
    for c in R.CASES:
        y = GU.load(c)["Y_pca_truncated"]
        N = y.shape[0]
        for k in (2, 5, N):
            np.testing.assert_array_equal(emulation.kfold_labels(N, k), g9[f"{c}_k{k}_fold"])
    lab = emulation.kfold_labels(7, 3)                  # the first N % k folds are one larger
    np.testing.assert_array_equal(lab, [0, 0, 0, 1, 1, 2, 2])


@pytest.mark.parametrize("N,k", [(10, 1), (10, 0), (10, 11), (3, -2)])
def test_kfold_labels_refuse_bad_k(N, k):
    from bayesian_inference import emulation
    with pytest.raises(ValueError):
        emulation.kfold_labels(N, k)


def _group_config(tmp_path, **keys):
    from bayesian_inference import emulation
    path, analysis = DU.write_config(tmp_path)
    analysis["parameters"]["emulators"]["main"].update(keys)
    return emulation.EmulationGroupConfig("test_analysis", "exponential", analysis, path, "main")


def test_config_keys_and_defaults(tmp_path):
    cfg = _group_config(tmp_path)
    assert cfg.cross_validation is False and cfg.cross_validation_k == 5
    cfg = _group_config(tmp_path, cross_validation=True, cross_validation_k=10)
    assert cfg.cross_validation is True and cfg.cross_validation_k == 10
    cfg = _group_config(tmp_path, cross_validation=False, cross_validation_k=5)
    assert cfg.cross_validation is False


@pytest.mark.parametrize("k", [1, 0, 2.5, "5", True])
def test_config_refuses_bad_k(tmp_path, k):
    with pytest.raises(ValueError):
        _group_config(tmp_path, cross_validation=True, cross_validation_k=k)


@pytest.mark.parametrize("fold", [
    np.zeros(10, dtype=int),                          # one fold
    np.r_[np.zeros(5, int), 2 * np.ones(5, int)],     # fold 1 empty
    np.r_[-1, np.zeros(9, int)],                      # negative label
    np.arange(11)[:10] + 1,                           # 11 folds > N (fold 0 empty too)
    np.zeros(9, dtype=int),                           # wrong length
    np.r_[0.5, np.zeros(9)],                          # not an integer
])
def test_fold_labels_refused_before_any_library_call(fold):
    from gpemu.model import DeviceModel
    with pytest.raises(ValueError):
        DeviceModel.check_folds(fold, 10)


def test_fold_labels_accepted():
    from gpemu.model import DeviceModel
    fold, n = DeviceModel.check_folds(np.array([2, 0, 1, 1, 0, 2]), 6)
    assert n == 3 and fold.dtype == np.int32


@pytest.mark.parametrize("case", R.CASES)
def test_closed_form_against_sklearn_golden(case):
    g9 = _g9()
    model, y, jitter, _ = R.case_model(case)
    N = y.shape[0]
    for k in (2, 5, N):
        m, v = R.closed_form_group(model, y, g9[f"{case}_k{k}_fold"], jitter)
        gm, gv = g9[f"{case}_k{k}_mean_pc"], g9[f"{case}_k{k}_var_pc"]
        assert np.max(np.abs(m - gm)) <= 1e-12 * np.max(np.abs(y)), (case, k)
        assert np.all(np.abs(v - gv) <= 1e-12 * np.abs(gv) + 1e-15), (case, k)


@pytest.mark.parametrize("case", ["g1_rbf_noise", "g1_matern25_const_noise", "g2_rbf_noise"])
def test_closed_form_against_brute_force_refits(case):
    model, y, jitter, _ = R.case_model(case)
    N = y.shape[0]
    rng = np.random.default_rng(3)
    for fold in (_kfold(N, 5), rng.permutation(_kfold(N, 4))):
        m, v = R.closed_form_group(model, y, fold, jitter)
        bm, bv = R.brute_force_group(model, y, fold, jitter)
        assert np.max(np.abs(m - bm)) <= 1e-12 * np.max(np.abs(y))
        assert np.all(np.abs(v - bv) <= 1e-12 * np.abs(bv) + 1e-15)


def _kfold(N, k):
    from bayesian_inference import emulation
    return emulation.kfold_labels(N, k)


def test_back_projection_matches_predict_group_at_one_point():
    model, _, _, _ = R.case_model("g1_matern25_const_noise")
    cu = O.cov_unexplained(model)
    x = model.X_train[:1] * 0.97 + 0.01
    m, v = O.gp_predict_all(x, model)
    cv, var = R.back_project(model, m, v, cu)
    ref = O.predict_group(x, model, cu)
    np.testing.assert_allclose(cv, ref["central_value"], rtol=1e-13, atol=1e-13 * np.max(np.abs(cv)))
    np.testing.assert_allclose(var[0], np.diag(ref["cov"][0]), rtol=1e-12)
