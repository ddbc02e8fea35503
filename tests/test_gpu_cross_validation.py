"""-m gpu tests of cross-validation at the fitted hyper-parameters on the device (gpemu_model_cross_validate,
DeviceModel.cross_validate, emulation.cross_validate) against scikit-learn (golden G9), the numpy
restatement (tests/cv_ref.py) and brute-force oracle refits."""
import pickle

import numpy as np
import pytest

import cv_ref as R
import dropin_util as DU
import golden_util as GU
from oracle import gp_oracle as O
from oracle.workloads import fixed_theta_model

pytestmark = pytest.mark.gpu
MTOL = 1e-9          # mean: 1e-9 max|y|
VREL, VABS = 1e-9, 1e-14


def _check(m, v, rm, rv, y, what):
    dm = np.max(np.abs(m - rm))
    assert dm <= MTOL * np.max(np.abs(y)), f"{what}: mean off by {dm:.3e}"
    bad = np.abs(v - rv) > VREL * np.abs(rv) + VABS
    assert not bad.any(), f"{what}: var off by {np.max(np.abs(v - rv)):.3e} at {np.argwhere(bad)[:3].tolist()}"


def _kfold(N, k):
    from bayesian_inference import emulation
    return emulation.kfold_labels(N, k)


@pytest.mark.parametrize("case", R.CASES)
def test_golden_parity(case):
    g9 = GU.load("g9_cross_validation")
    model, y, jitter, _ = R.case_model(case)
    dm = GU.device_model(model)
    cu = O.cov_unexplained(model)
    N = y.shape[0]
    for k in (2, 5, N):
        fold = g9[f"{case}_k{k}_fold"]
        m, v, cv, var = dm.cross_validate(y, fold)
        _check(m, v, g9[f"{case}_k{k}_mean_pc"], g9[f"{case}_k{k}_var_pc"], y, f"{case} k={k}")
        # observable space: the back-projection of the device's own PC-space results, and of the golden's
        rcv, rvar = R.back_project(model, m, v, cu)
        np.testing.assert_allclose(cv, rcv, rtol=0, atol=1e-12 * np.max(np.abs(rcv)))
        np.testing.assert_allclose(var, rvar, rtol=1e-12, atol=0)
        gcv, gvar = R.back_project(model, g9[f"{case}_k{k}_mean_pc"], g9[f"{case}_k{k}_var_pc"], cu)
        assert np.max(np.abs(cv - gcv)) <= MTOL * np.max(np.abs(gcv))
        assert np.all(np.abs(var - gvar) <= VREL * np.abs(gvar) + VABS)
    dm.close()


def _ragged(sizes, seed):
    lab = np.repeat(np.arange(len(sizes)), sizes)
    return np.random.default_rng(seed).permutation(lab)


@pytest.mark.parametrize("N,fold_kind", [
    (130, "loo"),              # m = 1 (the LOO kernel)
    (150, 10),                 # m = 15
    (176, 11),                 # m = 16
    (189, 3),                  # m = 63
    (200, "ragged"),           # m in {15, 16, 63, 64, 42}, shuffled
    (195, 3),                  # m = 65
    (400, 2),                  # m = 200
    (97, "ragged2"),           # a single point next to large folds: the general path with m = 1 folds
])
def test_shapes_against_brute_force_refits(N, fold_kind):
    model, prob, pca = fixed_theta_model(N, 24, 3, seed=N)
    y = pca["Y_pca"][:, :3]
    if fold_kind == "loo":
        fold = np.arange(N)
    elif fold_kind == "ragged":
        fold = _ragged([15, 16, 63, 64, 42], seed=1)
    elif fold_kind == "ragged2":
        fold = _ragged([1, 30, 66], seed=2)
    else:
        fold = _kfold(N, fold_kind)
    dm = GU.device_model(model)
    m, v, cv, var = dm.cross_validate(y, fold)
    bm, bv = R.brute_force_group(model, y, fold, 1e-10)
    _check(m, v, bm, bv, y, f"N={N} folds={fold_kind}")
    rcv, rvar = R.back_project(model, bm, bv, O.cov_unexplained(model))
    assert np.max(np.abs(cv - rcv)) <= MTOL * np.max(np.abs(rcv))
    assert np.all(np.abs(var - rvar) <= VREL * np.abs(rvar) + VABS)
    dm.close()


def test_c3_size_and_reproducible():
    model, prob, pca = fixed_theta_model(1000, 100, 10, seed=0)
    y = pca["Y_pca"][:, :10]
    fold = _kfold(1000, 5)
    dm = GU.device_model(model)
    out1 = dm.cross_validate(y, fold)
    out2 = dm.cross_validate(y, fold)
    for a, b in zip(out1, out2):
        assert a.tobytes() == b.tobytes()
    rm, rv = R.closed_form_group(model, y, fold, 1e-10)
    _check(out1[0], out1[1], rm, rv, y, "C3 k=5")
    dm.close()


def test_chunks_give_the_same_bits(monkeypatch):
    model, prob, pca = fixed_theta_model(2000, 40, 4, seed=5)
    y = pca["Y_pca"][:, :4]
    fold = _kfold(2000, 2)
    dm = GU.device_model(model)
    one = dm.cross_validate(y, fold)
    monkeypatch.setenv("GPEMU_CV_CHUNK", "3")          # 8 problems -> chunks of 3, 3, 2 (one straddles the folds)
    many = dm.cross_validate(y, fold)
    for a, b in zip(one, many):
        assert a.tobytes() == b.tobytes()
    rm, rv = R.closed_form_group(model, y, fold, 1e-10)
    _check(one[0], one[1], rm, rv, y, "N=2000 k=2")
    dm.close()


def test_bad_folds_refused():
    from gpemu import _lib
    model, prob, pca = fixed_theta_model(40, 8, 2, seed=1)
    y = pca["Y_pca"][:, :2]
    dm = GU.device_model(model)
    for fold in (np.zeros(40, int), np.r_[np.zeros(20, int), 2 * np.ones(20, int)]):
        with pytest.raises(ValueError):
            dm.cross_validate(y, fold)
    # the C ABI refuses them on its own too
    L = _lib.lib()
    out = [np.empty((40, 2)) for _ in range(2)]
    for n_folds, fold in ((1, np.zeros(40, np.int32)), (3, np.r_[np.zeros(20), 2 * np.ones(20)].astype(np.int32)),
                          (2, np.r_[np.zeros(39), 5].astype(np.int32)), (41, np.arange(40, dtype=np.int32))):
        rc = L.gpemu_model_cross_validate(dm.handle, n_folds, _lib.ptr(fold), _lib.ptr(np.ascontiguousarray(y)),
                                          _lib.ptr(out[0]), _lib.ptr(out[1]), None, None)
        assert rc == -1, (n_folds, rc)
    dm.close()


def _g7_results(g, name):
    prefix = name + "_"
    sub = {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}
    sub["gpr_alpha"] = g["gpr_alpha"]
    res = DU.results_at_golden_theta(sub, design=g["design"])
    res["PCA"]["Y"] = sub["Y"]
    return res


class _GroupCfg:
    def __init__(self, n_pc, k):
        self.n_pc, self.cross_validation_k, self.analysis_config = n_pc, k, {}


class _EmuCfg:
    def __init__(self, groups, sorter):
        self.emulation_groups_config = groups
        self.sort_observables_in_matrix = sorter

    def _need_groups(self, what):
        pass


def test_several_groups_merged():
    from bayesian_inference import emulation
    g = GU.load("g7_shipped_config")
    names, mapping, _, _ = GU.g7_groups(g)
    results = {n: _g7_results(g, n) for n in names}
    groups = {n: _GroupCfg(int(g[n + "_n_pc"]), 5) for n in names}
    sorter = emulation.SortEmulationGroupObservables(mapping, tuple(int(s) for s in g["map_shape"]))
    out = emulation.cross_validate(_EmuCfg(groups, sorter), results)
    F = int(g["map_shape"][1])
    assert out["central_value"].shape == (200, F) and out["variance"].shape == (200, F)
    np.testing.assert_array_equal(out["fold"], _kfold(200, 5))
    models = GU.g7_models(g)
    for n in names:
        per = emulation.cross_validate_emulator_group(groups[n], results[n])
        assert per["mean_pc"].tobytes() == out["mean_pc"][n].tobytes()
        for obs, (grp, so, sg) in mapping.items():
            if grp == n:
                assert out["central_value"][:, so].tobytes() == per["central_value"][:, sg].tobytes()
                assert out["variance"][:, so].tobytes() == per["variance"][:, sg].tobytes()
        rm, rv = R.closed_form_group(models[n], g[n + "_Y_pca_truncated"], out["fold"], float(g["gpr_alpha"]))
        _check(per["mean_pc"], per["var_pc"], rm, rv, g[n + "_Y_pca_truncated"], n)
    Y = emulation.SortEmulationGroupObservables(mapping, sorter.shape).convert(
        {n: {"Y": results[n]["PCA"]["Y"]} for n in names})["Y"]
    assert out["residual"].tobytes() == (Y - out["central_value"]).tobytes()
    assert 0.0 <= out["coverage"] <= 1.0 and np.all(np.isfinite(out["mean_z2"]))


CV_KEYS = {"fold", "n_folds", "mean_pc", "var_pc", "central_value", "variance", "residual", "z", "rmse", "mean_z2",
           "mean_z2_pc", "chi2_pc", "coverage", "confidence"}


@pytest.mark.parametrize("setting", ["on", "off", "absent"])
def test_dropin_fit_emulators_pickle(tmp_path, setting):
    from bayesian_inference import emulation
    g = GU.load("g1_rbf_noise")
    DU.install_fake_data_IO(g["Y"], g["design"], g["y_exp"], g["y_err"], {})
    path, analysis = DU.write_config(tmp_path, kernels_active=("rbf", "noise"), n_pc=5, n_restarts=1)
    block = analysis["parameters"]["emulators"]["main"]
    if setting != "absent":
        block["cross_validation"] = setting == "on"
        block["cross_validation_k"] = 5
    ec = emulation.EmulationConfig.from_config_file("test_analysis", "exponential", path, analysis)
    np.random.seed(12345)
    emulation.fit_emulators(ec)
    cfg = ec.emulation_groups_config["main"]
    res = pickle.loads(open(cfg.emulation_outputfile, "rb").read())
    if setting != "on":
        assert set(res) == {"PCA", "emulators"}
        return
    assert set(res) == {"PCA", "emulators", "cross_validation"}
    cv = res["cross_validation"]
    assert set(cv) == CV_KEYS
    N, F = g["Y"].shape
    assert cv["n_folds"] == 5 and cv["fold"].shape == (N,)
    assert cv["mean_pc"].shape == (N, 5) and cv["var_pc"].shape == (N, 5)
    for key in ("central_value", "variance", "residual", "z"):
        assert cv[key].shape == (N, F)
    assert cv["rmse"].shape == (F,) and cv["mean_z2"].shape == (F,) and cv["chi2_pc"].shape == (N,)
    assert np.all(np.isfinite(cv["mean_z2"])) and np.all(np.isfinite(cv["mean_z2_pc"]))
    assert cv["confidence"] == 0.9
