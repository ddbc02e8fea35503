"""CPU tests of the host side of the global (Sobol') sensitivity (no GPU): the estimators of tests/sobol_ref.py against
the closed form of an RBF emulator, gpemu.sensitivity.indices_from_moments against a brute-force numpy evaluation,
base_samples, the merge of emulation.global_sensitivity, the reference helpers and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

import sobol_ref as R
from oracle import gp_oracle as O

LD = np.longdouble


# ---- 1. the estimator against the closed form --------------------------------------------------------------------------
def test_estimators_against_the_closed_form_of_an_rbf_emulator():
    """V, V_i and VT_i of the centred estimators (float64 oracle means, 'random' base matrices, n = 4096) within 5 of
    their own standard errors (the sample standard deviation of the estimator's terms over sqrt of their number) of
    the exact integrals, for every feature and parameter"""
    from gpemu import sensitivity
    N, d, F, k, n = 100, 6, 40, 3, 4096
    model, lo, hi = R.problem(N, d, F, k, O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=False, has_noise=True), seed=1)
    V, Vi, VTi = R.rbf_closed_form(model, lo, hi)
    assert np.all(V > 0) and np.all(VTi >= Vi - 1e-12 * V) and np.all(Vi > -1e-12 * V)      # T_i >= S_i >= 0
    assert np.all(Vi.sum(axis=0) <= V * (1 + 1e-9)) and np.all(VTi.sum(axis=0) >= V * (1 - 1e-9))
    A, B = sensitivity.base_samples(n, lo, hi, seed=1, method="random")
    X = R.pick_freeze_rows(A, B)
    Z = O.gp_predict_all(X.reshape(-1, d), model)[0].reshape(d + 2, n, k)
    Y = (Z @ model.components[:k]) * model.scaler_scale + model.scaler_mean             # (d + 2, n, F)
    yAB = np.concatenate([Y[0], Y[1]])
    y0 = yAB.mean(axis=0)
    tV = (yAB - y0) ** 2
    worst = 0.0
    dev = np.abs(tV.mean(axis=0) - V) / (tV.std(axis=0, ddof=1) / np.sqrt(2 * n))
    worst = max(worst, dev.max())
    assert np.all(dev <= 5.0)
    for i in range(d):
        ti = (Y[1] - y0) * (Y[2 + i] - Y[0])
        tt = 0.5 * (Y[2 + i] - Y[0]) ** 2
        for terms, exact in ((ti, Vi[i]), (tt, VTi[i])):
            dev = np.abs(terms.mean(axis=0) - exact) / (terms.std(axis=0, ddof=1) / np.sqrt(n))
            worst = max(worst, dev.max())
            assert np.all(dev <= 5.0), i
    print(f"closed form: largest deviation {worst:.2f} standard errors")
    # the moment route of the reference and of gpemu.sensitivity gives the same estimates as the feature-space terms
    ref, _ = R.indices(Z, np.zeros(Z.shape), model, Z[0, :7].mean(axis=0), 4)
    mom = R.moments(Z, Z[0, :7].mean(axis=0), 4)
    out = sensitivity.indices_from_moments({key: np.asarray(v, dtype=np.float64) if key != "count" else v
                                            for key, v in mom.items() if key not in ("n", "n_batches")},
                                           model.components[:k], model.scaler_scale, model.scaler_mean)
    for i in range(d):
        assert np.allclose(out["first_order"][i], ((Y[1] - y0) * (Y[2 + i] - Y[0])).mean(axis=0) / tV.mean(axis=0),
                           rtol=1e-9, atol=1e-12)
    for key in ("first_order", "total", "variance", "mean", "first_order_se", "total_se"):
        assert np.allclose(out[key], np.asarray(ref[key], dtype=np.float64), rtol=1e-9, atol=1e-12), key
    assert np.allclose(out["variance"], tV.mean(axis=0), rtol=1e-10) and np.allclose(out["mean"], y0, rtol=1e-12)


# ---- 2. indices_from_moments against brute force ----------------------------------------------------------------------
def _brute(Z, comp, scale, smean, T):
    """the definitions row by row in feature space, numpy only"""
    s, n, k = Z.shape
    d = s - 2
    Y = (Z @ comp) * scale + smean

    def est(rows):
        yA, yB = Y[0][rows], Y[1][rows]
        y0 = np.concatenate([yA, yB]).mean(axis=0)
        V = np.concatenate([(yA - y0) ** 2, (yB - y0) ** 2]).mean(axis=0)
        S = np.array([((yB - y0) * (Y[2 + i][rows] - yA)).mean(axis=0) for i in range(d)]) / V
        Tt = np.array([((Y[2 + i][rows] - yA) ** 2).mean(axis=0) for i in range(d)]) / (2 * V)
        return V, S, Tt, y0

    V, S, Tt, y0 = est(np.arange(n))
    out = {"variance": V, "first_order": S, "total": Tt, "mean": y0}
    bt = (np.arange(n) * T) // n
    if T > 1:
        per = [est(np.flatnonzero(bt == t)) for t in range(T)]
        out["first_order_se"] = np.std([p[1] for p in per], axis=0, ddof=1) / np.sqrt(T)
        out["total_se"] = np.std([p[2] for p in per], axis=0, ddof=1) / np.sqrt(T)
    return out


@pytest.mark.parametrize("T", [1, 4, 16])
@pytest.mark.parametrize("pivot", [0.0, 1e3])
def test_indices_from_moments_against_a_brute_force_evaluation(T, pivot):
    from gpemu import sensitivity
    d, k, F, n = 3, 4, 7, 50                     # 50 rows in 4 or 16 batches: uneven batches (12 / 13, 3 / 4 rows)
    rng = np.random.default_rng(7)
    Z = rng.normal(size=(d + 2, n, k)) + np.array([3.0, -2.0, 0.5, 10.0])
    Z[2:] = Z[0] + 0.3 * rng.normal(size=(d, n, k)) * np.arange(1, d + 1)[:, None, None]
    comp, scale, smean = rng.normal(size=(k, F)), rng.uniform(0.5, 2.0, F), rng.normal(size=F)
    piv = np.full(k, pivot)
    mom = R.moments(Z, piv, T)
    counts = np.bincount((np.arange(n) * T) // n, minlength=T)
    assert np.array_equal(mom["count"], counts) and (T == 1 or counts.min() != counts.max())
    m64 = {key: (v if key in ("count", "n", "n_batches") else np.asarray(v, dtype=np.float64)) for key, v in mom.items()}
    out = sensitivity.indices_from_moments(m64, comp, scale, smean)
    ref = _brute(Z, comp, scale, smean, T)
    # a far pivot costs the cancellation |pivot|^2 u in the second moments: the reason the device centres near the mean
    rtol = 1e-10 if pivot == 0.0 else 1e-7
    for key in ("variance", "first_order", "total", "mean"):
        assert np.allclose(out[key], ref[key], rtol=rtol, atol=rtol), key
    assert out["first_order"].shape == (d, F) and out["total"].shape == (d, F) and out["variance"].shape == (F,)
    assert out["n"] == n and out["n_batches"] == T
    if T > 1:
        assert np.allclose(out["first_order_se"], ref["first_order_se"], rtol=10 * rtol, atol=10 * rtol)
        assert np.allclose(out["total_se"], ref["total_se"], rtol=10 * rtol, atol=10 * rtol)
    else:
        assert np.all(np.isnan(out["first_order_se"])) and np.all(np.isnan(out["total_se"]))


def test_a_feature_of_zero_variance_has_nan_indices_and_nothing_is_clipped():
    from gpemu import sensitivity
    d, k, F, n = 2, 2, 3, 40
    rng = np.random.default_rng(1)
    Z = rng.normal(size=(d + 2, n, k))
    comp = rng.normal(size=(k, F))
    comp[:, 1] = 0.0                                                  # feature 1 does not move
    mom = R.moments(Z, np.zeros(k), 2)
    m64 = {key: (v if key in ("count", "n", "n_batches") else np.asarray(v, dtype=np.float64)) for key, v in mom.items()}
    out = sensitivity.indices_from_moments(m64, comp, np.ones(F), np.zeros(F))
    assert out["variance"][1] == 0.0 and np.all(np.isnan(out["first_order"][:, 1])) and np.all(np.isnan(out["total"][:, 1]))
    assert np.all(np.isfinite(out["first_order"][:, [0, 2]]))
    assert (out["first_order"] < 0).any() or (out["total"] > 1).any()   # independent noise rows: estimates leave [0, 1]


# ---- 3. base_samples --------------------------------------------------------------------------------------------------
def test_base_samples():
    from scipy.stats import qmc

    from gpemu import sensitivity
    lo, hi = np.array([-1.0, 0.0, 2.0]), np.array([1.0, 0.5, 7.0])
    for method in ("sobol", "random"):
        A, B = sensitivity.base_samples(100, lo, hi, seed=3, method=method)
        assert A.shape == (100, 3) and B.shape == (100, 3) and A.flags.c_contiguous and B.flags.c_contiguous
        assert np.all(A >= lo) and np.all(A <= hi) and np.all(B >= lo) and np.all(B <= hi)
        A2, B2 = sensitivity.base_samples(100, lo, hi, seed=3, method=method)
        assert np.array_equal(A, A2) and np.array_equal(B, B2)
        A3, _ = sensitivity.base_samples(100, lo, hi, seed=4, method=method)
        assert not np.array_equal(A, A3)
        assert not np.array_equal(A, B) and np.abs(np.corrcoef(A[:, 0], B[:, 0])[0, 1]) < 0.3
    # 'sobol': A and B are the two halves of the columns of ONE scrambled sequence of dimension 2 d
    A, B = sensitivity.base_samples(64, lo, hi, seed=5)
    u = qmc.Sobol(d=6, scramble=True, seed=5).random(64)
    assert np.array_equal(A, lo + (hi - lo) * u[:, :3]) and np.array_equal(B, lo + (hi - lo) * u[:, 3:])
    # 'random': numpy's default_rng(seed)
    A, B = sensitivity.base_samples(10, lo, hi, seed=9, method="random")
    u = np.random.default_rng(9).random((2, 10, 3))
    assert np.array_equal(A, lo + (hi - lo) * u[0]) and np.array_equal(B, lo + (hi - lo) * u[1])
    for bad in (dict(n=0), dict(method="halton"), dict(lo=[0.0, 1.0]), dict(hi=[0.0, 0.0, 0.0]), dict(lo=[np.nan, 0, 0]),
                dict(lo=np.zeros(17), hi=np.ones(17))):
        kw = dict(n=8, lo=lo, hi=hi)
        kw.update(bad)
        with pytest.raises(ValueError):
            sensitivity.base_samples(**kw)


# ---- 4. the merge of global_sensitivity --------------------------------------------------------------------------------
def _fake_indices(d, F, base):
    v = base + np.arange(F, dtype=np.float64)
    m = v[None, :] + 1000.0 * np.arange(d)[:, None]
    return {"first_order": m, "total": m + 0.25, "first_order_se": m + 0.5, "total_se": m + 0.75, "variance": v + 0.1,
            "mean": v + 0.2, "n": 64, "n_batches": 4}


def test_global_sensitivity_merge_places_every_block_where_predict_places_the_central_value():
    import dropin_util as DU
    from bayesian_inference import emulation
    from test_posterior_predictive_host import _FakeSorter          # two groups of different F, interleaved
    d = 3
    groups = {"A": _fake_indices(d, 5, 100.0), "B": _fake_indices(d, 4, 200.0)}
    out = emulation.merge_global_sensitivity(_FakeSorter(), groups)
    order = [100, 101, 102, 200, 201, 202, 203, 103, 104]
    for i in range(d):
        assert out["first_order"][i].tolist() == [v + 1000.0 * i for v in order]
    assert np.array_equal(out["total"], out["first_order"] + 0.25)
    assert np.array_equal(out["first_order_se"], out["first_order"] + 0.5)
    assert np.array_equal(out["total_se"], out["first_order"] + 0.75)
    assert np.array_equal(out["variance"], np.array(order) + 0.1) and np.array_equal(out["mean"], np.array(order) + 0.2)
    assert out["n"] == 64 and out["n_batches"] == 4
    # ... which is where convert() places the groups' central_value
    cv = {"A": {"central_value": groups["A"]["first_order"]}, "B": {"central_value": groups["B"]["first_order"]}}
    sorter = emulation.SortEmulationGroupObservables(_FakeSorter.emulation_group_to_observable_matrix, (d, 9))
    assert np.array_equal(sorter.convert(cv)["central_value"], out["first_order"])
    # a sorter that only converts
    one = emulation.merge_global_sensitivity(DU.TrivialSort("main"), {"main": groups["A"]})
    for key in ("first_order", "total", "first_order_se", "total_se", "variance", "mean"):
        assert np.array_equal(one[key], groups["A"][key]), key
    # the posterior-predictive merge still goes through the same scatter
    rows = {"A": np.arange(10.0).reshape(2, 5), "B": 100 + np.arange(8.0).reshape(2, 4)}
    assert emulation.scatter_feature_rows(_FakeSorter(), rows)[1].tolist() == [5, 6, 7, 104, 105, 106, 107, 8, 9]


# ---- the reference helpers ---------------------------------------------------------------------------------------------
def test_reference_means_are_hp_refs_and_the_cases_carry_the_planted_rows():
    import hp_ref as H
    model, lo, hi, A, B = R.case("rbf_d1")
    assert A.shape == (R.N_BASE, 1) and np.array_equal(A[0], model.X_train[3]) and B[1, 0] == model.X_train[5, 0]
    X = R.pick_freeze_rows(A[:5], B[:5]).reshape(-1, 1)
    mean, _, mb, _, _ = H.gp_predict(X, model, cx=R.c_x_pf(1))
    Z, eps = R.pc_means(model, X, cx=R.c_x_pf(1))
    assert np.array_equal(np.asarray(mean, dtype=np.float64), np.asarray(Z, dtype=np.float64)) and np.array_equal(mb, eps)
    model, lo, hi, A, B = R.case("matern05_d6")
    c = 2
    X = R.pick_freeze_rows(A[:2], B[:2])
    assert np.array_equal(X[2 + c, 1], model.X_train[5]) and not np.array_equal(X[0, 1], model.X_train[5])
    assert np.all(A >= lo) and np.all(A <= hi)
    ls = np.stack([gp.ls for gp in model.gps])
    assert len({tuple(row) for row in ls}) == model.n_pc              # per-PC length scales
    assert R.c_x_pf(6) == 36.0 and R.c_x_pf(16) == 56.0
    assert [R.moment_rows(n) for n in ("rbf_d6", "rbf_const_d8", "matern25_d9", "rbf_d16")] == [257, 129, 129, 65]


# ---- the C ABI's declarations -------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_cite_the_reference():
    from gpemu import _lib
    from gpemu.sensitivity import SOBOL_PATHS, sobol_workspace_bytes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gpemu.h")).read()
    declared = set(re.findall(r"\b(gpemu_[a-z0-9_]+)\s*\(", hdr))
    for name in ("gpemu_gp_mean_pick_freeze", "gpemu_sobol_moments", "gpemu_sobol_moments_dev", "gpemu_sobol_path_counts"):
        assert name in declared and name in _lib.exported_symbols(), name
    assert "plot_qhat.py:172-258" in hdr
    enum = re.search(r"enum gpemu_sobol_path \{(.*?)\};", hdr, re.S).group(1)
    names = re.findall(r"GPEMU_SOBOL_PATH_([A-Z0-9]+)", enum)
    assert [n.lower() for n in names[:-1]] == list(SOBOL_PATHS) and names[-1] == "COUNT"
    src = open(os.path.join(root, "bayesian-inference_amd", "csrc", "Makefile")).read()
    assert "k_sobol.hip" in src
    assert sobol_workspace_bytes(1000, 6, 10) == 8 * 1000 * 8 * 10
