"""CPU tests of the host side of the second-order Sobol' indices (no GPU): the pair estimators against
the closed form of an RBF emulator (tests/sobol_pairs_ref.py), gpemu.sensitivity.pair_indices_from_moments against a
row-by-row longdouble evaluation, two analytic checks (d = 2; an additive function), interacting_pairs, the defaults
of the new keywords, the reference's own helpers and the C ABI's declarations."""
import inspect
import os
import re

import numpy as np
import pytest

import sobol_pairs_ref as PR
import sobol_ref as R
from oracle import gp_oracle as O

LD = np.longdouble
FIRST_KEYS = {"first_order", "total", "first_order_se", "total_se", "variance", "mean", "n", "n_batches"}
PAIR_KEYS = {"pairs", "closed_pair", "interaction", "total_pair", "closed_pair_se", "interaction_se", "total_pair_se"}


def _m64(mom):
    keep = ("count", "n", "n_batches", "pairs")
    return {key: (v if key in keep else np.asarray(v, dtype=np.float64)) for key, v in mom.items()}


# ---- 1. the estimators against the closed form -----------------------------------------------------------------------------
def _batch_means_se(terms, T):
    """batch-means standard error of the mean of ``terms`` (n, ...): batches floor(r T / n), ddof 1, / sqrt(T)"""
    bt = R.batch_of(terms.shape[0], T)
    per = np.array([terms[bt == t].mean(axis=0) for t in range(T)])
    return per.std(axis=0, ddof=1) / np.sqrt(T)


def test_pair_estimators_against_the_closed_form_of_an_rbf_emulator():
    """Sc_ij V, T_ij V and the interaction's variance of the centred estimators (float64 oracle means, 'random' base
    matrices, n = 4096, test_sobol_host.py's shape with the pair rows added) within 5 of their own batch-means standard
    errors (16 batches) of the exact integrals, for every feature and pair; and the moment route gives the estimates"""
    from gpemu import sensitivity
    N, d, F, k, n, T = 100, 6, 40, 3, 4096, 16
    model, lo, hi = R.problem(N, d, F, k, O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=False, has_noise=True), seed=1)
    pairs = PR.all_pairs(d)
    V, Vc, VT = PR.rbf_closed_form_pairs(model, lo, hi, pairs)
    V1, Vi, VTi = R.rbf_closed_form(model, lo, hi)
    assert np.allclose(V, V1, rtol=1e-12)
    Vint = Vc - Vi[pairs[:, 0]] - Vi[pairs[:, 1]]
    # a closed index is monotone in its set, the interaction variance of two parameters is non-negative, the total of
    # a pair lies between the larger and the sum of its members' totals
    assert np.all(Vint >= -1e-12 * V) and np.all(Vc <= V * (1 + 1e-9))
    assert np.all(VT >= np.maximum(VTi[pairs[:, 0]], VTi[pairs[:, 1]]) - 1e-12 * V)
    assert np.all(VT <= VTi[pairs[:, 0]] + VTi[pairs[:, 1]] + 1e-12 * V) and np.all(VT >= Vc - 1e-12 * V)
    A, B = sensitivity.base_samples(n, lo, hi, seed=1, method="random")
    X = PR.all_rows(A, B, pairs)
    Z = O.gp_predict_all(X.reshape(-1, d), model)[0].reshape(d + 2 + len(pairs), n, k)
    Y = (Z @ model.components[:k]) * model.scaler_scale + model.scaler_mean
    y0 = np.concatenate([Y[0], Y[1]]).mean(axis=0)
    ti = [(Y[1] - y0) * (Y[2 + i] - Y[0]) for i in range(d)]
    worst = 0.0
    for q, (i, j) in enumerate(pairs):
        Dij = Y[2 + d + q] - Y[0]
        tc = (Y[1] - y0) * Dij
        for what, terms, exact in (("closed", tc, Vc[q]), ("total", 0.5 * Dij ** 2, VT[q]),
                                   ("interaction", tc - ti[i] - ti[j], Vint[q])):
            dev = np.abs(terms.mean(axis=0) - exact) / _batch_means_se(terms, T)
            worst = max(worst, dev.max())
            assert np.all(dev <= 5.0), (what, i, j, dev.max())
    print(f"closed form of the pairs: largest deviation {worst:.2f} batch-means standard errors")
    # the moment route of the reference and of gpemu.sensitivity gives the feature-space estimates
    piv = Z[0, :7].mean(axis=0)
    mom = _m64(dict(PR.moments(Z, d, piv, T), pairs=pairs))
    out = sensitivity.pair_indices_from_moments(mom, model.components[:k], model.scaler_scale, model.scaler_mean)
    Vhat = np.concatenate([(Y[0] - y0) ** 2, (Y[1] - y0) ** 2]).mean(axis=0)
    for q, (i, j) in enumerate(pairs):
        Dij = Y[2 + d + q] - Y[0]
        assert np.allclose(out["closed_pair"][q], ((Y[1] - y0) * Dij).mean(axis=0) / Vhat, rtol=1e-9, atol=1e-12)
        assert np.allclose(out["total_pair"][q], 0.5 * (Dij ** 2).mean(axis=0) / Vhat, rtol=1e-9, atol=1e-12)
    ref, _ = PR.indices(Z, np.zeros(Z.shape), model, pairs, piv, T)
    for key in sorted(PAIR_KEYS - {"pairs"}):
        assert np.allclose(out[key], np.asarray(ref[key], dtype=np.float64), rtol=1e-9, atol=1e-12), key


# ---- 2. pair_indices_from_moments row by row --------------------------------------------------------------------------------
def _brute(Z, d, pairs, comp, scale, smean, T):
    """the definitions row by row in feature space, in longdouble"""
    Y = (np.asarray(Z, dtype=LD) @ np.asarray(comp, dtype=LD)) * np.asarray(scale, dtype=LD) + np.asarray(smean, dtype=LD)
    n = Y.shape[1]

    def est(rows):
        yA, yB = Y[0][rows], Y[1][rows]
        y0 = np.concatenate([yA, yB]).mean(axis=0)
        V = np.concatenate([(yA - y0) ** 2, (yB - y0) ** 2]).mean(axis=0)
        S = np.array([((yB - y0) * (Y[2 + i][rows] - yA)).mean(axis=0) for i in range(d)]) / V
        Sc = np.array([((yB - y0) * (Y[2 + d + q][rows] - yA)).mean(axis=0) for q in range(len(pairs))]) / V
        Tp = np.array([((Y[2 + d + q][rows] - yA) ** 2).mean(axis=0) for q in range(len(pairs))]) / (2 * V)
        return Sc, Sc - S[pairs[:, 0]] - S[pairs[:, 1]], Tp

    names = ("closed_pair", "interaction", "total_pair")
    out = dict(zip(names, est(np.arange(n))))
    if T > 1:
        bt = (np.arange(n) * T) // n
        per = [est(np.flatnonzero(bt == t)) for t in range(T)]
        for a, key in enumerate(names):
            out[key + "_se"] = np.std(np.array([p[a] for p in per]), axis=0, ddof=1) / np.sqrt(LD(T))
    return out


@pytest.mark.parametrize("T", [1, 4, 16])
@pytest.mark.parametrize("pivot", [0.0, 1e3])
def test_pair_indices_from_moments_against_a_row_by_row_evaluation(T, pivot):
    from gpemu import sensitivity
    d, k, F, n = 4, 3, 7, 50                     # 50 rows in 4 or 16 batches: uneven batches (12 / 13, 3 / 4 rows)
    pairs = np.array([(0, 1), (1, 3), (0, 3), (2, 3)])                # a subset, not in row-major order
    rng = np.random.default_rng(11)
    Z = rng.normal(size=(d + 2 + len(pairs), n, k)) + np.array([3.0, -2.0, 10.0])
    Z[2:] = Z[0] + 0.3 * rng.normal(size=(d + len(pairs), n, k)) * np.arange(1, d + len(pairs) + 1)[:, None, None]
    comp, scale, smean = rng.normal(size=(k, F)), rng.uniform(0.5, 2.0, F), rng.normal(size=F)
    mom = PR.moments(Z, d, np.full(k, pivot), T)
    counts = np.bincount((np.arange(n) * T) // n, minlength=T)
    assert np.array_equal(mom["count"], counts) and (T == 1 or counts.min() != counts.max())
    assert mom["M2"].shape == (T, len(pairs), k, k) and mom["sumD2"].shape == (T, len(pairs), k)
    out = sensitivity.pair_indices_from_moments(_m64(dict(mom, pairs=pairs)), comp, scale, smean)
    ref = _brute(Z, d, pairs, comp, scale, smean, T)
    assert set(out) == PAIR_KEYS and np.array_equal(out["pairs"], pairs)
    # a far pivot costs the cancellation |pivot|^2 u in the second moments: the reason the device centres near the mean
    rtol = 1e-10 if pivot == 0.0 else 1e-7
    for key in ("closed_pair", "interaction", "total_pair"):
        assert out[key].shape == (len(pairs), F)
        assert np.allclose(out[key], np.asarray(ref[key], dtype=np.float64), rtol=rtol, atol=rtol), key
        if T > 1:
            assert np.allclose(out[key + "_se"], np.asarray(ref[key + "_se"], dtype=np.float64), rtol=10 * rtol,
                               atol=10 * rtol), key
        else:
            assert np.all(np.isnan(out[key + "_se"])), key
    # the first-order keys of the same dict are untouched by the extra moments
    a = sensitivity.indices_from_moments(_m64(dict(mom, pairs=pairs)), comp, scale, smean)
    b = sensitivity.indices_from_moments(_m64(R.moments(Z[:2 + d], np.full(k, pivot), T)), comp, scale, smean)
    assert set(a) == FIRST_KEYS and all(np.array_equal(a[key], b[key], equal_nan=True) for key in FIRST_KEYS)


def test_a_feature_of_zero_variance_has_nan_pair_indices_and_nothing_is_clipped():
    from gpemu import sensitivity
    d, k, F, n = 3, 2, 3, 40
    pairs = PR.all_pairs(d)
    rng = np.random.default_rng(2)
    Z = rng.normal(size=(d + 2 + len(pairs), n, k))
    comp = rng.normal(size=(k, F))
    comp[:, 1] = 0.0
    out = sensitivity.pair_indices_from_moments(_m64(dict(PR.moments(Z, d, np.zeros(k), 2), pairs=pairs)), comp,
                                                np.ones(F), np.zeros(F))
    for key in ("closed_pair", "interaction", "total_pair"):
        assert np.all(np.isnan(out[key][:, 1])) and np.all(np.isfinite(out[key][:, [0, 2]])), key
    assert (out["closed_pair"] < 0).any() or (out["total_pair"] > 1).any()   # independent noise rows leave [0, 1]


# ---- 3. analytic checks --------------------------------------------------------------------------------------------------
def _indices_of(fn, d, pairs, n, T, seed):
    """first- and second-order results of the k outputs of ``fn`` (rows -> (rows, k)) over the unit box"""
    from gpemu import sensitivity
    rng = np.random.default_rng(seed)
    A, B = rng.random((n, d)), rng.random((n, d))
    X = PR.all_rows(A, B, pairs)
    Z = fn(X.reshape(-1, d)).reshape(X.shape[0], n, -1)
    k = Z.shape[2]
    comp = np.random.default_rng(seed + 1).normal(size=(k, 5))
    mom = _m64(dict(PR.moments(Z, d, Z[0, :16].mean(axis=0), T), pairs=pairs))
    args = (comp, np.ones(5), np.zeros(5))
    return sensitivity.indices_from_moments(mom, *args), sensitivity.pair_indices_from_moments(mom, *args)


def test_at_two_parameters_the_pair_explains_everything():
    """d = 2: AB_01 is B, so Var E[y | x_0, x_1] = V and the pair's total effect is V: both indices 1 within 5 errors"""
    fn = lambda x: np.stack([4 * (x[:, 0] - 0.5) * (x[:, 1] - 0.5) + 0.3 * x[:, 0], np.cos(6 * x[:, 0] * x[:, 1]),
                             np.sin(5 * (x[:, 0] - x[:, 1]) ** 2)], axis=1)
    _, out = _indices_of(fn, 2, PR.all_pairs(2), 4096, 16, seed=3)
    for key in ("closed_pair", "total_pair"):
        dev = np.abs(out[key] - 1.0) / out[key + "_se"]
        print(f"d = 2 {key}: {out[key].ravel()}, largest deviation {dev.max():.2f} standard errors")
        assert np.all(dev <= 5.0), key
    assert np.all(out["interaction"] > 5 * out["interaction_se"])      # x_0 x_1 terms: a real interaction


def test_an_additive_function_has_no_interaction():
    """y = sum_l g_l(x_l): D_ij = D_i + D_j row by row, so the estimator itself gives closed_pair = S_i + S_j: the
    interaction and its own error are 0 up to the rounding of the float64 moments (1e-12 here: moments of O(n) terms
    of O(1) over V of O(0.1)), while the closed index is far from 0 and the sum of the three errors is not small"""
    d = 4
    fn = lambda x: np.stack([np.sin(3 * x[:, 0]) + x[:, 1] ** 2 + 0.5 * x[:, 2] + np.exp(x[:, 3]),
                             x[:, 0] - np.cos(4 * x[:, 1]) + x[:, 2] ** 3 + 0.1 * x[:, 3]], axis=1)
    first, out = _indices_of(fn, d, PR.all_pairs(d), 4096, 16, seed=5)
    dev = np.abs(out["interaction"]) / out["interaction_se"]
    print(f"additive: largest |interaction| {np.abs(out['interaction']).max():.3e}, {dev.max():.2f} standard errors")
    assert np.all(np.abs(out["interaction"]) <= 5.0 * out["interaction_se"] + 1e-12)
    assert np.all(out["closed_pair"] > 5 * out["closed_pair_se"])
    # the interaction's error comes from the difference itself, not from adding three errors
    three = out["closed_pair_se"] + first["first_order_se"][out["pairs"][:, 0]] + first["first_order_se"][out["pairs"][:, 1]]
    assert np.all(out["interaction_se"] <= 1e-12) and np.all(three > 1e-3)


# ---- 4. interacting_pairs -----------------------------------------------------------------------------------------------
def test_interacting_pairs_on_a_constructed_result():
    from gpemu import sensitivity
    d, F = 5, 3
    S = np.full((d, F), 0.1)
    Tt = S.copy()
    se = np.full((d, F), 0.01)
    Tt[1, 2] += 0.07                               # 0.07 > 3 (0.01 + 0.01): acts through interactions, in one feature
    Tt[3, 0] += 0.30
    Tt[4, 1] += 0.05                               # 0.05 < 0.06: not at 3 sigma ...
    Tt[0, 0] = np.nan                              # a feature of zero variance flags nothing
    res = {"first_order": S, "total": Tt, "first_order_se": se, "total_se": se}
    assert sensitivity.interacting_pairs(res).tolist() == [[1, 3]]
    assert sensitivity.interacting_pairs(res, n_sigma=2).tolist() == [[1, 3], [1, 4], [3, 4]]     # ... but at 2
    none = sensitivity.interacting_pairs(dict(res, total=S))
    assert none.shape == (0, 2) and none.dtype == np.int64
    one_batch = dict(res, first_order_se=np.full((d, F), np.nan), total_se=np.full((d, F), np.nan))
    assert sensitivity.interacting_pairs(one_batch).shape == (0, 2)
    with pytest.raises(ValueError):
        sensitivity.interacting_pairs(res, n_sigma=-1)


def test_check_pairs():
    from gpemu import marginals, sensitivity
    assert np.array_equal(sensitivity.check_pairs(None, 4), marginals.pair_indices(4))
    assert np.array_equal(PR.all_pairs(6), marginals.pair_indices(6))
    got = sensitivity.check_pairs([(2, 3), (0, 1)], 4)
    assert got.dtype == np.int64 and got.tolist() == [[2, 3], [0, 1]]
    for bad, d in (([(1, 1)], 4), ([(2, 1)], 4), ([(0, 4)], 4), ([(-1, 2)], 4), ([(0, 1), (0, 1)], 4), ([], 4),
                   ([0, 1], 4), ([(0.5, 1)], 4), (None, 1), ([(0, 1)], 1)):
        with pytest.raises(ValueError):
            sensitivity.check_pairs(bad, d)


# ---- 5. settings and defaults -----------------------------------------------------------------------------------------------
class _OldModel:
    """a model with the signature of before the keywords: the pass-through may send nothing new by default"""

    def sobol_indices(self, A, B, n_batches=16, workspace_bytes=0):
        from test_sobol_host import _fake_indices
        return _fake_indices(A.shape[1], 4, 100.0)


class _NewModel:
    def __init__(self):
        self.calls = []

    def sobol_indices(self, A, B, n_batches=16, workspace_bytes=0, second_order=False, pairs=None):
        from test_sobol_host import _fake_indices
        self.calls.append((second_order, pairs))
        out = _fake_indices(A.shape[1], 4, 100.0)
        if second_order:
            P = len(pairs) if pairs is not None else A.shape[1] * (A.shape[1] - 1) // 2
            base = np.arange(4.0)[None, :] + 10.0 * np.arange(P)[:, None]
            out.update(pairs=PR.all_pairs(A.shape[1])[:P] if pairs is None else np.asarray(pairs),
                       **{key: base + a for a, key in enumerate(sorted(PAIR_KEYS - {"pairs"}))})
        return out


class _GroupCfg:
    n_pc = 2


class _EmuCfg:
    emulation_groups_config = {"main": _GroupCfg()}
    analysis_config = {"parameterization": {"p": {"names": ["a", "b", "c"], "min": [0.0, 0.0, 0.0], "max": [1.0, 2.0, 3.0]}}}
    parameterization = "p"

    def __init__(self):
        import dropin_util as DU
        self.sort_observables_in_matrix = DU.TrivialSort("main")


def test_without_second_order_the_key_sets_and_the_calls_are_todays(monkeypatch):
    from bayesian_inference import emulation
    from gpemu import model, sensitivity
    A = B = np.zeros((8, 3))
    assert set(sensitivity.sobol_indices(_OldModel(), A, B)) == FIRST_KEYS
    assert set(sensitivity.sobol_indices({"g": _OldModel()}, A, B, n_batches=4)["g"]) == FIRST_KEYS
    new = _NewModel()
    assert set(sensitivity.sobol_indices(new, A, B, second_order=True, pairs=[(0, 2)])) == FIRST_KEYS | PAIR_KEYS
    assert new.calls == [(True, [(0, 2)])]
    for fn in (model.DeviceModel.sobol_indices, sensitivity.sobol_indices, emulation.global_sensitivity):
        par = inspect.signature(fn).parameters
        assert par["second_order"].default is False and par["pairs"].default is None, fn
    par = inspect.signature(model.DeviceModel.sobol_moments_pairs).parameters
    assert list(par)[1:] == ["A", "B", "pairs", "n_batches", "workspace_bytes"]
    assert par["pairs"].default is None and par["n_batches"].default == 16 and par["workspace_bytes"].default == 0
    # the drop-in: the first-order call reaches the model as before and returns today's keys; second_order adds seven
    old = _OldModel()
    monkeypatch.setattr(emulation, "device_model_for", lambda result, n_pc, cov=None: old)
    out = emulation.global_sensitivity(_EmuCfg(), n=8, n_batches=2, emulation_group_results={"main": {}})
    assert set(out) == FIRST_KEYS | {"parameter_names"}
    new = _NewModel()
    monkeypatch.setattr(emulation, "device_model_for", lambda result, n_pc, cov=None: new)
    out2 = emulation.global_sensitivity(_EmuCfg(), n=8, n_batches=2, emulation_group_results={"main": {}},
                                        second_order=True, pairs=[(0, 1), (1, 2)])
    assert set(out2) == FIRST_KEYS | {"parameter_names"} | PAIR_KEYS
    assert out2["pairs"].tolist() == [[0, 1], [1, 2]] and out2["closed_pair"].shape == (2, 4)
    for key in FIRST_KEYS - {"n", "n_batches"}:
        assert np.array_equal(out[key], out2[key]), key
    with pytest.raises(ValueError):
        emulation.global_sensitivity(_EmuCfg(), n=8, emulation_group_results={"main": {}}, pairs=[(0, 1)])


def test_the_pair_merge_places_every_block_where_predict_places_the_central_value():
    from bayesian_inference import emulation
    from test_posterior_predictive_host import _FakeSorter          # two groups of different F, interleaved
    P = 3
    keys = sorted(PAIR_KEYS - {"pairs"})

    def fake(F, base):
        m = base + np.arange(F, dtype=np.float64)[None, :] + 1000.0 * np.arange(P)[:, None]
        return dict({key: m + 0.125 * a for a, key in enumerate(keys)}, pairs=PR.all_pairs(3))

    out = emulation.merge_global_sensitivity_pairs(_FakeSorter(), {"A": fake(5, 100.0), "B": fake(4, 200.0)})
    order = [100, 101, 102, 200, 201, 202, 203, 103, 104]
    for a, key in enumerate(keys):
        for q in range(P):
            assert out[key][q].tolist() == [v + 1000.0 * q + 0.125 * a for v in order], key
    assert out["pairs"].tolist() == [[0, 1], [0, 2], [1, 2]] and set(out) == PAIR_KEYS


# ---- the reference helpers ---------------------------------------------------------------------------------------------------
def test_the_cases_carry_the_planted_pair_row_and_the_reference_is_sobol_refs():
    assert PR.c_x_pp(6) == 36.0 and PR.c_x_pp(16) == 56.0
    for name in ("rbf_d2", "matern05_d6", "rbf_d16"):
        model, lo, hi, A, B, pairs = PR.case(name)
        i, j = pairs[0]
        X = PR.all_rows(A[:3], B[:3], pairs)
        d = A.shape[1]
        x = model.X_train[PR.PLANT_TRAIN]
        assert np.array_equal(X[2 + d, PR.PLANT_ROW], x)                          # AB_ij ON the training point
        for s in (0, 2 + i, 2 + j):                                               # A, AB_i, AB_j are not
            assert not any(np.array_equal(X[s, PR.PLANT_ROW], t) for t in model.X_train), (name, s)
        assert np.all(A >= lo) and np.all(A <= hi) and np.all(B >= lo) and np.all(B <= hi)
    assert [tuple(p) for p in PR.case("rbf_d16")[5][:2]] == [(0, 15), (14, 15)] and len(PR.case("rbf_d16")[5]) == 5
    # rows 0, 1 are sobol_ref's planted rows, and away from row 2 the first d + 2 slots are sobol_ref's reference
    model, lo, hi, A, B, pairs = PR.case("matern15_d6")
    _, _, _, A0, B0 = R.case("matern15_d6")
    keep = np.arange(R.N_BASE) != PR.PLANT_ROW
    assert np.array_equal(A[keep], A0[keep]) and np.array_equal(B[keep], B0[keep])
    Z, eps = PR.means(model, A[:5], B[:5], pairs[:2])
    Z0, eps0 = R.case_means("matern15_d6")
    rows = [0, 1, 3, 4]
    assert np.array_equal(Z[:8, rows], Z0[:, rows]) and np.array_equal(eps[:8, rows], eps0[:, rows])
    # a pair row whose B column equals A's IS the first-order row
    Bs = B[:5].copy()
    Bs[:, 0] = A[:5, 0]
    assert np.array_equal(PR.pair_rows(A[:5], Bs, [(0, 3)])[0], R.pick_freeze_rows(A[:5], Bs)[2 + 3])


# ---- the C ABI's declarations ---------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    import ctypes as C

    from gpemu import _lib, sensitivity
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gpemu.h")).read()
    declared = set(re.findall(r"\b(gpemu_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in ("gpemu_sobol_moments_pairs", "gpemu_sobol_pairs_path_counts"):
        assert name in declared and name in _lib.exported_symbols() and hasattr(L, name), name
    proto = re.search(r"int gpemu_sobol_moments_pairs\((.*?)\);", hdr, re.S).group(1)
    assert proto.lstrip().startswith("gpemu_model *m") and "stream" not in proto and "gpemu_call_ctx" not in proto
    assert len(proto.split(",")) == len(_lib._SIGNATURES["gpemu_sobol_moments_pairs"][1]) == 19
    enum = re.search(r"enum gpemu_sobol_pairs_path \{(.*?)\};", hdr, re.S).group(1)
    names = re.findall(r"GPEMU_SOBOL_PAIRS_PATH_([A-Z0-9]+)", enum)
    assert [n.lower() for n in names[:-1]] == list(sensitivity.SOBOL_PAIRS_PATHS) and names[-1] == "COUNT"
    out = (C.c_int64 * 16)()
    assert L.gpemu_sobol_pairs_path_counts(out, 16) == len(sensitivity.SOBOL_PAIRS_PATHS)
    assert L.gpemu_sobol_pairs_path_counts(None, 16) == -1
    assert L.gpemu_sobol_path_counts(out, 16) == len(sensitivity.SOBOL_PATHS)          # the first order's set keeps its size
    assert sensitivity.sobol_pairs_workspace_bytes(1000, 6, 10, 15) == 8 * 1000 * (8 + 15) * 10
    assert sensitivity.sobol_workspace_bytes(1000, 6, 10) == 8 * 1000 * 8 * 10
