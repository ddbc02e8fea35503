"""Host tests of the LOO / WAIC reference (tests/loo_ref.py) and of the library's host-side logic (gpemu.loo, the YAML
settings, the declared symbols).  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import loo_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def _gpdfit64(a):
    """ArviZ's _gpdfit in float64, as numpy writes it: what the restated fit is compared with"""
    n = len(a)
    m = 30 + int(np.sqrt(n))
    b = 1 - np.sqrt(m / (np.arange(1, m + 1) - 0.5))
    b /= 3 * a[int(n / 4 + 0.5) - 1]
    b += 1 / a[-1]
    k = np.mean(np.log1p(-b[:, None] * a), axis=1)
    L = n * (np.log(-(b / k)) - k - 1)
    w = 1 / np.sum(np.exp(L - L[:, None]), axis=1)
    keep = w >= 10 * np.finfo(float).eps
    w, b = w[keep], b[keep]
    w /= w.sum()
    bp = np.sum(b * w)
    kp = np.mean(np.log1p(-bp * a))
    return (n * kp + 10 * 0.5) / (n + 10), -kp / bp


def test_the_restated_fit_approaches_the_true_shape_and_equals_the_float64_one():
    for ktrue, at2000, at100 in ((0.3, 0.3015, 0.329), (0.7, 0.6989, 0.680)):
        err = []
        for n in (100, 2000, 20000):
            t = R.gpd_quantile_sample(n, ktrue)
            khat, sigma = R.gpdfit(t)
            k64, s64 = _gpdfit64(np.asarray(t, dtype=np.float64))
            assert abs(float(khat) - k64) < 1e-9 and abs(float(sigma) - s64) < 1e-9, (ktrue, n)
            err.append(abs(float(khat) - ktrue))
            if n == 2000:
                assert round(float(khat), 4) == at2000
            if n == 100:
                assert round(float(khat), 3) == at100
        assert err[0] > err[1] > err[2], (ktrue, err)


@pytest.mark.parametrize("S,n", [(20, 4), (21, 5), (25, 5), (63, 13), (64, 13), (65, 13), (2049, 136), (100003, 949)])
def test_tail_length_rule(S, n):
    V = -1.5 * np.random.default_rng(S).standard_normal(S) ** 2      # continuous: no ties
    out = R.psis_row(V)
    assert out["n_tail"] == n == R.tail_size(S)
    if n <= 4:
        assert np.isinf(float(out["pareto_k"])) and float(out["pareto_k"]) > 0
        x = (-V) - np.max(-V)
        raw = x.astype(LD) - np.log(np.sum(np.exp(x.astype(LD))))
        assert np.max(np.abs(np.asarray(out["logw"] - raw, dtype=np.float64))) < 1e-17
    else:
        assert np.isfinite(float(out["pareto_k"]))
    # ties at the cutoff shorten the tail: the elements strictly above it
    V2 = V.copy()
    order = np.argsort(V2)                     # the largest ratios are the smallest V
    M = R.tail_size(S)
    if M >= 2:
        V2[order[M - 1]] = V2[order[M]]        # the tail's lowest element ties with the cutoff
        assert R.psis_row(V2)["n_tail"] == M - 1


def test_a_row_of_equal_values():
    for S in (1, 7, 300):
        out = R.psis_row(np.full(S, -3.25))
        assert out["n_tail"] == 0 and np.isinf(float(out["pareto_k"]))
        assert np.max(np.abs(np.asarray(out["logw"] + np.log(LD(S)), dtype=np.float64))) < 1e-18
        assert abs(float(out["elpd_loo"] + LD(3.25))) < 1e-17 and abs(float(out["lppd"] + LD(3.25))) < 1e-17
        if S > 1:
            assert float(out["p_waic"]) == 0.0
        else:
            assert math.isnan(float(out["p_waic"]))


def test_adding_a_constant_shifts_the_elpds_only():
    for c, S in ((0.05, 300), (0.5, 2049), (1.5, 2049)):
        # values on a grid of 2^-20 and a shift of 16: V + 16 is exact, so x = (-V) - max(-V) has the same bits
        V = np.round(R.synthetic_rows(1, S, c, seed=5)[0] * 2.0 ** 20) / 2.0 ** 20
        a, b = R.psis_row(V), R.psis_row(V + 16.0)
        assert a["n_tail"] == b["n_tail"] > 4 and float(a["cutoff"]) == float(b["cutoff"])
        for key in ("elpd_loo", "lppd", "elpd_waic"):
            print(f"c={c} {key}: shift error {abs(float(b[key] - a[key]) - 16.0):.3e}, bound {a['bound'][key]:.3e}")
            assert abs(float(b[key] - a[key]) - 16.0) <= a["bound"][key] + b["bound"][key], key
        for key in ("p_loo", "p_waic", "pareto_k", "ess_w"):
            assert abs(float(b[key] - a[key])) <= a["bound"][key] + b["bound"][key], key
        assert np.all(np.abs(np.asarray(b["logw"] - a["logw"], dtype=np.float64)) <= a["bound"]["logw"] + b["bound"]["logw"])


def test_repeated_samples_in_any_permutation():
    rng = np.random.default_rng(8)
    base = R.synthetic_rows(1, 600, 0.5, seed=9)[0]
    V = np.repeat(base, 4)
    a = R.psis_row(V)
    assert a["n_tail"] % 4 == 0 and a["n_tail"] > 4
    for _ in range(3):
        perm = rng.permutation(V.size)
        b = R.psis_row(V[perm])
        assert b["n_tail"] == a["n_tail"] and float(b["cutoff"]) == float(a["cutoff"])
        for key in ("elpd_loo", "lppd", "p_loo", "pareto_k", "ess_w", "p_waic", "elpd_waic"):
            assert abs(float(b[key] - a[key])) <= 1e-15 * max(1.0, abs(float(a[key]))), key
        # the tie rule makes the weights permutation-equivariant: equal raw values, equal weights
        assert np.max(np.abs(np.asarray(b["logw"] - a["logw"][perm], dtype=np.float64))) <= 1e-15
    lw = np.asarray(a["logw"], dtype=np.float64).reshape(-1, 4)
    assert np.all(lw == lw[:, :1])


def test_a_nan_makes_every_statistic_of_the_row_nan():
    V = R.synthetic_rows(1, 50, 0.5, seed=1)[0]
    V[17] = np.nan
    out = R.psis_row(V)
    assert out["n_tail"] == -1 and all(math.isnan(float(out[k])) for k in ("elpd_loo", "lppd", "pareto_k", "p_waic"))
    assert np.isnan(np.asarray(out["logw"], dtype=np.float64)).all()


def test_the_planted_influence_case_holds_in_the_reference_with_a_margin():
    """tests/test_gpu_loo.py::test_planted_influence asserts orderings only; here the reference itself satisfies them
    by more than ten times its bounds, for the seed that test uses."""
    import test_gpu_loo as G
    rows, shift, dshift = G.planted_reference(G.PLANTED_SEED)
    col = np.abs(shift[:, 0])
    for o in (1, 2):
        assert col[0] - col[o] > 10 * (dshift[0, 0] + dshift[o, 0]), (o, col, dshift[:, 0])
    for r in rows:
        gap = float(r["lppd"] - r["elpd_loo"])
        assert np.isfinite(r["bound"]["lppd"] + r["bound"]["elpd_loo"])
        assert gap > 10 * (r["bound"]["lppd"] + r["bound"]["elpd_loo"]), gap


def test_weighted_moments_reference():
    rng = np.random.default_rng(2)
    X = rng.normal(size=(65, 3))
    mean, var, dm, dv = R.weighted_moments(X, np.zeros((1, 65)))
    assert np.allclose(np.asarray(mean[0], dtype=np.float64), X.mean(axis=0), atol=1e-15)
    assert np.allclose(np.asarray(var[0], dtype=np.float64), X.var(axis=0), atol=1e-15)
    assert np.all(dm > 0) and np.all(dm < 1e-13) and np.all(dv > 0) and np.all(dv < 1e-13)


def test_summary_arithmetic():
    from gpemu import loo
    S = 1000
    stats = {"elpd_loo": np.array([-1.0, -2.5, -4.0]), "lppd": np.array([-0.5, -2.0, -3.0]),
             "p_loo": np.array([0.5, 0.5, 1.0]), "pareto_k": np.array([0.1, 0.68, np.inf]),
             "n_tail": np.array([95, 95, 3]), "ess_w": np.array([900.0, 40.0, 2.0]),
             "p_waic": np.array([0.4, 0.6, 0.9]), "elpd_waic": np.array([-0.9, -2.6, -3.9])}
    s = loo.assemble(stats, S, labels=["a", "b", "c"])
    assert s["n_obs"] == 3 and s["n_samples"] == S and s["labels"] == ["a", "b", "c"]
    assert s["elpd_loo_total"] == -7.5 and s["p_loo_total"] == 2.0 and s["lppd_total"] == -5.5
    assert s["se"] == pytest.approx(math.sqrt(3 * np.var([-1.0, -2.5, -4.0])), rel=1e-15)
    thr = min(1 - 1 / math.log10(S), 0.7)
    assert np.all(s["k_threshold"] == thr) and thr == pytest.approx(2.0 / 3.0)
    assert list(s["warning"]) == [False, True, True]
    assert loo.k_threshold(10 ** 6) == 0.7 and loo.k_threshold(100) == 0.5
    assert [loo.tail_size(n) for n in (20, 21, 65, 2049, 100003)] == [4, 5, 13, 136, 949]
    assert loo.tail_size(2049, r_eff=0.25) == 272
    with pytest.raises(ValueError):
        loo.assemble(stats, S, labels=["a"])
    # leave_out: a list of non-empty lists of rows, flattened in the given order
    start, rows = loo.check_leave_out([[2, 0], [1]], 3)
    assert start.tolist() == [0, 2, 3] and rows.tolist() == [2, 0, 1]
    for bad in ([], [[]], [[3]], [[-1]], "01"):
        with pytest.raises((ValueError, IndexError)):
            loo.check_leave_out(bad, 3)
    other = dict(stats, elpd_loo=np.array([-1.5, -2.0, -4.25]), elpd_waic=np.array([-1.0, -2.0, -4.0]))
    c = loo.compare(s, loo.assemble(other, S, labels=["a", "b", "c"]))
    assert c["elpd_diff"] == pytest.approx(0.25) and c["pointwise_diff"].tolist() == [0.5, -0.5, 0.25]
    assert c["se_diff"] == pytest.approx(math.sqrt(3 * np.var([0.5, -0.5, 0.25])), rel=1e-15)
    with pytest.raises(ValueError):
        loo.compare(s, loo.assemble(other, S, labels=["a", "b", "x"]))


def test_loo_settings():
    from bayesian_inference import mcmc
    assert mcmc.loo_settings({}) == (False, None)
    assert mcmc.loo_settings({"loo": False}) == (False, None)
    assert mcmc.loo_settings({"loo": True}) == (True, None)
    assert mcmc.loo_settings({"loo": True, "loo_leave_out": [["a", "b"], ["c"]]}) == (True, [["a", "b"], ["c"]])
    for bad in ({"loo": "yes"}, {"loo": 1}, {"loo": True, "loo_leave_out": []}, {"loo": True, "loo_leave_out": [[]]},
                {"loo": True, "loo_leave_out": ["a"]}, {"loo": True, "loo_leave_out": [["a", 3]]},
                {"loo": True, "loo_leave_out": "a"}):
        with pytest.raises(ValueError):
            mcmc.loo_settings(bad)
    assert mcmc.LOO_KEYS == ("labels", "elpd_loo", "p_loo", "pareto_k", "k_threshold", "ess_w", "elpd_waic", "p_waic",
                             "lppd", "se")


def test_symbols_are_declared_bound_and_built():
    from gpemu import _lib
    hdr = open(os.path.join(ROOT, "include", "gpemu.h")).read()
    names = ["gpemu_model_observable_blocks", "gpemu_loglik_pointwise", "gpemu_loglik_pointwise_dev", "gpemu_psis",
             "gpemu_psis_dev", "gpemu_weighted_moments_dev", "gpemu_loo_group_rows_dev", "gpemu_loo_path_counts"]
    L = _lib.lib()
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.exported_symbols() and hasattr(L, name), name
    for path in ("SORT_PASS", "ROW_SMOOTHED", "ROW_RAW", "CHUNK", "ROW_BATCH"):
        assert "GPEMU_LOO_PATH_" + path in hdr
    sec = hdr[hdr.index("PSIS-LOO and WAIC"):hdr.index("gpemu_model_observable_blocks(")]
    assert "ref: emulation.py:370-388" in sec and "ref: plot_analyses.py:144" in sec
    mk = open(os.path.join(ROOT, "bayesian-inference_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bk_loo\.hip\b", mk, re.M)
    from gpemu import loo
    assert len(loo.FIELDS) == int(re.search(r"#define GPEMU_PSIS_NOUT (\d+)", hdr).group(1))


def test_the_reference_does_not_import_the_library():
    src = open(os.path.join(ROOT, "tests", "loo_ref.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(gpemu|bayesian_inference)", src, re.M)
