"""Host-side tests of the weighted bands, intervals and densities: the references of
tests/wsummary_ref.py against independent statements of the same definitions, the bandwidth rule against scipy, the new
symbols and the ``parameters.mcmc.reweight_summaries`` settings.  No GPU."""
import os
import re

import numpy as np
import pytest

import marginals_ref as MR
import wsummary_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gpemu_posterior_predictive_weighted", "gpemu_posterior_predictive_weighted_dev", "gpemu_weighted_hpd",
       "gpemu_weighted_hpd_dev", "gpemu_weighted_kde1d", "gpemu_weighted_kde1d_dev", "gpemu_wsummary_path_counts"]


def _sample(rng, S):
    kind = rng.integers(0, 3)
    if kind == 0:
        return rng.normal(size=S)
    if kind == 1:
        return np.round(rng.normal(size=S), 1)                  # heavy ties
    return rng.integers(0, 4, S).astype(np.float64)             # a handful of values


def test_hpd_reference_is_the_narrowest_window_under_equal_weights():
    rng = np.random.default_rng(0)
    for _ in range(400):
        S = int(rng.integers(1, 60))
        x = _sample(rng, S)
        c = int(rng.integers(1, 1 << 40))
        q = np.full(S, c, dtype=np.uint64)
        n_out = int(rng.integers(1, S + 1))
        got = WR.hpd(x, q, c * (S - n_out + 1))
        want = MR.hpd_ref(x + 0.0, n_out)
        assert got == tuple(float(v) for v in want), (x, n_out)


def test_hpd_reference_is_the_brute_force_over_value_pairs():
    rng = np.random.default_rng(1)
    for _ in range(300):
        S = int(rng.integers(1, 25))
        x = _sample(rng, S)
        q = rng.integers(0, 1 << 30, S).astype(np.uint64)
        q[rng.random(S) < 0.4] = 0
        Q = int(q.sum())
        for t in {1, max(1, Q // 3), max(1, (2 * Q) // 3), max(Q, 1), Q + 1}:
            a, b = WR.hpd(x, q, t), WR.hpd_brute(x, q, t)
            assert a == b or (np.isnan(a[0]) and np.isnan(b[0])), (x, q, t, a, b)
            if t > Q:
                assert np.isnan(a[0]) and np.isnan(a[1])
    bad = np.array([0.0, np.nan, 1.0])
    assert np.isnan(WR.hpd(bad, np.ones(3, dtype=np.uint64), 1)[0])
    assert np.isnan(WR.hpd(np.array([0.0, np.inf]), np.ones(2, dtype=np.uint64), 1)[0])


def test_bandwidth_and_density_formula_are_scipys():
    from scipy.stats import gaussian_kde
    from gpemu import reweight as RW
    rng = np.random.default_rng(2)
    for S in (7, 200, 3000):
        x = rng.normal(1.0, 2.0, S)
        w = rng.random(S) ** 3
        w[rng.random(S) < 0.3] = 0.0
        w /= w.sum()
        k = gaussian_kde(x, weights=w)
        mean = np.sum(w * x)
        var_w, n_eff = np.sum(w * (x - mean) ** 2), 1.0 / np.sum(w * w)
        h = float(RW.weighted_bandwidth(var_w, n_eff))
        assert abs(h - WR.scipy_bandwidth(x, w)) <= 1e-13 * h
        assert abs(n_eff - k.neff) <= 1e-12 * n_eff
        # the density formula with fixed-point weights, on scipy's evaluation
        q = np.rint(w * 2.0 ** 52).astype(np.uint64)
        grid = np.linspace(x.min() - 3 * h, x.max() + 3 * h, 50)
        ours = WR.kde(x, q, grid, h).astype(np.float64)
        theirs = k(grid)
        assert np.all(np.abs(ours - theirs) <= 1e-10 * theirs.max())
    assert np.isnan(RW.weighted_bandwidth(1.0, 1.0))            # all the weight on one sample
    assert RW.weighted_bandwidth(np.ones((2, 3)), np.array([[4.0], [9.0]])).shape == (2, 3)


def _prototypes(hdr):
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(?:int|void|int64_t)\s+(gpemu_\w+)\s*\(([^;{]*?)\)\s*;", code)}


def test_new_symbols_are_declared_bound_and_exported():
    import ctypes as C
    from gpemu import _lib
    from gpemu import reweight as RW
    hdr = open(os.path.join(ROOT, "include", "gpemu.h")).read()
    protos = _prototypes(hdr)
    L = _lib.lib()
    for name in NEW:
        assert name in protos and name in _lib.exported_symbols() and hasattr(L, name), name
        assert not re.search(r"\bvoid\s*\*\s*stream\b", protos[name]), f"{name} takes a void *stream parameter"
        if name.endswith("_dev"):
            assert re.search(r"const\s+gpemu_call_ctx\s*\*\s*ctx\s*$", protos[name].strip()), name
    assert re.search(r"typedef struct \{ void \*stream; int64_t workspace_bytes; \} gpemu_call_ctx;", hdr)
    assert [f for f, _ in _lib.CallCtx._fields_] == ["stream", "workspace_bytes"] and C.sizeof(_lib.CallCtx) == 16
    # what the table of tests/stream_cases.py says for entries with a stream parameter, in the new section's own words
    section = re.sub(r"\s+", " ", re.sub(r"(?m)^\s*\*\s?", " ", hdr[hdr.index("/* ---- weighted bands"):]))
    assert "gpemu_weighted_hpd_dev and gpemu_weighted_kde1d_dev work on ctx->stream (NULL = the null stream)" in section
    assert "each waits for it before returning" in section
    assert "gpemu_posterior_predictive_weighted_dev works on ctx->stream (NULL = the model's) and waits for it" in section
    assert "ctx == NULL means stream NULL and workspace_bytes 0" in section
    assert "gpemu_call_ctx" in hdr[:hdr.index("#ifndef GPEMU_H")]
    enum = re.search(r"enum gpemu_wsummary_path \{(.*?)\};", hdr, re.S).group(1)
    names = re.findall(r"GPEMU_WSUMMARY_PATH_([A-Z0-9_]+?)\b", enum)
    assert names[:-1] == list(RW.WSUMMARY_PATHS) and names[-1] == "COUNT"
    out = (C.c_int64 * 32)()
    assert L.gpemu_wsummary_path_counts(out, 32) == len(RW.WSUMMARY_PATHS)
    src = open(os.path.join(ROOT, "bayesian-inference_amd", "csrc", "Makefile")).read()
    assert "k_wsummary.hip" in src


def test_python_level_argument_checks():
    from gpemu import reweight as RW
    with pytest.raises(ValueError):
        RW.targets([1.5], [10])
    with pytest.raises(ValueError):
        RW._kde_plan(np.ones((1, 2)), [4.0], np.zeros(2), np.ones(2), 1, 2, None, [[0.0, 1.0]], 10, 3.0)
    h, g = RW._kde_plan(np.ones((2, 3)), [4.0, 9.0], np.zeros(3), np.ones(3), 2, 3, None, None, 11, 3.0)
    assert h.shape == (2, 3) and g.shape == (2, 3, 11)
    assert np.allclose(g[:, :, 0], -3.0 * h) and np.allclose(g[:, :, -1], 1.0 + 3.0 * h)
    out = RW.add_hpd_kde([{}], [0.9], np.zeros((1, 1, 2, 2)), None)
    assert set(out[0]) == {"hpd_confidence", "hpd"}


def test_reweight_summaries_settings_parse_and_refuse():
    from bayesian_inference import mcmc
    on = {"reweight": {"reference_prior": True}}
    assert mcmc.reweight_summaries_settings(on) is None
    assert mcmc.reweight_summaries_settings(dict(on, reweight_summaries={})) == \
        {"hpd": None, "kde": False, "posterior_predictive": False}
    got = mcmc.reweight_summaries_settings(dict(on, reweight_summaries={"hpd": [0.68, 0.9], "kde": True,
                                                                        "posterior_predictive": True}))
    assert got == {"hpd": [0.68, 0.9], "kde": True, "posterior_predictive": True}
    for bad in ({"kde2d": True}, {"hpd": []}, {"hpd": [1.0]}, {"hpd": 0.9}, {"hpd": [True]}, {"kde": "yes"},
                {"posterior_predictive": 1}, [0.9]):
        with pytest.raises(ValueError):
            mcmc.reweight_summaries_settings(dict(on, reweight_summaries=bad))
    # only together with parameters.mcmc.reweight
    for without in ({}, {"reweight": {"reference_prior": False}}):
        with pytest.raises(ValueError, match="needs parameters.mcmc.reweight"):
            mcmc.reweight_summaries_settings(dict(without, reweight_summaries={"kde": True}))

    class Cfg:
        reweight_summaries = got
    assert mcmc._reweight_summary_kwargs(Cfg) == {"hpd": [0.68, 0.9], "kde": True, "posterior_predictive": True}
    Cfg.reweight_summaries = None
    assert mcmc._reweight_summary_kwargs(Cfg) == {}
    res = [{"hpd_confidence": np.array([0.9]), "hpd": np.zeros((1, 2, 2)), "kde_grid": np.zeros((2, 3)),
            "kde_density": np.zeros((2, 3)), "kde_bandwidth": np.ones(2),
            "posterior_predictive": {k: np.zeros(4) for k in mcmc.REWEIGHT_PP_KEYS}}]
    assert set(mcmc._reweight_summary_entries(res, ["a"])) == \
        {"reweight_hpd_confidence", "reweight_a_hpd", "reweight_a_kde_grid", "reweight_a_kde_density",
         "reweight_a_kde_bandwidth", "reweight_a_pp_mean", "reweight_a_pp_variance_parameters",
         "reweight_a_pp_variance_emulator", "reweight_a_pp_quantiles"}
    assert mcmc._reweight_summary_entries([{}], ["a"]) == {}
