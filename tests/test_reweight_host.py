"""Host tests of the reweighting rules (gpemu.reweight, bayesian_inference.mcmc.reweight_settings) and
of their reference tests/reweight_ref.py: no device needed."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import reweight_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 52


def _chain_like(seed, S=1001, d=2):
    """repeated rows, as a chain has, and the fixed-point weights of a log-uniform x normal scenario"""
    rng = np.random.default_rng(seed)
    base = rng.uniform([0.2, -1.0], [3.0, 2.0], (S // 4 + 1, d))
    x = base[rng.integers(0, base.shape[0], S)]
    l = -np.log(x[:, 0]) - (x[:, 1] - 0.4) ** 2 / (2 * 0.9 ** 2)
    lw = l - np.logaddexp.reduce(l)
    return x, RR.quantise(lw)


def test_the_reference_quantile_is_numpys_inverted_cdf():
    x, q = _chain_like(0)
    Q = int(q.astype(object).sum())
    assert 0 < abs(Q - ONE) < 2048          # the weights are normalised up to their roundings
    for j in range(x.shape[1]):
        for p in (0.05, 0.5, 0.95):
            want = np.quantile(x[:, j], p, weights=q.astype(np.float64), method="inverted_cdf")
            assert RR.weighted_select(x[:, j], q, RR.target(p, Q)) == want      # the definition, in Python ints
            assert RR.weighted_quantile(x[:, j], q, [p])[0] == want             # its searchsorted form
    # equal weights: the unweighted inverted CDF
    c = np.full(x.shape[0], 12345, dtype=np.uint64)
    for p in (0.05, 0.5, 0.95, 0.3333):
        assert RR.weighted_quantile(x[:, 0], c, [p])[0] == np.quantile(x[:, 0], p, method="inverted_cdf")


def test_the_reference_histogram_equals_the_integer_sums():
    from gpemu import marginals as M
    x, q = _chain_like(1)
    e1, e2 = M.bin_edges([0.2, -1.0], [3.0, 2.0], 7), M.bin_edges([0.2, -1.0], [3.0, 2.0], 5)
    h1, h2, wi = RR.hist_ref(x, q, e1, e2)
    for j in range(2):
        b = np.clip(np.searchsorted(e1[j], x[:, j], side="right") - 1, 0, 6)
        want = [int(q[b == k].astype(object).sum()) for k in range(7)]
        assert [int(v) for v in h1[j]] == want
    assert int(h2.astype(object).sum()) == int(q.astype(object).sum()) == int(wi[0])


def test_targets_hand_cases():
    from gpemu import reweight as R
    Q = np.array([10, ONE + 21], dtype=np.uint64)
    t = R.targets([0.0, 1.0, 0.5, 0.25, 0.3], Q)
    assert t.dtype == np.uint64 and t.shape == (2, 5)
    assert t[0].tolist() == [1, 10, 5, 3, 3]          # p = 0 -> 1; p = 1 -> Q; p Q an integer -> itself; 2.5 -> 3; 3.0000..01 -> ...
    assert t[0, 4] == math.ceil(Fraction(0.3) * 10)
    assert int(t[1, 1]) == ONE + 21 and int(t[1, 2]) == math.ceil(Fraction(ONE + 21, 2))
    assert int(t[1, 4]) == math.ceil(Fraction(0.3) * (ONE + 21))
    for bad in ([], [-0.1], [1.5], [np.nan]):
        with pytest.raises(ValueError):
            R.targets(bad, Q)
    with pytest.raises(ValueError):
        R.targets([0.5], [0])


def test_check_priors_tables_and_rejections():
    from gpemu import reweight as R
    lo, hi = [0.1, -1.0, 0.5], [3.0, 2.0, 4.0]
    k, a, b = R.check_priors([[1, ("normal", 0.5, 2.0), None],
                              {2: {"kind": "log_normal", "a": 0.25, "b": 1.5}},
                              ["flat", 0, "log_uniform"]], 3, lo, hi)
    assert k.dtype == np.int32 and k.tolist() == [[1, 2, 0], [0, 0, 3], [0, 0, 1]]
    assert a[0, 1] == 0.5 and b[0, 1] == 2.0 and a[1, 2] == 0.25 and b[1, 2] == 1.5
    bad = [
        [[1, 1, 0]],                                              # log-uniform on a parameter whose lower bound is -1
        [[0, ("log_normal", 0.0, 1.0), 0]],                       # log-normal likewise
        [[("normal", 0.0, 0.0), 0, 0]],                           # b = 0
        [[("normal", 0.0, -1.0), 0, 0]],                          # b < 0
        [[("normal", np.nan, 1.0), 0, 0]],                        # non-finite a
        [[("normal", 0.0, np.inf), 0, 0]],                        # non-finite b
        [[("normal", None, None), 0, 0]],                         # missing a, b
        [[{"kind": "normal", "a": 0.0, "b": 1.0, "lower": 0.5}, 0, 0]],   # a narrower box
        [[{"kind": "flat", "upper": 1.0}, 0, 0]],                 # a truncation
        [[0, 0]],                                                 # d priors per scenario
        [[4, 0, 0]], [["cauchy", 0, 0]],                          # unknown kinds
        [], "flat", [[0, 0, 0]] * 65,                             # no scenario, not a list, more than 64
    ]
    for spec in bad:
        with pytest.raises(ValueError):
            R.check_priors(spec, 3, lo, hi)
    with pytest.raises(IndexError):
        R.check_priors([{3: 1}], 3, lo, hi)
    with pytest.raises(ValueError):
        R.check_priors([[0, 0, 0]], 3, lo, [3.0, -2.0, 4.0])      # upper < lower
    with pytest.raises(ValueError):
        R.check_priors([[0] * 17], 17, np.zeros(17), np.ones(17))


def test_reference_prior_on_the_references_names():
    from gpemu import reweight as R
    # the parameter names of the reference's two parameterisations (ref: config/jet_substructure.yaml:129, 133)
    import json
    names = json.load(open(os.path.join(ROOT, "tests", "golden", "reweight_parameter_names.json")))
    assert R.reference_prior(names["exponential"]) == [0, 0, 1, 1, 0, 1]
    assert R.reference_prior(names["binomial"]) == [0, 0, 1, 1, 0, 0, 0]
    assert R.reference_prior(["a", "b"]) == [0, 0]


def test_log_prior_norm_against_quadrature():
    from scipy.integrate import quad
    from gpemu import reweight as R
    lo, hi = np.array([0.05, -1.0, 0.5, 2.0]), np.array([3.0, 2.0, 40.0, 9.0])
    spec = [[1, ("normal", 0.5, 2.0), ("log_normal", 1.0, 0.7), 0],
            [("log_normal", -1.0, 1.5), ("normal", 5.0, 1.0), 1, ("normal", 0.0, 3.0)],      # a normal far in its tail
            [0, 0, 0, 0]]
    kind, a, b = R.check_priors(spec, 4, lo, hi)
    got = R.log_prior_norm(kind, a, b, lo, hi)
    dens = {0: lambda x, a, b: 1.0, 1: lambda x, a, b: 1.0 / x,
            2: lambda x, a, b: math.exp(-(x - a) ** 2 / (2 * b * b)),
            3: lambda x, a, b: math.exp(-math.log(x) - (math.log(x) - a) ** 2 / (2 * b * b))}
    for r in range(kind.shape[0]):
        want, err = 0.0, 0.0
        for i in range(4):
            v, e = quad(dens[int(kind[r, i])], lo[i], hi[i], args=(a[r, i], b[r, i]), epsabs=0.0, epsrel=1e-13, limit=200)
            want += math.log(v)
            err += e / v          # d log v = dv / v: quad's own error estimate, nothing added
        assert abs(got[r] - want) <= err + 4 * np.spacing(abs(want)), (r, got[r], want, err)
    assert got[2] == pytest.approx(np.sum(np.log(hi - lo)), rel=1e-15)


def test_reweight_settings():
    from bayesian_inference import mcmc
    assert mcmc.reweight_settings({}) is None
    assert mcmc.reweight_settings({"reweight": None}) is None and mcmc.reweight_settings({"reweight": False}) is None
    assert mcmc.reweight_settings({"reweight": {"reference_prior": False}}) is None
    assert mcmc.reweight_settings({"reweight": {"reference_prior": True}}) == [("reference_prior", None)]
    got = mcmc.reweight_settings({"reweight": [
        {"name": "logc", "priors": {"c_1": {"kind": "log_uniform"}, "tau": {"kind": "normal", "a": 1.0, "b": 0.5}}},
        {"name": "ln", "priors": {"c_2": {"kind": "log_normal", "a": 0, "b": 2}}}]})
    assert [n for n, _ in got] == ["logc", "ln"]
    assert got[0][1] == {"c_1": {"kind": "log_uniform"}, "tau": {"kind": "normal", "a": 1.0, "b": 0.5}}
    for bad in (True, "yes", 1, [], {"reference_prior": "yes"}, {"reference_prior": True, "x": 1}, [{"name": "a"}],
                [{"name": "a b", "priors": {"c": {"kind": "flat"}}}], [{"name": "a", "priors": {}}],
                [{"name": "a", "priors": {"c": {"kind": "cauchy"}}}], [{"name": "a", "priors": {"c": {"kind": "normal"}}}],
                [{"name": "a", "priors": {"c": {"kind": "normal", "a": 0.0, "b": 0.0}}}],
                [{"name": "a", "priors": {"c": {"kind": "normal", "a": 0.0, "b": 1.0, "lower": 0.0}}}],
                [{"name": "a", "priors": {"c": {"kind": "flat"}}}, {"name": "a", "priors": {"c": {"kind": "flat"}}}]):
        with pytest.raises(ValueError):
            mcmc.reweight_settings({"reweight": bad})
    assert "Q" in mcmc.REWEIGHT_KEYS and "hist_2d_q" in mcmc.REWEIGHT_KEYS


def test_symbols_are_declared_bound_and_built():
    from gpemu import _lib, reweight
    hdr = open(os.path.join(ROOT, "include", "gpemu.h")).read()
    names = ["gpemu_logprior", "gpemu_logprior_dev", "gpemu_logmeanexp_dev", "gpemu_weights_fixed_dev",
             "gpemu_weighted_select", "gpemu_weighted_select_dev", "gpemu_weighted_hist", "gpemu_weighted_hist_dev",
             "gpemu_reweight_path_counts"]
    L = _lib.lib()
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.exported_symbols() and hasattr(L, name), name
    for path in reweight.PATHS:
        assert "GPEMU_REWEIGHT_PATH_" + path in hdr
    order = [hdr.index("GPEMU_REWEIGHT_PATH_" + p + ("," if p != "LOGPRIOR" else " = 0")) for p in reweight.PATHS]
    assert order == sorted(order)
    sec = hdr[hdr.index("importance reweighting of a chain"):hdr.index("gpemu_logprior(")]
    assert "ref: log_posterior.py:97" in sec and "ref: plot_qhat.py:298-326" in sec
    mk = open(os.path.join(ROOT, "bayesian-inference_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bk_reweight\.hip\b", mk, re.M)


def test_the_reference_does_not_import_the_library():
    src = open(os.path.join(ROOT, "tests", "reweight_ref.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(gpemu|bayesian_inference)", src, re.M)
