"""CPU tests of the host side of the posterior-predictive summaries and the selection (no GPU): the virtual-index /
lerp helper against np.quantile, the merge over emulation groups, the YAML keys, argument validation, and the
reference tests/pp_ref.py against a brute-force computation with oracle.gp_oracle on a tiny model."""
import os
import re

import numpy as np
import pytest

import pp_ref as P
from oracle import gp_oracle as O


# ---- virtual index and lerp ---------------------------------------------------------------------------------------
def _host_quantile(v, probs):
    from gpemu import select
    lo, hi, t = select.virtual_index(v.shape[-1], probs)
    srt = np.sort(v, axis=-1)
    return select.lerp(srt[..., lo], srt[..., hi], t), (srt[..., lo], srt[..., hi], t)


@pytest.mark.parametrize("S", [1, 2, 3, 10, 101, 1000, 4097])
def test_virtual_index_and_lerp_equal_numpy_on_random_cases(S):
    rng = np.random.default_rng(S)
    v = rng.normal(size=(13, S)) * 10.0 ** rng.integers(-5, 6, (13, 1))
    probs = np.r_[0.0, 1.0, 0.5, rng.random(40)]
    got, (a, b, t) = _host_quantile(v, probs)
    want = np.quantile(v, probs, axis=-1, method="linear").T
    # the same expression on the same operands: the same bits (the helper IS numpy's rule)
    assert np.array_equal(got, want)


def test_integer_virtual_indices_return_the_element():
    rng = np.random.default_rng(1)
    v = rng.normal(size=(4, 101))
    probs = np.arange(0, 101, 5) / 100.0
    got, (a, b, t) = _host_quantile(v, probs)
    exact = t == 0
    assert exact.sum() >= 15          # 5 j / 100 * 100 is an integer unless the product rounds
    assert np.array_equal(got[:, exact], a[:, exact])
    assert np.array_equal(got, np.quantile(v, probs, axis=-1, method="linear").T)
    # next to an infinity the element itself, where numpy's expression gives inf * 0 = NaN
    from gpemu import select
    assert select.lerp(2.0, np.inf, 0.0) == 2.0


def test_virtual_index_bounds():
    from gpemu import select
    lo, hi, t = select.virtual_index(10, [0.0, 1.0, 0.5])
    assert lo.tolist() == [0, 9, 4] and hi.tolist() == [1, 9, 5] and t[0] == 0 and t[1] == 0 and t[2] == 0.5
    lo, hi, t = select.virtual_index(1, [0.0, 0.3, 1.0])
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [0, 0, 0]
    for bad in ([-0.1], [1.1], [np.nan], []):
        with pytest.raises(ValueError):
            select.virtual_index(10, bad)
    with pytest.raises(ValueError):
        select.virtual_index(0, [0.5])


def test_rank_validation():
    from gpemu import select
    assert select.check_ranks([0, 3, 3], 4).dtype == np.int64
    for bad, S in (([-1], 4), ([4], 4), ([0.5], 4), ([], 4), ([[0]], 4), ([0], 0), ([np.nan], 4)):
        with pytest.raises(ValueError):
            select.check_ranks(bad, S)


def test_quantile_plan_brackets_and_assembles():
    from gpemu.model import QuantilePlan
    plan = QuantilePlan(11, (0.05, 0.5, 0.95))
    assert plan.ranks.tolist() == [0, 1, 5, 6, 9, 10]        # sorted, distinct (0.5 * 10 is an integer: 5 and 6)
    rng = np.random.default_rng(0)
    v = rng.normal(size=(7, 11))
    order = np.sort(v, axis=1)[:, plan.ranks]
    out = plan.result(np.zeros(7), np.ones(7), 2 * np.ones(7), order)
    assert np.array_equal(out["quantiles"], np.quantile(v, (0.05, 0.5, 0.95), axis=1, method="linear"))
    assert np.array_equal(out["variance"], 3 * np.ones(7))
    empty = QuantilePlan(11, None)
    assert empty.ranks.size == 0 and empty.quantiles(np.zeros((7, 1))).shape == (0, 7)


# ---- the merge over groups -------------------------------------------------------------------------------------------
class _FakeSorter:
    """two groups interleaved in the merged order: A's first observable, B's only one, A's second"""
    shape = (5, 9)
    emulation_group_to_observable_matrix = {
        "obs1": ("A", slice(0, 3), slice(0, 3)),
        "obs2": ("B", slice(3, 7), slice(0, 4)),
        "obs3": ("A", slice(7, 9), slice(3, 5)),
    }


def _fake_group(F, base):
    v = base + np.arange(F, dtype=np.float64)
    return {"mean": v, "variance_parameters": v + 0.25, "variance_emulator": v + 0.5, "variance": 2 * v + 0.75,
            "quantiles": np.stack([v - 1, v, v + 1]), "probabilities": np.array([0.05, 0.5, 0.95])}


def test_group_merge_is_a_scatter_in_the_sorters_order():
    from bayesian_inference import emulation
    groups = {"A": _fake_group(5, 100.0), "B": _fake_group(4, 200.0)}
    out = emulation.merge_posterior_predictive(_FakeSorter(), groups)
    assert out["mean"].tolist() == [100, 101, 102, 200, 201, 202, 203, 103, 104]
    assert np.array_equal(out["variance"], 2 * out["mean"] + 0.75)
    assert out["quantiles"].shape == (3, 9) and np.array_equal(out["quantiles"][1], out["mean"])
    assert np.array_equal(out["quantiles"][2] - out["quantiles"][0], 2 * np.ones(9))
    assert np.array_equal(out["probabilities"], [0.05, 0.5, 0.95])


def test_group_merge_with_a_sorter_that_only_converts():
    import dropin_util as DU
    from bayesian_inference import emulation
    g = _fake_group(6, 10.0)
    out = emulation.merge_posterior_predictive(DU.TrivialSort("main"), {"main": g})
    for key in ("mean", "variance_parameters", "variance_emulator", "variance", "quantiles", "probabilities"):
        assert np.array_equal(out[key], g[key]), key


# ---- YAML ------------------------------------------------------------------------------------------------------------
def test_yaml_keys_default_off():
    from bayesian_inference import mcmc
    assert mcmc.posterior_predictive_settings({}) == (False, (0.05, 0.5, 0.95))
    assert mcmc.posterior_predictive_settings({"posterior_predictive": False}) == (False, (0.05, 0.5, 0.95))
    assert mcmc.posterior_predictive_settings({"posterior_predictive": True}) == (True, (0.05, 0.5, 0.95))
    on, probs = mcmc.posterior_predictive_settings({"posterior_predictive": True,
                                                    "posterior_predictive_probabilities": [0.16, 0.84]})
    assert on and probs == (0.16, 0.84)
    assert mcmc.posterior_predictive_settings({"posterior_predictive_probabilities": 0.5}) == (False, (0.5,))
    for bad in ([1.5], [-0.1], []):
        with pytest.raises(ValueError):
            mcmc.posterior_predictive_settings({"posterior_predictive_probabilities": bad})


def test_mcmc_config_reads_the_keys(tmp_path):
    import dropin_util as DU
    from bayesian_inference import mcmc
    path, analysis = DU.write_config(tmp_path, n_pc=5, n_restarts=0)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.posterior_predictive is False and cfg.posterior_predictive_probabilities == (0.05, 0.5, 0.95)
    analysis["parameters"]["mcmc"]["posterior_predictive"] = True
    analysis["parameters"]["mcmc"]["posterior_predictive_probabilities"] = [0.025, 0.975]
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.posterior_predictive is True and cfg.posterior_predictive_probabilities == (0.025, 0.975)


def test_without_the_key_nothing_is_added_to_the_results():
    from bayesian_inference import mcmc

    class Cfg:
        posterior_predictive = False
    results = {"chain": np.zeros((2, 3, 4))}
    mcmc._add_posterior_predictive(Cfg(), results, None, None, None)
    assert set(results) == {"chain"}


# ---- the C ABI's declarations ---------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_cite_the_reference():
    from gpemu import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gpemu.h")).read()
    declared = set(re.findall(r"\b(gpemu_[a-z0-9_]+)\s*\(", hdr))
    for name in ("gpemu_select", "gpemu_select_dev", "gpemu_posterior_predictive", "gpemu_posterior_predictive_dev",
                 "gpemu_sampler_chain_ptr", "gpemu_postpred_path_counts"):
        assert name in declared and name in _lib.exported_symbols(), name
    assert "plot_mcmc.py:343-371" in hdr and "plot_qhat.py:102-109" in hdr
    src = open(os.path.join(root, "bayesian-inference_amd", "csrc", "Makefile")).read()
    assert "k_postpred.hip" in src


def test_workspace_helper_matches_the_headers_rule():
    from gpemu.model import POSTPRED_FIXED_BYTES, postpred_workspace_bytes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gpemu.h")).read()
    assert re.search(r"#define GPEMU_POSTPRED_FIXED_BYTES \(32ll << 20\)", hdr) and POSTPRED_FIXED_BYTES == 32 << 20
    assert postpred_workspace_bytes(1000, 10, 16) == 16 * 1000 * 10 + (32 << 20) + 8 * 1000 * 16


# ---- pp_ref against a brute-force computation ---------------------------------------------------------------------
@pytest.mark.parametrize("spec", [O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=False, has_noise=True),
                                  O.KernelSpec(kind=O.MATERN, nu=2.5, has_const=True, has_noise=True)])
def test_pp_ref_against_brute_force_on_a_tiny_model(spec):
    model, lo, hi = P.problem(24, 3, 7, 2, spec, seed=1)
    X = np.random.default_rng(2).uniform(lo, hi, (33, 3))
    probs = (0.05, 0.5, 0.95)
    mu, sigma2, delta = P.per_sample(model, X)
    ref = P.summaries(mu, sigma2, probs)
    brute = P.brute_force(model, X, probs)
    assert np.all(delta > 0) and np.all(delta < 1e-9 * np.abs(np.asarray(mu, float)).max())
    scale = float(np.abs(np.asarray(mu, float)).max())
    for key in ("mean", "variance_parameters", "variance_emulator", "variance", "quantiles"):
        a, b = np.asarray(ref[key], float), np.asarray(brute[key], float)
        assert a.shape == b.shape
        # the float64 oracle against the extended reference: the oracle's own rounding, far below 1e-9 of the scale
        assert np.max(np.abs(a - b)) <= 1e-9 * max(scale, scale * scale), key
    # law of total variance on the brute-force samples: var(mu) + mean(sigma2), population form
    assert np.allclose(np.asarray(ref["variance_parameters"], float), np.var(np.asarray(mu, float), axis=0), rtol=1e-12)
    tol = P.tolerances(mu, delta, ref["variance_parameters"])
    assert set(tol) == {"mean", "quantiles", "variance_parameters"} and all(np.all(v > 0) for v in tol.values())
