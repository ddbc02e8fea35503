"""Host tests of the marginal summaries (gpemu.marginals, the drop-in's settings): the rules that run
in numpy -- contour levels, settings validation, n_out and the window rule, the default bandwidth and grid -- and the
references the GPU tests are held to."""
import numpy as np
import pytest

import marginals_ref as MR


def test_credible_levels_on_hand_made_histograms():
    from gpemu import marginals as M
    h = np.array([[5, 3], [2, 0]])
    assert M.credible_levels(h, [0.5, 0.51, 0.8, 0.81, 1.0]).tolist() == [5, 3, 3, 2, 2]
    assert M.credible_levels(h, 0.5) == 5 and np.ndim(M.credible_levels(h, 0.5)) == 0
    # ties: the bins tied with the level come along, so the level is the tied count itself
    t = np.array([[4, 4], [4, 4]])
    assert M.credible_levels(t, [0.1, 0.25, 0.26, 1.0]).tolist() == [4, 4, 4, 4]
    u = np.array([[6, 2, 2], [2, 2, 2], [2, 1, 1]])          # total 20
    assert M.credible_levels(u, [0.3, 0.31, 0.9, 0.91, 0.95, 0.96, 1.0]).tolist() == [6, 2, 2, 1, 1, 1, 1]
    # p = 1 is the smallest non-zero count; p = 0 the largest count; an empty histogram gives 0
    assert M.credible_levels(np.array([[0, 7], [1, 0]]), [0.0, 1.0]).tolist() == [7, 1]
    assert M.credible_levels(np.zeros((3, 3), dtype=np.int64), [0.5, 1.0]).tolist() == [0, 0]
    # a stack of histograms: one row of levels per pair
    out = M.credible_levels(np.stack([h, t]), [0.5, 1.0])
    assert out.shape == (2, 2) and out.tolist() == [[5, 2], [4, 4]]
    # the defining property on a random histogram
    rng = np.random.default_rng(0)
    r = rng.integers(0, 50, (9, 9))
    for p in (0.1, 0.5, 0.683, 0.9, 0.99, 1.0):
        c = int(M.credible_levels(r, p))
        assert r[r >= c].sum() >= p * r.sum() and r[r >= c + 1].sum() < p * r.sum()
    with pytest.raises(ValueError):
        M.credible_levels(h, 1.5)


def test_marginals_settings_validation():
    from bayesian_inference import mcmc
    assert mcmc.marginals_settings({}) == (False, (100, 50), (0.9,), True)
    assert mcmc.marginals_settings({}, default_confidence=0.68)[2] == (0.68,)
    got = mcmc.marginals_settings({"marginals": True, "marginals_bins": [64, 32], "marginals_confidence": [0.5, 0.9],
                                   "marginals_kde": False}, default_confidence=0.68)
    assert got == (True, (64, 32), (0.5, 0.9), False)
    for bad in ({"marginals": "yes"}, {"marginals": 1}, {"marginals_kde": "no"}, {"marginals_bins": 100},
                {"marginals_bins": [100]}, {"marginals_bins": [0, 50]}, {"marginals_bins": [100, 257]},
                {"marginals_bins": [4097, 50]}, {"marginals_bins": [10.5, 5]}, {"marginals_bins": [True, 5]},
                {"marginals_confidence": 0.9}, {"marginals_confidence": []}, {"marginals_confidence": [0.0]},
                {"marginals_confidence": [0.5, 1.0]}, {"marginals_confidence": ["a"]}, {"marginals_confidence": [True]}):
        with pytest.raises(ValueError):
            mcmc.marginals_settings(bad)


def test_n_out_and_the_window_rule_equal_the_dropin():
    from bayesian_inference import mcmc
    from gpemu import marginals as M
    # n_out as the reference writes it: int((1 - confidence) * S), with the rounding of 1 - confidence
    for S in (2, 3, 10, 64, 1000, 100003):
        for c in (0.5, 0.68, 0.9, 0.99):
            want = int((1 - c) * S)
            if want == 0:
                with pytest.raises(ValueError):
                    M.n_outside(c, S)
            else:
                assert M.n_outside(c, S).tolist() == [want]
    assert int((1 - 0.9) * 10) == 0          # 0.0999.. * 10 truncates: the case the library refuses
    assert M.n_outside([0.5, 0.99], 1000).tolist() == [500, 10]
    rng = np.random.default_rng(1)
    samples = [rng.normal(size=1000), rng.integers(0, 8, 1000).astype(np.float64), np.full(50, 1.25),
               rng.normal(size=7), -np.abs(rng.normal(size=333)) * 1e3]
    for x in samples:
        for c in (0.5, 0.68, 0.9):
            n_out = int((1 - c) * x.size)
            if n_out == 0:
                continue
            lo, hi = mcmc.credible_interval(x, c, "hpd")
            assert MR.hpd_ref(x, n_out) == (lo, hi)
    # ties go to the lowest window
    assert MR.hpd_ref(np.array([0.0, 1.0, 2.0, 3.0]), 2) == (0.0, 2.0)
    assert np.isnan(MR.hpd_ref(np.array([0.0, np.nan, 1.0]), 1)[0]) and np.isnan(MR.hpd_ref(np.array([0.0, np.inf]), 1)[1])


def test_default_bandwidth_and_grid_follow_scipy_and_seaborn():
    from scipy.stats import gaussian_kde
    from gpemu import marginals as M
    rng = np.random.default_rng(2)
    x = rng.normal(1.0, 2.0, (40, 3)) * np.array([1.0, 1e-3, 50.0])
    h, g = M._kde_plan(40, 3, None, None, 200, 3.0, lambda: (x.std(axis=0, ddof=1), x.min(axis=0), x.max(axis=0)))
    for j in range(3):
        k = gaussian_kde(x[:, j])
        bw = float(np.sqrt(k.covariance[0, 0]))             # factor * std(ddof=1), factor = n ** (-1 / 5)
        assert abs(k.factor - 40 ** (-0.2)) < 1e-15
        assert abs(h[j] - bw) <= 4 * np.finfo(float).eps * bw
        # seaborn's support: linspace(min - bw * cut, max + bw * cut, gridsize), cut = 3, gridsize = 200
        want = np.linspace(x[:, j].min() - bw * 3.0, x[:, j].max() + bw * 3.0, 200)
        # (the bandwidths differ by 4 eps at most, the ends by 3 h of that plus their own rounding)
        assert g.shape == (3, 200) and np.max(np.abs(g[j] - want)) <= 16 * np.finfo(float).eps * np.max(np.abs(want))
    h2, g2 = M._kde_plan(40, 3, np.linspace(-1, 1, 7), 0.5, 200, 3.0, None)     # given: nothing is estimated
    assert h2.tolist() == [0.5] * 3 and g2.shape == (3, 7)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            M._kde_plan(40, 3, np.linspace(-1, 1, 7), bad, 200, 3.0, None)
    with pytest.raises(ValueError):          # the default bandwidth of one sample
        M._kde_plan(1, 1, None, None, 200, 3.0, lambda: (np.array([np.nan]), np.zeros(1), np.zeros(1)))


def test_direct_sum_reference_agrees_with_scipy():
    from scipy.stats import gaussian_kde
    rng = np.random.default_rng(3)
    x = rng.normal(size=500)
    k = gaussian_kde(x)
    h = float(np.sqrt(k.covariance[0, 0]))
    grid = np.linspace(x.min() - 3 * h, x.max() + 3 * h, 200)
    want = k.evaluate(grid)
    for dtype in (np.float64, np.longdouble):
        got = np.asarray(MR.kde_ref(x, grid, h, dtype=dtype), dtype=np.float64)
        assert np.max(np.abs(got - want) / want) < 1e-12


def test_edges_pairs_and_the_bound_factor():
    from gpemu import marginals as M
    e = M.bin_edges([0.0, -1.0], [1.0, 1.0], 4)
    assert np.array_equal(e[0], np.linspace(0.0, 1.0, 5)) and np.array_equal(e[1], np.linspace(-1.0, 1.0, 5))
    for bad in (([0.0], [0.0], 4), ([0.0], [np.inf], 4), ([0.0, 1.0], [1.0], 4), ([0.0], [1.0], 0)):
        with pytest.raises(ValueError):
            M.bin_edges(*bad)
    assert M.pair_indices(1).shape == (0, 2)
    assert M.pair_indices(4).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    # the summation depth the GPU test's bound assumes: one sample, one chunk, many chunks
    assert MR.kde_bound_factor(1) == 0.55 * (1 + 2 + 1 + 9 + 8)
    assert MR.kde_bound_factor(100003) == 0.55 * (2048 + 2 + 1 + 9 + 8)
