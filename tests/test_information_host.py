"""Host-side checks of the k-th neighbour information estimators (gpemu/information.py): the numpy
reference against scipy's tree, the reference estimators against the analytic Gaussian cases, the subsets, the rules of
use, the drop-in's settings and the exported symbols.  No device is needed."""
import os
import re

import numpy as np
import pytest

import information_ref as R


def _gauss(d, n=4096, sigma=0.05, seed=0, mean=0.5):
    return mean + sigma * np.random.default_rng(seed).standard_normal((n, d))


@pytest.mark.parametrize("d,k", [(1, 1), (2, 4), (3, 4), (6, 5), (16, 16)])
def test_reference_kth_distances_are_the_trees(d, k):
    """Copy-free data: the brute force in longdouble and cKDTree.query (float64) agree to 1e-12 relative, in a self
    search, in a cross search and in a subset of the coordinates."""
    rng = np.random.default_rng(d)
    u, v = rng.random((300, d)), rng.random((257, d))
    subsets = [tuple(range(d)), (d - 1,)] + ([(0, d - 1)] if d > 2 else [])
    r2, zeros = R.knn(u, None, k, subsets)
    assert np.array_equal(zeros, np.ones_like(zeros))            # every row finds itself, and nothing else
    c2, z2 = R.knn(u, v, k, subsets)
    assert not z2.any()
    for p, s in enumerate(subsets):
        assert np.allclose(r2[p].astype(np.float64), R.tree_kth_sq(u, None, k, s), rtol=1e-12, atol=0)
        assert np.allclose(c2[p].astype(np.float64), R.tree_kth_sq(u, v, k, s), rtol=1e-12, atol=0)


def test_reference_zero_distance_rule():
    u = np.array([[0.1, 0.2], [0.1, 0.7], [0.1, 0.2], [0.4, 0.2], [np.nan, 0.3]])
    r2, zeros = R.knn(u, None, 1, [(0,), (1,), (0, 1)])
    # coordinate 0: rows 0, 1, 2 coincide; the only other value is 0.4; the NaN row is no reference and gets NaN
    assert zeros[0].tolist() == [3, 3, 3, 1, 0] and np.isnan(r2[0, 4])
    assert np.allclose(r2[0, :4].astype(float), [0.09, 0.09, 0.09, 0.09])
    # coordinate 1 is finite in every row: 0.2 three times, then 0.3 (the NaN row's) is the nearest other
    assert zeros[1].tolist() == [3, 1, 3, 3, 1]
    assert np.allclose(r2[1].astype(float), [0.01, 0.16, 0.01, 0.01, 0.01])
    assert zeros[2].tolist() == [2, 1, 2, 1, 0]
    # fewer than k others: +inf
    r2, _ = R.knn(u[:4], None, 4, [(0,)])
    assert np.all(np.isinf(r2.astype(float)))


@pytest.mark.parametrize("d", [3, 2])
def test_reference_estimator_reproduces_the_gaussian_gain(d):
    """x = 0.5 + 0.05 N(0, I), default_rng(0).standard_normal((n, d)), n = 4096, k = 4 against -(d / 2) log(2 pi e
    0.05^2): within max(4 se, 0.1) nats -- a sanity bound on the estimator at these seeds, not on the kernel.  With
    this draw: 4.7767 against 4.7304 (se 0.019) for d = 3, 3.1502 against 3.1536 (se 0.017) for d = 2."""
    x = _gauss(d)
    assert x.min() > 0.0 and x.max() < 1.0
    est, se = R.tree_information_gain(x, k=4)
    exact = R.gaussian_gain(d, 0.05)
    print(f"d = {d}: estimate {est:.4f}, analytic {exact:.4f}, se {se:.4f}")
    assert abs(est - exact) <= max(4.0 * se, 0.1)


def test_reference_estimator_reproduces_the_gaussian_divergence():
    """0.05-wide against 0.07-wide Gaussians 0.02 apart per coordinate, d = 3, k = 4 (y from default_rng(1)): 0.4369
    against 0.3972 (se 0.015), within max(4 se, 0.1) nats."""
    x = _gauss(3)
    y = 0.52 + 0.07 * np.random.default_rng(1).standard_normal((4096, 3))
    est, se = R.tree_kl_divergence(x, y, k=4)
    exact = R.gaussian_kl(3, 0.05, 0.07, 0.02)
    print(f"estimate {est:.4f}, analytic {exact:.4f}, se {se:.4f}")
    assert abs(exact - 0.3972) < 1e-4
    assert abs(est - exact) <= max(4.0 * se, 0.1)


def test_small_brute_force_estimate_is_the_trees():
    x = _gauss(3, n=400)
    out = R.information_gain(x, np.zeros(3), np.ones(3), k=4, subsets=[(0, 1, 2)])
    est, se = R.tree_information_gain(x, k=4)
    assert abs(out["nats"][0] - est) < 1e-11 and abs(out["se"][0] - se) < 1e-11


def test_default_subsets_and_checks():
    from gpemu import information as I
    from gpemu import marginals as M
    for d in (1, 2, 3, 6, 16):
        subs = I.default_subsets(d)
        assert subs == R.default_subsets(d)
        assert subs[:d] == [(j,) for j in range(d)]
        assert subs[d:d + d * (d - 1) // 2] == [tuple(p) for p in M.pair_indices(d).tolist()]
        assert len(subs) == d + d * (d - 1) // 2 + (d > 2)
    subs, masks = I.check_subsets([(2, 0), 1, [3]], 4)
    assert subs == [(0, 2), (1,), (3,)] and masks.tolist() == [5, 2, 8] and masks.dtype == np.uint32
    for bad, err in (([], ValueError), ([()], ValueError), ([(0, 0)], ValueError), ([(4,)], IndexError),
                     ([(-1,)], IndexError)):
        with pytest.raises(err):
            I.check_subsets(bad, 4)
    with pytest.raises(ValueError):
        I.default_subsets(17)
    for k in (0, 17, 2.5):
        with pytest.raises(ValueError):
            I.check_k(k)
    assert I.selected_rows(10, 4).tolist() == [0, 2, 5, 7] == R.selected_rows(10, 4).tolist()
    assert I.selected_rows(3, 100).tolist() == [0, 1, 2]


def test_constants_follow_scipy():
    from scipy.special import digamma
    from gpemu import information as I
    for n in (1, 2, 4, 16, 63, 64, 65, 4096, 65536, 2 ** 31 - 1):
        assert abs(I.digamma_int(n) - float(digamma(n))) <= 4e-16 * max(1.0, abs(float(digamma(n))))
    for d in range(1, 17):
        # two terms of up to 28 in magnitude, each within an ulp (3.6e-15)
        assert abs(I.log_unit_ball(d) - R.log_unit_ball(d)) <= 4e-15
    assert abs(I.log_unit_ball(2) - np.log(np.pi)) < 1e-15 and abs(I.log_unit_ball(1) - np.log(2.0)) < 1e-15


def test_host_unit_rows_are_the_references():
    from gpemu import information as I
    rng = np.random.default_rng(2)
    x = rng.normal(size=(50, 3))
    x[7, 1] = np.nan
    x[9, 2] = np.inf
    lo, hi = np.array([-4.0, -5.0, -3.0]), np.array([4.5, 5.0, 7.0])
    u, skipped = I.unit_rows(x, lo, hi, 20)
    ur, sr = R.unit_rows(x, lo, hi, 20)
    assert skipped == sr == int((~np.isfinite(x[R.selected_rows(50, 20)]).all(axis=1)).sum())
    assert u.tobytes() == ur.tobytes()
    with pytest.raises(ValueError):
        I.unit_rows(x, hi, lo)


def test_rules_of_use():
    """_finish: rows with too few distinct neighbours always raise; copies beyond a tenth raise unless allowed, and the
    message says what to do about it."""
    from gpemu import information as I
    subs = [(0,), (0, 1)]
    sums = np.array([[-10.0, 60.0], [-12.0, 80.0]])
    ok = np.array([[2, 0, 2], [2, 0, 2]], dtype=np.int64)
    mean, sem, n_used, copies = I._finish(subs, 2, 4, ok, sums, 2, True, False, "t")
    assert mean.tolist() == [-5.0, -6.0] and n_used.tolist() == [2, 2] and copies.tolist() == [0, 0]
    assert np.allclose(sem, np.sqrt(np.array([10.0, 8.0]) / 2.0))
    with pytest.raises(ValueError, match="fewer than k = 4 distinct neighbours"):
        I._finish(subs, 2, 4, np.array([[2, 0, 2], [1, 1, 2]], dtype=np.int64), sums, 2, True, True, "t")
    many = np.array([[20, 0, 23], [20, 0, 22]], dtype=np.int64)
    with pytest.raises(ValueError, match="thin the chain by its autocorrelation time"):
        I._finish(subs, 2, 4, many, sums, 20, True, False, "t")
    assert I._finish(subs, 2, 4, many, sums, 20, True, True, "t")[3].tolist() == [3, 2]
    assert I._finish(subs, 2, 4, np.array([[20, 0, 22], [20, 0, 22]], dtype=np.int64), sums, 20, True, False,
                     "t")[3].tolist() == [2, 2]                  # exactly a tenth is allowed
    assert I.MAX_COPIES == 0.1


def test_information_gain_settings_validation():
    from bayesian_inference import mcmc
    assert mcmc.information_gain_settings({}) == (False, 4, 65536)
    assert mcmc.information_gain_settings({"information_gain": True, "information_gain_k": 16,
                                           "information_gain_max_points": 2}) == (True, 16, 2)
    for bad in ({"information_gain": 1}, {"information_gain": "yes"}, {"information_gain_k": 0},
                {"information_gain_k": 17}, {"information_gain_k": 4.0}, {"information_gain_k": True},
                {"information_gain_max_points": 1}, {"information_gain_max_points": 2 ** 31},
                {"information_gain_max_points": "all"}):
        with pytest.raises(ValueError, match="parameters.mcmc.information_gain"):
            mcmc.information_gain_settings(bad)
    assert {"information_gain_" + k for k in mcmc.INFORMATION_GAIN_KEYS} >= {
        "information_gain_nats", "information_gain_bits", "information_gain_se", "information_gain_joint",
        "information_gain_per_parameter", "information_gain_per_pair", "information_gain_copies"}


def test_new_symbols_paths_and_constants():
    from gpemu import _lib
    from gpemu import information as I
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gpemu.h")).read()
    declared = set(re.findall(r"\b(gpemu_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in ("gpemu_unit_rows_dev", "gpemu_knn_dist", "gpemu_knn_dist_dev", "gpemu_knn_logsum_dev",
                 "gpemu_knn_path_counts"):
        assert name in declared and name in _lib.exported_symbols() and hasattr(L, name), name
    enum = re.search(r"enum gpemu_knn_path \{(.*?)\};", hdr, re.S).group(1)
    names = re.findall(r"GPEMU_KNN_PATH_([A-Z0-9_]+?)\b", enum)
    assert names[:-1] == list(I.PATHS) == ["UNIT_ROWS", "SEARCH", "MERGE", "SUBSET_BATCH", "LOGSUM"]
    assert names[-1] == "COUNT"
    assert int(re.search(r"#define GPEMU_KNN_REF_TILE (\d+)", hdr).group(1)) == I.REF_TILE
    assert int(re.search(r"#define GPEMU_KNN_MAX_K (\d+)", hdr).group(1)) == I.MAX_K
    assert "plot_qhat.py:116" in hdr and "plot_analyses.py:144" in hdr
