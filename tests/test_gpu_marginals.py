"""-m gpu tests of the marginal summaries on the device (gpemu_marginal_hist*, gpemu_hpd*, gpemu_kde1d*, gpemu.marginals,
DeviceSampler.marginals): histograms equal numpy's as integers, both ends of every highest-density
interval equal the restated narrowest-window rule as doubles, the kernel density stays within an error bound derived
from the kernel's own operations, and the sampler's in-place forms equal the module functions on the downloaded chain."""
import numpy as np
import pytest

import marginals_ref as MR

pytestmark = pytest.mark.gpu


def _counts():
    from gpemu import marginals as M
    return M.path_counts()


def _box(d, rng):
    lo = rng.uniform(-2.0, 0.0, d)
    return lo, lo + rng.uniform(0.5, 3.0, d)


def _check_hist(x, lo, hi, nb1, nb2, **kw):
    from gpemu import marginals as M
    got = M.histograms(x, lo, hi, nb1, nb2, **kw)
    h1, h2, ni = MR.hist_ref(x, got["edges_1d"], got["edges_2d"])
    d = x.shape[1]
    assert got["hist_1d"].dtype == np.int64 and got["hist_2d"].dtype == np.int64
    assert got["hist_1d"].shape == (d, nb1) and got["hist_2d"].shape == (d * (d - 1) // 2, nb2, nb2)
    assert np.array_equal(got["pairs"], M.pair_indices(d))
    assert np.array_equal(got["hist_1d"], h1), np.argwhere(got["hist_1d"] != h1)[:5]
    assert np.array_equal(got["hist_2d"], h2), np.argwhere(got["hist_2d"] != h2)[:5]
    assert np.array_equal(got["n_inside"], ni)
    return got


# ---- 1. histograms ---------------------------------------------------------------------------------------------------
# every S, d and bin count of the issue at least once; (4096, 256) needs a sweep per pair and one for the 1-D counters
HIST_SHAPES = [(1, 1, 1, 1), (2, 2, 2, 3), (63, 8, 7, 5), (64, 9, 100, 50), (65, 16, 2, 3), (2049, 2, 4096, 256),
               (2049, 16, 100, 50), (100003, 8, 100, 50), (100003, 1, 4096, 256), (2049, 9, 7, 5), (63, 16, 4096, 256)]


@pytest.mark.parametrize("S,d,nb1,nb2", HIST_SHAPES)
def test_histograms_equal_numpy_on_every_shape(S, d, nb1, nb2):
    rng = np.random.default_rng(S * 131 + d * 7 + nb1)
    lo, hi = _box(d, rng)
    x = rng.uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), (S, d))      # a few per cent outside the box
    _check_hist(x, lo, hi, nb1, nb2)


def _edge_data(kind, S, d, lo, hi, nb, rng):
    from gpemu import marginals as M
    e = M.bin_edges(lo, hi, nb)
    if kind == "uniform":
        return rng.uniform(lo, hi, (S, d))
    pick = np.stack([e[j][rng.integers(0, nb + 1, S)] for j in range(d)], axis=1)      # lo and hi included
    if kind == "on_edge":
        return pick
    if kind == "ulp":
        return np.nextafter(pick, np.where(rng.random((S, d)) < 0.5, -np.inf, np.inf))
    if kind == "outside":
        x = rng.uniform(lo - (hi - lo), hi + (hi - lo), (S, d))
        x[0], x[1] = lo, hi
        return x
    if kind == "special":
        x = rng.uniform(lo, hi, (S, d))
        m = rng.random((S, d))
        x[m < 0.1] = np.nan
        x[(m >= 0.1) & (m < 0.2)] = np.inf
        x[(m >= 0.2) & (m < 0.3)] = -np.inf
        x[(m >= 0.3) & (m < 0.4)] = -0.0
        x[(m >= 0.4) & (m < 0.5)] = 0.0
        return x
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["uniform", "on_edge", "ulp", "outside", "special"])
def test_histograms_equal_numpy_on_every_kind_of_data(kind):
    rng = np.random.default_rng(["uniform", "on_edge", "ulp", "outside", "special"].index(kind))
    d = 3
    lo, hi = np.array([-1.0, -2.0, 0.0]), np.array([1.0, 2.0, 3.0])        # linspace(-1, 1, 5) and (-2, 2, 5) hold 0.0
    for S, nb in ((2049, 4), (65, 100)):
        x = _edge_data(kind, S, d, lo, hi, nb, rng)
        got = _check_hist(x, lo, hi, nb, nb)
        if kind == "on_edge":
            assert np.all(got["n_inside"] == S)


def test_histograms_of_one_bin_under_contention_and_the_counters():
    # every sample in one bin: the worst case for the LDS atomics, and 100003 > 2^16 samples on one counter
    S, d = 100003, 8
    lo, hi = np.zeros(d), np.ones(d)
    x = np.full((S, d), 0.4)
    got = _check_hist(x, lo, hi, 100, 50)
    assert got["hist_1d"].max() == S and got["hist_2d"].max() == S and np.all(got["n_inside"] == S)


def test_histograms_in_the_block_layout_and_bit_identical_runs():
    import torch
    from gpemu import marginals as M
    rng = np.random.default_rng(5)
    steps, W, d = 61, 48, 8
    lo, hi = _box(d, rng)
    buf = rng.uniform(lo - 0.02, hi + 0.02, (steps, W, d))
    t = torch.as_tensor(buf, device="cuda")
    e1, e2 = M.bin_edges(lo, hi, 100), M.bin_edges(lo, hi, 50)
    # thinned by 3
    n_blocks = (steps + 2) // 3
    h1, h2, ni = M._hist_dev(0, t.data_ptr(), n_blocks, W, 3 * W, d, e1, e2)
    r1, r2, rn = MR.hist_ref(buf[::3].reshape(-1, d), e1, e2)
    assert np.array_equal(h1, r1) and np.array_equal(h2, r2) and np.array_equal(ni, rn)
    # walkers [w0, w0 + nw) of every step
    w0, nw = 16, 20
    h1, h2, ni = M._hist_dev(0, t.data_ptr() + 8 * w0 * d, steps, nw, W, d, e1, e2)
    r1, r2, rn = MR.hist_ref(buf[:, w0:w0 + nw].reshape(-1, d), e1, e2)
    assert np.array_equal(h1, r1) and np.array_equal(h2, r2) and np.array_equal(ni, rn)
    # two runs and three splits of the pairs over the sweeps give the same integers, and the sweeps are counted
    x = buf.reshape(-1, d)
    base = M.histograms(x, lo, hi, 100, 50)
    for group_counters, sweeps, groups in ((0, 1, 1), (2500 * 5, 6, 6), (2500, 29, 28)):
        c0 = _counts()
        for _ in range(2):
            got = M.histograms(x, lo, hi, 100, 50, group_counters=group_counters)
            for k in ("hist_1d", "hist_2d", "n_inside"):
                assert np.array_equal(got[k], base[k]), (k, group_counters)
        c1 = _counts()
        assert c1["HIST_SWEEP"] - c0["HIST_SWEEP"] == 2 * sweeps and c1["PAIR_GROUP"] - c0["PAIR_GROUP"] == 2 * groups
    # a device tensor is read in place
    got = M.histograms(t.reshape(-1, d), lo, hi, 100, 50)
    assert np.array_equal(got["hist_2d"], base["hist_2d"]) and np.array_equal(got["hist_1d"], base["hist_1d"])


def test_histogram_arguments_are_checked_before_any_launch():
    from gpemu import _lib
    from gpemu import marginals as M
    L = _lib.lib()
    x = np.zeros((4, 2))
    ok = M.bin_edges([0.0, 0.0], [1.0, 1.0], 4)
    h1, h2, ni = np.zeros((2, 4), np.int64), np.zeros((1, 4, 4), np.int64), np.zeros(2, np.int64)
    p = _lib.ptr
    c0 = _counts()

    def call(S=4, d=2, nb1=4, e1=ok, nb2=4, e2=ok, gc=0):
        return L.gpemu_marginal_hist(0, S, d, p(x), nb1, p(np.ascontiguousarray(e1)), nb2, p(np.ascontiguousarray(e2)), gc,
                                     p(h1), p(h2), p(ni))
    bad = ok.copy()
    bad[1, 2] = bad[1, 1]
    nan = ok.copy()
    nan[0, 0] = np.nan
    for kw in (dict(S=0), dict(S=2 ** 31), dict(d=0), dict(d=17), dict(nb1=0), dict(nb1=4097), dict(nb2=0), dict(nb2=257),
               dict(e1=bad), dict(e2=bad), dict(e1=nan), dict(gc=3), dict(gc=73729)):
        assert call(**kw) == -1, kw
    assert _counts() == c0
    assert call() == 0


# ---- 2. highest-density intervals -----------------------------------------------------------------------------------------
def _hpd_data(kind, R, S, rng):
    if kind == "normal":
        return rng.normal(size=(R, S))
    if kind == "duplicates":        # many tied widths: the smallest window must win
        return rng.integers(0, 8, (R, S)).astype(np.float64)
    if kind == "all_equal":
        return np.repeat(rng.normal(size=(R, 1)), S, axis=1)
    if kind == "low_bits":          # values that differ only in the low 11 bits
        base = np.float64(1.2345678901234567).view(np.uint64) & ~np.uint64(0x7FF)
        return (base | rng.integers(0, 2048, (R, S)).astype(np.uint64)).view(np.float64)
    if kind == "negative":
        return -np.abs(rng.normal(size=(R, S))) * 1e3
    raise KeyError(kind)


HPD_KINDS = ["normal", "duplicates", "all_equal", "low_bits", "negative"]
CONFIDENCES = (0.5, 0.68, 0.9, 0.99)


def _levels(S):
    """the confidences whose n_out is not 0 at this S"""
    return [c for c in CONFIDENCES if int((1 - c) * S) >= 1]


def _check_hpd(v, conf):
    """v: (R, S) rows; all levels at once and one alone"""
    from gpemu import marginals as M
    R, S = v.shape
    got = M.hpd_intervals(v.T, conf)
    assert got.shape == (len(conf), R, 2)
    for l, c in enumerate(conf):
        n_out = int((1 - c) * S)
        for r in range(R):
            want = MR.hpd_ref(v[r], n_out)
            assert (got[l, r, 0], got[l, r, 1]) == want, (c, r, got[l, r], want)
    one = M.hpd_intervals(v.T, conf[-1])
    assert one.shape == (R, 2) and np.array_equal(one, got[-1])


@pytest.mark.parametrize("S", [2, 3, 64, 2047, 2048, 2049, 100003])
@pytest.mark.parametrize("R", [1, 16])
def test_hpd_equals_the_window_rule_on_every_shape(R, S):
    rng = np.random.default_rng(R * 1000 + S)
    _check_hpd(_hpd_data("normal", R, S, rng), _levels(S))


@pytest.mark.parametrize("kind", HPD_KINDS)
def test_hpd_equals_the_window_rule_on_every_kind_of_data(kind):
    rng = np.random.default_rng(200 + HPD_KINDS.index(kind))
    for R, S in ((3, 64), (5, 5003)):
        _check_hpd(_hpd_data(kind, R, S, rng), _levels(S))


def test_hpd_through_the_c_abi_extremes_strides_and_bad_rows():
    import torch
    from gpemu import _lib
    from gpemu import marginals as M
    L, p = _lib.lib(), _lib.ptr
    rng = np.random.default_rng(7)
    R, S = 4, 4099
    v = rng.normal(size=(R, S))
    v[1] = rng.integers(0, 5, S)
    # n_out = 1 (the whole range) and n_out = S (the narrowest single point, the first of ties), with one in between
    n_out = np.array([1, S, 17], dtype=np.int64)
    out = np.empty((R, 3, 2))
    c0 = _counts()
    assert L.gpemu_hpd(0, R, S, p(v), 3, p(n_out), p(out)) == 0
    c1 = _counts()
    assert c1["SORT_BATCH"] - c0["SORT_BATCH"] == 1 and c1["WINDOW_SEARCH"] - c0["WINDOW_SEARCH"] == 1
    for r in range(R):
        s = np.sort(v[r])
        assert (out[r, 0, 0], out[r, 0, 1]) == (s[0], s[-1])
        assert (out[r, 1, 0], out[r, 1, 1]) == (s[0], s[0])
        assert (out[r, 2, 0], out[r, 2, 1]) == MR.hpd_ref(v[r], 17)
    # n_out of 0 or S + 1: refused before any launch
    for bad in ([0], [S + 1], [5, 0]):
        nb = np.array(bad, dtype=np.int64)
        assert L.gpemu_hpd(0, R, S, p(v), nb.size, p(nb), p(out)) == -1
    assert L.gpemu_hpd(0, R, S, p(v), 0, p(n_out), p(out)) == -1
    assert _counts() == c1
    # the strided form on a chain buffer [steps][W][d]: parameter j is the row with row_stride 1, elem_stride d
    steps, W, d = 50, 12, 5
    buf = rng.normal(size=(steps, W, d))
    t = torch.as_tensor(buf, device="cuda")
    n2 = M.n_outside([0.68, 0.9], steps * W)
    got = M._hpd_dev(0, t.data_ptr(), steps * W, d, n2)
    for l in range(2):
        for j in range(d):
            assert (got[l, j, 0], got[l, j, 1]) == MR.hpd_ref(buf[:, :, j].reshape(-1), int(n2[l]))
    # a small workspace sorts the rows in batches: the same intervals
    one = M._hpd_dev(0, t.data_ptr(), steps * W, d, n2, workspace_bytes=2 * (16 * steps * W + 1024 + 4 + 64))
    assert np.array_equal(one, got)
    with pytest.raises(_lib.GpemuError) as err:
        M._hpd_dev(0, t.data_ptr(), steps * W, d, n2, workspace_bytes=1000)
    assert err.value.code == -2 and "bytes" in str(err.value)
    # NaN and infinite extremes give NaN at every level; an interior row is not disturbed
    w = rng.normal(size=(4, 1000))
    w[0, 17] = np.nan
    w[1, 3] = np.inf
    w[2, 999] = -np.inf
    got = M.hpd_intervals(w.T, [0.5, 0.9])
    assert np.all(np.isnan(got[:, :3])) and np.all(np.isfinite(got[:, 3]))
    assert (got[1, 3, 0], got[1, 3, 1]) == MR.hpd_ref(w[3], int((1 - 0.9) * 1000))
    with pytest.raises(ValueError):
        M.hpd_intervals(rng.normal(size=(9, 2)), 0.9)        # int((1 - 0.9) * 9) = 0


# ---- 3. kernel density ------------------------------------------------------------------------------------------------
KDE_SHAPES = [(1, 1, 1), (2, 7, 16), (65, 200, 1), (4097, 513, 1), (4097, 200, 16), (100003, 200, 1), (100003, 7, 16)]


@pytest.mark.parametrize("S,G,R", KDE_SHAPES)
def test_kde_within_the_error_bound(S, G, R):
    """|got - ref| <= c eps (ref + 1 / (sqrt(2 pi) h)) against the direct sum in np.longdouble, eps = 2^-52 = 2 u.

    c comes from the kernel's operations (csrc/k_marginal.hip), to first order in u with 10 % added for the rest:
      * t = (g - x) * (1 / h): the difference, the reciprocal and the product round once each, |dt / t| <= 3 u;
      * a = -0.5 * (t * t): twice that and the product's rounding, |da / a| <= 7 u (the factor 0.5 is exact), so the
        term exp(a) moves by at most 7 u |a| exp(a) <= 7 u / e (|a| e^a <= 1 / e for a <= 0): an ABSOLUTE error per
        term -- after the factor 1 / (S h sqrt(2 pi)) and S terms it is (7 / e) u / (h sqrt(2 pi)), which is why the
        bound carries the second summand;
      * exp is accurate to 1 ulp = 2 u of the term (the device library's documented bound for fp64);
      * the sum adds non-negative terms, so each addition costs at most u of the total: ceil(min(S, 8192) / 4)
        additions per interleaved sum, 2 to join the four, ceil(chunks / 256) in the lane-strided sum over chunks,
        6 in the butterfly and 3 over the waves -- the depth;
      * the factor 1 / (S h sqrt(2 pi)) rounds five times on the host and the last product once: 6 u;
      * a term whose exponent is below -746 is skipped: it is below 2^-1076, nothing against u / (h sqrt(2 pi)).
    Together u ((depth + 2 + 6) ref + (7 / e) / (h sqrt(2 pi))) <= c eps (ref + 1 / (h sqrt(2 pi))) with
    c = 1.1 (depth + 8) / 2 (marginals_ref.kde_bound_factor; 7 / e < depth + 8).  The longdouble reference itself is
    good to S 2^-64 of the value, far inside."""
    from gpemu import marginals as M
    rng = np.random.default_rng(S * 7 + G * 3 + R)
    x = rng.normal(0.3, 1.7, (S, R)) * (1.0 + np.arange(R))
    sd = x.std(axis=0) if S > 1 else np.ones(R)
    sd = np.where(sd > 0, sd, 1.0)
    # bandwidths from 1e-3 to 10 standard deviations across the rows (and both ends for one row)
    # (the many-chunk shape takes the two extreme bandwidths: the reference there is 20 M longdouble terms each)
    single = [np.array([f]) for f in ((1e-3, 10.0) if S > 10000 else (1e-3, 0.3, 10.0))]
    for factors in ([np.geomspace(1e-3, 10.0, R)] if R > 1 else single):
        h = factors * sd
        grid = np.stack([np.linspace(x[:, r].min() - 3 * h[r], x[:, r].max() + 3 * h[r], G) for r in range(R)])
        if G >= 7:      # far outside the sample: the density underflows to exactly 0, in longdouble too
            grid[:, 0] = x.min(axis=0) - 1e6 * h
            grid[:, -1] = x.max(axis=0) + 1e6 * h
        got = M.kde_1d(x, grid=grid, bandwidth=h)
        assert got["density"].shape == (R, G) and np.array_equal(got["grid"], grid) and np.array_equal(got["bandwidth"], h)
        again = M.kde_1d(x, grid=grid, bandwidth=h)["density"]
        assert got["density"].tobytes() == again.tobytes()
        worst = 0.0
        for r in range(R):
            ref = MR.kde_ref(x[:, r], grid[r], h[r])
            tol = MR.kde_tolerance(S, h[r], ref)
            err = np.abs(got["density"][r].astype(np.longdouble) - ref)
            worst = max(worst, float(np.max(err / tol)))
            assert np.all(err <= tol), (r, h[r], float(np.max(err / tol)))
            if G >= 7:
                assert ref[0] == 0 and ref[-1] == 0 and got["density"][r, 0] == 0.0 and got["density"][r, -1] == 0.0
        print(f"kde S={S} G={G} R={R}: worst error / bound = {worst:.3e}")


def test_kde_defaults_device_tensors_and_arguments():
    import torch
    from gpemu import _lib
    from gpemu import marginals as M
    rng = np.random.default_rng(11)
    S, d = 5000, 3
    x = rng.normal(size=(S, d)) * np.array([1.0, 0.01, 30.0])
    c0 = _counts()
    host = M.kde_1d(x)
    assert _counts()["KDE"] - c0["KDE"] == 1
    assert host["grid"].shape == (d, 200) and host["density"].shape == (d, 200)
    assert np.allclose(host["bandwidth"], S ** -0.2 * x.std(axis=0, ddof=1), rtol=1e-14, atol=0.0)
    # a density: it integrates to 1 over its support (trapezoid; the tails beyond 3 h hold ~1e-3)
    area = np.sum(0.5 * (host["density"][:, 1:] + host["density"][:, :-1]) * np.diff(host["grid"], axis=1), axis=1)
    assert np.all(np.abs(area - 1.0) < 5e-3), area
    # the same samples on the device: bandwidth and support from the device moments and extremes, then the same kernel
    dev = M.kde_1d(torch.as_tensor(x, device="cuda"))
    assert np.allclose(dev["bandwidth"], host["bandwidth"], rtol=1e-12, atol=0.0)
    assert np.allclose(dev["grid"], host["grid"], rtol=0.0, atol=1e-12 * np.abs(host["grid"]).max())
    same = M.kde_1d(torch.as_tensor(x, device="cuda"), grid=host["grid"], bandwidth=host["bandwidth"])
    assert same["density"].tobytes() == host["density"].tobytes()
    L, p = _lib.lib(), _lib.ptr
    v, g, h, out = np.zeros((1, 4)), np.zeros((1, 3)), np.ones(1), np.zeros((1, 3))
    c1 = _counts()
    assert L.gpemu_kde1d(0, 1, 4, p(v), 0, p(g), p(h), p(out)) == -1
    assert L.gpemu_kde1d(0, 0, 4, p(v), 3, p(g), p(h), p(out)) == -1
    assert L.gpemu_kde1d(0, 1, 0, p(v), 3, p(g), p(h), p(out)) == -1
    assert L.gpemu_kde1d(0, 1, 4, p(v), 3, p(g), p(np.zeros(1)), p(out)) == -1
    assert L.gpemu_kde1d(0, 1, 4, p(v), 3, p(np.full((1, 3), np.nan)), p(h), p(out)) == -1
    assert _counts() == c1


# ---- 4. through the samplers ----------------------------------------------------------------------------------------------
def _same_marginals(got, chain2d, lo, hi, bins, conf, n_grid):
    """the in-place result against the module functions on the downloaded samples"""
    from gpemu import marginals as M
    want = M.histograms(chain2d, lo, hi, *bins)
    for k in ("edges_1d", "edges_2d", "hist_1d", "pairs", "hist_2d", "n_inside"):
        assert np.array_equal(got[k], want[k]), k
    hpd = M.hpd_intervals(chain2d, conf)
    assert got["hpd"].shape == hpd.shape and np.array_equal(got["hpd"], hpd)
    assert np.array_equal(got["confidence"], np.asarray(conf, dtype=np.float64))
    S = chain2d.shape[0]
    # the bandwidth and the support come from device moments and extremes: Scott's rule up to their rounding ...
    assert np.allclose(got["kde_bandwidth"], S ** -0.2 * chain2d.std(axis=0, ddof=1), rtol=1e-12, atol=0.0)
    assert got["kde_grid"].shape == (chain2d.shape[1], n_grid)
    assert np.array_equal(got["kde_grid"][:, 0], chain2d.min(axis=0) - 3.0 * got["kde_bandwidth"])
    # ... and the density on them is the module function's, bit for bit (the same code after the copy)
    dens = M.kde_1d(chain2d, grid=got["kde_grid"], bandwidth=got["kde_bandwidth"])["density"]
    assert got["kde_density"].tobytes() == dens.tobytes()


def test_sampler_marginals_equal_the_module_functions_on_the_downloaded_chain():
    import golden_util as GU
    from gpemu import diagnostics, model as gmodel, sensitivity
    from gpemu.sampler import DeviceSampler, HMCSampler, TemperedSampler
    model, prob, _ = GU.fixed_theta_model(200, 100, 5, seed=0)
    dm = GU.device_model(model)
    lo, hi = np.asarray(prob["lo"], dtype=np.float64), np.asarray(prob["hi"], dtype=np.float64)
    d, W, steps = lo.size, 32, 40
    rng = np.random.default_rng(3)
    dm.likelihood_setup(prob["y_exp"], prob["y_err"], lo, hi, 1.0)
    s = DeviceSampler([dm], W, seed=4)
    s.set_state(rng.uniform(lo, hi, (W, d)))
    s.run(steps)
    chain, _ = s.get_chain()

    def others():        # the counters of the families this call has no business with
        return (diagnostics.path_counts(), gmodel.postpred_path_counts().tolist(), gmodel.hmc_path_counts().tolist(),
                gmodel.grad_path_counts().tolist(), sensitivity.sobol_path_counts().tolist())
    c0, o0 = _counts(), others()
    got = s.marginals(bins_1d=20, bins_2d=10, confidence=(0.68, 0.9), n_grid=50)          # the prior box by default
    c1 = _counts()
    # in place: one sweep (every pair's 100 counters and the 1-D counters fit), one sort of all parameters for the levels
    # and the extremes, one density launch -- and no other family of counters moves
    assert {k: c1[k] - c0[k] for k in c1} == {"HIST_SWEEP": 1, "PAIR_GROUP": 1, "SORT_BATCH": 1, "WINDOW_SEARCH": 1, "KDE": 1}
    assert others() == o0
    _same_marginals(got, chain.reshape(-1, d), lo, hi, (20, 10), (0.68, 0.9), 50)
    # discard and thin: a dense copy for the sort and the density
    got = s.marginals(lower=lo, upper=hi, bins_1d=7, bins_2d=5, confidence=(0.5,), n_grid=33, discard=7, thin=3)
    _same_marginals(got, chain[7::3].reshape(-1, d), lo, hi, (7, 5), (0.5,), 33)
    no_kde = s.marginals(kde=False, discard=7, thin=3, confidence=(0.5,), bins_1d=7, bins_2d=5)
    assert "kde_density" not in no_kde and np.array_equal(no_kde["hpd"], got["hpd"])
    with pytest.raises(ValueError):
        s.marginals(discard=steps)
    with pytest.raises(ValueError):
        s.marginals(confidence=(0.9999999,))         # n_out = 0
    s.close()

    # a stacked sampler takes a chain index
    dm.likelihood_setup(np.stack([prob["y_exp"], prob["y_exp"] * 1.01]), prob["y_err"], lo, hi, 1.0)
    s2 = DeviceSampler([dm], W, seeds=[3, 4])
    s2.set_state(rng.uniform(lo, hi, (2 * W, d)))
    s2.run(steps)
    chain2, _ = s2.get_chain()
    with pytest.raises(ValueError):
        s2.marginals()
    got = s2.marginals(chain=1, bins_1d=20, bins_2d=10, n_grid=40, discard=2)
    _same_marginals(got, np.ascontiguousarray(chain2[2:, W:2 * W]).reshape(-1, d), lo, hi, (20, 10), (0.9,), 40)
    s2.close()

    dm.likelihood_setup(prob["y_exp"], prob["y_err"], lo, hi, 1.0)
    ts = TemperedSampler([dm], W, [1.0, 0.5, 0.1], seed=5, swap_every=2)
    ts.set_state(rng.uniform(lo, hi, (3 * W, d)))
    ts.run(steps)
    got = ts.marginals(bins_1d=20, bins_2d=10, n_grid=40, discard=4)       # rung 0
    _same_marginals(got, ts.get_chain(temp=0, discard=4)[0].reshape(-1, d), lo, hi, (20, 10), (0.9,), 40)
    got = ts.marginals(temp=2, bins_1d=20, bins_2d=10, n_grid=40)
    _same_marginals(got, ts.get_chain(temp=2)[0].reshape(-1, d), lo, hi, (20, 10), (0.9,), 40)
    ts.close()

    hs = HMCSampler([dm], W, n_leapfrog=3, step_size=0.05, seed=8)
    hs.set_state(rng.uniform(lo, hi, (W, d)))
    hs.run(steps)
    got = hs.marginals(bins_1d=20, bins_2d=10, n_grid=40, discard=5, thin=2)
    _same_marginals(got, hs.get_chain()[0][5::2].reshape(-1, d), lo, hi, (20, 10), (0.9,), 40)
    hs.close()
    dm.close()


def _host_log_prob(x):
    raise AssertionError("the device path does not call the host function")


def test_ensemble_sampler_get_marginals_in_place_and_from_the_host_copy():
    import pickle
    import golden_util as GU
    from gpemu import marginals as M
    from gpemu.sampler import EnsembleSampler
    model, prob, _ = GU.fixed_theta_model(200, 100, 5, seed=0)
    dm = GU.device_model(model)
    lo, hi = np.asarray(prob["lo"], dtype=np.float64), np.asarray(prob["hi"], dtype=np.float64)
    dm.likelihood_setup(prob["y_exp"], prob["y_err"], lo, hi, 1.0)

    _host_log_prob._gpemu_device_models = lambda: [dm]
    W, d = 32, lo.size
    es = EnsembleSampler(W, d, _host_log_prob, seed=2)
    es.run_mcmc(np.random.default_rng(1).uniform(lo, hi, (W, d)), 40)
    kw = dict(bins_1d=20, bins_2d=10, confidence=(0.68,), n_grid=30)
    live = es.get_marginals(discard=3, thin=2, **kw)
    flat = es.get_chain(discard=3, thin=2, flat=True)
    _same_marginals(live, flat, lo, hi, (20, 10), (0.68,), 30)
    del _host_log_prob._gpemu_device_models
    frozen = pickle.loads(pickle.dumps(es))
    with pytest.raises(ValueError):
        frozen.get_marginals(discard=3, thin=2, **kw)            # the host copy knows no box
    host = frozen.get_marginals(discard=3, thin=2, lower=lo, upper=hi, **kw)
    want = M.summary(flat, lo, hi, **kw)
    for k in M.KEYS:
        assert np.array_equal(host[k], want[k]), k
    for k in ("hist_1d", "hist_2d", "n_inside", "hpd"):
        assert np.array_equal(host[k], live[k]), k
    dm.close()
