"""-m gpu tests of the 2-D kernel densities on the device (gpemu_kde2d*, gpemu_pair_moments_dev, gpemu.marginals.kde_2d,
DeviceSampler.marginals(kde2d=True)): the panels stay within an error bound derived from the kernel's
own operations against the longdouble sheared product sum, agree with scipy as far as the reference does, do not depend
on the run or on the pair batches, and the sampler's in-place form equals the module function on the downloaded chain."""
import numpy as np
import pytest

import kde2d_ref as KR

pytestmark = pytest.mark.gpu

CHUNK = 8192          # K2_CHUNK of csrc/k_kde2d.hip: samples per partial tile (test_kde2d_host.py holds it to the source)
SCALES = (1.0, 0.01, 30.0)


def _counts():
    from gpemu import marginals as M
    return M.kde2d_path_counts()


def _others():
    """the counters of the families a 2-D density has no business with"""
    from gpemu import diagnostics, marginals as M, model as gmodel, sensitivity
    return (M.path_counts(), diagnostics.path_counts(), gmodel.postpred_path_counts().tolist(),
            gmodel.hmc_path_counts().tolist(), gmodel.grad_path_counts().tolist(), sensitivity.sobol_path_counts().tolist())


def _samples(S, d, seed):
    """columns of very different scales (1, 0.01, 30, ...), neighbours correlated, means away from 0"""
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(S, d))
    z[:, 1:] = 0.8 * z[:, :-1] + 0.6 * z[:, 1:]
    scale = np.array([SCALES[k % 3] for k in range(d)])
    return (z + 0.5 * np.arange(d)) * scale


def _explicit_plan(x, sheared, G, seed, factor=None):
    """pairs, shear, bandwidths and grids that ask nothing of the device: Scott-like bandwidths times factors from 0.05
    to 5 across the pairs (or times ``factor``), the support 3 h beyond the sample and, for G >= 5, the outermost points
    1e6 bandwidths away"""
    from gpemu import marginals as M
    S, d = x.shape
    rng = np.random.default_rng(seed)
    pairs = M.pair_indices(d)
    P = pairs.shape[0]
    c = np.atleast_2d(np.cov(x, rowvar=False)) if S > 1 else np.eye(d)
    beta = np.array([c[i, j] / c[i, i] for i, j in pairs]) * rng.uniform(0.5, 1.5, P) if sheared else np.zeros(P)
    f = S ** (-1.0 / 6.0) * (np.geomspace(0.05, 5.0, P)[rng.permutation(P)] if factor is None else np.full(P, factor))
    h, ga, gb = np.empty((P, 2)), np.empty((P, G)), np.empty((P, G))
    for p, (i, j) in enumerate(pairs):
        v = x[:, j] - beta[p] * x[:, i]
        h[p] = f[p] * x[:, i].std(), f[p] * v.std()
        ga[p] = np.linspace(x[:, i].min() - 3 * h[p, 0], x[:, i].max() + 3 * h[p, 0], G)
        gb[p] = np.linspace(v.min() - 3 * h[p, 1], v.max() + 3 * h[p, 1], G)
        if G >= 5:
            ga[p, 0], ga[p, -1] = x[:, i].min() - 1e6 * h[p, 0], x[:, i].max() + 1e6 * h[p, 0]
            gb[p, 0], gb[p, -1] = v.min() - 1e6 * h[p, 1], v.max() + 1e6 * h[p, 1]
    return dict(pairs=pairs, shear=beta, bandwidth=h, grid_a=ga, grid_b=gb)


def _ref_panel(x, plan, p):
    i, j = plan["pairs"][p]
    return KR.kde2d_ref(x[:, i], x[:, j], plan["shear"][p], plan["bandwidth"][p, 0], plan["bandwidth"][p, 1],
                        plan["grid_a"][p], plan["grid_b"][p])


# (the last three: the largest panel of the 64 x 64 tile, the smallest of the 128 x 128 tile, and two 128 x 128 tiles per
# axis with a ragged edge)
KDE2D_SHAPES = [(3, 5, 2), (65, 17, 2), (4097, 70, 3), (CHUNK + 1, 33, 2), (100003, 33, 2), (1000, 16, 16),
                (257, 64, 2), (257, 65, 2), (300, 130, 2)]


@pytest.mark.parametrize("sheared", [True, False], ids=["sheared", "aligned"])
@pytest.mark.parametrize("S,G,d", KDE2D_SHAPES)
def test_kde2d_within_the_error_bound(S, G, d, sheared):
    """|got - ref| <= c eps (ref + 1 / (2 pi h_a h_b)) + S DBL_MIN / (S 2 pi h_a h_b) against the sheared product sum in
    np.longdouble (kde2d_ref), eps = 2^-52 = 2 u.

    c comes from the kernel's operations (csrc/k_kde2d.hip), to first order in u with 10 % added for the rest:
      * t_a = (g_a - x) * (1 / h_a): the difference, the reciprocal and the product round once each, |dt / t| <= 3 u.
        t_b = ((g_b - v) - v_lo) * (1 / h_b): v + v_lo is y - beta x to second order (the rounding of the fma is carried
        beside it), so the difference is again relative to t_b, with one more rounding: 4 u;
      * a = -0.5 * (t * t): twice that and the product's rounding, |da / a| <= 9 u, so a factor exp(a) moves by at most
        9 u |a| exp(a) <= 9 u / e: an ABSOLUTE error, in units of the factor's peak 1.  A term is the product of two
        factors <= 1, so it moves by at most (7 + 9) u / e < 6 u; after S terms and the factor 1 / (S 2 pi h_a h_b)
        that is 6 u / (2 pi h_a h_b) -- why the bound carries the second summand;
      * exp is accurate to 1 ulp = 2 u of each factor: 4 u of the term; the product of the two factors inside the
        matrix instruction rounds at most once: 1 u;
      * the sums add non-negative terms, so each addition costs at most u of the total.  The longest chain of one
        output element: the samples of a chunk go through v_mfma_f64_16x16x4_f64 four at a time, counted as four
        additions per instruction -- min(S, 8192) additions that are not of an exact zero (the padding up to a
        multiple of 16 adds zeros, exactly) -- and the partial tiles are added one by one in chunk order:
        ceil(S / 8192) additions;
      * the factor 1 / (S 2 pi h_a h_b) rounds five times on the host (2 pi, three products, the reciprocal) and the
        last product once: 6 u;
      * a factor whose exponent is below -746 is skipped: it is below 2^-1076; a factor or a product below DBL_MIN
        loses its low bits or all of them -- at most DBL_MIN per term, the last summand.
    Together u ((depth + 4 + 1 + 6) ref + 6 / (2 pi h_a h_b)) <= c eps (ref + 1 / (2 pi h_a h_b)) with depth =
    min(S, 8192) + ceil(S / 8192) and c = 1.1 (depth + 11) / 2 (kde2d_ref.kde2d_bound_factor; 6 < depth + 11).  c stays
    below 0.55 (S + 16), what any order of S positive terms needs.  The longdouble reference is good to S 2^-64 of the
    value, far inside."""
    from gpemu import marginals as M
    x = _samples(S, d, seed=S + G + d)
    # many pairs: bandwidths from 0.05 to 5 times Scott's across them; one pair: each end and the middle in turn (the
    # many-chunk shape takes the two ends: its reference is 7 M longdouble terms each)
    factors = [None] if d > 2 else ([0.05, 5.0] if S > 10000 else [0.05, 1.0, 5.0])
    worst, peak_share = 0.0, 0.0
    for factor in factors:
        plan = _explicit_plan(x, sheared, G, seed=G, factor=factor)
        got = M.kde_2d(x, **plan)
        P = plan["pairs"].shape[0]
        assert got["density"].shape == (P, G, G) and got["density"].dtype == np.float64
        for k, v in plan.items():
            assert np.array_equal(got[k], v), k
        assert sheared == bool(np.all(plan["shear"] != 0.0))
        again = M.kde_2d(x, **plan)["density"]
        assert got["density"].tobytes() == again.tobytes()
        for p in range(P):
            ref = _ref_panel(x, plan, p)
            ha, hb = plan["bandwidth"][p]
            tol = KR.kde2d_tolerance(S, ha, hb, ref)
            err = np.abs(got["density"][p].astype(np.longdouble) - ref)
            worst = max(worst, float(np.max(err / tol)))
            peak_share = max(peak_share, float(ref.max()) * 2.0 * np.pi * ha * hb)
            assert np.all(err <= tol), (p, plan["pairs"][p], plan["bandwidth"][p], float(np.max(err / tol)))
            assert float(ref.max()) > 0.0
            if G >= 5:
                z = got["density"][p]
                for edge, redge in ((z[0], ref[0]), (z[-1], ref[-1]), (z[:, 0], ref[:, 0]), (z[:, -1], ref[:, -1])):
                    assert np.all(redge == 0) and np.all(edge == 0.0)
    print(f"kde2d S={S} G={G} d={d} {'sheared' if sheared else 'aligned'}: worst error / bound = {worst:.3e}"
          f" (largest density, in units of one kernel's peak times S / S: {peak_share:.3e})")
    assert peak_share > 0.05          # the grids meet the samples: the sums under test are not all tails


def test_pair_batches_do_not_change_a_bit():
    from gpemu import marginals as M
    S, G, d = 1000, 16, 16
    x = _samples(S, d, seed=S + G + d)
    plan = _explicit_plan(x, True, G, seed=G)
    c0 = _counts()
    one = M.kde_2d(x, **plan)["density"]
    c1 = _counts()
    assert {k: c1[k] - c0[k] for k in c1} == {"DENSITY": 1, "PAIR_BATCH": 1, "PARTIAL_SUM": 1, "MOMENTS": 0, "EXTENTS": 0}
    per_pair = 8 * G * G * 1                      # the partial tiles of a pair: one chunk
    many = M.kde_2d(x, workspace_bytes=50 * per_pair, **plan)["density"]
    c2 = _counts()
    assert {k: c2[k] - c1[k] for k in c2} == {"DENSITY": 3, "PAIR_BATCH": 3, "PARTIAL_SUM": 3, "MOMENTS": 0, "EXTENTS": 0}
    assert many.tobytes() == one.tobytes()
    single = M.kde_2d(x, workspace_bytes=per_pair, **plan)["density"]
    assert _counts()["PAIR_BATCH"] - c2["PAIR_BATCH"] == 120 and single.tobytes() == one.tobytes()
    from gpemu._lib import GpemuError
    with pytest.raises(GpemuError, match="out of memory"):
        M.kde_2d(x, workspace_bytes=per_pair - 1, **plan)
    # a pair on its own, or in the other order of its two parameters' neighbours, is the same panel
    sub = {k: v[7:9] for k, v in plan.items()}
    assert M.kde_2d(x, **sub)["density"].tobytes() == one[7:9].tobytes()


@pytest.mark.parametrize("S,G,d", [(4097, 33, 2), (65, 17, 3)])
def test_kde2d_default_plan_against_scipy(S, G, d):
    """Self-calibrating: the device panel is as close to scipy.stats.gaussian_kde on the plan's mesh as the longdouble
    reference is, plus the kernel's bound; and the panel is a density."""
    from scipy.stats import gaussian_kde
    from gpemu import marginals as M
    x = _samples(S, d, seed=S + d)
    got = M.kde_2d(x, n_grid=G)
    host = M.kde2d_plan_host(x, n_grid=G)
    for k in ("pairs", "shear", "bandwidth", "grid_a", "grid_b"):
        assert np.array_equal(got[k], host[k]), k
    for p, (i, j) in enumerate(got["pairs"]):
        ref = _ref_panel(x, got, p)
        X, Y = M.kde_2d_mesh(got, p)
        sp = gaussian_kde(np.stack([x[:, i], x[:, j]])).evaluate(np.stack([X.ravel(), Y.ravel()])).reshape(G, G)
        tol = KR.kde2d_tolerance(S, got["bandwidth"][p, 0], got["bandwidth"][p, 1], ref)
        dev_err = np.abs(got["density"][p].astype(np.longdouble) - sp)
        ref_err = np.abs(ref - sp)
        print(f"kde2d vs scipy S={S} pair ({i}, {j}): device {float(dev_err.max()):.3e}, reference {float(ref_err.max()):.3e},"
              f" peak {float(ref.max()):.3e}")
        assert np.all(dev_err <= ref_err + tol), (p, float(np.max(dev_err - ref_err - tol)))
        cell = (got["grid_a"][p, 1] - got["grid_a"][p, 0]) * (got["grid_b"][p, 1] - got["grid_b"][p, 0])
        area = float(got["density"][p].sum()) * cell
        assert abs(area - 1.0) < 5e-3, (p, area)


def test_kde2d_defaults_device_tensors_and_arguments():
    import torch
    from gpemu import _lib
    from gpemu import marginals as M
    rng = np.random.default_rng(11)
    S, d, G = 5000, 3, 40
    x = rng.normal(size=(S, d)) * np.array(SCALES)
    x[:, 2] += 20.0 * x[:, 0]
    c0, o0 = _counts(), _others()
    host = M.kde_2d(x, n_grid=G)
    c1 = _counts()
    # numpy samples: the plan is numpy's; one batch of pairs -- one density launch and one partial-sum launch
    assert {k: c1[k] - c0[k] for k in c1} == {"DENSITY": 1, "PAIR_BATCH": 1, "PARTIAL_SUM": 1, "MOMENTS": 0, "EXTENTS": 0}
    assert host["density"].shape == (3, G, G) and np.array_equal(host["pairs"], M.pair_indices(d))
    xt = torch.as_tensor(x, device="cuda")
    dev = M.kde_2d(xt, n_grid=G)
    c2 = _counts()
    # device samples: one moments pass (mean and covariance), one extents pass (x and v of every pair), then the same
    assert {k: c2[k] - c1[k] for k in c2} == {"DENSITY": 1, "PAIR_BATCH": 1, "PARTIAL_SUM": 1, "MOMENTS": 1, "EXTENTS": 1}
    assert _others() == o0
    assert np.array_equal(dev["pairs"], host["pairs"])
    assert np.allclose(dev["shear"], host["shear"], rtol=1e-12, atol=0.0)
    assert np.allclose(dev["bandwidth"], host["bandwidth"], rtol=1e-12, atol=0.0)
    for k in ("grid_a", "grid_b"):
        assert np.allclose(dev[k], host[k], rtol=0.0, atol=1e-12 * np.abs(host[k]).max()), k
    given = {k: host[k] for k in ("pairs", "shear", "bandwidth", "grid_a", "grid_b")}
    same = M.kde_2d(xt, **given)
    assert same["density"].tobytes() == host["density"].tobytes()
    diag = M.kde_2d(xt, covariance="diagonal", n_grid=G, pairs=[(2, 0)])
    assert diag["shear"].tolist() == [0.0] and diag["density"].shape == (1, G, G)
    assert np.allclose(diag["bandwidth"][0], S ** (-1 / 6) * x.std(axis=0, ddof=1)[[2, 0]], rtol=1e-12, atol=0.0)
    # the device moments themselves
    mean, cov, ext = M._pair_moments_dev(0, xt.data_ptr(), 1, S, S, d, host["pairs"], host["shear"])
    assert np.allclose(mean, x.mean(axis=0), rtol=1e-12, atol=1e-14 * np.abs(x).max())
    assert np.allclose(cov, np.cov(x, rowvar=False, ddof=0), rtol=1e-11, atol=0.0) and np.array_equal(cov, cov.T)
    for p, (i, j) in enumerate(host["pairs"]):
        v = x[:, j] - host["shear"][p] * x[:, i]
        assert np.allclose(ext[p], [v.min(), v.max()], rtol=0.0, atol=1e-13 * np.abs(x[:, j]).max())

    # one NaN sample: exactly the pairs that read its column are NaN, everywhere
    xn = x.copy()
    xn[123, 1] = np.nan
    nan = M.kde_2d(xn, **given)["density"]
    for p, (i, j) in enumerate(host["pairs"]):
        if 1 in (i, j):
            assert np.all(np.isnan(nan[p])), p
        else:
            assert nan[p].tobytes() == host["density"][p].tobytes()

    # every argument check returns -1 and launches nothing
    L, p = _lib.lib(), _lib.ptr
    X = np.zeros((4, 2))
    pr, sh, bw = np.array([[0, 1]], dtype=np.int64), np.zeros(1), np.ones((1, 2))
    g, out = np.zeros((1, 3)), np.zeros((1, 3, 3))
    i64 = lambda *v: np.array([v], dtype=np.int64)
    c3, o3 = _counts(), _others()
    call = lambda S=4, d=2, X=X, P=1, pr=pr, sh=sh, bw=bw, G=3, ga=g, gb=g, ws=0: L.gpemu_kde2d(
        0, S, d, p(X), P, p(pr), p(sh), p(bw), G, p(ga), p(gb), p(out), ws)
    assert call() == 0
    c4 = _counts()
    assert c4["DENSITY"] - c3["DENSITY"] == 1
    big = np.zeros((1, 513))
    bad = [dict(P=0), dict(G=0), dict(G=513, ga=big, gb=big), dict(d=0), dict(d=17), dict(S=0), dict(S=2 ** 31),
           dict(pr=i64(0, 2)), dict(pr=i64(-1, 1)), dict(pr=i64(1, 1)), dict(bw=np.array([[1.0, 0.0]])),
           dict(bw=np.array([[-1.0, 1.0]])), dict(bw=np.array([[np.inf, 1.0]])), dict(bw=np.array([[1.0, np.nan]])),
           dict(ga=np.array([[0.0, np.nan, 1.0]])), dict(gb=np.array([[0.0, np.inf, 1.0]])), dict(sh=np.array([np.nan])),
           dict(sh=np.array([np.inf])), dict(ws=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert _lib.last_error(), kw
    dX = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    dout = torch.zeros((1, 3, 3), dtype=torch.float64, device="cuda")
    dev_call = lambda nb=1, br=4, bs=4, d=2, P=1, pr=pr: L.gpemu_kde2d_dev(
        0, dX.data_ptr(), nb, br, bs, d, P, p(pr), p(sh), p(bw), 3, p(g), p(g), dout.data_ptr(), 0, None)
    for kw in (dict(nb=0), dict(br=0), dict(nb=2, br=2, bs=1), dict(nb=2 ** 20, br=2 ** 11, bs=2 ** 11), dict(d=17),
               dict(P=0), dict(pr=i64(0, 0))):
        assert dev_call(**kw) == -1, kw
    mom = lambda d=2, P=1, pr=pr, sh=sh: L.gpemu_pair_moments_dev(0, dX.data_ptr(), 1, 4, 4, d, None, None, P, p(pr), p(sh),
                                                                 p(np.zeros((1, 2))), None)
    for kw in (dict(d=0), dict(P=0), dict(pr=i64(0, 2)), dict(pr=i64(1, 1)), dict(sh=np.array([np.nan]))):
        assert mom(**kw) == -1, kw
    assert _counts() == c4 and _others() == o3
    with pytest.raises(ValueError):
        M.kde_2d(x[:, :1])
    with pytest.raises(ValueError):
        M.kde_2d(x[:2])


def _same_kde2d(got, chain2d, G, covariance="full"):
    """the in-place result against the module function on the downloaded samples"""
    from gpemu import marginals as M
    want = M.kde2d_plan_host(chain2d, covariance=covariance, n_grid=G)
    d = chain2d.shape[1]
    P = d * (d - 1) // 2
    assert got["kde2d_density"].shape == (P, G, G) and got["kde2d_grid_a"].shape == (P, G)
    assert np.array_equal(got["kde2d_pairs"], want["pairs"])
    # the plan comes from device moments and extents: numpy's up to their rounding ...
    assert np.allclose(got["kde2d_shear"], want["shear"], rtol=1e-10, atol=1e-13 * np.abs(want["shear"]).max())
    assert np.allclose(got["kde2d_bandwidth"], want["bandwidth"], rtol=1e-10, atol=0.0)
    for k in ("grid_a", "grid_b"):
        assert np.allclose(got["kde2d_" + k], want[k], rtol=0.0, atol=1e-10 * np.abs(want[k]).max()), k
    # ... and the density on it is the module function's, bit for bit (the same kernel on the same rows)
    given = {k: got["kde2d_" + k] for k in ("pairs", "shear", "bandwidth", "grid_a", "grid_b")}
    dens = M.kde_2d(chain2d, **given)["density"]
    assert got["kde2d_density"].tobytes() == dens.tobytes()
    assert np.all(np.isfinite(dens)) and np.all(dens.max(axis=(1, 2)) > 0.0)


def test_sampler_kde2d_equals_the_module_function_on_the_downloaded_chain():
    import golden_util as GU
    from gpemu import marginals as M
    from gpemu.sampler import DeviceSampler, TemperedSampler
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
    kw = dict(bins_1d=20, bins_2d=10, n_grid=30)
    m0, c0, o0 = M.path_counts(), _counts(), _others()[1:]
    plain = s.marginals(**kw)
    assert set(plain) == set(M.KEYS) and _counts() == c0          # the default: today's keys, no launch of this family
    m1 = M.path_counts()
    got = s.marginals(kde2d=True, n_grid_2d=20, **kw)
    c1, m2 = _counts(), M.path_counts()
    assert set(got) == set(M.KEYS) | set(M.KEYS_KDE2D)
    assert {k: c1[k] - c0[k] for k in c1} == {"DENSITY": 1, "PAIR_BATCH": 1, "PARTIAL_SUM": 1, "MOMENTS": 1, "EXTENTS": 1}
    assert {k: m2[k] - m1[k] for k in m2} == {k: m1[k] - m0[k] for k in m1} and _others()[1:] == o0
    for k in M.KEYS:
        assert np.array_equal(got[k], plain[k]), k
    _same_kde2d(got, chain.reshape(-1, d), 20)
    # discard and thin: the blocks of the view are read in place
    got = s.marginals(kde2d=True, n_grid_2d=17, covariance_2d="diagonal", discard=7, thin=3, **kw)
    assert np.all(got["kde2d_shear"] == 0.0)
    _same_kde2d(got, chain[7::3].reshape(-1, d), 17, "diagonal")
    with pytest.raises(ValueError):
        s.marginals(kde2d=True, covariance_2d="scott", **kw)
    with pytest.raises(ValueError):
        s.marginals(kde2d=True, n_grid_2d=513, **kw)
    s.close()

    # one chain of a stacked sampler
    dm.likelihood_setup(np.stack([prob["y_exp"], prob["y_exp"] * 1.01]), prob["y_err"], lo, hi, 1.0)
    s2 = DeviceSampler([dm], W, seeds=[3, 4])
    s2.set_state(rng.uniform(lo, hi, (2 * W, d)))
    s2.run(steps)
    chain2, _ = s2.get_chain()
    got = s2.marginals(chain=1, kde2d=True, n_grid_2d=12, discard=2, **kw)
    _same_kde2d(got, np.ascontiguousarray(chain2[2:, W:2 * W]).reshape(-1, d), 12)
    s2.close()

    dm.likelihood_setup(prob["y_exp"], prob["y_err"], lo, hi, 1.0)
    ts = TemperedSampler([dm], W, [1.0, 0.5], seed=5, swap_every=2)
    ts.set_state(rng.uniform(lo, hi, (2 * W, d)))
    ts.run(steps)
    got = ts.marginals(temp=1, kde2d=True, n_grid_2d=12, discard=4, **kw)
    _same_kde2d(got, ts.get_chain(temp=1, discard=4)[0].reshape(-1, d), 12)
    ts.close()
    dm.close()
