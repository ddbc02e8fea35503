"""-m gpu tests of the chain diagnostics on the device: exact average ranks (gpemu_rank*), the
transformed split chains and their chain-averaged autocovariances (gpemu_diag_*), the five diagnostics
(gpemu.diagnostics), the sampler methods and the drop-in switch, against tests/diag_ref.py.

Tolerances.  Ranks are exact.  A normal score is compared with scipy.special.ndtri at the same probability, the
deviation in units of max(|z|, 1): the test allows 4x what the first GPU run measures (Z_DEV_MEASURED), capped at 1e-13
(a wrong branch of an inverse-normal approximation is off by more than 1e-9).  No GPU run had been made when this file was
written: until Z_DEV_MEASURED is filled in from the printed "z deviation" lines, the cap is the limit.  Moments and lag sums lie within their
a-priori bounds (diag_ref.acov_bound, moment_bounds) with that allowance for the scores.  The diagnostics stay within
4x the deviation the reference shows when g, W and b move by those bounds (8 random sign patterns; the 4 covers the
patterns not drawn); tests/test_diagnostics_host.py shows that no such move changes a branch of the scan."""
import numpy as np
import pytest
from scipy.special import ndtri
from scipy.stats import rankdata

import diag_ref as R
from test_gpu_select import KINDS as DATA_KINDS
from test_gpu_select import _data

pytestmark = pytest.mark.gpu

# The largest deviation of a device normal score from ndtri that the first GPU run of these tests printed ("z deviation"
# lines), or None while no GPU run has been made: the cap alone stands in then, the widest limit the rule allows.
Z_DEV_MEASURED = None
Z_CAP = 1e-13 if Z_DEV_MEASURED is None else min(4.0 * Z_DEV_MEASURED, 1e-13)

RANK_SHAPES = [(1, 1), (3, 2), (2, 255), (2, 256), (2, 257), (3, 4099), (3, 70001), (1, 2 ** 20 + 5)]
CASES = [(shape, seed) for shape in R.SHAPES for seed in R.SEEDS]


def _kinds():
    from gpemu import diagnostics as D
    return {"rank_z": (D.RANK_Z, 0.0), "folded_rank_z": (D.FOLDED_RANK_Z, 0.0), "le_05": (D.INDICATOR_LE, 0.05),
            "le_95": (D.INDICATOR_LE, 0.95), "identity": (D.IDENTITY, 0.0)}


def _counts():
    from gpemu import diagnostics as D
    return D.path_counts()


def _same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


# ---- 1. ranks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R_,S", RANK_SHAPES)
def test_ranks_equal_scipy_on_every_shape(R_, S):
    from gpemu import select
    rng = np.random.default_rng(R_ * 31 + S)
    v = rng.normal(size=(R_, S))
    v[:, ::3] = np.round(v[:, ::3], 1)            # ties among a third of the values
    got = select.rankdata(v)
    assert _same_bits(got, rankdata(v, method="average", axis=-1)), np.argwhere(got != rankdata(v, axis=-1))[:5]


@pytest.mark.parametrize("kind", DATA_KINDS)
def test_ranks_equal_scipy_on_every_kind_of_data_dense_and_strided(kind):
    import torch
    from gpemu import select
    rng = np.random.default_rng(200 + DATA_KINDS.index(kind))
    for R_, S in [(3, 2), (2, 257), (3, 4099)]:
        v = _data(kind, R_, S, rng)
        want = rankdata(v, method="average", axis=-1)
        assert _same_bits(select.rankdata(v), want), (kind, R_, S, "dense")
        # chain-strided: parameter r of a chain [S][R_] with row_stride 1 and elem_stride R_ (= 3), read in place
        t = torch.as_tensor(np.ascontiguousarray(v.T), device="cuda")
        assert t.stride(0) == R_ or S == 1
        got = select.rankdata(t, axis=0)
        assert got.shape == t.shape and _same_bits(got.cpu().numpy().T, want), (kind, R_, S, "strided")


def test_rank_of_a_nan_row_is_nan_and_axis_argument():
    from gpemu import select
    rng = np.random.default_rng(5)
    v = rng.normal(size=(3, 600))
    v[1, 77] = np.nan
    got = select.rankdata(v)
    assert np.all(np.isnan(got[1])) and _same_bits(got[[0, 2]], rankdata(v[[0, 2]], axis=-1))
    w = rng.integers(0, 5, (4, 7, 5)).astype(np.float64)
    assert _same_bits(select.rankdata(w, axis=1), rankdata(w, method="average", axis=1))


def test_ranks_do_not_depend_on_the_workspace():
    """A workspace of one row's sort buffers forces one row per batch: the same bits, and the counters show it."""
    import torch
    from gpemu import _lib, select
    rng = np.random.default_rng(6)
    R_, S = 5, 4099
    v = np.round(rng.normal(size=(R_, S)), 2)
    t = torch.as_tensor(v, device="cuda")
    c0 = _counts()
    whole = select.rankdata(t).cpu().numpy()
    c1 = _counts()
    one_row = 16 * S + 1024 * ((S + 2047) // 2048) + 4
    batched = select.rankdata(t, workspace_bytes=one_row).cpu().numpy()
    c2 = _counts()
    assert _same_bits(whole, batched) and _same_bits(whole, rankdata(v, axis=-1))
    assert (c1["ROW_BATCH"] - c0["ROW_BATCH"], c1["SORT_PASS"] - c0["SORT_PASS"]) == (1, 8)
    assert (c2["ROW_BATCH"] - c1["ROW_BATCH"], c2["SORT_PASS"] - c1["SORT_PASS"]) == (R_, 8 * R_)
    assert c2["RANK_LOOKUP"] - c1["RANK_LOOKUP"] == R_
    with pytest.raises(_lib.GpemuError) as err:      # not one row fits: the sizes are in the text
        select.rankdata(t, workspace_bytes=one_row - 1)
    assert err.value.code == -2 and str(one_row) in str(err.value)
    assert _counts() == c2


# ---- 2. transforms and lag sums ---------------------------------------------------------------------------------------
def _z_deviation(y_dev, ref_before_z):
    """Largest deviation of the device's normal scores from ndtri at the same probability, in units of max(|z|, 1)."""
    z = ndtri(R.rank_prob(ref_before_z))
    return float(np.max(np.abs(y_dev - z) / np.maximum(np.abs(z), 1.0)))


@pytest.mark.parametrize("shape,seed", CASES)
def test_transforms_moments_and_lag_sums(shape, seed):
    """The transformed series element by element (identity and indicators exactly, normal scores against ndtri at the
    same probability); the split chains' moments and every g[l] the reference's scan reads (lags up to max_t + 2),
    requested as blocks of 64, within the a-priori bounds."""
    from gpemu import diagnostics as D
    c = R.case(shape, seed)
    n, M, d = shape
    N, K, x = c["N"], c["K"], c["x"]
    bounds = R.case_bounds(c, Z_CAP)
    worst = {"z": 0.0, "moments": 0.0, "g": 0.0}
    c0 = _counts()
    with D.Diag(x) as h:
        assert (h.N, h.K) == (N, K)
        for k, (kind, prob) in _kinds().items():
            gm, W, b = h.transform(kind, prob)
            Y = h.series()
            lo, hi = h.value_range()
            L = max(per[k]["g"].size for per in c["kinds"])
            g = np.concatenate([h.acov(l0, min(64, N - l0)) for l0 in range(0, L, 64)], axis=0)
            for dd in range(d):
                ref = c["kinds"][dd][k]
                if k == "rank_z":
                    worst["z"] = max(worst["z"], _z_deviation(Y[:, :, dd], R.split(x[:, :, dd])))
                elif k == "folded_rank_z":
                    worst["z"] = max(worst["z"], _z_deviation(Y[:, :, dd], R.split(np.abs(x[:, :, dd] - np.median(x[:, :, dd])))))
                else:
                    assert _same_bits(Y[:, :, dd], ref["y"]), (k, dd)
                assert (lo[dd], hi[dd]) == (Y[:, :, dd].min(), Y[:, :, dd].max())
                (egm, eW, eb), eg = bounds[dd][k]
                for got, want, e in zip((gm[dd], W[dd], b[dd]), ref["moments"], (egm, eW, eb)):
                    assert abs(got - want) <= e, (k, dd, got, want, e)
                    if e > 0:
                        worst["moments"] = max(worst["moments"], abs(got - want) / e)
                err = np.abs(g[:eg.size, dd] - ref["g"])
                assert np.all(err <= eg), (k, dd, int(np.argmax(err - eg)), err.max())
                worst["g"] = max(worst["g"], float(np.max(err[eg > 0] / eg[eg > 0])) if np.any(eg > 0) else 0.0)
    dc = {k: v - c0[k] for k, v in _counts().items()}
    assert dc["TRANSFORM"] == 5 and dc["SORT_PASS"] == 16 and dc["RANK_LOOKUP"] == 2, dc
    print(f"\n{shape} seed {seed}: z deviation {worst['z']:.2e} (limit {Z_CAP:.2e}); moments at {worst['moments']:.2e} and "
          f"lag sums at {worst['g']:.2e} of their bounds")
    assert worst["z"] <= Z_CAP


def test_normal_scores_in_the_tails():
    """Chains without ties at sizes whose extreme probabilities reach the tail branch of an inverse-normal
    approximation (S up to 48 000: p down to 1.3e-5)."""
    from gpemu import diagnostics as D
    worst = 0.0
    for M in (1, 50, 6000):
        x = np.random.default_rng(M).permutation(8 * M).astype(np.float64).reshape(8, M, 1)
        with D.Diag(x) as h:
            h.transform(D.RANK_Z)
            worst = max(worst, _z_deviation(h.series()[:, :, 0], R.split(x[:, :, 0])))
    print(f"\nnormal scores of 8 .. 48 000 distinct values: deviation {worst:.2e} (limit {Z_CAP:.2e})")
    assert worst <= Z_CAP


# ---- 3. the diagnostics -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", CASES)
def test_diagnostics_within_the_perturbed_reference(shape, seed):
    from gpemu import diagnostics as D
    c = R.case(shape, seed)
    dev, same, _ = R.perturbed(c, Z_CAP)
    assert same
    with D.Diag(c["x"]) as h:
        got = h.summary()
    assert got["n_chains"] == c["K"] and got["n_draws"] == c["N"]
    ratios = {}
    for k in D.KEYS:
        err = np.abs(got[k] - c["diag"][k])
        assert np.all(err <= 4.0 * dev[k]), (k, err, dev[k])
        ratios[k] = float(np.max(err / np.where(dev[k] > 0, dev[k], 1.0)))
    print(f"\n{shape} seed {seed}: deviation / perturbed deviation " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def test_constant_and_nan_parameters_and_the_single_functions():
    from gpemu import diagnostics as D
    x = R.metropolis(40, 3, 3, seed=1)
    x[:, :, 1] = 2.5
    x[7, 1, 2] = np.nan
    got, ref = D.summary(x), R.diagnostics(x)
    for k in D.KEYS:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
        assert np.allclose(got[k][0], ref[k][0], rtol=1e-10) and (np.isnan(ref[k][1]) or got[k][1] == ref[k][1]), k
    y = R.metropolis(64, 5, 3, seed=3)
    s = D.summary(y)
    for name in D.KEYS:
        assert _same_bits(getattr(D, name)(y), s[name]), name


# ---- 4. sampler paths -------------------------------------------------------------------------------------------------
def test_sampler_diagnostics_equal_the_summary_of_the_downloaded_chain():
    from gpemu import _lib
    from gpemu import diagnostics as D
    from gpemu.sampler import DeviceSampler, HMCSampler, TemperedSampler
    from test_gpu_hmc import case_model
    dm, lo, hi, rng = case_model("n16_d7_m15_const")
    W = 24
    s = DeviceSampler([dm], W, seed=11)
    s.set_state(rng.uniform(lo, hi, (W, lo.size)))
    s.run(120)
    chain, _ = s.get_chain()
    for discard, thin in ((0, 1), (20, 3)):
        got, want = s.diagnostics(discard=discard, thin=thin), D.summary(np.ascontiguousarray(chain[discard::thin]))
        for k in D.KEYS:
            assert _same_bits(got[k], want[k]), (k, discard, thin)
        assert got["n_chains"] == 2 * W and got["n_draws"] == len(chain[discard::thin]) // 2
    # a borrowed chain is stale after a run
    h = D.Diag.from_sampler(s._h, 0, 120, 1, 0, W, s.d)
    h.transform(D.IDENTITY)
    s.run(1)
    c0 = _counts()
    for call in (lambda: h.transform(D.IDENTITY), lambda: h.acov(0, 16), h.pooled, h.value_range):
        with pytest.raises(_lib.GpemuError) as err:
            call()
        assert err.value.code == -4
    h.close()
    # argument errors come before any launch
    for bad in (lambda: D.Diag.from_sampler(s._h, 0, 7, 1, 0, W, s.d), lambda: D.Diag.from_sampler(s._h, 0, 122, 1, 0, W, s.d),
                lambda: D.Diag.from_sampler(s._h, 0, 61, 2, 0, W + 1, s.d), lambda: D.Diag(np.zeros((7, 3, 2)))):
        with pytest.raises(_lib.GpemuError) as err:
            bad()
        assert err.value.code == -1
    with D.Diag(chain[:40]) as h2:
        for bad in (lambda: h2.transform(7), lambda: h2.transform(D.INDICATOR_LE, 1.5)):
            with pytest.raises(_lib.GpemuError) as err:
                bad()
            assert err.value.code == -1
        with pytest.raises(_lib.GpemuError) as err:
            h2.acov(0, 16)                      # nothing transformed yet
        assert err.value.code == -4
        assert _counts() == c0
        h2.transform(D.IDENTITY)
        for l0, nl in ((8, 8), (0, 21), (16, 4), (0, 0)):      # not a multiple of 16; beyond N = 20; not started at 0
            with pytest.raises(_lib.GpemuError) as err:
                h2.acov(l0, nl)
            assert err.value.code == -1
    s.close()

    ts = TemperedSampler([dm], W, [1.0, 0.5, 0.1], seed=5, swap_every=2)
    ts.set_state(rng.uniform(lo, hi, (3 * W, lo.size)))
    ts.run(60)
    for temp in (0, 2):
        got, want = ts.diagnostics(temp=temp, discard=4), D.summary(ts.get_chain(temp=temp, discard=4)[0])
        for k in D.KEYS:
            assert _same_bits(got[k], want[k]), (k, temp)
    ts.close()

    hs = HMCSampler([dm], 24, n_leapfrog=3, step_size=0.3, seed=8)
    hs.set_state(rng.uniform(lo, hi, (24, lo.size)))
    hs.run(80)
    got, want = hs.diagnostics(discard=10), D.summary(hs.get_chain(first=10)[0])
    for k in D.KEYS:
        assert _same_bits(got[k], want[k]) and np.all(np.isfinite(got[k])), k
    assert got["n_chains"] == 48
    hs.close()

    dm.close()


def test_stacked_chains_take_a_chain_index():
    from gpemu import diagnostics as D
    from gpemu.sampler import DeviceSampler
    import golden_util as GU
    import path_cases as PC
    c = [x for x in PC.cases() if x.name == "n16_d7_m15_const"][0]
    model, lo, hi, y_exp, y_err, bs, rng = PC.problem(c)
    dm = GU.device_model(model)
    dm.likelihood_setup(np.stack([y_exp, y_exp * 1.01]), y_err, lo, hi, 1.0, block_start=bs)
    W = 16
    s = DeviceSampler([dm], W, seeds=[3, 4])
    s.set_state(rng.uniform(lo, hi, (2 * W, lo.size)))
    s.run(40)
    chain, _ = s.get_chain()
    with pytest.raises(ValueError):
        s.diagnostics()
    for ci in (0, 1):
        got, want = s.diagnostics(chain=ci), D.summary(np.ascontiguousarray(chain[:, ci * W:(ci + 1) * W]))
        for k in D.KEYS:
            assert _same_bits(got[k], want[k]), (k, ci)
    s.close()
    dm.close()


# ---- 5. the drop-in route ---------------------------------------------------------------------------------------------
def test_dropin_diagnostics_key(tmp_path, monkeypatch):
    from bayesian_inference import mcmc
    from gpemu import diagnostics as D
    from test_gpu_hmc import USUAL, _g1_analysis
    path, analysis, h5io = _g1_analysis(tmp_path, monkeypatch)
    mc = analysis["parameters"]["mcmc"]
    mc.update(n_burn_steps=20, n_sampling_steps=40)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.diagnostics is False
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    plain = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(plain) == USUAL, set(plain)
    mc.update(diagnostics=True)
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.diagnostics is True
    np.random.seed(3)
    mcmc.run_mcmc(cfg)
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(back) == USUAL | set(mcmc.DIAGNOSTICS_KEYS), set(back)
    d = back["chain"].shape[2]
    assert np.array_equal(back["chain"], plain["chain"])
    for k in mcmc.DIAGNOSTICS_KEYS:
        assert back[k].shape == (d,) and np.all(np.isfinite(back[k])), k
    again = mcmc.diagnostics(cfg)
    want = D.summary(back["chain"])
    for k in mcmc.DIAGNOSTICS_KEYS:
        assert _same_bits(back[k], want[k]) and _same_bits(again[k], want[k]), k
    thinned = mcmc.diagnostics(cfg, discard=4, thin=2)
    assert thinned["n_draws"] == 9 and thinned["rhat"].shape == (d,)
