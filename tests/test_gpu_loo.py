"""-m gpu tests of the per-observable log-likelihood terms, PSIS-LOO, WAIC and the weighted parameter moments
(gpemu_loglik_pointwise*, gpemu_psis*, gpemu_weighted_moments_dev, gpemu.loo, DeviceSampler.loo) against
tests/loo_ref.py: hp_ref's extended-precision terms block by block, and the specification of the smoothing step by step
in longdouble, each with its a-priori bound.

Figures measured on an MI355X are printed by every test before it asserts (run with -s)."""
import functools

import numpy as np
import pytest

import hp_ref as H
import loo_ref as R
import pp_ref as P
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SPECS = {
    "rbf": O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=False, has_noise=True),
    "matern25": O.KernelSpec(kind=O.MATERN, nu=2.5, has_const=False, has_noise=True),
    "matern_nu": O.KernelSpec(kind=O.MATERN, nu=1.2, has_const=False, has_noise=True),
    "const_white": O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=True, has_noise=True),
}
BLOCKS = {
    "one": [1],
    "two": [2, 21],
    "three": [1, 2, 21],
    "ten": [1, 2, 21, 3, 3, 3, 3, 3, 3, 24],
}
# every KMAX instance of the likelihood (4, 8, ..., 32), both sides of the register / LDS split (32 | 33), every kernel
# kind, the 8- and 16-wide instances; B = 2049 crosses the 2048-row predict chunk
CASES = {
    "k1": dict(kind="rbf", d=1, N=17, k=1, blocks="one", B=63),
    "k4": dict(kind="matern25", d=8, N=17, k=4, blocks="two", B=2049),
    "k5": dict(kind="matern_nu", d=9, N=17, k=5, blocks="three", B=65),
    "k12": dict(kind="const_white", d=16, N=17, k=12, blocks="three", B=63),
    "k16": dict(kind="rbf", d=8, N=17, k=16, blocks="three", B=65),
    "k17": dict(kind="matern25", d=9, N=64, k=17, blocks="ten", B=63),
    "k32": dict(kind="rbf", d=16, N=64, k=32, blocks="ten", B=65),
    "k33": dict(kind="matern_nu", d=1, N=64, k=33, blocks="ten", B=65),
    "k64": dict(kind="const_white", d=8, N=64, k=64, blocks="ten", B=1),
    "cov": dict(kind="rbf", d=8, N=17, k=4, blocks="three", B=65, cov=True),
}


def _data(model, seed):
    rng = np.random.default_rng(1000 + seed)
    F = model.scaler_mean.size
    y_exp = model.scaler_mean + 0.3 * model.scaler_scale * rng.normal(size=F)
    y_err = (0.05 + 0.05 * rng.uniform(size=F)) * np.abs(model.scaler_scale)
    return y_exp, y_err


def _within_cov(y_err, bs):
    """exponential correlation between neighbouring bins inside each observable, zero across observables"""
    F = y_err.size
    i = np.arange(F)
    obs = np.searchsorted(bs, i, side="right")
    cov = np.outer(y_err, y_err) * np.exp(-np.abs(i[:, None] - i[None, :]) / 3.0)
    return np.where(obs[:, None] == obs[None, :], cov, 0.0)


@functools.lru_cache(maxsize=None)
def _case(name):
    import golden_util as GU
    c = CASES[name]
    sizes = BLOCKS[c["blocks"]]
    bs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    seed = sorted(CASES).index(name)
    model, lo, hi = P.problem(c["N"], c["d"], int(bs[-1]), c["k"], SPECS[c["kind"]], seed=seed)
    y_exp, y_err = _data(model, seed)
    cov = _within_cov(y_err, bs) if c.get("cov") else None
    dm = GU.device_model(model)
    dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0, block_start=bs, cov=cov)
    X = np.random.default_rng(50 + seed).uniform(lo, hi, (c["B"], c["d"]))
    return dict(model=model, dm=dm, lo=lo, hi=hi, bs=bs, y_exp=y_exp, y_err=y_err, cov=cov, X=X)


# ---- 1. the terms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_terms_against_the_extended_precision_reference(name):
    c = _case(name)
    dm, X, model = c["dm"], c["X"], c["model"]
    T = dm.loglik_pointwise(X)
    assert T.shape == (len(c["bs"]) - 1, X.shape[0]) == (dm.n_observable_blocks, X.shape[0])
    with P.oracle_for(model.spec):
        pred = H.gp_predict(X, model)
    Tref, bound = R.terms(model, X, c["y_exp"], c["y_err"], c["bs"], cov=c["cov"], pred=pred)
    err = np.abs(np.asarray(T - Tref, dtype=np.float64))
    print(f"{name}: terms max err {err.max():.3e}, max err / bound {np.max(err / bound):.3e}")
    assert np.all(err <= bound)
    # the sum of the terms, added in block order from 0.0, against the log-posterior of rows inside the box
    lp = dm.logpost(X)
    total = np.zeros(X.shape[0])
    for o in range(T.shape[0]):
        total = total + T[o]
    setups = R.setup_blocks(model, c["y_exp"], c["y_err"], c["bs"], cov=c["cov"])
    full = H.loglik_bound(pred[0], pred[1], pred[2], pred[3], setups)
    tol = bound.sum(axis=0) + full + T.shape[0] * U * np.abs(T).sum(axis=0)
    d = np.abs(total - lp)
    print(f"{name}: sum of terms vs logpost: max diff {d.max():.3e}, max diff / tol {np.max(d / tol):.3e}, "
          f"bit for bit: {bool(np.array_equal(total, lp))} ({int(np.sum(total == lp))} of {lp.size} rows)")
    assert np.all(np.isfinite(lp)) and np.all(d <= tol)
    # normalised: -(F_o / 2) log 2 pi per block
    Tn = dm.loglik_pointwise(X, normalised=True)
    assert np.array_equal(Tn, T - 0.5 * np.log(2 * np.pi) * np.diff(c["bs"])[:, None])


def test_a_term_is_a_likelihood_and_a_non_finite_row_gives_nan():
    c = _case("k16")
    dm, X = c["dm"], c["X"][:9].copy()
    ref = dm.loglik_pointwise(X)
    X2 = X.copy()
    X2[3] = c["hi"] + 0.25          # outside the box: the term is evaluated all the same
    X2[5, 2] = np.nan
    T = dm.loglik_pointwise(X2)
    keep = [0, 1, 2, 4, 6, 7, 8]
    assert T[:, keep].tobytes() == ref[:, keep].tobytes()
    assert np.all(np.isfinite(T[:, 3])) and np.all(np.isnan(T[:, 5]))
    assert dm.logpost(X2)[3] == -np.inf


# ---- 2. the view forms ----------------------------------------------------------------------------------------------------
def _device_terms(dm, view, d, S, chain=0):
    import torch
    src, n_blocks, nw, stride = view
    T = torch.empty((dm.n_observable_blocks, S), dtype=torch.float64, device=torch.device("cuda", dm.device))
    dm.loglik_pointwise_dev(src, n_blocks, nw, stride, T.data_ptr(), S, chain=chain)
    return T.cpu().numpy()


def test_view_forms_equal_the_host_form_bit_for_bit():
    from gpemu import loo
    from gpemu.sampler import DeviceSampler
    c = _case("k16")
    dm, d, W = c["dm"], c["X"].shape[1], 16
    s = DeviceSampler([dm], W, seed=3)
    s.set_state(np.random.default_rng(4).uniform(c["lo"], c["hi"], (W, d)))
    s.run(140)                                  # 2240 rows: more than one predict chunk
    chain, _ = s.get_chain()
    for thin in (1, 3):
        view = s._stored_view(0, thin, None)
        S = view.rows
        got = _device_terms(dm, view.layout, d, S)
        want = dm.loglik_pointwise(chain[::thin].reshape(-1, d))
        print(f"in place, thin {thin}: {S} rows, equal bits: {got.tobytes() == want.tobytes()}")
        assert got.tobytes() == want.tobytes()
    s.close()
    # one chain of a stacked sampler, scored against its own data vector
    rng = np.random.default_rng(6)
    y2 = np.stack([c["y_exp"], c["y_exp"] + 0.1 * c["y_err"] * rng.normal(size=c["y_exp"].size)])
    dm.likelihood_setup(y2, c["y_err"], c["lo"], c["hi"], 1.0, block_start=c["bs"])
    try:
        st = DeviceSampler([dm], W, seeds=[7, 8])
        st.set_state(np.random.default_rng(5).uniform(c["lo"], c["hi"], (2 * W, d)))
        st.run(20)
        chain, _ = st.get_chain()
        view = st._stored_view(0, 1, 1)
        S = view.rows
        got = _device_terms(dm, view.layout, d, S, chain=1)
        rows = chain[:, W:].reshape(-1, d)
        assert got.tobytes() == dm.loglik_pointwise(rows, chain=1).tobytes()
        assert got.tobytes() != dm.loglik_pointwise(rows, chain=0).tobytes()
        out = st.loo(chain=1, shifts=False)
        assert out["n_samples"] == S and np.array_equal(out["elpd_loo"], loo.psis(got)["elpd_loo"])
        st.close()
    finally:
        dm.likelihood_setup(c["y_exp"], c["y_err"], c["lo"], c["hi"], 1.0, block_start=c["bs"])


def test_declined_calls_launch_nothing():
    import golden_util as GU
    from gpemu import _lib, loo
    c = _case("k4")
    fresh = GU.device_model(c["model"])
    before = loo.path_counts()
    with pytest.raises(_lib.GpemuError) as e:
        fresh.loglik_pointwise(c["X"][:5])
    assert e.value.code == -4
    src = np.zeros((1, c["y_exp"].size))
    src[0, :3] = 0.01
    fresh.likelihood_setup(c["y_exp"], c["y_err"], c["lo"], c["hi"], 1.0, block_start=c["bs"], sys_sources=src)
    assert fresh.n_observable_blocks == 2
    with pytest.raises(_lib.GpemuError) as e:
        fresh.loglik_pointwise(c["X"][:5])
    assert e.value.code == -5 and "sources" in str(e.value)
    assert loo.path_counts() == before
    fresh.close()


# ---- 3. PSIS / WAIC --------------------------------------------------------------------------------------------------------
S_ALL = (1, 5, 20, 21, 25, 63, 64, 65, 2049, 4097, 100003)
STATS = ("pareto_k", "elpd_loo", "lppd", "p_loo", "p_waic", "elpd_waic", "ess_w")


@functools.lru_cache(maxsize=None)
def _device_term_rows():
    """(a): the device's own terms of a three-observable model for 100 003 rows"""
    c = _case("k5")
    X = np.random.default_rng(77).uniform(c["lo"], c["hi"], (max(S_ALL), c["X"].shape[1]))
    return c["dm"].loglik_pointwise(X)


def _matrix(S, R16=True):
    """the rows of one size: (a) device terms, (b) -c z^2, (c) Metropolis-like repeats, (d) constant, (e) one NaN,
    (f) ratios spanning more than 700 in the log; padded with more of (b) to 16 rows"""
    rows = [_device_term_rows()[:, :S]]
    rows += [R.synthetic_rows(1, S, cc, seed=S + i) for i, cc in enumerate((0.05, 0.5, 1.5))]
    rows += [R.metropolis_rows(1, S, seed=S + 10, repeat=4), R.metropolis_rows(1, S, seed=S + 11, repeat=7, c=1.5)]
    rows += [np.full((1, S), -2.75)]
    bad = R.synthetic_rows(1, S, 0.5, seed=S + 20)
    bad[0, S // 2] = np.nan
    rows += [bad, R.wide_rows(1, S, seed=S + 30)]
    V = np.concatenate(rows)
    if R16:
        V = np.concatenate([V, R.synthetic_rows(16 - V.shape[0], S, 0.8, seed=S + 40)])
    return np.ascontiguousarray(V)


def _one_shift_reproduces(xr, lwr):
    """is there one float64 L with lwr == xr - L, bit for bit?  L is x_j - logw_j up to the rounding of logw_j (an ulp of
    |x_j| + |L|, read off the element nearest 0): the candidates within that distance are tried, first on a few elements"""
    j = int(np.argmax(xr))
    L0 = xr[j] - lwr[j]
    step = np.spacing(abs(L0)) if L0 != 0 else 0.0
    span = int(min(4096, 4 + 4 * np.spacing(abs(xr[j]) + abs(L0)) / max(step, 5e-324)))
    Ls = L0 + np.arange(-span, span + 1) * step
    few = np.unique(np.linspace(0, xr.size - 1, min(xr.size, 64)).astype(int))
    ok = Ls[np.all(xr[few][None, :] - Ls[:, None] == lwr[few][None, :], axis=1)]
    return any(np.array_equal(xr - L, lwr) for L in ok)


def _check_rows(V, out, label, r_eff=None):
    ref = R.psis(V, r_eff)
    worst = {k: 0.0 for k in STATS + ("logw",)}
    for r, rr in enumerate(ref):
        if rr["n_tail"] < 0:                    # (e): NaN everywhere
            assert out["n_tail"][r] == -1 and all(np.isnan(out[k][r]) for k in STATS + ("cutoff",))
            assert np.isnan(out["log_weights"][r]).all()
            continue
        assert out["n_tail"][r] == rr["n_tail"], (label, r)
        assert out["cutoff"][r] == float(rr["cutoff"]), (label, r)
        lw_err = np.abs(np.asarray(out["log_weights"][r] - rr["logw"], dtype=np.float64))
        assert all(np.all(np.isfinite(b)) for b in rr["bound"].values()), (label, r)     # no bound is vacuous
        # the weights outside the tail stay raw, as bits: logw = x - L in float64 for one L, the log-sum-exp
        x = (-V[r]) - np.max(-V[r])
        raw = x <= float(rr["cutoff"]) if rr["n_tail"] > 4 else np.ones(x.size, dtype=bool)
        if raw.any():
            assert _one_shift_reproduces(x[raw], out["log_weights"][r][raw]), (label, r)
        if rr["n_tail"] <= 4:
            assert out["pareto_k"][r] == np.inf, (label, r)
        for k in STATS:
            want, b = float(rr[k]), rr["bound"][k]
            if k == "pareto_k" and rr["n_tail"] <= 4:
                continue
            if np.isnan(want):                  # p_waic of a single sample
                assert np.isnan(out[k][r]), (label, r, k)
                continue
            e = abs(out[k][r] - want)
            assert e <= b, (label, r, k, e, b)
            if np.isfinite(b) and b > 0:
                worst[k] = max(worst[k], e / b)
        b = rr["bound"]["logw"]
        assert np.all(lw_err <= b), (label, r, "logw", float(lw_err.max()))
        fin = np.isfinite(b) & (b > 0)
        if fin.any():
            worst["logw"] = max(worst["logw"], float(np.max(lw_err[fin] / b[fin])))
    print(f"{label}: largest error / bound: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


@pytest.mark.parametrize("S", [s for s in S_ALL if s <= 4097])
def test_psis_of_sixteen_rows_against_the_reference(S):
    from gpemu import loo
    V = _matrix(S)
    assert V.shape == (16, S)
    before = loo.path_counts()
    out = loo.psis(V, return_weights=True)
    after = loo.path_counts()
    assert after["SORT_PASS"] - before["SORT_PASS"] == 8 and after["ROW_BATCH"] - before["ROW_BATCH"] == 1
    assert (after["ROW_SMOOTHED"] - before["ROW_SMOOTHED"]) + (after["ROW_RAW"] - before["ROW_RAW"]) == 16
    assert after["ROW_SMOOTHED"] - before["ROW_SMOOTHED"] == int(np.sum(out["n_tail"] > 4))
    _check_rows(V, out, f"S={S} R=16")
    # one row on its own: the same bits as in the batch; r_eff changes the tail
    one = loo.psis(V[2], return_weights=True)
    for k in STATS + ("cutoff", "n_tail"):
        assert one[k][0].tobytes() == out[k][2].tobytes(), k
    assert one["log_weights"].tobytes() == out["log_weights"][2].tobytes()
    re = np.linspace(0.3, 1.7, 16)
    _check_rows(V, loo.psis(V, r_eff=re, return_weights=True), f"S={S} R=16 r_eff", re)
    # several batches of rows through a small workspace: the same bits
    per_row = 16 * S + 1024 * ((S + 2047) // 2048) + 4 + 16 * max(loo.tail_size(S), 1) + 40 * ((S + 4095) // 4096) + 136 + 8192
    before = loo.path_counts()
    small = loo.psis(V, return_weights=True, workspace_bytes=int(2.5 * per_row))
    after = loo.path_counts()
    print(f"S={S}: {after['ROW_BATCH'] - before['ROW_BATCH']} batches of rows in {int(2.5 * per_row)} bytes")
    assert after["ROW_BATCH"] - before["ROW_BATCH"] == 8 and after["SORT_PASS"] - before["SORT_PASS"] == 64
    for k in STATS + ("cutoff", "n_tail", "log_weights"):
        assert np.asarray(small[k]).tobytes() == np.asarray(out[k]).tobytes(), k
    from gpemu import _lib
    with pytest.raises(_lib.GpemuError) as e:
        loo.psis(V, workspace_bytes=16 * S)
    assert e.value.code == -2 and "out of memory" in str(e.value)


def test_psis_of_one_and_three_long_rows_on_the_device():
    import torch
    from gpemu import loo
    S = 100003
    V = np.ascontiguousarray(np.concatenate([_device_term_rows()[:1, :S], R.synthetic_rows(1, S, 0.5, seed=1),
                                             R.metropolis_rows(1, S, seed=2, repeat=4)]))
    dV = torch.from_numpy(V).cuda()
    out = loo.psis(dV, return_weights=True)
    out["log_weights"] = out["log_weights"].cpu().numpy()
    assert list(out["n_tail"][:2]) == [949, 949]
    _check_rows(V, out, f"S={S} R=3 (device tensor)")
    one = loo.psis(V[1], return_weights=True)
    _check_rows(V[1:2], one, f"S={S} R=1")
    assert one["elpd_loo"][0].tobytes() == out["elpd_loo"][1].tobytes()
    w = loo.waic(V)
    assert np.array_equal(w["elpd_waic"], out["elpd_waic"]) and np.array_equal(w["p_waic"], out["p_waic"])


def test_an_infinite_value_makes_the_row_nan():
    from gpemu import loo
    V = R.synthetic_rows(3, 50, 0.5, seed=4)
    V[0, 7], V[2, 11] = -np.inf, np.inf
    out = loo.psis(V, return_weights=True)
    ref = R.psis(V)
    assert ref[0]["n_tail"] == ref[2]["n_tail"] == -1 and out["n_tail"].tolist() == [-1, ref[1]["n_tail"], -1]
    for r in (0, 2):
        assert all(np.isnan(out[k][r]) for k in STATS + ("cutoff",)) and np.isnan(out["log_weights"][r]).all()
    _check_rows(V, out, "S=50 with infinite values")


def test_summary_and_leave_out_on_the_device():
    from gpemu import loo
    T = _device_term_rows()[:, :4097]
    s = loo.summary(T, labels=["a", "b", "c"])
    p = loo.psis(T)
    assert np.array_equal(s["elpd_loo"], p["elpd_loo"]) and s["elpd_loo_total"] == float(np.sum(p["elpd_loo"]))
    assert np.all(s["elpd_loo"] <= s["lppd"])
    g = loo.summary(T, labels=["a", "b", "c"], leave_out=[[2, 0], [1]])
    assert g["labels"] == ["c+a", "b"] and g["n_obs"] == 2
    want = loo.psis(np.stack([T[2] + T[0], T[1]]))
    assert np.array_equal(g["elpd_loo"], want["elpd_loo"]) and np.array_equal(g["pareto_k"], want["pareto_k"])
    assert np.array_equal(g["elpd_loo"][1:], s["elpd_loo"][1:2])
    c = loo.compare(s, s)
    assert c["elpd_diff"] == 0.0 and c["se_diff"] == 0.0


# ---- 4. weighted moments ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 8, 16])
def test_weighted_moments_on_a_thinned_view(d):
    import torch
    from gpemu import loo
    for S, nw in ((1, 1), (65, 5), (4097, 17)):
        rng = np.random.default_rng(100 * d + S)
        n_blocks, thin = S // nw, 3
        store = rng.normal(size=(n_blocks * thin, nw + 2, d)) * (1.0 + np.arange(d)) + np.arange(d)
        X = np.ascontiguousarray(store[::thin, :nw].reshape(-1, d))
        lw = rng.normal(size=(3, S)) * np.array([[0.1], [1.0], [4.0]])
        lw -= np.log(np.sum(np.exp(lw), axis=1, keepdims=True))
        ds, dlw = torch.from_numpy(store).cuda(), torch.from_numpy(lw).cuda()
        mean, var = loo.weighted_moments_dev(0, ds.data_ptr(), n_blocks, nw, thin * (nw + 2), d, dlw)
        rm, rv, bm, bv = R.weighted_moments(X, lw)
        em = np.abs(np.asarray(mean - rm, dtype=np.float64))
        ev = np.abs(np.asarray(var - rv, dtype=np.float64))
        print(f"d={d} S={S}: mean max err / bound {np.max(em / bm):.3e}, var max err / bound "
              f"{np.max(np.where(bv > 0, ev / np.where(bv > 0, bv, 1.0), 0.0)):.3e}")
        assert np.all(em <= bm) and np.all(ev <= bv)
        dX = torch.from_numpy(X).cuda()
        dense = loo.weighted_moments_dev(0, dX.data_ptr(), 1, S, S, d, dlw)
        assert dense[0].tobytes() == mean.tobytes() and dense[1].tobytes() == var.tobytes()


def test_sampler_loo_equals_the_summary_of_the_downloaded_chain():
    from gpemu import loo
    from gpemu.sampler import DeviceSampler
    c = _case("k16")
    dm, d, W = c["dm"], c["X"].shape[1], 16
    s = DeviceSampler([dm], W, seed=11)
    s.set_state(np.random.default_rng(12).uniform(c["lo"], c["hi"], (W, d)))
    s.run(300)
    for discard, thin in ((40, 1), (41, 3)):
        got = s.loo(discard=discard, thin=thin)
        rows = s.get_chain()[0][discard::thin].reshape(-1, d)
        want = loo.chain_loo([dm], rows)
        table = loo.summary(dm.loglik_pointwise(rows), labels=got["labels"])
        for k in loo.SUMMARY_KEYS + ("loo_mean", "loo_sd"):
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
        for k in loo.SUMMARY_KEYS:
            assert np.asarray(got[k]).tobytes() == np.asarray(table[k]).tobytes(), k
        assert got["se"] == table["se"] and got["labels"] == ["g0o0", "g0o1", "g0o2"]
        assert np.allclose(got["mean"], rows.mean(axis=0), rtol=0, atol=1e-13 * np.abs(rows).max())
        assert np.allclose(got["sd"], rows.std(axis=0), rtol=1e-12)
        assert np.array_equal(got["shift"], (got["loo_mean"] - got["mean"][None]) / got["sd"][None])
        print(f"discard {discard}, thin {thin}: {rows.shape[0]} rows, pareto_k {got['pareto_k']}, largest |shift| "
              f"{np.abs(got['shift']).max():.3f}")
    g = s.loo(discard=40, leave_out=[[0, 2], [1]], shifts=False)
    assert g["labels"] == ["g0o0+g0o2", "g0o1"] and "shift" not in g
    s.close()


# ---- 5. planted influence -----------------------------------------------------------------------------------------------------
PLANTED_SEED = 3


def planted(seed):
    """Three one-observable groups over (theta_0, theta_1): only the first depends on theta_0.  Returns the models, the
    data and a posterior sample of 1500 rows drawn on the host (sampling-importance-resampling of 30 000 uniform draws
    under the float64 oracle: repeated rows, as a chain has)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-1.0, -1.0]), np.array([1.0, 1.0])
    N, F = 24, 4
    Xd = rng.uniform(lo, hi, (N, 2))
    spec = SPECS["rbf"]
    truth = np.array([0.35, -0.2])
    models, datas = [], []
    for g in range(3):
        a = rng.normal(size=(2, F))
        if g > 0:
            a[0] = 0.0
        f = lambda x: np.sin(x @ a) + 0.3 * (x ** 2) @ np.abs(a)
        Y = f(Xd) + 0.002 * rng.normal(size=(N, F))
        mean, scale, _ = O.scaler_fit(Y)
        pca = O.pca_fit((Y - mean) / scale)
        theta = np.log(np.r_[1.2, 1.2, 0.001])
        gps = [O.gp_fit_at_theta(Xd, pca["Y_pca"][:, i], theta, spec, 1e-10) for i in range(2)]
        models.append(O.GroupModel(X_train=Xd, spec=spec, gps=gps, components=pca["components"],
                                   explained_variance=pca["explained_variance"], scaler_mean=mean, scaler_scale=scale,
                                   n_pc=2))
        y_err = np.full(F, 0.15)
        datas.append((f(truth[None])[0] + y_err * rng.normal(size=F), y_err))
    pool = rng.uniform(lo, hi, (30000, 2))
    lp = np.zeros(pool.shape[0])
    for m, (y, e) in zip(models, datas):
        mean, var, _, _, _ = H.gp_predict(pool, m)
        st = H.lowrank_setup_blocks(m, y, e, [0, F])
        lp += np.asarray(H.loglik_blocks(mean, var, st)[0], dtype=np.float64)
    w = np.exp(lp - lp.max())
    X = pool[rng.choice(pool.shape[0], 1500, p=w / w.sum())]
    return models, datas, lo, hi, X


def planted_reference(seed):
    """the reference's shift table, elpd_loo and lppd with their bounds, from the reference's own terms"""
    models, datas, lo, hi, X = planted(seed)
    T = np.concatenate([R.terms(m, X, y, e, [0, y.size])[0] for m, (y, e) in zip(models, datas)])
    rows = R.psis(np.asarray(T, dtype=np.float64))
    lw = np.stack([np.asarray(r["logw"], dtype=np.float64) for r in rows])
    mean, var, dm, dv = R.weighted_moments(X, lw)
    m0, v0, dm0, dv0 = R.weighted_moments(X, np.zeros((1, X.shape[0])))
    shift = np.asarray((mean - m0) / np.sqrt(v0), dtype=np.float64)
    sd0 = np.sqrt(np.asarray(v0, dtype=np.float64))
    dshift = (dm + dm0) / sd0 + np.abs(shift) * dv0 / (2 * np.asarray(v0, dtype=np.float64))
    return rows, shift, dshift


def test_planted_influence():
    """Observable 0 alone depends on parameter 0: leaving it out moves parameter 0 the most.  The seed was chosen on the
    host with tests/loo_ref.py (planted_reference): there |shift[0][0]| exceeds the other entries of column 0, and
    lppd - elpd_loo is positive, by more than ten times the reference's bounds."""
    import golden_util as GU
    from gpemu import loo
    models, datas, lo, hi, X = planted(PLANTED_SEED)
    dms = []
    for m, (y, e) in zip(models, datas):
        dm = GU.device_model(m)
        dm.likelihood_setup(y, e, lo, hi, 1.0)
        dms.append(dm)
    out = loo.chain_loo(dms, X)
    col = np.abs(out["shift"][:, 0])
    print(f"planted: |shift[:, 0]| {col}, elpd_loo {out['elpd_loo']}, lppd {out['lppd']}, pareto_k {out['pareto_k']}")
    assert out["shift"].shape == (3, 2) and np.argmax(col) == 0 and col[0] > col[1] and col[0] > col[2]
    assert np.all(out["elpd_loo"] <= out["lppd"])
    for dm in dms:
        dm.close()
