"""The reference of the device autocorrelation estimate and of the pooled moments (tests/acf_ref.py), held to account on
the CPU: it agrees with the host FFT estimator and with the analytic AR(1) function; the float64 emulation of the
device's order lies inside the a-priori bound for every case; the bound is not vacuous (seven planted mistakes each
leave it by 100x on a named case); no window decision of a case lies near its bound; and the cases satisfy the input
conditions the bound needs."""
from __future__ import annotations

import math

import numpy as np
import pytest

import acf_ref as A
from gpemu import sampler as S

BENIGN = [r for r in A.ROWS if r.kind == "ar1"]


def _f(row):
    return A.ref(row).f(row.n_lags)


# ---- 1. the reference against the host estimator and the analytic function ---------------------------------------------
@pytest.mark.parametrize("row", BENIGN, ids=lambda r: r.name)
def test_reference_equals_the_host_fft_estimator(row):
    R = A.ref(row)
    _, x = A.data(row)
    _, tau, _, _, _ = R.tau()
    with np.errstate(invalid="ignore", divide="ignore"):
        host = S.integrated_time(x, quiet=True)
    np.testing.assert_allclose(tau, host, rtol=1e-10, atol=0, equal_nan=True)
    if row.n_t > 1:
        f, _ = _f(row)
        L = min(f.shape[0], 48)
        fft = np.stack([np.mean([S.function_1d(x[:, w, dd])[:L] for w in range(row.nw)], axis=0)
                        for dd in range(row.d)], axis=1)
        np.testing.assert_allclose(f[:L], fft, rtol=0, atol=1e-10)


def test_reference_follows_the_analytic_ar1_function():
    """f[l] = phi^l for a long AR(1) chain, within the statistical error of the estimate: Bartlett's variance of r[l]
    is about (1 + phi^2) / ((1 - phi^2) N) per series, so 5 standard errors of the mean over nw walkers (the bias, of
    order 1 / N, lies far inside)."""
    n_t, nw, L = 20000, 64, 12
    for phi in (0.5, 0.95):
        x = A.ar1(n_t, nw, 1, phi, np.random.default_rng(77))
        f, _ = A.Ref(x).f(L)
        tol = 5.0 * math.sqrt((1.0 + phi * phi) / (1.0 - phi * phi) / n_t / nw) + 4.0 * (1.0 + phi) / (1.0 - phi) / n_t
        err = np.abs(f[:, 0] - phi ** np.arange(L))
        print(f"\nAR(1) phi = {phi}: max |f - phi^l| = {err.max():.2e}, tolerance {tol:.2e}")
        assert np.all(err <= tol)


# ---- 2. the emulation inside the bound ----------------------------------------------------------------------------------
def test_emulation_lies_inside_the_bound_for_every_case():
    worst = {}
    for row in A.ROWS:
        f, df = _f(row)
        lags, got = A.emulate_row(row)
        q, same_nan = A.err_over_bound(got, f[lags], df[lags])
        assert same_nan, f"{row.name}: NaN pattern differs from the reference"
        worst[row.kind] = max(worst.get(row.kind, 0.0), q)
        assert q <= 1.0, f"{row.name}: emulation leaves the bound, err / bound = {q:.3g}"
    print("\nworst err / bound of the float64 emulation per data kind:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_plain_kernels_leave_a_stuck_walker_finite_and_the_constant_mean_makes_it_nan():
    """What the emulation says of a constant series: without acf_constant_mean_kernel the stuck walker's series is a
    rounding residue and its parameter a finite number; with it the parameter is NaN at every lag."""
    for name in ("n127_stuck_walker", "n130_stuck_walker_nw300"):
        row = A.ROW[name]
        assert A.constant_residue(A.stuck_value(row.n_t), row.n_t) != 0.0
        lags = np.arange(min(row.n_t, 20))
        _, plain = A.emulate_row(row, constant_fix=False, lags=lags)
        _, fixed = A.emulate_row(row, lags=lags)
        for dd in A.stuck_parameters(row):
            assert np.all(np.isfinite(plain[:, dd])), "the residue was expected to give a finite ratio"
            assert np.all(np.isnan(fixed[:, dd]))
        other = [dd for dd in range(row.d) if dd not in A.stuck_parameters(row)]
        assert np.array_equal(plain[:, other], fixed[:, other])
    assert all(A.constant_residue(c, 17) == 0.0 for c in A.STUCK_CANDIDATES)      # n = 2^4 + 1 (acf_ref.STUCK_CANDIDATES)


# ---- 3. the bound is not vacuous -----------------------------------------------------------------------------------------
# the case each planted mistake is caught on (any row may catch it; this one must)
CAUGHT_ON = {
    "drop_last_step": "n130_nw300",
    "shift_lags": "n129_s528_blocks",
    "no_zero_padding": "n16_s259",
    "ld_of_block": "n130_w5_first3_blocks",
    "divide_by_nw_plus_1": "n15_one_series",
    "skip_walkers_256": "n128_nw257",
    "other_series_lag0": "n17_s528",
}


@pytest.mark.parametrize("mistake", A.MISTAKES)
def test_planted_mistake_leaves_the_bound_by_100(mistake):
    row = A.ROW[CAUGHT_ON[mistake]]
    f, df = _f(row)
    lags, got = A.emulate_row(row, mistake=mistake)
    q, _ = A.err_over_bound(got, f[lags], df[lags])
    print(f"\n{mistake}: caught on {row.name}, err / bound = {q:.3g}")
    assert q >= 100.0, f"{mistake} stays within 100x the bound on {row.name}: {q:.3g}"


def test_every_mistake_has_a_case():
    assert set(CAUGHT_ON) == set(A.MISTAKES) and len(A.MISTAKES) == 7


# ---- 4. no window decision near its bound --------------------------------------------------------------------------------
def test_no_window_decision_lies_near_its_bound():
    rng = np.random.default_rng(0)
    for row in A.ROWS:
        R = A.ref(row)
        windows, tau, dtau, margins, dread = R.tau()
        for dd in range(row.d):
            m = min(margins[dd])
            if math.isfinite(m):
                assert m >= 100.0 * dread[dd], f"{row.name} parameter {dd}: margin {m:.3g}, tau bound {dread[dd]:.3g}"
        L = max(len(m) for m in margins)
        f, df = R.f(L)
        for _ in range(8):
            g = f + df * rng.choice((-1.0, 1.0), size=f.shape)
            w2, tau2, _ = A.sokal(g, row.n_t)
            assert np.array_equal(w2, windows), f"{row.name}: a +-bound perturbation of f moves a window"
            fin = np.isfinite(tau)
            assert np.array_equal(np.isnan(tau2), ~fin) and np.all(np.abs(tau2 - tau)[fin] <= dtau[fin] + 2.0 * (windows[fin] + 1) * A.U)   # + the rounding of g itself


# ---- 5. input conditions ------------------------------------------------------------------------------------------------
def test_cases_satisfy_the_conditions_of_the_bound():
    for row in A.ROWS:
        R = A.ref(row)
        assert R.conditioned, f"{row.name}: a[0] <= 2 da[0] for some series"
        _, df = _f(row)
        stuck = A.stuck_parameters(row)
        assert np.array_equal(np.flatnonzero(np.isnan(df).all(axis=0)), np.array(stuck, dtype=int))
        fin = [dd for dd in range(row.d) if dd not in stuck]
        if not fin:
            continue
        worst = float(df[:, fin].max())
        if row.kind == "plus1e6":
            print(f"\n{row.name}: bound on f = {worst:.3e} (the centring error of a mean near 1e6)")
        else:
            assert worst <= 1e-9, f"{row.name}: bound on f {worst:.3e}"


def test_table_covers_every_edge():
    n_ts = {r.n_t for r in A.ROWS}
    assert {1, 15, 16, 17, 127, 128, 129, 130, 1000, 4100} <= n_ts
    assert sum(r.n_t == 4100 for r in A.ROWS) == 1 and A.ROW["n4100_lag_cap"].n_lags == 4096
    assert {(1, 1), (37, 7), (33, 16), (257, 1), (300, 2)} == {(r.nw, r.d) for r in A.ROWS}
    assert any(r.w0 == 5 and r.nw % 2 == 1 and r.width > r.nw + 5 for r in A.ROWS)
    assert {0, 3} == {r.first for r in A.ROWS}
    assert {"all", "one", "17", "blocks"} == {r.lags for r in A.ROWS}
    assert set(A.KINDS) == {r.kind for r in A.ROWS} and len(A.ROWS) <= 26
    assert A.chunking(130) == (8, 32) and A.chunking(1000) == (8, 128) and A.chunking(15) == (1, 16)


# ---- the pooled moments -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", A.MOMENT_KINDS)
def test_pooled_moments_reference_and_bounds(kind):
    """numpy's float64 moments lie inside the bound (pairwise sums: far fewer roundings than the bound allows), and the
    bound is small against the quantities themselves except for the variance under the +1e6 centring error."""
    for R in A.MOMENT_ROWS[:-1]:
        for d in A.MOMENT_D:
            x = A.moment_rows(R, d, kind)
            mean, var = A.pooled_moments(x)
            em, ev = A.pooled_bounds(x)
            assert np.all(np.abs(x.mean(axis=0) - mean.astype(np.float64)) <= em)
            assert np.all(np.abs(x.var(axis=0) - var.astype(np.float64)) <= ev)
            if R == 1:
                assert np.all(var == 0)
