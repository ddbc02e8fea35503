"""tests/grad_ref.py against central differences of hp_ref's log-likelihood, in np.longdouble (CPU only).

Every supported case of path_cases.cases() (Matern 0.5 rerun as 1.5; the general-nu cases are not differentiable by
this path), every reference row, every component: ``|analytic - FD(h/2)| <= |FD(h) - FD(h/2)| + 2^-60 |lp| / h`` -- the
difference scheme's own error estimate plus the rounding floor of a longdouble difference quotient.  The box prior is
left out: the queries on the box edge take part.  Step: ``h_i = 1e-4 min(hi_i - lo_i, min_p l_pi)``, so that a case
with a 1e-5 length scale is still differenced inside the kernel's range (fd_check: the one exception to the step)."""
from __future__ import annotations

import numpy as np
import pytest

import grad_ref as G
import hp_ref as H
import path_cases as PC

LD = np.longdouble
CASES, SKIPPED = G.sweep_cases()


def steps(X, model, lo, hi):
    """the common difference step h [d]: 1e-4 of the box width or of the smallest length scale, whichever is smaller"""
    lsmin = np.min(np.stack([gp.ls for gp in model.gps]), axis=0)
    return 1e-4 * np.minimum(hi - lo, lsmin)


def beside_a_training_row(X, model):
    """rows [B] whose stencil holds a point where the function is not three times differentiable.
    ``|FD(h) - FD(h/2)|`` estimates the scheme's error where it is.  A Matern kernel of finite nu is not at r = 0
    (a |r|^3 term at nu = 1.5, |r|^5 at 2.5): a query 1e-7 length scales beside a training row (path_cases.queries
    places them) has that row inside its stencil, and the scheme's error gains a share of order (offset) h that its
    estimate need not cover.  A query exactly ON a training row is not meant: the kernel is even about it, and the
    central difference of an even term is zero, as its derivative is."""
    spec = model.spec
    if not (spec.kind == G.O.MATERN and np.isfinite(spec.nu)):
        return np.zeros(X.shape[0], dtype=bool)
    return nearest_scaled_distance(X, model) < 1e-3


def nearest_scaled_distance(X, model):
    """[B] the smallest non-zero scaled distance of each row to a training row, over the PCs' length scales"""
    near = np.full(X.shape[0], np.inf)
    for gp in model.gps:
        r = np.sqrt((((X[:, None, :] - model.X_train[None]) / gp.ls) ** 2).sum(axis=2))
        near = np.minimum(near, np.where(r > 0, r, np.inf).min(axis=1))
    return near


def fd_quotients(X, model, setups, h, chunk=512):
    """central differences of the log-likelihood at steps h and h / 2 along every coordinate: (FD(h), FD(h/2)) [d, B]"""
    B, d = X.shape
    pts = []
    for i in range(d):
        for s in (1.0, 0.5):
            e = np.zeros(d, LD)
            e[i] = LD(s * h[i])
            pts += [X.astype(LD) + e, X.astype(LD) - e]
    P = np.concatenate(pts)
    vals = np.concatenate([G.loglik_ld(P[o:o + chunk], model, setups) for o in range(0, len(P), chunk)])
    vals = vals.reshape(d, 2, 2, B)
    hl = np.asarray(h, dtype=np.float64).astype(LD)[:, None]
    return (vals[:, 0, 0] - vals[:, 0, 1]) / (2 * hl), (vals[:, 1, 0] - vals[:, 1, 1]) / (2 * (0.5 * h).astype(LD)[:, None])


def fd_check(X, model, setups, grad, lp, lo, hi, what):
    """asserts ``|analytic - FD(h/2)| <= |FD(h) - FD(h/2)| + 2^-60 |lp| / h`` for grad [B, d] at the common step, in
    every component of every row.  A component of a row beside a training row (beside_a_training_row) that misses it
    there is held to the same criterion at ten times the step, where the non-smooth share, of order h, is a tenth as
    large against the h^2 term the estimate measures; and, if it misses that too (a model whose other training rows
    contribute nothing, so that there is no smooth h^2 term to dominate: the 1e-5 length scales), at a quarter of the
    row's scaled distance to that training row, where no stencil point comes nearer to it than three quarters of the
    query's own distance.  Nothing else gets another step.  Returns the largest err / tolerance at the common step
    and the number of components that took another step."""
    h = steps(X, model, lo, hi)
    fd1, fd2 = fd_quotients(X, model, setups, h)
    hl = h.astype(LD)[:, None]
    est = np.abs(fd1 - fd2) + LD(2.0) ** -60 * np.abs(lp)[None] / hl
    err = np.abs(grad.T - fd2)
    ratio = np.asarray(np.where(est > 0, err / np.where(est > 0, est, 1), np.where(err > 0, np.inf, 0)), dtype=np.float64)
    bad = ratio > 1.0
    second = 0
    if bad.any():
        beside = beside_a_training_row(X, model)
        rows = np.flatnonzero(bad.any(axis=0))
        stray = [int(r) for r in rows if not beside[r]]
        assert not stray, (f"{what}: rows {stray} miss the criterion: err / tolerance {ratio[:, stray].max(axis=0)}")
        g1, g2 = fd_quotients(X[rows], model, setups, 10 * h)
        est2 = np.abs(g1 - g2) + LD(2.0) ** -60 * np.abs(lp[rows])[None] / (10 * hl)
        err2 = np.abs(grad[rows].T - g2)
        still = bad[:, rows] & np.asarray(err2 > est2)
        if still.any():
            near = nearest_scaled_distance(X, model)
            lsmin = np.min(np.stack([gp.ls for gp in model.gps]), axis=0)
            for j in np.flatnonzero(still.any(axis=0)):
                r = rows[j]
                h3 = np.minimum(h, 0.25 * near[r] * lsmin)
                k1, k2 = fd_quotients(X[r:r + 1], model, setups, h3)
                est2[:, j] = np.abs(k1 - k2)[:, 0] + LD(2.0) ** -60 * np.abs(lp[r]) / h3.astype(LD)
                err2[:, j] = np.abs(grad[r] - k2[:, 0])
            still = still & np.asarray(err2 > est2)
        assert not still.any(), (f"{what}: (coordinate, row) {[(int(i), int(rows[j])) for i, j in np.argwhere(still)]} miss "
                                 f"the criterion at every step: err {np.asarray(err2[still], float)} tolerance "
                                 f"{np.asarray(est2[still], float)}")
        second = int(bad.sum())
        ratio = np.where(bad, 0.0, ratio)
    return float(ratio.max()), second


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c.name for c in CASES])
def test_gradient_reference_against_central_differences(idx):
    c = CASES[idx]
    model, lo, hi, y_exp, y_err, bs, rng = PC.problem(c)
    Xq, _, cols = PC.queries(c, model, lo, hi, rng)
    X = Xq[cols]
    ref = G.reference(X, model, y_exp, y_err, bs)
    clipped = np.argwhere(ref["clipped"])
    assert clipped.size == 0, f"{c.name}: clipped variances at (row, PC) {clipped.tolist()}: the function is not smooth there"
    # the function that is differenced is hp_ref's: the same values, up to longdouble rounding (far inside its bound)
    pred = H.gp_predict(X, model, input_rounding=c.ls_bounds)
    lp_h = H.loglik_blocks(pred[0], pred[1], ref["setups"])[0]
    lb = H.loglik_bound(pred[0], pred[1], pred[2], pred[3], ref["setups"])
    assert np.all(np.abs(np.asarray(ref["lp"] - lp_h, float)) <= 1e-3 * lb + 1e-300)
    on_edge = np.any((X <= lo) | (X >= hi), axis=1)
    n_special, n_free = PC.special_count(c)            # (specials beyond the free columns are dropped, edge rows first)
    assert on_edge.sum() >= max(0, c.d - max(0, n_special - n_free)), "the box-edge rows take part"
    worst, second = fd_check(X, model, ref["setups"], ref["grad"], ref["lp"], lo, hi, c.name)
    assert np.all(np.isfinite(ref["grad_bound"])) and np.all(ref["grad_bound"] >= 0)
    print(f"\nFD {c.name}: rows {len(X)} (on the edge {int(on_edge.sum())}) max err / tolerance {worst:.3g}"
          + (f"; {second} component(s) beside a training row at another step" if second else ""))


def test_general_nu_cases_are_counted():
    assert SKIPPED == ["n63_nu075_direct", "n64_nu2_const", "w12_ks4_nu075_direct_tasks_multi"]
    assert len(CASES) + len(SKIPPED) == len(PC.cases())
    assert all(G.supported(c.spec) for c in CASES)


@pytest.mark.parametrize("name", ["n16_d7_m15_const", "n65_halfstep_small_xcd", "n300_tasks_multi"])
def test_second_derivatives_against_differences_of_the_adjoints(name):
    """da/dm, da/dv, db/dm, db/dv (closed forms from z and P) against central differences of a and b in (m, v)"""
    c = [x for x in CASES if x.name == name][0]
    model, lo, hi, y_exp, y_err, bs, rng = PC.problem(c)
    Xq, _, cols = PC.queries(c, model, lo, hi, rng)
    X = Xq[cols][:6]
    mean, var, _ = G.predict_ld(X, model)
    setups = H.lowrank_setup_blocks(model, y_exp, y_err, bs)
    adj0 = G.adjoints(mean, var, setups)
    a0, b0, dadm, dadv, dbdm, dbdv, _ = adj0
    # the rounding floor: a and b themselves are evaluated with the error grad_ref's analysis gives for the device
    # (adjoint_bounds without input errors), at longdouble roundoff 2^-64 instead of 2^-53; a difference of two such
    # values over 2 (h / 2) carries twice that over h
    zero = np.zeros(mean.shape)
    na, nb = (2.0 ** -11 * x for x in G.adjoint_bounds(var, zero, zero, setups, adj0))
    k = model.n_pc
    for q in range(k):
        for wrt, da_ref, db_ref in (("m", dadm[:, :, q], dbdm[:, :, q]), ("v", dadv[:, :, q], dbdv[:, :, q])):
            base = mean if wrt == "m" else var
            scale = np.maximum(np.abs(np.asarray(base[:, q], float)), 1e-3)
            fds = []
            for s in (1.0, 0.5):
                e = np.zeros(base.shape, LD)
                e[:, q] = LD(1e-4 * s) * scale
                ap, bp = G.adjoints(mean + e, var, setups)[:2] if wrt == "m" else G.adjoints(mean, var + e, setups)[:2]
                am, bm = G.adjoints(mean - e, var, setups)[:2] if wrt == "m" else G.adjoints(mean, var - e, setups)[:2]
                fds.append(((ap - am) / (2 * e[:, q, None]), (bp - bm) / (2 * e[:, q, None])))
            hq = (1e-4 * scale)[:, None]
            for an, (f1, f2), noise in ((da_ref, (fds[0][0], fds[1][0]), na), (db_ref, (fds[0][1], fds[1][1]), nb)):
                est = np.abs(f1 - f2) + 2 * noise / hq
                assert np.all(np.abs(an - f2) <= est), (name, q, wrt, float(np.max(np.abs(an - f2) / est)))


def test_clip_case_has_both_branches_and_its_gradient_matches_differences():
    model, lo, hi, y_exp, y_err, bs, Xq = G.clip_case()
    ref = G.reference(Xq, model, y_exp, y_err, bs)
    sure_clipped = ref["clipped"] & ~ref["ambiguous"]
    sure_open = ~ref["clipped"] & ~ref["ambiguous"]
    assert sure_clipped.any(), "no variance is clipped beyond its bound"
    assert sure_open.any(), "no variance is unclipped beyond its bound"
    assert sure_clipped[:8, 0].all(), "PC 0 is clipped on every training row"
    assert np.all(ref["dvar"][ref["clipped"]] == 0) and np.all(ref["dvar_bound"][ref["clipped"]] == 0)
    # both branches of an ambiguous entry are on offer
    alt = G.reference(Xq, model, y_exp, y_err, bs, clip_choice=~ref["clipped"])
    assert np.array_equal(alt["clipped"][~ref["ambiguous"]], ref["clipped"][~ref["ambiguous"]])
    assert np.array_equal(alt["clipped"][ref["ambiguous"]], ~ref["clipped"][ref["ambiguous"]])
    # the reference's own branch is constant over the difference stencil: the function is smooth there
    h = steps(Xq, model, lo, hi)
    for i in range(Xq.shape[1]):
        for s in (-1.0, 1.0):
            e = np.zeros(Xq.shape[1], LD)
            e[i] = LD(s * h[i])
            raw = G.predict_ld(Xq.astype(LD) + e, model)[2]
            assert np.array_equal(raw < 0, ref["var_raw"] < 0)
    worst, second = fd_check(Xq, model, ref["setups"], ref["grad"], ref["lp"], lo, hi, "clip case")
    assert second == 0
    print(f"\nFD clip case: clipped {int(ref['clipped'].sum())} (beyond the bound {int(sure_clipped.sum())}), ambiguous "
          f"{int(ref['ambiguous'].sum())}, max err / tolerance {worst:.3g}")


def _within_observable_cov(y_err, bs, ell=3.0):
    """a dense data covariance inside each observable block (exponential correlation of neighbouring bins), zero across"""
    F = len(y_err)
    i = np.arange(F)
    obs = np.searchsorted(np.asarray(bs)[1:], i, side="right")
    C = np.outer(y_err, y_err) * np.exp(-np.abs(i[:, None] - i[None, :]) / ell)
    return np.where(obs[:, None] == obs[None, :], C, 0.0)


def test_dense_within_observable_covariance_changes_only_the_setup():
    """setups_with_cov with cov = diag(y_err^2) is hp_ref's setup; with a dense covariance the gradient still matches
    central differences of the log-likelihood built on those setups"""
    c = [x for x in CASES if x.name == "n300_tasks_multi"][0]
    model, lo, hi, y_exp, y_err, bs, rng = PC.problem(c)
    Xq, _, cols = PC.queries(c, model, lo, hi, rng)
    X = Xq[cols][:16]
    plain = H.lowrank_setup_blocks(model, y_exp, y_err, bs)
    same = G.setups_with_cov(model, y_exp, np.diag(y_err ** 2), bs)
    for a, b in zip(plain, same):
        # (y_err^2 squared in float64 here, in longdouble there: equal to float64 rounding, amplified by cond(A))
        for key in ("G", "g0", "q0", "logdetA"):
            np.testing.assert_allclose(np.asarray(a[key], float), np.asarray(b[key], float), rtol=1e-11, atol=1e-13)
    cov = _within_observable_cov(y_err, bs)
    assert np.count_nonzero(cov - np.diag(np.diag(cov))) > 0
    setups = G.setups_with_cov(model, y_exp, cov, bs)
    ref = G.reference(X, model, y_exp, y_err, bs, setups=setups)
    assert np.max(np.abs(np.asarray(ref["grad"] - G.reference(X, model, y_exp, y_err, bs)["grad"], float))) > 1e-3
    worst, _ = fd_check(X, model, setups, ref["grad"], ref["lp"], lo, hi, "dense covariance")
    print(f"\nFD dense covariance: max err / tolerance {worst:.3g}")
