"""CPU tests of the extended-precision cross-validation reference and its error bound (tests/cv_hp_ref.py) on the
table of tests/cv_cases.py: the table's admission record, a float64 run of the device's algorithm inside the bound,
the reference against an extended brute-force refit, the bound's tightness where the problem is easy, and the defects
the bound catches (which today's fixed tolerances of test_gpu_cross_validation.py let through)."""
import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

import cv_cases as CC
import cv_hp_ref as H
from hp_ref import LD, _chol_ld, _solve_lower_ld

# today's tolerances (tests/test_gpu_cross_validation.py): the gap the bound closes is stated against them
MTOL, VREL, VABS = 1e-9, 1e-9, 1e-14
# the tightness caps: conditions on the reference alone, on every noise = 5e-2 case
MEAN_CAP, VAR_CAP_REL, VAR_CAP_ABS = 1e-11, 1e-11, 1e-15

ADMITTED = [c.name for c in CC.cases()]
EASY = [c.name for c in CC.cases() if c.noise == 5e-2]
DEFECTS = ["alpha_entry", "G_row", "M_entry", "u_scaled", "no_jitter", "A_term_dropped", "pad_leak"]
SMALL_PERTURBATIONS = DEFECTS[:4]          # the four relative 1e-11 changes
EPS = 1e-11


def restate64(p: H.Problem, defect=None):
    """The device's algorithm in float64 with LAPACK / BLAS for its blocked kernels: W = L^-1 by substitution, per fold
    the gathered G, A = G G^T, its Cholesky, M = C^-1 by substitution, u = M alpha_I, v = M^T u, s = column sums of M^2,
    then cv_hp_ref.back_project's formula in float64.  defect: one departure, applied to every PC's largest fold."""
    N, k = p.y.shape
    mean, var = np.empty((N, k)), np.empty((N, k))
    folds = p.folds
    big = max(range(len(folds)), key=lambda f: len(folds[f]))
    for pc in range(k):
        W = solve_triangular(p.L[pc], np.eye(N), lower=True, check_finite=False)
        for f, I in enumerate(folds):
            d = defect if f == big else None
            m = len(I)
            G = W[int(I[0]):, I].T.copy()
            al = p.alpha[pc][I].copy()
            if d == "alpha_entry":
                al[np.argmax(np.abs(al))] *= 1 + EPS
            if d == "G_row":
                G[m // 2] *= 1 + EPS
            A = G @ G.T
            if d == "A_term_dropped" and m > 1:              # one product of one off-diagonal element never added
                c = np.argmax(np.abs(G[0] * G[1]))
                A[1, 0] -= G[1, c] * G[0, c]
                A[0, 1] = A[1, 0]
            if d == "pad_leak":
                # A padded row of G not zero.  The padded rows come last, and the factor and inverse of a leading block
                # do not depend on later rows: on its own the leak cannot reach the m results.  It shows where the
                # epilogue's column sums run over the padded rows as well, which is how it is modelled here.
                g = G @ (1e-3 * G[0])
                A = np.block([[A, g[:, None]], [g[None, :], np.ones((1, 1))]])
            Cf = cholesky(A, lower=True, check_finite=False)
            M = solve_triangular(Cf, np.eye(len(A)), lower=True, check_finite=False)[:, :m]
            if d == "M_entry":
                M[np.unravel_index(np.argmax(np.abs(M)), M.shape)] *= 1 + EPS
            u = M[:m] @ al
            if d == "u_scaled":
                u = u * (1 + EPS)
            v, s = M[:m].T @ u, np.sum(M * M, axis=0)      # (M has m rows unless the padding leaks)
            mean[I, pc] = p.y[I, pc] - v
            raw = s if d == "no_jitter" else s - p.jitter[pc]
            var[I, pc] = raw if d == "no_clip" else np.maximum(raw, 0.0)
    S, sc = p.components, p.scaler_scale
    cv = (mean @ S) * sc + p.scaler_mean
    vo = (var @ S ** 2 + p.cov_unexpl_diag) * sc ** 2
    return mean, var, cv, vo


@pytest.mark.parametrize("name", [c.name for c in CC.drafted()])
def test_admission_record_is_right(name):
    c = CC.case(name)
    try:
        ref = CC.reference(name)
        holds = True
        print(f"{name}: ||Sigma|| ||dA|| = {ref.first_order:.2e}, dW / (C u |W||L||W|) <= {ref.dW_over_closed_form:.1f}")
        assert ref.first_order <= H.FIRST_ORDER_LIMIT
    except H.NotFirstOrder as e:
        holds = False
        print(f"{name}: refused: {e}")
    assert holds == c.admitted, f"{name}: the table records admitted={c.admitted}, the first-order condition says {holds}"


def test_a_noise_free_case_of_every_kernel_family_is_admitted():
    free = {(c.kind, c.nu, c.const) for c in CC.cases() if c.noise is None}
    assert {(kind, nu, const) for _, kind, nu, const in CC._KERNELS} <= free


def test_the_table_reaches_what_it_says():
    """fold sizes of the padding / tile edges, the layouts and the PCs named in cv_cases' docstring"""
    sizes = {}
    for c in CC.cases():
        lab = CC.fold_labels(c)
        assert lab.shape == (c.N,) and set(lab) == set(range(lab.max() + 1))
        sizes[c.name] = np.bincount(lab)
    biggest = {int(s.max()) for s in sizes.values()}
    assert {63, 64, 65, 129, 257} <= biggest
    assert {1, 15, 129} <= set(sizes["mixed_1_15_129"])
    lab = CC.fold_labels(CC.case("last_point_alone"))
    N = len(lab)
    assert np.flatnonzero(lab == 0).tolist() == [N - 1] and np.flatnonzero(lab == 1).min() >= N - 15
    lab = CC.fold_labels(CC.case("ends_in_one_fold"))
    assert lab[0] == lab[-1]
    assert {c.N for c in CC.cases() if c.folds == "loo"} == {2, 3, 63, 64, 65, 129}
    assert {1, 3} <= {c.k for c in CC.cases()} and max(c.k for c in CC.cases()) >= 11
    assert max(c.N for c in CC.cases()) <= 400


@pytest.mark.parametrize("name", ADMITTED)
def test_float64_run_of_the_algorithm_is_inside_the_bound(name):
    p, ref = CC.problem(name), CC.reference(name)
    out = restate64(p)
    r = H.ratios(out, ref)
    print(f"{name} [{CC.case(name).conditioning}] max err / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert not H.violations(out, ref)


def _brute_force_ld(p: H.Problem, pc):
    """drop fold I, factor K_RR + jitter I (rebuilt as L L^T in longdouble), predict I: (mean, var before the clip,
    |Sigma A_I:| |K alpha - y|: what an alpha that is not exactly K^-1 y moves the identity's mean by)"""
    N = p.y.shape[0]
    L = np.tril(p.L[pc]).astype(LD)
    Kt = L @ L.T
    y, al = p.y[:, pc].astype(LD), p.alpha[pc].astype(LD)
    res = np.abs(Kt @ al - y)
    mean, var, aterm = np.empty(N, dtype=LD), np.empty(N, dtype=LD), np.empty(N, dtype=LD)
    for I in p.folds:
        Rr = np.setdiff1d(np.arange(N), I)
        Cr = _chol_ld(Kt[np.ix_(Rr, Rr)])
        V = _solve_lower_ld(Cr, np.concatenate([Kt[np.ix_(Rr, I)], y[Rr, None]], axis=1))
        Vk, vy = V[:, :-1], V[:, -1]
        mean[I] = Vk.T @ vy
        var[I] = np.diag(Kt)[I] - LD(p.jitter[pc]) - np.sum(Vk * Vk, axis=0)
        # Sigma A_I: = [1 on I itself, -K_IR K_RR^-1 on R]
        wts = _solve_lower_ld(np.swapaxes(Cr, 0, 1)[::-1, ::-1], Vk[::-1])[::-1]     # K_RR^-1 K_RI
        aterm[I] = res[I] + np.abs(wts).T @ res[Rr]
    return mean, var, aterm


@pytest.mark.parametrize("name", ["loo_n3", "loo_n63", "last_point_alone", "sweep_m05_free", "alien_alpha_free"])
def test_reference_against_extended_brute_force_refits(name):
    """The closed form is evaluated from the GIVEN alpha, the refit from y: with r = (K + jitter I) alpha - y they
    differ by Sigma (A r)_I, bounded here by |Sigma A_I:| |r| -- the one term added to the bound."""
    p, ref = CC.problem(name), CC.reference(name)
    if CC.case(name).data == "alien_alpha":
        # the refit knows nothing of a foreign alpha: compare at the y it belongs to, y' = (K + jitter I) alpha
        L = np.tril(p.L[0]).astype(LD)
        yp = (L @ (L.T @ p.alpha[0].astype(LD))).astype(np.float64)
        p = H.Problem(L=p.L[:1], alpha=p.alpha[:1], jitter=p.jitter[:1], y=yp[:, None], fold=p.fold,
                      components=p.components[:1], scaler_mean=p.scaler_mean, scaler_scale=p.scaler_scale,
                      cov_unexpl_diag=p.cov_unexpl_diag)
        ref = H.reference(p)
    for pc in range(p.y.shape[1]):
        bm, bv, aterm = _brute_force_ld(p, pc)
        em = np.abs(ref.mean_pc[:, pc] - bm).astype(np.float64)
        ev = np.abs(ref.var_raw[:, pc] - bv).astype(np.float64)
        allowed = ref.mean_bound[:, pc] + aterm.astype(np.float64)
        print(f"{name} PC {pc}: mean err / (bound + alpha term) {np.max(em / allowed):.3g} (alpha term up to "
              f"{float(np.max(aterm)):.2e}), var err / bound {np.max(ev / ref.var_bound[:, pc]):.3g}")
        assert np.all(em <= allowed) and np.all(ev <= ref.var_bound[:, pc])


@pytest.mark.parametrize("name", EASY)
def test_bound_is_tight_where_the_problem_is_easy(name):
    p, ref = CC.problem(name), CC.reference(name)
    ymax = np.max(np.abs(p.y))
    var = ref.var_pc.astype(np.float64)
    print(f"{name}: mean bound / max|y| {np.max(ref.mean_bound) / ymax:.2e}, "
          f"var bound / var {np.max(ref.var_bound / var):.2e}")
    assert np.max(ref.mean_bound) <= MEAN_CAP * ymax
    assert np.all(ref.var_bound <= VAR_CAP_REL * var + VAR_CAP_ABS)


def _passes_todays_tolerances(out, ref, p):
    m, v = out[0], out[1]
    rm, rv = ref.mean_pc.astype(np.float64), ref.var_pc.astype(np.float64)
    return bool(np.max(np.abs(m - rm)) <= MTOL * np.max(np.abs(p.y)) and np.all(np.abs(v - rv) <= VREL * np.abs(rv) + VABS))


@pytest.mark.parametrize("defect", DEFECTS)
def test_defects_leave_the_bound(defect):
    caught = []
    for name in EASY:
        p, ref = CC.problem(name), CC.reference(name)
        if max(len(I) for I in p.folds) == 1 and defect in ("A_term_dropped", "M_entry", "G_row", "pad_leak"):
            continue                                        # leave-one-out has no off-diagonal, M or padding
        out = restate64(p, defect)
        if H.violations(out, ref):
            caught.append(name)
        if defect in SMALL_PERTURBATIONS:
            assert _passes_todays_tolerances(out, ref, p), f"{defect} on {name}: today's tolerances do catch it"
    print(f"{defect}: outside the bound on {len(caught)} of {len(EASY)} noise = 5e-2 cases: {caught}")
    assert caught, f"{defect} stays inside the bound on every noise = 5e-2 case"


DUPS = [c.name for c in CC.cases() if c.data.startswith("dup")]


@pytest.mark.parametrize("name", DUPS)
def test_near_duplicates_and_the_clip(name):
    """On a consistent model the exact variance is a predictive variance: never negative, and at a held-out twin about
    the jitter, far above the bound -- the reference never clips there.  Only the raised-pivot case clips."""
    ref = CC.reference(name)
    clipped = ref.var_raw < 0
    print(f"{name}: smallest unclipped variance {float(ref.var_raw.min()):.2e}, its bound "
          f"{float(ref.var_bound.flat[np.argmin(ref.var_raw)]):.2e}, {int(clipped.sum())} clipped")
    if CC.case(name).data == "dup_split_pivot":
        assert clipped.any() and np.all(ref.var_pc[clipped] == 0)
    else:
        assert not clipped.any()


def test_clip_left_out_is_caught_on_a_near_duplicate_case():
    caught = []
    for name in DUPS:
        p, ref = CC.problem(name), CC.reference(name)
        assert not H.violations(restate64(p), ref)
        if H.violations(restate64(p, "no_clip"), ref):
            caught.append(name)
    print(f"no_clip: caught on {caught}")
    assert caught
