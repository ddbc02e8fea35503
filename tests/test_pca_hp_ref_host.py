"""CPU tests of the extended-precision scaler + PCA reference, its bounds and its certificates (tests/pca_hp_ref.py) on
the table of tests/pca_cases.py: the admission conditions on the reference alone; the split-operand product against
longdouble; the reference itself, LAPACK's float64 SVD and a float64 run of the device's algorithm inside every Kind A
bound and every Kind B certificate; and the defects the checks catch, each on a named case by a named check.

``device64`` restates csrc/k_pca.hip in float64 numpy: the scaler's sums in row order and the corrected two-pass
variance, blocks of PB columns paired round-robin, the Gram matrix of a pair summed over row splits in split order, a
two-sided Jacobi solve on it accumulating J (every pair of the 2 PB columns in a sweep's first round, the pairs across
the two blocks afterwards; larger column first; a second inner sweep per encounter from the 19th sweep on), X <- X J
on data and rotation rows, the stopping rule and the residue rule of DESIGN 4.7, and the host assembly with the sign
rule.  One argument seeds one defect:

    a  convergence tolerance x 1000           e  rotation rows of the last 16-row strip not updated
    b  pairs inside a block never rotated     f  one-pass variance
    c  residue threshold x 1e6                g  the sign index taken last instead of first on exact ties
    d  the last Gram split left out           h  explained_variance divided by N instead of N - 1
"""
import math

import numpy as np
import pytest

import pca_cases as PC
import pca_hp_ref as H

EPS = 2.220446049250313e-16
SWEEP_LIMIT = 60
SECOND_INNER_FROM = 18       # from the 19th sweep on the PB = 16 instance makes two inner sweeps per encounter


# ---- the device's algorithm in float64 --------------------------------------------------------------------------------------
def scaler64(Y, one_pass=False):
    N = Y.shape[0]
    T = Y.sum(axis=0) / N                                    # numpy adds the rows in order
    if one_pass:
        var = (Y * Y).sum(axis=0) / N - T * T
    else:
        t = Y - T
        corr, sq = t.sum(axis=0), (t * t).sum(axis=0)
        var = (sq - corr * corr / N) / N
    bound = N * EPS * var + (N * T * EPS) ** 2
    with np.errstate(invalid="ignore"):
        sc = np.sqrt(var)
    sc = np.where((var <= bound) | (sc == 0.0) | np.isnan(sc), 1.0, sc)
    Ys = (Y - T) / sc
    pm = Ys.sum(axis=0) / N
    return T, var, sc, pm, Ys - pm


def _block_pair(nb, rnd, i):
    nm1 = nb - 1
    P, Q = (nm1, rnd % nm1) if i == 0 else ((rnd + i) % nm1, (rnd - i + nm1) % nm1)
    return (P, Q) if P < Q else (Q, P)


def _solve(A, full, inner, tol, noise2):
    """Jacobi rotations on the Gram matrix A of one pair of blocks; returns J (or None: nothing rotated)"""
    PP = A.shape[0]
    PB = PP // 2
    A = A.copy()
    J = np.eye(PP)
    tol2 = tol * tol
    any_rotation = False
    if full:
        players = list(range(PP))
        rounds = []
        for _ in range(PP - 1):
            p, q = np.array(players[:PB]), np.array(players[PB:][::-1])
            rounds.append((np.minimum(p, q), np.maximum(p, q)))
            players = [players[0], players[-1]] + players[1:-1]
    else:
        x = np.arange(PB)
        rounds = [(x, PB + (x + r) % PB) for r in range(PB)]
    for _ in range(inner):
        rotated = False
        for p, q in rounds:
            a, b, g = A[p, p], A[q, q], A[p, q]
            live = (g * g > tol2 * (a * b)) & ((a > noise2) | (b > noise2))
            if not live.any():
                continue
            d, h = b - a, 2.0 * np.where(live, g, 1.0)
            t = np.abs(h) / (np.abs(d) + np.sqrt(d * d + h * h))
            t = np.where((d < 0) != (h < 0), -t, t)
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = c * t
            swap = (a - t * g) < (b + t * g)                         # larger column first: (c, s) <- (s, -c)
            c, s = np.where(swap, s, c), np.where(swap, -c, s)
            c, s = np.where(live, c, 1.0), np.where(live, s, 0.0)
            R = np.eye(PP)
            R[p, p], R[q, q], R[q, p], R[p, q] = c, c, -s, s
            A = R.T @ A @ R
            A[p[live], q[live]] = 0.0
            A[q[live], p[live]] = 0.0
            J = J @ R
            rotated = any_rotation = True
        if not rotated:
            break
    return J if any_rotation else None


def device64(Y, defect=None, flip_u=False, sweep_limit=SWEEP_LIMIT):
    """gpemu_pca_fit's outputs (all min(N, F) components) by the device's algorithm in float64; "converged" tells whether
    the stopping rule was met within the sweep limit"""
    Y = np.asarray(Y, dtype=np.float64)
    N, F = Y.shape
    mean, var, scale, pmean, Xc = scaler64(Y, one_pass=defect == "f")
    tw = N < F
    A0 = Xc.T if tw else Xc
    m, n = A0.shape
    PB = 16 if n <= 1024 else 32
    nb = max(2, 2 * math.ceil(n / (2 * PB)))
    ncols, npairs = nb * PB, nb // 2
    chunks = math.ceil(m / 64)
    nsplit = max(1, min(chunks, min(8, 256 // npairs)))
    inner = 1 if PB == 16 else 2
    W = np.zeros((m + n, ncols))
    W[:m, :n] = A0
    W[m + np.arange(n), np.arange(n)] = 1.0
    tol = 4.0 * math.sqrt(m) * EPS * (1000.0 if defect == "a" else 1.0)
    lim = 4.0 * math.sqrt(m) * EPS * (1e6 if defect == "c" else 1.0)
    noise2 = lim * lim * float((Xc * Xc).sum())
    edges = [min(m, 64 * (chunks * s // nsplit)) for s in range(nsplit + 1)]
    frozen = slice(m + 16 * ((n - 1) // 16), m + n) if defect == "e" else None
    converged, sweeps = False, 0
    for sweeps in range(1, sweep_limit + 1):
        off = 0.0
        for rnd in range(nb - 1):
            for i in range(npairs):
                P, Q = _block_pair(nb, rnd, i)
                cols = np.r_[P * PB:(P + 1) * PB, Q * PB:(Q + 1) * PB]
                X = W[:, cols]
                parts = [X[edges[s]:edges[s + 1]].T @ X[edges[s]:edges[s + 1]] for s in range(nsplit)]
                if defect == "d" and nsplit > 1:
                    parts = parts[:-1]
                G = parts[0]
                for part in parts[1:]:
                    G = G + part
                dg = np.diag(G)
                den2 = np.outer(dg, dg)
                ok = (den2 > 0) & (G != 0) & ((dg[:, None] > noise2) | (dg[None, :] > noise2))
                np.fill_diagonal(ok, False)
                worst = math.sqrt(float(np.max(np.where(ok, G * G / np.where(den2 > 0, den2, 1.0), 0.0))))
                off = max(off, worst)
                if not worst > tol:
                    continue
                J = _solve(G, full=(rnd == 0 and defect != "b"), inner=2 if (PB == 16 and sweeps > SECOND_INNER_FROM) else inner,
                           tol=tol, noise2=noise2)
                if J is None:
                    continue
                keep = W[frozen, cols].copy() if frozen is not None else None
                W[:, cols] = X @ J
                if frozen is not None:
                    W[frozen, cols] = keep
        if off <= tol:
            converged = True
            break
    # host assembly
    sigma = np.sqrt((W[:m] ** 2).sum(axis=0))
    real = np.flatnonzero(np.any(W[m:] != 0.0, axis=0))
    assert real.size == n
    order = real[np.argsort(-sigma[real], kind="stable")]
    total = float(np.sum(sigma[order] ** 2 / (N - 1)))
    comp, scores = np.zeros((n, F)), np.zeros((N, n))
    arg = np.zeros(n, dtype=np.int64)
    ev = sigma[order] ** 2 / (N if defect == "h" else N - 1)
    for c, j in enumerate(order):
        g, v, sg = W[:m, j], W[m:, j], sigma[j]
        row = v if not tw else (g / sg if sg > 0 else np.zeros(F))
        us = (v if tw else g) if flip_u else row
        mag = np.abs(us)
        arg[c] = (mag.size - 1 - int(np.argmax(mag[::-1]))) if defect == "g" else int(np.argmax(mag))
        sign = -1.0 if us[arg[c]] < 0 else 1.0
        comp[c] = sign * row
        scores[:, c] = sign * g if not tw else sign * sg * v
    with np.errstate(divide="ignore", invalid="ignore"):
        evr = ev / total
    return dict(scaler_mean=mean, scaler_var=var, scaler_scale=scale, pca_mean=pmean, components=comp, explained_variance=ev,
                explained_variance_ratio=evr, Y_pca=scores, flip_argmax=arg, n_sweeps=sweeps, converged=converged)


def lapack64(Y, flip_u=False):
    """the same outputs from LAPACK's float64 SVD of the float64 centred matrix, signs by sklearn's rule"""
    N, F = Y.shape
    mean, var, scale, pmean, Xc = scaler64(np.asarray(Y, dtype=np.float64))
    Ul, s, Vt = np.linalg.svd(Xc, full_matrices=False)
    scores = Ul * s
    n = s.size
    arg = np.zeros(n, dtype=np.int64)
    for c in range(n):
        us = scores[:, c] if flip_u else Vt[c]
        arg[c] = int(np.argmax(np.abs(us)))
        if us[arg[c]] < 0:
            Vt[c], scores[:, c] = -Vt[c], -scores[:, c]
    ev = s * s / (N - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        evr = ev / ev.sum()
    return dict(scaler_mean=mean, scaler_var=var, scaler_scale=scale, pca_mean=pmean, components=Vt, explained_variance=ev,
                explained_variance_ratio=evr, Y_pca=scores, flip_argmax=arg)


def reference_as_output(ref):
    """the reference rounded to float64, in the shape of the device's outputs"""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    n = ref.geo.n
    arg = np.zeros(n, dtype=np.int64)
    arg[:ref.n_pc] = ref.flip_argmax
    return dict(scaler_mean=f(ref.scaler_mean), scaler_var=f(ref.scaler_var), scaler_scale=f(ref.scaler_scale),
                pca_mean=f(ref.pca_mean), components=f(ref.components), explained_variance=f(ref.ev),
                explained_variance_ratio=f(ref.evr), Y_pca=f(ref.scores), flip_argmax=arg)


def truncation64(out, k):
    C, lam = out["components"][k:], out["explained_variance"][k:]
    return (C.T * lam) @ C


def all_checks(name, out):
    """{check: ratio} and the list of violated checks of one decomposition of one referenced case"""
    c, ref = PC.case(name), PC.reference(name)
    ra = H.ratios_a(out, ref, truncation64(out, c.n_pc))
    bad = H.violations_a(out, ref, truncation64(out, c.n_pc))
    cert = H.certificates(out, ref.Xc, ref.geo, sigma_ref=ref.sigma)
    rb, bad_b = H.violations_b(cert, ref.R_b)
    return {**ra, **rb}, bad + bad_b


def _fmt(r):
    return ", ".join(f"{k} {v:.2g}" for k, v in r.items())


# ---- the table and the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.REFERENCED)
def test_admission_conditions_hold_on_the_reference(name):
    c, ref = PC.case(name), PC.reference(name)
    undecided = int((~ref.flip_decided).sum())
    print(f"{name}: gap factor {ref.min_gap_factor:.2f}, constant-feature margin {ref.const_margin.min():.3g}, "
          f"{undecided} undecided sign decisions, reference cosine {ref.cos_max:.1e} after {ref.ref_sweeps} sweeps")
    assert ref.min_gap_factor >= H.GAP_FACTOR
    assert ref.const_margin.min() >= H.CONST_MARGIN
    assert undecided <= 1
    assert ref.cos_max <= 4 * math.sqrt(ref.geo.m) * float(np.finfo(H.LD).eps)


def test_the_table_reaches_what_it_says():
    geo = {c.name: H.geometry(c.N, c.F) for c in PC.cases()}
    assert [geo[n].nb for n in ("cols31", "cols32", "cols33", "cols64", "cols65", "cols96")] == [2, 2, 4, 4, 6, 6]
    assert geo["rows64"].m == 64 and geo["rows65"].m == 65
    assert math.ceil(geo["splits5"].m / 64) == 5 and math.ceil(geo["splits8"].m / 64) == 9
    assert geo["wide24x70"].transposed and geo["wide33x300"].transposed and not geo["square40"].transposed
    assert [geo[n].PB for n in PC.CERTIFICATE_ONLY] == [32, 32] and geo["pb32_wide1025x1100"].transposed
    assert all(geo[n].PB == 16 for n in PC.REFERENCED)
    both = {bool(v) for n in ("const_edge_tall", "const_edge_wide") for v in PC.reference(n).constant[:4]}
    assert both == {True, False}
    for n in ("allconst_tall", "allconst_wide"):
        ref = PC.reference(n)
        assert ref.constant.all() and np.all(ref.ev == 0) and np.isnan(np.asarray(ref.evr, dtype=np.float64)).all()
    assert {c.flip for c in PC.cases()} == {"v", "u"}
    for n in ("graded_tall", "graded_wide"):                # real columns between the residue threshold and 1e6 times it
        ref = PC.reference(n)
        thr = ref.geo.residue_threshold(ref.fro)
        sg = np.asarray(ref.sigma, dtype=np.float64)
        assert ((sg > 10 * thr) & (sg < 1e5 * thr)).sum() >= 4 and (sg > 1e6 * thr).sum() > ref.n_pc
    ref = PC.reference("dup_tall")                          # and residue proper: exact rank deficiency (20 duplicates, 3 constants)
    assert (np.asarray(ref.sigma, dtype=np.float64) < ref.geo.residue_threshold(ref.fro)).sum() == 23
    assert {(c.F, c.n_comp - c.n_pc) for c in PC.trunc_cases()} >= {(1, 1), (70, 1), (70, 31), (70, 32), (70, 33)}
    assert {c.F for c in PC.trunc_cases()} >= {1, 63, 64, 65, 130}


def test_split_product_equals_longdouble_over_eight_decades():
    rng = np.random.default_rng(7)
    A = rng.normal(size=(1025, 96)) * 10.0 ** rng.uniform(-8, 0, 96)
    Al = A.astype(H.LD)
    G, Gl = H.xgram(A), Al.T @ Al
    d = np.sqrt(np.diag(Gl))
    err = float(np.max(np.abs(G - Gl) / np.outer(d, d)))
    print(f"split-operand Gram against longdouble, 1025 x 96, norms over eight decades: {err:.2e} in cosine units")
    assert err <= 2e-18       # the longdouble sum of 1025 terms itself is good to about sqrt(1025) 2^-64 = 1.7e-18
    B = rng.normal(size=(96, 40))
    P, Pl = H.xmatmul(A, B), Al @ B.astype(H.LD)
    scale = np.outer(np.max(np.abs(A), axis=1), np.max(np.abs(B), axis=0)) * 96
    assert float(np.max(np.abs(P - Pl) / scale)) <= 2e-18


@pytest.mark.parametrize("name", PC.REFERENCED)
def test_reference_lapack_and_the_float64_algorithm_pass_every_check(name):
    c, ref = PC.case(name), PC.reference(name)
    Y, flip_u = PC.data(name), c.flip == "u"
    runs = {"reference": reference_as_output(ref), "lapack": lapack64(Y, flip_u), "device64": device64(Y, flip_u=flip_u)}
    for who, out in runs.items():
        r, bad = all_checks(name, out)
        print(f"{name} {who}: {_fmt(r)}")
        assert not bad, f"{name}, {who}: " + "; ".join(bad)
    # (the model's sweep count is printed, not held to 30: its rotations are not the device's bit for bit, and the
    # graded spectra sit at the limit -- the device's own count is asserted in test_gpu_pca_hp.py)
    print(f"{name} device64: {runs['device64']['n_sweeps']} sweeps")
    assert runs["device64"]["converged"]


def test_the_non_convergence_case_needs_more_than_three_sweeps():
    out = device64(PC.data(PC.NEEDS_SWEEPS))
    assert 3 < out["n_sweeps"] <= H.SWEEPS
    assert not device64(PC.data(PC.NEEDS_SWEEPS), sweep_limit=1)["converged"]


# ---- the defects -----------------------------------------------------------------------------------------------------------
# defect -> (case, the check that must reject it)
DEFECTS = {
    "a": ("cols96", "cosines"),
    "b": ("cols33", "n_sweeps"),
    "c": ("graded_tall", "cosines"),
    "d": ("splits5", "cosines"),
    "e": ("cols33", "rotation_orthogonality"),
    "f": ("offset_tall", "scaler_var"),
    "g": ("n2x2", "flip"),
    "g_u": ("n2x2_u", "flip"),
    "h": ("flat_tall", "explained_variance"),
}
# today's fixed tolerances (test_gpu_fit.py, test_gpu_shapes.py), against LAPACK: what defects a and c pass
TODAY = dict(ev=1e-11, comp=1e-9)


def _passes_todays_tolerances(name, out):
    c = PC.case(name)
    ref = lapack64(PC.data(name), c.flip == "u")
    k = c.n_pc
    ev_ok = np.max(np.abs(out["explained_variance"] - ref["explained_variance"])) < TODAY["ev"] * ref["explained_variance"][0]
    s = np.sign(np.sum(out["components"][:k] * ref["components"][:k], axis=1))
    comp_ok = np.max(np.abs(out["components"][:k] * s[:, None] - ref["components"][:k])) < TODAY["comp"]
    return bool(ev_ok and comp_ok)


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_defects_are_rejected(defect):
    name, check = DEFECTS[defect]
    c = PC.case(name)
    out = device64(PC.data(name), defect=defect[0], flip_u=c.flip == "u")
    r, bad = all_checks(name, out)
    print(f"defect {defect} on {name}: n_sweeps {out['n_sweeps']}, converged {out['converged']}; {_fmt(r)}; violated: {bad}")
    if check == "n_sweeps":
        assert not out["converged"] or out["n_sweeps"] > H.SWEEPS
    elif check == "flip":
        assert any("flip_argmax" in b for b in bad)
    else:
        assert not r[check] <= 1.0, f"defect {defect} stays inside {check} on {name}"
    if defect in ("a", "c"):
        print(f"defect {defect} on {name} passes today's fixed tolerances: {_passes_todays_tolerances(name, out)}")
        assert _passes_todays_tolerances(name, out)


# ---- the truncation covariance's reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in PC.trunc_cases()])
def test_truncation_cov_float64_is_inside_its_bound(name):
    c = PC.trunc_case(name)
    comp, ev = PC.trunc_data(name)
    val, bound = H.truncation_cov_ld(comp, ev, c.n_pc)
    got = (comp[c.n_pc:].T * ev[c.n_pc:]) @ comp[c.n_pc:]
    assert got.shape == (c.F, c.F) and np.all(np.abs(got - val) <= bound)
    if c.n_pc == c.n_comp:
        assert np.all(val == 0) and np.all(bound == 0)
    # a term left out, or a variance of the kept side let in, leaves the bound
    if c.n_pc < c.n_comp:
        r = c.n_pc
        assert not np.all(np.abs(got - ev[r] * np.outer(comp[r], comp[r]) - val) <= bound)
    if c.n_pc > 0:
        r = c.n_pc - 1
        assert not np.all(np.abs(got + ev[r] * np.outer(comp[r], comp[r]) - val) <= bound)


# ---- non-finite input is refused before the library is asked for a device ---------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_Y_raises_value_error_on_the_host(bad):
    from gpemu.fit import pca_fit
    Y = np.array(PC.data("n9x4"))
    Y[3, 1] = bad
    with pytest.raises(ValueError, match="NaN or infinity"):
        pca_fit(Y)
