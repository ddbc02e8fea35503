"""CPU: the extended-precision fit-side reference of tests/fit_ref.py and its error bound.

- the reference agrees with 40-digit mpmath arithmetic on small shapes (K, log det, gradient);
- calibration: honest float64 arithmetic (the LAPACK oracle) stays inside the bound on every shape of the sweep;
- sensitivity: a numpy restatement of the device's algorithm (64-wide blocked Cholesky in panels of four blocks,
  bottom-up triangular inverse with ragged pairs, the block-lower gemv, the gradient by (16-row group, 256-column block)
  pairs) stays inside the bound, and every injected bug leaves it on at least one shape where it applies.  Which of
  them the suite's old tolerances (L 1e-9, alpha 1e-7 relative, LML 1e-8 |lml|, gradient 1e-6 max|g|) also catch is
  printed (pytest -s).
"""
import math

import mpmath
import numpy as np
import pytest
from scipy.linalg import cho_solve, cholesky, solve_triangular

import fit_cases as FC
import fit_ref as FR
import hp_ref as H
import matern_nu_ref as MR
from oracle import gp_oracle as O

LD = np.longdouble
HOST_SHAPES = ["n17_nu07_noise", "n65_m15_dup", "n129_m25_lsb", "n271_nu07_all", "n273_rbf_dup", "n320_m05_ragged",
               "n448_nu2_ragged_steps", "n513_rbf_all",
               "w9_n130_m15_dup", "w12_n320_nu07_ragged", "w12_n129_m25_lsb", "w16_n200_rbf_lsb_steps", "w16_n257_m05_dup"]


def _case(name):
    return next(c for c in FC.cases() if c.name == name)


@pytest.fixture(scope="module")
def sweep():
    out = []
    for name in HOST_SHAPES:
        c = _case(name)
        p = FC.problem(c)
        out.append((c, p, FR.FitRef(p)))
    return out


# ---- mpmath ------------------------------------------------------------------------------------------------------------
def _mp_base(r, spec):
    if spec.kind == O.RBF or np.isinf(spec.nu):
        return mpmath.exp(-r * r / 2)
    nu = mpmath.mpf(spec.nu)
    t = mpmath.sqrt(2 * nu) * r
    return 2 ** (1 - nu) / mpmath.gamma(nu) * t ** nu * mpmath.besselk(nu, t)


@pytest.mark.parametrize("kind,nu,tol", [(O.RBF, np.inf, 1e-16), (O.MATERN, 0.5, 1e-16), (O.MATERN, 1.5, 1e-16),
                                         (O.MATERN, 2.5, 1e-16), (O.MATERN, 0.7, 1e-14), (O.MATERN, 3.5, 1e-14)])
def test_reference_matches_mpmath(kind, nu, tol):
    mpmath.mp.dps = 40
    c = FC.FitCase("mp", 6, 2, kind, nu, True, True)
    p = FC.problem(c)
    ref = FR.FitRef(p)
    ls, const, noise = p.hyper
    N, d = p.X.shape
    spec = p.spec
    X = [[mpmath.mpf(float(v)) for v in row] for row in p.X]
    lsm = [mpmath.mpf(float(v)) for v in ls]
    h = mpmath.mpf("1e-12")

    def kmat(lsv):
        K = mpmath.matrix(N, N)
        for i in range(N):
            for j in range(N):
                if i == j:
                    K[i, j] = 1 + mpmath.mpf(const) + mpmath.mpf(noise) + mpmath.mpf(p.jitter)
                else:
                    r = mpmath.sqrt(sum(((X[i][k] - X[j][k]) / lsv[k]) ** 2 for k in range(d)))
                    K[i, j] = _mp_base(r, spec) + mpmath.mpf(const)
        return K

    def lml(lsv):
        Km = kmat(lsv)
        return -(y.T * (Km ** -1) * y)[0] / 2 - mpmath.log(mpmath.det(Km)) / 2

    K = kmat(lsm)
    Kinv = K ** -1
    y = mpmath.matrix([mpmath.mpf(float(v)) for v in p.y])
    a = Kinv * y
    kscale = max(abs(float(K[i, j])) for i in range(N) for j in range(N))
    for i in range(N):
        for j in range(N):
            assert abs(float(ref.K[i, j] - LD(mpmath.nstr(K[i, j], 30)))) <= tol * kscale, (i, j)
    logdet = mpmath.log(mpmath.det(K)) / 2
    assert abs(float(ref.logdet_half - LD(mpmath.nstr(logdet, 30)))) <= 10 * tol * max(1.0, abs(float(logdet)))
    # the length-scale gradient against a central difference of the exact LML (step 1e-12: truncation ~1e-24)
    gscale = max(1.0, float(np.max(np.abs(ref.grad.astype(np.float64)))))
    for t in range(d):
        lp = [v * mpmath.exp(h) if k == t else v for k, v in enumerate(lsm)]
        lm = [v * mpmath.exp(-h) if k == t else v for k, v in enumerate(lsm)]
        gt = (lml(lp) - lml(lm)) / (2 * h)
        assert abs(float(ref.grad[t] - LD(mpmath.nstr(gt, 30)))) <= 100 * tol * gscale, (t, float(ref.grad[t]), gt)
    P = a * a.T - Kinv
    gc = sum(P[i, j] for i in range(N) for j in range(N)) * mpmath.mpf(const) / 2
    gn = sum(P[i, i] for i in range(N)) * mpmath.mpf(noise) / 2
    assert abs(float(ref.grad[d] - LD(mpmath.nstr(gc, 30)))) <= tol * gscale
    assert abs(float(ref.grad[d + 1] - LD(mpmath.nstr(gn, 30)))) <= tol * gscale


# ---- the oracle inside the bound ------------------------------------------------------------------------------------------
def _oracle(p):
    K = MR.kernel_matrix(p.X, p.theta, p.spec, p.jitter)
    L = cholesky(K, lower=True, check_finite=False)
    W = solve_triangular(L, np.eye(len(p.y)), lower=True)
    a = cho_solve((L, True), p.y)
    lml = -0.5 * p.y @ a - np.log(np.diag(L)).sum() - len(p.y) / 2 * np.log(2 * np.pi)
    return dict(K=K, L=L, W=W, alpha=a, Kinv=W.T @ W, lml=lml)


def _ratios(p, ref, out, grad=None):
    r = {"K": FR.ratio(FR.err_ld(out["K"], ref.K), ref.dK).max()}
    R, B = FR.chol_residual(p, out["L"], np.arange(ref.N))
    r["L_res"] = FR.ratio(R, B).max()
    aW, aL = np.abs(out["W"]), np.abs(out["L"])
    r["W"] = FR.ratio(FR.err_ld(out["W"], FR.tri_inv_ld(out["L"])), FR.g(ref.N) * (aW @ (aL @ aW))).max()
    r["alpha"] = FR.ratio(FR.err_ld(out["alpha"], ref.alpha), ref.d_alpha).max()
    r["lml"] = float(FR.ratio(FR.err_ld(out["lml"], ref.lml), ref.d_lml))
    tri = np.tril_indices(ref.N)
    r["Kinv"] = FR.ratio(FR.err_ld(out["Kinv"][tri], ref.Kinv[tri]), ref.d_Kinv[tri]).max()
    if grad is not None:
        r["grad"] = FR.ratio(FR.err_ld(grad, ref.grad), ref.d_grad).max()
    return r


def test_oracle_inside_the_bound(sweep):
    worst = {}
    for c, p, ref in sweep:
        out = _oracle(p)
        grad = None
        if not c.general_nu:        # (the oracle's general-nu gradient is sklearn's forward difference)
            spec = O.KernelSpec(O.RBF, np.inf, c.const, c.noise) if np.isinf(c.nu) else p.spec
            grad = O.lml_and_grad(p.X, p.y, p.theta, spec, p.jitter)[1]
        r = _ratios(p, ref, out, grad)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert max(r.values()) <= 1.0, (c.name, r)
    print("\noracle: largest err/bound " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


# ---- a numpy restatement of the device's algorithm, with injectable bugs ------------------------------------------------
NB = 64


def device_sim(p, bug=None):
    """(K, L, W, alpha, K^-1, lml) and the gradient the way csrc/k_fit.hip computes them, in float64"""
    X = np.asarray(p.X, dtype=np.float64)
    N, d = X.shape
    ls, const, noise = p.hyper
    Np = FC.rup(N, NB)
    nblk = Np // NB
    xs = X / ls
    if bug == "kmat_ls_stride8":
        xs[:, 8:] = X[:, 8:] / ls[:d - 8]
    df = xs[:, None, :] - xs[None, :, :]
    if bug == "kmat_r2_first8":
        df = df[:, :, :8]
    k = H._base64(np.sum(df * df, axis=2), p.spec) + (const if p.spec.has_const else 0.0)
    if bug == "jitter_offdiag":
        k = k + p.jitter
    np.fill_diagonal(k, 1.0 + const + noise + p.jitter)
    A = np.eye(Np)
    A[:N, :N] = k

    def blk(i):
        return slice(i * NB, (i + 1) * NB)

    # blocked right-looking Cholesky: 64-wide steps inside a panel of 4 blocks, one update beyond it per panel
    Dinv = np.zeros((nblk, NB, NB))
    for jb0 in range(0, nblk, 4):
        jb1 = min(nblk, jb0 + 4)
        for jb in range(jb0, jb1):
            L11 = cholesky(A[blk(jb), blk(jb)], lower=True)
            A[blk(jb), blk(jb)] = L11
            Dinv[jb] = solve_triangular(L11, np.eye(NB), lower=True)
            for ti in range(jb + 1, nblk):
                A[blk(ti), blk(jb)] = A[blk(ti), blk(jb)] @ Dinv[jb].T
            for ti in range(jb + 1, nblk):
                for tj in range(jb + 1, min(jb1, ti + 1)):
                    if bug == "skip_panel_tile" and (ti, tj, jb) == (jb1 - 1, jb1 - 1, jb0):
                        continue
                    A[blk(ti), blk(tj)] -= A[blk(ti), blk(jb)] @ A[blk(tj), blk(jb)].T
        pan = slice(jb0 * NB, jb1 * NB)
        for ti in range(jb1, nblk):
            for tj in range(jb1, ti + 1):
                if bug == "skip_edge_tile" and (ti, tj, jb0) == (nblk - 1, jb1, 0):
                    continue
                A[blk(ti), blk(tj)] -= A[blk(ti), pan] @ A[blk(tj), pan].T
    L = np.tril(A)
    # W = L^-1: the inverted diagonal blocks, then bottom-up merges W21 = -W22 (L21 W11), ragged pair last
    W = np.zeros((Np, Np))
    for jb in range(nblk):
        W[blk(jb), blk(jb)] = Dinv[jb + 1 if (bug == "dinv_next" and jb == 0) else jb]
    b = NB
    while b < Np:
        nfull = Np // (2 * b)
        rem = Np - nfull * 2 * b
        pairs = [(2 * b * t, b) for t in range(nfull)]
        if rem > b and bug != "ragged_unmerged":
            pairs.append((nfull * 2 * b, rem - b))
        for p0, b2 in pairs:
            r1, r2 = slice(p0, p0 + b), slice(p0 + b, p0 + b + b2)
            W[r2, r1] = -W[r2, r2] @ (L[r2, r1] @ W[r1, r1])
        b *= 2
    y = np.zeros(Np)
    y[:N] = p.y
    Wv = W.copy()
    if bug == "gemv_drop_last":
        Wv[:, (nblk - 1) * NB:] = 0.0
    alpha = W.T @ (Wv @ y)
    lml = -0.5 * y[:N] @ alpha[:N] - np.sum(np.log(np.diag(L)[:N])) - N / 2 * math.log(2 * math.pi)
    Kinv = W.T @ W
    out = dict(K=k, L=L[:N, :N], W=W[:N, :N], alpha=alpha[:N], Kinv=Kinv[:N, :N], lml=lml)
    # the gradient by (16-row group, 256-column block) pairs on and under the diagonal
    nth = d + int(p.spec.has_const) + int(p.spec.has_noise)
    grad = np.zeros(nth)
    ngroups = -(-N // 16)
    drop = {"grad_pair_row": (ngroups - 1, 0), "grad_pair_col": (ngroups - 1, (ngroups - 1) // 16)}.get(bug)
    a, Ki = alpha[:N], Kinv[:N, :N]
    for gy in range(ngroups):
        for bx in range(gy // 16 + 1):
            if (gy, bx) == drop or (bug == "grad_last_group" and gy == ngroups - 1):
                continue
            jj, ll = np.meshgrid(np.arange(16 * gy, min(N, 16 * gy + 16)), np.arange(256 * bx, min(N, 256 * bx + 256)),
                                 indexing="ij")
            m = ll <= jj
            jj, ll = jj[m], ll[m]
            w = np.where(ll < jj, 2.0, 2.0 if bug == "grad_diag2" else 1.0) * (a[jj] * a[ll] - Ki[jj, ll])
            D = (X[jj] - X[ll]) ** 2 / ls ** 2
            f = FR._f64(D.sum(axis=1), p.spec)
            grad[:d] += 0.5 * np.sum((w * f)[:, None] * D, axis=0)
            if p.spec.has_const and not (bug == "grad_const_group" and gy == 0):
                grad[d] += 0.5 * np.sum(w) * const
            if p.spec.has_noise:
                grad[-1] += 0.5 * np.sum(w[jj == ll]) * noise
    if bug == "grad_wide_dropped":
        grad[8:d] = 0.0
    if bug == "grad_last_dropped":
        grad[d - 1] = 0.0
    if bug == "grad_wide_swapped":
        grad[[7, 8]] = grad[[8, 7]]
    return out, grad


BUGS = {   # injected bug -> the shapes it applies to
    "skip_panel_tile": lambda c: FC.rup(c.N, NB) // NB >= 2,        # last tile row of a panel, its own update
    "skip_edge_tile": lambda c: FC.rup(c.N, NB) // NB > 4,          # the trailing tile at the padding edge
    "dinv_next": lambda c: FC.rup(c.N, NB) // NB >= 2,              # diagonal block 0 given Dinv of block 1
    "ragged_unmerged": lambda c: FC.ragged_merges(c.N) > 0,         # Np = 320, 448
    "gemv_drop_last": lambda c: True,                               # the last (partial) 64-block of W in W y
    "grad_diag2": lambda c: c.noise or c.const,                     # the diagonal weighted 2 (D = 0 there otherwise)
    "grad_pair_row": lambda c: True,                                # (last row group, first column block) dropped
    "grad_pair_col": lambda c: c.N > 256,                           # (last row group, last column block) dropped
    "grad_last_group": lambda c: c.N % 16 != 0,                     # the last partial 16-row group dropped
    "grad_const_group": lambda c: c.const,                          # the constant's term of row group 0 dropped
    "jitter_offdiag": lambda c: True,                               # the jitter added off the diagonal too
    # 16-wide instances (d > 8)
    "kmat_r2_first8": lambda c: c.d > 8,                            # r^2 of the kernel matrix over coordinates 0..7
    "kmat_ls_stride8": lambda c: c.d > 8,                           # coordinate j >= 8 scaled by ls[j - 8]
    "grad_wide_dropped": lambda c: c.d > 8,                         # the gradient of coordinates 8..d-1 dropped
    "grad_last_dropped": lambda c: c.d > 8,                         # ... of coordinate d - 1 (ls_bounds: at 1e5)
    "grad_wide_swapped": lambda c: c.d > 8,                         # coordinates 7 and 8 in each other's slots
}


def _old_catches(ref, out, grad):
    def rel(a, b):
        b = np.asarray(b, dtype=np.float64)
        return np.max(np.abs(a - b)) / np.max(np.abs(b))
    g = ref.grad.astype(np.float64)
    return (rel(out["L"], ref.L) >= 1e-9 or rel(out["alpha"], ref.alpha) >= 1e-7
            or abs(out["lml"] - float(ref.lml)) > 1e-8 * abs(float(ref.lml))
            or np.max(np.abs(grad - g)) > 1e-6 * max(1.0, np.max(np.abs(g))))


def _old_wide_catches(p, ref, out, grad):
    """test_gpu_wide_d.py's tolerances: K 1e-12 of max|K|, LML 1e-9 |lml|, gradient 1e-7 max(1, max|g|) (1e-6 for a
    general nu)"""
    g = ref.grad.astype(np.float64)
    K = np.asarray(ref.K, dtype=np.float64)
    gtol = 1e-6 if FR.general_nu(p.spec) else 1e-7
    return (np.max(np.abs(out["K"] - K)) >= 1e-12 * np.max(np.abs(K))
            or abs(out["lml"] - float(ref.lml)) >= 1e-9 * abs(float(ref.lml))
            or np.max(np.abs(grad - g)) >= gtol * max(1.0, np.max(np.abs(g))))


def test_distance_factor():
    """kmat_kernel's distance factor: the 8-wide constant for d <= 8, the number of squared differences beyond"""
    assert all(FR.c_x(d) == FR.C_X8 == 8.0 for d in range(1, 9))
    assert [FR.c_x(d) for d in (9, 12, 16)] == [9.0, 12.0, 16.0]


def test_device_restatement_inside_the_bound_and_every_bug_leaves_it(sweep):
    worst = {}
    for c, p, ref in sweep:
        out, grad = device_sim(p)
        r = _ratios(p, ref, out, grad)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert max(r.values()) <= 1.0, (c.name, r)
    print("\nrestatement: largest err/bound " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    for bug, applies in BUGS.items():
        flagged, old, shapes = [], [], []
        for c, p, ref in sweep:
            if not applies(c):
                continue
            shapes.append(c.name)
            try:
                with np.errstate(invalid="ignore", divide="ignore"):
                    out, grad = device_sim(p, bug)
                    r = _ratios(p, ref, out, grad)
            except np.linalg.LinAlgError:
                # a later diagonal block became indefinite: the evaluation fails (info > 0), visible to any test
                flagged.append(c.name)
                old.append(c.name)
                continue
            if not max(r.values()) <= 1.0:
                flagged.append(c.name)
            if (_old_wide_catches(p, ref, out, grad) if c.d > 8 else _old_catches(ref, out, grad)):
                old.append(c.name)
        print(f"{bug}: flagged on {len(flagged)}/{len(shapes)} {flagged}; old tolerances catch {len(old)}/{len(shapes)}"
              + (f"; let through by test_gpu_wide_d.py's: {sorted(set(flagged) - set(old))}"
                 if all(_case(n).d > 8 for n in shapes) else ""))
        assert shapes and flagged, f"{bug} is not flagged on any shape where it applies ({shapes})"
