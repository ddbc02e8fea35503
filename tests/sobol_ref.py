"""Reference of the global (Sobol') sensitivity of the emulators (tests only, CPU): the pick-freeze PC means of
tests/hp_ref.py in ``np.longdouble`` with their per-row bounds, the moments and the estimators of
``gpemu/sensitivity.py`` restated in longdouble with error-bounded tolerances, and the closed form of the indices of an
RBF emulator over a uniform box.

Definitions (the issue's): base matrices A, B (n, d); AB_i = A with column i from B; row r in batch floor(r T / n).
With z the PC means, z0 their mean over the 2 n rows of A and B, D_i = z(AB_i) - z(A):
    C = mean (z - z0)(z - z0)^T,  M_i = 1/n sum (z(B) - z0) D_i^T,  DD_i = 1/n sum D_i D_i^T,
    V_f = s_f^2 c_f^T C c_f,  S_if = s_f^2 c_f^T M_i c_f / V_f,  T_if = s_f^2 c_f^T DD_i c_f / (2 V_f),
    mean_f = s_f c_f^T z0 + m_f;  standard errors: batch means (each batch about its own centre), ddof 1, / sqrt(T).

The distance factor of the device's form.  ``hp_ref.kstar`` bounds the error of r^2 by ``cx u (|q~|^2 + |x~_j|^2)``.
The pick-freeze kernel (csrc/k_sobol.hip) forms every distance as a sum of non-negative terms, per coordinate
``t_l = fl(fl(fl(q_l - x_l) fl(1 / ls_l))^2)``:
  - the difference, the rounded reciprocal and their product: 3 roundings of the scaled difference, 6 u relative in
    its square, and the squaring itself: 7 u relative in t_l;
  - r2_A, r2_B are serial sums of the d terms; r2_i = (prefix_i + t^B_i) + suffix_i: every term passes through at most
    d - 1 additions.  First order (Higham, Accuracy and Stability, ch. 3): (7 + d - 1) u = (d + 6) u RELATIVE to r^2;
  - behind the distance and in front of the exponential: the square root (u in r, 2 u in r^2), the rounded constant
    sqrt(3) or sqrt(5) and its product (2 u in r, 4 u in r^2), or the halving (exact) for the RBF kernel: at most
    6 u relative to r^2.  These move the kernel's ARGUMENT, which ``EPS_EXP |k|`` does not cover where the argument is
    large, so they are counted with the distance: (d + 12) u r^2 in all;
  - r^2 = |q~ - x~|^2 <= 2 (|q~|^2 + |x~|^2) for any centre, so measured against ``|q~|^2 + |x~_j|^2`` the factor is
        c_x_pf(d) = 2 (d + 12).
There is no cancellation anywhere in this form, so its absolute error vanishes with r^2: the near-pair rule of the
Matern-0.5 / nu < 1 kernels (``hp_ref.kstar``: the direct-distance bound for ``r2 < 2e-7 (|q~|^2 + 1)``) is met by the
same factor (delta_r = delta_r2 / 2 r <= (d + 12) u r / 2 <= (d + 12) / 2 u sum_l (|q_l| + |x_l|) / ls_l).
The mean's sum runs in blocks of 16 training rows, the block sums in order: depth 16 + N / 16, within ``hp_ref.C_M`` = 64
for N <= 768 in the worst case (and far beyond it in the mean).

Tolerances (same sums in absolute values, at the PC level, so that they hold whether the device back-projects rows or
moments).  With b = z(B) - c, D = D_i, eps the row's bound (the largest of its d + 2 rows' ``mean_bound``, per PC):
    moment entry  sum_r (2 eps_p |D_q| + 2 |b_p| eps_q + 4 eps_p eps_q) + 64 u sum_r |b_p| |D_q|   (C2, D alike; sums:
                  sum_r 2 eps_p + 64 u sum_r |b_p|)
    feature level through |c_pf| |c_qf| s_f^2, with the re-centring's terms; tol(S) = (tol(V_i) + |S| tol(V)) /
                  (V - tol(V)), likewise T;  tol(mean) = pp_ref.tolerances' mean rule with 2 n rows.
"""
from __future__ import annotations

import functools
import math

import numpy as np
from scipy.special import erf

import hp_ref as H
import pp_ref as P
from oracle import gp_oracle as O

LD = np.longdouble
U = H.U


def c_x_pf(d):
    """the distance factor of the pick-freeze kernel's form (module docstring): 2 (d + 12)"""
    return 2.0 * (d + 12)


# ---- problems and cases ---------------------------------------------------------------------------------------------
def problem(N, d, F, k, spec, seed=0):
    """pp_ref.problem with PER-PC length scales (every PC its own theta: an indexing error between PCs shows):
    (GroupModel, lo, hi)"""
    rng = np.random.default_rng(seed)
    lo = -1.0 - rng.uniform(0.0, 1.0, d)
    hi = 1.0 + rng.uniform(0.0, 1.0, d)
    X = rng.uniform(lo, hi, (N, d))
    Wm = rng.normal(size=(d, F))
    Y = np.sin(X @ Wm) + 0.1 * (X ** 2) @ np.abs(Wm) + 0.01 * rng.normal(size=(N, F))
    mean, scale, _ = O.scaler_fit(Y)
    pca = O.pca_fit((Y - mean) / scale)
    gps = []
    with P.oracle_for(spec):
        for i in range(k):
            ls = (hi - lo) * (0.4 + 0.1 * ((np.arange(d) + 2 * i) % d) / d) * (1.0 + 0.35 * i)
            theta = np.log(np.r_[ls, [0.7 + 0.1 * i] if spec.has_const else [], [0.03] if spec.has_noise else []])
            gps.append(O.gp_fit_at_theta(X, pca["Y_pca"][:, i], theta, spec, 1e-10))
    model = O.GroupModel(X_train=X, spec=spec, gps=gps, components=pca["components"],
                         explained_variance=pca["explained_variance"], scaler_mean=mean, scaler_scale=scale, n_pc=k)
    return model, lo, hi


def _spec(kind, nu=np.inf, const=False):
    return O.KernelSpec(kind=kind, nu=nu, has_const=const, has_noise=True)


CASES = {
    "rbf_d6": dict(d=6, spec=_spec(O.RBF)),
    "rbf_const_d8": dict(d=8, spec=_spec(O.RBF, const=True)),
    "matern05_d6": dict(d=6, spec=_spec(O.MATERN, 0.5)),
    "matern15_d6": dict(d=6, spec=_spec(O.MATERN, 1.5)),
    "matern25_d9": dict(d=9, spec=_spec(O.MATERN, 2.5)),
    "matern_nu12_d5": dict(d=5, spec=_spec(O.MATERN, 1.2)),
    "rbf_d16": dict(d=16, spec=_spec(O.RBF)),
    "rbf_d1": dict(d=1, spec=_spec(O.RBF), N=37, F=12, k=2),
    "rbf_d6_k1": dict(d=6, spec=_spec(O.RBF), k=1),
}
N_BASE = 257


def moment_rows(case):
    """rows of the moment / index tests: 257; 129 for d >= 8; 65 at d = 16"""
    d = CASES[case]["d"]
    return 65 if d == 16 else 129 if d >= 8 else N_BASE


def plant(A, B, X_train):
    """A[0] on a training point; AB_c row 1 ON a training point while A row 1 is not (c = min(2, d - 1))"""
    d = A.shape[1]
    A[0] = X_train[3]
    if A.shape[0] >= 2:
        c = min(2, d - 1)
        keep = A[1, c]
        A[1] = X_train[5]
        A[1, c] = keep
        B[1, c] = X_train[5, c]
    return A, B


@functools.lru_cache(maxsize=None)
def case(name):
    """(model, lo, hi, A, B) of a named case: N_BASE rows in the box with the planted rows"""
    c = CASES[name]
    model, lo, hi = problem(c.get("N", 100), c["d"], c.get("F", 40), c.get("k", 3), c["spec"],
                            seed=sorted(CASES).index(name))
    rng = np.random.default_rng(100 + sorted(CASES).index(name))
    A = rng.uniform(lo, hi, (N_BASE, c["d"]))
    B = rng.uniform(lo, hi, (N_BASE, c["d"]))
    plant(A, B, model.X_train)
    return model, lo, hi, A, B


def pick_freeze_rows(A, B):
    """(d + 2, n, d): A, B, AB_0 .. AB_(d-1)"""
    n, d = A.shape
    X = np.empty((d + 2, n, d))
    X[0], X[1] = A, B
    for i in range(d):
        X[2 + i] = A
        X[2 + i, :, i] = B[:, i]
    return X


def pc_means(model, X, cx=None):
    """hp_ref's longdouble PC means of the rows of X and their bounds ``mean_bound`` (the mean's part of
    ``hp_ref.PCRef``, without the variance's forward substitution): (mean [B, k] longdouble, bound [B, k] float64)"""
    X = np.asarray(X, dtype=np.float64)
    means, bounds = [], []
    with P.oracle_for(model.spec):
        for gp in model.gps:
            K, dk = H.kstar(X, model.X_train, gp, model.spec, cx)
            k64 = np.abs(np.asarray(K, dtype=np.float64))
            means.append(K @ np.asarray(gp.alpha, dtype=LD))
            bounds.append(H.C_M * U * (k64 @ np.abs(gp.alpha)) + dk @ np.abs(gp.alpha))
    return np.stack(means, axis=1), np.stack(bounds, axis=1)


@functools.lru_cache(maxsize=None)
def case_means(name):
    """the reference of a case, computed once: Z (d + 2, N_BASE, k) longdouble and eps (d + 2, N_BASE, k); every
    smaller n is a prefix of its rows"""
    model, lo, hi, A, B = case(name)
    X = pick_freeze_rows(A, B)
    s, n, d = X.shape
    Z, eps = pc_means(model, X.reshape(s * n, d), cx=c_x_pf(d))
    Z.setflags(write=False)
    eps.setflags(write=False)
    return Z.reshape(s, n, -1), eps.reshape(s, n, -1)


# ---- moments and estimators in longdouble -------------------------------------------------------------------------------
def batch_of(n, T):
    return (np.arange(n) * T) // n


def moments(Z, pivot, T):
    """the device's moments (include/gpemu.h) of Z (d + 2, n, k) about ``pivot`` per batch, in longdouble"""
    Z = np.asarray(Z, dtype=LD)
    s, n, k = Z.shape
    d = s - 2
    c = np.asarray(pivot, dtype=LD)
    a, b = Z[0] - c, Z[1] - c
    Dl = Z[2:] - Z[0]
    bt = batch_of(n, T)
    out = {"count": np.bincount(bt, minlength=T).astype(np.int64), "sumA": np.zeros((T, k), LD), "sumB": np.zeros((T, k), LD),
           "C2": np.zeros((T, k, k), LD), "sumD": np.zeros((T, d, k), LD), "M": np.zeros((T, d, k, k), LD),
           "D": np.zeros((T, d, k, k), LD), "pivot": c, "n": n, "n_batches": T}
    for t in range(T):
        r = bt == t
        out["sumA"][t], out["sumB"][t] = a[r].sum(axis=0), b[r].sum(axis=0)
        out["C2"][t] = a[r].T @ a[r] + b[r].T @ b[r]
        for i in range(d):
            out["sumD"][t, i] = Dl[i][r].sum(axis=0)
            out["M"][t, i] = b[r].T @ Dl[i][r]
            out["D"][t, i] = Dl[i][r].T @ Dl[i][r]
    return out


def moment_tolerances(Z, eps, pivot, T):
    """the entry tolerances of ``moments`` (module docstring), float64, same keys"""
    Z64 = np.asarray(Z, dtype=np.float64)
    s, n, k = Z64.shape
    d = s - 2
    e = np.max(np.asarray(eps, dtype=np.float64), axis=0)            # the row's bound, per PC
    c = np.asarray(pivot, dtype=np.float64)
    a, b = np.abs(Z64[0] - c), np.abs(Z64[1] - c)
    Dl = np.abs(Z64[2:] - Z64[0])
    bt = batch_of(n, T)

    def prod(u, v, ee):
        return 2 * ee.T @ v + 2 * u.T @ ee + 4 * ee.T @ ee + H.C_M * U * (u.T @ v)

    def vec(u, ee):
        return 2 * ee.sum(axis=0) + H.C_M * U * u.sum(axis=0)

    out = {"sumA": np.zeros((T, k)), "sumB": np.zeros((T, k)), "C2": np.zeros((T, k, k)), "sumD": np.zeros((T, d, k)),
           "M": np.zeros((T, d, k, k)), "D": np.zeros((T, d, k, k))}
    for t in range(T):
        r = bt == t
        er = e[r]
        out["sumA"][t], out["sumB"][t] = vec(a[r], er), vec(b[r], er)
        out["C2"][t] = prod(a[r], a[r], er) + prod(b[r], b[r], er)
        for i in range(d):
            out["sumD"][t, i] = vec(Dl[i][r], er)
            out["M"][t, i] = prod(b[r], Dl[i][r], er)
            out["D"][t, i] = prod(Dl[i][r], Dl[i][r], er)
    return out


def _quad(X, comp, s2):
    return np.einsum("pf,...pq,qf->...f", comp, X, comp) * s2


def estimates(count, mom, comp, scale, smean, tol=None):
    """(V, V_i, VT_i, mean) per feature from summed moments ``mom`` (dict of sumA .. D, pivot) over ``count`` rows, in
    the dtype of the moments; with ``tol`` (the summed entry tolerances) also their tolerances (tV, tVi, tVTi)"""
    n = count
    k = comp.shape[0]
    a = (mom["sumA"] + mom["sumB"]) / (2 * n)
    C = mom["C2"] / (2 * n) - np.multiply.outer(a, a)
    Mi = (mom["M"] - a[None, :, None] * mom["sumD"][:, None, :]) / n
    Di = mom["D"] / n
    s2 = scale * scale
    V, Vi, VTi = _quad(C, comp, s2), _quad(Mi, comp, s2), _quad(Di, comp, s2) / 2
    mean = ((mom["pivot"] + a) @ comp) * scale + smean
    if tol is None:
        return V, Vi, VTi, mean
    f64 = lambda x: np.abs(np.asarray(x, dtype=np.float64))
    ac, as2 = f64(comp), f64(s2)
    ta = (tol["sumA"] + tol["sumB"]) / (2 * n)
    aa = f64(a)
    host = (k * k + 8) * U                                            # the float64 evaluation of the quadratic forms
    tC = (tol["C2"] / (2 * n) + np.multiply.outer(aa, ta) + np.multiply.outer(ta, aa) + np.multiply.outer(ta, ta)
          + host * (f64(mom["C2"]) / (2 * n) + np.multiply.outer(aa, aa)))
    sD = f64(mom["sumD"])
    tM = (tol["M"] + ta[None, :, None] * sD[:, None, :] + aa[None, :, None] * tol["sumD"][:, None, :]
          + ta[None, :, None] * tol["sumD"][:, None, :] + host * (f64(mom["M"]) + aa[None, :, None] * sD[:, None, :])) / n
    tD = (tol["D"] + host * f64(mom["D"])) / n
    return V, Vi, VTi, mean, _quad(tC, ac, as2), _quad(tM, ac, as2), _quad(tD, ac, as2) / 2


def _sum_t(m, keys=("sumA", "sumB", "C2", "sumD", "M", "D")):
    return {key: m[key].sum(axis=0) for key in keys}


def indices(Z, eps, model, pivot, T):
    """The reference result dict (longdouble) of Z (d + 2, n, k) and the feature-level tolerances (float64):
    ``(ref, tol)`` with keys first_order, total, first_order_se, total_se, variance, mean; ``tol['cond']`` =
    max_f tol(V_f) / V_f, the condition every test asserts to be <= 1e-9."""
    k = model.n_pc
    comp = np.asarray(model.components[:k], dtype=LD)
    scale = np.asarray(model.scaler_scale, dtype=LD)
    smean = np.asarray(model.scaler_mean, dtype=LD)
    mom = moments(Z, pivot, T)
    mt = moment_tolerances(Z, eps, pivot, T)
    n = Z.shape[1]
    tot = dict(_sum_t(mom), pivot=mom["pivot"])
    V, Vi, VTi, mean, tV, tVi, tVTi = estimates(n, tot, comp, scale, smean, _sum_t(mt))
    V64 = np.asarray(V, dtype=np.float64)
    S, Tt = Vi / V, VTi / V
    ref = {"first_order": S, "total": Tt, "variance": V, "mean": mean}
    tol = {"variance": tV, "cond": float(np.max(tV / V64)),
           "first_order": (tVi + np.abs(np.asarray(S, dtype=np.float64)) * tV) / (V64 - tV),
           "total": (tVTi + np.abs(np.asarray(Tt, dtype=np.float64)) * tV) / (V64 - tV)}
    # the mean: pp_ref.tolerances' rule with the 2 n rows of A and B
    ZAB = np.concatenate([Z[0], Z[1]])
    mu, _, delta = P.back_project(model, ZAB, np.zeros(ZAB.shape), np.concatenate([eps[0], eps[1]]))
    tol["mean"] = delta.max(axis=0) + 2 * n * U * np.max(np.abs(np.asarray(mu, dtype=np.float64)), axis=0)
    if T > 1:
        Sb, Tb, tSb, tTb = [], [], [], []
        for t in range(T):
            one = {key: mom[key][t] for key in ("sumA", "sumB", "C2", "sumD", "M", "D")}
            one["pivot"] = mom["pivot"]
            v, vi, vti, _, tv, tvi, tvti = estimates(int(mom["count"][t]), one, comp, scale, smean,
                                                     {key: mt[key][t] for key in mt})
            v64 = np.asarray(v, dtype=np.float64)
            Sb.append(vi / v)
            Tb.append(vti / v)
            tSb.append((tvi + np.abs(np.asarray(vi / v, dtype=np.float64)) * tv) / (v64 - tv))
            tTb.append((tvti + np.abs(np.asarray(vti / v, dtype=np.float64)) * tv) / (v64 - tv))
        for key, est, te in (("first_order_se", Sb, tSb), ("total_se", Tb, tTb)):
            se = np.std(np.array(est), axis=0, ddof=1) / math.sqrt(T)
            ref[key] = se
            # |std(x + e) - std(x)| <= std(e) <= sqrt(T / (T - 1)) max|e|, over sqrt(T)
            tol[key] = 1e-9 * np.asarray(se, dtype=np.float64) + np.max(np.array(te), axis=0) / math.sqrt(T - 1)
    else:
        ref["first_order_se"] = np.full(S.shape, np.nan)
        ref["total_se"] = np.full(S.shape, np.nan)
    return ref, tol


# ---- the closed form of an RBF emulator over a uniform box ------------------------------------------------------------
def _gauss_mean(a, ell, lo, hi):
    """1 / (hi - lo) int_lo^hi exp(-(x - a)^2 / (2 ell^2)) dx"""
    s = ell * math.sqrt(2.0)
    return ell * math.sqrt(math.pi / 2.0) * (erf((hi - a) / s) - erf((lo - a) / s)) / (hi - lo)


def rbf_closed_form(model, lo, hi):
    """Exact (V, V_i, VT_i) per feature of the GP mean of an RBF model (no constant) over the uniform box: products of
    erf integrals of one Gaussian (the mean and the conditional means) and of two Gaussians with the two PCs' length
    scales (the second moments).  V (F,), V_i and VT_i (d, F); VT_i is the total-effect variance E Var(y | x_~i)."""
    assert model.spec.kind == O.RBF and not model.spec.has_const
    X = model.X_train
    N, d = X.shape
    k = model.n_pc
    ls = np.stack([gp.ls for gp in model.gps])                        # (k, d)
    al = np.stack([gp.alpha for gp in model.gps])                     # (k, N)
    I1 = _gauss_mean(X[None, :, :], ls[:, None, :], lo, hi)           # (k, N, d)
    lp2, lq2 = ls[:, None, :] ** 2, ls[None, :, :] ** 2               # (k, k, d)
    sig = np.sqrt(lp2 * lq2 / (lp2 + lq2))
    a, b = X[:, None, :], X[None, :, :]                               # (N, N, d)
    m = (a[None, None] * lq2[:, :, None, None, :] + b[None, None] * lp2[:, :, None, None, :]) / (lp2 + lq2)[:, :, None, None, :]
    I2 = (np.exp(-(a - b)[None, None] ** 2 / (2 * (lp2 + lq2)[:, :, None, None, :]))
          * _gauss_mean(m, sig[:, :, None, None, :], lo, hi))         # (k, k, N, N, d)
    I11 = I1[:, None, :, None, :] * I1[None, :, None, :, :]           # (k, k, N, N, d): I1_pjl I1_qj'l
    w = al[:, None, :, None] * al[None, :, None, :]                   # alpha_pj alpha_qj'
    E = np.einsum("pj,pj->p", al, I1.prod(axis=2))
    EE = np.multiply.outer(E, E)
    C = np.sum(w * I2.prod(axis=4), axis=(2, 3)) - EE
    Vi, VTi = np.empty((d, k, k)), np.empty((d, k, k))
    for i in range(d):
        rest = [l for l in range(d) if l != i]
        Vi[i] = np.sum(w * I2[..., i] * I11[..., rest].prod(axis=4), axis=(2, 3)) - EE
        VTi[i] = C - (np.sum(w * I11[..., i] * I2[..., rest].prod(axis=4), axis=(2, 3)) - EE)
    comp, s2 = model.components[:k], model.scaler_scale ** 2
    return _quad(C, comp, s2), _quad(Vi, comp, s2), _quad(VTi, comp, s2)
