"""Reference of the second-order Sobol' indices of the emulators (tests only, CPU): the pair rows built
explicitly, their PC means from the extended-precision ``sobol_ref.pc_means`` with its per-element bound, the pair
moments and the indices in ``np.longdouble`` with tolerances built as ``sobol_ref.moment_tolerances`` and
``sobol_ref.indices`` build the first order's, and the closed form of the pair indices of an RBF emulator over a
uniform box.

Definitions (the issue's; the notation is sobol_ref's).  For a pair i < j, AB_ij = A with columns i and j from B and
D_ij = z(AB_ij) - z(A).  Per batch, about the pivot c:
    sumD2 = sum D_ij,   M2 = sum (z(B) - c) D_ij^T,   D2 = sum D_ij D_ij^T
re-centred as M_i and DD_i are, and per feature
    Sc_ijf = s_f^2 c_f^T M_ij c_f / V_f     the closed pair index (Saltelli et al. 2010, the estimator on the pair row)
    S_ijf  = Sc_ijf - S_if - S_jf           the interaction index
    T_ijf  = s_f^2 c_f^T DD_ij c_f / (2 V_f)  the total effect of the pair (Jansen 1999)
standard errors by batch means; the interaction's from the per-batch values of the difference itself.

The distance factor of the pair walk.  csrc/k_sobol.hip (sobol_pair_mean_kernel) forms, for a fixed i and j walking
upward,
    r2_ij = ((pre_i + t^B_i) + t^A_(i+1) + .. + t^A_(j-1) + t^B_j) + suf_j
with pre_i the serial prefix of t^A below i (from the left) and suf_j the serial suffix above j (from the right), the
two sums ``sobol_mean_kernel`` forms.  Counting as the ``c_x_pf(d)`` paragraph of sobol_ref.py counts:
  - every term t_l carries 7 u relative (difference, rounded reciprocal, product: 6 u in the square; the squaring);
  - the terms: the left chain up to and including t^B_j has j + 1 terms, its first term passes through j additions,
    one or two more than the first-order row's prefix of the same term (there the chain ends at i < j); the final
    addition of suf_j is one more: j + 1.  A term of the suffix passes through at most d - 2 - j additions inside it
    and the final one: d - 1 - j.  For j = d - 1 the suffix is the exact 0 (no rounding): j = d - 1 additions.  So at
    most max(j + 1, d - 1 - j) <= d - 1 additions for j <= d - 2, and d - 1 for j = d - 1 -- as any summation tree of
    d non-negative terms: no term of a d-term sum passes through more than d - 1 additions.  The longer left chain
    moves roundings from the suffix to the prefix; the worst term's count, which is what the first-order bound uses,
    stays d - 1: (7 + d - 1) u = (d + 6) u RELATIVE to r^2, and the padded coordinates add exact zeros;
  - behind the distance the same 6 u (square root, rounded constant and product): (d + 12) u r^2, and against
    |q~|^2 + |x~_j|^2 the factor is that of the first order,
        c_x_pp(d) = c_x_pf(d) = 2 (d + 12).
  - the lanes that take another row's distance (a_i == b_i: row AB_j's; a_j == b_j: row AB_i's; both: row A's) take a
    distance the same factor covers, of the very row they are (AB_ij IS that row there).
Nothing is formed by cancellation, so the near-pair rule of the Matern-0.5 / nu < 1 kernels is met as for the first
order.  The mean's sum is sobol_mean_kernel's (blocks of 16 training rows): ``hp_ref.C_M``.

Tolerances.  The pair moments are the first-order moments with the pair row in the place of AB_i, so
``sobol_ref.moment_tolerances`` applies entry for entry with the row's bound taken over ALL its rows (A, B, the d
first-order rows and the P pair rows).  Feature level, with tol() of sobol_ref.estimates:
    tol(Sc) = (tol(Vc) + |Sc| tol(V)) / (V - tol(V)),   tol(T_ij) likewise,   tol(S_ij) = tol(Sc) + tol(S_i) + tol(S_j)
    standard errors: 1e-9 se + max_t tol_t / sqrt(T - 1)      (sobol_ref.indices' rule)
"""
from __future__ import annotations

import functools
import math

import numpy as np

import sobol_ref as R
from oracle import gp_oracle as O

LD = np.longdouble
MOMENT_KEYS = ("sumA", "sumB", "C2", "sumD", "M", "D")
PAIR_KEYS = ("sumD2", "M2", "D2")


def c_x_pp(d):
    """the distance factor of the pair walk (module docstring): the first order's 2 (d + 12)"""
    return R.c_x_pf(d)


def all_pairs(d):
    return np.array([(i, j) for i in range(d) for j in range(i + 1, d)], dtype=np.int64).reshape(-1, 2)


# ---- cases ---------------------------------------------------------------------------------------------------------------
# the issue's list; pairs None = all i < j.  The models are sobol_ref's where it has the case (the same seeds).
CASES = {
    "rbf_d2": dict(d=2, spec=R._spec(O.RBF), seed=41),
    "rbf_d6": dict(ref="rbf_d6"),
    "rbf_const_d8": dict(ref="rbf_const_d8"),
    "matern05_d6": dict(ref="matern05_d6"),
    "matern15_d6": dict(ref="matern15_d6"),
    "matern25_d9": dict(ref="matern25_d9"),
    "matern_nu12_d5": dict(ref="matern_nu12_d5"),
    "rbf_d16": dict(ref="rbf_d16", pairs=((0, 15), (14, 15), (3, 7), (0, 1), (8, 9))),
    "rbf_d6_k1": dict(ref="rbf_d6_k1"),
}
N_BASE = R.N_BASE
PLANT_ROW, PLANT_TRAIN = 2, 7                 # base row 2: AB_ij ON training point 7, for the case's first pair


def moment_rows(name):
    """rows of the moment / index tests: 257; 129 for d >= 8; 65 at d = 16 (sobol_ref.moment_rows' rule)"""
    d = case(name)[3].shape[1]
    return 65 if d == 16 else 129 if d >= 8 else N_BASE


@functools.lru_cache(maxsize=None)
def case(name):
    """(model, lo, hi, A, B, pairs): sobol_ref's planted rows (rows 0, 1) and one more, row 2: AB_ij lands ON a training
    point for the case's first pair (i, j) while A, AB_i and AB_j do not (A keeps its own columns i and j)"""
    c = CASES[name]
    if "ref" in c:
        model, lo, hi, A, B = R.case(c["ref"])
        A, B = A.copy(), B.copy()
    else:
        model, lo, hi = R.problem(100, c["d"], 40, 3, c["spec"], seed=c["seed"])
        rng = np.random.default_rng(100 + c["seed"])
        A = rng.uniform(lo, hi, (N_BASE, c["d"]))
        B = rng.uniform(lo, hi, (N_BASE, c["d"]))
        R.plant(A, B, model.X_train)
    d = A.shape[1]
    pairs = all_pairs(d) if c.get("pairs") is None else np.array(c["pairs"], dtype=np.int64)
    i, j = pairs[0]
    x = model.X_train[PLANT_TRAIN]
    keep = A[PLANT_ROW, [i, j]].copy()
    A[PLANT_ROW] = x
    A[PLANT_ROW, [i, j]] = keep
    B[PLANT_ROW, [i, j]] = x[[i, j]]
    A.setflags(write=False)
    B.setflags(write=False)
    return model, lo, hi, A, B, pairs


def pair_rows(A, B, pairs):
    """(P, n, d): AB_ij = A with columns i and j from B, built explicitly"""
    X = np.empty((len(pairs),) + A.shape)
    for q, (i, j) in enumerate(pairs):
        X[q] = A
        X[q, :, i] = B[:, i]
        X[q, :, j] = B[:, j]
    return X


def all_rows(A, B, pairs):
    """(d + 2 + P, n, d): sobol_ref.pick_freeze_rows, then the pair rows"""
    return np.concatenate([R.pick_freeze_rows(A, B), pair_rows(A, B, pairs)])


def means(model, A, B, pairs):
    """Z (d + 2 + P, n, k) longdouble and eps (same shape, float64) of all rows of a base pair"""
    X = all_rows(A, B, pairs)
    s, n, d = X.shape
    Z, eps = R.pc_means(model, X.reshape(s * n, d), cx=c_x_pp(d))
    return Z.reshape(s, n, -1), eps.reshape(s, n, -1)


@functools.lru_cache(maxsize=None)
def case_means(name):
    """the reference of a case, computed once; every smaller n is a prefix of its rows"""
    model, lo, hi, A, B, pairs = case(name)
    Z, eps = means(model, A, B, pairs)
    Z.setflags(write=False)
    eps.setflags(write=False)
    return Z, eps


# ---- moments --------------------------------------------------------------------------------------------------------------
def _as_first_order(Z, d):
    """[A, B, pair rows]: the pair rows in the place of the AB_i, so that sobol_ref's moment code serves them"""
    return np.concatenate([Z[:2], Z[2 + d:]])


def moments(Z, d, pivot, T):
    """sobol_ref.moments of the first d + 2 slots and, under sumD2 / M2 / D2, of the pair slots (longdouble)"""
    out = R.moments(Z[:2 + d], pivot, T)
    pm = R.moments(_as_first_order(Z, d), pivot, T)
    out.update(sumD2=pm["sumD"], M2=pm["M"], D2=pm["D"])
    return out


def moment_tolerances(Z, eps, d, pivot, T):
    """entry tolerances of ``moments``: sobol_ref.moment_tolerances with the row's bound over all d + 2 + P rows"""
    e = np.broadcast_to(np.max(np.asarray(eps, dtype=np.float64), axis=0), eps.shape)
    out = R.moment_tolerances(Z[:2 + d], e[:2 + d], pivot, T)
    pt = R.moment_tolerances(_as_first_order(Z, d), _as_first_order(e, d), pivot, T)
    out.update(sumD2=pt["sumD"], M2=pt["M"], D2=pt["D"])
    return out


def _pair_view(m):
    return {"sumA": m["sumA"], "sumB": m["sumB"], "C2": m["C2"], "sumD": m["sumD2"], "M": m["M2"], "D": m["D2"]}


def _one(count, mom, mt, pivot, comp, scale, smean, pairs):
    """(values, tolerances) of closed_pair, interaction, total_pair from one set of summed moments"""
    fo = dict({key: mom[key] for key in MOMENT_KEYS}, pivot=pivot)
    V, Vi, _, _, tV, tVi, _ = R.estimates(count, fo, comp, scale, smean, {key: mt[key] for key in MOMENT_KEYS})
    _, Vc, VTp, _, _, tVc, tVTp = R.estimates(count, dict(_pair_view(mom), pivot=pivot), comp, scale, smean, _pair_view(mt))
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    V64 = f64(V)
    S, Sc, Tp = Vi / V, Vc / V, VTp / V
    tS = (tVi + np.abs(f64(S)) * tV) / (V64 - tV)
    tSc = (tVc + np.abs(f64(Sc)) * tV) / (V64 - tV)
    tTp = (tVTp + np.abs(f64(Tp)) * tV) / (V64 - tV)
    pi, pj = pairs[:, 0], pairs[:, 1]
    val = {"closed_pair": Sc, "interaction": Sc - S[pi] - S[pj], "total_pair": Tp}
    tol = {"closed_pair": tSc, "interaction": tSc + tS[pi] + tS[pj], "total_pair": tTp}
    return val, tol, float(np.max(tV / V64))


def indices(Z, eps, model, pairs, pivot, T):
    """The reference second-order result (longdouble) of Z (d + 2 + P, n, k) and its feature-level tolerances (float64):
    ``(ref, tol)`` with keys closed_pair, interaction, total_pair and their _se; ``tol['cond']`` = max_f tol(V_f) / V_f"""
    k = model.n_pc
    d = Z.shape[0] - 2 - len(pairs)
    comp = np.asarray(model.components[:k], dtype=LD)
    scale = np.asarray(model.scaler_scale, dtype=LD)
    smean = np.asarray(model.scaler_mean, dtype=LD)
    pivot = np.asarray(pivot, dtype=LD)
    mom = moments(Z, d, pivot, T)
    mt = moment_tolerances(Z, eps, d, pivot, T)
    keys = MOMENT_KEYS + PAIR_KEYS
    n = Z.shape[1]
    ref, tol, cond = _one(n, {key: mom[key].sum(axis=0) for key in keys}, {key: mt[key].sum(axis=0) for key in keys},
                          pivot, comp, scale, smean, pairs)
    tol["cond"] = cond
    names = ("closed_pair", "interaction", "total_pair")
    if T > 1:
        per = [_one(int(mom["count"][t]), {key: mom[key][t] for key in keys}, {key: mt[key][t] for key in keys}, pivot,
                    comp, scale, smean, pairs) for t in range(T)]
        for key in names:
            se = np.std(np.array([p[0][key] for p in per]), axis=0, ddof=1) / math.sqrt(T)
            ref[key + "_se"] = se
            tol[key + "_se"] = (1e-9 * np.asarray(se, dtype=np.float64)
                                + np.max(np.array([p[1][key] for p in per]), axis=0) / math.sqrt(T - 1))
    else:
        for key in names:
            ref[key + "_se"] = np.full(ref[key].shape, np.nan)
    return ref, tol


# ---- the closed form of the pair indices of an RBF emulator over a uniform box ----------------------------------------------
def rbf_closed_form_pairs(model, lo, hi, pairs):
    """Exact (V, Vc_ij, VT_ij) per feature of the GP mean of an RBF model (no constant) over the uniform box.  The mean
    is a sum over training points of products of one-dimensional Gaussians, so Var E[y | x_i, x_j] is a double sum over
    training points whose term takes the two-Gaussian overlap integrals for l in {i, j} and the product of the
    one-Gaussian means for the others (the ingredients of ``sobol_ref.rbf_closed_form``); the pair's total effect
    VT_ij = V - Var E[y | x_~ij] follows from the closed index of the complementary set.  V (F,); Vc, VT (P, F)."""
    assert model.spec.kind == O.RBF and not model.spec.has_const
    X = model.X_train
    N, d = X.shape
    k = model.n_pc
    ls = np.stack([gp.ls for gp in model.gps])                        # (k, d)
    al = np.stack([gp.alpha for gp in model.gps])                     # (k, N)
    I1 = R._gauss_mean(X[None, :, :], ls[:, None, :], lo, hi)         # (k, N, d)
    lp2, lq2 = ls[:, None, :] ** 2, ls[None, :, :] ** 2               # (k, k, d)
    sig = np.sqrt(lp2 * lq2 / (lp2 + lq2))
    a, b = X[:, None, :], X[None, :, :]                               # (N, N, d)
    s2 = (lp2 + lq2)[:, :, None, None, :]
    m = (a[None, None] * lq2[:, :, None, None, :] + b[None, None] * lp2[:, :, None, None, :]) / s2
    I2 = np.exp(-(a - b)[None, None] ** 2 / (2 * s2)) * R._gauss_mean(m, sig[:, :, None, None, :], lo, hi)
    I11 = I1[:, None, :, None, :] * I1[None, :, None, :, :]           # (k, k, N, N, d)
    w = al[:, None, :, None] * al[None, :, None, :]
    E = np.einsum("pj,pj->p", al, I1.prod(axis=2))
    EE = np.multiply.outer(E, E)
    C = np.sum(w * I2.prod(axis=4), axis=(2, 3)) - EE
    Vc, VT = np.empty((len(pairs), k, k)), np.empty((len(pairs), k, k))
    for q, (i, j) in enumerate(pairs):
        rest = [l for l in range(d) if l not in (i, j)]
        Vc[q] = np.sum(w * I2[..., i] * I2[..., j] * I11[..., rest].prod(axis=4), axis=(2, 3)) - EE
        VT[q] = C - (np.sum(w * I11[..., i] * I11[..., j] * I2[..., rest].prod(axis=4), axis=(2, 3)) - EE)
    comp, sc2 = model.components[:k], model.scaler_scale ** 2
    return R._quad(C, comp, sc2), R._quad(Vc, comp, sc2), R._quad(VT, comp, sc2)
