"""Extended-precision reference of cross-validation at the fitted hyper-parameters (csrc/k_cv.hip), with an
a-priori error bound of the device's algorithm per element (tests only, CPU).  Written in the style of hp_ref.py.

From the float64 inputs the device model holds -- per PC ``L``, ``alpha`` and the jitter as ``gpemu_model_create``
derives it (``L_00^2 - kernel_.diag``), ``y_train``, the fold labels, the components, the scaler and the diagonal of
``cov_unexplained`` -- it recomputes in ``np.longdouble`` (x87 80-bit, unit roundoff 2^-64):

- ``W = L^-1`` by forward substitution and ``A_II = W[:, I]^T W[:, I]`` per fold I;
- the Cholesky factor ``C`` of ``A_II``, ``M = C^-1`` by substitution, ``Sigma = M^T M``;
- ``mean_I = y_I - Sigma alpha_I`` and ``var = max(diag Sigma - jitter, 0)``;
- ``central_value`` and ``variance`` as ``cv_backproject_kernel`` forms them.

Error bound.  ``u = 2^-53``, first order, componentwise: the device's sums retaken in absolute values.  ``C = 64``
(hp_ref.C_M, C_V: the project's constant for one rounded sum, whatever its length) multiplies every rounded sum below.

1. The resident ``W`` (device_trtri_blocked, k_fit.hip).  The device inverts the 16 x 16 diagonal blocks by
   substitution and merges pairs of inverted blocks bottom-up, b = 16, 32 (inside a 64-tile: merge_level), then 64,
   128, ... with a ragged last pair: ``T = L21 W11``, ``W21 = -W22 T``, two rounded products with errors
   ``|E1| <= C u |L21||W11|`` and ``|E2| <= C u |W22||T|``.  Expanded to first order the computed block has the error
       ``dW21 = -dW22 T - W22 L21 dW11 - W22 E1 + E2``.
   The closed form ``C u |W||L||W|`` that hp_ref uses for the same routine does NOT bound this in absolute values:
   ``|W22||L21||W11|`` is one of the three products of ``(|W||L||W|)_21``, but with ``|dW22| <= C u |W22||L22||W22|``
   the inherited ``|dW22||T|`` has five factors.  What keeps the scheme accurate is that the inherited errors enter
   through RESIDUALS: write ``dW11 = W11 Rr11`` (right residual ``Rr = L W^ - I``) and ``dW22 = Rl22 W22`` (left
   residual ``Rl = W^ L - I``); then ``-dW22 T = Rl22 W21`` and ``-W22 L21 dW11 = W21 Rr11``, first order in W again.
   So ``trtri_bound`` carries bounds of both residuals through the device's own partition,
       base:   ``Rr = C u |D||X|``,  ``Rl = |X| Rr |D|``             (column substitution: (D + dD_c) x_c = e_c)
       merge:  ``Rr21 = Rr22 |T| + E1 + |L22| E2``,   ``Rl21 = |W22 L21| Rl11 + (|W22| E1 + E2) |L11|``
   (from ``Rr21 = L21 dW11 + L22 dW21`` and ``Rl21 = dW21 L11 + dW22 L21``, where the inherited terms cancel against
   ``L22 W21 = -T`` and ``W21 L11 = -W22 L21``; ``|T|`` and ``|W22 L21|`` are the moduli of the true products), and
   ``|dW| <= min(|W| Rr, Rl |W|)`` elementwise.  The host tests print how far this lies above ``C u |W||L||W|``
   (3.4 to 17 times on the table).
2. ``dA``, the error of ``A_II`` (cv_gather_kernel is exact, the SYRK is one MFMA chain per element).  Because
   ``dW = W Rr`` exactly, ``d(W^T W) = Rr^T A + A Rr`` with the exact ``A = K^-1``: the cancellation inside ``W^T W``
   is kept, which ``|dW_I|^T |W_I|`` would lose (measured: 3 times wider).  The sums start at r0 = min I, below
   which the columns I of W are zero:
       ``dA = C u |W_I|^T |W_I| + |A_I:| Rr_:I + (|A_I:| Rr_:I)^T``.
3. ``E``, the backward error of the blocked Cholesky (device_cholesky_blocked): ``C u |C||C|^T`` for the factor of the
   64-tiles (substitution inside a tile: panel_step) and the rank updates, plus a term the textbook form does not
   have: below a diagonal tile D_s the panel is not solved but MULTIPLIED by the inverted tile,
   ``L_rs = A'_rs Dinv_s^T`` (chol_panel_kernel, potrf + launch_gemm).  With ``|A'_rs| <= |C_rs||D_s|^T`` its error is
   ``|dL_rs| <= |C_rs||D_s|^T (C u |Dinv_s|^T + dDinv_s^T)`` and it leaves the residual ``|dL_rs||D_s|^T`` in block
   (r, s) of ``A - C C^T`` (and its transpose in (s, r)); ``dDinv_s`` is the diagonal tile of item 4's ``dM``.  The project's
   summation constant alone does not cover this term: it is why ``E`` is not the textbook ``C u |C||C|^T``.
4. ``dM``, the forward error of ``M = C^-1``: item 1's ``min(|M| Rr, Rl |M|)`` with ``C`` for ``L``.
5. mean.  ``v = Sigma alpha_I``; the exact inverse of the perturbed matrix moves it by ``Sigma (dA + E) v``; the
   epilogue computes ``u = M alpha_I`` (cv_u_kernel) and ``v = M^T u`` (cv_out_kernel):
       ``du = dM |alpha_I| + C u |M||alpha_I|``,   ``dv = |Sigma| (dA + E) |v| + dM^T |u| + |M|^T du + C u |M|^T |u|``,
   and the final subtraction adds ``u (|y| + |v|)``.
6. var.  ``s_l = sum_j M_jl^2``:  ``ds = diag(|Sigma| (dA + E) |Sigma|) + 2 sum_j |M_jl| dM_jl + C u s_l``; the
   derived jitter adds ``u K_00`` (``K_00 = L_00^2``) and the subtraction ``u |s - jitter|``.  The clip at 0 does not
   widen a bound.  Leave-one-out calls take cv_loo_kernel (``1 / sum_r W_ri^2``, no factor): the m = 1 instance of
   the same terms covers it.
7. back-projection, counting cv_backproject_kernel's roundings: a chain of k fmas, then one fma / two products:
       ``d cv  = (mean_bound |S|) |scale| + (k + 2) u (|mean| |S| |scale| + |scaler_mean|)``
       ``d var = ((var_bound S^2) + (2 k + 3) u (var S^2 + cov_unexplained_ff)) scale^2``.

The bound is first order.  Per (PC, fold) problem the module checks ``||Sigma||_inf ||dA + E||_inf <= 0.01`` and raises
``NotFirstOrder`` otherwise: such a problem is not a case of the table (tests/cv_cases.py).
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from hp_ref import C_M, LD, U, _chol_ld

C = C_M                      # = hp_ref.C_V: one rounded sum of the device
FIRST_ORDER_LIMIT = 0.01     # ||Sigma||_inf ||dA + E||_inf above this: the first-order bound is not trusted


class NotFirstOrder(ValueError):
    """a (PC, fold) problem whose perturbation is too large for a first-order bound"""


@dataclass(frozen=True, eq=False)
class Problem:
    """what the device holds, float64 (hashed by identity: build once per case, see cv_cases.problem)"""
    L: np.ndarray                 # (k, N, N)
    alpha: np.ndarray             # (k, N)
    jitter: np.ndarray            # (k,)  as the device derives it
    y: np.ndarray                 # (N, k)
    fold: np.ndarray              # (N,) labels 0 .. n_folds - 1
    components: np.ndarray        # (k, F)
    scaler_mean: np.ndarray       # (F,)
    scaler_scale: np.ndarray      # (F,)
    cov_unexpl_diag: np.ndarray   # (F,)

    @property
    def folds(self):
        return [np.flatnonzero(self.fold == f) for f in range(int(self.fold.max()) + 1)]


def device_jitter(gp, spec):
    """L_00^2 - kernel_.diag as gpemu_model_create forms it: kdiag = 1 (+ const) (+ noise) summed in float64 in that
    order, then one fma (here: the extended difference rounded once)"""
    kd = 1.0
    if spec.has_const:
        kd += float(gp.const)
    if spec.has_noise:
        kd += float(gp.noise)
    return float(LD(gp.L[0, 0]) * LD(gp.L[0, 0]) - LD(kd))


def problem_of_model(model, y, fold, cov_unexpl):
    k = model.n_pc
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    return Problem(L=f64(np.stack([gp.L for gp in model.gps])), alpha=f64(np.stack([gp.alpha for gp in model.gps])),
                   jitter=np.array([device_jitter(gp, model.spec) for gp in model.gps]), y=f64(y),
                   fold=np.asarray(fold, dtype=np.int64), components=f64(model.components[:k]),
                   scaler_mean=f64(model.scaler_mean), scaler_scale=f64(model.scaler_scale),
                   cov_unexpl_diag=f64(np.diag(cov_unexpl)))


# ---- extended-precision pieces ---------------------------------------------------------------------------------------
def tri_inverse_ld(L):
    """L^-1 in longdouble by forward substitution, row by row (L lower, any float type)"""
    L = np.asarray(L, dtype=LD)
    n = L.shape[0]
    W = np.zeros((n, n), dtype=LD)
    for i in range(n):
        W[i, :i] = -(L[i, :i] @ W[:i, :i]) / L[i, i]
        W[i, i] = LD(1) / L[i, i]
    return W


def trtri_bound(L, W):
    """item 1 of the module docstring: (dW, Rr), the first-order bounds of the error and of the right residual of
    device_trtri_blocked's W = L^-1, from L and W (float64, lower), over the device's own partition (16-blocks merged
    pairwise, ragged last pair)"""
    n = L.shape[0]
    aL, aW = np.abs(L), np.abs(W)
    Rr, Rl = np.zeros((n, n)), np.zeros((n, n))
    for p in range(0, n, 16):
        s = slice(p, min(p + 16, n))
        Rr[s, s] = C * U * (aL[s, s] @ aW[s, s])
        Rl[s, s] = aW[s, s] @ Rr[s, s] @ aL[s, s]
    b = 16
    while b < n:
        for p0 in range(0, n, 2 * b):
            mid, end = p0 + b, min(p0 + 2 * b, n)
            if mid >= n:
                continue
            one, two = slice(p0, mid), slice(mid, end)
            aT = np.abs(L[two, one] @ W[one, one])
            E1 = C * U * (aL[two, one] @ aW[one, one])
            E2 = C * U * (aW[two, two] @ aT)
            Rr[two, one] = Rr[two, two] @ aT + E1 + aL[two, two] @ E2
            Rl[two, one] = np.abs(W[two, two] @ L[two, one]) @ Rl[one, one] + (aW[two, two] @ E1 + E2) @ aL[one, one]
        b *= 2
    return np.minimum(aW @ Rr, Rl @ aW), Rr


def chol_backward_bound(aC, aM, dM):
    """item 3: |A - C C^T| of device_cholesky_blocked from |C|, |M| = |C^-1| and dM (float64)"""
    m = aC.shape[0]
    E = C * U * (aC @ aC.T)
    for s0 in range(0, m - 64, 64):
        s, below = slice(s0, s0 + 64), slice(s0 + 64, m)
        Dt, Dit = aC[s, s].T, aM[s, s].T
        blk = aC[below, s] @ (Dt @ (C * U * Dit + dM[s, s].T) @ Dt)
        E[below, s] += blk
        E[s, below] += blk.T
    return E


@dataclass
class FoldTerms:
    """one (PC, fold) problem: the extended results and the float64 bounds; what the host tests look into"""
    I: np.ndarray
    mean: np.ndarray
    s: np.ndarray                 # diag Sigma
    Sigma: np.ndarray             # float64
    mean_bound: np.ndarray
    s_bound: np.ndarray
    first_order: float


def fold_terms(W, aW, aA, Rr, alpha, y, I):
    """items 2 - 6 for one fold I (ascending) of one PC; W longdouble, the rest as pc_terms returns it"""
    r0 = int(I[0])
    WI = W[r0:, I]
    A = WI.T @ WI
    Cf = _chol_ld(A)
    M = tri_inverse_ld(Cf)
    Sig = M.T @ M
    al = alpha[I].astype(LD)
    v = Sig @ al
    mean = y[I].astype(LD) - v
    s = np.sum(M * M, axis=0)
    aWI = aW[r0:, I]
    prop = aA[I] @ Rr[:, I]
    dA = C * U * (aWI.T @ aWI) + prop + prop.T
    C64, M64 = Cf.astype(np.float64), M.astype(np.float64)
    aC, aM = np.abs(C64), np.abs(M64)
    dM, _ = trtri_bound(C64, M64)
    dAE = dA + chol_backward_bound(aC, aM, dM)
    aS = np.abs(Sig.astype(np.float64))
    first_order = float(np.max(aS.sum(axis=1)) * np.max(dAE.sum(axis=1)))
    aal, av = np.abs(alpha[I]), np.abs(v.astype(np.float64))
    au = aM @ aal                                     # >= |u|
    du = dM @ aal + C * U * au
    dv = aS @ (dAE @ av) + dM.T @ au + aM.T @ du + C * U * (aM.T @ au)
    mean_bound = dv + U * (np.abs(y[I]) + av)
    s64 = s.astype(np.float64)
    s_bound = np.sum((aS @ dAE) * aS, axis=1) + 2 * np.sum(aM * dM, axis=0) + C * U * s64
    return FoldTerms(I=I, mean=mean, s=s, Sigma=Sig.astype(np.float64), mean_bound=mean_bound, s_bound=s_bound,
                     first_order=first_order)


@dataclass
class Reference:
    mean_pc: np.ndarray           # (N, k) longdouble
    var_pc: np.ndarray            # (N, k) longdouble, clipped at 0
    var_raw: np.ndarray           # (N, k) longdouble, diag Sigma - jitter before the clip
    central_value: np.ndarray     # (N, F) longdouble
    variance: np.ndarray          # (N, F) longdouble
    mean_bound: np.ndarray        # float64, shapes as above
    var_bound: np.ndarray
    cv_bound: np.ndarray
    variance_bound: np.ndarray
    first_order: float            # the largest ||Sigma|| ||dA + E|| of the problems
    dW_over_closed_form: float    # max of item 1's recursion over C u |W||L||W| (reported by the host tests)

    def outputs(self):
        """(name, reference, bound) of the four outputs, in DeviceModel.cross_validate's order"""
        return [("mean_pc", self.mean_pc, self.mean_bound), ("var_pc", self.var_pc, self.var_bound),
                ("central_value", self.central_value, self.cv_bound), ("variance", self.variance, self.variance_bound)]


def back_project(p: Problem, mean, var, mean_bound, var_bound):
    """item 7: (central_value, variance) longdouble and their bounds"""
    k = p.components.shape[0]
    S, sc, sm = p.components.astype(LD), p.scaler_scale.astype(LD), p.scaler_mean.astype(LD)
    cv = (mean @ S) * sc + sm
    vo = (var @ (S * S) + p.cov_unexpl_diag.astype(LD)) * (sc * sc)
    aS, asc = np.abs(p.components), np.abs(p.scaler_scale)
    cvb = (mean_bound @ aS) * asc + (k + 2) * U * ((np.abs(mean.astype(np.float64)) @ aS) * asc + np.abs(p.scaler_mean))
    vob = ((var_bound @ aS ** 2) + (2 * k + 3) * U * (var.astype(np.float64) @ aS ** 2 + np.abs(p.cov_unexpl_diag))) \
        * asc ** 2
    return cv, vo, cvb, vob


def pc_terms(p: Problem, pc):
    """(W longdouble, |W|, |A| = |W^T W|, Rr, max of dW over the closed form C u |W||L||W|) of one PC"""
    W = tri_inverse_ld(p.L[pc])
    L64, W64 = np.tril(p.L[pc]), W.astype(np.float64)
    aW, aL = np.abs(W64), np.abs(L64)
    dW, Rr = trtri_bound(L64, W64)
    closed = C * U * (aW @ aL @ aW)
    low = np.tril(np.ones_like(dW, dtype=bool))
    return W, aW, np.abs(W64.T @ W64), Rr, float(np.max(dW[low] / closed[low]))


@lru_cache(maxsize=None)
def reference(p: Problem, check=True) -> Reference:
    """the reference of a whole call; check: raise NotFirstOrder where the first-order condition fails (else the
    figure is only recorded: cv_cases' admission test)"""
    N, k = p.y.shape
    mean = np.empty((N, k), dtype=LD)
    raw = np.empty((N, k), dtype=LD)
    mb, vb = np.empty((N, k)), np.empty((N, k))
    worst, ratio = 0.0, 0.0
    for pc in range(k):
        W, aW, aA, Rr, r = pc_terms(p, pc)
        ratio = max(ratio, r)
        K00 = p.L[pc, 0, 0] ** 2
        for I in p.folds:
            t = fold_terms(W, aW, aA, Rr, p.alpha[pc], p.y[:, pc], I)
            worst = max(worst, t.first_order)
            if check and not t.first_order <= FIRST_ORDER_LIMIT:
                raise NotFirstOrder(f"PC {pc}, fold of {len(I)} from {I[0]}: ||Sigma|| ||dA|| = {t.first_order:.3e}")
            mean[I, pc], mb[I, pc] = t.mean, t.mean_bound
            raw[I, pc] = t.s - LD(p.jitter[pc])
            vb[I, pc] = t.s_bound + U * K00 + U * np.abs(raw[I, pc].astype(np.float64))
    var = np.where(raw < 0, LD(0), raw)
    cv, vo, cvb, vob = back_project(p, mean, var, mb, vb)
    return Reference(mean_pc=mean, var_pc=var, var_raw=raw, central_value=cv, variance=vo, mean_bound=mb, var_bound=vb,
                     cv_bound=cvb, variance_bound=vob, first_order=worst, dW_over_closed_form=ratio)


def err_over_bound(got, ref, bound):
    """max |got - ref| / bound over the elements (longdouble difference; a zero bound with a zero error counts 0)"""
    err = np.abs(np.asarray(got, dtype=LD) - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(q))


def ratios(out, ref: Reference):
    """{output: max err / bound} of (mean_pc, var_pc, central_value, variance) as DeviceModel.cross_validate returns them"""
    return {name: err_over_bound(got, r, b) for got, (name, r, b) in zip(out, ref.outputs())}


def violations(out, ref: Reference):
    """what both test modules assert to be empty: every element of the four outputs within its bound of the reference,
    none NaN, no variance negative"""
    bad = []
    for got, (name, r, b) in zip(out, ref.outputs()):
        got = np.asarray(got)
        if np.isnan(got).any():
            bad.append(f"{name}: NaN at {np.argwhere(np.isnan(got))[:3].tolist()}")
            continue
        err = np.abs(got.astype(LD) - r).astype(np.float64)
        over = err > b
        if over.any():
            w = np.unravel_index(np.argmax(np.where(over, err / np.maximum(b, 1e-300), 0.0)), err.shape)
            bad.append(f"{name}: {int(over.sum())} of {over.size} outside the bound, worst at {tuple(int(i) for i in w)}: "
                       f"err {err[w]:.3e}, bound {b[w]:.3e}")
        if name in ("var_pc", "variance") and (got < 0).any():
            bad.append(f"{name}: negative at {np.argwhere(got < 0)[:3].tolist()}")
    return bad
