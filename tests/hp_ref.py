"""Extended-precision reference of the GP predict and low-rank log-likelihood, with an a-priori error bound of the
device's algorithm per element (tests only, CPU).

From the same float64 inputs the device model is given (``X_train``, ``ls``, ``const``, ``noise``, ``alpha``, ``L``,
the components, the scaler, ``cov_unexplained``, ``y_exp``, ``y_err``, the observable block starts) it recomputes in
``np.longdouble`` (x87 80-bit, unit roundoff 2^-64):

- ``K_*`` (the distance per query / training pair directly from the coordinates);
- the mean ``K_* alpha``;
- ``V = L^-1 K_*^T`` by forward substitution;
- ``var = kdiag - sum V^2``, clipped at 0 as scikit-learn clips it (skl _gpr.py:479-485);
- the block-diagonal low-rank log-likelihood of ``oracle/gp_oracle.py`` (``lowrank_setup_blocks``,
  ``loglik_lowrank_blocks``): per observable block the Woodbury / determinant-lemma form.

The general-nu Matern kernel is the one exception: its Bessel part ``t^nu K_nu(t)`` is scipy's, in float64 (the distance
is still extended).  Its relative error is budgeted in ``EPS_BESSEL`` below, with the device's own.

Error bound.  ``u = 2^-53``.  A running error analysis of the device's algorithm, as the same sums in absolute values:

- cross-kernel entry ``k_j``:  the device forms r^2 by the expanded, centred form ``|q~|^2 + |x~_j|^2 - 2 q~.x~_j``
  (``kstar_host.h``, ``predict_dev.h``), whose absolute error is ``C_X u (|q~|^2 + |x~_j|^2)`` (plus the rounding of
  the inputs, see "Limit" below).  It moves the kernel by
  at most ``|k(r^2 +- delta) - k(r^2)|`` (the kernel is monotone in r).  Pairs the device measures by the direct
  distance (Matern 0.5, nu < 1, ``r^2 < 1e-7 (|q~|^2 + 1)``) have ``delta_r = C_Xd u sum_i (|q_i| + |x_ji|) / ls_i``
  instead.  On top: the evaluation of the kernel, ``EPS_EXP |k|`` (table exponential, closed forms) or
  ``EPS_BESSEL |k|`` (general nu), the exponential's clamp at -700 (closed forms: ``prefactor(t) e^-700`` where the
  argument is below it, ~1e-304), and the constant's addition ``u (|k| + const)``.  Call this ``dk_j``.
- mean:  ``C_M u sum_j |k_j||alpha_j| + sum_j dk_j |alpha_j|``.
- variance:  with ``W = L^-1`` (device: inverted once), ``a = |W||k|`` and ``b = |W||L||W||k|`` (the componentwise error
  of a triangular inverse, Higham, Accuracy and Stability, ch. 8), ``V`` the exact product:
  ``C_V u (kdiag + sum_r V_r^2 + 2 sum_r |V_r| (a_r + b_r)) + 2 sum_r |V_r| (|W| dk)_r``.
  This is the issue's ``c_v u kappa_1(L) (kdiag + sum_r (sum_j |W_rj||k_j|)^2)`` taken componentwise, which is
  never larger and keeps the bound tight where ``W`` has large entries of both signs.
- log-posterior:  first-order propagation of the mean and variance bounds through the analytic ``d lp / d m_p`` and
  ``d lp / d v_p``, plus ``C_L u kappa_2(Sigma_o) (|quad_o| + |logdet_o|)`` per observable block (the Cholesky of the
  setup and of the walker's k x k matrix).  An absolute bound, not a fraction of ``|lp|``.

Constants, chosen once for every shape (the depth of the device's summation trees is at most a few dozen levels):
``C_M = 64``, ``C_V = 64``, ``C_L = 64``, ``EPS_EXP = 4 u``, ``EPS_BESSEL = 2e-14``; ``C_X = c_x(d)`` and
``C_Xd = c_x_direct(d)`` depend on the number of parameters, as follows.

The distance factors.  ``C_X8 = 8`` was set for the 8-wide instances (d <= 8) and covers their longest sums: the
d + 1 = 9 rounded product-adds of the d = 8 product and the 8 squared differences of the direct distance.  The
first-order worst-case error of a sum of n rounded terms is ``gamma_n ~ n u`` times the sum of the absolute terms
(Higham, Accuracy and Stability, ch. 3), linear in n, so a longer sum scales the factor by the ratio of the counts:

- expanded form: ``r^2 = fma(acc, -2, |q'|^2)``.  ``acc`` is a chain of KS = ``kstar_ksteps(d)`` MFMA k-steps
  (``kstar_tile_product``) of 4 product-adds each; ``|q'|^2`` is, per lane, a chain of at most KS fmas over the
  components 4 s + (lane >> 4) and then two cross-lane adds (``kstar_mfma_block``), at most KS + 2 <= 7 roundings.
  Rounding assumption for the f64 MFMA: one rounding per product-add, in an order that is not documented.  A padded
  slot adds an exact zero, which a rounding leaves exact, so of the 4 KS slots the d + 1 that hold a coordinate or
  the training row's -1/2 |x'|^2 are rounded, whatever KS is; the |q'|^2 chain is never longer.  Then
  ``c_x(d) = C_X8 max(d + 1, 9) / 9``: 8 for d <= 8, 80/9 at d = 9, 128/9 at d = 15 and 136/9 at d = 16.
- direct distance: ``kstar_direct_r2<DP>`` sums ``fma(df, df, r2)`` serially over the DP = 8 or 16 padded
  coordinates; a padded coordinate has ``df = 0``, whose fma is exact, so d terms are rounded:
  ``c_x_direct(d) = C_X8 max(d, 8) / 8 = max(d, 8)``.

Both are exactly 8 for d <= 8, so every bound of the 8-wide instances is the one it was.  A caller that wants the
8-wide factor at d > 8 passes ``cx=C_X8``.

Limit: the rounding of the inputs.  ``C_X u (|q~|^2 + |x~_j|^2)`` counts the roundings of the product and of the sums,
measured in the centred coordinates.  The centred operands are themselves rounded from the uncentred scaled ones:
the query's ``fma(q, s / ls, -s c)`` with both constants rounded on the host, the training row's ``(X / ls - c) s``.
That moves ``q~ - x~_j`` by up to ``u (|q / ls| + |X_j / ls| + |c| + |q~| + 2 |x~_j|)`` per coordinate, and r^2 by
twice its product with ``|q~ - x~_j|``.  Where a length scale is small against the coordinates' distance from the
origin (sklearn's lower bound 1e-5: ``|q / ls| ~ 1e5`` while ``|q~ - x~_j|`` stays O(1) for near pairs) this term
dominates: without it the float64 oracle leaves the bound (err/bound up to 11 on the 8-wide shapes), and the
device rounds the same inputs.  ``input_rounding=True``
adds it.  It is off by default so that the bounds the sweep was calibrated with stay as they were; a case with
``path_cases.Case.ls_bounds`` must turn it on.
"""
from __future__ import annotations

import math

import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import gamma, kv

from oracle import gp_oracle as O

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "tests/hp_ref.py needs an extended np.longdouble (x87 80-bit or better)"

U = 2.0 ** -53
C_X8, C_M, C_V, C_L = 8.0, 64.0, 64.0, 64.0
EPS_EXP = 4 * U
EPS_BESSEL = 2e-14


def kstar_ksteps(d):
    """MFMA k-steps of the cross-kernel for d parameters (kstar_host.h: kstar_ksteps)"""
    return 2 if d + 1 <= 8 else (d + 4) // 4


def c_x(d):
    """the expanded-form distance factor of d parameters (module docstring): C_X8 max(d + 1, 9) / 9"""
    return C_X8 * max(d + 1, 9) / 9


def c_x_direct(d):
    """the direct-distance factor of d parameters (module docstring): C_X8 max(d, 8) / 8"""
    return C_X8 * max(d, 8) / 8


def _is_direct(spec):
    return spec.kind == O.MATERN and spec.nu < 1.0


def _base_ld(r2, spec):
    """base kernel of squared scaled distances, longdouble (general nu: scipy's Bessel function in float64)"""
    if spec.kind == O.RBF or np.isinf(spec.nu):
        return np.exp(-r2 / 2)
    r = np.sqrt(r2)
    if spec.nu == 0.5:
        return np.exp(-r)
    if spec.nu == 1.5:
        t = r * np.sqrt(LD(3))
        return (1 + t) * np.exp(-t)
    if spec.nu == 2.5:
        t = r * np.sqrt(LD(5))
        return (1 + t + t * t / 3) * np.exp(-t)
    nu = spec.nu
    t = np.sqrt(LD(2 * nu)) * r
    t64 = np.asarray(t, dtype=np.float64).copy()
    t64[t64 == 0.0] = math.sqrt(2 * nu) * np.finfo(float).eps      # skl kernels.py:1725-1733 (d = 0 -> eps)
    with np.errstate(over="ignore", invalid="ignore"):
        val = (2.0 ** (1.0 - nu)) / gamma(nu) * t64 ** nu * kv(nu, t64)
    val[~np.isfinite(val)] = 0.0                                     # kv underflow far out
    return val.astype(LD)


def _base64(r2, spec):
    return np.asarray(_base_ld(np.asarray(np.maximum(r2, 0.0), dtype=LD), spec), dtype=np.float64)


def _clamp_floor(r2, spec):
    """what the closed forms' exponential returns where it clamps: exp2_scaled4 (predict_dev.h) takes arguments below
    -700 (natural units) as -700, so there the device gives prefactor(t) e^-700 (~1e-304 times the prefactor) where
    the kernel is ~0.  An absolute term of dk (0 for general nu, whose Bessel routine does not clamp)"""
    if spec.kind == O.MATERN and spec.nu not in (0.5, 1.5, 2.5) and not np.isinf(spec.nu):
        return np.zeros_like(r2)
    if spec.kind == O.RBF or np.isinf(spec.nu):
        a, pref = r2 / 2, np.ones_like(r2)
    else:
        a = np.sqrt(r2) * {0.5: 1.0, 1.5: math.sqrt(3.0), 2.5: math.sqrt(5.0)}[spec.nu]
        pref = 1 + a if spec.nu == 1.5 else 1 + a + a * a / 3 if spec.nu == 2.5 else np.ones_like(r2)
    return np.where(a > 700.0, pref * math.exp(-700.0) * (1 + 16 * U), 0.0)


def kstar(Xq, X_train, gp, spec, cx=None, input_rounding=False):
    """longdouble K_* [B, N] and its error bound dk [B, N] (module docstring); cx: one distance factor for both forms
    instead of c_x(d) and c_x_direct(d); input_rounding: add the rounding of the centred inputs (module docstring)"""
    ls = np.asarray(gp.ls, dtype=np.float64)
    d = X_train.shape[1]
    cx, cxd = (c_x(d), c_x_direct(d)) if cx is None else (cx, cx)
    q = Xq.astype(LD) / ls.astype(LD)
    x = X_train.astype(LD) / ls.astype(LD)
    diff = q[:, None, :] - x[None, :, :]
    r2 = np.sum(diff * diff, axis=2)
    K = _base_ld(r2, spec)
    # the device's centred coordinates: mid-range of the scaled training set (kstar_host.h)
    u = X_train / ls
    cen = 0.5 * (u.min(axis=0) + u.max(axis=0))
    qt = Xq / ls - cen
    xt = u - cen
    nq = np.sum(qt * qt, axis=1)
    nx = np.sum(xt * xt, axis=1)
    r2f = np.asarray(r2, dtype=np.float64)
    k64 = np.asarray(K, dtype=np.float64)
    d2 = cx * U * (nq[:, None] + nx[None, :])
    if input_rounding:
        aq = np.abs(Xq / ls) + np.abs(cen) + np.abs(qt)
        ax = np.abs(u) + 2 * np.abs(xt)
        d2 = d2 + 2 * U * np.einsum("bnd,bnd->bn", np.abs(qt[:, None, :] - xt[None, :, :]), aq[:, None, :] + ax[None, :, :])
    dk = np.maximum(np.abs(_base64(r2f - d2, spec) - k64), np.abs(_base64(r2f + d2, spec) - k64))
    if _is_direct(spec):
        near = r2f < 2e-7 * (nq[:, None] + 1.0)
        if np.any(near):
            rr = np.sqrt(r2f)
            dr = cxd * U * (np.abs(Xq / ls).sum(axis=1)[:, None] + np.abs(u).sum(axis=1)[None, :])
            ddir = np.maximum(np.abs(_base64((rr + dr) ** 2, spec) - k64),
                              np.abs(_base64(np.maximum(rr - dr, 0.0) ** 2, spec) - k64))
            strictly = r2f < 0.5e-7 * (nq[:, None] + 1.0)
            dk = np.where(strictly, ddir, np.where(near, np.maximum(dk, ddir), dk))
    eps = EPS_BESSEL if (spec.kind == O.MATERN and spec.nu not in (0.5, 1.5, 2.5) and not np.isinf(spec.nu)) else EPS_EXP
    dk = dk + eps * np.abs(k64) + _clamp_floor(r2f + d2, spec)
    if spec.has_const:
        K = K + LD(gp.const)
        dk = dk + U * (np.abs(k64) + gp.const)
    return K, dk


def forward_subst(L, B):
    """L^-1 B in longdouble, L lower [N, N], B [N, m]"""
    L = L.astype(LD)
    V = np.empty(B.shape, dtype=LD)
    for i in range(L.shape[0]):
        V[i] = (B[i] - L[i, :i] @ V[:i]) / L[i, i]
    return V


class PCRef:
    """the reference of one PC for B queries: mean, var (longdouble) and their bounds (float64); V kept for tests"""

    def __init__(self, Xq, X_train, gp, spec, cx=None, input_rounding=False):
        K, dk = kstar(Xq, X_train, gp, spec, cx, input_rounding)
        self.K, self.dk = K, dk
        self.mean = K @ np.asarray(gp.alpha, dtype=LD)
        V = forward_subst(gp.L, K.T.astype(LD))
        self.V = V
        kd = 1.0 + (gp.const if spec.has_const else 0.0) + (gp.noise if spec.has_noise else 0.0)
        self.kdiag = kd
        var = LD(kd) - np.sum(V * V, axis=0)
        self.var_raw = var
        self.var = np.where(var < 0, LD(0), var)
        k64 = np.abs(np.asarray(K, dtype=np.float64))
        L64 = np.asarray(gp.L, dtype=np.float64)
        W = solve_triangular(L64, np.eye(L64.shape[0]), lower=True, check_finite=False)
        aW, aL = np.abs(W), np.abs(L64)
        a = aW @ k64.T                                   # [N, B]
        b = aW @ (aL @ a)
        Vf = np.abs(np.asarray(V, dtype=np.float64))
        self.mean_bound = C_M * U * (k64 @ np.abs(gp.alpha)) + dk @ np.abs(gp.alpha)
        self.var_bound = (C_V * U * (kd + np.sum(Vf * Vf, axis=0) + 2 * np.sum(Vf * (a + b), axis=0))
                          + 2 * np.sum(Vf * (aW @ dk.T), axis=0))


def gp_predict(Xq, model, cx=None, input_rounding=False):
    """(mean, var) [B, k] longdouble and (mean_bound, var_bound) [B, k] float64; the PCRef objects"""
    pcs = [PCRef(Xq, model.X_train, gp, model.spec, cx, input_rounding) for gp in model.gps]
    mean = np.stack([p.mean for p in pcs], axis=1)
    var = np.stack([p.var for p in pcs], axis=1)
    mb = np.stack([p.mean_bound for p in pcs], axis=1)
    vb = np.stack([p.var_bound for p in pcs], axis=1)
    return mean, var, mb, vb, pcs


# ---- low-rank block likelihood ---------------------------------------------------------------------------------------
def _chol_ld(A):
    """lower Cholesky of a batch of SPD matrices [..., n, n] in longdouble"""
    A = A.astype(LD).copy()
    n = A.shape[-1]
    Lc = np.zeros_like(A)
    for j in range(n):
        s = A[..., j, j] - np.sum(Lc[..., j, :j] ** 2, axis=-1)
        Lc[..., j, j] = np.sqrt(s)
        if j + 1 < n:
            Lc[..., j + 1:, j] = (A[..., j + 1:, j] - np.einsum("...ik,...k->...i", Lc[..., j + 1:, :j], Lc[..., j, :j])) \
                / Lc[..., j, j][..., None]
    return Lc


def _solve_lower_ld(Lc, b):
    """Lc^-1 b, Lc [..., n, n], b [..., n, m]"""
    n = Lc.shape[-1]
    x = np.zeros(b.shape, dtype=LD)
    for i in range(n):
        x[..., i, :] = (b[..., i, :] - np.einsum("...k,...km->...m", Lc[..., i, :i], x[..., :i, :])) / Lc[..., i, i][..., None]
    return x


def lowrank_setup_blocks(model, y_exp, y_err, block_start, n_div=1.0, cov_unexpl=None):
    """oracle.lowrank_setup_blocks in longdouble: per block G, g0, q0, logdetA (and A, U, r0 for the bound)"""
    if cov_unexpl is None:
        cov_unexpl = O.cov_unexplained(model)
    s = model.scaler_scale.astype(LD)
    k = model.n_pc
    A = (cov_unexpl.astype(LD) / LD(n_div)) * np.outer(s, s) + np.diag(y_err.astype(LD) ** 2)
    Uf = s[:, None] * model.components[:k].T.astype(LD)
    r0 = model.scaler_mean.astype(LD) - y_exp.astype(LD)
    out = []
    for o in range(len(block_start) - 1):
        sl = slice(int(block_start[o]), int(block_start[o + 1]))
        Ab, Ub, rb = A[sl, sl], Uf[sl], r0[sl]
        cA = _chol_ld(Ab)
        y1 = _solve_lower_ld(cA, np.concatenate([Ub, rb[:, None]], axis=1))
        AiU, Air0 = y1[:, :k], y1[:, k]
        out.append(dict(G=AiU.T @ AiU, g0=AiU.T @ Air0, q0=Air0 @ Air0,
                        logdetA=2 * np.sum(np.log(np.diag(cA))), A=np.asarray(Ab, dtype=np.float64),
                        U=np.asarray(Ub, dtype=np.float64)))
    return out


def loglik_blocks(m, var, setups):
    """per walker [B] the sum over blocks of oracle.loglik_lowrank, longdouble; m, var [B, k] longdouble.
    Returns (lp [B], terms [B, nblk], quad [B, nblk], logdet [B, nblk])"""
    m = m.astype(LD)
    sd = np.sqrt(np.maximum(var.astype(LD), 0))
    k = m.shape[1]
    terms, quads, logdets = [], [], []
    for st in setups:
        G, g0, q0 = st["G"], st["g0"], st["q0"]
        M = np.eye(k, dtype=LD)[None] + sd[:, :, None] * G[None] * sd[:, None, :]
        LM = _chol_ld(M)
        h = m @ G + g0[None]
        w = _solve_lower_ld(LM, (sd * h)[:, :, None])[:, :, 0]
        quad = np.einsum("bi,ij,bj->b", m, G, m) + 2 * (m @ g0) + q0 - np.sum(w * w, axis=1)
        logdet = st["logdetA"] + 2 * np.sum(np.log(np.diagonal(LM, axis1=1, axis2=2)), axis=1)
        terms.append(-0.5 * quad - 0.5 * logdet)
        quads.append(quad)
        logdets.append(logdet)
    terms = np.stack(terms, axis=1)
    return np.sum(terms, axis=1), terms, np.stack(quads, axis=1), np.stack(logdets, axis=1)


def loglik_bound(m, var, mb, vb, setups):
    """a-priori bound [B] of the device's low-rank log-likelihood given mean / variance bounds mb, vb [B, k]"""
    m = np.asarray(m, dtype=np.float64)
    v = np.maximum(np.asarray(var, dtype=np.float64), 0.0)
    _, _, quad, logdet = loglik_blocks(np.asarray(m, dtype=LD), np.asarray(v, dtype=LD), setups)
    quad = np.asarray(quad, dtype=np.float64)
    logdet = np.asarray(logdet, dtype=np.float64)
    bound = np.zeros(m.shape[0])
    for o, st in enumerate(setups):
        A, Uo = st["A"], st["U"]
        G = np.asarray(st["G"], dtype=np.float64)
        g0 = np.asarray(st["g0"], dtype=np.float64)
        # Sigma = A + U diag(v) U^T; U^T Sigma^-1 r = h - G S M^-1 S h, U^T Sigma^-1 U = G - G S M^-1 S G
        sd = np.sqrt(v)
        M = np.eye(G.shape[0])[None] + sd[:, :, None] * G[None] * sd[:, None, :]
        h = m @ G + g0[None]
        Mi = np.linalg.inv(M)
        t = np.einsum("bij,bj->bi", Mi, sd * h)
        z = h - (sd * t) @ G                                          # U^T Sigma^-1 r
        GS = G[None] * sd[:, None, :]
        P = G[None] - np.einsum("bij,bjk,bkl->bil", GS, Mi, np.transpose(GS, (0, 2, 1)))
        dm = np.abs(z)                                                 # |d lp / d m|
        dv = 0.5 * np.abs(z * z - np.diagonal(P, axis1=1, axis2=2))    # |d lp / d v|
        Sig = A[None] + np.einsum("fi,bi,gi->bfg", Uo, v, Uo)
        ev = np.linalg.eigvalsh(Sig)
        kappa = ev[:, -1] / ev[:, 0]
        bound += np.sum(dm * mb + dv * vb, axis=1) + C_L * U * kappa * (np.abs(quad[:, o]) + np.abs(logdet[:, o]))
    return bound


def log_posterior(Xq, model, lo, hi, y_exp, y_err, block_start, n_div=1.0, cov_unexpl=None, pred=None,
                  input_rounding=False):
    """(lp [B] longdouble with -inf outside the open box, bound [B] float64); pred: gp_predict(Xq, model) if at hand"""
    mean, var, mb, vb, _ = pred if pred is not None else gp_predict(Xq, model, input_rounding=input_rounding)
    setups = lowrank_setup_blocks(model, y_exp, y_err, block_start, n_div, cov_unexpl)
    lp, _, _, _ = loglik_blocks(mean, var, setups)
    bound = loglik_bound(mean, var, mb, vb, setups)
    inside = np.all((Xq > lo) & (Xq < hi), axis=1)
    lp = np.where(inside, lp, LD(-np.inf))
    bound = np.where(inside, bound, 0.0)
    return lp, bound, setups
