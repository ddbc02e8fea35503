"""Extended-precision reference of the GP fit side, with an a-priori error bound of the device's algorithm per element
(tests only, CPU).

From the float64 inputs the device fit is given (``X``, ``theta``, ``y``, ``jitter``; the hyper-parameters are
``exp(theta)`` in float64, as the host forms them) it recomputes in ``np.longdouble`` (x87 80-bit, unit roundoff 2^-64):

- ``K`` (skl's distance form: ``X / ls``, then the difference) with the jitter on the diagonal;
- ``L`` by a column Cholesky, ``W = L^-1`` by forward substitution;
- ``alpha = W^T (W y)``, ``1/2 log det K = sum log L_ii``, ``y.alpha`` and the log-marginal likelihood;
- ``K^-1 = W^T W``;
- the gradient ``1/2 sum_jl (alpha_j alpha_l - K^-1_jl) dK_jl / dtheta_t`` for every component of theta (log length
  scales, log constant, log noise: skl kernels.py:733-760, 861-866).

The general-nu Matern kernel takes its Bessel parts from scipy in float64 (``t^nu K_nu(t)`` for the value,
``t^(nu-1) K_(nu-1)(t)`` for the derivative); their error is budgeted in ``EPS_BESSEL``, as in ``hp_ref.py``.

Error bound.  ``u = 2^-53``, ``g(n) = (n + 64) u``: the error factor of a sum of at most ``n`` terms, whatever its order
(Higham, Accuracy and Stability, ch. 3: ``gamma_n``), with 64 ulps for the roundings of the terms themselves.  First
order, componentwise, computed in float64 on absolute values; only the reference values are extended.

- ``K``:  off the diagonal the device forms ``r^2 = sum (X_i / l - X_j / l)^2``; with ``a, b`` the two quotients the
  error of ``r^2`` is at most ``C_X u (sum (|a| + |b|) |a - b| + r^2)``, which moves the kernel by at most
  ``|k(r^2 +- delta) - k(r^2)|`` (the kernel is monotone in r); on top ``EPS_K |k|`` for its evaluation (``EPS_BESSEL``
  for general nu) and ``u (|k| + const)`` for the constant's addition.  The diagonal ``1 + const + noise + jitter``:
  ``4 u`` of it.  Call this ``dK``.
- Cholesky: the backward error ``|K^ - L^ L^T| <= g(N) |L^||L^T|`` (Higham Thm 10.3), so the device factor satisfies
  ``|K - L^ L^T| <= dK + g(N) |L^||L^T|`` -- a residual check that does not depend on the condition number.
  ``dKc = dK + g(N) |L||L^T|`` is the total perturbation of ``K`` that the forward bounds below propagate.
- ``W``: ``|W^ - L^-1| <= EW = g(N) |W||L||W|`` (Higham ch. 8: blocked triangular inverses); so
  ``|W^ L^ - I| <= EW |L|``.
- ``alpha``:  ``|K^-1| dKc |alpha| + EW^T |W y| + |W|^T EW |y| + 2 g(N) |W|^T |W| |y|``.
- ``y.alpha``:  ``|y|.dalpha + g(N) |y|.|alpha|``;  ``1/2 log det K``:  ``1/2 sum |K^-1| o dKc + g(N) sum |log L_ii|``;
  the LML: half the first plus the second plus ``4 u`` of its terms.
- ``K^-1``:  ``|K^-1| dKc |K^-1| + EW^T |W| + |W|^T EW + g(N) |W|^T |W|``.
- gradient component t, with ``P = alpha alpha^T - K^-1`` and ``G_t = dK / dtheta_t``:
  ``1/2 sum (|alpha| dalpha^T + dalpha |alpha|^T + dKinv) o |G_t| + 1/2 sum |P| o dG_t + g(N^2) 1/2 sum |P| o |G_t|``,
  where ``dG_t`` is, for a length scale, ``EPS_K |G_t| + D_t |f(r^2 +- delta) - f(r^2)|`` with
  ``delta = (d + 8) u r^2`` (the device's ``(x - x')^2 / l^2`` per dimension, ``G_t = f(r^2) D_t``), and ``u`` of
  ``G_t`` for the constant and the noise.

Constants, fixed once from the algorithm: ``EPS_K = 8 u`` (closed forms: at most seven roundings of positive terms and
a correctly rounded-to-1-ulp exponential), ``EPS_BESSEL = 2e-14`` (hp_ref.py), and ``C_X = c_x(d)``:

``kmat_kernel<DP, ..>`` (k_fit.hip) sums ``fma(df, df, r2)`` serially over the DP = 8 or 16 padded coordinates.  A
padded coordinate has ``df = 0`` and its fma is exact, so d terms are rounded, each once.  ``C_X8 = 8`` was set for the
8-wide instance, whose sums have at most 8 terms; the first-order worst-case error of a sum grows linearly in its
length (``gamma_n ~ n u``, Higham ch. 3), so ``c_x(d) = C_X8 max(d, 8) / 8 = max(d, 8)``: exactly 8 for d <= 8, 16
for the 16 squared differences at d = 16 (the rule of ``hp_ref.c_x_direct``).  The gradient's ``delta`` above already
counts its d terms.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
from scipy.special import gamma, kv

import hp_ref as H
from oracle import gp_oracle as O

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "tests/fit_ref.py needs an extended np.longdouble (x87 80-bit or better)"

U = 2.0 ** -53
C_X8 = 8.0
EPS_K = 8 * U
EPS_BESSEL = H.EPS_BESSEL


def g(n):
    return (n + 64) * U


def c_x(d):
    """the kernel matrix's distance factor of d parameters (module docstring)"""
    return C_X8 * max(d, 8) / 8


def general_nu(spec):
    return spec.kind == O.MATERN and spec.nu not in (0.5, 1.5, 2.5) and not np.isinf(spec.nu)


@dataclass
class FitProblem:
    X: np.ndarray          # (N, d)
    y: np.ndarray          # (N,)
    theta: np.ndarray      # (n_theta,) sklearn's log hyper-parameters
    spec: O.KernelSpec
    jitter: float = 1e-10

    @property
    def hyper(self):
        return O.split_theta(self.theta, self.X.shape[1], self.spec)

    @property
    def eps_k(self):
        return EPS_BESSEL if general_nu(self.spec) else EPS_K


# ---- kernel matrix ---------------------------------------------------------------------------------------------------
def _scaled(X, ls):
    return X.astype(LD) / ls.astype(LD)


def kernel_rows(p, rows):
    """longdouble K[rows, :] (jitter on the diagonal) and its bound dK[rows, :]"""
    X = np.asarray(p.X, dtype=np.float64)
    ls, const, noise = p.hyper
    rows = np.asarray(rows)
    x = _scaled(X, ls)
    diff = x[rows][:, None, :] - x[None, :, :]
    r2 = np.sum(diff * diff, axis=2)
    K = H._base_ld(r2, p.spec)
    a = np.abs(X / ls)
    df = np.abs(np.asarray(diff, dtype=np.float64))
    r2f = np.asarray(r2, dtype=np.float64)
    delta = c_x(X.shape[1]) * U * (np.einsum("rjd,rjd->rj", a[rows][:, None, :] + a[None, :, :], df) + r2f)
    k64 = np.asarray(K, dtype=np.float64)
    dK = np.maximum(np.abs(H._base64(r2f - delta, p.spec) - k64), np.abs(H._base64(r2f + delta, p.spec) - k64))
    dK += p.eps_k * np.abs(k64)
    if p.spec.has_const:
        K = K + LD(const)
        dK += U * (np.abs(k64) + const)
    diag = LD(1) + LD(const) + LD(noise) + LD(p.jitter)
    on = rows[:, None] == np.arange(X.shape[0])[None, :]
    K = np.where(on, diag, K)
    dK = np.where(on, 4 * U * float(diag), dK)
    return K, dK


# ---- longdouble factorisations ----------------------------------------------------------------------------------------
def chol_ld(K):
    """lower Cholesky factor of an SPD matrix, longdouble (column by column)"""
    A = np.array(K, dtype=LD)
    n = A.shape[0]
    Lc = np.zeros_like(A)
    for j in range(n):
        s = A[j, j] - Lc[j, :j] @ Lc[j, :j]
        if not s > 0:
            raise np.linalg.LinAlgError(f"not positive definite at pivot {j}")
        Lc[j, j] = np.sqrt(s)
        if j + 1 < n:
            Lc[j + 1:, j] = (A[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
    return Lc


def tri_inv_ld(L):
    """L^-1 of a lower triangular matrix, longdouble (forward substitution by rows)"""
    L = np.asarray(L, dtype=LD)
    n = L.shape[0]
    W = np.zeros_like(L)
    for i in range(n):
        W[i, :i] = -(L[i, :i] @ W[:i, :i]) / L[i, i]
        W[i, i] = LD(1) / L[i, i]
    return W


# ---- derivative of the base kernel -------------------------------------------------------------------------------------
def _f_ld(r2, spec):
    """dK_base / dlog l_t = f(r^2) D_t, longdouble (general nu: scipy's Bessel function in float64)"""
    r2 = np.asarray(r2, dtype=LD)
    if spec.kind == O.RBF or np.isinf(spec.nu):
        return np.exp(-r2 / 2)
    r = np.sqrt(r2)
    if spec.nu == 0.5:
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(r > 0, np.exp(-r) / np.where(r > 0, r, 1), LD(0))
    if spec.nu == 1.5:
        return 3 * np.exp(-np.sqrt(3 * r2))
    if spec.nu == 2.5:
        t = np.sqrt(5 * r2)
        return LD(5) / 3 * (t + 1) * np.exp(-t)
    nu = spec.nu
    # K = c t^nu K_nu(t), t = sqrt(2 nu) r:  dK/dr = -c sqrt(2 nu) t^nu K_(nu-1)(t),  dr / dlog l_t = -D_t / r
    t = np.asarray(np.sqrt(LD(2 * nu)) * r, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        val = 2 * nu * (2.0 ** (1.0 - nu)) / gamma(nu) * t ** (nu - 1) * kv(nu - 1, t)
    val[~np.isfinite(val)] = 0.0
    return val.astype(LD)


def _f64(r2, spec):
    return np.asarray(_f_ld(np.maximum(r2, 0.0).astype(LD), spec), dtype=np.float64)


# ---- the reference and its bounds --------------------------------------------------------------------------------------
class FitRef:
    """Every fit-side quantity of one problem in longdouble (``K, L, W, alpha, logdet_half, yalpha, lml, Kinv, grad``)
    and its a-priori bound in float64 (``dK, dKc, EW, d_alpha, d_lml, d_Kinv, d_grad``)."""

    def __init__(self, p: FitProblem, grad=True):
        self.p = p
        X = np.asarray(p.X, dtype=np.float64)
        N, d = X.shape
        self.N = N
        idx = np.arange(N)
        self.K, self.dK = kernel_rows(p, idx)
        self.L = chol_ld(self.K)
        self.W = tri_inv_ld(self.L)
        y = np.asarray(p.y, dtype=LD)
        self.alpha = self.W.T @ (self.W @ y)
        self.logdet_half = np.sum(np.log(np.diagonal(self.L)))
        self.yalpha = y @ self.alpha
        self.lml = -self.yalpha / 2 - self.logdet_half - LD(N) / 2 * np.log(2 * LD(math.pi))
        self.Kinv = self.W.T @ self.W
        # bounds
        L64, W64, Ki = (np.abs(np.asarray(a, dtype=np.float64)) for a in (self.L, self.W, self.Kinv))
        y64, a64 = np.abs(p.y), np.abs(np.asarray(self.alpha, dtype=np.float64))
        self.dKc = self.dK + g(N) * (L64 @ L64.T)
        self.EW = g(N) * (W64 @ (L64 @ W64))
        Wy = W64 @ y64
        self.d_alpha = (Ki @ (self.dKc @ a64) + self.EW.T @ Wy + W64.T @ (self.EW @ y64) + 2 * g(N) * (W64.T @ Wy))
        d_yalpha = y64 @ self.d_alpha + g(N) * (y64 @ a64)
        d_logdet = 0.5 * np.sum(Ki * self.dKc) + g(N) * np.sum(np.abs(np.log(np.diagonal(L64))))
        self.d_lml = 0.5 * d_yalpha + d_logdet + 4 * U * (abs(float(self.yalpha)) / 2 + abs(float(self.logdet_half))
                                                         + N / 2 * math.log(2 * math.pi))
        self.d_Kinv = Ki @ self.dKc @ Ki + self.EW.T @ W64 + W64.T @ self.EW + g(N) * (W64.T @ W64)
        if grad:
            self._gradient(X)

    def _gradient(self, X):
        p, N, d = self.p, self.N, X.shape[1]
        ls, const, noise = p.hyper
        al = self.alpha
        P = np.outer(al, al) - self.Kinv
        aP = np.abs(np.asarray(P, dtype=np.float64))
        a64 = np.abs(np.asarray(al, dtype=np.float64))
        dP = np.outer(a64, self.d_alpha) + np.outer(self.d_alpha, a64) + self.d_Kinv
        diff = X.astype(LD)[:, None, :] - X.astype(LD)[None, :, :]
        Dt = diff * diff / (ls.astype(LD) ** 2)                           # (N, N, d)
        r2 = np.sum(Dt, axis=2)
        f = _f_ld(r2, p.spec)
        r2f = np.asarray(r2, dtype=np.float64)
        f64 = np.asarray(f, dtype=np.float64)
        delta = (d + 8) * U * r2f
        df = np.maximum(np.abs(_f64(r2f - delta, p.spec) - f64), np.abs(_f64(r2f + delta, p.spec) - f64))
        eps = p.eps_k
        grads, bounds = [], []
        for t in range(d):
            G = f * Dt[:, :, t]
            D64 = np.asarray(Dt[:, :, t], dtype=np.float64)
            aG = np.abs(np.asarray(G, dtype=np.float64))
            dG = eps * aG + D64 * df
            grads.append(np.sum(P * G) / 2)
            bounds.append(0.5 * np.sum(dP * aG) + 0.5 * np.sum(aP * dG) + g(N * N) * 0.5 * np.sum(aP * aG))
        if p.spec.has_const:
            grads.append(np.sum(P) * LD(const) / 2)
            aG = np.full((N, N), const)
            bounds.append(0.5 * np.sum(dP * aG) + 0.5 * np.sum(aP * U * aG) + g(N * N) * 0.5 * np.sum(aP * aG))
        if p.spec.has_noise:
            grads.append(np.trace(P) * LD(noise) / 2)
            dia = np.diagonal(aP)
            bounds.append(0.5 * noise * (np.sum(np.diagonal(dP)) + U * np.sum(dia) + g(N) * np.sum(dia)))
        self.grad = np.array(grads, dtype=LD)
        self.d_grad = np.array(bounds)


# ---- residual checks (every shape; the only ones at the large shapes) ----------------------------------------------------
def chol_residual(p, Lhat, rows):
    """|K - L^ L^T| on the given rows (longdouble) and its bound dK + g(N) |L^||L^T|, both (len(rows), N)"""
    N = Lhat.shape[0]
    K, dK = kernel_rows(p, rows)
    Lh = np.asarray(Lhat, dtype=LD)
    R = np.abs(K - Lh[rows] @ Lh.T)
    aL = np.abs(Lhat)
    return np.asarray(R, dtype=np.float64), dK + g(N) * (aL[rows] @ aL.T)


def inverse_residual(What, Lhat, rows):
    """|W^ L^ - I| on the given rows (longdouble) and its bound g(N) |W^||L^||W^||L^|"""
    N = Lhat.shape[0]
    R = np.asarray(What, dtype=LD)[rows] @ np.asarray(Lhat, dtype=LD)
    R[np.arange(len(rows)), rows] -= 1
    aW, aL = np.abs(What), np.abs(Lhat)
    return np.asarray(np.abs(R), dtype=np.float64), g(N) * (((aW[rows] @ aL) @ aW) @ aL)


def edge_rows(N, step=64):
    """every row at a 64-row block edge (both sides) and N - 1"""
    r = {0, N - 1}
    for e in range(step, N, step):
        r.update((e - 1, e))
    return np.array(sorted(r))


def ratio(err, bound):
    err = np.abs(np.asarray(err, dtype=np.float64))
    return np.where(err == 0, 0.0, err / np.maximum(np.asarray(bound, dtype=np.float64), 1e-300))


def err_ld(dev, ref):
    return np.abs(np.asarray(dev, dtype=np.float64).astype(LD) - ref).astype(np.float64)
