"""Extended-precision reference of the joint predictive covariance ``C = K12 - V1^T V2`` (gpemu_gp_predict_cov) and of
the draws ``mean + chol(C + tau I) Z`` (gpemu_gp_sample), with a-priori error bounds of the device's algorithm per
element (tests only, CPU).

Built on ``hp_ref``: ``np.longdouble`` (unit roundoff 2^-64), the forward substitution ``V = L^-1 K(X_train, X)^T``
and the longdouble Cholesky.  The symmetric form (``X2 is None``) carries ``kernel_.diag`` (1 + const + noise) on its
diagonal, as ``kernel_(X)`` does in scikit-learn; the two-set form carries no noise (skl _gpr.py:367-469).

Error bound.  ``u = 2^-53``.  The device (k_pcov.hip) forms every kernel entry from the coordinates directly,
``r^2 = sum_i ((a_i - b_i) (1 / ls_i))^2``: a relative error of at most ``C_D u r^2``, ``C_D = 2 d + 16``, that moves the
kernel by at most ``|k(r^2 +- dr^2) - k(r^2)|`` (monotone in r), plus the evaluation ``EPS_K |k|`` (library exp, closed
forms; ``hp_ref.EPS_BESSEL`` for general nu) and the constant's addition ``u (|k| + const)``: ``dk``.  The diagonal of
the symmetric form is ``kernel_.diag`` exactly (``dk = 0``).  With ``W = L^-1`` inverted once on the device
(componentwise error ``|W||L||W|``, Higham ch. 8), ``a = |W||K|``, ``b = |W||L| a``:

    |dC_ab| <= C_V u (|K12_ab| + sum_r |V1_ra||V2_rb| + sum_r |V1_ra| (a2 + b2)_rb + sum_r (a1 + b1)_ra |V2_rb|)
               + sum_r |V1_ra| (|W| dk2)_rb + sum_r (|W| dk1)_ra |V2_rb| + dk12_ab

-- the style of ``hp_ref``'s variance bound, which it equals on the diagonal up to the kernel's ``dk`` form.

Draws: the device factors ``A + tau I`` with ``A`` within ``|dC|`` of the reference's ``C``, and the factorisation adds a
backward error of at most ``C_V M u |Lc||Lc|^T``.  First-order perturbation of the Cholesky factor (Sun 1991) with a
factor 2 of slack: ``||dLc||_F <= 2 ||Lc||_2 ||(C + tau I)^-1||_2 ||dA||_F``, so that per element
``|dY_as| <= ||dLc||_F ||Z_s||_2 + C_V u (|Lc||Z|)_as + mean_bound_a``.
"""
from __future__ import annotations

import numpy as np
from scipy.linalg import solve_triangular

import hp_ref as H
from oracle import gp_oracle as O

LD = np.longdouble
U = H.U
C_V = H.C_V
EPS_K = 8 * U


def _eps_eval(spec):
    general = spec.kind == O.MATERN and spec.nu not in (0.5, 1.5, 2.5) and not np.isinf(spec.nu)
    return H.EPS_BESSEL if general else EPS_K


def kmat(A, B, gp, spec, sym=False):
    """K(A rows, B rows) [na, nb] in longdouble (+ const) and its bound dk [na, nb]; ``sym``: B is A and the diagonal
    is kernel_.diag exactly (noise included)"""
    ls = np.asarray(gp.ls, dtype=np.float64)
    a = A.astype(LD) / ls.astype(LD)
    b = B.astype(LD) / ls.astype(LD)
    diff = a[:, None, :] - b[None, :, :]
    r2 = np.sum(diff * diff, axis=2)
    K = H._base_ld(r2, spec)
    r2f = np.asarray(r2, dtype=np.float64)
    k64 = np.asarray(K, dtype=np.float64)
    dr2 = (2 * A.shape[1] + 16) * U * r2f
    dk = np.maximum(np.abs(H._base64(r2f - dr2, spec) - k64), np.abs(H._base64(r2f + dr2, spec) - k64))
    dk = dk + _eps_eval(spec) * np.abs(k64)
    const = gp.const if spec.has_const else 0.0
    if spec.has_const:
        K = K + LD(const)
        dk = dk + U * (np.abs(k64) + const)
    if sym:
        kd = 1.0 + const + (gp.noise if spec.has_noise else 0.0)
        idx = np.arange(A.shape[0])
        K[idx, idx] = LD(kd)
        dk[idx, idx] = 0.0
    return K, dk


class PCCov:
    """the reference of one PC: C [M1, M2] (longdouble) and its bound (float64); ``X2 is None``: the symmetric form"""

    def __init__(self, X1, X2, X_train, gp, spec):
        sym = X2 is None
        Xb = X1 if sym else X2
        K1, dk1 = kmat(X_train, X1, gp, spec)
        K2, dk2 = (K1, dk1) if sym else kmat(X_train, Xb, gp, spec)
        K12, dk12 = kmat(X1, Xb, gp, spec, sym=sym)
        V1 = H.forward_subst(gp.L, K1)
        V2 = V1 if sym else H.forward_subst(gp.L, K2)
        self.C = K12 - V1.T @ V2
        L64 = np.asarray(gp.L, dtype=np.float64)
        W = solve_triangular(L64, np.eye(L64.shape[0]), lower=True, check_finite=False)
        aW, aL = np.abs(W), np.abs(L64)
        a1 = aW @ np.abs(np.asarray(K1, dtype=np.float64))
        a2 = a1 if sym else aW @ np.abs(np.asarray(K2, dtype=np.float64))
        e1 = a1 + aW @ (aL @ a1)
        e2 = e1 if sym else a2 + aW @ (aL @ a2)
        v1 = np.abs(np.asarray(V1, dtype=np.float64))
        v2 = v1 if sym else np.abs(np.asarray(V2, dtype=np.float64))
        w1, w2 = aW @ dk1, (aW @ dk1 if sym else aW @ dk2)
        self.bound = (C_V * U * (np.abs(np.asarray(K12, dtype=np.float64)) + v1.T @ v2 + v1.T @ e2 + e1.T @ v2)
                      + v1.T @ w2 + w1.T @ v2 + dk12)


def predict_cov(X1, X2, model):
    """[k] PCCov objects of a GroupModel"""
    return [PCCov(X1, X2, model.X_train, gp, model.spec) for gp in model.gps]


def chol_ld(A):
    """lower Cholesky of a symmetric positive definite matrix in longdouble"""
    return H._chol_ld(np.asarray(A, dtype=LD))


def draws(C, bound, mean, mean_bound, tau, Z):
    """(Y [M, n] longdouble, bound [M, n]) of mean + chol(C + tau I) Z (module docstring)"""
    M = C.shape[0]
    A = np.asarray(C, dtype=LD) + LD(tau) * np.eye(M, dtype=LD)
    Lc = chol_ld(A)
    Y = np.asarray(mean, dtype=LD)[:, None] + Lc @ Z.astype(LD)
    L64 = np.abs(np.asarray(Lc, dtype=np.float64))
    A64 = np.asarray(A, dtype=np.float64)
    ev = np.linalg.eigvalsh(A64)
    dA = np.linalg.norm(bound) + C_V * M * U * np.linalg.norm(L64 @ L64.T)
    dL = 2 * np.linalg.norm(L64, 2) / ev[0] * dA
    yb = (dL * np.linalg.norm(Z, axis=0)[None, :] + C_V * U * (L64 @ np.abs(Z))
          + np.asarray(mean_bound, dtype=np.float64)[:, None])
    return Y, yb
