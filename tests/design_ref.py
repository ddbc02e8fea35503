"""Extended-precision reference of the sequential-design criterion (gpemu_design_*), with a-priori
error bounds of the device's algorithm per candidate (tests only, CPU).

Built on ``cov_ref`` / ``hp_ref``: per PC the two-set covariance ``C = K12 - V1^T V2`` in ``np.longdouble`` with
``cov_ref.PCCov``'s bound (the same formula, with ``V`` of each set of rows formed once), then

    num_p(c) = sum_s omega_s C_p(s, c)^2      den_p(c) = C_p(c, c) + tau_p      IV_p = sum_s omega_s C_p(s, s)
    score(c) = sum_p w_p num_p(c) / den_p(c)              (a PC with den_p(c) <= min_variance kernel_.diag_p: 0)

and the conditioning on a pick c*: ``u(.) = C(., c*) / sqrt(den(c*))`` (0 for a PC under the floor at c*),
``C <- C - u u^T``, ``den <- den - u(c)^2``, ``IV <- IV - sum_s omega_s u(s)^2``.

Error bound, ``u = 2^-53``, ``dC`` the bound of an element of C (``PCCov.bound`` before the first pick):

    numerator    dnum = sum_s omega_s (2 |C| dC + dC^2) + C_SUM u num      C_SUM = C_V + 16 + S / 64: the squares, the
                 weights (normalised with one division each) and a sum of 8 + 8 + S / 64 terms in a fixed order
    denominator  dden = dC(c, c) + u (|den| + tau)
    quotient     dq = dnum / (den - dden) + num dden / (den (den - dden)) + 4 u q
    score        sum_p w_p dq_p + k u score

A candidate whose ``den`` lies within ``dden`` of the floor may fall on either side of it: ``near_floor`` flags it.

Conditioning.  The device forms the pick's column by the same sums as an element of C (bound ``dC(., c*)``) and divides
by the square root of its own ``den(c*)``:

    du(x) = dC(x, c*) / sqrt(den* - dden*) + |u(x)| dden* / (2 (den* - dden*)) + 4 u |u(x)|
    dC(a, b) += |u(a)| du(b) + du(a) |u(b)| + du(a) du(b) + C_V u |u(a)| |u(b)|
    dden(c)  += 2 |u(c)| du(c) + du(c)^2 + 2 u (|den(c)| + u(c)^2)
    dIV      += sum_s omega_s (2 |u(s)| du(s) + du(s)^2) + C_SUM u (sum_s omega_s u(s)^2 + |IV|)

Every constant here follows from the algorithm (k_design.hip) and ``hp_ref``'s C_V; none is fitted to device output.
"""
from __future__ import annotations

import numpy as np
from scipy.linalg import solve_triangular

import cov_ref as CR
import hp_ref as H

LD = np.longdouble
U = H.U
C_V = H.C_V


def f64(a):
    return np.asarray(a, dtype=np.float64)


class _Side:
    """V = L^-1 K(X_train, X)^T of one set of rows for one PC, with the pieces of PCCov's bound"""

    def __init__(self, X, X_train, gp, spec, aW, aL):
        K, dk = CR.kmat(X_train, X, gp, spec)
        self.X = X
        self.V = H.forward_subst(gp.L, K)
        a = aW @ np.abs(f64(K))
        self.e = a + aW @ (aL @ a)
        self.v = np.abs(f64(self.V))
        self.w = aW @ dk


def _block(A, B, gp, spec):
    """(C, bound) of the rows of side A against the rows of side B: cov_ref.PCCov's two-set form"""
    K12, dk12 = CR.kmat(A.X, B.X, gp, spec)
    C = K12 - A.V.T @ B.V
    bound = (C_V * U * (np.abs(f64(K12)) + A.v.T @ B.v + A.v.T @ B.e + A.e.T @ B.v) + A.v.T @ B.w + A.w.T @ B.v + dk12)
    return C, bound


def _diag(A, gp, spec):
    """(C(x, x), bound) over the rows of side A: the diagonal of _block(A, A) without the block"""
    k0, dk0 = CR.kmat(A.X[:1], A.X[:1], gp, spec)
    C = k0[0, 0] - np.sum(A.V * A.V, axis=0)
    bound = (C_V * U * (float(k0[0, 0]) + np.sum(A.v * A.v, axis=0) + 2 * np.sum(A.v * A.e, axis=0))
             + 2 * np.sum(A.v * A.w, axis=0) + dk0[0, 0])
    return C, bound


class PCDesign:
    """the state of one PC: Csc [S, M], Ccc [M, M], den [M], iv and their bounds"""

    def __init__(self, Xref, Xcand, omega, X_train, gp, spec, tau, floor):
        L64 = f64(gp.L)
        W = solve_triangular(L64, np.eye(L64.shape[0]), lower=True, check_finite=False)
        aW, aL = np.abs(W), np.abs(L64)
        R = _Side(Xref, X_train, gp, spec, aW, aL)
        Cn = _Side(Xcand, X_train, gp, spec, aW, aL)
        self.omega = omega.astype(LD)
        self.om64 = f64(omega)
        self.tau, self.floor = float(tau), float(floor)
        self.c_sum = C_V + 16 + len(Xref) / 64.0
        self.Csc, self.dSc = _block(R, Cn, gp, spec)
        self.Ccc, self.dCc = _block(Cn, Cn, gp, spec)
        css, dss = _diag(R, gp, spec)
        self.den = np.diag(self.Ccc) + LD(self.tau)
        self.dden = np.diag(self.dCc) + U * (np.abs(f64(self.den)) + self.tau)
        self.iv = np.sum(self.omega * css)
        self.div = float(np.sum(self.om64 * dss) + self.c_sum * U * np.sum(self.om64 * np.abs(f64(css))))

    def terms(self):
        """(q [M] longdouble, dq [M], near_floor [M] bool): num / den under the floor rule"""
        C64, den64 = np.abs(f64(self.Csc)), f64(self.den)
        num = np.sum(self.omega[:, None] * self.Csc * self.Csc, axis=0)
        n64 = f64(num)
        dnum = np.sum(self.om64[:, None] * (2 * C64 * self.dSc + self.dSc ** 2), axis=0) + self.c_sum * U * n64
        above = den64 > self.floor
        near = np.abs(den64 - self.floor) <= self.dden
        lo = np.where(den64 - self.dden > 0, den64 - self.dden, np.nan)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(above, num / self.den, LD(0))
            dq = dnum / lo + n64 * self.dden / (den64 * lo) + 4 * U * np.abs(f64(q))
        dq = np.where(above, dq, 0.0)
        dq = np.where(np.isnan(dq), np.inf, dq)
        return q, dq, near

    def condition(self, c):
        ds, dds = self.den[c], self.dden[c]
        if not float(ds) > self.floor:
            return
        lo = float(ds) - dds
        if lo <= 0:
            raise ValueError("the pick's denominator is not resolved by its bound")
        root = np.sqrt(ds)
        uS, uC = self.Csc[:, c] / root, self.Ccc[:, c] / root
        aS, aC = np.abs(f64(uS)), np.abs(f64(uC))
        duS = self.dSc[:, c] / np.sqrt(lo) + aS * dds / (2 * lo) + 4 * U * aS
        duC = self.dCc[:, c] / np.sqrt(lo) + aC * dds / (2 * lo) + 4 * U * aC
        self.Csc = self.Csc - np.outer(uS, uC)
        self.dSc = self.dSc + np.outer(aS, duC) + np.outer(duS, aC) + np.outer(duS, duC) + C_V * U * np.outer(aS, aC)
        self.Ccc = self.Ccc - np.outer(uC, uC)
        self.dCc = self.dCc + np.outer(aC, duC) + np.outer(duC, aC) + np.outer(duC, duC) + C_V * U * np.outer(aC, aC)
        self.dden = self.dden + 2 * aC * duC + duC ** 2 + 2 * U * (np.abs(f64(self.den)) + aC ** 2)
        self.den = self.den - uC * uC
        drop = np.sum(self.omega * uS * uS)
        self.div = self.div + float(np.sum(self.om64 * (2 * aS * duS + duS ** 2))
                                    + self.c_sum * U * (float(drop) + abs(float(self.iv))))
        self.iv = self.iv - drop


def pc_weights(model, feature_weights=None):
    """w_p = sum_f fw_f (scaler_scale_f components[p, f])^2 of a GroupModel, in longdouble arithmetic"""
    comp = np.asarray(model.components[:model.n_pc], dtype=LD) * np.asarray(model.scaler_scale, dtype=LD)[None, :]
    fw = np.ones(comp.shape[1], dtype=LD) if feature_weights is None else np.asarray(feature_weights, dtype=LD)
    return f64((comp * comp) @ fw)


class DesignRef:
    """the reference of one emulation group (an oracle GroupModel)"""

    def __init__(self, model, Xref, Xcand, weights=None, tau=None, pcw=None, min_variance=1e-6):
        Xref, Xcand = f64(Xref), f64(Xcand)
        S = len(Xref)
        w = np.full(S, 1.0) if weights is None else f64(weights)
        omega = w.astype(LD) / np.sum(w.astype(LD))
        spec = model.spec
        self.pcw = pc_weights(model) if pcw is None else f64(pcw)
        self.pcs = []
        for p, gp in enumerate(model.gps[:model.n_pc]):
            noise = gp.noise if spec.has_noise else 0.0
            kdiag = 1.0 + (gp.const if spec.has_const else 0.0) + noise
            t = noise if tau is None else float(np.asarray(tau).reshape(-1)[p])
            self.pcs.append(PCDesign(Xref, Xcand, omega, model.X_train, gp, spec, t, min_variance * kdiag))

    def scores(self):
        """(score [M] longdouble, bound [M], near_floor [M] bool, per PC: w_p q_p [k, M] longdouble)"""
        parts = [pc.terms() for pc in self.pcs]
        per = np.stack([LD(w) * q for w, (q, _, _) in zip(self.pcw, parts)])
        score = np.sum(per, axis=0)
        bound = sum(w * dq for w, (_, dq, _) in zip(self.pcw, parts)) + len(self.pcs) * U * np.abs(f64(score))
        near = np.any(np.stack([n for _, _, n in parts]), axis=0)
        return score, bound, near, per

    def condition(self, c):
        for pc in self.pcs:
            pc.condition(int(c))

    def iv(self):
        """(IV_p [k] longdouble, bounds [k])"""
        return np.array([pc.iv for pc in self.pcs], dtype=LD), np.array([pc.div for pc in self.pcs])

    def integrated_variance(self):
        """(sum_p w_p IV_p, bound)"""
        iv, div = self.iv()
        return np.sum(self.pcw.astype(LD) * iv), float(np.sum(self.pcw * div) + len(self.pcs) * U * abs(float(np.sum(self.pcw * f64(iv)))))

    def den(self):
        """(den [k, M] longdouble, bounds [k, M])"""
        return np.stack([pc.den for pc in self.pcs]), np.stack([pc.dden for pc in self.pcs])


def brute_force_iv(model, Xref, weights, added, tau=None, pcw=None):
    """sum_p w_p IV_p after refitting every PC's GP at fixed theta with the rows ``added`` appended to the design, each
    carrying noise variance tau_p: the training covariance [[L L^T, k], [k^T, k(x, x) + tau]] factored in longdouble"""
    Xref, added = f64(Xref), f64(added).reshape(-1, model.X_train.shape[1])
    w = np.full(len(Xref), 1.0) if weights is None else f64(weights)
    omega = w.astype(LD) / np.sum(w.astype(LD))
    pcw = pc_weights(model) if pcw is None else f64(pcw)
    spec = model.spec
    total = LD(0)
    for p, gp in enumerate(model.gps[:model.n_pc]):
        noise = gp.noise if spec.has_noise else 0.0
        t = noise if tau is None else float(np.asarray(tau).reshape(-1)[p])
        N, n = model.X_train.shape[0], len(added)
        A = np.zeros((N + n, N + n), dtype=LD)
        Lld = np.tril(gp.L).astype(LD)
        A[:N, :N] = Lld @ Lld.T
        if n:
            A[:N, N:] = CR.kmat(model.X_train, added, gp, spec)[0]
            A[N:, :N] = A[:N, N:].T
            A[N:, N:] = CR.kmat(added, added, gp, spec)[0] + LD(t) * np.eye(n, dtype=LD)
        Lc = H._chol_ld(A)
        Xall = np.concatenate([model.X_train, added])
        V = H.forward_subst(Lc, CR.kmat(Xall, Xref, gp, spec)[0])
        k0 = CR.kmat(Xref[:1], Xref[:1], gp, spec)[0][0, 0]
        total = total + LD(pcw[p]) * np.sum(omega * (k0 - np.sum(V * V, axis=0)))
    return total
