"""Correlated experimental uncertainties: the reference's dense log-posterior with the full data
covariance, in extended precision, with an error bound of the device's algorithm (tests only, CPU).

The reference's ``log_posterior`` with its TODO resolved (ref: log_posterior.py:90-94): the emulator covariance of the
merge step (block diagonal over the observables, ref: emulation.py:370-388) plus ``C_d`` instead of
``diag(y_err**2)``, where ``C_d = blockdiag_o(C_o) + sum_s b_s b_s^T``.  ``dense_logpost`` restates it in
``np.longdouble`` on the merged observable order; ``woodbury_logpost`` restates the device's algebra (the setup's
``G, g0, q0, W, Q, w0`` per observable block, the walker's ``T_o, c_o, Z_o`` and the S x S factorisation of ``K``) in
float64, for the host tests.

Error bound, in the style of ``tests/hp_ref.py``: first-order propagation of the GP stage's mean / variance bounds
through ``d lp / d m`` and ``d lp / d v`` of the dense formula, plus ``C_L u kappa_2 (|quad| + |logdet|)`` for every
factorisation the device makes: ``Sigma`` as a whole, each block's ``Sigma_o`` and the sources' ``K``.
"""
from __future__ import annotations

import numpy as np

import golden_util as GU
import hp_ref as H
from oracle import gp_oracle as O

LD = np.longdouble
U = H.U
C_L = H.C_L


# ---- the cases: G1, G5, G7 as (groups, data) ---------------------------------------------------------------------------
def case(name):
    """dict(groups=[(GroupModel, columns in the merged order, block starts in the group)], y, y_err, lo, hi, Xq,
    obs (observable index of every merged column))"""
    if name == "G1":
        g = GU.load("g1_rbf_noise")
        F = g["y_exp"].shape[0]
        groups = [(GU.group_model(g), np.arange(F), [0, 12, F])]
    elif name == "G5":
        g = GU.load("g5_multigroup")
        groups = [(GU.group_model(g, prefix=p + "_"), g["cols_" + p], bs)
                  for p, bs in (("g1", [0, 10, 22]), ("g2", [0, 8]))]
    elif name == "G7":
        g = GU.load("g7_shipped_config")
        names, _, block_start, cols = GU.g7_groups(g)
        models = GU.g7_models(g)
        groups = [(models[n], cols[n], block_start[n]) for n in names]
    else:
        raise KeyError(name)
    F = g["y_exp"].shape[0]
    obs = np.full(F, -1, dtype=np.int64)
    nobs = 0
    for _, cols, bs in groups:
        for o in range(len(bs) - 1):
            obs[np.asarray(cols)[bs[o]:bs[o + 1]]] = nobs
            nobs += 1
    assert np.all(obs >= 0)
    return dict(groups=groups, y=g["y_exp"], y_err=g["y_err"], lo=g["lo"], hi=g["hi"], Xq=g["Xq"], obs=obs)


def within_cov(y_err, obs, ell=3.0):
    """exponential correlation across neighbouring bins inside each observable: C_ij = e_i e_j exp(-|i - j| / ell)"""
    F = y_err.shape[0]
    i = np.arange(F)
    C = np.outer(y_err, y_err) * np.exp(-np.abs(i[:, None] - i[None, :]) / ell)
    return np.where(obs[:, None] == obs[None, :], C, 0.0)


def sources(y_err, S, seed):
    """S fully correlated sources over all features (so over every observable and group): a normalisation-like
    source, then smooth shape shifts of a few tens of percent of the uncertainty"""
    rng = np.random.default_rng(seed)
    F = y_err.shape[0]
    x = np.linspace(0.0, 1.0, F)
    out = np.empty((S, F))
    for s in range(S):
        amp = rng.uniform(0.2, 0.8)
        if s == 0:
            prof = np.ones(F)
        else:
            prof = np.cos(np.pi * (s + rng.uniform()) * x + rng.uniform(0, 2 * np.pi))
        out[s] = amp * y_err * prof
    return out


def data_covariance(c, S, seed, correlated=True):
    """(C_d (dense, merged order), cov (the within-observable part or None), sources (S, F) or None)"""
    y_err = c["y_err"]
    cov = within_cov(y_err, c["obs"]) if correlated else None
    src = sources(y_err, S, seed) if S > 0 else None
    Cd = cov.copy() if cov is not None else np.diag(y_err ** 2)
    if src is not None:
        Cd = Cd + src.T @ src
    return Cd, cov, src


# ---- the dense reference (longdouble) -------------------------------------------------------------------------------
def _group_parts(model, cols, bs, n_div):
    k = model.n_pc
    s = model.scaler_scale.astype(LD)
    cun = O.cov_unexplained(model).astype(LD) / LD(n_div) * np.outer(s, s)
    Uf = s[:, None] * model.components[:k].T.astype(LD)
    mask = np.zeros(cun.shape, dtype=bool)
    for o in range(len(bs) - 1):
        mask[bs[o]:bs[o + 1], bs[o]:bs[o + 1]] = True
    return k, cun, Uf, mask


def dense_logpost(c, X, means, vars_, Cd, n_div=1.0):
    """lp [B] (longdouble) of every row of X; means / vars_: per group [B, k].  Rows outside the box: -inf.
    Also returns (Sigma [B, F, F], r [B, F]) in float64 for the bound."""
    F = c["y"].shape[0]
    B = means[0].shape[0]
    Sig = np.broadcast_to(Cd.astype(LD), (B, F, F)).copy()
    r = np.broadcast_to(-c["y"].astype(LD), (B, F)).copy()
    for (model, cols, bs), m, v in zip(c["groups"], means, vars_):
        k, cun, Uf, mask = _group_parts(model, cols, bs, n_div)
        v = np.maximum(v.astype(LD), 0)
        emu = np.einsum("fp,bp,gp->bfg", Uf, v, Uf) + cun[None]
        ix = np.ix_(cols, cols)
        Sig[(slice(None),) + ix] += np.where(mask[None], emu, 0)
        r[:, cols] += m.astype(LD) @ Uf.T + model.scaler_mean.astype(LD)
    lp = np.empty(B, dtype=LD)
    quad = np.empty(B)
    ld = np.empty(B)
    for b in range(B):
        Lc = H._chol_ld(Sig[b])
        z = H._solve_lower_ld(Lc, r[b][:, None])[:, 0]
        quad[b] = float(z @ z)
        ld[b] = float(2 * np.sum(np.log(np.diag(Lc))))
        lp[b] = -0.5 * (z @ z) - np.sum(np.log(np.diag(Lc)))
    inside = np.all((X > c["lo"]) & (X < c["hi"]), axis=1)
    lp = np.where(inside, lp, LD(-np.inf))
    return lp, np.asarray(Sig, dtype=np.float64), np.asarray(r, dtype=np.float64), quad, ld


def bound(c, X, means, vars_, mbs, vbs, Cd, src, n_div=1.0):
    """a-priori bound [B] of the device's result (rows outside the box: 0)"""
    _, Sig, r, quad, ld = dense_logpost(c, X, means, vars_, Cd, n_div)
    B = r.shape[0]
    out = np.zeros(B)
    for b in range(B):
        Si = np.linalg.inv(Sig[b])
        z = Si @ r[b]
        ev = np.linalg.eigvalsh(Sig[b])
        out[b] += C_L * U * (ev[-1] / ev[0]) * (abs(quad[b]) + abs(ld[b]))
        Kb = np.eye(src.shape[0]) if src is not None else None
        for (model, cols, bs), m, v, mb, vb in zip(c["groups"], means, vars_, mbs, vbs):
            k, _, Uf, _ = _group_parts(model, cols, bs, n_div)
            Ug = np.asarray(Uf, dtype=np.float64)
            zg = Ug.T @ z[cols]
            P = Ug.T @ Si[np.ix_(cols, cols)] @ Ug
            out[b] += np.sum(np.abs(zg) * mb[b] + 0.5 * np.abs(zg * zg - np.diag(P)) * vb[b])
            for o in range(len(bs) - 1):
                fc = np.asarray(cols)[bs[o]:bs[o + 1]]
                So = Sig[b][np.ix_(fc, fc)] - (src[:, fc].T @ src[:, fc] if src is not None else 0.0)
                evo = np.linalg.eigvalsh(So)
                Soi = np.linalg.inv(So)
                qo = abs(r[b][fc] @ Soi @ r[b][fc])
                out[b] += C_L * U * (evo[-1] / evo[0]) * (qo + abs(np.sum(np.log(evo))))
                if src is not None:
                    Kb = Kb + src[:, fc] @ Soi @ src[:, fc].T
        if src is not None:
            evk = np.linalg.eigvalsh(Kb)
            out[b] += C_L * U * (evk[-1] / evk[0]) * (abs(quad[b]) + abs(np.sum(np.log(evk))))
    inside = np.all((X > c["lo"]) & (X < c["hi"]), axis=1)
    return np.where(inside, out, 0.0)


# ---- the device's algebra in float64 (host tests) -------------------------------------------------------------------
def woodbury_setup(model, cols, bs, y, y_err, cov, src, n_div=1.0):
    """per observable block: G, g0, q0, logdetA, W, Q, w0 (the setup kernels' Gram products)"""
    k = model.n_pc
    s = model.scaler_scale
    A = O.cov_unexplained(model) / n_div * np.outer(s, s)
    A = A + (cov[np.ix_(cols, cols)] if cov is not None else np.diag(y_err[cols] ** 2))
    Uf = s[:, None] * model.components[:k].T
    r0 = model.scaler_mean - y[cols]
    Bm = src[:, cols].T if src is not None else np.zeros((len(cols), 0))
    out = []
    for o in range(len(bs) - 1):
        sl = slice(bs[o], bs[o + 1])
        C = np.linalg.cholesky(A[sl, sl])
        Z = np.linalg.solve(C, np.concatenate([Uf[sl], r0[sl, None], Bm[sl]], axis=1))
        Zu, zr, Zb = Z[:, :k], Z[:, k], Z[:, k + 1:]
        out.append(dict(G=Zu.T @ Zu, g0=Zu.T @ zr, q0=zr @ zr, logdetA=2 * np.sum(np.log(np.diag(C))),
                        W=Zu.T @ Zb, Q=Zb.T @ Zb, w0=Zb.T @ zr))
    return out


def woodbury_logpost(setups_per_group, means, vars_, S):
    """[B] float64: the block-diagonal sum plus the sources' term, as the device computes them"""
    B = means[0].shape[0]
    out = np.zeros(B)
    for b in range(B):
        total = 0.0
        K = np.eye(S)
        cs = np.zeros(S)
        for setups, m, v in zip(setups_per_group, means, vars_):
            mu, sd = m[b], np.sqrt(np.maximum(v[b], 0.0))
            k = mu.shape[0]
            for st in setups:
                G, g0 = st["G"], st["g0"]
                M = np.eye(k) + sd[:, None] * G * sd[None, :]
                L = np.linalg.cholesky(M)
                h = G @ mu + g0
                yv = np.linalg.solve(L, sd * h)
                quad = mu @ G @ mu + 2 * mu @ g0 + st["q0"] - yv @ yv
                total += -0.5 * quad - 0.5 * (st["logdetA"] + 2 * np.sum(np.log(np.diag(L))))
                if S:
                    T = np.linalg.solve(L, sd[:, None] * st["W"])
                    cs += st["W"].T @ mu + st["w0"] - T.T @ yv
                    K += st["Q"] - T.T @ T
        if S:
            LK = np.linalg.cholesky(K)
            vv = np.linalg.solve(LK, cs)
            total += 0.5 * vv @ vv - np.sum(np.log(np.diag(LK)))
        out[b] = total
    return out
