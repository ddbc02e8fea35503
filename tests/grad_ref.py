"""Extended-precision reference of the derivatives with respect to the model parameters x, with an
a-priori error bound of the device's algorithm per component (tests only, CPU).  Built on the pieces of ``hp_ref``.

Formulas (np.longdouble throughout), for PC p, query x, training row X_j, r^2 = sum_i ((x_i - X_ji) / l_pi)^2:

    dk_pj/dx_i = -rho(r) (x_i - X_ji) / l_pi^2
        RBF / nu = inf: rho = exp(-r^2 / 2);  Matern 1.5: 3 exp(-sqrt3 r);  Matern 2.5: (5/3)(1 + sqrt5 r) exp(-sqrt5 r)
    dm_p/dx_i  = sum_j alpha_pj dk_pj/dx_i
    dv_p/dx_i  = -2 sum_j u_pj dk_pj/dx_i,   u_p = L_p^-T (L_p^-1 k_p);   0 where the variance was clipped
    a_p = dlp/dm_p = -sum_o z_op,   b_p = dlp/dv_p = 1/2 sum_o (z_op^2 - (P_o)_pp)
        z_o = h_o - G_o S t_o,  h_o = G_o m + g0_o,  t_o = M_o^-1 S h_o,  P_o = G_o - G_o S M_o^-1 S G_o,
        M_o = I + S G_o S,  S = diag(sqrt v)
    dlp/dx_i   = sum_p (a_p dm_p/dx_i + b_p dv_p/dx_i)
    second derivatives, for the bound:  da_p/dm_q = -sum_o P_pq,  da_p/dv_q = sum_o P_pq z_q,
        db_p/dm_q = sum_o z_p P_pq,  db_p/dv_q = sum_o (1/2 P_pq^2 - z_p z_q P_pq)
        (from dz/dm = P, dz/dv_q = -P_:q z_q, dP/dv_q = -P_:q P_q:)

Error bound.  u = 2^-53.  A running error analysis of the device's algorithm (csrc/k_grad.hip), as the same sums in
absolute values, first order.  The device takes every distance of this path directly from the coordinates,
``df_i = (x_i - X_ji) (1 / l_i)``, ``r^2 = sum df_i^2`` (serial fma), and evaluates the kernels with the library's exp.

- distance:  ``delta_r = c_x_direct(d) u sum_i (|x_i| + |X_ji|) / l_i``  (hp_ref: the direct distance's term).
- kernel value:  ``dk_j = max |k(r +- delta_r) - k(r)| + EPS_EXP |k| [+ u (|k| + const)]``.
- rho:  ``drho_j = max |rho(r +- delta_r) - rho(r)| + (EPS_EXP + 4 u) rho``  (4: sqrt, the product with sqrt(2 nu),
  1 + t, the prefactor's product).
- kernel derivative:  ``d(dk_j/dx_i) = drho_j |x_i - X_ji| / l_i^2 + C_DK u rho_j (|x_i| + |X_ji|) / l_i^2`` with
  ``C_DK = 8``: the subtraction (1), two products with 1 / l_i, each carrying the division's rounding (4), the product of
  rho with the weight a alpha_j - 2 b u_j and its sign (2), the accumulating fma (1).
- sums over the training rows.  mean / sum V^2 (grad_meanvar_kernel): sixteen chains of Npad / 16 fmas, then 2 + 2
  pairwise adds: ``c_mv(N) = max(C_M, Npad / 16 + 4)``.  Contraction (grad_contract_kernel, grad_final*_kernel): a chain of
  GRAD_RB / 4 = 64 fmas per wave, 2 pairwise adds across the four waves, then one add per row block (Jacobians:
  ``c_jac(N) = 64 + 2 + nrb``) or per (PC, row block) (gradient: ``c_grad(N, k) = 64 + 2 + k nrb``), nrb = ceil(N / 256).
- mean:  ``mb = c_mv u sum_j |k_j||alpha_j| + sum_j dk_j |alpha_j|``;  d mean:
  ``sum_j |alpha_j| d(dk_j)_i + c_jac u sum_j |alpha_j||dk_j/dx_i|``.
- V = W k and u = W^T V with the inverted factor W (Higham, Accuracy and Stability, ch. 8: the computed inverse errs by
  ``u |W||L||W|`` componentwise), a = |W||k|, b = |W||L||W||k| as in hp_ref:
  ``dV = |W| dk + C_V u (a + b)``,  ``du = |W^T| dV + C_V u (|W^T||V| + |W^T||L^T||W^T||V|)``.
- variance:  hp_ref's form with dk above and max(C_V, c_mv);  d var:
  ``2 sum_j (du_j |dk_j/dx_i| + |u_j| d(dk_j)_i) + c_jac u 2 sum_j |u_j||dk_j/dx_i|``; exactly 0 where clipped.
- a, b:  ``da_p = sum_q (|da_p/dm_q| mb_q + |da_p/dv_q| vb_q) + sum_o C_L u kappa_2(Sigma_o) zabs_op`` with
  ``zabs_o = |G_o||m| + |g0_o| + |G_o| S |t_o|`` (the sums of z in absolute values; the solves amplify by at most the
  condition number, applied to all three);  ``db_p`` likewise with ``|z_op| zabs_op + 1/2 (|G_pp| + (G_pp - P_pp))``.
- gradient:  ``sum_p (|a_p| d(dm_p)_i + |b_p| d(dv_p)_i + da_p |dm_p|_i + db_p |dv_p|_i)
  + c_grad u sum_p sum_j |a_p alpha_j - 2 b_p u_j||dk_j/dx_i|``.

C_M, C_V, C_L, EPS_EXP and c_x_direct are hp_ref's.  No constant here was set from what the device returns.

Clipping.  Where ``|var_raw| <= var_bound`` the device's decision to clip is not determined: ``ambiguous`` marks those
entries and ``clip_choice`` selects their branch (a caller that has the device's dvar passes ``dvar == 0`` there); every
other entry keeps the reference's own decision.
"""
from __future__ import annotations

import numpy as np
from scipy.linalg import solve_triangular

import hp_ref as H
from oracle import gp_oracle as O

LD = H.LD
U = H.U
GRAD_RB = 256
C_DK = 8.0


def supported(spec):
    """the kernels the derivative path covers"""
    return spec.kind == O.RBF or np.isinf(spec.nu) or spec.nu in (1.5, 2.5)


def nrb(N):
    return (N + GRAD_RB - 1) // GRAD_RB


def c_mv(N):
    return max(H.C_M, ((N + 127) // 128 * 128) / 16 + 4)


def c_jac(N):
    return GRAD_RB / 4 + 2 + nrb(N)


def c_grad(N, k):
    return GRAD_RB / 4 + 2 + k * nrb(N)


def rho(r, spec):
    """-dk/dr / r of the base kernel (module docstring), in r's precision"""
    one = r.dtype.type(1)
    if spec.kind == O.RBF or np.isinf(spec.nu):
        return np.exp(-r * r / 2)
    if spec.nu == 1.5:
        return 3 * np.exp(-np.sqrt(one * 3) * r)
    if spec.nu == 2.5:
        t = np.sqrt(one * 5) * r
        return one * 5 / 3 * (1 + t) * np.exp(-t)
    raise ValueError(f"no derivative reference for Matern nu = {spec.nu}")


def backward_subst(L, B):
    """L^-T B in longdouble, L lower [N, N], B [N, m]"""
    L = L.astype(LD)
    X = np.empty(B.shape, dtype=LD)
    n = L.shape[0]
    for i in range(n - 1, -1, -1):
        X[i] = (B[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def kdiag_of(gp, spec):
    return 1.0 + (gp.const if spec.has_const else 0.0) + (gp.noise if spec.has_noise else 0.0)


def kernel_ld(Xq, X_train, gp, spec):
    """(K [B, N] with the constant, diff [B, N, d] = (x - X_j) / l, r [B, N]) in longdouble"""
    ls = np.asarray(gp.ls, dtype=np.float64).astype(LD)
    diff = (Xq.astype(LD)[:, None, :] - X_train.astype(LD)[None]) / ls
    r2 = np.sum(diff * diff, axis=2)
    K = H._base_ld(r2, spec)
    if spec.has_const:
        K = K + LD(gp.const)
    return K, diff, np.sqrt(r2)


def predict_ld(Xq, model):
    """(mean, var, var_raw) [B, k] in longdouble, no bounds: hp_ref.PCRef's values (the finite differences' function)"""
    mean, var, raw = [], [], []
    for gp in model.gps:
        K, _, _ = kernel_ld(Xq, model.X_train, gp, model.spec)
        V = H.forward_subst(gp.L, K.T)
        vr = LD(kdiag_of(gp, model.spec)) - np.sum(V * V, axis=0)
        mean.append(K @ np.asarray(gp.alpha, dtype=LD))
        raw.append(vr)
        var.append(np.where(vr < 0, LD(0), vr))
    return np.stack(mean, axis=1), np.stack(var, axis=1), np.stack(raw, axis=1)


def loglik_ld(Xq, model, setups):
    """the log-likelihood (no box prior) of the rows of Xq, longdouble: hp_ref.loglik_blocks of predict_ld"""
    mean, var, _ = predict_ld(Xq, model)
    return H.loglik_blocks(mean, var, setups)[0]


class PCGrad:
    """one PC for B queries: mean, var, dmean [B, d], dvar [B, d] (unclipped form) and their bounds"""

    def __init__(self, Xq, X_train, gp, spec):
        Xq = np.asarray(Xq, dtype=np.float64)
        N, d = X_train.shape
        ls = np.asarray(gp.ls, dtype=np.float64)
        K, diff, r = kernel_ld(Xq, X_train, gp, spec)
        rh = rho(r, spec)
        dK = -rh[:, :, None] * diff / ls.astype(LD)                       # [B, N, d]
        alpha = np.asarray(gp.alpha, dtype=LD)
        self.mean = K @ alpha
        V = H.forward_subst(gp.L, K.T)                                    # [N, B]
        u = backward_subst(gp.L, V)
        kd = kdiag_of(gp, spec)
        self.var_raw = LD(kd) - np.sum(V * V, axis=0)
        self.var = np.where(self.var_raw < 0, LD(0), self.var_raw)
        self.dmean = np.einsum("bnd,n->bd", dK, alpha)
        self.dvar_unclipped = -2 * np.einsum("bnd,nb->bd", dK, u)
        # ---- bounds (float64) -------------------------------------------------------------------------------------
        r64 = np.asarray(r, dtype=np.float64)
        cst = gp.const if spec.has_const else 0.0
        kb = np.asarray(K, dtype=np.float64) - cst                        # base kernel
        dr = H.c_x_direct(d) * U * (np.abs(Xq / ls).sum(axis=1)[:, None] + np.abs(X_train / ls).sum(axis=1)[None, :])
        rlo = np.maximum(r64 - dr, 0.0)
        dk = np.maximum(np.abs(H._base64((r64 + dr) ** 2, spec) - kb), np.abs(H._base64(rlo ** 2, spec) - kb))
        dk = dk + H.EPS_EXP * np.abs(kb)
        if spec.has_const:
            dk = dk + U * (np.abs(kb) + cst)
        rh64 = np.asarray(rh, dtype=np.float64)
        drho = np.maximum(np.abs(rho(r64 + dr, spec) - rh64), np.abs(rho(rlo, spec) - rh64)) + (H.EPS_EXP + 4 * U) * rh64
        l2 = ls * ls
        adiff = np.abs(Xq[:, None, :] - X_train[None]) / l2
        asum = (np.abs(Xq)[:, None, :] + np.abs(X_train)[None]) / l2
        ddK = drho[:, :, None] * adiff + C_DK * U * rh64[:, :, None] * asum
        adK = np.abs(np.asarray(dK, dtype=np.float64))
        k64 = np.abs(np.asarray(K, dtype=np.float64))
        aal = np.abs(np.asarray(gp.alpha, dtype=np.float64))
        L64 = np.asarray(gp.L, dtype=np.float64)
        W = solve_triangular(L64, np.eye(N), lower=True, check_finite=False)
        aW, aL = np.abs(W), np.abs(L64)
        a = aW @ k64.T                                                    # [N, B]
        b = aW @ (aL @ a)
        Vf = np.abs(np.asarray(V, dtype=np.float64))
        uf = np.abs(np.asarray(u, dtype=np.float64))
        cmv, cj = c_mv(N), c_jac(N)
        Wdk = aW @ dk.T
        self.mean_bound = cmv * U * (k64 @ aal) + dk @ aal
        self.var_bound = (max(H.C_V, cmv) * U * (kd + np.sum(Vf * Vf, axis=0) + 2 * np.sum(Vf * (a + b), axis=0))
                          + 2 * np.sum(Vf * Wdk, axis=0))
        dV = Wdk + H.C_V * U * (a + b)
        WtV = aW.T @ Vf
        du = aW.T @ dV + H.C_V * U * (WtV + aW.T @ (aL.T @ WtV))
        self.sa = np.einsum("n,bnd->bd", aal, adK)                        # sum_j |alpha_j||dk_j/dx_i|
        self.su = np.einsum("nb,bnd->bd", uf, adK)                        # sum_j |u_j||dk_j/dx_i|
        self.dmean_bound = np.einsum("n,bnd->bd", aal, ddK) + cj * U * self.sa
        self.dvar_bound = 2 * (np.einsum("nb,bnd->bd", du, adK) + np.einsum("nb,bnd->bd", uf, ddK)) + cj * U * 2 * self.su
        self.ambiguous = np.abs(np.asarray(self.var_raw, dtype=np.float64)) <= self.var_bound
        self.clipped = np.asarray(self.var_raw < 0)


def gp_jacobian(Xq, model, clip_choice=None):
    """dict of [B, k(, d)] arrays: mean, var, var_raw, dmean, dvar (longdouble); mean_bound, var_bound, dmean_bound,
    dvar_bound (float64); clipped (the branch taken: clip_choice where ambiguous), ambiguous; pcs"""
    assert supported(model.spec), model.spec
    pcs = [PCGrad(Xq, model.X_train, gp, model.spec) for gp in model.gps]
    st = lambda name: np.stack([getattr(p, name) for p in pcs], axis=1)      # noqa: E731
    out = {n: st(n) for n in ("mean", "var_raw", "dmean", "mean_bound", "var_bound", "dmean_bound", "ambiguous")}
    clipped = st("clipped")
    if clip_choice is not None:
        clipped = np.where(out["ambiguous"], np.asarray(clip_choice, dtype=bool), clipped)
    out["clipped"] = clipped
    out["var"] = np.where(clipped, LD(0), np.maximum(out["var_raw"], LD(0)))
    out["dvar"] = np.where(clipped[:, :, None], LD(0), st("dvar_unclipped"))
    out["dvar_bound"] = np.where(clipped[:, :, None], 0.0, st("dvar_bound"))
    out["sa"], out["su"] = st("sa"), st("su")
    out["pcs"] = pcs
    return out


def _minv_ld(M):
    """inverse of a batch of SPD matrices in longdouble, through the Cholesky factor: W^T W, W = L^-1"""
    k = M.shape[-1]
    Lc = H._chol_ld(M)
    Wl = H._solve_lower_ld(Lc, np.broadcast_to(np.eye(k, dtype=LD), M.shape).copy())
    return np.einsum("bji,bjk->bik", Wl, Wl)


def adjoints(mean, var, setups):
    """a, b [B, k] (longdouble), the four second-derivative matrices [B, k, k] and per block (z, P, zabs, pabs)"""
    m = mean.astype(LD)
    v = np.maximum(var.astype(LD), 0)
    sd = np.sqrt(v)
    B, k = m.shape
    a = np.zeros((B, k), LD)
    b = np.zeros((B, k), LD)
    dadm = np.zeros((B, k, k), LD)
    dadv = np.zeros((B, k, k), LD)
    dbdm = np.zeros((B, k, k), LD)
    dbdv = np.zeros((B, k, k), LD)
    blocks = []
    for st in setups:
        G, g0 = st["G"], st["g0"]
        M = np.eye(k, dtype=LD)[None] + sd[:, :, None] * G[None] * sd[:, None, :]
        Mi = _minv_ld(M)
        h = m @ G + g0[None]
        t = np.einsum("bij,bj->bi", Mi, sd * h)
        z = h - (sd * t) @ G
        GS = G[None] * sd[:, None, :]
        P = G[None] - np.einsum("bij,bjk,blk->bil", GS, Mi, GS)
        a += -z
        b += 0.5 * (z * z - np.diagonal(P, axis1=1, axis2=2))
        dadm += -P
        dadv += P * z[:, None, :]
        dbdm += z[:, :, None] * P
        dbdv += 0.5 * P * P - z[:, :, None] * z[:, None, :] * P
        aG = np.abs(np.asarray(G, dtype=np.float64))
        zabs = (np.abs(np.asarray(m, float)) @ aG + np.abs(np.asarray(g0, float))[None]
                + (np.asarray(sd, float) * np.abs(np.asarray(t, float))) @ aG)
        gd = np.diag(np.asarray(G, dtype=np.float64))[None]
        pabs = np.abs(gd) + (gd - np.asarray(np.diagonal(P, axis1=1, axis2=2), dtype=np.float64))
        blocks.append(dict(z=z, P=P, zabs=zabs, pabs=pabs))
    return a, b, dadm, dadv, dbdm, dbdv, blocks


def adjoint_bounds(var, mb, vb, setups, adj):
    """a-priori bounds (da, db) [B, k] of the device's a_p and b_p (module docstring)"""
    a, b, dadm, dadv, dbdm, dbdv, blocks = adj
    f = lambda x: np.abs(np.asarray(x, dtype=np.float64))                     # noqa: E731
    da = np.einsum("bpq,bq->bp", f(dadm), mb) + np.einsum("bpq,bq->bp", f(dadv), vb)
    db = np.einsum("bpq,bq->bp", f(dbdm), mb) + np.einsum("bpq,bq->bp", f(dbdv), vb)
    v = np.maximum(np.asarray(var, dtype=np.float64), 0.0)
    for st, bl in zip(setups, blocks):
        Sig = st["A"][None] + np.einsum("fi,bi,gi->bfg", st["U"], v, st["U"])
        ev = np.linalg.eigvalsh(Sig)
        kappa = (ev[:, -1] / ev[:, 0])[:, None]
        da += H.C_L * U * kappa * bl["zabs"]
        db += H.C_L * U * kappa * (f(bl["z"]) * bl["zabs"] + 0.5 * bl["pabs"])
    return da, db


def setups_with_cov(model, y_exp, cov, block_start, n_div=1.0, cov_unexpl=None):
    """hp_ref.lowrank_setup_blocks with a dense within-observable data covariance ``cov`` (F, F; zero across the
    blocks) in place of diag(y_err^2): the same Woodbury constants per block, in longdouble"""
    if cov_unexpl is None:
        cov_unexpl = O.cov_unexplained(model)
    s = model.scaler_scale.astype(LD)
    k = model.n_pc
    A = (cov_unexpl.astype(LD) / LD(n_div)) * np.outer(s, s) + np.asarray(cov, dtype=np.float64).astype(LD)
    Uf = s[:, None] * model.components[:k].T.astype(LD)
    r0 = model.scaler_mean.astype(LD) - y_exp.astype(LD)
    out = []
    for o in range(len(block_start) - 1):
        sl = slice(int(block_start[o]), int(block_start[o + 1]))
        Ab, Ub, rb = A[sl, sl], Uf[sl], r0[sl]
        cA = H._chol_ld(Ab)
        y1 = H._solve_lower_ld(cA, np.concatenate([Ub, rb[:, None]], axis=1))
        AiU, Air0 = y1[:, :k], y1[:, k]
        out.append(dict(G=AiU.T @ AiU, g0=AiU.T @ Air0, q0=Air0 @ Air0, logdetA=2 * np.sum(np.log(np.diag(cA))),
                        A=np.asarray(Ab, dtype=np.float64), U=np.asarray(Ub, dtype=np.float64)))
    return out


def reference(Xq, model, y_exp, y_err, block_start, clip_choice=None, n_div=1.0, cov_unexpl=None, setups=None):
    """Everything of gp_jacobian plus: lp [B] (longdouble, the log-likelihood without the box prior), a, b, da, db
    [B, k], grad [B, d] (longdouble) and grad_bound [B, d] (float64)."""
    out = gp_jacobian(Xq, model, clip_choice)
    if setups is None:
        setups = H.lowrank_setup_blocks(model, y_exp, y_err, block_start, n_div, cov_unexpl)
    N, k = model.X_train.shape[0], model.n_pc
    adj = adjoints(out["mean"], out["var"], setups)
    a, b = adj[0], adj[1]
    da, db = adjoint_bounds(out["var"], out["mean_bound"], out["var_bound"], setups, adj)
    f = lambda x: np.abs(np.asarray(x, dtype=np.float64))                     # noqa: E731
    out.update(setups=setups, a=a, b=b, da=da, db=db)
    out["lp"] = H.loglik_blocks(out["mean"], out["var"], setups)[0]
    out["grad"] = np.einsum("bp,bpd->bd", a, out["dmean"]) + np.einsum("bp,bpd->bd", b, out["dvar"])
    su = np.where(out["clipped"][:, :, None], 0.0, out["su"])
    out["grad_bound"] = (np.einsum("bp,bpd->bd", f(a), out["dmean_bound"]) + np.einsum("bp,bpd->bd", f(b), out["dvar_bound"])
                         + np.einsum("bp,bpd->bd", da, f(out["dmean"])) + np.einsum("bp,bpd->bd", db, f(out["dvar"]))
                         + c_grad(N, k) * U * (np.einsum("bp,bpd->bd", f(a), out["sa"]) + 2 * np.einsum("bp,bpd->bd", f(b), su)))
    return out


# ---- the noise-free case with clipped variances ---------------------------------------------------------------------
def clip_case(seed=3):
    """(model, lo, hi, y_exp, y_err, block_start, Xq): a noise-free RBF model of 3 PCs on 24 design points in 2
    parameters; the queries are 8 training rows and 8 random points.  PC 0's factor is that of (1 - 1e-6) K, so its
    sum V^2 is 1 + 1e-6 on a training row: var_raw = -1e-6 there, clipped beyond any rounding.  The other PCs' factors
    are those of K + 1e-10 I: on a training row their variance is ~1e-10, for the bound to decide.  Away from the design
    every variance is well above its bound."""
    rng = np.random.default_rng(seed)
    N, d, k, F = 24, 2, 3, 6
    lo = np.array([-1.0, 0.0])
    hi = np.array([1.0, 2.0])
    design = rng.uniform(lo, hi, (N, d))
    spec = O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=False, has_noise=False)
    Y = np.tanh(((design - lo) / (hi - lo)) @ rng.normal(size=(d, F))) + 0.05 * rng.normal(size=(N, F))
    mean, scale, _ = O.scaler_fit(Y)
    pca = O.pca_fit((Y - mean) / scale)
    gps = []
    for i in range(k):
        th = np.log((hi - lo) * rng.uniform(0.15, 0.3, d))
        gp = O.gp_fit_at_theta(design, pca["Y_pca"][:, i], th, spec, 1e-10)
        if i == 0:
            gp.L = gp.L * np.sqrt(1.0 - 1e-6)
        gps.append(gp)
    model = O.GroupModel(X_train=design, spec=spec, gps=gps, components=pca["components"],
                         explained_variance=pca["explained_variance"], scaler_mean=mean, scaler_scale=scale, n_pc=k)
    y_exp = Y[0] + 0.05
    y_err = rng.uniform(0.02, 0.2, F)
    Xq = np.concatenate([design[:8], rng.uniform(lo + 0.05, hi - 0.05, (8, d))])
    return model, lo, hi, y_exp, y_err, np.array([0, F], dtype=np.int64), Xq


def sweep_cases(num_cu=256):
    """(supported cases of path_cases.cases(), Matern 0.5 rerun as 1.5; names of the general-nu cases left out)"""
    import path_cases as PC
    run, skipped = [], []
    for c in PC.cases(num_cu):
        if c.general_nu:
            skipped.append(c.name)
            continue
        if c.kind == O.MATERN and c.nu == 0.5:
            c.nu = 1.5
        run.append(c)
    return run, skipped
