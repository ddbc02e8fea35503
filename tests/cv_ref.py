"""numpy restatement of cross-validation at fixed hyper-parameters, pinned to the scikit-learn golden
g9_cross_validation.npz and to brute-force oracle refits (tests only)."""
from __future__ import annotations

import numpy as np
from scipy.linalg import solve_triangular

from oracle import gp_oracle as O

# the fixtures of tests/golden/make_goldens_cv.py, in its order
CASES = ["g1_rbf_noise", "g1_rbf_only", "g1_matern15_noise", "g1_matern25_const_noise", "g2_rbf_noise",
         "g3_realdata_matern15", "g8_matern_nu_2p0"]


def closed_form(L, alpha, y, fold, jitter):
    """Block form of the LOO identities (R&W 5.4.2) for one PC: A = K^-1 = L^-T L^-1, per fold I
    mean_I = y_I - (A_II)^-1 alpha_I, var_I = diag((A_II)^-1) - jitter clipped at 0."""
    W = solve_triangular(L, np.eye(L.shape[0]), lower=True)
    A = W.T @ W
    mean = np.empty(len(y))
    var = np.empty(len(y))
    for f in range(int(fold.max()) + 1):
        I = np.flatnonzero(fold == f)
        S = np.linalg.inv(A[np.ix_(I, I)])
        mean[I] = y[I] - S @ alpha[I]
        var[I] = np.maximum(np.diag(S) - jitter, 0.0)
    return mean, var


def closed_form_group(model: O.GroupModel, y_pc, fold, jitter):
    """(mean_pc, var_pc), each (N, n_pc), of every PC of an oracle GroupModel."""
    cols = [closed_form(gp.L, gp.alpha, y_pc[:, p], fold, jitter) for p, gp in enumerate(model.gps)]
    return np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1)


def theta_of(gp: O.GP, spec: O.KernelSpec):
    return np.log(np.r_[gp.ls, [gp.const] if spec.has_const else [], [gp.noise] if spec.has_noise else []])


def brute_force_group(model: O.GroupModel, y_pc, fold, jitter):
    """Refit every PC's GP at its theta to the other folds (oracle.gp_fit_at_theta) and predict the held-out fold."""
    X = model.X_train
    N = X.shape[0]
    mean = np.empty((N, model.n_pc))
    var = np.empty((N, model.n_pc))
    for f in range(int(fold.max()) + 1):
        I, R = np.flatnonzero(fold == f), np.flatnonzero(fold != f)
        for p, gp in enumerate(model.gps):
            fit = O.gp_fit_at_theta(X[R], y_pc[R, p], theta_of(gp, model.spec), model.spec, jitter)
            mean[I, p], var[I, p] = O.gp_predict(X[I], X[R], fit, model.spec)
    return mean, var


def back_project(model: O.GroupModel, mean_pc, var_pc, cov_unexpl):
    """central_value and the diagonal of the covariance of predict_emulation_group for one sample
    (ref: emulation.py:516-548, n_div = 1)."""
    k = model.n_pc
    S = model.components[:k]
    cv = mean_pc @ S * model.scaler_scale + model.scaler_mean
    variance = (var_pc @ (S ** 2) + np.diag(cov_unexpl)) * model.scaler_scale ** 2
    return cv, variance


def case_model(name):
    """(GroupModel, Y_pca_truncated, jitter, Y) of one golden fixture at its fitted theta.  Where the golden stores
    L_ and alpha_ of every PC (G1, G8) they are used as they are; the others are refitted at theta by the oracle."""
    import golden_util as GU
    g = GU.load(name)
    design = g["design"] if "design" in g else GU.load("observables_fixture")["design"]
    k = int(g["n_pc"])
    jitter = float(g["gpr_alpha"])
    if sorted(int(i) for i in g["L_index"]) == list(range(k)):
        spec = GU.spec_of(g)
        gps = []
        for j, i in enumerate(g["L_index"]):
            ls, const, noise = O.split_theta(g["theta"][int(i)], design.shape[1], spec)
            gps.append((int(i), O.GP(ls=ls, const=const, noise=noise, alpha=g["alpha"][int(i)], L=g["L"][j])))
        gps = [gp for _, gp in sorted(gps, key=lambda t: t[0])]
        model = O.GroupModel(X_train=design, spec=spec, gps=gps, components=g["pca_components"],
                             explained_variance=g["pca_explained_variance"], scaler_mean=g["scaler_mean"],
                             scaler_scale=g["scaler_scale"], n_pc=k)
    else:
        model = GU.group_model(g, design=design)
    Y = g["Y"] if "Y" in g else GU.load("observables_fixture")["Y"]
    return model, g["Y_pca_truncated"], jitter, Y
