"""Reference of the posterior-predictive summaries (tests only, CPU): numpy restatements in ``np.longdouble`` on top of
the extended-precision per-sample reference of tests/hp_ref.py, with the error bound of the device's central value.

Per sample s and feature f (ref: emulation.py:516-548 for one sample, n_div = 1):
    mu[s][f]     = (sum_p mean_p(theta_s) comp[p][f]) scale_f + mean_f
    sigma2[s][f] = (sum_p comp[p][f]^2 var_p(theta_s) + cov_unexplained[f][f]) scale_f^2
``delta[s][f]`` bounds |mu_dev - mu| of the device's float64 back-projection: hp_ref's bound of the PC means carried
through |comp| |scale|, plus the k fused multiply-adds, the scaling and the shift of the projection itself,
``(k + 2) u (sum_p |mean_p| |comp[p][f]| |scale_f| + |mean_f|)``.

Summaries over the S rows: the mean of mu, its population variance, the mean of sigma2, and
``np.quantile(mu, p, axis=0, method='linear')`` -- all in longdouble.  Tolerances (module functions below) follow the
issue: with delta_f = max_s delta[s][f],
    mean            delta_f + S 2^-53 max|mu|
    order stats     delta_f                       (an order statistic is 1-Lipschitz in the sup norm; so is a quantile,
                                                   a convex combination of two, up to 2 ulp of its lerp)
    var_param       2 sqrt(var_ref) delta_f + delta_f^2 + 1e-12 var_ref
    var_emu         1e-9 relative + 1e-14 absolute  (the cross-validation tests' bound for ``variance``)
"""
from __future__ import annotations

import contextlib

import numpy as np

import hp_ref as H
import matern_nu_ref as R
from oracle import gp_oracle as O

LD = np.longdouble
U = 2.0 ** -53


def oracle_for(spec):
    closed = spec.kind == O.RBF or spec.nu in (0.5, 1.5, 2.5, np.inf)
    return contextlib.nullcontext() if closed else R.general_nu()


def problem(N, d, F, k, spec, seed=0):
    """A synthetic d-parameter emulation group at a fixed theta, fitted by the oracle: (GroupModel, lo, hi)."""
    rng = np.random.default_rng(seed)
    lo = -1.0 - rng.uniform(0.0, 1.0, d)
    hi = 1.0 + rng.uniform(0.0, 1.0, d)
    X = rng.uniform(lo, hi, (N, d))
    Wm = rng.normal(size=(d, F))
    Y = np.sin(X @ Wm) + 0.1 * (X ** 2) @ np.abs(Wm) + 0.01 * rng.normal(size=(N, F))
    mean, scale, _ = O.scaler_fit(Y)
    pca = O.pca_fit((Y - mean) / scale)
    ls = (hi - lo) * (0.4 + 0.1 * np.arange(d) / d)
    theta = np.log(np.r_[ls, [0.7] if spec.has_const else [], [0.03] if spec.has_noise else []])
    with oracle_for(spec):
        gps = [O.gp_fit_at_theta(X, pca["Y_pca"][:, i], theta, spec, 1e-10) for i in range(k)]
    model = O.GroupModel(X_train=X, spec=spec, gps=gps, components=pca["components"],
                         explained_variance=pca["explained_variance"], scaler_mean=mean, scaler_scale=scale, n_pc=k)
    return model, lo, hi


def back_project(model, mean_pc, var_pc, mean_bound=None, cov_unexpl=None):
    """(mu, sigma2) [S, F] in longdouble and, with ``mean_bound`` [S, k], delta [S, F] (float64)."""
    k = model.n_pc
    comp = np.asarray(model.components[:k], dtype=LD)
    scale = np.asarray(model.scaler_scale, dtype=LD)
    smean = np.asarray(model.scaler_mean, dtype=LD)
    cu = O.cov_unexplained(model) if cov_unexpl is None else cov_unexpl
    m = np.asarray(mean_pc, dtype=LD)
    v = np.asarray(var_pc, dtype=LD)
    mu = (m @ comp) * scale + smean
    sigma2 = (v @ (comp * comp) + np.diag(cu).astype(LD)) * (scale * scale)
    if mean_bound is None:
        return mu, sigma2
    ac = np.abs(np.asarray(comp, dtype=np.float64))
    asc = np.abs(np.asarray(scale, dtype=np.float64))
    mag = (np.abs(np.asarray(m, dtype=np.float64)) @ ac) * asc + np.abs(np.asarray(smean, dtype=np.float64))
    delta = (np.asarray(mean_bound, dtype=np.float64) @ ac) * asc + (k + 2) * U * mag
    return mu, sigma2, delta


def per_sample(model, X):
    """hp_ref's extended-precision predict of the rows of X, back-projected: mu, sigma2 (longdouble), delta (float64)"""
    with oracle_for(model.spec):
        mean, var, mb, _, _ = H.gp_predict(np.asarray(X, dtype=np.float64), model)
    return back_project(model, mean, var, mb)


def summaries(mu, sigma2, probabilities):
    """dict of longdouble summaries over axis 0"""
    mu = np.asarray(mu, dtype=LD)
    mean = mu.mean(axis=0)
    out = {"mean": mean, "variance_parameters": ((mu - mean) ** 2).mean(axis=0),
           "variance_emulator": np.asarray(sigma2, dtype=LD).mean(axis=0)}
    out["variance"] = out["variance_parameters"] + out["variance_emulator"]
    p = np.asarray(probabilities, dtype=np.float64).reshape(-1)
    out["quantiles"] = (np.quantile(mu, p, axis=0, method="linear") if p.size else np.zeros((0, mu.shape[1]), dtype=LD))
    return out


def tolerances(mu, delta, var_ref):
    """the issue's tolerances per feature: dict(mean, quantiles, variance_parameters)"""
    S = mu.shape[0]
    d = np.max(np.asarray(delta, dtype=np.float64), axis=0)
    vr = np.asarray(var_ref, dtype=np.float64)
    return {"mean": d + S * U * np.max(np.abs(np.asarray(mu, dtype=np.float64)), axis=0),
            "quantiles": d,
            "variance_parameters": 2 * np.sqrt(vr) * d + d * d + 1e-12 * vr}


VAR_EMU_RTOL, VAR_EMU_ATOL = 1e-9, 1e-14


def brute_force(model, X, probabilities):
    """The same summaries from the float64 oracle's full prediction (central_value and the diagonal of cov of
    ``oracle.gp_oracle.predict_group``, one sample per call as the sampler evaluates it): tiny models only."""
    cv, var = [], []
    with oracle_for(model.spec):
        for x in np.asarray(X, dtype=np.float64):
            out = O.predict_group(x[None, :], model)
            cv.append(out["central_value"][0])
            var.append(np.diag(out["cov"][0]))
    return summaries(np.array(cv), np.array(var), probabilities)
