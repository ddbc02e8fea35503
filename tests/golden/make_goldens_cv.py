#!/usr/bin/env python3
"""Golden vectors of cross-validation at the fitted hyper-parameters (g9_cross_validation.npz) from scikit-learn.

Run in the build container (needs scikit-learn):

    python tests/golden/make_goldens_cv.py          # writes tests/golden/g9_cross_validation.npz

For every fixture below, every PC and k in {2, 5, N}: the fold labels of ``KFold(n_splits=k)`` (no shuffling) and, per
fold, ``GaussianProcessRegressor(kernel=<the golden's fitted kernel_>, alpha=gpr_alpha, optimizer=None)`` fitted to the
other folds and ``predict(X[I], return_std=True)`` on the held-out ones (the variance is std squared, as the reference
squares it, ref: emulation.py:497-499).  Keys: ``<case>_k<k>_fold``, ``_mean_pc``, ``_var_pc``, and ``ks`` (the k of
every case, in the order of CASES).  Only numeric arrays are written.
"""
from __future__ import annotations

import os

import numpy as np
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern, WhiteKernel
from sklearn.model_selection import KFold

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["g1_rbf_noise", "g1_rbf_only", "g1_matern15_noise", "g1_matern25_const_noise", "g2_rbf_noise",
         "g3_realdata_matern15", "g8_matern_nu_2p0"]


def design_of(name, g):
    if "design" in g:
        return g["design"]
    return np.load(os.path.join(HERE, "observables_fixture.npz"))["design"]   # G3: the real design


def fitted_kernel(g, theta, d):
    """base (RBF | Matern nu) [+ ConstantKernel] [+ WhiteKernel], theta = log of the hyper-parameters (skl order)."""
    ls = np.exp(theta[:d])
    base = RBF(length_scale=ls) if int(g["kernel_kind"]) == 0 else Matern(length_scale=ls, nu=float(g["nu"]))
    j = d
    kern = base
    if bool(g["has_const"]):
        kern = kern + ConstantKernel(constant_value=np.exp(theta[j]))
        j += 1
    if bool(g["has_noise"]):
        kern = kern + WhiteKernel(noise_level=np.exp(theta[j]))
    return kern


def main():
    out = {}
    ks_all = []
    for name in CASES:
        g = dict(np.load(os.path.join(HERE, name + ".npz")))
        X = design_of(name, g)
        y = g["Y_pca_truncated"]
        N, d = X.shape
        k_pc = int(g["n_pc"])
        ks = [2, 5, N]
        for k in ks:
            fold = np.zeros(N, dtype=np.int32)
            mean = np.zeros((N, k_pc))
            var = np.zeros((N, k_pc))
            for f, (train, test) in enumerate(KFold(n_splits=k).split(X)):
                fold[test] = f
                for p in range(k_pc):
                    gp = GaussianProcessRegressor(kernel=fitted_kernel(g, g["theta"][p], d), alpha=float(g["gpr_alpha"]),
                                                  optimizer=None).fit(X[train], y[train, p])
                    m, s = gp.predict(X[test], return_std=True)
                    mean[test, p] = m
                    var[test, p] = s ** 2
            out[f"{name}_k{k}_fold"] = fold
            out[f"{name}_k{k}_mean_pc"] = mean
            out[f"{name}_k{k}_var_pc"] = var
        ks_all.append(ks)
    out["ks"] = np.array(ks_all, dtype=np.int64)
    path = os.path.join(HERE, "g9_cross_validation.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "cases:", ", ".join(CASES))


if __name__ == "__main__":
    main()
