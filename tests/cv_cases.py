"""The cross-validation sweep (tests only): one table of cases shared by the CPU tests of the extended-precision
reference (test_cv_hp_ref_host.py) and the GPU sweep (test_gpu_cv_hp.py), in the pattern of path_cases.py and
fit_cases.py.  Shapes are the smallest that reach each path of csrc/k_cv.hip:

- the fold operands are padded to mp = 64 ceil(m_max / 64); the blocked Cholesky works in 64-tiles and the merge
  inverse in pairs of them with a ragged last pair (mp = 192: three tiles, mp = 320: five);
- a call whose folds are all single points takes cv_loo_kernel (wave-strided sums, N on either side of 64), every
  other call the general path, single-point folds included;
- the SYRK of a fold runs over K = 16 ceil((N - r0) / 16) columns from the fold's first point r0;
- problems are dealt fold-major into chunks (GPEMU_CV_CHUNK caps a chunk).

``admitted`` records, per case, whether the first-order condition of cv_hp_ref holds (``||Sigma|| ||dA|| <= 0.01`` for
every problem of the case).  It is decided here, on the CPU -- test_cv_hp_ref_host.py recomputes it for every drafted
case and fails if the record is wrong -- and cases() hands out the admitted ones only: nothing is skipped at run time.
"""
from __future__ import annotations

import math
import os
import sys
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import cv_hp_ref as H
from oracle import gp_oracle as O

R, M = O.RBF, O.MATERN
JITTER = 1e-10
F = 12                       # observables of every case (>= the largest number of PCs + 1)
CLASSES = ["noise 5e-2", "noise 1e-4", "noise-free"]


@dataclass(frozen=True)
class CvCase:
    name: str
    N: int
    k: int                   # PCs
    kind: int
    nu: float
    const: bool
    noise: float | None      # WhiteKernel level; None: no white kernel at all (the jitter alone)
    folds: str               # key of fold_labels
    data: str = "plain"      # plain | dup_split | dup_same | dup_split_pivot | offset | alien_alpha
    ls_factor: float = 0.5   # length scale / box width
    admitted: bool = True

    @property
    def spec(self):
        return O.KernelSpec(kind=self.kind, nu=self.nu, has_const=self.const, has_noise=self.noise is not None)

    @property
    def conditioning(self):
        return "noise-free" if self.noise is None else "noise 5e-2" if self.noise == 5e-2 else "noise 1e-4"


_KERNELS = [("rbf", R, np.inf, False), ("m05", M, 0.5, False), ("m25", M, 2.5, False), ("m15_const", M, 1.5, True)]
_NOISES = [("n5e-2", 5e-2), ("n1e-4", 1e-4), ("free", None)]


def drafted():
    out = []
    # conditioning sweep: every kernel x every noise level at N = 130, 5 contiguous folds of 26.  The length scale
    # is 2.5 box widths: at the generator's 0.5 the noise-free RBF has cond(L) = 70 and behaves like noise 1e-4;
    # at 2.5 it has cond(L) = 6.6e4 (Matern 2.5: 1.5e3) and every combination still meets the first-order condition
    for kn, kind, nu, const in _KERNELS:
        for nn, noise in _NOISES:
            out.append(CvCase(f"sweep_{kn}_{nn}", 130, 2, kind, nu, const, noise, "k5", ls_factor=2.5))
    out += [
        # fold sizes round the padding and tile edges (two folds: m and the rest)
        CvCase("m63_rbf", 126, 1, R, np.inf, False, 5e-2, "k2"),
        CvCase("m64_m25", 128, 1, M, 2.5, False, 5e-2, "k2"),
        CvCase("m65_m05", 130, 1, M, 0.5, False, 5e-2, "k2"),
        CvCase("m129_rbf_ragged", 258, 1, R, np.inf, False, 5e-2, "k2"),
        CvCase("m129_m25_1e-4", 258, 1, M, 2.5, False, 1e-4, "k2"),
        CvCase("m257_m15_const", 400, 1, M, 1.5, True, 5e-2, "first257"),
        CvCase("m257_m05_free", 400, 1, M, 0.5, False, None, "first257"),
        # layouts
        CvCase("mixed_1_15_129", 290, 1, R, np.inf, False, 5e-2, "mixed"),
        CvCase("mixed_1_15_129_m05_free", 290, 1, M, 0.5, False, None, "mixed"),
        CvCase("last_point_alone", 100, 1, M, 2.5, False, 5e-2, "last_alone"),
        CvCase("ends_in_one_fold", 100, 1, R, np.inf, False, 5e-2, "ends"),
        CvCase("shuffled_ragged", 150, 3, M, 1.5, True, 5e-2, "shuffled"),
        CvCase("shuffled_ragged_1e-4", 150, 3, R, np.inf, False, 1e-4, "shuffled"),
        # leave-one-out: cv_loo_kernel's wave-strided sums on either side of 64; N = 2 is the smallest legal call
        CvCase("loo_n2", 2, 1, R, np.inf, False, 5e-2, "loo"),
        CvCase("loo_n3", 3, 1, M, 0.5, False, 5e-2, "loo"),
        CvCase("loo_n63", 63, 1, M, 2.5, False, 5e-2, "loo"),
        CvCase("loo_n64", 64, 1, R, np.inf, False, 1e-4, "loo"),
        CvCase("loo_n65", 65, 3, M, 1.5, True, 5e-2, "loo"),
        CvCase("loo_n129_m05_free", 129, 1, M, 0.5, False, None, "loo"),
        # PCs: chunks that hold problems of several folds (GPEMU_CV_CHUNK=3 straddles them)
        CvCase("pcs11", 96, 11, R, np.inf, False, 5e-2, "k3"),
        # hard data
        CvCase("dup_split_rbf_free", 96, 1, R, np.inf, False, None, "k3", data="dup_split"),
        CvCase("dup_same_rbf_free", 96, 1, R, np.inf, False, None, "k3", data="dup_same"),
        CvCase("dup_split_m25_free", 96, 1, M, 2.5, False, None, "k3", data="dup_split", ls_factor=2.0),
        CvCase("dup_same_m25_free", 96, 1, M, 2.5, False, None, "k3", data="dup_same", ls_factor=2.0),
        # In exact arithmetic diag Sigma - jitter is a predictive variance of a consistent model and stays above about
        # jitter / (number of duplicates): 1e-10 at a split pair, far above any bound of an admitted case, so on the
        # cases above neither the device nor the reference ever clips.  Here the first pivot L_00 is raised so that the
        # jitter the device derives from it (1e-6) exceeds diag Sigma at the held-out twin: the clip branch runs.
        CvCase("dup_split_rbf_free_pivot", 96, 1, R, np.inf, False, None, "k3", data="dup_split_pivot"),
        CvCase("offset_1e6", 130, 2, R, np.inf, False, 5e-2, "k5", data="offset"),
        CvCase("alien_alpha", 130, 2, M, 2.5, False, 5e-2, "k5", data="alien_alpha"),
        CvCase("alien_alpha_free", 130, 1, M, 0.5, False, None, "k5", data="alien_alpha"),
    ]
    return out


def cases():
    """the admitted cases: what both test modules parametrise over"""
    return [c for c in drafted() if c.admitted]


def case(name):
    return next(c for c in drafted() if c.name == name)


def kfold(N, k):
    """contiguous folds as emulation.kfold_labels deals them (KFold without shuffling: the first N % k one larger)"""
    sizes = np.full(k, N // k)
    sizes[:N % k] += 1
    return np.repeat(np.arange(k), sizes)


def fold_labels(c: CvCase):
    N = c.N
    if c.folds == "loo":
        return np.arange(N)
    if c.folds.startswith("k"):
        return kfold(N, int(c.folds[1:]))
    if c.folds == "first257":                       # m = 257 (mp = 320) and the rest
        return (np.arange(N) >= 257).astype(int)
    if c.folds == "mixed":                           # m = 1, 15 and 129 (and the rest) in one call, interleaved
        return np.random.default_rng(7).permutation(np.repeat([0, 1, 2, 3], [1, 15, 129, N - 145]))
    if c.folds == "last_alone":
        # fold 0 = {N - 1} in a general-path call (r0 = N - 1, K = 16); fold 1 lies in the last 15 rows;
        # folds 2 and 3 = the rest, alternating
        lab = 2 + np.arange(N) % 2
        lab[N - 1] = 0
        lab[[N - 15, N - 12, N - 9, N - 4, N - 2]] = 1
        return lab
    if c.folds == "ends":                            # fold 0 starts at point 0 and ends at point N - 1
        return np.r_[0, np.random.default_rng(11).permutation(np.arange(N - 2) % 3), 0]
    if c.folds == "shuffled":                        # ragged sizes, shuffled labels
        return np.random.default_rng(3).permutation(np.repeat(np.arange(4), [15, 16, 65, N - 96]))
    raise ValueError(c.folds)


def _synthetic():
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bayesian-inference_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    from gpemu import synthetic
    return synthetic


@lru_cache(maxsize=None)
def build(name):
    """(GroupModel, y_train (N, k), fold, cov_unexplained) of a case"""
    c = case(name)
    prob = _synthetic().make_problem(c.N, F, seed=c.N + 17 * c.k)
    X = prob["design"].copy()
    width = prob["hi"] - prob["lo"]
    ls = width * c.ls_factor
    fold = fold_labels(c)
    if c.data in ("dup_split", "dup_same", "dup_split_pivot"):
        # a near-duplicate pair 1e-7 ls apart: rows a and b of one fold, or of two
        a = int(np.flatnonzero(fold == 0)[3])
        b = int(np.flatnonzero(fold == (0 if c.data == "dup_same" else 1))[5])
        e = np.zeros(X.shape[1])
        e[0] = 1.0
        X[b] = X[a] + 1e-7 * ls * e
    mean, scale, _ = O.scaler_fit(prob["Y"])
    pca = O.pca_fit((prob["Y"] - mean) / scale)
    y = pca["Y_pca"][:, :c.k].copy()
    if c.data == "offset":
        y += 1e6
    theta = list(np.log(ls))
    if c.const:
        theta.append(math.log(0.7))
    if c.noise is not None:
        theta.append(math.log(c.noise))
    gps = [O.gp_fit_at_theta(X, y[:, i], np.array(theta), c.spec, JITTER) for i in range(c.k)]
    if c.data == "dup_split_pivot":
        for gp in gps:
            gp.L = gp.L.copy()
            gp.L[0, 0] *= math.sqrt(1 + 1e-6)
    if c.data == "alien_alpha":
        rng = np.random.default_rng(5)
        for gp in gps:                               # not the fit's own: the identity is evaluated from what is given
            gp.alpha = gp.alpha * (1 + 0.3 * rng.standard_normal(c.N)) + 0.1 * rng.standard_normal(c.N)
    model = O.GroupModel(X_train=X, spec=c.spec, gps=gps, components=pca["components"],
                         explained_variance=pca["explained_variance"], scaler_mean=mean, scaler_scale=scale, n_pc=c.k)
    return model, y, fold, O.cov_unexplained(model)


@lru_cache(maxsize=None)
def problem(name):
    """the cv_hp_ref.Problem of a case (one object per case: cv_hp_ref.reference caches on it)"""
    model, y, fold, cu = build(name)
    return H.problem_of_model(model, y, fold, cu)


def reference(name):
    return H.reference(problem(name))
