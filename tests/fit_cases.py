"""The fit-side sweep (tests only): cases derived from the dispatch rules of csrc/k_fit.hip, the adversarial designs they
run on, and the paths each evaluation must take (restated from device_cholesky_blocked, device_trtri_blocked and
fit_eval_batch).  Shared by the CPU tests of the extended-precision reference (test_fit_ref_host.py) and the GPU sweep
(test_gpu_fit_paths.py).  The counters are gpemu_fit_path_counts (enum gpemu_fit_path), a set of their own beside the
predict / likelihood set of tests/path_cases.py.

Rules restated here:
- the kernel matrix: kmat_kernel<DP, true> for a Matern of general nu, kmat_kernel<DP, false> otherwise;
- the Cholesky runs as one fused launch per panel of 4 blocks of 64 when nblk * nb <= 320 (and GPEMU_CHOL_PANEL is not
  0), else as three-launch steps; the stand-alone gpemu_cholesky always takes the steps;
- a fused panel updates the columns beyond the next panel on the side stream when at least 40 tile rows lie beyond it;
- the heads of a fused panel sit on one XCD (GPEMU_CHOL_HEADS_ONE_XCD=1) when the panel has at least 32 tile rows;
- the triangular inverse merges a ragged pair at every level b where Np - 2 b floor(Np / 2b) > b;
- the gradient: lml_grad_kernel<DP, true> for a general nu, lml_grad_kernel<DP, false> otherwise.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

import fit_ref as FR
from oracle import gp_oracle as O
from path_cases import DPAD

# enum gpemu_fit_path (include/gpemu.h), read through gpemu_fit_path_counts
FIT_PATHS = ["FIT_KMAT", "FIT_KMAT_NU", "CHOL_PANEL", "CHOL_STEPS", "CHOL_LOOKAHEAD", "CHOL_HEADS_ONE_XCD", "TRTRI_RAGGED",
             "FIT_GRAD", "FIT_GRAD_NU", "FIT_BATCH"]
FIT_PATH = {n: i for i, n in enumerate(FIT_PATHS)}
# the 16-wide instances of d = 9 .. 16 count in gpemu_wide_path_counts (tests/path_cases.WIDE_PATHS), not above

NB, CHOL_Q, PANEL_MAX_WG, LA_MIN = 64, 4, 320, 40
R, M = O.RBF, O.MATERN


def rup(x, m):
    return (x + m - 1) // m * m


@dataclass
class FitCase:
    name: str
    N: int
    d: int
    kind: int
    nu: float
    const: bool
    noise: bool
    design: str = "random"     # random | dup (near-duplicate rows at block / row-group edges) | ls_bounds
    jitter: float = 1e-10
    env: dict = field(default_factory=dict)
    full: bool = True          # the full longdouble reference (else residual rows only: the large shapes)

    @property
    def spec(self):
        return O.KernelSpec(kind=self.kind, nu=self.nu, has_const=self.const, has_noise=self.noise)

    @property
    def general_nu(self):
        return FR.general_nu(self.spec)


def cases():
    return [
        FitCase("n1_rbf", 1, 1, R, np.inf, False, True),
        FitCase("n2_m05_const", 2, 2, M, 0.5, True, False),
        FitCase("n15_m15_noise", 15, 3, M, 1.5, False, True),
        FitCase("n16_m25_all", 16, 8, M, 2.5, True, True),
        FitCase("n17_nu07_noise", 17, 2, M, 0.7, False, True, design="dup"),
        FitCase("n63_rbf_jitter_only", 63, 2, R, np.inf, False, False, jitter=1e-6),
        FitCase("n64_nuinf_const", 64, 4, M, np.inf, True, True),
        FitCase("n65_m15_dup", 65, 3, M, 1.5, True, True, design="dup"),
        FitCase("n127_nu2_all", 127, 5, M, 2.0, True, True),
        FitCase("n128_m05_noise", 128, 1, M, 0.5, False, True),
        FitCase("n129_m25_lsb", 129, 6, M, 2.5, False, True, design="ls_bounds"),
        FitCase("n255_nu35_const", 255, 3, M, 3.5, True, False, jitter=1e-8),
        FitCase("n256_rbf_steps", 256, 7, R, np.inf, True, True, env={"GPEMU_CHOL_PANEL": "0"}),
        FitCase("n257_m15_dup", 257, 4, M, 1.5, False, True, design="dup"),
        FitCase("n271_nu07_all", 271, 2, M, 0.7, True, True),
        FitCase("n272_m25_const", 272, 8, M, 2.5, True, False, jitter=1e-8),
        FitCase("n273_rbf_dup", 273, 3, R, np.inf, False, True, design="dup"),
        FitCase("n320_m05_ragged", 320, 3, M, 0.5, True, True),
        FitCase("n448_nu2_ragged_steps", 448, 4, M, 2.0, False, True, env={"GPEMU_CHOL_PANEL": "0"}),
        FitCase("n449_m15_lsb", 449, 5, M, 1.5, True, True, design="ls_bounds"),
        FitCase("n513_rbf_all", 513, 6, R, np.inf, True, True),
        FitCase("n1000_m25_all", 1000, 6, M, 2.5, True, True),
        FitCase("n2300_m15_heads_one_xcd", 2300, 6, M, 1.5, False, True, env={"GPEMU_CHOL_HEADS_ONE_XCD": "1"},
                full=False),
        FitCase("n3300_rbf_lookahead", 3300, 6, R, np.inf, True, True, env={"GPEMU_CHOL_HEADS_ONE_XCD": "0"},
                full=False),
        # 9 .. 16 parameters: kmat_kernel<16, ..> and lml_grad_kernel<16, ..>
        FitCase("w9_n130_m15_dup", 130, 9, M, 1.5, True, True, design="dup"),
        FitCase("w12_n320_nu07_ragged", 320, 12, M, 0.7, False, True),
        FitCase("w12_n129_m25_lsb", 129, 12, M, 2.5, True, True, design="ls_bounds"),
        FitCase("w16_n200_rbf_lsb_steps", 200, 16, R, np.inf, True, True, design="ls_bounds",
                env={"GPEMU_CHOL_PANEL": "0"}),
        # (noise 1e-5 beside near-duplicates: the gradient's bound is wide here, so that even all eight wide gradient
        # components dropped stay inside it -- this case covers the wide kernel matrix, not the wide gradient)
        FitCase("w16_n257_m05_dup", 257, 16, M, 0.5, True, True, design="dup"),
    ]


def design(c: FitCase, seed=0):
    """(X, y, theta) of a case: a random design in the unit box, or one with adversarial rows"""
    rng = np.random.default_rng(1000 + seed + c.N)
    X = rng.random((c.N, c.d))
    if c.design == "dup":
        # near-duplicates 1e-7 apart: across the 64-row block edges and the 16-row gradient groups
        for e in range(16, c.N, 16):
            X[e] = X[e - 1] + 1e-7 * (rng.random(c.d) - 0.5)
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(c.N)
    ls = np.full(c.d, 0.4) * (1 + 0.5 * rng.random(c.d))
    if c.design == "ls_bounds":
        ls[0], ls[-1] = 1e-5, 1e5        # the default bounds of sklearn's length scales (skl kernels.py:1549)
    theta = list(np.log(ls))
    if c.const:
        theta.append(math.log(0.7))
    if c.noise:
        theta.append(math.log(1e-3 if c.design != "dup" else 1e-5))
    return X, y, np.array(theta)


def problem(c: FitCase, seed=0):
    X, y, theta = design(c, seed)
    return FR.FitProblem(X=X, y=y, theta=theta, spec=c.spec, jitter=c.jitter)


# ---- the paths an evaluation must take -------------------------------------------------------------------------------
def chol_paths(N, nb, env, fit=True):
    """counter increments of one device_cholesky_blocked call on nb problems of size N"""
    Np = rup(N, NB)
    nblk = Np // NB
    panels = range(0, nblk, CHOL_Q)
    fused = fit and env.get("GPEMU_CHOL_PANEL", "1") != "0" and nblk * nb <= PANEL_MAX_WG
    out = {}
    if not fused:
        out["CHOL_STEPS"] = len(panels)
        return out
    out["CHOL_PANEL"] = len(panels)
    if env.get("GPEMU_CHOL_HEADS_ONE_XCD") == "1":
        out["CHOL_HEADS_ONE_XCD"] = sum(1 for jb0 in panels if nblk - jb0 >= 32)
    elif env.get("GPEMU_CHOL_HEADS_ONE_XCD") == "0":
        out["CHOL_HEADS_ONE_XCD"] = 0
    if env.get("GPEMU_CHOL_LOOKAHEAD", "1") != "0":
        la = 0
        for jb0 in panels:
            t0 = min(nblk, jb0 + CHOL_Q) * NB
            t1 = min(Np, t0 + CHOL_Q * NB)
            if t0 < Np and t1 < Np and Np - t1 >= LA_MIN * NB:
                la += 1
        out["CHOL_LOOKAHEAD"] = la
    else:
        out["CHOL_LOOKAHEAD"] = 0
    return out


def ragged_merges(N):
    Np = rup(N, NB)
    n, b = 0, NB
    while b < Np:
        if Np - (Np // (2 * b)) * 2 * b > b:
            n += 1
        b *= 2
    return n


def fit_paths(c: FitCase, nb=1, grad=True, env=None):
    """exact counter increments of one fit evaluation (gpemu_fit_lml / _lml_batch / _factor) of nb problems; the keys
    WIDE_FIT_KMAT / WIDE_FIT_GRAD are gpemu_wide_path_counts' FIT_KMAT / FIT_GRAD"""
    env = c.env if env is None else env
    out = kmat_paths(c)
    out.update(chol_paths(c.N, nb, env))
    out["TRTRI_RAGGED"] = ragged_merges(c.N)
    wide = c.d > DPAD
    out["FIT_GRAD_NU" if c.general_nu else "FIT_GRAD"] = 1 if grad and not wide else 0
    out["FIT_GRAD" if c.general_nu else "FIT_GRAD_NU"] = 0
    out["WIDE_FIT_GRAD"] = 1 if grad and wide else 0
    out["FIT_BATCH"] = 1 if nb > 1 else 0
    return out


def kmat_paths(c: FitCase):
    """exact counter increments of one kernel-matrix launch: 8-wide by kind, or the 16-wide instance"""
    wide = c.d > DPAD
    out = {"FIT_KMAT_NU" if c.general_nu else "FIT_KMAT": 0 if wide else 1, "FIT_KMAT" if c.general_nu else "FIT_KMAT_NU": 0}
    out["WIDE_FIT_KMAT"] = 1 if wide else 0
    return out
