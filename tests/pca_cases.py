"""The scaler + PCA sweep (tests only): one table of cases shared by the CPU tests of the extended-precision reference
(test_pca_hp_ref_host.py) and the GPU sweep (test_gpu_pca_hp.py), in the pattern of cv_cases.py.  Shapes are the smallest
that reach each mechanism of csrc/k_pca.hip (work orientation m = max(N, F) rows, n = min(N, F) columns):

- n = 31, 32, 33: the columns are dealt into blocks of PB = 16, an even number nb of them: nb 2 -> 4;
- n = 64, 65: nb 4 -> 6, the sixth block all padding; n = 96: six full blocks;
- m = 64, 65: the rows are padded to 64-row chunks (64 -> 128);
- 300 x 40: five chunks over five row splits, whose sum runs in passes of four: a partial second pass;
- 520 x 40: nine chunks, the largest number of row splits (8);
- wide (N < F): the transpose is factored; square; the smallest legal shapes;
- n > 1024: the PB = 32 instance with two inner sweeps (1026 x 1025, and the wide 1025 x 1100): certificates only, a
  longdouble SVD of that size is not affordable.

Every case with a reference must meet the admission conditions of pca_hp_ref on the REFERENCE alone
(test_pca_hp_ref_host.py checks them): its n_pc leading singular values a factor 1.5 from every other one, every column
a factor 100 from the constant-feature threshold, at most one undecided sign decision.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import pca_hp_ref as H

REF_LIMIT = 100              # a reference exists where min(N, F) <= this


@dataclass(frozen=True)
class PcaCase:
    name: str
    N: int
    F: int
    n_pc: int = 5
    data: str = "flat"       # flat | graded | dup | equal2 | offset | const_edge | allconst
    flip: str = "v"          # the sign rule: GPEMU_SVD_FLIP unset, or "u"
    seed: int = 0            # of the generator (chosen where the first draw missed an admission condition)

    @property
    def has_reference(self):
        return min(self.N, self.F) <= REF_LIMIT


def cases():
    out = [
        PcaCase("n2x2", 2, 2, n_pc=1), PcaCase("n3x7", 3, 7, n_pc=2), PcaCase("n9x4", 9, 4, n_pc=2, seed=2),
        PcaCase("cols31", 110, 31), PcaCase("cols32", 110, 32), PcaCase("cols33", 110, 33),
        PcaCase("cols64", 110, 64), PcaCase("cols65", 110, 65), PcaCase("cols96", 130, 96),
        PcaCase("rows64", 64, 20), PcaCase("rows65", 65, 20),
        PcaCase("splits5", 300, 40, seed=5), PcaCase("splits8", 520, 40),
        PcaCase("wide24x70", 24, 70), PcaCase("wide33x300", 33, 300), PcaCase("square40", 40, 40),
        PcaCase("pb32_1026x1025", 1026, 1025), PcaCase("pb32_wide1025x1100", 1025, 1100),
        PcaCase("cols33_u", 110, 33, flip="u"), PcaCase("wide24x70_u", 24, 70, flip="u"),
        # the u rule on an exact tie: the one score column of a 2 x 2 matrix is (x, -x), and the first index must win
        PcaCase("n2x2_u", 2, 2, n_pc=1, flip="u"),
    ]
    for tag, (N, F) in (("tall", (130, 70)), ("wide", (40, 150))):
        out += [
            PcaCase(f"flat_{tag}", N, F), PcaCase(f"graded_{tag}", N, F, data="graded"),
            PcaCase(f"dup_{tag}", N, F, n_pc=3, data="dup", seed=1), PcaCase(f"equal2_{tag}", N, F, n_pc=3, data="equal2"),
            PcaCase(f"offset_{tag}", N, F, data="offset"), PcaCase(f"const_edge_{tag}", N, F, n_pc=2, data="const_edge"),
            PcaCase(f"allconst_{tag}", N, F, n_pc=0, data="allconst"),
        ]
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


REFERENCED = [c.name for c in cases() if c.has_reference]
CERTIFICATE_ONLY = [c.name for c in cases() if not c.has_reference]
NEEDS_SWEEPS = "cols96"      # needs more than 3 sweeps (test_pca_hp_ref_host.py checks it on the float64 model)


def _orthonormal(rng, rows, cols):
    q, _ = np.linalg.qr(rng.normal(size=(rows, cols)))
    return q


@lru_cache(maxsize=None)
def data(name):
    """the case's Y (N, F), float64, read-only"""
    c = case(name)
    N, F = c.N, c.F
    rng = np.random.default_rng([N, F, sum(map(ord, c.data)), c.seed])
    r = min(N - 1, F)                       # rank after centring
    if c.data == "allconst":
        Y = np.tile(np.arange(F, dtype=np.float64) - 3.0, (N, 1))
    else:
        ks = min(5, r)
        amp = math.sqrt(N * F) * 3.0 ** -np.arange(ks)
        if c.data == "equal2":
            amp[4] = amp[3]
        Ul, Vr = _orthonormal(rng, N, ks), _orthonormal(rng, F, ks)
        Y = (Ul * amp) @ Vr.T
        if c.data == "graded":
            # the rest of the spectrum graded geometrically down to 1e-12 of the largest: real columns all the way down to
            # a hundred times the residue threshold (4 sqrt(m) eps ||Xc||_F, about 1e-14 of the largest here)
            rest = r - ks
            Ur, Vt = _orthonormal(rng, N, r), _orthonormal(rng, F, r)
            Ur -= Ul @ (Ul.T @ Ur)
            Vt -= Vr @ (Vr.T @ Vt)
            s = np.geomspace(amp[-1] / 4, 1e-12 * amp[0], rest)
            Y = Y + (Ur[:, :rest] * s) @ Vt[:, :rest].T
        else:
            nu = amp[-1] / (math.sqrt(N) + math.sqrt(F)) / 4
            Y = Y + nu * rng.normal(size=(N, F))
        if c.data == "dup":
            # twenty exact duplicates and three constant columns, among the columns the signal loads least: an exactly
            # tied pair of entries must not be the largest of a leading component more than once (the sign decisions)
            quiet = np.argsort(np.max(np.abs(Vr), axis=1), kind="stable")
            Y[:, quiet[20:40]] = Y[:, quiet[:20]]
            Y[:, quiet[40]], Y[:, quiet[41]], Y[:, quiet[42]] = 3.0, -7.0, 0.0
        if c.data == "offset":
            Y = 1e6 + 1e-3 * (Y - Y.mean(axis=0)) / Y.std(axis=0)
        if c.data == "const_edge":
            # columns a factor ~300 either side of sklearn's threshold N eps var + (N mean eps)^2 at mean 1e6
            thr = (N * 1e6 * H.EPS) ** 2
            z = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
            z[N - 1] = 0.0 if N % 2 else z[N - 1]
            for j, factor in ((0, 300.0), (1, 1 / 300.0), (2, 1000.0), (3, 1 / 1000.0)):
                Y[:, j] = 1e6 + math.sqrt(factor * thr) * rng.permutation(z) * math.sqrt(N / np.count_nonzero(z))
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    Y.setflags(write=False)
    return Y


@lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    assert c.has_reference, name
    return H.reference(data(name), c.n_pc, flip_u=c.flip == "u")


@lru_cache(maxsize=None)
def centred(name):
    """the longdouble Xc of a case (what the certificates need)"""
    return H.centred_ld(data(name))[0]


# ---- gpemu_truncation_cov on its own ------------------------------------------------------------------------------------
@dataclass(frozen=True)
class TruncCase:
    name: str
    F: int
    n_comp: int
    n_pc: int


def trunc_cases():
    out = [TruncCase(f"F{F}", F, min(F, 40), min(F, 40) // 2 if F > 1 else 0) for F in (1, 63, 64, 65, 130)]
    out += [TruncCase(f"K{K}", 70, 40, 40 - K) for K in (1, 31, 32, 33)]
    out += [TruncCase("npc0", 70, 40, 0), TruncCase("npc_all", 70, 40, 40), TruncCase("ncomp_lt_F", 130, 12, 3)]
    return out


def trunc_case(name):
    return next(c for c in trunc_cases() if c.name == name)


@lru_cache(maxsize=None)
def trunc_data(name):
    """(components (n_comp, F) with rows orthonormal to longdouble rounding, rounded to float64; explained_variance)"""
    c = trunc_case(name)
    rng = np.random.default_rng([c.F, c.n_comp, c.n_pc])
    A = rng.normal(size=(c.F, c.n_comp)).astype(H.LD)
    for j in range(c.n_comp):                                          # modified Gram-Schmidt, twice, in longdouble
        for _ in range(2):
            A[:, j] -= A[:, :j] @ (A[:, :j].T @ A[:, j])
        A[:, j] /= np.sqrt((A[:, j] ** 2).sum())
    comp = np.ascontiguousarray(A.T, dtype=np.float64)
    ev = np.geomspace(3.0, 1e-9, c.n_comp)
    return comp, ev
