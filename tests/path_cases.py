"""The launch-path sweep (tests only): a table of cases, each there for a path of the predict / likelihood pipeline, the
models and adversarial queries they run on, and the paths the host dispatch must take for them (mirrored from
csrc/gpemu_api.hip, k_predict.hip, k_trmm_small.hip, k_halfstep.hip and k_loglik.hip).  Shared by the CPU tests of the
extended-precision reference (test_hp_ref_host.py) and the GPU sweep (test_gpu_paths.py).  The cases of 9 to 16
parameters run the 16-wide instances; wide_paths gives the exact increments of their counters (gpemu_wide_path_counts)."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

import matern_nu_ref as MR
from oracle import gp_oracle as O

# enum gpemu_path (include/gpemu.h)
PATHS = ["KSTAR_SMALL", "KSTAR_BIG", "KSTAR_KSTEPS2", "KSTAR_KSTEPS3", "KSTAR_DIRECT",
         "TRMM_SMALL_44", "TRMM_SMALL_36", "TRMM_SMALL_XCD", "TRMM_SMALL_LEFTOVER", "TRMM_SMALL_FEW_ITEMS",
         "TRMM_SMALL_FALLBACK", "TRMM_DMA_LPT", "TRMM_DMA_XCD", "TRMM_DMA_WHOLE", "TRMM_DMA_PIECES",
         "HALFSTEP_SMALL", "HALFSTEP_GENERAL", "LOGLIK_LOWRANK", "LOGLIK_GROUPS", "LOGLIK_TASKS_ONE",
         "LOGLIK_TASKS_MULTI", "LOGLIK_TASKS_MULTI_BIG", "PREDICT_PASS"]
PATH = {n: i for i, n in enumerate(PATHS)}
# enum gpemu_wide_path (include/gpemu.h): the 16-wide instances (d = 9 .. 16), read through gpemu_wide_path_counts
WIDE_PATHS = ["KSTAR_KSTEPS3", "KSTAR_KSTEPS4", "KSTAR_KSTEPS5", "FIT_KMAT", "FIT_GRAD"]
WIDE_PATH = {n: i for i, n in enumerate(WIDE_PATHS)}
DPAD = 8

EDGE_ROWS = (0, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256)
EDGE_COLS = (0, 31, 32, 63, 64, 127, 128)
MAX_CHUNK, KSTAR_SMALL_MAX, HS_NMAX, HS_COLS = 2048, 128, 256, 32


def rup(x, m):
    return (x + m - 1) // m * m


@dataclass
class Case:
    name: str            # the path the case is there for
    N: int
    d: int
    k: int
    B: int
    kind: int
    nu: float
    const: bool
    nblk: int = 1
    F: int = 0           # 0: k + 3 (at least nblk)
    # length scale 1e-5 on coordinate 0 and 1e5 on coordinate d - 1 (problem()).  The reference of such a case needs
    # hp_ref's input_rounding=True: without it the bound leaves out the rounding of the uncentred scaled coordinates,
    # which dominates at ls = 1e-5 (hp_ref docstring, "Limit")
    ls_bounds: bool = False

    @property
    def spec(self):
        return O.KernelSpec(kind=self.kind, nu=self.nu, has_const=self.const, has_noise=True)

    @property
    def general_nu(self):
        return self.kind == O.MATERN and self.nu not in (0.5, 1.5, 2.5) and not np.isinf(self.nu)


def cases(num_cu=256):
    """the sweep; the shapes of the <3, 6> and left-over cases follow from the CU count"""
    R, M = O.RBF, O.MATERN
    # <3, 6>: at least 5 num_cu items of (PC, 32-row block, 32-column block) at 128 columns and 10 PCs
    n36 = rup(32 * math.ceil(5 * num_cu / (10 * 4)), 128) - 5
    # every group left over: fewer than 8 (PC, column block) groups, at least num_cu items (1 PC, 4 column blocks)
    nleft = rup(32 * math.ceil(num_cu / 4), 128) - 3
    return [
        Case("n1_few_items", 1, 1, 1, 1, R, np.inf, False),
        Case("n15_d8_ksteps3_m05", 15, 8, 4, 31, M, 0.5, False),
        Case("n16_d7_m15_const", 16, 7, 5, 32, M, 1.5, True),
        Case("n17_d1_m25", 17, 1, 4, 33, M, 2.5, False),
        Case("n63_nu075_direct", 63, 3, 16, 64, M, 0.75, False),
        Case("n64_nu2_const", 64, 2, 17, 127, M, 2.0, True),
        Case("n65_halfstep_small_xcd", 65, 4, 32, 128, R, np.inf, False, nblk=2),
        Case("n64_k33_lds", 64, 3, 33, 33, M, 2.5, False, nblk=2, F=40),
        Case("n255_kstar_big_lpt", 255, 6, 4, 129, R, np.inf, True),
        Case("n256_hs_edge", 256, 5, 16, 100, M, 1.5, False),
        Case("n257_hs_general_dma_lpt", 257, 5, 16, 100, M, 1.5, False),
        Case("n257_b300_k3_lpt", 257, 6, 3, 300, R, np.inf, False),
        Case("n300_tasks_multi", 300, 3, 5, 256, M, 2.5, True, nblk=6),
        Case("n300_b257_blocks_serial", 300, 3, 5, 257, M, 2.5, False, nblk=4),
        Case("n1000_b512_tasks_big", 1000, 6, 10, 512, R, np.inf, False, nblk=10),
        Case("n300_b513_whole", 300, 2, 4, 513, M, 0.5, False),
        Case("n300_b1024_pieces", 300, 3, 4, 1024, M, 2.5, False),
        Case("n100_b2049_two_passes", 100, 2, 2, 2049, R, np.inf, True, nblk=2),
        Case("small_36", n36, 6, 10, 128, R, np.inf, False, nblk=2),
        Case("small_leftover", nleft, 3, 1, 128, M, 1.5, False),
        Case("n100_blocks65_fallback", 100, 2, 4, 64, R, np.inf, False, nblk=65, F=70),
        # 9 .. 16 parameters: rows padded to 16, 3 .. 5 MFMA k-steps; shapes fixed (no CU count), every special fits
        Case("w9_ks3_m05_small_lowrank", 40, 9, 3, 100, M, 0.5, False),
        Case("w11_ks3_rbf_const_big_tasks_one", 130, 11, 4, 200, R, np.inf, True, nblk=3),
        Case("w12_ks4_nu075_direct_tasks_multi", 64, 12, 5, 128, M, 0.75, False, nblk=6),
        Case("w15_ks4_m25_big_dma", 100, 15, 3, 160, M, 2.5, False),
        Case("w16_ks5_m15_pieces_tasks_big", 200, 16, 4, 768, M, 1.5, False, nblk=8),
        Case("w16_ks5_m05_direct_small", 50, 16, 2, 96, M, 0.5, False),
        Case("w16_ks5_rbf_const_two_passes", 60, 16, 2, 2100, R, np.inf, True, nblk=2),
        Case("w13_ks4_m15_lsb_big", 90, 13, 3, 150, M, 1.5, False, ls_bounds=True),
        Case("w10_ks3_m05_lsb_direct_small", 48, 10, 2, 80, M, 0.5, False, ls_bounds=True),
    ]


# ---- the dispatch rules, restated --------------------------------------------------------------------------------------
def _trmm_small(c, nb, num_cu, out):
    Npad = rup(c.N, 128)
    nrb, ncb = Npad // 32, math.ceil(nb / 32)
    nitems = nrb * c.k * ncb
    wpc = 3 if nitems >= 5 * num_cu else 2 if nitems >= 2 * num_cu else 1
    ncu = num_cu * wpc
    nworkers = min(ncu, nitems)
    if nworkers < ncu:
        out.add("TRMM_SMALL_FEW_ITEMS")
    elif ncu % 8 == 0 and c.k * ncb >= 8:
        out.add("TRMM_SMALL_XCD")
    else:
        out.add("TRMM_SMALL_LEFTOVER")
    out.add("TRMM_SMALL_36" if nworkers > 2 * num_cu else "TRMM_SMALL_44")


def _trmm_dma(c, cols, num_cu, out):
    nrb, ncb = rup(c.N, 128) // 64, math.ceil(cols / 128)
    split_below = nrb if ncb <= 2 else nrb // 4
    items = c.k * ncb * (nrb + split_below)
    xcd = min(items, num_cu) == num_cu and num_cu % 8 == 0 and (c.k * ncb) % 8 == 0
    out.add("TRMM_DMA_XCD" if xcd else "TRMM_DMA_LPT")


def predict_paths(c, num_cu):
    """paths gpemu_gp_predict(B) takes"""
    out = {"PREDICT_PASS"}
    for off in range(0, c.B, MAX_CHUNK):
        nb = min(MAX_CHUNK, c.B - off)
        out.add("KSTAR_SMALL" if nb <= KSTAR_SMALL_MAX else "KSTAR_BIG")
        if c.d <= DPAD:                                     # 16-wide instances: wide_paths
            out.add("KSTAR_KSTEPS2" if c.d + 1 <= 8 else "KSTAR_KSTEPS3")
        if c.kind == O.MATERN and c.nu < 1.0:
            out.add("KSTAR_DIRECT")
        n = math.ceil(nb / 512)
        per = rup(math.ceil(nb / n), 128)
        last = nb - (n - 1) * per
        if nb > 512 and last > 0 and rup(last, 128) == per:
            out.add("TRMM_DMA_PIECES")
            _trmm_dma(c, per, num_cu, out)
        elif nb <= 128:
            _trmm_small(c, nb, num_cu, out)
        else:
            out.add("TRMM_DMA_WHOLE")
            _trmm_dma(c, nb, num_cu, out)
    return out


def kstar_ksteps(d):
    """MFMA k-steps of the cross-kernel (kstar_host.h: kstar_ksteps)"""
    return 2 if d + 1 <= 8 else (d + 4) // 4


def wide_paths(c):
    """exact increments of gpemu_wide_path_counts and of the 8-wide KSTAR_KSTEPS2 / 3 counters in one gp_predict, or
    one logpost (mode 0), of B rows: one cross-kernel launch per pass of MAX_CHUNK rows, counted by its width and
    k-steps (k_predict.hip: kstar_count)"""
    passes = math.ceil(c.B / MAX_CHUNK)
    out = {"WIDE_" + p: 0 for p in WIDE_PATHS}
    out["KSTAR_KSTEPS2"] = out["KSTAR_KSTEPS3"] = 0
    ks = kstar_ksteps(c.d)
    if c.d > DPAD:
        out[f"WIDE_KSTAR_KSTEPS{ks}"] = passes
    else:
        out[f"KSTAR_KSTEPS{ks}"] = passes
    return out


def logpost_paths(c, num_cu):
    """the half-step and likelihood paths gpemu_logpost(B, mode 0) takes"""
    out = set()
    for off in range(0, c.B, MAX_CHUNK):
        nb = min(MAX_CHUNK, c.B - off)
        hs = (rup(c.N, 128) <= HS_NMAX and c.k <= 32 and c.d + 1 <= 8 and nb <= 128
              and c.k * math.ceil(nb / HS_COLS) >= 64)
        out.add("HALFSTEP_SMALL" if hs else "HALFSTEP_GENERAL")
        tasks = c.nblk > 1 and c.k <= 32 and c.nblk <= 64 and not (nb > 256 and c.nblk < 8)
        if tasks:
            nwg = math.ceil(c.nblk / 4)
            out.add("LOGLIK_TASKS_ONE" if nwg == 1 else "LOGLIK_TASKS_MULTI_BIG" if nb > 256 else "LOGLIK_TASKS_MULTI")
        else:
            out.add("LOGLIK_LOWRANK")
    return out


# ---- models and queries --------------------------------------------------------------------------------------------------
def problem(c, seed=0, ls_bounds=None):
    """(model, lo, hi, y_exp, y_err, block_start, rng): noise >= 1e-2 in every PC.  ls_bounds (default: the case's):
    every PC's length scale of coordinate 0 at 1e-5 and of coordinate d - 1 at 1e5, sklearn's default bounds"""
    ls_bounds = c.ls_bounds if ls_bounds is None else ls_bounds
    rng = np.random.default_rng(seed + 7919 * c.N + 104729 * c.k + c.B)
    d = c.d
    lo = rng.uniform(-2.0, 0.0, d)
    hi = lo + rng.uniform(0.5, 3.0, d)
    design = rng.uniform(lo, hi, (c.N, d))
    F = c.F or max(c.k + 3, c.nblk)
    Wm = rng.normal(size=(d, F))
    Y = np.tanh(((design - lo) / (hi - lo)) @ Wm) + 0.05 * rng.normal(size=(c.N, F))
    mean, scale, _ = O.scaler_fit(Y)
    with np.errstate(invalid="ignore"):                     # one design point: 0 / 0 explained variance
        pca = O.pca_fit((Y - mean) / scale)
    pca["explained_variance"] = np.nan_to_num(pca["explained_variance"])
    k = min(c.k, pca["components"].shape[0])
    assert k == c.k, (c.name, k)
    gps = []
    for i in range(k):
        th = [np.log((hi - lo) * rng.uniform(0.3, 1.5, d))]
        if ls_bounds:
            th[0][0], th[0][d - 1] = np.log(1e-5), np.log(1e5)
        if c.const:
            th.append(np.log(rng.uniform(0.1, 2.0, 1)))
        th.append(np.log(rng.uniform(1e-2, 5e-2, 1)))
        with MR.general_nu():
            gps.append(O.gp_fit_at_theta(design, pca["Y_pca"][:, i], np.concatenate(th), c.spec, 1e-10))
    model = O.GroupModel(X_train=design, spec=c.spec, gps=gps, components=pca["components"],
                         explained_variance=pca["explained_variance"], scaler_mean=mean, scaler_scale=scale, n_pc=k)
    y_exp = Y[0] + 0.05
    y_err = rng.uniform(0.02, 0.2, F)
    cuts = np.sort(rng.choice(np.arange(1, F), size=c.nblk - 1, replace=False)) if c.nblk > 1 else np.array([], int)
    block_start = np.concatenate([[0], cuts, [F]]).astype(np.int64)
    return model, lo, hi, y_exp, y_err, block_start, rng


def edge_rows(c):
    return sorted({r for r in EDGE_ROWS if r < c.N} | {c.N - 1})


def repeat_cols(c):
    return sorted({cc for cc in EDGE_COLS if cc < c.B} | {c.B - 1})


def special_count(c):
    """(specials queries() places, free columns it has for them): specials beyond the free columns are dropped, the
    box-edge walkers of the last coordinates first"""
    n = 2 * len(edge_rows(c)) + (5 if c.general_nu else 0) + 1 + c.d
    return n, c.B - len(repeat_cols(c))


def queries(c, model, lo, hi, rng):
    """(Xq [B, d], repeat_cols, ref_cols): adversarial queries (training rows at the tile edges, 1e-7 ls beside them,
    the t = 2 switch of the general-nu Bessel routine, far outside the design, one query repeated at the edge columns,
    walkers on the box edge) on a background of random ones; ref_cols holds every special column"""
    B, d, X = c.B, c.d, model.X_train
    ls = model.gps[0].ls
    Xq = rng.uniform(lo, hi, (B, d))
    special = []
    for r in edge_rows(c):
        special.append(X[r].copy())
        special.append(X[r] + 1e-7 * ls * rng.choice([-1.0, 1.0], d))
    if c.general_nu:
        rr = 2.0 / math.sqrt(2 * c.nu)                      # t = sqrt(2 nu) r = 2
        for f in (1 - 1e-9, 1 - 1e-3, 1.0, 1 + 1e-3, 1 + 1e-9):
            q = X[c.N // 2].copy()
            q[0] += f * rr * ls[0]
            special.append(q)
    special.append(hi + 50.0 * (hi - lo))                   # far out: k_* underflows to 0
    for j in range(d):                                      # on the box edge (a prior edge: -inf in the likelihood)
        q = 0.5 * (lo + hi)
        q[j] = lo[j] if j % 2 == 0 else hi[j]
        special.append(q)
    rep_cols = repeat_cols(c)
    q_rep = X[min(c.N - 1, 16)] + 1e-7 * ls
    for cc in rep_cols:
        Xq[cc] = q_rep
    free = [i for i in range(B) if i not in set(rep_cols)]
    sp_cols = []
    for q, i in zip(special, free):
        Xq[i] = q
        sp_cols.append(i)
    extra = [i for i in free[len(sp_cols):]][:: max(1, (B - len(sp_cols)) // 8)][:8]
    ref_cols = np.array(sorted(set(rep_cols) | set(sp_cols) | set(extra)), dtype=np.int64)
    return Xq, np.array(rep_cols, dtype=np.int64), ref_cols
