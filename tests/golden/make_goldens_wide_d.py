#!/usr/bin/env python3
"""Golden vectors of emulation groups with 9 to 16 parameters (g10_wide_d_*.npz) by RUNNING THE REFERENCE.

Run in the build container only (needs the reference's sources and scikit-learn), in the manner of make_goldens.py,
whose helpers it uses (the reference's own ``fit_emulator_group``, ``predict_emulation_group``,
``compute_emulator_group_cov_unexplained``, ``predict`` and ``log_posterior``):

    python tests/golden/make_goldens_wide_d.py          # writes tests/golden/g10_wide_d_*.npz

Only numeric arrays are written.  The product's synthetic generator has a fixed parameter count, so the boxes, designs
and observables of these cases are made here.  Cases: d = 10 RBF + constant + white noise, d = 16 Matern 2.5 + noise,
d = 12 Matern nu = 0.75 + constant + noise (the direct distance of near pairs), three emulation groups at d = 9.
The queries are walkers in the box, rows ON training points and rows far outside the design.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as MG  # noqa: E402  (puts the reference on the path; its helpers run the reference)

NOISE = {"type": "white", "args": {"noise_level": 0.1, "noise_level_bounds": [1e-3, 1e1]}}
CONST = {"constant_value": 1.0, "constant_value_bounds": [1e-3, 1e3]}
KERNELS = {
    "rbf_const_noise": {"rbf": {"length_scale_bounds_factor": [0.01, 100]}, "constant": CONST, "noise": NOISE},
    "matern25_noise": {"matern": {"length_scale_bounds_factor": [0.01, 100], "nu": 2.5}, "noise": NOISE},
    "nu0p75_const_noise": {"matern": {"length_scale_bounds_factor": [0.01, 100], "nu": 0.75}, "constant": CONST,
                           "noise": NOISE},
}


def make_problem(N, F, d, seed):
    """A d-parameter box, a uniform design in it, smooth observables of the design and a data vector."""
    rng = np.random.default_rng(seed)
    lo = -1.0 - rng.uniform(0.0, 2.0, d)
    hi = 1.0 + rng.uniform(0.0, 2.0, d)
    design = rng.uniform(lo, hi, (N, d))
    u = (design - lo) / (hi - lo)
    Wm = rng.normal(size=(d, F)) / np.sqrt(d)
    Y = np.exp(np.sin(2.0 * u @ Wm) + 0.3 * (u ** 2) @ np.abs(Wm)) + 0.01 * rng.normal(size=(N, F))
    truth = rng.uniform(lo + 0.3 * (hi - lo), hi - 0.3 * (hi - lo))
    ut = (truth - lo) / (hi - lo)
    y_true = np.exp(np.sin(2.0 * ut @ Wm) + 0.3 * (ut ** 2) @ np.abs(Wm))
    y_err = 0.05 * np.abs(y_true) + 0.01
    y_exp = y_true + y_err * rng.normal(size=F)
    return dict(design=design, Y=Y, lo=lo, hi=hi, y_exp=y_exp, y_err=y_err)


def walkers(n, lo, hi, seed):
    return np.random.default_rng(seed).uniform(lo, hi, (n, lo.size))


def queries(design, lo, hi, n_box=24, seed=1):
    """walkers in the box, 6 training points exactly, 2 rows far outside the design"""
    far = np.stack([hi + 50.0 * (hi - lo), lo - 80.0 * (hi - lo)])
    return np.concatenate([walkers(n_box, lo, hi, seed), design[[0, 3, 7, 11, 20, 41]], far])


def golden_single(tag, d, kern, N=120, F=30, k=4, n_restarts=1, seed=5):
    prob = make_problem(N, F, d, seed)
    lo, hi = prob["lo"], prob["hi"]
    active = KERNELS[kern]
    cfg = MG.GroupCfg(k, lo, hi, active, n_restarts)
    np.random.seed(2468)  # restarts draw from the global RNG (sklearn _gpr.py:327)
    res = MG.fit_with_reference(prob["Y"], prob["design"], cfg)
    Xq = queries(prob["design"], lo, hi)
    out = dict(Y=prob["Y"], design=prob["design"], lo=lo, hi=hi, gpr_alpha=np.float64(cfg.alpha),
               n_restarts=np.int64(n_restarts))
    out.update(MG.kernel_spec(active))
    out.update(MG.pack_fit(res, cfg))
    out.update(MG.pack_predict(res, cfg, Xq))
    out["kernel_matrix_pc0"] = res["emulators"][0].kernel_(prob["design"])
    emu_cfg = MG.EmuCfg({"g": cfg}, MG.TrivialSort("g"))
    Xw = walkers(24, lo, hi, 1)
    out["Xw"] = Xw
    out.update(MG.pack_logpost({"g": res}, emu_cfg, lo, hi, prob["y_exp"], prob["y_err"], Xw))
    MG.save(f"{tag}.npz", **out)


def golden_three_groups(tag, d=9, N=100, F=30, seed=9):
    prob = make_problem(N, F, d, seed)
    lo, hi = prob["lo"], prob["hi"]
    cols = {"g1": np.r_[0:10], "g2": np.r_[10:18], "g3": np.r_[18:30]}
    mapping = {"A": ("g1", slice(0, 10), slice(0, 10)),
               "B": ("g2", slice(10, 18), slice(0, 8)),
               "C": ("g3", slice(18, 30), slice(0, 12))}
    sorter = MG.emulation.SortEmulationGroupObservables(emulation_group_to_observable_matrix=mapping, shape=(N, F))
    cfgs = {g: MG.GroupCfg(kk, lo, hi, KERNELS["rbf_const_noise"], 1) for g, kk in (("g1", 3), ("g2", 3), ("g3", 4))}
    np.random.seed(1357)
    res = {g: MG.fit_with_reference(np.ascontiguousarray(prob["Y"][:, cols[g]]), prob["design"], cfgs[g])
           for g in cfgs}
    Xq = queries(prob["design"], lo, hi, n_box=16)
    emu_cfg = MG.EmuCfg(cfgs, sorter)
    merged = MG.emulation.predict(Xq, emu_cfg, emulation_group_results=res)
    out = dict(Y=prob["Y"], design=prob["design"], lo=lo, hi=hi, Xq=Xq, gpr_alpha=np.float64(1e-10),
               merged_central_value=merged["central_value"], merged_cov_head=merged["cov"][:2].copy())
    for g in cfgs:
        out[f"cols_{g}"] = cols[g].astype(np.int64)
        for kk, vv in {**MG.kernel_spec(cfgs[g].active_kernels), **MG.pack_fit(res[g], cfgs[g])}.items():
            out[f"{g}_{kk}"] = vv
    Xw = walkers(24, lo, hi, 1)
    out["Xw"] = Xw
    out.update(MG.pack_logpost(res, emu_cfg, lo, hi, prob["y_exp"], prob["y_err"], Xw))
    MG.save(f"{tag}.npz", **out)


if __name__ == "__main__":
    golden_single("g10_wide_d_rbf_const_noise_d10", 10, "rbf_const_noise")
    golden_single("g10_wide_d_matern25_d16", 16, "matern25_noise")
    golden_single("g10_wide_d_nu0p75_d12", 12, "nu0p75_const_noise")
    golden_three_groups("g10_wide_d_3groups_d9")
