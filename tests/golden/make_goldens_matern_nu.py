#!/usr/bin/env python3
"""Golden vectors of the Matern kernel of general smoothness nu (g8_matern_nu_*.npz) by RUNNING THE REFERENCE.

Run in the build container only (needs the reference's sources and scikit-learn), in the manner of make_goldens.py,
whose helpers it uses (the reference's own ``fit_emulator_group``, ``predict_emulation_group``,
``compute_emulator_group_cov_unexplained``, ``predict`` and ``log_posterior``):

    python tests/golden/make_goldens_matern_nu.py          # writes tests/golden/g8_matern_nu_*.npz

Only numeric arrays are written.  Cases: one emulation group (Matern nu + constant + white noise) for nu in
{0.75, 2.0, 3.5, inf}, and three groups at nu = 2.0 (the small-emulator launch).  The prediction queries are walkers
in the box, rows ON training points (where the Matern with nu < 1 is not flat) and rows far outside the design
(where every kernel value is 0).
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as MG  # noqa: E402  (puts the reference on the path; its helpers run the reference)
from gpemu import synthetic  # noqa: E402

NUS = {"0p75": 0.75, "2p0": 2.0, "3p5": 3.5, "inf": np.inf}


def kernels(nu):
    return {
        "matern": {"length_scale_bounds_factor": [0.01, 100], "nu": float(nu)},
        "constant": {"constant_value": 1.0, "constant_value_bounds": [1e-3, 1e3]},
        "noise": {"type": "white", "args": {"noise_level": 0.1, "noise_level_bounds": [1e-3, 1e1]}},
    }


def queries(design, lo, hi, n_box=24, seed=1):
    """walkers in the box, 6 training points exactly, 2 rows far outside the design"""
    Xb = synthetic.make_walkers(n_box, seed=seed, lo=lo, hi=hi)
    far = np.stack([hi + 50.0 * (hi - lo), lo - 80.0 * (hi - lo)])
    return np.concatenate([Xb, design[[0, 3, 7, 11, 20, 41]], far])


def golden_single(tag, nu, N=90, F=30, k=4, n_restarts=2, seed=5):
    prob = synthetic.make_problem(N, F, seed=seed)
    lo, hi = prob["lo"], prob["hi"]
    active = kernels(nu)
    cfg = MG.GroupCfg(k, lo, hi, active, n_restarts)
    np.random.seed(2468)  # restarts draw from the global RNG (sklearn _gpr.py:327)
    res = MG.fit_with_reference(prob["Y"], prob["design"], cfg)
    Xq = queries(prob["design"], lo, hi)
    out = dict(Y=prob["Y"], design=prob["design"], lo=lo, hi=hi, gpr_alpha=np.float64(cfg.alpha),
               n_restarts=np.int64(n_restarts))
    out.update(MG.kernel_spec(active))
    out.update(MG.pack_fit(res, cfg))
    out.update(MG.pack_predict(res, cfg, Xq))
    # the kernel matrix of the fitted kernel_ of PC 0 (with its constant and noise), as sklearn forms it
    out["kernel_matrix_pc0"] = res["emulators"][0].kernel_(prob["design"])
    emu_cfg = MG.EmuCfg({"g": cfg}, MG.TrivialSort("g"))
    Xw = synthetic.make_walkers(24, seed=1, lo=lo, hi=hi)
    out["Xw"] = Xw
    out.update(MG.pack_logpost({"g": res}, emu_cfg, lo, hi, prob["y_exp"], prob["y_err"], Xw))
    MG.save(f"{tag}.npz", **out)


def golden_three_groups(tag, nu=2.0, N=80, F=30, seed=9):
    prob = synthetic.make_problem(N, F, seed=seed)
    lo, hi = prob["lo"], prob["hi"]
    cols = {"g1": np.r_[0:10], "g2": np.r_[10:18], "g3": np.r_[18:30]}
    mapping = {"A": ("g1", slice(0, 10), slice(0, 10)),
               "B": ("g2", slice(10, 18), slice(0, 8)),
               "C": ("g3", slice(18, 30), slice(0, 12))}
    sorter = MG.emulation.SortEmulationGroupObservables(emulation_group_to_observable_matrix=mapping, shape=(N, F))
    cfgs = {g: MG.GroupCfg(kk, lo, hi, kernels(nu), 1) for g, kk in (("g1", 3), ("g2", 3), ("g3", 4))}
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
    Xw = synthetic.make_walkers(24, seed=1, lo=lo, hi=hi)
    out["Xw"] = Xw
    out.update(MG.pack_logpost(res, emu_cfg, lo, hi, prob["y_exp"], prob["y_err"], Xw))
    MG.save(f"{tag}.npz", **out)


if __name__ == "__main__":
    for name, nu in NUS.items():
        golden_single(f"g8_matern_nu_{name}", nu)
    golden_three_groups("g8_matern_nu_3groups")
