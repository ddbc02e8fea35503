#!/usr/bin/env python3
"""The sequential-design criterion (gpemu.design) on the C3 model (N = 1000, d = 6, k = 10 PCs) with
S = 4096 reference rows and M = 2048 candidates: the first-round scores, one conditioning step and a 16-point select,
against the unfused composition of the calls that were there before -- gpemu_gp_predict_cov_dev in its two-set form
(which writes the k x S x M covariance, 671 MB) and a torch square-and-sum over the reference rows (the numerator only:
the unfused side is not charged for the denominators).

The two routes alternate in one process after a warm-up; every call waits for its stream before it returns, so the
figures are wall times of synchronous calls (median, minimum and maximum over the repeats).  The score kernel's own time
comes from a separate `rocprofv3 --kernel-trace --stats` run of this script.
    python tools/time_design.py [repeats]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from gpemu import design as DS  # noqa: E402
from gpemu import synthetic  # noqa: E402
from gpemu.model import DeviceModel  # noqa: E402

PEAK_TF = 78.6   # fp64 MFMA peak of the MI355X
S, M, Q = 4096, 2048, 16
reps = max(10, int(sys.argv[1])) if len(sys.argv) > 1 else 12

wl = bench.build_workload(0, 1000, 500, 10, seed=0)
prob = wl["prob"]
dm = DeviceModel(X_train=prob["design"], ls=wl["ls"], alpha=wl["alpha"], L=wl["L"], components=wl["components"],
                 scaler_mean=wl["mean"], scaler_scale=wl["scale"], kernel_kind=0, noise=wl["noise"], device=0)
N, k = dm.N, dm.k
Xref = synthetic.make_walkers(S, seed=5)
Xcand = synthetic.make_walkers(M, seed=6)
dR = torch.tensor(Xref, dtype=torch.float64, device="cuda:0")
dC = torch.tensor(Xcand, dtype=torch.float64, device="cuda:0")
cov = torch.empty((k, S, M), dtype=torch.float64, device="cuda:0")
torch.cuda.synchronize()


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def unfused():
    dm.gp_predict_cov_dev(dR.data_ptr(), S, dC.data_ptr(), M, 0, cov.data_ptr(), stream=0)
    num = (cov * cov).sum(dim=1) / S
    torch.cuda.synchronize()
    return num


def stats(name, ms, flop=None):
    row = {"what": name, "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
           "max_ms": round(max(ms), 3), "repeats": len(ms)}
    if flop:
        tf = flop / statistics.median(ms) / 1e9
        row.update(gflop=round(flop / 1e9, 1), tflops=round(tf, 2), frac_peak=round(tf / PEAK_TF, 3))
    print(json.dumps(row), flush=True)
    return row


ds = DS.Design([dm], Xref, Xcand, max_picks=Q)
ds.scores()
num = unfused()          # warm-up of both routes (workspaces, code objects)
# the two numerators agree (the fused one is not returned: compare through the scores of a unit denominator instead)
t_create, t_scores, t_unfused, t_cond, t_select = [], [], [], [], []
for r in range(reps):
    t_scores.append(timed(ds.scores)[0])
    t_unfused.append(timed(unfused)[0])
for r in range(reps):
    ms, one = timed(lambda: DS.Design([dm], Xref, Xcand, max_picks=Q))
    t_create.append(ms)
    s = one.scores()
    t_cond.append(timed(lambda: one.condition(int(np.argmax(s))))[0])
    one.close()
    one = DS.Design([dm], Xref, Xcand, max_picks=Q)
    t_select.append(timed(lambda: one.select(Q))[0])
    one.close()
flop = 2.0 * k * N * S * M
print(json.dumps({"N": N, "d": dm.d, "k": k, "S": S, "M": M, "picks": Q, "device": torch.cuda.get_device_name(0)}))
stats("create (V of both sets, den_0, IV_0)", t_create, 2.0 * k * N * N * (S + M) / 2)
a = stats("fused first-round scores", t_scores, flop)
b = stats("unfused: predict_cov two-set + torch square-and-sum", t_unfused, flop)
stats("one conditioning step", t_cond)
stats(f"select({Q}) (scores + condition, {Q} rounds)", t_select)
print(json.dumps({"unfused_over_fused": round(b["median_ms"] / a["median_ms"], 3)}))
ds.close()
dm.close()
