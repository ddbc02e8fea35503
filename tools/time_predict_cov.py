#!/usr/bin/env python3
"""The joint predictive covariance (gpemu_gp_predict_cov_dev, symmetric form) on the C3 model (N = 1000, k = 10 PCs):
wall time per call on the device buffers for M query points, and the fraction of the fp64 matrix-core peak the call's
FLOPs (N^2 M for V = W K^T, N M^2 for the lower triangle of V^T V, per PC) would need.  The per-kernel split comes from
a separate `rocprofv3 --kernel-trace --stats` run of this script.   python tools/time_predict_cov.py [M ...]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd")]
import torch  # noqa: E402

import bench  # noqa: E402
from gpemu import synthetic  # noqa: E402
from gpemu.model import DeviceModel  # noqa: E402

PEAK_TF = 78.6   # fp64 MFMA peak of the MI355X
Ms = [int(a) for a in sys.argv[1:]] or [256, 2048, 4096]
wl = bench.build_workload(0, 1000, 500, 10, seed=0)
prob = wl["prob"]
dm = DeviceModel(X_train=prob["design"], ls=wl["ls"], alpha=wl["alpha"], L=wl["L"], components=wl["components"],
                 scaler_mean=wl["mean"], scaler_scale=wl["scale"], kernel_kind=0, noise=wl["noise"], device=0)
N, k = dm.N, dm.k
for M in Ms:
    X = torch.tensor(synthetic.make_walkers(M, seed=5), dtype=torch.float64, device="cuda:0")
    cov = torch.empty((k, M, M), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    dm.gp_predict_cov_dev(X.data_ptr(), M, 0, 0, 0, cov.data_ptr(), stream=0)   # warm-up (and the workspace's first allocation)
    dm.sync()
    reps = 20 if M <= 2048 else 8
    t0 = time.perf_counter()
    for _ in range(reps):
        dm.gp_predict_cov_dev(X.data_ptr(), M, 0, 0, 0, cov.data_ptr(), stream=0)
    dm.sync()
    ms = (time.perf_counter() - t0) / reps * 1e3
    flop = k * (N * N * M + N * M * M)
    print(json.dumps({"M": M, "N": N, "k": k, "ms_per_call": round(ms, 3), "gflop": round(flop / 1e9, 2),
                      "tflops": round(flop / ms / 1e9, 2), "frac_peak": round(flop / ms / 1e9 / PEAK_TF, 3)}))
dm.close()
