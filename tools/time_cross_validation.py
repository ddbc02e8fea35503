#!/usr/bin/env python3
"""Cost of cross-validation at the fitted hyper-parameters (gpemu_model_cross_validate, csrc/k_cv.hip):
  * C3 (N = 1000, 500 observables, 10 PCs) with k = 5, k = 10 and leave-one-out,
  * the shipped three-group shape of golden G7 (N = 200; 5 + 11 + 25 PCs), k = 5 for each group,
  * C5 (N = 5000, 500 observables, 10 PCs), k = 5.
Per case: the time of one whole call (host arrays in and out, the device workspace allocated and freed), median of
R calls after a warm-up, by HIP events on the current stream and by the host clock.  Models are built by the product's
own device fit path (bench.build_workload), as bench.py does.
    python tools/time_cross_validation.py                # every case
    python tools/time_cross_validation.py c3_k5          # one case (for a rocprofv3 --kernel-trace --stats run)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from gpemu.model import DeviceModel  # noqa: E402


def kfold(N, k):
    sizes = np.full(k, N // k)
    sizes[:N % k] += 1
    return np.repeat(np.arange(k, dtype=np.int32), sizes)


def synthetic_model(N, k_pc, seed=0):
    wl = bench.build_workload(0, N, 500, k_pc, seed=seed)
    prob = wl["prob"]
    dm = DeviceModel(X_train=prob["design"], ls=wl["ls"], alpha=wl["alpha"], L=wl["L"], components=wl["components"],
                     scaler_mean=wl["mean"], scaler_scale=wl["scale"], kernel_kind=0, noise=wl["noise"],
                     cov_unexplained=wl["cun"], device=0)
    y = np.stack([wl["L"][p] @ (wl["L"][p].T @ wl["alpha"][p]) for p in range(k_pc)], axis=1)   # K alpha
    return [(dm, y)]


def g7_models():
    import golden_util as GU
    g = GU.load("g7_shipped_config")
    out = []
    for name, model in GU.g7_models(g).items():
        out.append((GU.device_model(model), g[name + "_Y_pca_truncated"]))
    return out


def time_case(models, k_of, reps):
    def run():
        for dm, y in models:
            dm.cross_validate(y, kfold(y.shape[0], k_of(y.shape[0])))
    run()                                                     # warm-up (code objects, first allocations)
    ev, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        run()
        b.record()
        b.synchronize()
        host.append(time.perf_counter() - t0)
        ev.append(a.elapsed_time(b))
    return float(np.median(ev)), float(np.median(host)) * 1e3


CASES = {
    "c3_k5": (lambda: synthetic_model(1000, 10), lambda N: 5, 20),
    "c3_k10": (lambda: synthetic_model(1000, 10), lambda N: 10, 20),
    "c3_loo": (lambda: synthetic_model(1000, 10), lambda N: N, 20),
    "g7_k5": (g7_models, lambda N: 5, 20),
    "c5_k5": (lambda: synthetic_model(5000, 10), lambda N: 5, 5),
}


def main():
    torch.zeros(1, device="cuda")
    names = sys.argv[1:] or list(CASES)
    for name in names:
        build, k_of, reps = CASES[name]
        models = build()
        ev_ms, host_ms = time_case(models, k_of, reps)
        shape = " + ".join(f"N={y.shape[0]} PCs={y.shape[1]}" for _, y in models)
        print(f"{name:8s} {shape:40s} events {ev_ms:9.3f} ms   host {host_ms:9.3f} ms   (median of {reps})", flush=True)
        for dm, _ in models:
            dm.close()


if __name__ == "__main__":
    main()
