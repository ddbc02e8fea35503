#!/usr/bin/env python3
"""Cost of the Matern kernel of general nu (csrc/matern_dev.h) against the closed form nu = 2.5 and nu = inf (RBF):
  * us per sampler step at C3 (N = 1000, 500 observables, 10 PCs, 1024 walkers),
  * us per step at the shipped three-group shape (N = 150; 5 / 11 / 25 PCs; 200 walkers),
  * one N = 1000 LML + gradient (10 PCs' worth of calls, timed one by one).
Each model is built with the product's own device fit at the kernel being timed (bench.build_workload).
    python tools/time_matern_nu.py              # everything
    python tools/time_matern_nu.py c3 2.0       # C3 sampler only, one nu (for a rocprofv3 kernel trace)
GPEMU_LIBRARY selects another build of the library (A/B of a kernel variant)."""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd")]
import numpy as np  # noqa: E402

import bench  # noqa: E402
from gpemu import synthetic  # noqa: E402
from gpemu.fit import DeviceFit  # noqa: E402
from gpemu.model import DeviceModel  # noqa: E402
from gpemu.sampler import DeviceSampler  # noqa: E402

NUS = [2.5, 2.0, 0.75, math.inf]


def models(shapes, nu):
    dms = []
    for gi, (N, F, k) in enumerate(shapes):
        wl = bench.build_workload(0, N, F, k, seed=gi, kernel_kind=1, nu=nu)
        prob = wl["prob"]
        dm = DeviceModel(X_train=prob["design"], ls=wl["ls"], alpha=wl["alpha"], L=wl["L"], components=wl["components"],
                         scaler_mean=wl["mean"], scaler_scale=wl["scale"], kernel_kind=1, nu=nu, noise=wl["noise"],
                         cov_unexplained=wl["cun"], device=0)
        dm.likelihood_setup(prob["y_exp"], prob["y_err"], prob["lo"], prob["hi"], 1.0)
        dms.append(dm)
    return dms


def us_per_step(dms, W, warm, steps):
    ds = DeviceSampler(dms, W, seed=11)
    ds.set_state(synthetic.make_walkers(W, seed=3))
    ds.run(warm, store=False)
    dms[0].sync()
    t0 = time.perf_counter()
    ds.run(steps, store=False)
    dms[0].sync()
    dt = time.perf_counter() - t0
    lp = ds.get_state()[1]
    ds.close()
    assert np.all(np.isfinite(lp)), "non-finite log-probability in the ensemble"
    return dt / steps * 1e6


def lml_grad_us(nu, reps=10):
    prob = synthetic.make_problem(1000, 50, seed=0)
    y = prob["Y"][:, 0] - prob["Y"][:, 0].mean()
    theta = np.log(np.r_[(prob["hi"] - prob["lo"]) * 0.5, 0.05])
    f = DeviceFit(prob["design"], 1, nu, has_noise=True, jitter=1e-10)
    f.lml(y, theta)
    t0 = time.perf_counter()
    for _ in range(reps):
        f.lml(y, theta)
    dt = (time.perf_counter() - t0) / reps
    f.close()
    return dt * 1e6


def main():
    lib = os.environ.get("GPEMU_LIBRARY", "in-tree build")
    if len(sys.argv) > 2 and sys.argv[1] == "c3":
        nu = float(sys.argv[2])
        dms = models([(1000, 500, 10)], nu)
        print(f"C3 nu={nu:g}: {us_per_step(dms, 1024, 20, 100):8.1f} us per step  [{lib}]", flush=True)
        for d in dms:
            d.close()
        return
    print(f"library: {lib}")
    for nu in NUS:
        dms = models([(1000, 500, 10)], nu)
        print(f"C3 (1000 x 500, 10 PCs, 1024 walkers)   nu={nu:<5g}: {us_per_step(dms, 1024, 20, 200):8.1f} us per step",
              flush=True)
        for d in dms:
            d.close()
    for nu in NUS:
        dms = models([(150, 60, 5), (150, 120, 11), (150, 215, 25)], nu)
        print(f"shipped three groups (150; 5/11/25, 200 walkers) nu={nu:<5g}: "
              f"{us_per_step(dms, 200, 200, 2000):8.1f} us per step", flush=True)
        for d in dms:
            d.close()
    for nu in NUS:
        print(f"LML + gradient, N = 1000, d = 6 + noise    nu={nu:<5g}: {lml_grad_us(nu):8.1f} us per call", flush=True)


if __name__ == "__main__":
    main()
