#!/usr/bin/env python3
"""Cost of correlated experimental uncertainties: microseconds per sampler step with S fully
correlated sources (S = 0: today's path) and with / without exponential correlation inside the observables, on
  1. the shipped three-group shape (golden G7), 200 walkers;
  2. the C3 fixed-theta shape (oracle.workloads.fixed_theta_model(1000, 500, 10), one observable), 1024 walkers.
Samplers of one shape alternate in the same process; medians of `reps` runs of `steps` steps.
python tools/time_srccorr.py [steps] [reps]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import golden_util as GU  # noqa: E402
import srccorr_ref as R  # noqa: E402
from gpemu.sampler import DeviceSampler  # noqa: E402
from oracle import workloads  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
VARIANTS = [(S, corr) for corr in (False, True) for S in (0, 4, 16)]


def run_shape(label, groups, y, y_err, lo, hi, obs, W):
    """groups: [(GroupModel, columns, block starts)]"""
    rng = np.random.default_rng(1)
    start = rng.uniform(lo, hi, (W, lo.size))
    samplers, models = {}, []
    for S, corr in VARIANTS:
        cov = R.within_cov(y_err, obs) if corr else None
        src = R.sources(y_err, S, seed=5) if S else None
        dms = []
        for model, cols, bs in groups:
            dm = GU.device_model(model)
            kw = {}
            if cov is not None:
                kw["cov"] = cov[np.ix_(cols, cols)]
            if src is not None:
                kw["sys_sources"] = src[:, cols]
            dm.likelihood_setup(y[cols], y_err[cols], lo, hi, 1.0, block_start=bs, **kw)
            dms.append(dm)
        models += dms
        s = DeviceSampler(dms, W, seed=3)
        s.set_state(start)
        s.run(20, store=True)
        s.reset()
        samplers[(S, corr)] = s
    sync = models[0].sync
    times = {key: [] for key in samplers}
    for _ in range(reps):
        for key, s in samplers.items():
            sync()
            t0 = time.perf_counter()
            s.run(steps, store=True)
            sync()
            times[key].append((time.perf_counter() - t0) / steps * 1e6)
            s.reset()
    base = float(np.median(times[(0, False)]))
    for (S, corr), v in times.items():
        med = float(np.median(v))
        print(f"{label}: S = {S:2d}, within-observable correlation {'yes' if corr else 'no '}: {med:9.1f} us per step "
              f"(median of {reps} x {steps} steps; {100.0 * (med / base - 1.0):+7.1f} % against S = 0 without)",
              flush=True)
    for s in samplers.values():
        s.close()
    for m in models:
        m.close()


c = R.case("G7")
run_shape("G7 W=200", c["groups"], c["y"], c["y_err"], c["lo"], c["hi"], c["obs"], 200)

model, prob, _ = workloads.fixed_theta_model(1000, 500, 10)
F = prob["y_exp"].shape[0]
run_shape("C3 W=1024", [(model, np.arange(F), [0, F])], prob["y_exp"], prob["y_err"], prob["lo"], prob["hi"],
          np.zeros(F, dtype=np.int64), 1024)
