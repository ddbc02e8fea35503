#!/usr/bin/env python3
"""Cost of parallel tempering: milliseconds per step of a TemperedSampler against an untempered
stacked sampler with the same walker count, in the same process, alternated.
  1. C3 fixed-theta shape (oracle.workloads.fixed_theta_model(1000, 500, 10)), T = 8 rungs x 1024 walkers, against
     DeviceSampler with 8 stacked chains x 1024 (the difference is the beta and swap work);
  2. the shipped three-group shape (golden G7), T = 8 x 200, against 8 stacked chains x 200 and one chain of 200.
python tools/time_tempered.py [steps] [reps]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import golden_util as GU  # noqa: E402
from gpemu.sampler import DeviceSampler, TemperedSampler  # noqa: E402
from gpemu.tempering import geometric_ladder  # noqa: E402
from oracle import workloads  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
T = 8


def ms_per_step(s, sync, n):
    sync()
    t0 = time.perf_counter()
    s.run(n, store=True)
    sync()
    dt = (time.perf_counter() - t0) / n * 1e3
    s.reset()
    return dt


def compare(label, samplers, sync, starts):
    for name, s in samplers.items():
        s.set_state(starts[name])
        s.run(20, store=True)
        s.reset()
    times = {name: [] for name in samplers}
    for _ in range(reps):
        for name, s in samplers.items():
            times[name].append(ms_per_step(s, sync, steps))
    med = {name: float(np.median(v)) for name, v in times.items()}
    base = med["stacked"]
    for name, v in med.items():
        print(f"{label}: {name:>9s} {v:8.4f} ms per step (median of {reps} x {steps} steps; "
              f"{100.0 * (v / base - 1.0):+6.2f} % against the stacked sampler)", flush=True)
    ts = samplers["tempered"]
    ts.run(steps, store=True)
    print(f"{label}: swap acceptance {np.array2string(ts.tswap_acceptance_fraction, precision=3)}", flush=True)
    t0 = time.perf_counter()
    ts.mean_log_likelihood()
    print(f"{label}: mean_log_likelihood over {steps} steps {1e3 * (time.perf_counter() - t0):.3f} ms (host call)",
          flush=True)
    return med


rng = np.random.default_rng(1)
# 1. C3 fixed-theta shape
model, prob, _ = workloads.fixed_theta_model(1000, 500, 10)
dm1 = GU.device_model(model)
dm1.likelihood_setup(prob["y_exp"], prob["y_err"], prob["lo"], prob["hi"], 1.0)
dm8 = GU.device_model(model)
dm8.likelihood_setup(np.tile(prob["y_exp"], (T, 1)), prob["y_err"], prob["lo"], prob["hi"], 1.0)
Wc = 1024
start = rng.uniform(prob["lo"], prob["hi"], (T * Wc, prob["lo"].size))
samplers = {"tempered": TemperedSampler([dm1], Wc, geometric_ladder(T, 1e5), seed=3, swap_every=1),
            "stacked": DeviceSampler([dm8], Wc, seeds=[3 + t for t in range(T)])}
compare(f"C3 T={T} Wc={Wc}", samplers, dm1.sync, {"tempered": start, "stacked": start})
for s in samplers.values():
    s.close()
dm1.close()
dm8.close()

# 2. the shipped shape (G7)
g = GU.load("g7_shipped_config")
names, mapping, block_start, cols = GU.g7_groups(g)
one, eight = [], []
for n in names:
    m = GU.group_model(g, prefix=n + "_")
    a, b = GU.device_model(m), GU.device_model(m)
    a.likelihood_setup(g["y_exp"][cols[n]], g["y_err"][cols[n]], g["lo"], g["hi"], 1.0, block_start=block_start[n])
    b.likelihood_setup(np.tile(g["y_exp"][cols[n]], (T, 1)), g["y_err"][cols[n]], g["lo"], g["hi"], 1.0,
                       block_start=block_start[n])
    one.append(a)
    eight.append(b)
Wc = 200
start = rng.uniform(g["lo"], g["hi"], (T * Wc, len(g["lo"])))
samplers = {"tempered": TemperedSampler(one, Wc, geometric_ladder(T, 1e5), seed=5, swap_every=1),
            "stacked": DeviceSampler(eight, Wc, seeds=[5 + t for t in range(T)]),
            "one-chain": DeviceSampler(one, Wc, seed=5)}
compare(f"G7 T={T} W={Wc}", samplers, one[0].sync,
        {"tempered": start, "stacked": start, "one-chain": start[:Wc]})
for s in samplers.values():
    s.close()
for m in one + eight:
    m.close()
