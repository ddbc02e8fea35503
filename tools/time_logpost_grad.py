#!/usr/bin/env python3
"""Time value + gradient of the log-posterior against the value alone, on device buffers.

    python tools/time_logpost_grad.py [--baseline-library PATH] [--no-map]

Shapes: C3 (N = 1000, d = 6, 10 PCs, F = 500; one observable block and ten) at B = 64 and 1024 through the device-pointer
calls, and the shipped three-group shape (golden G7) at B = 32 and 200 through the host-buffer group calls (there is no
device-pointer group call: both sides carry the same small copies).  Per shape: a warm-up, then the median over blocks
of the mean time per call.  ``--baseline-library``: another build of libgpemu.so (the parent commit's), timed on the
value call in a child process of its own through GPEMU_LIBRARY; the condition the gradient has to meet is
``t(value + gradient) < (d + 1) t(baseline value)``, the cost of the cheapest finite-difference gradient.
Then ``find_map`` at C3 with 32 starts: wall time and the share spent inside the device calls.
One JSON line per measurement."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd"), os.path.join(ROOT, "tests")]

NEW = ("gpemu_gp_predict_grad", "gpemu_gp_predict_grad_dev", "gpemu_logpost_grad", "gpemu_logpost_grad_dev",
       "gpemu_logpost_groups_grad", "gpemu_grad_path_counts")
WARMUP, BLOCKS = 5, 7


def median_ms(call, sync, reps):
    for _ in range(WARMUP):
        call()
    sync()
    times = []
    for _ in range(BLOCKS):
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        sync()
        times.append((time.perf_counter() - t0) / reps * 1e3)
    times.sort()
    return times[len(times) // 2]


def run(value_only, do_map):
    import numpy as np
    import torch
    from gpemu import _lib
    if value_only:                       # an older build: bind what it has
        for name in NEW:
            _lib._SIGNATURES.pop(name, None)
    import bench
    import golden_util as GU
    from gpemu import model as M
    from gpemu import synthetic
    out = []
    wl = bench.build_workload(0, 1000, 500, 10, seed=0)
    prob = wl["prob"]
    dm = M.DeviceModel(X_train=prob["design"], ls=wl["ls"], alpha=wl["alpha"], L=wl["L"], components=wl["components"],
                       scaler_mean=wl["mean"], scaler_scale=wl["scale"], kernel_kind=0, noise=wl["noise"],
                       cov_unexplained=wl["cun"], device=0)
    d = prob["design"].shape[1]
    for nb in (1, 10):
        blocks = [int(round(i * 500 / nb)) for i in range(nb + 1)]
        dm.likelihood_setup(prob["y_exp"], prob["y_err"], prob["lo"], prob["hi"], 1.0, block_start=blocks if nb > 1 else None)
        for B in (64, 1024):
            X = torch.tensor(synthetic.make_walkers(B, seed=1), dtype=torch.float64, device="cuda:0")
            lp = torch.empty(B, dtype=torch.float64, device="cuda:0")
            gr = torch.empty((B, d), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            reps = 40 if B <= 64 else 10
            rec = {"shape": "C3", "blocks": nb, "B": B, "d": d,
                   "value_ms": median_ms(lambda: dm.logpost_dev(X.data_ptr(), B, lp.data_ptr(), stream=0), dm.sync, reps)}
            if not value_only:
                rec["value_grad_ms"] = median_ms(lambda: dm.logpost_grad_dev(X.data_ptr(), B, lp.data_ptr(), gr.data_ptr(), stream=0),
                                                 dm.sync, reps)
            out.append(rec)
            print(json.dumps(rec), flush=True)
    if do_map and not value_only:
        from gpemu import mapfit
        spent = [0.0, 0]

        def vg(Xh):
            t0 = time.perf_counter()
            r = dm.logpost_grad(Xh)
            spent[0] += time.perf_counter() - t0
            spent[1] += 1
            return r
        lo, hi = np.asarray(prob["lo"], float), np.asarray(prob["hi"], float)
        starts = np.random.default_rng(0).uniform(lo, hi, (32, d))
        t0 = time.perf_counter()
        found = mapfit.find_map(vg, starts, lo, hi)
        wall = time.perf_counter() - t0
        rec = {"shape": "C3 find_map", "blocks": 10, "starts": 32, "wall_s": wall, "device_calls": spent[1],
               "device_share": spent[0] / wall, "nfev_max": int(found["nfev"].max()), "status": found["status"].tolist(),
               "map_log_prob": found["map_log_prob"]}
        print(json.dumps(rec), flush=True)
    dm.close()
    g = GU.load("g7_shipped_config")
    names, mapping, block_start, cols = GU.g7_groups(g)
    models = GU.g7_models(g)
    dms = []
    for n in names:
        m = GU.device_model(models[n])
        m.likelihood_setup(g["y_exp"][cols[n]], g["y_err"][cols[n]], g["lo"], g["hi"], 1.0, block_start=block_start[n])
        dms.append(m)
    rng = np.random.default_rng(1)
    for B in (32, 200):
        X = rng.uniform(g["lo"], g["hi"], (B, len(g["lo"])))
        rec = {"shape": "G7 three groups (host buffers)", "B": B, "d": int(len(g["lo"])),
               "value_ms": median_ms(lambda: M.logpost_groups(dms, X), dms[0].sync, 20)}
        if not value_only:
            rec["value_grad_ms"] = median_ms(lambda: M.logpost_groups_grad(dms, X), dms[0].sync, 20)
        out.append(rec)
        print(json.dumps(rec), flush=True)
    for m in dms:
        m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-library", default=None)
    ap.add_argument("--value-only", action="store_true", help="(the child process of --baseline-library)")
    ap.add_argument("--no-map", action="store_true")
    args = ap.parse_args()
    if args.value_only:
        run(True, False)
        return
    base = {}
    if args.baseline_library:
        env = dict(os.environ, GPEMU_LIBRARY=os.path.abspath(args.baseline_library))
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--value-only"], env=env, capture_output=True,
                             text=True, timeout=900)
        if res.returncode != 0:
            raise SystemExit(f"baseline run failed ({res.returncode}):\n{res.stdout}\n{res.stderr}")
        for line in res.stdout.splitlines():
            if line.startswith("{"):
                r = json.loads(line)
                base[(r["shape"], r.get("blocks"), r["B"])] = r["value_ms"]
    for r in run(False, not args.no_map):
        b = base.get((r["shape"], r.get("blocks"), r["B"]))
        if b is not None:
            r["baseline_value_ms"] = b
            r["ratio_to_baseline_value"] = r["value_grad_ms"] / b
            r["fd_cost_ms"] = (r["d"] + 1) * b
            r["condition_met"] = bool(r["value_grad_ms"] < (r["d"] + 1) * b)
            print(json.dumps(dict(r, summary=True)), flush=True)


if __name__ == "__main__":
    main()
