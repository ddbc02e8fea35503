#!/usr/bin/env python3
"""Time the global (Sobol') sensitivity against the route the package had without it.

    python tools/time_sobol.py [--n 65536] [--batches 16] [--shapes c3,shipped] [--repeats 5] [--new-only]

Shapes: C3 (N = 1000, F = 500, k = 10, d = 6; bench.build_workload) and the shipped three groups (golden G7).
(a) ``sobol_indices``: ``DeviceModel.sobol_moments_dev`` on base matrices resident on the device, on a stream of its
    own, plus ``indices_from_moments`` on the host.  Wall time of the whole call and the HIP-event time of its device
    part (events on that stream), after a warm-up, the median of ``--repeats``.
(b) the baseline, the route without the pick-freeze kernel on the same rows: ``DeviceModel.gp_predict`` over the
    (d + 2) n pick-freeze rows (it passes them through its K_* workspace in its largest blocks, 2048 rows) and the
    estimators reduced with numpy on the host.  Wall time, the same warm-up and repeats.
One JSON line per measurement and a summary per shape (the ratio, and the largest difference of the indices)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd"), os.path.join(ROOT, "tests")]


def pick_freeze_rows(A, B):
    import numpy as np
    n, d = A.shape
    X = np.empty((d + 2, n, d))
    X[0], X[1] = A, B
    for i in range(d):
        X[2 + i] = A
        X[2 + i, :, i] = B[:, i]
    return X


def baseline(dm, A, B):
    """gp_predict over the pick-freeze rows, the estimators with numpy in PC space (k x k forms per feature)"""
    import numpy as np
    comp, scale, smean = dm._projection
    n, d = A.shape
    Z = dm.gp_predict(pick_freeze_rows(A, B).reshape(-1, d))[0].reshape(d + 2, n, dm.k)
    z0 = np.concatenate([Z[0], Z[1]]).mean(axis=0)
    a, b, D = Z[0] - z0, Z[1] - z0, Z[2:] - Z[0]
    s2 = scale * scale
    quad = lambda X: np.einsum("pf,...pq,qf->...f", comp, X, comp) * s2
    V = quad((a.T @ a + b.T @ b) / (2 * n))
    S = quad(np.einsum("rp,irq->ipq", b, D) / n) / V
    T = quad(np.einsum("irp,irq->ipq", D, D) / n) / (2 * V)
    return {"first_order": S, "total": T, "variance": V}


def new_path(dm, dA, dB, n, T, stream):
    import torch
    from gpemu import sensitivity
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(stream)
    mom = dm.sobol_moments_dev(dA.data_ptr(), dB.data_ptr(), n, n_batches=T, stream=stream.cuda_stream)
    e1.record(stream)
    out = sensitivity.indices_from_moments(mom, *dm._projection)
    dt = time.perf_counter() - t0
    e1.synchronize()
    return dt, e0.elapsed_time(e1) * 1e-3, out


def models_of(shape):
    import numpy as np
    if shape == "c3":
        import bench
        from gpemu import model as M
        wl = bench.build_workload(0, 1000, 500, 10, seed=0)
        prob = wl["prob"]
        dm = M.DeviceModel(X_train=prob["design"], ls=wl["ls"], alpha=wl["alpha"], L=wl["L"], components=wl["components"],
                           scaler_mean=wl["mean"], scaler_scale=wl["scale"], kernel_kind=0, noise=wl["noise"],
                           cov_unexplained=wl["cun"], device=0)
        return {"c3": dm}, np.asarray(prob["lo"]), np.asarray(prob["hi"])
    import golden_util as GU
    g = GU.load("g7_shipped_config")
    return {name: GU.device_model(m) for name, m in GU.g7_models(g).items()}, np.asarray(g["lo"]), np.asarray(g["hi"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--shapes", default="c3,shipped")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--new-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from gpemu import sensitivity
    n, T = args.n, args.batches
    stream = torch.cuda.Stream(device="cuda:0")
    for shape in args.shapes.split(","):
        models, lo, hi = models_of(shape)
        A, B = sensitivity.base_samples(n, lo, hi, seed=0)
        dA, dB = torch.as_tensor(A, device="cuda:0"), torch.as_tensor(B, device="cuda:0")
        torch.cuda.synchronize()
        wall, dev, base = [], [], []
        new = old = None
        for rep in range(args.repeats + 1):                         # the first pass warms up
            c0 = sensitivity.sobol_path_counts()
            w = e = 0.0
            new = {}
            for name, dm in models.items():
                dt, de, new[name] = new_path(dm, dA, dB, n, T, stream)
                w, e = w + dt, e + de
            counters = dict(zip(sensitivity.SOBOL_PATHS, (sensitivity.sobol_path_counts() - c0).tolist()))
            if rep:
                wall.append(w)
                dev.append(e)
        rec = {"what": "sobol_indices", "shape": shape, "groups": len(models), "n": n, "n_batches": T,
               "wall_s": statistics.median(wall), "hip_event_s": statistics.median(dev), "wall_all_s": wall,
               "counters": counters}
        print(json.dumps(rec), flush=True)
        if not args.new_only:
            for rep in range(args.repeats + 1):
                t0 = time.perf_counter()
                old = {name: baseline(dm, A, B) for name, dm in models.items()}
                if rep:
                    base.append(time.perf_counter() - t0)
            brec = {"what": "baseline gp_predict + numpy", "shape": shape, "rows": (lo.size + 2) * n,
                    "wall_s": statistics.median(base), "wall_all_s": base}
            print(json.dumps(brec), flush=True)
            diff = max(float(np.nanmax(np.abs(new[g][key] - old[g][key]))) for g in models for key in ("first_order", "total"))
            print(json.dumps({"what": "summary", "shape": shape, "new_wall_s": rec["wall_s"],
                              "new_hip_event_s": rec["hip_event_s"], "baseline_wall_s": brec["wall_s"],
                              "ratio_baseline_over_new": brec["wall_s"] / rec["wall_s"], "max_index_diff": diff,
                              "faster": bool(rec["wall_s"] < brec["wall_s"])}), flush=True)
        for dm in models.values():
            dm.close()
        del dA, dB
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
