#!/usr/bin/env python3
"""Time the second-order Sobol' indices against the route the package had without them.

    python tools/time_sobol_pairs.py [--n 65536] [--batches 16] [--shapes c3,shipped] [--repeats 5] [--new-only]

Shapes: C3 (N = 1000, F = 500, k = 10, d = 6; bench.build_workload) and the shipped three groups (golden G7), all
pairs i < j.  Host base matrices, one warm-up, the median of ``--repeats``, wall time host to host:
(a) ``DeviceModel.sobol_indices(A, B, second_order=True)``: gpemu_sobol_moments_pairs and the float64 algebra;
(b) the baseline, the route without the pair kernel on the same rows, in the same process: ``DeviceModel.gp_predict``
    over the (d + 2 + P) n rows built explicitly and the estimators reduced with numpy;
(c) ``DeviceModel.sobol_indices(A, B)`` without the keyword (the first order alone), for the record.
One JSON line per measurement and a summary per shape (the ratio, and the largest difference of the indices)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd"), os.path.join(ROOT, "tests")]

from time_sobol import models_of, pick_freeze_rows  # noqa: E402  (tools/ is the script's directory)


def all_rows(A, B, pairs):
    import numpy as np
    X = np.empty((len(pairs),) + A.shape)
    for q, (i, j) in enumerate(pairs):
        X[q] = A
        X[q, :, i] = B[:, i]
        X[q, :, j] = B[:, j]
    return np.concatenate([pick_freeze_rows(A, B), X])


def baseline(dm, A, B, pairs):
    """gp_predict over all rows, the estimators with numpy in PC space (k x k forms per feature)"""
    import numpy as np
    comp, scale, smean = dm._projection
    n, d = A.shape
    X = all_rows(A, B, pairs)
    Z = dm.gp_predict(X.reshape(-1, d))[0].reshape(X.shape[0], n, dm.k)
    z0 = np.concatenate([Z[0], Z[1]]).mean(axis=0)
    a, b, D, D2 = Z[0] - z0, Z[1] - z0, Z[2:2 + d] - Z[0], Z[2 + d:] - Z[0]
    s2 = scale * scale
    quad = lambda M: np.einsum("pf,...pq,qf->...f", comp, M, comp) * s2
    V = quad((a.T @ a + b.T @ b) / (2 * n))
    S = quad(np.einsum("rp,irq->ipq", b, D) / n) / V
    Sc = quad(np.einsum("rp,irq->ipq", b, D2) / n) / V
    Tp = quad(np.einsum("irp,irq->ipq", D2, D2) / n) / (2 * V)
    return {"closed_pair": Sc, "interaction": Sc - S[pairs[:, 0]] - S[pairs[:, 1]], "total_pair": Tp}


def timed(fn, repeats):
    out, ts = None, []
    for rep in range(repeats + 1):                                   # the first pass warms up
        t0 = time.perf_counter()
        out = fn()
        if rep:
            ts.append(time.perf_counter() - t0)
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--shapes", default="c3,shipped")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--new-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    from gpemu import marginals, sensitivity
    n, T = args.n, args.batches
    for shape in args.shapes.split(","):
        models, lo, hi = models_of(shape)
        d = lo.size
        pairs = marginals.pair_indices(d)
        A, B = sensitivity.base_samples(n, lo, hi, seed=0)
        c0 = sensitivity.sobol_pairs_path_counts()
        new, wall = timed(lambda: {g: dm.sobol_indices(A, B, n_batches=T, second_order=True) for g, dm in models.items()},
                          args.repeats)
        counters = dict(zip(sensitivity.SOBOL_PAIRS_PATHS, (sensitivity.sobol_pairs_path_counts() - c0).tolist()))
        rec = {"what": "sobol_indices second_order", "shape": shape, "groups": len(models), "n": n, "n_batches": T,
               "pairs": len(pairs), "wall_s": statistics.median(wall), "wall_all_s": wall,
               "counters_all_passes": counters}
        print(json.dumps(rec), flush=True)
        _, first = timed(lambda: {g: dm.sobol_indices(A, B, n_batches=T) for g, dm in models.items()}, args.repeats)
        print(json.dumps({"what": "sobol_indices first order", "shape": shape, "wall_s": statistics.median(first),
                          "wall_all_s": first}), flush=True)
        if not args.new_only:
            old, base = timed(lambda: {g: baseline(dm, A, B, pairs) for g, dm in models.items()}, args.repeats)
            brec = {"what": "baseline gp_predict + numpy", "shape": shape, "rows": (d + 2 + len(pairs)) * n,
                    "wall_s": statistics.median(base), "wall_all_s": base}
            print(json.dumps(brec), flush=True)
            diff = max(float(np.nanmax(np.abs(new[g][key] - old[g][key]))) for g in models
                       for key in ("closed_pair", "interaction", "total_pair"))
            print(json.dumps({"what": "summary", "shape": shape, "new_wall_s": rec["wall_s"],
                              "first_order_wall_s": statistics.median(first), "baseline_wall_s": brec["wall_s"],
                              "ratio_baseline_over_new": brec["wall_s"] / rec["wall_s"], "max_index_diff": diff,
                              "faster": bool(rec["wall_s"] < brec["wall_s"])}), flush=True)
        for dm in models.values():
            dm.close()


if __name__ == "__main__":
    main()
