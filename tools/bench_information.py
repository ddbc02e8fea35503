#!/usr/bin/env python3
"""Timing of the k-th neighbour information gain on the device.

    timeout 600 python tools/bench_information.py [--n 65536] [--d 6] [--k 4] [--reps 5] [--no-host]
                                                  [--valu-tflops 59.11]

Workload: the synthetic chain of tools/bench_marginals.py, n rows of d parameters on the device.  Timed with a host
clock around calls that end in a device synchronise, one warm-up each and --reps repeats (median, min and max):
  gain    gpemu.information.information_gain, default subsets (every parameter, every pair, the joint): the unit-box
          rows, the searches of the three widths, the sums
  joint   the same for the joint subset alone
  search  gpemu_knn_dist_dev alone, default subsets and joint
Beside them the pair rate n^2 P / t of the searches and what it is of the fp64 vector rate: a (pair, coordinate) costs
one v_add_f64 and one v_fma_f64, 3 flop in the counting of profiles/r01_fp64_rates.txt (`v_fma_f64 only`, 59.11 TF at 4
waves per SIMD, an fma as 2: --valu-tflops); the compare, the branch and the LDS reads come on top.
  host    scipy.spatial.cKDTree's time for the same neighbours (build + query of k + 1, per subset), for information
          only: a tree is another algorithm, and it wins in 1-D and 2-D.
One JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--d", type=int, default=6)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--valu-tflops", type=float, default=59.11)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bench_marginals import synthetic_chain, timed
    from gpemu import _lib
    from gpemu import information as I
    if _lib.device_count() <= 0 or not torch.cuda.is_available():
        raise SystemExit("bench_information: no GPU visible; nothing is measured without one")
    n, d, k = args.n, args.d, args.k
    W = 256
    x = synthetic_chain(-(-n // W), W, d).reshape(-1, d)[:n].contiguous()
    # the clipped rows of the synthetic chain coincide in a coordinate: allowed here, the time does not depend on it
    lo, hi = np.zeros(d), np.ones(d)
    subs = I.default_subsets(d)
    joint = [tuple(range(d))]
    rec = {"n": n, "d": d, "k": k, "subsets": len(subs), "reps": args.reps}
    c0 = I.path_counts()
    out = I.information_gain(x, lo, hi, k=k, allow_copies=True)
    c1 = I.path_counts()
    rec["launches"] = {key: c1[key] - c0[key] for key in c1}
    rec["joint_nats"], rec["joint_se"] = float(out["joint"]), float(out["se"][-1])
    rec["gain"] = timed(lambda: I.information_gain(x, lo, hi, k=k, allow_copies=True), args.reps)
    rec["joint"] = timed(lambda: I.information_gain(x, lo, hi, k=k, subsets=joint, allow_copies=True), args.reps)
    U, _ = I.unit_rows_dev(0, x.data_ptr(), 1, n, n, d, lo, hi, n)
    for name, ss in (("search", subs), ("search_joint", joint)):
        _, masks = I.check_subsets(ss, d)
        rec[name] = timed(lambda: I.knn_dist_dev(0, U, None, masks, k), args.reps)
        coords = float(sum(len(s) for s in ss))
        t = rec[name]["median_s"]
        rec[name + "_pairs_per_s"] = float(n) * n * len(ss) / t
        rec[name + "_valu_tflops"] = 3.0 * float(n) * n * coords / t / 1e12
        rec[name + "_fraction_of_valu_rate"] = rec[name + "_valu_tflops"] / args.valu_tflops
    if not args.no_host:
        from scipy.spatial import cKDTree
        h = U.cpu().numpy()
        t_all, t_joint = 0.0, 0.0
        for s in subs:
            t0 = time.perf_counter()
            cKDTree(h[:, list(s)]).query(h[:, list(s)], k=k + 1)
            dt = time.perf_counter() - t0
            t_all += dt
            t_joint = dt if len(s) == d else t_joint
        rec["host_ckdtree"] = {"all_subsets_s": t_all, "joint_s": t_joint, "threads": 1}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
