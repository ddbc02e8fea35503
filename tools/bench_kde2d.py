#!/usr/bin/env python3
"""Timing of the 2-D kernel densities of parameter pairs on the device against the host route.

    timeout 1500 python tools/bench_kde2d.py [--steps 11000] [--walkers 1024] [--d 8 16] [--thin 1 10] [--n-grid 100]
                                             [--reps 5] [--covariance full] [--host-fraction 0.01] [--host-pairs 2]

Workload: the synthetic chain of tools/bench_marginals.py, [steps][walkers][d] on the device (the headline run stores
1024 walkers x 11 000 steps), read in place -- whole and thinned by steps (--thin: the block view the samplers hand to
the library, no copy).  All d (d - 1) / 2 pairs on --n-grid points per axis.  Timed with a host clock around calls that
end in a device synchronise, one warm-up each and --reps repeats (median, min and max are reported):
  plan     gpemu_pair_moments_dev twice: mean and covariance, then the extents of x and of the sheared coordinate
  density  gpemu_kde2d_dev on that plan: the partial tiles on the matrix cores and their sum in chunk order
  total    both, as DeviceSampler.marginals(kde2d=True) calls them
  host     scipy.stats.gaussian_kde per pair on the first --host-fraction of the samples of the view, evaluated on the
           same mesh, for the first --host-pairs pairs; its time is PROJECTED to all samples and all pairs (x 1 / fraction
           x pairs / timed pairs: the direct sum is linear in both); the record says so (host_projected).
Beside them the floor of the matrix product alone, 2 P G_pad^2 S flop (G_pad: --n-grid rounded up to the tile: 128, or
64 where the grid fits it) over the fp64 matrix rate (--mfma-tflops, default 77.51: `mfma_f64_16x16x4 only`,
profiles/r01_fp64_rates.txt), and the number of exp evaluations, 2 P (G_pad / tile) G_pad S: on this hardware fp64 vector
and matrix instructions share an issue port (the `both` rows of that profile), so the time over the floor is the
generation of the operands.
One JSON line per (d, thin)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=11000)
    ap.add_argument("--walkers", type=int, default=1024)
    ap.add_argument("--d", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--thin", type=int, nargs="+", default=[1, 10])
    ap.add_argument("--n-grid", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--covariance", default="full", choices=["full", "diagonal"])
    ap.add_argument("--host-fraction", type=float, default=0.01)
    ap.add_argument("--host-pairs", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--mfma-tflops", type=float, default=77.51)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bench_marginals import synthetic_chain, timed
    from gpemu import _lib
    from gpemu import marginals as M
    from gpemu.rows import DeviceRows
    if _lib.device_count() <= 0 or not torch.cuda.is_available():
        raise SystemExit("bench_kde2d: no GPU visible; nothing is measured without one")
    G, W = args.n_grid, args.walkers
    tile = 64 if G <= 64 else 128
    gpad = -(-G // tile) * tile
    for d in args.d:
        x = synthetic_chain(args.steps, W, d)
        base = x.data_ptr()
        for thin in args.thin:
            nb = args.steps // thin
            S, P = nb * W, d * (d - 1) // 2
            rows = DeviceRows(base, nb, W, thin * W, device=0, d=d)
            flat = (0, *rows.layout, d)                     # as the wrappers of one C prototype take them
            rec = {"steps": args.steps, "walkers": W, "d": d, "thin": thin, "samples": S, "pairs": P, "n_grid": G,
                   "covariance": args.covariance, "reps": args.reps}
            c0 = M.kde2d_path_counts()
            res = M._kde2d_view(rows, covariance=args.covariance, n_grid=G)
            c1 = M.kde2d_path_counts()
            rec["launches"] = {k: c1[k] - c0[k] for k in c1}
            plan = {k: res[k] for k in ("pairs", "shear", "bandwidth", "grid_a", "grid_b")}

            def plan_only():
                M._pair_moments_dev(*flat)
                M._pair_moments_dev(*flat, np.concatenate([plan["pairs"][:, ::-1], plan["pairs"]]),
                                    np.concatenate([np.zeros(P), plan["shear"]]), moments=False)
            rec["plan"] = timed(plan_only, args.reps)
            rec["density"] = timed(lambda: M._kde2d_dev(*flat, plan), args.reps)
            rec["total"] = timed(lambda: M._kde2d_view(rows, covariance=args.covariance, n_grid=G), max(1, args.reps // 2))
            flop = 2.0 * P * gpad * gpad * S
            rec["mfma_flop"] = flop
            rec["mfma_floor_s"] = flop / (args.mfma_tflops * 1e12)
            rec["mfma_floor_fraction_of_density"] = rec["mfma_floor_s"] / rec["density"]["median_s"]
            rec["achieved_tflops"] = flop / rec["density"]["median_s"] / 1e12
            rec["exp_evaluations"] = 2.0 * P * (gpad // tile) * gpad * S
            cell = np.diff(res["grid_a"], axis=1)[:, 0] * np.diff(res["grid_b"], axis=1)[:, 0]
            rec["panel_area_min_max"] = [float((res["density"].sum(axis=(1, 2)) * cell).min()),
                                         float((res["density"].sum(axis=(1, 2)) * cell).max())]
            if not args.no_host:
                from scipy.stats import gaussian_kde
                n_sub = max(3, int(S * args.host_fraction))
                host = x[::thin].reshape(-1, d)[:n_sub].cpu().numpy()
                n_pairs = min(P, max(1, args.host_pairs))
                t0 = time.perf_counter()
                for p in range(n_pairs):
                    i, j = plan["pairs"][p]
                    X, Y = M.kde_2d_mesh(res, p)
                    gaussian_kde(np.stack([host[:, i], host[:, j]])).evaluate(np.stack([X.ravel(), Y.ravel()]))
                t_sub = time.perf_counter() - t0
                rec["host"] = {"subsample": n_sub, "timed_pairs": n_pairs, "subsample_s": t_sub,
                               "projected_s": t_sub * (S / n_sub) * (P / n_pairs), "host_projected": True}
                rec["host_over_device"] = rec["host"]["projected_s"] / rec["total"]["median_s"]
            print(json.dumps(rec), flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
