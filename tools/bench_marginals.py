#!/usr/bin/env python3
"""Timing of the marginal summaries on the device against what a user computes today on the host.

    timeout 1500 python tools/bench_marginals.py [--steps 11000] [--walkers 1024] [--d 8 16] [--reps 5]
                                                 [--bins 100 50] [--n-grid 200] [--host-kde-fraction 0.01]

Workload: a synthetic chain [steps][walkers][d] of correlated normal samples inside the unit box, written to the device
once (the headline run stores 1024 walkers x 11 000 steps, d = 8: 11.3 M samples, 0.72 GB; d = 16 is the widest the
library takes).  Timed with a host clock around calls that end in a device synchronise, one warm-up each and --reps
repeats (median, min and max are reported):
  hist     gpemu_marginal_hist_dev on the chain in place (block layout, one block)
  hpd      gpemu_hpd_dev, every parameter a row of stride d, one confidence level
  kde      gpemu_kde1d_dev, --n-grid points per parameter, Scott bandwidth
  total    the three and the moments, as DeviceSampler.marginals calls them
  host     the same summaries with what exists without this feature: the download of the chain (timed: a device-to-host
           copy), np.histogram per parameter, np.histogram2d per pair, the drop-in's credible_interval(x, 0.9, 'hpd')
           per parameter and scipy.stats.gaussian_kde(x).evaluate(grid) per parameter.  The KDE runs on the first
           --host-kde-fraction of the samples and its time is PROJECTED to the full sample (x 1 / fraction: the direct
           sum is linear in the samples); the record says so (host_kde_projected).
Lower bounds, from the shapes alone:
  hist     chain bytes x sweeps / HBM bandwidth (--hbm-gbs, default 8000: the MI355X's specified 8 TB/s; the achieved
           fraction is reported against it), sweeps = the library's own count (HIST_SWEEP);
  kde      S x G x d terms, --term-instructions fp64 vector instructions each (default 25: the density kernel's ISA has
           99 for the four terms of its unrolled loop -- the difference, the scaling, the square, exp's range reduction,
           polynomial and ldexp, the sum), against the hardware's fp64 issue limit, 256 CUs x 4 SIMDs x 16 lanes per
           clock at 2.4 GHz (--fp64-valu-tera, default 39.32 tera-instructions per second; the v_fma_f64 loop of
           profiles/r01_fp64_rates.txt sustained 59.11 TF = 29.55).  The kernel does not evaluate a term that is exactly
           0 in fp64, so it may come close to, or beat, a bound that counts every term.
One JSON line per d."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd"), os.path.join(ROOT, "tests")]


def synthetic_chain(steps, W, d, seed=0):
    """[steps][W][d] float64 on the device: correlated normals around the middle of the unit box, clipped to it."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    z = torch.randn((steps, W, d), generator=g, device="cuda", dtype=torch.float64)
    mix = torch.eye(d, device="cuda", dtype=torch.float64) + 0.3 * torch.rand((d, d), generator=g, device="cuda",
                                                                               dtype=torch.float64)
    x = 0.5 + 0.08 * (z @ mix)
    return x.clamp_(0.0, 1.0).contiguous()


def timed(fn, reps):
    import torch
    fn()                                    # warm-up: code objects, allocations
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=11000)
    ap.add_argument("--walkers", type=int, default=1024)
    ap.add_argument("--d", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", type=int, nargs=2, default=[100, 50])
    ap.add_argument("--n-grid", type=int, default=200)
    ap.add_argument("--confidence", type=float, default=0.9)
    ap.add_argument("--host-kde-fraction", type=float, default=0.01)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--fp64-valu-tera", type=float, default=39.32)
    ap.add_argument("--term-instructions", type=float, default=25.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    from gpemu import _lib
    from gpemu import marginals as M
    if _lib.device_count() <= 0 or not torch.cuda.is_available():
        raise SystemExit("bench_marginals: no GPU visible; nothing is measured without one")
    nb1, nb2 = args.bins
    for d in args.d:
        x = synthetic_chain(args.steps, args.walkers, d)
        S = args.steps * args.walkers
        base = x.data_ptr()
        lo, hi = np.zeros(d), np.ones(d)
        e1, e2 = M.bin_edges(lo, hi, nb1), M.bin_edges(lo, hi, nb2)
        n_out = M.n_outside([args.confidence], S)
        rec = {"steps": args.steps, "walkers": args.walkers, "d": d, "samples": S, "chain_bytes": 8 * S * d,
               "bins": [nb1, nb2], "n_grid": args.n_grid, "confidence": args.confidence, "reps": args.reps}

        c0 = M.path_counts()
        hist = M._hist_dev(0, base, 1, S, S, d, e1, e2)
        sweeps = M.path_counts()["HIST_SWEEP"] - c0["HIST_SWEEP"]
        rec["hist"] = timed(lambda: M._hist_dev(0, base, 1, S, S, d, e1, e2), args.reps)
        rec["hist_sweeps"] = sweeps
        rec["hist_lower_bound_s"] = 8 * S * d * sweeps / (args.hbm_gbs * 1e9)
        rec["hist_fraction_of_bound"] = rec["hist_lower_bound_s"] / rec["hist"]["median_s"]

        ends = M._hpd_dev(0, base, S, d, np.append(n_out, 1))
        rec["hpd"] = timed(lambda: M._hpd_dev(0, base, S, d, n_out), args.reps)
        _, var = M._moments_dev(0, base, S, d)
        h = M.scott_bandwidth(S, np.sqrt(var * (S / (S - 1.0))))
        grid = M.default_grid(ends[-1, :, 0], ends[-1, :, 1], h, args.n_grid)
        dens = M._kde_dev(0, base, S, d, grid, h)
        rec["kde"] = timed(lambda: M._kde_dev(0, base, S, d, grid, h), args.reps)
        rec["kde_exp_evaluations"] = S * args.n_grid * d
        rec["kde_lower_bound_s"] = S * args.n_grid * d * args.term_instructions / (args.fp64_valu_tera * 1e12)
        rec["kde_fraction_of_bound"] = rec["kde_lower_bound_s"] / rec["kde"]["median_s"]

        def total():
            M._hist_dev(0, base, 1, S, S, d, e1, e2)
            en = M._hpd_dev(0, base, S, d, np.append(n_out, 1))
            _, v = M._moments_dev(0, base, S, d)
            hh = M.scott_bandwidth(S, np.sqrt(v * (S / (S - 1.0))))
            M._kde_dev(0, base, S, d, M.default_grid(en[-1, :, 0], en[-1, :, 1], hh, args.n_grid), hh)
        rec["total"] = timed(total, max(1, args.reps // 2))

        if not args.no_host:
            from bayesian_inference import mcmc
            from scipy.stats import gaussian_kde
            t0 = time.perf_counter()
            host = x.cpu().numpy().reshape(-1, d)
            t_dl = time.perf_counter() - t0
            t0 = time.perf_counter()
            h1 = np.stack([np.histogram(host[:, j], bins=e1[j])[0] for j in range(d)])
            t_h1 = time.perf_counter() - t0
            t0 = time.perf_counter()
            pairs = M.pair_indices(d)
            h2 = np.stack([np.histogram2d(host[:, i], host[:, j], bins=[e2[i], e2[j]])[0] for i, j in pairs])
            t_h2 = time.perf_counter() - t0
            t0 = time.perf_counter()
            hp = np.array([mcmc.credible_interval(host[:, j], args.confidence, "hpd") for j in range(d)])
            t_hpd = time.perf_counter() - t0
            n_sub = max(2, int(S * args.host_kde_fraction))
            t0 = time.perf_counter()
            for j in range(d):
                gaussian_kde(host[:n_sub, j]).evaluate(grid[j])
            t_kde_sub = time.perf_counter() - t0
            t_kde = t_kde_sub * (S / n_sub)
            rec["host"] = {"download_s": t_dl, "histogram_1d_s": t_h1, "histogram_2d_s": t_h2, "hpd_s": t_hpd,
                           "kde_subsample": n_sub, "kde_subsample_s": t_kde_sub, "kde_projected_s": t_kde,
                           "host_kde_projected": True, "total_s": t_dl + t_h1 + t_h2 + t_hpd + t_kde}
            rec["host_over_device"] = rec["host"]["total_s"] / rec["total"]["median_s"]
            # the device results are the host's: counts and interval ends exactly
            rec["hist_1d_equal"] = bool(np.array_equal(hist[0], h1))
            rec["hist_2d_equal"] = bool(np.array_equal(hist[1], h2.astype(np.int64)))
            rec["hpd_equal"] = bool(np.array_equal(ends[0], hp))
        rec["kde_density_max"] = float(dens.max())
        print(json.dumps(rec), flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
