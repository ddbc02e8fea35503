#!/usr/bin/env python3
"""Timing of the chain diagnostics on the device against the only path the library offered before them.

    timeout 1200 python tools/time_diagnostics.py [--n 2000 10000] [--reps 5] [--walkers 1024]

A stretch run on the C3 synthetic model (W = 1024, d = 6) stores n steps.  Timed alternately, medians of --reps after
one warm-up of each:
  device   DeviceSampler.diagnostics(): ranks, transforms and lag sums where the chain lies;
  host     get_chain() (the download), scipy.stats.rankdata for the two rank kinds, FFT autocovariances of all five
           transformed series on 16 threads (scipy.fft, workers=16), the same scan.
Condition: the device path is faster than the host path including the download; the ratio is recorded.  One JSON line
per n.  For the per-kernel split run it once under `rocprofv3 --kernel-trace --stats -- python tools/time_diagnostics.py
--n 2000 --reps 1 --device-only`; --sort-bytes prints the bytes one sort pass moves (read for the histogram, read and
write for the scatter: 24 bytes per key) to set against the kernel times."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd"), os.path.join(ROOT, "tests")]

THREADS = 16


def c3_sampler(W, seed=3):
    import numpy as np
    import bench
    from gpemu import model as M
    from gpemu.sampler import DeviceSampler
    wl = bench.build_workload(0, 1000, 500, 10, seed=0)
    prob = wl["prob"]
    dm = M.DeviceModel(X_train=prob["design"], ls=wl["ls"], alpha=wl["alpha"], L=wl["L"], components=wl["components"],
                       scaler_mean=wl["mean"], scaler_scale=wl["scale"], kernel_kind=0, noise=wl["noise"],
                       cov_unexplained=wl["cun"], device=0)
    dm.likelihood_setup(prob["y_exp"], prob["y_err"], prob["lo"], prob["hi"], 1.0)
    s = DeviceSampler([dm], W, seed=seed)
    s.set_state(np.random.default_rng(2).uniform(prob["lo"], prob["hi"], (W, len(prob["lo"]))))
    return s, dm


def host_summary(chain):
    """The five diagnostics from a host chain [n][M][d] with numpy / scipy: what a user of the parent commit runs."""
    import numpy as np
    import scipy.fft
    from scipy.special import ndtri
    from scipy.stats import rankdata
    from gpemu.diagnostics import geyer_ess, plain_rhat
    n, M, d = chain.shape
    N, K = n // 2, 2 * M

    def split(x):
        return np.concatenate([x[:N], x[n - N:]], axis=1)

    def zscore(y):
        r = rankdata(y.reshape(-1), method="average").reshape(y.shape)
        return ndtri((r - 0.375) / (y.size + 0.25))

    def moments_acov(y):
        m = y.mean(axis=0)
        c = y - m
        f = scipy.fft.rfft(c, n=2 * N, axis=0, workers=THREADS)
        acov = scipy.fft.irfft(f * np.conj(f), n=2 * N, axis=0, workers=THREADS)[:N].mean(axis=1) / N
        return acov, c.var(axis=0, ddof=1).mean(), m.var(ddof=1)

    out = {k: np.empty(d) for k in ("rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean")}
    for dd in range(d):
        x = chain[:, :, dd]
        z = zscore(split(x))
        g, W, b = moments_acov(z)
        out["ess_bulk"][dd] = geyer_ess(N, K, g, W, b)
        rb = plain_rhat(N, W, b)
        zf = zscore(split(np.abs(x - np.median(x))))
        mf = zf.mean(axis=0)
        rf = plain_rhat(N, (zf - mf).var(axis=0, ddof=1).mean(), mf.var(ddof=1))
        out["rhat"][dd] = max(rb, rf)
        tails = []
        for p in (0.05, 0.95):
            g, W, b = moments_acov(split((x <= np.quantile(x, p)).astype(np.float64)))
            tails.append(geyer_ess(N, K, g, W, b))
        out["ess_tail"][dd] = min(tails)
        g, W, b = moments_acov(split(x))
        out["ess_mean"][dd] = geyer_ess(N, K, g, W, b)
        out["mcse_mean"][dd] = x.std(ddof=1) / np.sqrt(out["ess_mean"][dd])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2000, 10000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--walkers", type=int, default=1024)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--sort-bytes", action="store_true")
    args = ap.parse_args()
    import numpy as np
    os.environ.setdefault("OMP_NUM_THREADS", str(THREADS))
    W = args.walkers
    for n in args.n:
        s, dm = c3_sampler(W)
        s.run(200, store=False)
        s.reserve(n)
        s.run(n)

        def device():
            t0 = time.perf_counter()
            out = s.diagnostics()
            return time.perf_counter() - t0, out

        def host():
            t0 = time.perf_counter()
            chain, _ = s.get_chain()
            t1 = time.perf_counter()
            out = host_summary(chain)
            return time.perf_counter() - t0, t1 - t0, out

        rec = {"n": n, "W": W, "d": s.d, "split_chains": 2 * W, "draws": n // 2}
        if args.sort_bytes:
            rec["sort_bytes_per_pass"] = 24 * (n // 2) * 2 * W * s.d
        _, dev_out = device()                                   # warm-up
        td, th, tdl = [], [], []
        if args.device_only:
            td = [device()[0] for _ in range(args.reps)]
        else:
            _, _, host_out = host()
            for _ in range(args.reps):
                td.append(device()[0])
                a, b, _ = host()
                th.append(a)
                tdl.append(b)
            rec["host_s"], rec["host_download_s"] = float(np.median(th)), float(np.median(tdl))
            rec["max_rel_diff_ess_bulk"] = float(np.max(np.abs(dev_out["ess_bulk"] - host_out["ess_bulk"]) / host_out["ess_bulk"]))
            rec["max_abs_diff_rhat"] = float(np.max(np.abs(dev_out["rhat"] - host_out["rhat"])))
        rec["device_s"] = float(np.median(td))
        if th:
            rec["host_over_device"] = rec["host_s"] / rec["device_s"]
            rec["condition_met"] = bool(rec["device_s"] < rec["host_s"])
        rec["max_rhat"], rec["min_ess_bulk"] = float(np.max(dev_out["rhat"])), float(np.min(dev_out["ess_bulk"]))
        print(json.dumps(rec), flush=True)
        s.close()
        dm.close()


if __name__ == "__main__":
    main()
