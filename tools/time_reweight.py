#!/usr/bin/env python3
"""Timing of the weighted summaries against their unweighted forms on the same rows.

    timeout 900 python tools/time_reweight.py [--log2-s 24] [--d 6] [--reps 5] [--bins 100 50] [--out FILE]

Workload: a synthetic chain [S][d] on the device (S = 2^24, d = 6: 0.8 GB) and one row of normalised weights quantised by
gpemu_weights_fixed_dev.  Timed with a host clock around calls that end in a device synchronise, one warm-up each, the two
members of a pair alternating, --reps repeats (median, min and max are reported):
  select            gpemu_select_dev, the d parameters as rows of stride d, 3 ranks
  weighted_select   gpemu_weighted_select_dev on the same rows, 3 targets at the same probabilities, one weight row
  hist              gpemu_marginal_hist_dev, --bins
  weighted_hist     gpemu_weighted_hist_dev, the same edges, one weight row
the histograms on a diffuse sample (uniform in the box) and on a concentrated one (a normal of width 0.01 of the box: the
LDS atomics contend).  Read rates count the bytes the algorithm needs: 8 passes x d rows x 8 S bytes for a select (the
weighted one besides 8 S bytes of weights per row in every pass in which all samples match: the first two, bounded above
by all eight), d x 8 S (+ 8 S of weights) bytes per sweep for a histogram, sweeps = the library's own count.
Before timing, the weighted forms under equal weights are compared with the unweighted ones (the same elements, c times
the counts).  One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd")]


def timed_pair(fa, fb, reps):
    import torch
    fa(), fb()                                   # warm-up: code objects, allocations
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for f, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
    out = []
    for ts in (ta, tb):
        ts.sort()
        out.append({"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-s", type=int, default=24)
    ap.add_argument("--d", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", type=int, nargs=2, default=[100, 50])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from gpemu import _lib, marginals as M, reweight as R
    from gpemu._lib import check, ptr
    if _lib.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured")
    L = _lib.lib()
    S, d = 1 << args.log2_s, args.d
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    lo, hi = np.zeros(d), np.ones(d)
    diffuse = torch.rand((S, d), generator=g, device="cuda", dtype=torch.float64)
    l = 1.5 * torch.randn((1, S), generator=g, device="cuda", dtype=torch.float64)
    _, lw = R.logmeanexp_dev(l, normalise=True)
    q, Q = R.fixed_weights_dev(lw)
    del l, lw
    probs = (0.05, 0.5, 0.95)
    tgt = R.targets(probs, Q)
    ranks = np.ascontiguousarray([min(S - 1, int(p * S)) for p in probs], dtype=np.int64)
    out_u = torch.empty((d, 3), dtype=torch.float64, device="cuda")
    out_w = torch.empty((1, d, 3), dtype=torch.float64, device="cuda")
    st = lambda: _lib.current_stream(0)

    def sel(x):
        check(L.gpemu_select_dev(0, d, S, C.c_void_p(x.data_ptr()), 1, d, 3, ptr(ranks), C.c_void_p(out_u.data_ptr()), st()))

    def wsel(x, qq=None, t=None):
        qq, t = (q if qq is None else qq), (tgt if t is None else t)
        check(L.gpemu_weighted_select_dev(0, d, S, C.c_void_p(x.data_ptr()), 1, d, 1, C.c_void_p(qq.data_ptr()), S, 3, ptr(t),
                                          C.c_void_p(out_w.data_ptr()), 0, st()))

    # equal weights: the same elements as the unweighted select at rank t - 1
    ones = torch.ones((1, S), dtype=torch.int64, device="cuda")
    sel(diffuse)
    wsel(diffuse, ones, np.ascontiguousarray((ranks + 1)[None, :], dtype=np.uint64))
    same = bool(torch.equal(out_u, out_w[0]))
    emit({"check": "weighted select under unit weights equals select", "ok": same})
    assert same
    tu, tw = timed_pair(lambda: sel(diffuse), lambda: wsel(diffuse), args.reps)
    base = 8 * d * 8 * S
    emit({"what": "select", "S": S, "d": d, **tu, "read_gbs": base / tu["median_s"] / 1e9})
    emit({"what": "weighted_select", "S": S, "d": d, **tw, "ratio": tw["median_s"] / tu["median_s"],
          "read_gbs_values_only": base / tw["median_s"] / 1e9,
          "read_gbs_with_weights_of_two_passes": (base + 2 * d * 8 * S) / tw["median_s"] / 1e9,
          "read_gbs_with_weights_of_all_passes": (base + 8 * d * 8 * S) / tw["median_s"] / 1e9})

    e1, e2 = M.bin_edges(lo, hi, args.bins[0]), M.bin_edges(lo, hi, args.bins[1])
    conc = (0.5 + 0.01 * torch.randn((S, d), generator=g, device="cuda", dtype=torch.float64)).clamp_(0.0, 1.0)
    for name, x in (("diffuse", diffuse), ("concentrated", conc)):
        c0, r0 = M.path_counts(), R.path_counts()
        h1, h2, ni = M._hist_dev(0, x.data_ptr(), 1, S, S, d, e1, e2)
        w1, w2, wi = R.weighted_hist_dev(0, x.data_ptr(), 1, S, S, d, ones * 3, e1, e2)
        sweeps_u = M.path_counts()["HIST_SWEEP"] - c0["HIST_SWEEP"]
        sweeps_w = R.path_counts()["WHIST_SWEEP"] - r0["WHIST_SWEEP"]
        same = bool(np.array_equal(w1[0], h1.astype(np.uint64) * np.uint64(3)) and np.array_equal(w2[0], h2.astype(np.uint64) * np.uint64(3)))
        emit({"check": f"weighted hist under equal weights equals 3 x the counts ({name})", "ok": same})
        assert same
        tu, tw = timed_pair(lambda: M._hist_dev(0, x.data_ptr(), 1, S, S, d, e1, e2),
                            lambda: R.weighted_hist_dev(0, x.data_ptr(), 1, S, S, d, q, e1, e2), args.reps)
        emit({"what": "hist", "sample": name, "S": S, "d": d, "bins": args.bins, "sweeps": sweeps_u, **tu,
              "read_gbs": sweeps_u * d * 8 * S / tu["median_s"] / 1e9})
        emit({"what": "weighted_hist", "sample": name, "S": S, "d": d, "bins": args.bins, "sweeps": sweeps_w, **tw,
              "ratio": tw["median_s"] / tu["median_s"], "read_gbs": sweeps_w * (d + 1) * 8 * S / tw["median_s"] / 1e9})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
