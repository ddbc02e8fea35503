#!/usr/bin/env python3
"""Timing of the weighted bands, intervals and densities against their unweighted forms on the same rows.

    timeout 900 python tools/time_wsummary.py [--bands-s 1000000] [--log2-s 24] [--d 6] [--grid 200] [--reps 5]
                                              [--only bands|hpd|kde] [--out FILE]

Timed with a host clock around calls that end in a device synchronise, one warm-up each, the two members of a pair
alternating, --reps repeats (median, min and max are reported):
  bands   gpemu_posterior_predictive_dev against gpemu_posterior_predictive_weighted_dev with R_w = 1 and 4 weight rows, at
          the C3 shape (N = 1000, d = 6, 10 PCs, F = 500; bench.build_workload), --bands-s rows resident on the device,
          mean, both variances and three quantiles;
  hpd     gpemu_hpd_dev against gpemu_weighted_hpd_dev, the d parameters of a chain [S][d] (S = 2^--log2-s) as rows of
          stride d, two levels, one weight row;
  kde     gpemu_kde1d_dev against gpemu_weighted_kde1d_dev on the same rows, --grid points, one weight row.
The weights are one row (bands: R_w rows) of normalised weights quantised by gpemu_weights_fixed_dev.  Before timing, the
weighted forms under equal weights are compared with the unweighted ones.  One JSON line per check and measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd")]

PROBS = (0.05, 0.5, 0.95)
CONF = (0.68, 0.9)


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


def weights(R_w, S, gen):
    import torch
    from gpemu import reweight as R
    l = 1.5 * torch.randn((R_w, S), generator=gen, device="cuda", dtype=torch.float64)
    _, lw = R.logmeanexp_dev(l, normalise=True)
    return R.fixed_weights_dev(lw)


def bands(args, emit):
    import numpy as np
    import torch
    import bench
    from gpemu import model as M, reweight as R
    wl = bench.build_workload(0, 1000, 500, 10, seed=0)
    prob = wl["prob"]
    dm = M.DeviceModel(X_train=prob["design"], ls=wl["ls"], alpha=wl["alpha"], L=wl["L"], components=wl["components"],
                       scaler_mean=wl["mean"], scaler_scale=wl["scale"], kernel_kind=0, noise=wl["noise"],
                       cov_unexplained=wl["cun"], device=0)
    S, F = args.bands_s, dm.F
    gen = torch.Generator(device="cuda").manual_seed(S)
    lo, hi = torch.as_tensor(prob["lo"], device="cuda"), torch.as_tensor(prob["hi"], device="cuda")
    X = lo + (hi - lo) * torch.rand((S, lo.numel()), dtype=torch.float64, device="cuda", generator=gen)
    plan = M.QuantilePlan(S, PROBS)
    u = torch.empty((3, F), dtype=torch.float64, device="cuda")
    uo = torch.empty((F, plan.ranks.size), dtype=torch.float64, device="cuda")

    def plain():
        dm.posterior_predictive_dev(X.data_ptr(), 1, S, S, plan.ranks, u[0].data_ptr(), u[1].data_ptr(), u[2].data_ptr(),
                                    uo.data_ptr(), stream=0)

    for R_w in (1, 4):
        q, Q = weights(R_w, S, gen)
        tgt = R.targets(PROBS, Q)
        w = torch.empty((3, R_w, F), dtype=torch.float64, device="cuda")
        wq = torch.empty((R_w, F, 3), dtype=torch.float64, device="cuda")

        def weighted(qq=q, t=tgt):
            dm.posterior_predictive_weighted_dev(X.data_ptr(), 1, S, S, qq, t, w[0].data_ptr(), w[1].data_ptr(),
                                                 w[2].data_ptr(), wq.data_ptr(), stream=0)
        if R_w == 1 and S & (S - 1) == 0:        # a power of two: 2^e weights give the unweighted bits
            plain()
            weighted(torch.full((1, S), (1 << 52) // S, dtype=torch.int64, device="cuda"),
                     np.ascontiguousarray([[1, 1, 1]], dtype=np.uint64))
            same = bool(torch.equal(u[0], w[0, 0]) and torch.equal(u[2], w[2, 0]))
            emit({"check": "weighted bands under equal power-of-two weights equal the unweighted mean and var_emu", "ok": same})
            assert same
        c0 = R.wsummary_path_counts()
        weighted()
        c1 = R.wsummary_path_counts()
        tu, tw = timed_pair(plain, weighted, args.reps)
        emit({"what": "bands", "S": S, "F": F, "k": dm.k, **tu})
        emit({"what": "weighted_bands", "S": S, "F": F, "k": dm.k, "R_w": R_w, **tw, "ratio": tw["median_s"] / tu["median_s"],
              "counters": {k: c1[k] - c0[k] for k in c1 if c1[k] != c0[k]},
              "row_reduce_bytes": 2 * (8 * S * F + -(-F // 4) * R_w * 8 * S)})
    dm.close()


def rows(args, emit, which):
    import numpy as np
    import torch
    from gpemu import _lib, marginals as M, reweight as R
    from gpemu._lib import check, ptr
    L = _lib.lib()
    S, d, G = 1 << args.log2_s, args.d, args.grid
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((S, d), generator=gen, device="cuda", dtype=torch.float64)
    q, Q = weights(1, S, gen)
    st = lambda: _lib.current_stream(0)
    vp = lambda t: C.c_void_p(t.data_ptr())
    if which == "hpd":
        n_out = M.n_outside(CONF, S)
        tgt = R.targets(CONF, Q)
        ou = torch.empty((d, 2, 2), dtype=torch.float64, device="cuda")
        ow = torch.empty((1, d, 2, 2), dtype=torch.float64, device="cuda")

        def plain():
            check(L.gpemu_hpd_dev(0, d, S, vp(x), 1, d, 2, ptr(n_out), vp(ou), 0, st()))

        def weighted(qq=q, t=tgt):
            ctx = _lib.call_ctx(0)
            check(L.gpemu_weighted_hpd_dev(0, d, S, vp(x), 1, d, 1, vp(qq), S, 2, ptr(t), vp(ow), C.byref(ctx)))
        c = (1 << 52) // S
        plain()
        weighted(torch.full((1, S), c, dtype=torch.int64, device="cuda"),
                 np.ascontiguousarray((c * (S - n_out + 1))[None, :], dtype=np.uint64))
        same = bool(torch.equal(ou, ow[0]))
        emit({"check": "weighted hpd under equal weights equals hpd", "ok": same})
        assert same
        tu, tw = timed_pair(plain, weighted, args.reps)
        emit({"what": "hpd", "S": S, "d": d, "levels": 2, **tu})
        emit({"what": "weighted_hpd", "S": S, "d": d, "levels": 2, **tw, "ratio": tw["median_s"] / tu["median_s"]})
    else:
        h = np.full(d, 0.05)
        grid = np.ascontiguousarray(np.tile(np.linspace(-4.0, 4.0, G), (d, 1)))
        du = torch.empty((d, G), dtype=torch.float64, device="cuda")
        dw = torch.empty((1, d, G), dtype=torch.float64, device="cuda")

        def plain():
            check(L.gpemu_kde1d_dev(0, d, S, vp(x), 1, d, G, ptr(grid), ptr(h), vp(du), st()))

        def weighted(qq=q):
            ctx = _lib.call_ctx(0)
            check(L.gpemu_weighted_kde1d_dev(0, d, S, vp(x), 1, d, 1, vp(qq), S, G, ptr(grid), ptr(h), vp(dw), C.byref(ctx)))
        plain()
        weighted(torch.full((1, S), (1 << 52) // S, dtype=torch.int64, device="cuda"))
        same = bool(torch.equal(du, dw[0]))
        emit({"check": "weighted kde under equal power-of-two weights equals kde", "ok": same})
        assert same
        tu, tw = timed_pair(plain, weighted, args.reps)
        emit({"what": "kde1d", "S": S, "d": d, "G": G, **tu, "terms_per_s": S * d * G / tu["median_s"]})
        emit({"what": "weighted_kde1d", "S": S, "d": d, "G": G, **tw, "ratio": tw["median_s"] / tu["median_s"],
              "terms_per_s": S * d * G / tw["median_s"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bands-s", type=int, default=1000000)
    ap.add_argument("--log2-s", type=int, default=24)
    ap.add_argument("--d", type=int, default=6)
    ap.add_argument("--grid", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("bands", "hpd", "kde"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gpemu import _lib
    if _lib.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured")
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    if args.only in (None, "bands"):
        bands(args, emit)
    for which in ("hpd", "kde"):
        if args.only in (None, which):
            rows(args, emit, which)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
