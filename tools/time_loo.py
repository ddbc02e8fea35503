#!/usr/bin/env python3
"""Time the per-observable terms, PSIS-LOO / WAIC and the weighted moments against what is possible
without them, from rows resident on the device, host to host.

    python tools/time_loo.py [--sizes 100000,1000000,10240000] [--new-only] [--term-rows 20000]

C3 shape (N = 1000, d = 6, 10 PCs, F = 500) with 10 observable blocks of 50 features.
(a) ``gpemu_loglik_pointwise_dev`` + ``gpemu_psis_dev`` (with the log-weights) + ``gpemu_weighted_moments_dev``, the
    table on the host at the end.
(b) the baseline, nothing the library lacked before: ``gpemu_gp_predict_dev`` in chunks, means and variances to the
    host, the terms by batched numpy Cholesky factorisations on 16 threads (timed on the first ``--term-rows`` rows and
    scaled to S: every row is independent), then the smoothing of tests/loo_ref.py restated in float64 numpy on the
    terms of (a).
One JSON line per measurement."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd"), os.path.join(ROOT, "tests")]

CHUNK = 1 << 18
N_BLOCKS = 10
THREADS = 16


def host_setup(wl, y_exp, y_err, bs):
    import numpy as np
    k = wl["ls"].shape[0]
    s = wl["scale"]
    A = wl["cun"] * np.outer(s, s) + np.diag(y_err ** 2)
    U = s[:, None] * wl["components"][:k].T
    r0 = wl["mean"] - y_exp
    out = []
    for o in range(len(bs) - 1):
        sl = slice(bs[o], bs[o + 1])
        c = np.linalg.cholesky(A[sl, sl])
        z = np.linalg.solve(c, np.concatenate([U[sl], r0[sl, None]], axis=1))
        out.append((z[:, :k].T @ z[:, :k], z[:, :k].T @ z[:, k], z[:, k] @ z[:, k], 2 * np.sum(np.log(np.diag(c)))))
    return out


def host_terms(m, v, setups):
    """T [n_obs, B] in float64: the Woodbury form per block, one k x k Cholesky per (row, block)"""
    import numpy as np
    sd = np.sqrt(np.maximum(v, 0.0))
    k = m.shape[1]
    T = np.empty((len(setups), m.shape[0]))
    for o, (G, g0, q0, ld) in enumerate(setups):
        M = np.eye(k)[None] + sd[:, :, None] * G[None] * sd[:, None, :]
        L = np.linalg.cholesky(M)
        h = m @ G + g0[None]
        w = np.linalg.solve(L, (sd * h)[:, :, None])[:, :, 0]
        quad = np.einsum("bi,ij,bj->b", m, G, m) + 2 * (m @ g0) + q0 - np.sum(w * w, axis=1)
        T[o] = -0.5 * quad - 0.5 * (ld + 2 * np.sum(np.log(np.diagonal(L, axis1=1, axis2=2)), axis=1))
    return T


def psis64(V):
    """tests/loo_ref.py's smoothing of one row in float64 numpy (r_eff = 1): (elpd_loo, pareto_k, logw)"""
    import numpy as np
    S = V.size
    x = (-V) - np.max(-V)
    M = int(np.ceil(min(S / 5.0, 3.0 * np.sqrt(S))))
    order = np.argsort(x, kind="stable")
    xs = x[order]
    xc = max(xs[max(S - M - 1, 0)], np.log(np.finfo(float).tiny))
    n = S - int(np.searchsorted(xs, xc, side="right"))
    lw, khat = x.copy(), np.inf
    if n > 4:
        xt = xs[S - n:]
        exc = np.exp(xc)
        t = np.exp(xt) - exc
        m = 30 + int(np.sqrt(n))
        b = (1 - np.sqrt(m / (np.arange(1, m + 1) - 0.5))) / (3 * t[int(n / 4 + 0.5) - 1]) + 1 / t[-1]
        kj = np.mean(np.log1p(-b[:, None] * t), axis=1)
        L = n * (np.log(-(b / kj)) - kj - 1)
        with np.errstate(over="ignore"):
            w = 1 / np.sum(np.exp(L - L[:, None]), axis=1)
        keep = w >= 10 * np.finfo(float).eps
        w, b = w[keep] / w[keep].sum(), b[keep]
        bb = np.sum(w * b)
        kk = np.mean(np.log1p(-bb * t))
        sigma, khat = -kk / bb, (n * kk + 5) / (n + 10)
        p = (np.arange(n) + 0.5) / n
        sm = np.minimum(np.log(exc + sigma * np.expm1(-khat * np.log1p(-p)) / khat), 0.0)
        _, inv, cnt = np.unique(xt, return_inverse=True, return_counts=True)
        sm = (np.bincount(inv, weights=sm) / cnt)[inv]          # tied raw values share the mean
        lw[order[S - n:]] = sm
    mx = lw.max()
    lw = lw - (mx + np.log(np.sum(np.exp(lw - mx))))
    e = lw + V
    return e.max() + np.log(np.sum(np.exp(e - e.max()))), khat, lw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,10240000")
    ap.add_argument("--new-only", action="store_true")
    ap.add_argument("--term-rows", type=int, default=20000)
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from gpemu import loo
    from gpemu import model as M
    wl = bench.build_workload(0, 1000, 500, 10, seed=0)
    prob = wl["prob"]
    dm = M.DeviceModel(X_train=prob["design"], ls=wl["ls"], alpha=wl["alpha"], L=wl["L"], components=wl["components"],
                       scaler_mean=wl["mean"], scaler_scale=wl["scale"], kernel_kind=0, noise=wl["noise"],
                       cov_unexplained=wl["cun"], device=0)
    F, d = dm.F, dm.d
    bs = np.arange(0, F + 1, F // N_BLOCKS, dtype=np.int64)
    dm.likelihood_setup(prob["y_exp"], prob["y_err"], prob["lo"], prob["hi"], 1.0, block_start=bs)
    setups = host_setup(wl, prob["y_exp"], prob["y_err"], bs)
    lo, hi = torch.as_tensor(prob["lo"], device="cuda:0"), torch.as_tensor(prob["hi"], device="cuda:0")
    for S in (int(s) for s in args.sizes.split(",")):
        gen = torch.Generator(device="cuda:0").manual_seed(S)
        X = lo + (hi - lo) * torch.rand((S, d), dtype=torch.float64, device="cuda:0", generator=gen)
        torch.cuda.synchronize()
        c0 = loo.path_counts()
        t0 = time.perf_counter()
        T = torch.empty((N_BLOCKS, S), dtype=torch.float64, device="cuda:0")
        dm.loglik_pointwise_dev(X.data_ptr(), 1, S, S, T.data_ptr(), S)
        t1 = time.perf_counter()
        stats = loo.psis_dev(0, T.data_ptr(), N_BLOCKS, S, S, 1, None, True)
        t2 = time.perf_counter()
        mean, var = loo.weighted_moments_dev(0, X.data_ptr(), 1, S, S, d, stats["log_weights"])
        table = loo.assemble(stats, S)
        t3 = time.perf_counter()
        c1 = loo.path_counts()
        rec = {"what": "device", "S": S, "terms_s": t1 - t0, "psis_s": t2 - t1, "moments_s": t3 - t2, "total_s": t3 - t0,
               "rows_per_s": S / (t3 - t0), "counters": {k: c1[k] - c0[k] for k in c1},
               "elpd_loo_total": table["elpd_loo_total"], "max_pareto_k": float(np.max(table["pareto_k"]))}
        print(json.dumps(rec), flush=True)
        if not args.new_only:
            t0 = time.perf_counter()
            m = torch.empty((S, dm.k), dtype=torch.float64, device="cuda:0")
            v = torch.empty((S, dm.k), dtype=torch.float64, device="cuda:0")
            for r0 in range(0, S, CHUNK):
                nb = min(CHUNK, S - r0)
                dm.gp_predict_dev(X[r0:r0 + nb].data_ptr(), nb, m[r0:r0 + nb].data_ptr(), v[r0:r0 + nb].data_ptr(), stream=0)
            dm.sync()
            hm, hv = m.cpu().numpy(), v.cpu().numpy()
            t1 = time.perf_counter()
            nt = min(S, args.term_rows)
            parts = np.array_split(np.arange(nt), THREADS)
            with ThreadPoolExecutor(THREADS) as ex:
                Th = np.concatenate(list(ex.map(lambda idx: host_terms(hm[idx], hv[idx], setups), parts)), axis=1)
            t2 = time.perf_counter()
            hT = T.cpu().numpy()
            t3 = time.perf_counter()
            with ThreadPoolExecutor(THREADS) as ex:
                res = list(ex.map(psis64, list(hT)))
            t4 = time.perf_counter()
            terms_scaled = (t2 - t1) * S / nt
            base = {"what": "baseline", "S": S, "predict_and_copy_s": t1 - t0, "terms_rows_timed": nt,
                    "terms_measured_s": t2 - t1, "terms_scaled_to_S_s": terms_scaled, "psis_float64_s": t4 - t3,
                    "total_scaled_s": (t1 - t0) + terms_scaled + (t4 - t3),
                    "max_term_diff": float(np.max(np.abs(Th - hT[:, :nt]))),
                    "max_elpd_diff": float(np.max(np.abs(np.array([r[0] for r in res]) - table["elpd_loo"]))),
                    "max_k_diff": float(np.max(np.abs(np.array([r[1] for r in res]) - table["pareto_k"])))}
            print(json.dumps(base), flush=True)
            print(json.dumps({"what": "summary", "S": S, "device_s": rec["total_s"], "baseline_s": base["total_scaled_s"],
                              "speedup": base["total_scaled_s"] / rec["total_s"]}), flush=True)
            del m, v
        del X, T, stats
        torch.cuda.empty_cache()
    dm.close()


if __name__ == "__main__":
    main()
