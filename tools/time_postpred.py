#!/usr/bin/env python3
"""Time the posterior-predictive reduction against what is possible without it, from a device chain.

    python tools/time_postpred.py [--sizes 100000,1000000,10240000] [--baseline-only] [--baseline-features N]

C3 shape (N = 1000, d = 6, 10 PCs, F = 500), S rows of a chain resident on the device.
(a) ``gpemu_posterior_predictive_dev``: mean, both variance parts and the 5 / 50 / 95 % bands of every feature.
(b) the baseline: ``gpemu_gp_predict_dev`` in chunks, back-projection, mean and variances with torch on the device,
    then the central values copied to the host block of features by block of features and reduced with ``np.quantile``.
    It uses nothing the library did not have before (``--baseline-only`` with GPEMU_LIBRARY set to an older build runs it
    against that build).  ``--baseline-features N``: time the host part on the first N features only and scale it to F
    (the host part is one independent np.quantile per feature); reported as measured and as scaled.
One JSON line per measurement; (a) also reports the path counters."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd"), os.path.join(ROOT, "tests")]

NEW = ("gpemu_select", "gpemu_select_dev", "gpemu_posterior_predictive", "gpemu_posterior_predictive_dev",
       "gpemu_sampler_chain_ptr", "gpemu_postpred_path_counts")
PROBS = (0.05, 0.5, 0.95)
CHUNK = 1 << 18          # rows per gp_predict_dev call of the baseline
FEATURE_BLOCK = 50       # features per device-to-host copy of the baseline


def baseline(dm, wl, X, host_features):
    import numpy as np
    import torch
    S, k, F = X.shape[0], dm.k, dm.F
    comp = torch.as_tensor(wl["components"][:k], device=X.device)
    scale = torch.as_tensor(wl["scale"], device=X.device)
    shift = torch.as_tensor(wl["mean"], device=X.device)
    cun = torch.as_tensor(np.diag(wl["cun"]).copy(), device=X.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = torch.empty((S, k), dtype=torch.float64, device=X.device)
    v = torch.empty((S, k), dtype=torch.float64, device=X.device)
    for r0 in range(0, S, CHUNK):
        nb = min(CHUNK, S - r0)
        dm.gp_predict_dev(X[r0:r0 + nb].data_ptr(), nb, m[r0:r0 + nb].data_ptr(), v[r0:r0 + nb].data_ptr(), stream=0)
    dm.sync()
    t_predict = time.perf_counter() - t0
    t_dev = t_host = 0.0
    mean, var_p, q = np.empty(F), np.empty(F), np.empty((len(PROBS), F))
    nf = min(F, host_features)
    for f0 in range(0, nf, FEATURE_BLOCK):
        f1 = min(nf, f0 + FEATURE_BLOCK)
        t1 = time.perf_counter()
        cv = (m @ comp[:, f0:f1]) * scale[f0:f1] + shift[f0:f1]
        mean[f0:f1] = cv.mean(dim=0).cpu().numpy()
        var_p[f0:f1] = cv.var(dim=0, unbiased=False).cpu().numpy()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        q[:, f0:f1] = np.quantile(cv.cpu().numpy(), PROBS, axis=0)
        t3 = time.perf_counter()
        t_dev += t2 - t1
        t_host += t3 - t2
        del cv
    var_e = ((v.mean(dim=0) @ (comp * comp)) + cun) * scale * scale
    var_e = var_e.cpu().numpy()
    total = t_predict + (t_dev + t_host) * F / nf
    return {"what": "baseline", "S": S, "predict_s": t_predict, "project_moments_s": t_dev, "copy_quantile_s": t_host,
            "features_timed": nf, "total_measured_s": t_predict + t_dev + t_host, "total_scaled_to_F_s": total}, \
        (mean, var_p, var_e, q, nf)


def new_path(dm, X):
    import numpy as np
    import torch
    from gpemu.model import POSTPRED_PATHS, QuantilePlan, postpred_path_counts
    S = X.shape[0]
    plan = QuantilePlan(S, PROBS)
    bufs = torch.empty((3, dm.F), dtype=torch.float64, device=X.device)
    order = torch.empty((dm.F, plan.ranks.size), dtype=torch.float64, device=X.device)
    torch.cuda.synchronize()
    c0 = postpred_path_counts()
    t0 = time.perf_counter()
    dm.posterior_predictive_dev(X.data_ptr(), 1, S, S, plan.ranks, bufs[0].data_ptr(), bufs[1].data_ptr(),
                                bufs[2].data_ptr(), order.data_ptr(), stream=0)
    h = bufs.cpu().numpy()
    out = plan.result(h[0], h[1], h[2], order.cpu().numpy())
    dt = time.perf_counter() - t0
    c1 = postpred_path_counts() - c0
    ws = 8 * S * dm.F
    return {"what": "posterior_predictive_dev", "S": S, "total_s": dt, "counters": dict(zip(POSTPRED_PATHS, c1.tolist())),
            "workspace_bytes": ws, "algorithmic_bytes": ws * (1 + 2 + 8)}, out     # written once, 2 moment reads, 8 passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,10240000")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--new-only", action="store_true")
    ap.add_argument("--baseline-features", type=int, default=500)
    ap.add_argument("--baseline-features-large", type=int, default=50, help="... for S > 2 000 000")
    args = ap.parse_args()
    import numpy as np
    import torch
    from gpemu import _lib
    if args.baseline_only:
        for name in NEW:
            _lib._SIGNATURES.pop(name, None)
    import bench
    from gpemu import model as M
    wl = bench.build_workload(0, 1000, 500, 10, seed=0)
    prob = wl["prob"]
    dm = M.DeviceModel(X_train=prob["design"], ls=wl["ls"], alpha=wl["alpha"], L=wl["L"], components=wl["components"],
                       scaler_mean=wl["mean"], scaler_scale=wl["scale"], kernel_kind=0, noise=wl["noise"],
                       cov_unexplained=wl["cun"], device=0)
    lo, hi = torch.as_tensor(prob["lo"], device="cuda:0"), torch.as_tensor(prob["hi"], device="cuda:0")
    for S in (int(s) for s in args.sizes.split(",")):
        gen = torch.Generator(device="cuda:0").manual_seed(S)
        X = lo + (hi - lo) * torch.rand((S, lo.numel()), dtype=torch.float64, device="cuda:0", generator=gen)
        new = base = None
        if not args.baseline_only:
            rec, new = new_path(dm, X)
            print(json.dumps(rec), flush=True)
        if not args.new_only:
            nf = args.baseline_features if S <= 2000000 else args.baseline_features_large
            brec, base = baseline(dm, wl, X, nf)
            print(json.dumps(brec), flush=True)
        if new is not None and base is not None:
            mean, var_p, var_e, q, nf = base
            scale = np.abs(mean[:nf]).max()
            summary = {"what": "summary", "S": S, "new_s": rec["total_s"], "baseline_s": brec["total_scaled_to_F_s"],
                       "speedup": brec["total_scaled_to_F_s"] / rec["total_s"],
                       "max_quantile_diff_rel": float(np.abs(new["quantiles"][:, :nf] - q[:, :nf]).max() / scale),
                       "max_mean_diff_rel": float(np.abs(new["mean"][:nf] - mean[:nf]).max() / scale),
                       "max_var_emu_diff_rel": float(np.max(np.abs(new["variance_emulator"] - var_e) / var_e)),
                       "condition_met": bool(rec["total_s"] < brec["total_scaled_to_F_s"])}
            print(json.dumps(summary), flush=True)
        del X
        torch.cuda.empty_cache()
    dm.close()


if __name__ == "__main__":
    main()
