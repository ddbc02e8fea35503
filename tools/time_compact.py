#!/usr/bin/env python
"""Kernel times of the sampler's compacted half-step per live block count.

At the benchmark's shape (N = 1000, 10 PCs, 1024 walkers: halves of 512 proposals, 8 blocks of 64 columns) every live
block count 1 .. 8 is forced through ``step_host_rng`` -- a stretch of 1 proposes the walker's own position, inside the
box; a huge one a point far outside -- and the HIP event pairs of ``DeviceModel.profile`` around the cross-kernel and the
triangular GEMM are read back.  Each count is timed for every way of dealing the live blocks to the XCDs
(``GPEMU_COMPACT_FORM`` = 0 the whole batch's schedule, 1 its placement without the dead blocks, 2 cut by cost, and unset:
the library's choice per count) against the uncompacted 512-column launch with every proposal inside the box
(``GPEMU_NO_COMPACT=1``: the parent's launch), timed first and last: the first entry of a process runs on clocks that are
still ramping.

    python tools/time_compact.py [--reps 40] [--forms off,auto,0,1,2,off] [--n 1000 --pcs 10 --walkers 1024]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bayesian-inference_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def draws(W, live, rng):
    inds = (np.arange(W) % 2).astype(np.int32)
    rng.shuffle(inds)
    ns = (W + 1) // 2, W // 2
    zz, rint, logu = [], [], []
    for h in range(2):
        z = np.full(ns[h], 1.0e9)
        z[rng.permutation(ns[h])[:min(live, ns[h])]] = 1.0
        zz.append(z)
        rint.append(rng.integers(0, W - ns[h], ns[h]).astype(np.int64))
        logu.append(np.log(rng.uniform(0.0, 1.0, ns[h])))
    return inds, zz, rint, logu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--obs", type=int, default=500)
    ap.add_argument("--pcs", type=int, default=10)
    ap.add_argument("--walkers", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--forms", default="off,auto,0,1,2,off")
    a = ap.parse_args()

    import golden_util as GU
    from gpemu import synthetic
    from gpemu.sampler import DeviceSampler
    model, prob, _ = GU.fixed_theta_model(a.n, a.obs, a.pcs, seed=0)
    dm = GU.device_model(model)
    dm.likelihood_setup(prob["y_exp"], prob["y_err"], prob["lo"], prob["hi"], 1.0)
    W = a.walkers
    lo, hi = prob["lo"], prob["hi"]
    X0 = synthetic.make_walkers(W, seed=1, lo=lo + 0.1 * (hi - lo), hi=hi - 0.1 * (hi - lo))
    lp0 = dm.logpost(X0)
    nblk = (W // 2 + 63) // 64
    print(f"# N={a.n} PCs={a.pcs} walkers={W}: halves of {W // 2} proposals, {nblk} blocks of 64 columns; "
          f"{a.reps} steps (2 launches each) per entry; us per launch (HIP event pairs)")
    print(f"{'form':>5} {'blocks':>6} {'live':>5} {'kstar':>8} {'trmm':>8} {'sum':>8} {'live_fraction':>13}")
    for form in a.forms.split(","):
        os.environ.pop("GPEMU_NO_COMPACT", None)
        os.environ.pop("GPEMU_COMPACT_FORM", None)
        if form == "off":
            os.environ["GPEMU_NO_COMPACT"] = "1"
        elif form != "auto":
            os.environ["GPEMU_COMPACT_FORM"] = form
        for c in ([nblk] if form == "off" else range(1, nblk + 1)):    # (off: every proposal inside, the parent's launch)
            live = min(64 * c, W // 2)
            ds = DeviceSampler([dm], W, seed=1)
            ds.set_state(X0, lp0)        # (a stretch of 1 leaves the walkers where they are: they all stay inside)
            rng = np.random.default_rng(c)
            steps = [draws(W, live, rng) for _ in range(a.reps)]
            for warm in (True, False):
                if not warm:
                    dm.profile(True)
                for d in steps[:10] if warm else steps:
                    ds.step_host_rng(*d, store=False)
            prof = dm.profile_read()
            dm.profile(False)
            frac = ds.live_fraction
            ds.close()
            ks = 1e3 * prof["kstar"][0] / max(prof["kstar"][1], 1)
            tr = 1e3 * prof["trmm_vsq"][0] / max(prof["trmm_vsq"][1], 1)
            print(f"{form:>5} {c:>6} {live:>5} {ks:>8.2f} {tr:>8.2f} {ks + tr:>8.2f} "
                  f"{'-' if frac is None else format(frac, '.4f'):>13}", flush=True)
    dm.close()


if __name__ == "__main__":
    main()
