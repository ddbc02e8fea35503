#!/usr/bin/env python3
"""Timing of the pairwise log-sum-exp behind the expected information gain on the device.

    timeout 900 python tools/bench_experiment.py [--n 65536] [--s 65536] [--f 4,32,256] [--reps 5] [--no-torch]
                                                 [--mfma-tflops 77.51]

Workload: n outer rows y_i = z_i + eps_i against S inner rows z_j ~ N(0, I_F) / sqrt(F) * 3 (a whitened candidate of a
few nats), dense float64 device tensors.  Timed with a host clock around calls that end in a device synchronise, one
warm-up each and --reps repeats (median, min and max):
  pair_lse  gpemu.experiment.pair_lse on the device tensors: the column means, the two centring passes, the partial
            kernel and the merge
Beside it the pair rate n S / t, the matrix-core rate 2 n S 4 ceil(F / 4) / t in TF and what that is of the measured fp64
matrix rate (profiles/r01_fp64_rates.txt, `mfma_f64_16x16x4 only` at 4 waves per SIMD: --mfma-tflops), and the
exponentials per second (one per pair).
  torch     torch.cdist + torch.logsumexp in float64 on the same tensors, the n rows in chunks whose n_chunk x S matrix
            stays below 2 GiB (whole, it would be 8 n S bytes = 34 GB at 65536^2), for information only.
One JSON line per F."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayesian-inference_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--s", type=int, default=65536)
    ap.add_argument("--f", type=str, default="4,32,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--mfma-tflops", type=float, default=77.51)
    args = ap.parse_args()
    import torch
    from bench_marginals import timed
    from gpemu import _lib
    from gpemu import experiment as E
    if _lib.device_count() <= 0 or not torch.cuda.is_available():
        raise SystemExit("bench_experiment: no GPU visible; nothing is measured without one")
    n, S = args.n, args.s
    dev = torch.device("cuda", 0)
    for F in (int(v) for v in args.f.split(",")):
        g = torch.Generator(device=dev).manual_seed(F)
        Z = torch.randn((S, F), dtype=torch.float64, device=dev, generator=g) * (3.0 / F ** 0.5)
        Y = Z[(torch.arange(n, device=dev) * S) // n] + torch.randn((n, F), dtype=torch.float64, device=dev, generator=g)
        rec = {"n": n, "S": S, "F": F, "reps": args.reps}
        c0 = E.path_counts()
        lse, ess = E.pair_lse(Y, Z)
        c1 = E.path_counts()
        rec["launches"] = {key: c1[key] - c0[key] for key in c1}
        rec["ess_mean"] = float(ess.mean())
        rec["pair_lse"] = timed(lambda: E.pair_lse(Y, Z), args.reps)
        t = rec["pair_lse"]["median_s"]
        rec["pairs_per_s"] = float(n) * S / t
        rec["mfma_tflops"] = 2.0 * float(n) * S * (4 * ((F + 3) // 4)) / t / 1e12
        rec["fraction_of_mfma_rate"] = rec["mfma_tflops"] / args.mfma_tflops
        rec["exp_per_s"] = float(n) * S / t
        if not args.no_torch:
            rows = max(1, min(n, (2 << 30) // (8 * S)))

            def torch_lse():
                out = torch.empty(n, dtype=torch.float64, device=dev)
                for a in range(0, n, rows):
                    d = torch.cdist(Y[a:a + rows], Z)
                    out[a:a + rows] = torch.logsumexp(-0.5 * d * d, dim=1)
                return out

            ref = torch_lse()
            rec["torch_max_abs_diff"] = float((ref - lse).abs().max())
            rec["torch_cdist_logsumexp"] = timed(torch_lse, max(1, min(args.reps, 3)))
            rec["torch_rows_per_chunk"] = rows
            del ref
        print(json.dumps(rec), flush=True)
        del Y, Z, lse, ess


if __name__ == "__main__":
    main()
