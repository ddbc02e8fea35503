#!/usr/bin/env python3
"""Per-kernel medians of a rocprofv3 kernel trace (--kernel-trace --output-format csv), by kernel and grid:
   python tools/kernel_trace_split.py <..._kernel_trace.csv> [min_calls]"""
import collections
import csv
import sys

WANTED = ("gemm_f64_kernel", "grad_", "trmm_vsq", "kstar_kernel", "loglik_")


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    min_calls = int(argv[2]) if len(argv) > 2 else 20
    with open(argv[1]) as handle:
        rows = list(csv.DictReader(handle))
    agg = collections.defaultdict(list)
    for r in rows:
        n = r["Kernel_Name"]
        if any(w in n for w in WANTED):
            key = (n.split("(")[0].replace("void gpemu::", "").replace("gpemu::", ""), r["Grid_Size_X"], r["Grid_Size_Y"],
                   r["Grid_Size_Z"])
            agg[key].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for k, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
        v2 = sorted(v)
        if len(v) >= min_calls:
            print(f"{k[0][:44]:44s} grid {k[1]:>7s} {k[2]:>5s} {k[3]:>3s} calls {len(v):3d} median {v2[len(v2) // 2] / 1e3:8.1f} us")


if __name__ == "__main__":
    main(sys.argv)
