#!/usr/bin/env python3
"""Host-side speed of two builds of libgpemu.so against each other, in alternation on one GPU.

    python tools/ab_libraries.py run OTHER/libgpemu.so --out ab.json [--reps 5]
    python tools/ab_libraries.py report ab.json

``run``: REPS times, for the other library (the parent commit's build) and the tree's in turn, each in child processes of
their own through GPEMU_LIBRARY: bench.py's headline and predict legs, and tools/time_logpost_grad.py (value and
value + gradient, device buffers at C3 and host buffers on the shipped three groups).  Every value is kept.  Stops at the
first child that fails.  ``report``: per leg the values, medians and spreads (largest minus smallest), and whether the
tree's median lies within the other library's own spread of the other's median."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(cmd, lib, limit):
    env = dict(os.environ, GPEMU_LIBRARY=lib)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"FAILED ({r.returncode}) {cmd} with {lib}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def run(other, out, reps):
    libs = {"parent": os.path.abspath(other), "tree": os.path.join(ROOT, "bayesian-inference_amd", "gpemu", "libgpemu.so")}
    vals = {name: {} for name in libs}
    for i in range(reps):
        # the order within a pair turns round from one repeat to the next: whatever the process before leaves behind
        # (clocks, caches) falls on both libraries alike
        for name, lib in (list(libs.items()) if i % 2 == 0 else list(libs.items())[::-1]):
            t0 = time.time()
            b = child([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20", "--no-fit",
                       "--no-extra", "--no-cpu-baseline"], lib, 300)[-1]
            vals[name].setdefault("bench headline (evals/s)", []).append(b["value"])
            vals[name].setdefault("bench gp_predict (GB/s)", []).append(b["gp_predict"]["value"])
            for r in child([sys.executable, "tools/time_logpost_grad.py", "--no-map"], lib, 300):
                key = f"{r['shape']}, blocks {r.get('blocks')}, B {r['B']}: "
                vals[name].setdefault(key + "value (ms)", []).append(r["value_ms"])
                vals[name].setdefault(key + "value + gradient (ms)", []).append(r["value_grad_ms"])
            print(f"repeat {i} {name}: {time.time() - t0:.1f} s, headline {b['value']:.0f} evals/s", flush=True)
            with open(out, "w") as f:
                json.dump(vals, f, indent=1)


def report(path):
    with open(path) as f:
        vals = json.load(f)
    for leg in vals["parent"]:
        p, t = vals["parent"][leg], vals["tree"][leg]
        mp, mt, sp, st = statistics.median(p), statistics.median(t), max(p) - min(p), max(t) - min(t)
        print(leg)
        print("  parent:", " ".join(f"{v:.6g}" for v in p), f"| median {mp:.6g}  spread {sp:.3g}")
        print("  tree:  ", " ".join(f"{v:.6g}" for v in t), f"| median {mt:.6g}  spread {st:.3g}")
        print(f"  medians differ by {abs(mt - mp):.3g} ({(mt - mp) / mp * 100:+.2f} %): "
              f"{'within' if abs(mt - mp) <= sp else 'OUTSIDE'} the parent's spread")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "report"])
    ap.add_argument("path", help="run: the other libgpemu.so; report: the JSON file of a run")
    ap.add_argument("--out", default="ab_libraries.json")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.mode == "run":
        run(a.path, a.out, a.reps)
    else:
        report(a.path)
