#!/usr/bin/env python3
"""What "is the solution any good" costs after a solve, on the host and on the device.  One process, one context on an
ny x nx x nt grid (default 1024 x 1024 x 128) after a short inPALM run; then, as same-run pairs (one warm-up pair, then
--reps timed pairs, the two ways alternating):
  (a) ctx.outputs() (six k_outputs launches, six staging copies, 8 (3 Nphi + 3 Nz) bytes over the host link)
      + check_massConservation(rho) + the host twin report.solution_report(output);
  (b) ctx.report() (one pass over alpha and q on the device, ~110 scalars + two per layer back).
Every step ends in a device synchronise of its own (the C calls return after sync_all()), so host clocks around them
measure the work.  The two reports of the last pair are compared (integers equal, sums to rounding).
usage: python tools/report_time.py [--grid NY NX NT] [--iters K] [--reps R] [--out profiles/report_time.txt]
--only-report: (b) alone, nothing written -- for `rocprofv3 --kernel-trace --stats -- python tools/report_time.py --only-report`,
which gives k_report's own time."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grid", nargs=3, type=int, default=[1024, 1024, 128])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only-report", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "report_time.txt"))
args = ap.parse_args()
ny, nx, nt = args.grid
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


rho0, rho1 = D.get_example_2d("example1", nx, ny)
var, model = D.initialize(rho0, rho1, nt, lazy_zeros=True)
D.InitialScaling(var, model, True, None, dim=2)
ctx = D.InPALMContext(var, dict(tau=1.9, sigma=1.0, tol=0.0, maxit=args.iters, scaling=True), model)
try:
    ctx.run(-1)
    ctx.finish(download=False)
    nq = (nt - 1) * nx * ny + nt * (nx - 1) * ny + nt * nx * (ny - 1)
    out_bytes = 8 * ny * nx * (3 * nt + 3 * (nt - 1))
    say(f"{ny} x {nx} x {nt} after {args.iters} inPALM iterations; outputs: {out_bytes / 1e9:.2f} GB over the host link, "
        f"report: {2 * 8 * nq / 1e9:.2f} GB read from device memory (alpha and q once)")
    if args.only_report:
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            dev = ctx.report()
            print(f"  report {time.perf_counter() - t0:8.5f} s", flush=True)
        print("  " + dev.summary())
        sys.exit(0)
    ta, tb = [], []
    for rep in range(-1, args.reps):
        t0 = time.perf_counter()
        out = ctx.outputs()
        t1 = time.perf_counter()
        ok_host = D.check_massConservation(out["rho"], 1e-2)
        t2 = time.perf_counter()
        twin = D.solution_report(out)
        t3 = time.perf_counter()
        dev = ctx.report()
        t4 = time.perf_counter()
        tag = "warm-up" if rep < 0 else f"pair {rep}"
        say(f"  {tag}: (a) outputs {t1 - t0:8.4f} s + check_massConservation {t2 - t1:7.4f} s + host twin {t3 - t2:8.4f} s = "
            f"{t3 - t0:8.4f} s | (b) report {t4 - t3:8.5f} s | outputs / report {(t1 - t0) / (t4 - t3):7.1f}x, (a) / (b) {(t3 - t0) / (t4 - t3):7.1f}x")
        if rep >= 0:
            ta.append((t1 - t0, t3 - t0))
            tb.append(t4 - t3)
        if rep < args.reps - 1:
            out = twin = None
    ints = ("n_nodes", "n_cells", "rho_neg", "fq_pos", "nonfinite")
    same = all(dev[k] == twin[k] for k in ints) and np.array_equal(dev["rho_hist"], twin["rho_hist"]) and \
        np.array_equal(dev["fq_hist"], twin["fq_hist"]) and dev["rho_min"] == twin["rho_min"] and dev["fq_max"] == twin["fq_max"]
    say(f"  device report == host twin on counts, histograms, min(rho), max(fq): {same}; cost {dev['cost']:.15g} / {twin['cost']:.15g}; "
        f"mass_ok {dev.mass_ok()} / {twin.mass_ok()} / {ok_host}")
    say("  " + dev.summary())
    med = lambda v: float(np.median(v))         # noqa: E731
    o, a, b = med([x[0] for x in ta]), med([x[1] for x in ta]), med(tb)
    say(f"median of {args.reps}: outputs alone {o:.4f} s, (a) {a:.4f} s, (b) {b:.5f} s; outputs / (b) = {o / b:.1f}x, (a) / (b) = {a / b:.1f}x "
        f"(bar: (b) at least 10x faster than outputs alone: {'met' if o / b >= 10 else 'MISSED'})")
finally:
    ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
