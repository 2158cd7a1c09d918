#!/usr/bin/env python3
"""What the geodesic's profile costs after a solve, on the host and on the device.  One process, one context on an
ny x nx x nt grid (default 1024 x 1024 x 128) after a short inPALM run; then, alternating in one process (one warm-up
round, then --reps timed rounds):
  (a) ctx.geodesic()  one pass over alpha on the device (k_geodesic), 13 numbers per layer back;
  (b) ctx.report()    the solution report's pass over alpha and q (k_report), the yardstick;
  (c) ctx.outputs() + the numpy twin geodesic.geodesic_profile(output): six grid-sized arrays over the host link.
Every step ends in a device synchronise of its own (the C calls return after sync_all()), so host clocks around them
measure the work.  The device's profile and the twin's of the last round are compared.
usage: python tools/geodesic_time.py [--grid NY NX NT] [--iters K] [--reps R] [--out profiles/geodesic_time.txt]
--only-device: (a) and (b) alone, nothing written -- for `rocprofv3 --kernel-trace --stats -- python tools/geodesic_time.py
--only-device`, which gives the kernels' own times."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402
from dotsocp_amd import geodesic as G  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grid", nargs=3, type=int, default=[1024, 1024, 128])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--only-device", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "geodesic_time.txt"))
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
    say(f"{ny} x {nx} x {nt} after {args.iters} inPALM iterations; geodesic: {8 * nq / 1e9:.2f} GB read from device memory (alpha once), "
        f"report: {2 * 8 * nq / 1e9:.2f} GB (alpha and q once), outputs: {out_bytes / 1e9:.2f} GB over the host link")
    ta, tb, tc = [], [], []
    for rep in range(-1, args.reps):
        t0 = time.perf_counter()
        dev = ctx.geodesic()
        t1 = time.perf_counter()
        ctx.report()
        t2 = time.perf_counter()
        tag = "warm-up" if rep < 0 else f"round {rep}"
        if args.only_device:
            print(f"  {tag}: geodesic {t1 - t0:8.5f} s | report {t2 - t1:8.5f} s", flush=True)
            continue
        out = ctx.outputs()
        t3 = time.perf_counter()
        twin = G.geodesic_profile(out)
        t4 = time.perf_counter()
        say(f"  {tag}: (a) geodesic {t1 - t0:8.5f} s | (b) report {t2 - t1:8.5f} s | (c) outputs {t3 - t2:8.4f} s + twin {t4 - t3:8.4f} s = "
            f"{t4 - t2:8.4f} s | (a) / (b) {(t1 - t0) / (t2 - t1):5.2f}, (c) / (a) {(t4 - t2) / (t1 - t0):7.1f}x")
        if rep >= 0:
            ta.append(t1 - t0)
            tb.append(t2 - t1)
            tc.append((t3 - t2, t4 - t2))
        if rep < args.reps - 1:
            out = twin = None
    if args.only_device:
        print("  " + dev.summary())
        sys.exit(0)
    N = ny * nx
    worst = {}
    for name, term in zip(G.NAMES, G.layer_terms(out)):
        scale = np.abs(term.reshape((N, -1), order="F")).mean(axis=0)
        worst[name] = float(np.max(np.abs(dev[name] - twin[name]) / np.where(scale > 0, scale, 1.0)))
    say("  device against twin, worst |difference| / mean|term| per layer mean: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    say(f"  rho_max equal: {np.array_equal(dev['rho_max'], twin['rho_max'])}; n_support equal: {np.array_equal(dev['n_support'], twin['n_support'])}; "
        f"cost {dev['cost']:.15g} / {twin['cost']:.15g}")
    say("  " + dev.summary())
    med = lambda v: float(np.median(v))         # noqa: E731
    a, b, o, c = med(ta), med(tb), med([x[0] for x in tc]), med([x[1] for x in tc])
    say(f"median of {args.reps}: (a) geodesic {a:.5f} s, (b) report {b:.5f} s, outputs alone {o:.4f} s, (c) {c:.4f} s; "
        f"(a) / (b) = {a / b:.2f}, outputs / (a) = {o / a:.1f}x, (c) / (a) = {c / a:.1f}x")
finally:
    ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
