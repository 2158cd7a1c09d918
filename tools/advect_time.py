#!/usr/bin/env python3
"""What "where does the mass go" costs after a solve, on the device and on the host.  One process, one context on an
ny x nx x nt grid (default 1024 x 1024 x 128) after a short inPALM run, one seed per node of the first layer (grid order),
nsub steps per time interval:
  (b) ctx.advect(...) -- one k_velocity_layer launch per node layer, one k_advect launch per time interval; host clock
      around the call (it returns after a synchronise) and the per-kernel device times of the profiling hooks
      (dotsocp_kernel_time "velocity_layer" / "advect"), one warm-up call and --reps timed ones;
  (a) the host route: ctx.outputs() (timed), the node velocity advect.velocity(output) on the whole grid (timed), and the
      numpy twin advect.advect on a SAMPLE of --sample seeds, whose particle part (its time minus the velocity's) is
      SCALED by n / sample -- labelled as scaled below.  The sample's positions are compared with the device's, bit for bit.
k_advect gathers nsub x 4 stages x 2 layers x 2 components x 4 corners doubles per particle and interval; that logical byte
count over the kernel's time is the gather rate reported, beside the 8.6 TB/s the chip reads uniformly random rows of a
38 MB table at out of its last-level cache (two velocity layers of two components are 34 MB at 1024 x 1024).
usage: python tools/advect_time.py [--grid NY NX NT] [--iters K] [--nsub S] [--reps R] [--sample M] [--order grid|random]
                                   [--no-host] [--out profiles/advect_time.txt]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402
from dotsocp_amd import advect as A, capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grid", nargs=3, type=int, default=[1024, 1024, 128])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--nsub", type=int, default=1)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sample", type=int, default=16384)
ap.add_argument("--order", choices=("grid", "random"), default="grid")
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "advect_time.txt"))
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
    x0, y0 = A.seeds_on_nodes(nx, ny)
    if args.order == "random":
        perm = np.random.default_rng(1).permutation(x0.size)
        x0, y0 = x0[perm], y0[perm]
    n = x0.size
    floor = A.default_rho_floor(rho0, rho1)
    say(f"{ny} x {nx} x {nt} after {args.iters} inPALM iterations; {n} seeds (one per node, {args.order} order), nsub {args.nsub}, "
        f"rho_floor {floor:.4g}; two velocity layers of two components: {4 * 8 * ny * nx / 1e6:.1f} MB")
    capi.check(capi.lib().dotsocp_set_profiling(ctx._ctx, 1))
    tb, dev = [], None
    base = {k: (0.0, 0) for k in ("velocity_layer", "advect")}
    for rep in range(-1, args.reps):
        t0 = time.perf_counter()
        dev = ctx.advect(x0, y0, nsub=args.nsub, rho_floor=floor)
        t1 = time.perf_counter()
        say(f"  {'warm-up' if rep < 0 else f'call {rep}'}: (b) ctx.advect {t1 - t0:8.5f} s, {dev['n_clamped']} clamped")
        if rep < 0:
            base = {k: ctx.kernel_time(k) for k in base}
        else:
            tb.append(t1 - t0)
    kt = {}
    for k in base:
        ms, cnt = ctx.kernel_time(k)
        ms0, cnt0 = base[k]
        kt[k] = ((ms * cnt - ms0 * cnt0) / max(cnt - cnt0, 1), cnt - cnt0)
    gathered = n * args.nsub * 4 * 16 * 8
    say(f"  per launch (the timed calls): k_velocity_layer {kt['velocity_layer'][0] * 1e3:8.1f} us x {kt['velocity_layer'][1]}, "
        f"k_advect {kt['advect'][0] * 1e3:8.1f} us x {kt['advect'][1]}")
    say(f"  k_advect gathers {gathered / 1e6:.0f} MB per launch: {gathered / (kt['advect'][0] * 1e-3) / 1e12:.2f} TB/s "
        f"(uniformly random rows out of the last-level cache: 8.6 TB/s)")
    moved = np.hypot((dev["x"] - np.clip(x0, 0, 1)) * (nx - 1), (dev["y"] - np.clip(y0, 0, 1)) * (ny - 1))
    say(f"  displacement of the particles in grid cells: mean {moved.mean():.1f}, largest {moved.max():.1f} "
        f"(neighbouring particles stay neighbours only while the flow is smooth: the gather rate is this flow's)")
    b = float(np.median(tb))
    say(f"median of {args.reps}: (b) {b:.5f} s")
    if not args.no_host:
        t0 = time.perf_counter()
        out = ctx.outputs()
        t1 = time.perf_counter()
        out = {k: out[k] for k in ("rho", "Ex", "Ey")}
        A.velocity(out, floor)
        t2 = time.perf_counter()
        m = min(args.sample, n)
        pick = np.random.default_rng(2).choice(n, m, replace=False)
        twin = A.advect(out, x0[pick], y0[pick], nsub=args.nsub, rho_floor=floor)
        t3 = time.perf_counter()
        part = max((t3 - t2) - (t2 - t1), 0.0)
        same = twin["x"].tobytes() == dev["x"][pick].tobytes() and twin["y"].tobytes() == dev["y"][pick].tobytes()
        a = (t1 - t0) + (t2 - t1) + part * n / m
        say(f"  (a) outputs {t1 - t0:8.4f} s + node velocity on the host {t2 - t1:8.4f} s + twin on {m} seeds {t3 - t2:8.4f} s "
            f"(its particle part {part:8.4f} s, SCALED by {n / m:.0f} to {part * n / m:8.2f} s) = {a:8.2f} s (scaled)")
        say(f"  the sample's positions on the device == twin, bit for bit: {same}")
        say(f"(a, scaled) / (b) = {a / b:.0f}x; outputs alone / (b) = {(t1 - t0) / b:.1f}x")
finally:
    ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
