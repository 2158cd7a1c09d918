#!/usr/bin/env python3
"""What the map report costs after a solve, on the device and on the host.  One process, one context on an ny x nx x nt
grid (default 1024 x 1024 x 128) after a short inPALM run, one particle per node of the first layer (grid order) with rho0
there as its mass:
  (b) ctx.map_report(...) -- the accumulating march (k_advect<., true>: the path sums read and written per particle and
      launch, 32 bytes on top of the gathers) and one k_map_final; host clock around the call, and
  (c) ctx.advect(...) on the same state and seeds -- the plain march, the yardstick;
      both with the per-kernel device times of the profiling hooks (dotsocp_kernel_time "velocity_layer" / "advect" /
      "advect_path" / "map_final"), one warm-up call and --reps timed ones each;
  (a) the host route: ctx.advect(..., trajectories=True) (n x nt positions per axis downloaded) and numpy over the columns:
      step lengths, their sums, displacement, the six sums in the twin's order.  (With nsub = 1 the trajectories hold every
      step, so this gives the device's per-particle values; they are compared.)
usage: python tools/map_report_time.py [--grid NY NX NT] [--iters K] [--nsub S] [--reps R] [--no-host]
                                       [--out profiles/map_report_time.txt]"""
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
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "map_report_time.txt"))
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
    mass = A.masses_on_nodes(model.rho0)
    n = x0.size
    floor = A.default_rho_floor(rho0, rho1)
    say(f"{ny} x {nx} x {nt} after {args.iters} inPALM iterations; {n} particles (one per node, grid order, mass rho0), nsub {args.nsub}")
    capi.check(capi.lib().dotsocp_set_profiling(ctx._ctx, 1))
    names = ("velocity_layer", "advect", "advect_path", "map_final")

    def timed(label, call):
        """one warm-up and --reps timed calls: median wall time, per-launch device times of the timed calls, last result"""
        ts, res = [], None
        base = {k: (0.0, 0) for k in names}
        for rep in range(-1, args.reps):
            t0 = time.perf_counter()
            res = call()
            t1 = time.perf_counter()
            say(f"  {'warm-up' if rep < 0 else f'call {rep}'}: {label} {t1 - t0:8.5f} s, {res['n_clamped']} clamped")
            if rep < 0:
                base = {k: ctx.kernel_time(k) for k in names}
            else:
                ts.append(t1 - t0)
        kt = {}
        for k in names:
            ms, cnt = ctx.kernel_time(k)
            ms0, cnt0 = base[k]
            kt[k] = ((ms * cnt - ms0 * cnt0) / max(cnt - cnt0, 1), cnt - cnt0)
        say("  per launch (the timed calls): " + ", ".join(f"{k} {kt[k][0] * 1e3:8.1f} us x {kt[k][1]}" for k in names if kt[k][1]))
        return float(np.median(ts)), kt, res

    b, ktb, dev = timed("(b) ctx.map_report", lambda: ctx.map_report(x0, y0, mass=mass, nsub=args.nsub, rho_floor=floor, per_particle=True))
    c, ktc, adv = timed("(c) ctx.advect    ", lambda: ctx.advect(x0, y0, nsub=args.nsub, rho_floor=floor))
    assert dev["x"].tobytes() == adv["x"].tobytes() and dev["y"].tobytes() == adv["y"].tobytes() and dev["n_clamped"] == adv["n_clamped"]
    pa, pl, fin = ktb["advect_path"][0], ktc["advect"][0], ktb["map_final"][0]
    say(f"median of {args.reps}: (b) ctx.map_report {b:.5f} s, (c) ctx.advect {c:.5f} s, (b) / (c) = {b / c:.3f}")
    say(f"  accumulating march {pa * 1e3:.1f} us per launch against the plain k_advect {pl * 1e3:.1f} us: x {pa / pl:.3f} "
        f"(32 B per particle and launch more: {32 * n / 1e6:.1f} MB, {32 * n / max(pa - pl, 1e-9) / 1e9:.2f} TB/s if the difference were traffic alone); "
        f"k_map_final {fin * 1e3:.1f} us, once")
    say(f"  report: cost_map {dev['cost_map']:.6f} <= cost_length {dev['cost_length']:.6f} <= cost_action {dev['cost_action']:.6f}; "
        f"detour_max {dev['detour_max']:.3e}, {dev['detour_over']} over 10 %, {dev['n_still']} still")
    if not args.no_host:
        t0 = time.perf_counter()
        tr = ctx.advect(x0, y0, nsub=args.nsub, rho_floor=floor, trajectories=True)
        t1 = time.perf_counter()
        sq, ln = np.zeros(n), np.zeros(n)
        for k in range(nt - 1):
            ex, ey = tr["traj_x"][:, k + 1] - tr["traj_x"][:, k], tr["traj_y"][:, k + 1] - tr["traj_y"][:, k]
            s2 = ex * ex + ey * ey
            sq, ln = sq + s2, ln + np.sqrt(s2)
        dx, dy = tr["traj_x"][:, -1] - tr["traj_x"][:, 0], tr["traj_y"][:, -1] - tr["traj_y"][:, 0]
        disp2 = dx * dx + dy * dy
        disp, action = np.sqrt(disp2), sq * float(nt - 1)
        total = A._tree_sum(mass)
        sums = [A._tree_sum(mass * t) / total for t in (disp2, ln * ln, action, disp, ln)]
        t2 = time.perf_counter()
        a = t2 - t0
        say(f"  (a) trajectories {t1 - t0:8.4f} s ({2 * n * nt * 8 / 1e9:.2f} GB downloaded) + numpy over the columns {t2 - t1:8.4f} s = {a:8.3f} s")
        if args.nsub == 1:
            same = all(u.tobytes() == v.tobytes() for u, v in ((disp, dev["disp"]), (ln, dev["len"]), (action, dev["action"])))
            say(f"  the host route's disp, len, action == the device's, bit for bit: {same}; cost_map {sums[0] == dev['cost_map']}, "
                f"cost_length {sums[1] == dev['cost_length']}, cost_action {sums[2] == dev['cost_action']}")
        say(f"(a) / (b) = {a / b:.0f}x")
finally:
    ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
