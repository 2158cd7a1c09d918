#!/usr/bin/env python3
"""What the pushed density costs after a solve, on the device and on the host.  One process, one context on an
ny x nx x nt grid (default 1024 x 1024 x 128) after a short inPALM run, one particle per node of the first layer (grid
order) with rho0 there as its mass, frames at every --every-th node (default 16):
  (b) ctx.push_forward(...) -- the march of ctx.advect plus, per frame, one k_deposit and one k_frame_l1 launch and the
      download of the frame; host clock around the call and the per-kernel device times of the profiling hooks
      (dotsocp_kernel_time "velocity_layer" / "advect" / "deposit" / "frame_l1"), one warm-up call and --reps timed ones;
  (a) the host route: ctx.advect(..., trajectories=True) (n x nt positions per axis downloaded), ctx.outputs() for rho, and
      the twin's deposit (np.add.at on int64 planes) and l1 per frame.  Its frames are compared with the device's, bit
      for bit.
k_deposit issues four 64-bit integer atomic adds per particle: 32 bytes added per particle and frame; that byte count over
the kernel's time is the atomic rate reported, beside the 1.3 TB/s measured for float atomics of the same shape.
usage: python tools/push_time.py [--grid NY NX NT] [--iters K] [--nsub S] [--every E] [--reps R] [--no-host]
                                 [--out profiles/push_time.txt]"""
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
ap.add_argument("--every", type=int, default=16)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "push_time.txt"))
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
    frames = list(range(0, nt, args.every))
    n, nf = x0.size, len(frames)
    floor = A.default_rho_floor(rho0, rho1)
    say(f"{ny} x {nx} x {nt} after {args.iters} inPALM iterations; {n} particles (one per node, grid order, mass rho0), nsub {args.nsub}, "
        f"{nf} frames at the nodes {frames[0]}, {frames[1] if nf > 1 else '-'}, .. {frames[-1]}; a frame adds {32 * n / 1e6:.1f} MB")
    capi.check(capi.lib().dotsocp_set_profiling(ctx._ctx, 1))
    names = ("velocity_layer", "advect", "deposit", "frame_l1")
    tb, dev = [], None
    base = {k: (0.0, 0) for k in names}
    for rep in range(-1, args.reps):
        t0 = time.perf_counter()
        dev = ctx.push_forward(x0, y0, mass=mass, frames=frames, nsub=args.nsub, rho_floor=floor)
        t1 = time.perf_counter()
        say(f"  {'warm-up' if rep < 0 else f'call {rep}'}: (b) ctx.push_forward {t1 - t0:8.5f} s, {dev['n_clamped']} clamped")
        if rep < 0:
            base = {k: ctx.kernel_time(k) for k in names}
        else:
            tb.append(t1 - t0)
    kt = {}
    for k in names:
        ms, cnt = ctx.kernel_time(k)
        ms0, cnt0 = base[k]
        kt[k] = ((ms * cnt - ms0 * cnt0) / max(cnt - cnt0, 1), cnt - cnt0)
    say("  per launch (the timed calls): " + ", ".join(f"{k} {kt[k][0] * 1e3:8.1f} us x {kt[k][1]}" for k in names))
    per_call = {k: kt[k][0] * kt[k][1] / args.reps for k in names}
    b = float(np.median(tb))
    say(f"  device time per call: " + ", ".join(f"{k} {per_call[k]:.3f} ms" for k in names)
        + f"; deposit / advect = {per_call['deposit'] / per_call['advect']:.3f}, "
        f"deposit + frame_l1 = {100 * (per_call['deposit'] + per_call['frame_l1']) / (1e3 * b):.1f} % of the call")
    say(f"  k_deposit adds {32 * n / 1e6:.1f} MB per launch with 64-bit integer atomics: "
        f"{32 * n / (kt['deposit'][0] * 1e-3) / 1e12:.2f} TB/s (float atomics of this shape: 1.3 TB/s)")
    units = dev["counts"].sum(axis=(0, 1))
    say(f"  units per frame - total units: {(units - dev['total_units']).tolist()} (unit 2^{int(np.log2(dev['unit']))})")
    say(f"  l1 against rho at the frame nodes: " + " ".join(f"{v:.3e}" for v in dev["l1"]))
    say(f"median of {args.reps}: (b) {b:.5f} s")
    if not args.no_host:
        t0 = time.perf_counter()
        tr = ctx.advect(x0, y0, nsub=args.nsub, rho_floor=floor, trajectories=True)
        t1 = time.perf_counter()
        rho = ctx.outputs()["rho"]
        t2 = time.perf_counter()
        M = np.rint(mass / dev["unit"]).astype(np.int64)
        same, l1 = True, []
        for k, node in enumerate(frames):
            plane = np.zeros((ny, nx), dtype=np.int64)
            A._deposit(plane, tr["traj_x"][:, node], tr["traj_y"][:, node], M)
            fr = plane.astype(np.float64) * dev["unit"]
            l1.append(float(np.mean(np.abs(fr - rho[..., node]))))
            same = same and fr.tobytes() == np.ascontiguousarray(dev["frames"][..., k]).tobytes()
        t3 = time.perf_counter()
        a = t3 - t0
        say(f"  (a) trajectories {t1 - t0:8.4f} s + outputs {t2 - t1:8.4f} s + deposit and l1 of {nf} frames on the host {t3 - t2:8.4f} s "
            f"= {a:8.3f} s")
        say(f"  the host route's frames == the device's, bit for bit: {same}; "
            f"l1 largest relative difference {np.max(np.abs(np.array(l1) - dev['l1']) / dev['l1']):.1e}")
        say(f"(a) / (b) = {a / b:.0f}x")
finally:
    ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
