#!/usr/bin/env python3
"""What the dual lower bound costs after a solve, on the device and on the host.  One process, one context on an
ny x nx x nt grid (default 1024 x 1024 x 128) after a short inPALM run; then
  (a) ctx.dual_bound(): one warm-up call, then --reps timed calls (the C call returns after its own synchronise, so the
      host clock around it measures the work: two layers scaled, two uploads of rho, four min-plus passes, one reduction,
      ~15 numbers back), with the per-kernel device times of the library's own profiling (HIP events around the launches);
  (b) the numpy twin dual.dual_bound() on the two downloaded layers, once (--no-twin: not at all).
The results of (a) and (b) are compared bit for bit.
usage: python tools/dual_time.py [--grid NY NX NT] [--iters K] [--reps R] [--no-twin] [--out profiles/dual_time.txt]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402
from dotsocp_amd import capi, dual as DU  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grid", nargs=3, type=int, default=[1024, 1024, 128])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-twin", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dual_time.txt"))
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
    cand = 2 * (ny * nx * nx + nx * ny * ny)
    say(f"{ny} x {nx} x {nt} after {args.iters} inPALM iterations; dual_bound(): {cand / 1e9:.2f} G candidates "
        f"(two transforms of two min-plus passes each)")
    ctx.dual_bound()                                           # warm-up: the scratch comes out of the block cache afterwards
    capi.check(capi.lib().dotsocp_set_profiling(ctx._ctx, 1))
    t = []
    for rep in range(args.reps):
        t0 = time.perf_counter()
        dev = ctx.dual_bound()
        t.append(time.perf_counter() - t0)
        say(f"  call {rep}: {t[-1] * 1e3:9.3f} ms")
    capi.check(capi.lib().dotsocp_set_profiling(ctx._ctx, 0))
    say(f"median of {args.reps}: dual_bound() {float(np.median(t)) * 1e3:.3f} ms (host clock, everything included)")
    total = 0.0
    for name, what in (("hl_pass_x", "k_hl_pass_x (strided axis)"), ("hl_pass_y", "k_hl_pass_y (contiguous axis)"),
                       ("hl_reduce", "k_hl_reduce + k_report_final")):
        ms, n = ctx.kernel_time(name)
        per_call = ms * n / args.reps
        total += per_call
        say(f"  {what:32s}: {ms:9.4f} ms per launch, {n // args.reps} per call = {per_call:9.4f} ms per call"
            + (f" = {cand / 4 / (ms * 1e-3) / 1e12:.2f} T candidates/s" if name != "hl_reduce" else ""))
    say(f"  kernels together: {total:.4f} ms per call")
    t0 = time.perf_counter()
    full = ctx.dual_bound(arrays=True)
    say(f"  with H, B and both winner arrays downloaded ({(2 * 8 + 2 * 4) * ny * nx / 1e6:.1f} MB): {(time.perf_counter() - t0) * 1e3:.3f} ms")
    say("  " + str(dev))
    if not args.no_twin:
        t0 = time.perf_counter()
        plane = ny * nx
        phi = np.empty(plane * nt)
        capi.check(capi.lib().dotsocp_download(ctx._ctx, capi.F_PHI, capi.fptr(phi)))
        t1 = time.perf_counter()
        p0 = (var.dScale * phi[:plane]).reshape((ny, nx), order="F")
        p1 = (var.dScale * phi[plane * (nt - 1):]).reshape((ny, nx), order="F")
        twin = DU.dual_bound(p0, p1, rho0, rho1)
        t2 = time.perf_counter()
        same = all(np.float64(full[k]).tobytes() == np.float64(twin[k]).tobytes() for k in DU.FIELDS) and \
            all(np.array_equal(full[k].view(np.uint64 if full[k].dtype == np.float64 else np.int32),
                               twin[k].view(np.uint64 if twin[k].dtype == np.float64 else np.int32))
                for k in ("H", "B", "arg_fwd", "arg_bwd"))
        say(f"host: download of phi ({8 * plane * nt / 1e9:.2f} GB) {t1 - t0:.3f} s + numpy twin on its two layers {t2 - t1:.3f} s; "
            f"same bits as the device (numbers, H, B, winners): {same}")
finally:
    ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
