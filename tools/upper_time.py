#!/usr/bin/env python3
"""What the upper bound costs after a solve, on the device and on the host.  One process, one context on an ny x nx x nt grid
(default 1024 x 1024 x 128) after a short inPALM run; then
  (a) ctx.upper_bound(eps_h2, max_sweeps): one warm-up call, then --reps timed calls (the C call returns after its own
      synchronise, so the host clock around it measures the work: the uploads of rho, 2 * sweeps + 4 soft transforms of two
      passes each, the node kernels and their reductions, one scalar back per sweep), with the per-kernel device times of the
      library's own profiling (HIP events around the launches);
  (b) the numpy twin upper.sinkhorn_round() at --twin-n x --twin-n (default 257 x 257) beside the stateless device call on the
      same problem, with the distance of the two results (--no-twin: not at all).
usage: python tools/upper_time.py [--grid NY NX NT] [--iters K] [--reps R] [--eps-h2 E] [--sweeps S] [--twin-n N] [--no-twin]
                                  [--out profiles/upper_time.txt]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402
from dotsocp_amd import capi, upper as U  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grid", nargs=3, type=int, default=[1024, 1024, 128])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--eps-h2", type=float, default=0.25)
ap.add_argument("--sweeps", type=int, default=50)
ap.add_argument("--twin-n", type=int, default=257)
ap.add_argument("--no-twin", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "upper_time.txt"))
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
kw = dict(eps_h2=args.eps_h2, max_sweeps=args.sweeps)
try:
    ctx.run(-1)
    ctx.finish(download=False)
    transforms = 2 * args.sweeps + 4
    cand = ny * nx * (nx + ny)
    say(f"{ny} x {nx} x {nt} after {args.iters} inPALM iterations; upper_bound(eps = {args.eps_h2} h^2, {args.sweeps} sweeps): "
        f"{transforms} soft transforms of {cand / 1e9:.2f} G candidates each, scanned twice (min, then sums)")
    ctx.upper_bound(**kw)                                      # warm-up: the scratch comes out of the block cache afterwards
    capi.check(capi.lib().dotsocp_set_profiling(ctx._ctx, 1))
    t = []
    for rep in range(args.reps):
        t0 = time.perf_counter()
        dev = ctx.upper_bound(**kw)
        t.append(time.perf_counter() - t0)
        say(f"  call {rep}: {t[-1] * 1e3:9.3f} ms")
    capi.check(capi.lib().dotsocp_set_profiling(ctx._ctx, 0))
    say(f"median of {args.reps}: upper_bound() {float(np.median(t)) * 1e3:.3f} ms (host clock, everything included; "
        f"with profiling on, which adds two events per launch)")
    total = 0.0
    for name, what, n_cand in (("sl_pass_x", "k_sl_pass_x (strided axis)", ny * nx * nx), ("sl_pass_y", "k_sl_pass_y (contiguous axis)", nx * ny * ny),
                               ("sl_node", "node kernels + k_report_final", 0)):
        ms, n = ctx.kernel_time(name)
        per_call = ms * n / args.reps
        total += per_call
        say(f"  {what:32s}: {ms:9.4f} ms per launch, {n // args.reps} per call = {per_call:9.3f} ms per call"
            + (f" = {2 * n_cand / (ms * 1e-3) / 1e12:.2f} T candidate visits/s" if n_cand else ""))
    say(f"  kernels together: {total:.3f} ms per call")
    t0 = time.perf_counter()
    ctx.upper_bound(**kw)
    say(f"  one call without profiling: {(time.perf_counter() - t0) * 1e3:.3f} ms")
    t0 = time.perf_counter()
    full = ctx.upper_bound(arrays=True, **kw)
    say(f"  with f, g, E, er, ec downloaded ({5 * 8 * ny * nx / 1e6:.1f} MB): {(time.perf_counter() - t0) * 1e3:.3f} ms")
    lo = ctx.dual_bound()
    say("  " + str(dev))
    say(f"  bracket: {lo['bound']:.10g} <= W2^2 <= {dev['upper']:.10g}  (upper / bound {dev['upper'] / lo['bound']:.6f})")
finally:
    ctx.close()
if not args.no_twin:
    n = args.twin_n
    r0, r1 = D.get_example_2d("example1", n, n)
    t0 = time.perf_counter()
    d = U.plan_bound(r0, r1, None, arrays=True, **kw)
    t1 = time.perf_counter()
    w = U.sinkhorn_round(r0, r1, None, **kw)
    t2 = time.perf_counter()
    far = {k: float(np.max(np.abs(d[k] - w[k]))) for k in ("f", "g", "E", "er", "ec", "defects")}
    say(f"{n} x {n}, cold start, the same sweeps: stateless device call {(t1 - t0) * 1e3:.3f} ms (uploads, downloads and the first "
        f"call's allocations included), numpy twin {t2 - t1:.3f} s")
    say(f"  device upper {d['upper']:.15g}, twin {w['upper']:.15g}; largest distances " + ", ".join(f"{k} {v:.2e}" for k, v in far.items()))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
