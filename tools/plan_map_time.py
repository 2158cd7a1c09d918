#!/usr/bin/env python3
"""What the transport map of the plan costs beside the bound it belongs to.  One process, one context on an ny x nx x nt grid
(default 1024 x 1024 x 33) after a short inPALM run; then, with the library's own profiling (HIP events around the launches),
  (a) the plain transform: ctx.upper_bound(max_sweeps=0) makes four plain soft transforms and nothing else in the pass
      phases -- the kernels of the parent commit, whose instructions this change leaves as they were;
  (b) the moment transform: ctx.plan_map(max_sweeps=0) makes three plain transforms and one in the moment flavour; its time per
      pass is the phase total minus three plain launches;
  (c) the whole calls at --sweeps sweeps: upper_bound() against plan_map() without frames and with three frames (host clock,
      the call returns after its own synchronise), median of --reps.
usage: python tools/plan_map_time.py [--grid NY NX NT] [--iters K] [--reps R] [--sweeps S] [--out profiles/plan_map_time.txt]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402
from dotsocp_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grid", nargs=3, type=int, default=[1024, 1024, 33])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--sweeps", type=int, default=50)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "plan_map_time.txt"))
args = ap.parse_args()
ny, nx, nt = args.grid
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


seen = {}


def phases(ctx, call):
    """per-launch time and launch count of the pass and node phases over --reps profiled calls"""
    capi.check(capi.lib().dotsocp_set_profiling(ctx._ctx, 1))
    for _ in range(args.reps):
        call()
    capi.check(capi.lib().dotsocp_set_profiling(ctx._ctx, 0))
    out = {}
    for k in ("sl_pass_x", "sl_pass_y", "sl_node"):
        ms, n = ctx.kernel_time(k)                             # the average and the count since the context was made
        tot, cnt = ms * n - seen.get(k, (0.0, 0))[0], n - seen.get(k, (0.0, 0))[1]
        seen[k] = (ms * n, n)
        out[k] = (tot / cnt, cnt)
    return out


def clock(call):
    t = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = call()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3, out


rho0, rho1 = D.get_example_2d("example1", nx, ny)
var, model = D.initialize(rho0, rho1, nt, lazy_zeros=True)
D.InitialScaling(var, model, True, None, dim=2)
ctx = D.InPALMContext(var, dict(tau=1.9, sigma=1.0, tol=0.0, maxit=args.iters, scaling=True), model)
frames = [0, nt // 2, nt - 1]
try:
    ctx.run(-1)
    ctx.finish(download=False)
    say(f"{ny} x {nx} x {nt} after {args.iters} inPALM iterations, eps = 0.25 h^2")
    ctx.plan_map(max_sweeps=1, frames=frames)                  # warm-up: the scratch comes out of the block cache afterwards
    plain = phases(ctx, lambda: ctx.upper_bound(max_sweeps=0))
    mixed = phases(ctx, lambda: ctx.plan_map(max_sweeps=0))
    for k, what in (("sl_pass_x", "x pass (strided axis)"), ("sl_pass_y", "y pass (contiguous axis)")):
        ms_p, n_p = plain[k]
        ms_m, n_m = mixed[k]
        mom = (ms_m * n_m - ms_p * 3 * args.reps) / args.reps
        say(f"  {what:26s}: plain {ms_p:8.4f} ms per launch ({n_p // args.reps} per call); moment flavour {mom:8.4f} ms "
            f"({mom / ms_p:.2f} x plain; the call's {n_m // args.reps} launches took {ms_m * n_m / args.reps:.4f} ms)")
    say(f"  node kernels and reductions per call: bound {plain['sl_node'][0] * plain['sl_node'][1] / args.reps:.4f} ms, "
        f"with the map {mixed['sl_node'][0] * mixed['sl_node'][1] / args.reps:.4f} ms")
    kw = dict(max_sweeps=args.sweeps)
    t_bound, up = clock(lambda: ctx.upper_bound(**kw))
    t_map, pm = clock(lambda: ctx.plan_map(**kw))
    t_frames, pf = clock(lambda: ctx.plan_map(frames=frames, **kw))
    say(f"whole calls at {args.sweeps} sweeps, median of {args.reps} (host clock): upper_bound() {t_bound:.3f} ms, plan_map() "
        f"{t_map:.3f} ms (five node arrays of {8 * ny * nx / 1e6:.1f} MB downloaded), with three frames and l1 {t_frames:.3f} ms")
    say("  " + str(pf))
    say("  l1 at nodes " + ", ".join(f"{k}: {v:.4e}" for k, v in zip(pf["nodes"], pf["l1"])) + f"; {pf['n_clamped']} nodes clamped")
    same = all(np.float64(up[k]).tobytes() == np.float64(pm["upper"][k]).tobytes() for k in up)
    say(f"  the bound inside plan_map() carries the bits of upper_bound(): {same}")
finally:
    ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
