#!/usr/bin/env python3
"""Set-up time of the weighted multilevel driver with the levels' weights made on the host and on the device:
solver_wdotsocp2d with the circle-pillar barrier, inPALM, tol 1e-3, weights="host" (the Nq array, numpy restriction,
one upload per level) and weights="device" (a SpaceWeight, the weight pyramid) alternating, three runs each.  Per run:
wall time of the call, the sum of the per-level loop seconds, and their difference -- the set-up.
usage: weights_setup_time.py [--maxit M] [--runs R] [n nt levelN] ...      (python tools/weights_setup_time.py > profiles/weights_setup.txt)
--only device|host: that path alone (a rocprofv3 --kernel-trace --stats run of the device path gives k_weight_restrict's times)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--maxit", type=int, default=10000)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--only", choices=["device", "host"])
ap.add_argument("cases", nargs="*", type=int)
args = ap.parse_args()
cases = [(257, 65, 3), (513, 129, 4)]
if args.cases:
    cases = [tuple(args.cases[i:i + 3]) for i in range(0, len(args.cases), 3)]
barrier = D.gene_barrier_of_circle_pillar()
# a small solve first: the timed runs do not pay for loading the library and the code objects
r0, r1, _ = D.ensure_barrier_validity(*D.get_example_2d("example1", 33, 33), barrier)
for mode, w in (("host", D.get_weight_by_barrier(33, 33, 17, barrier)), ("device", D.get_space_weight_by_barrier(33, 33, barrier))):
    if not args.only or mode == args.only:
        D.solver_wdotsocp2d(r0, r1, 17, 2, dict(tol=1e-3, weight=w, maxit=20), "inPALM", barrier, weights=mode)
for n, nt, L in cases:
    rho0, rho1 = D.get_example_2d("example1", n, n)
    rho0, rho1, _ = D.ensure_barrier_validity(rho0, rho1, barrier)
    print(f"{n}x{n}x{nt}, {L} levels, circle-pillar barrier, inPALM, tol 1e-3, maxit {args.maxit}", flush=True)
    setups = {"host": [], "device": []}
    for run in range(args.runs):
        for mode in ("host", "device"):
            if args.only and mode != args.only:
                continue
            out = None
            t = time.perf_counter()
            # building the weight is part of what the caller pays: Nq entries on the host, or two 2-D arrays
            if mode == "host":
                weight = D.get_weight_by_barrier(n, n, nt, barrier)
            else:
                weight = D.get_space_weight_by_barrier(n, n, barrier)
            out, timeML, histML, hist = D.solver_wdotsocp2d(rho0, rho1, nt, L, dict(tol=1e-3, weight=weight, maxit=args.maxit),
                                                            "inPALM", barrier, weights=mode)
            wall = time.perf_counter() - t
            weight = None
            loops = sum(float(x["Total_Time"]) for x in timeML[:-1])
            its = [int(x["Iters"]) for x in timeML[:-1]]
            setups[mode].append(wall - loops)
            print(f"  run {run} weights={mode:6s}: wall {wall:7.3f} s, loops {loops:7.3f} s, set-up {wall - loops:7.3f} s, "
                  f"iterations {its}, KKT(1,3,6) {hist['kkt'][-1][[0, 2, 5]].max():.2e}", flush=True)
    if not args.only:
        ratios = [h / d for h, d in zip(setups["host"], setups["device"])]
        print("  set-up host / device per pair: " + ", ".join(f"{r:.1f}x" for r in ratios), flush=True)
