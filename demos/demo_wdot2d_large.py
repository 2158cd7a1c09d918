#!/usr/bin/env python3
"""The circle-pillar obstacle of demo_wdot2d.m at the sizes of multilevel_large.py: the barrier weight is handed over as
a SpaceWeight (two 2-D arrays), so the weights of all levels are built, restricted and reduced on the GPU
(dotsocp_weights_*) and no Nq array exists on the host.  usage: demo_wdot2d_large.py [n nt levelN] ..."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402

cases = [(257, 65, 3), (513, 129, 4)]
if len(sys.argv) > 3:
    a = list(map(int, sys.argv[1:]))
    cases = [tuple(a[i:i + 3]) for i in range(0, len(a), 3)]
barrier = D.gene_barrier_of_circle_pillar()
for n, nt, L in cases:
    rho0, rho1 = D.get_example_2d("example1", n, n)
    rho0, rho1, _ = D.ensure_barrier_validity(rho0, rho1, barrier)
    weight = D.get_space_weight_by_barrier(n, n, barrier)
    out = None                                    # the previous case's output arrays are freed outside the timed call
    t = time.perf_counter()
    out, timeML, histML, hist = D.solver_wdotsocp2d(rho0, rho1, nt, L, dict(tol=1e-3, weight=weight, maxit=10000),
                                                    "inPALM", barrier)
    dt = time.perf_counter() - t
    its = [int(x["Iters"]) for x in timeML[:-1]]
    secs = [round(float(x["Total_Time"]), 2) for x in timeML[:-1]]
    print(f"{n}x{n}x{nt}, {L} levels: iterations {its}, loop seconds {secs}, wall {dt:.2f} s, "
          f"KKT(1,3,6) {hist['kkt'][-1][[0, 2, 5]].max():.2e}, mass ok {D.check_massConservation(out['rho'], 1e-2)}",
          flush=True)
