#!/usr/bin/env python3
"""How far is a finished solve from the quantity that was asked for?  Example 5.1 (Gaussian -> Gaussian, 129 x 129 x 33,
3 levels, inPALM) through the multilevel driver at three tolerances, with the dual lower bound on W2^2 (dual= of the
drivers; dot-socp_amd/dual.py) beside the Eulerian `cost` of the solution report.  The bound is certified -- for the
discrete static transport cost between the node histograms, which differs from the continuous W2^2 by O(h) -- whatever
state the solve stopped in; `cost` and the raw dual 2 (sum phi1 rho1 - sum phi0 rho0) are not: they live inside the
discretised dynamic problem and converge to its optimum, from either side."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402

nt, nx, levelN = 2 ** 5 + 1, 2 ** 7 + 1, 3
rho0, rho1 = D.get_example_2d("example1", nx, nx)
print(f"Example 5.1, {nx} x {nx} x {nt}, {levelN} levels, inPALM")
print(f"{'tol':>8} {'iters':>6} {'cost':>12} {'bound':>12} {'bound_fwd':>12} {'bound_bwd':>12} {'dual_raw':>12} {'cost - bound':>13}")
for tol in (1e-3, 1e-4, 1e-5):
    output, timeML, runHistML, runHist = D.solver_dotsocp2d(rho0, rho1, nt, levelN, dict(tol=tol, maxit=3000), "inPALM",
                                                            report=True, dual=True)
    d, cost = output["dual"], output["report"]["cost"]
    print(f"{tol:8.0e} {int(runHistML['iter'][-1]):6d} {cost:12.8f} {d['bound']:12.8f} {d['bound_fwd']:12.8f} {d['bound_bwd']:12.8f} "
          f"{d['dual_raw']:12.8f} {cost - d['bound']:+13.3e}")
print(str(d))
