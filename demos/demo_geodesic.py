#!/usr/bin/env python3
"""Is the solved flow a geodesic, or merely a curve that joins rho0 to rho1?  The profile per time node (geodesic= of the
drivers; dot-socp_amd/geodesic.py), formed on the device in one pass over the resident alpha:

  * the kinetic energy of every time layer next to the certified bracket  bound <= W2^2 <= upper  (dual=, upper= of the
    drivers): on an exact geodesic every layer's energy equals W2^2 (constant speed), so the profile sits inside the
    bracket layer by layer;
  * the centre of mass, which moves on a straight line at constant momentum;
  * the second moment about the origin, a parabola in t;
  * the entropy, convex in t (displacement convexity);
  * and, in the summary line, how far the solution is from each of these.

Example 5.1 (Gaussian -> Gaussian, 129 x 129 x 33, 3 levels, inPALM) at two tolerances."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402

UPPER = dict(eps_h2=0.25, max_sweeps=200, defect_tol=0.0)
nt, nx, levelN = 2 ** 5 + 1, 2 ** 7 + 1, 3
rho0, rho1 = D.get_example_2d("example1", nx, nx)
print(f"Example 5.1, {nx} x {nx} x {nt}, {levelN} levels, inPALM")
for tol in (1e-3, 1e-5):
    output, timeML, runHistML, runHist = D.solver_dotsocp2d(rho0, rho1, nt, levelN, dict(tol=tol, maxit=3000), "inPALM",
                                                            geodesic=True, dual=True, upper=UPPER)
    g, lo, hi = output["geodesic"], output["dual"]["bound"], output["upper"]["upper"]
    print(f"tol {tol:.0e}, {int(runHistML['iter'][-1])} iterations; certified bracket {lo:.8f} <= W2^2 <= {hi:.8f}")
    print(g.table(bracket=(lo, hi)))
    print(g.summary())
