#!/usr/bin/env python3
"""How far is a finished solve from the quantity that was asked for?  A bracket  bound <= W2^2(a, b) <= upper  around the
discrete static transport cost between the node histograms, both ends certified whatever state the solve stopped in:
the dual lower bound from the Hopf-Lax transform of the potential (dual= of the drivers; dot-socp_amd/dual.py) and the
upper bound from Sinkhorn sweeps started at the potential and rounded to a feasible plan (upper= of the drivers;
dot-socp_amd/upper.py).  The Eulerian `cost` of the solution report and the raw dual 2 (sum phi1 rho1 - sum phi0 rho0) are
not certified: they live inside the discretised dynamic problem and converge to its optimum, from either side.

First three problems small enough for the transport LP (scipy's HiGHS; skipped without scipy): the exact value lies inside
the bracket.  Then Example 5.1 (Gaussian -> Gaussian, 129 x 129 x 33, 3 levels, inPALM) at three tolerances."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402
from dotsocp_amd import upper as U  # noqa: E402

UPPER = dict(eps_h2=0.25, max_sweeps=200, defect_tol=0.0)


def exact_w2(rho0, rho1):
    """W2^2 between the node histograms: the transport LP"""
    from scipy.optimize import linprog
    from scipy.sparse import csr_matrix, eye, kron, vstack
    n = rho0.size
    a, b = rho0.ravel(order="F") / rho0.sum(), rho1.ravel(order="F") / rho1.sum()
    ones = csr_matrix(np.ones((1, n)))
    A = vstack([kron(eye(n), ones), kron(ones, eye(n))]).tocsr()[:-1]
    r = linprog(2.0 * U.pair_cost(rho0.shape).ravel(), A_eq=A, b_eq=np.concatenate([a, b])[:-1], bounds=(0, None), method="highs")
    return float(r.fun)


def asymmetric_problem():
    X, Y = np.meshgrid(np.linspace(0, 1, 17), np.linspace(0, 1, 13))
    g = lambda mx, my, sx, sy: np.exp(-((X - mx) ** 2 / 2 / sx ** 2 + (Y - my) ** 2 / 2 / sy ** 2))    # noqa: E731
    rho0 = g(.3, .35, .1, .12) + 0.05
    rho1 = g(.7, .6, .15, .08) + 0.5 * g(.4, .8, .07, .07) + 0.05
    return rho0 / rho0.mean(), rho1 / rho1.mean()


try:
    import scipy  # noqa: F401
    small = [("example1 9 x 9 x 9", D.get_example_2d("example1", 9, 9)), ("example1 17 x 17 x 9", D.get_example_2d("example1", 17, 17)),
             ("asymmetric 13 x 17 x 9", asymmetric_problem())]
except ImportError:
    small = []
    print("(no scipy: the small problems with the exact LP value are skipped)")
if small:
    print(f"{'problem':>24} {'bound':>12} {'exact (LP)':>12} {'upper':>12} {'upper / exact':>14} {'inside':>7}")
for name, (rho0, rho1) in small:
    output = D.solver_dotsocp2d(rho0, rho1, 9, 1, dict(tol=1e-4), "inPALM", dual=True, upper=UPPER)[0]
    lo, hi, exact = output["dual"]["bound"], output["upper"]["upper"], exact_w2(rho0, rho1)
    print(f"{name:>24} {lo:12.8f} {exact:12.8f} {hi:12.8f} {hi / exact:14.5f} {str(lo <= exact <= hi):>7}")

nt, nx, levelN = 2 ** 5 + 1, 2 ** 7 + 1, 3
rho0, rho1 = D.get_example_2d("example1", nx, nx)
print(f"Example 5.1, {nx} x {nx} x {nt}, {levelN} levels, inPALM; upper: eps = {UPPER['eps_h2']} h^2, {UPPER['max_sweeps']} sweeps from the potential")
print(f"{'tol':>8} {'iters':>6} {'cost':>12} {'bound':>12} {'<= W2^2 <=':>10} {'upper':>12} {'upper / bound':>14} {'dual_raw':>12} {'cost - bound':>13}")
for tol in (1e-3, 1e-4, 1e-5):
    output, timeML, runHistML, runHist = D.solver_dotsocp2d(rho0, rho1, nt, levelN, dict(tol=tol, maxit=3000), "inPALM",
                                                            report=True, dual=True, upper=UPPER)
    d, u, cost = output["dual"], output["upper"], output["report"]["cost"]
    print(f"{tol:8.0e} {int(runHistML['iter'][-1]):6d} {cost:12.8f} {d['bound']:12.8f} {'':>10} {u['upper']:12.8f} {u['upper'] / d['bound']:14.6f} "
          f"{d['dual_raw']:12.8f} {cost - d['bound']:+13.3e}")
print(str(d))
print(str(u))
