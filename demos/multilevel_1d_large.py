#!/usr/bin/env python3
"""A 1-D multilevel solve beyond 1025 points per axis: Gaussian -> Gaussian at 65537 x 257 in five levels (4097 x 17,
8193 x 33, 16385 x 65, 32769 x 129, 65537 x 257), inPALM.  None of these lengths has small coprime factors, so every level's
Poisson solve runs Bluestein's DCT with the two-level convolution of csrc/cdft_long.hip; DOTSOCP_CDFT_LONG_MIN=1026 is set
here (unless the caller has set it) so that the coarsest level, 4097 points, takes it too instead of a dense plan of
three 4097 x 4097 matrices.  Prints iterations and seconds per level.  usage: multilevel_1d_large.py [n nt levelN [tol]]"""
import os
import sys
import time

os.environ.setdefault("DOTSOCP_CDFT_LONG_MIN", "1026")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402

n, nt, L = (int(v) for v in (sys.argv[1:4] + ["65537", "257", "5"][len(sys.argv) - 1:]))
tol = float(sys.argv[4]) if len(sys.argv) > 4 else 1e-3
rho0, rho1 = D.get_example_1d("gaussian", n)
t = time.perf_counter()
out, timeML, histML, hist = D.solver_dotsocp1d(rho0, rho1, nt, L, dict(tol=tol, maxit=3000), "inPALM")
dt = time.perf_counter() - t
sizes = [((n - 1) >> (L - 1 - i)) + 1 for i in range(L)]
print(f"{n} x {nt}, {L} levels, tol {tol:g}: cdft_levels {[D.cdft_levels(m) for m in sizes]}")
for m, x in zip(sizes, timeML[:-1]):
    print(f"  level {m:6d} points: {int(x['Iters']):5d} iterations, {float(x['Total_Time']):7.2f} s", flush=True)
print(f"wall {dt:.2f} s, KKT(1,3,6,7) {hist['kkt'][-1][[0, 2, 5, 6]].max():.2e}, "
      f"mass ok {D.check_massConservation(out['rho'], 1e-2)}")
