#!/usr/bin/env python3
"""Generates tests/golden/*.npz.

Operators (operators.npz, ref_operators.npz): the expected outputs come from the reference's prebuilt MEX
binaries only, run through oracle/ref_mex.py (oracle/_ref/, filled by oracle.ref_mex.build_ref() from a
reference checkout); without them this script refuses to run.  Trajectories (traj_*.npz): the reference's
MATLAB loops cannot run here, so they come from the CPU oracle (oracle/), whose operators are pinned to the
binaries by the above.  The GPU path is compared with all of them at the boundary (tests/test_golden.py,
tests/test_gpu_operators.py, tests/test_gpu_mex_gateways.py).  Re-run:  python tests/golden/make_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import driver as OD, mexops, ref_mex as R       # noqa: E402
from oracle.examples import (ensure_barrier_validity, gene_barrier_of_circle_pillar, get_example_1d,  # noqa: E402
                             get_example_2d, get_weight_by_barrier)
from oracle.inpalm import InPALMState                         # noqa: E402


def operators():
    rng = np.random.default_rng(20260104)
    out = {}
    x = rng.standard_normal((40, 10)) * rng.choice([0.1, 1.0, 20.0], size=(40, 1))
    x[0] = 0.0                       # 0/0 -> NaN row
    x[1] = 0.0; x[1, 0] = 2.5        # n = 0, x1 > 0 -> unchanged
    x[2] = 0.0; x[2, 0] = -2.5       # n = 0, x1 < 0 -> zero row
    x[3, 1:] = 0.0; x[3, 1] = abs(x[3, 0])            # on the cone boundary
    x = np.asfortranarray(x)
    p = np.empty_like(x, order="F")
    R.mexProjSoc(p, x)
    out["proj_in"], out["proj_out"] = x, p
    x6 = np.asfortranarray(rng.standard_normal((17, 6)))
    p6 = np.empty_like(x6, order="F")
    R.mexProjSoc(p6, x6)
    out["proj6_in"], out["proj6_out"] = x6, p6
    nt, nx, ny = 4, 6, 5
    Nz = ny * nx * (nt - 1)
    Nq = Nz + ny * (nx - 1) * nt + (ny - 1) * nx * nt
    q = rng.standard_normal(Nq)
    z = np.zeros((Nz, 10), order="F")
    R.mexBFd(z, q, nt, nx, ny, 0.731, 1.37)
    w = np.asfortranarray(rng.standard_normal((Nz, 10)))
    qa = np.zeros(Nq)
    R.mexBFdConj(qa, w, nt, nx, ny, 0.731)
    out.update(bfd_dims=np.array([nt, nx, ny]), bfd_q=q, bfd_z=z, bfdc_w=w, bfdc_q=qa,
               bfd_scale=np.array([0.731, 1.37]))
    nt1, nx1 = 5, 9
    Nz1 = nx1 * (nt1 - 1)
    q1 = rng.standard_normal(Nz1 + (nx1 - 1) * nt1)
    z1 = np.zeros((Nz1, 6), order="F")
    R.mexBFd1d(z1, q1, nt1, nx1, 1.21, 0.6)
    w1 = np.asfortranarray(rng.standard_normal((Nz1, 6)))
    qa1 = np.zeros_like(q1)
    R.mexBFdConj1d(qa1, w1, nt1, nx1, 1.21)
    out.update(bfd1_dims=np.array([nt1, nx1]), bfd1_q=q1, bfd1_z=z1, bfdc1_w=w1, bfdc1_q=qa1,
               bfd1_scale=np.array([1.21, 0.6]))
    np.savez_compressed(os.path.join(HERE, "operators.npz"), **out)


SENTINEL = -7.25           # unwritten slots of z / q keep it
ERR_BINARIES = ("mexBFd1d", "mexBFdConj1d")


def _proj_rows(rng, K):
    """Rows scaled from 1e-3 to 30, rows next to the apex (x1 = -(1 - d) ||x_2..K||, c tiny) and edge rows."""
    x = rng.standard_normal((120, K)) * np.geomspace(1e-3, 30.0, 120)[:, None]
    xb = rng.standard_normal((40, K - 1)) * np.geomspace(1e-2, 10.0, 40)[:, None]
    apex = np.column_stack([-np.sqrt((xb * xb).sum(1)) * (1.0 - np.geomspace(1e-16, 1e-5, 40)), xb])
    e = np.zeros((12, K))
    e[1, 0] = 2.5                                # x1 > 0, xbar = 0: unchanged
    e[2, 0] = -2.5                               # x1 < 0, xbar = 0: zero row
    e[3, 1:] = rng.standard_normal(K - 1)
    e[4, 1:] = e[3, 1:]
    e[3, 0] = np.sqrt((e[3, 1:] ** 2).sum())     # x1 = ||xbar||
    e[4, 0] = -e[3, 0]                           # x1 = -||xbar||
    e[5] = 1e-200                                # squares underflow
    e[6] = 1e150                                 # squares overflow
    e[7, 0] = np.inf
    e[7, 1:] = 1.0
    e[8, 0] = -np.inf
    e[8, 1:] = 1.0
    e[9, 0] = 1.0
    e[9, K - 1] = np.inf
    e[10, 0] = np.nan
    e[10, 1:] = 1.0
    e[11, :] = 1.0
    e[11, K - 1] = np.nan                        # row 0 stays the all-zero row (0/0)
    return np.asfortranarray(np.vstack([x, apex, e]))


def _reset_1d_statics():
    """The 1-D binaries keep scale and dF in static variables: an argument left out takes the value of the last
    call that passed it (1.0 before any).  Set both to 1.0 so that the calls below record the documented defaults."""
    z, q = np.zeros((1, 6), order="F"), np.zeros(1)
    R.mexBFd1d(z, q, 2, 1, 1.0, 1.0)
    R.mexBFdConj1d(q, z, 2, 1, 1.0)


def ref_operators():
    """tests/golden/ref_operators.npz: inputs and the outputs the reference binaries give for them."""
    rng = np.random.default_rng(20261016)
    out = {}
    for K in (2, 3, 6, 10, 13):
        x = _proj_rows(rng, K)
        p = np.full_like(x, SENTINEL, order="F")
        R.mexProjSoc(p, x)
        out["proj%d_in" % K], out["proj%d_out" % K] = x, p
    # 2-D: dimensions as non-integer doubles (truncated), s != 1, dF not in {0, 1}; all 7 / 6 arguments (the binaries
    # read every slot whatever nrhs is)
    for c, (nt, nx, ny) in enumerate([(2, 1, 1), (2, 2, 2), (2, 1, 5), (3, 4, 1), (4, 6, 5), (3, 5, 7)]):
        Nz = ny * nx * (nt - 1)
        Nq = Nz + ny * (nx - 1) * nt + (ny - 1) * nx * nt
        dims = np.array([nt + 0.75, nx + 0.5, ny + 0.25])
        sdF = np.array([0.731 + 0.1 * c, 1.37 - 0.2 * c])
        q = rng.standard_normal(Nq)
        z = np.full((Nz, 10), SENTINEL, order="F")
        R.mexBFd(z, q, *dims, *sdF)
        w = np.asfortranarray(rng.standard_normal((Nz, 10)))
        qa = np.full(Nq, SENTINEL)
        R.mexBFdConj(qa, w, *dims, sdF[0])
        out.update({"bfd%d_dims" % c: dims, "bfd%d_sdF" % c: sdF, "bfd%d_q" % c: q, "bfd%d_z" % c: z,
                    "bfdc%d_w" % c: w, "bfdc%d_q" % c: qa})
    # 1-D: every argument count (4, 5, 6 for mexBFd1d; 4, 5 for mexBFdConj1d)
    for c, (nt, nx) in enumerate([(2, 1), (2, 2), (5, 1), (3, 7), (4, 9)]):
        Nz, Nq = nx * (nt - 1), nx * (nt - 1) + (nx - 1) * nt
        dims = np.array([nt + 0.5, nx + 0.75])
        sdF = np.array([1.21 - 0.15 * c, 0.6 + 0.3 * c])[:[0, 1, 2, 2, 1][c]]
        q = rng.standard_normal(Nq)
        _reset_1d_statics()
        z = np.full((Nz, 6), SENTINEL, order="F")
        R.mexBFd1d(z, q, *dims, *sdF)
        w = np.asfortranarray(rng.standard_normal((Nz, 6)))
        qa = np.full(Nq, SENTINEL)
        R.mexBFdConj1d(qa, w, *dims, *sdF[:1])
        out.update({"bfd1d%d_dims" % c: dims, "bfd1d%d_sdF" % c: sdF, "bfd1d%d_q" % c: q, "bfd1d%d_z" % c: z,
                    "bfdc1d%d_w" % c: w, "bfdc1d%d_q" % c: qa})
    # error identifiers of the 1-D binaries.  Row: binary (index into ERR_BINARIES), nrhs, nlhs, position of a
    # non-scalar argument (-1: none); arguments = the first nrhs of (out, in, nt, nx, s, dF) of a 3 x 4 grid.
    cases = [(0, 3, 0, -1), (0, 0, 0, -1), (0, 4, 1, -1), (0, 5, 0, 4), (0, 6, 0, 5), (0, 6, 0, 4),
             (1, 3, 0, -1), (1, 2, 0, -1), (1, 5, 1, -1), (1, 5, 0, 4)]
    ids = []
    for b, nrhs, nlhs, bad in cases:
        args = err_case_args(b, nrhs, bad)
        ids.append(R.call(ERR_BINARIES[b], args, nlhs=nlhs) or "")
    out["err1d_case"] = np.array(cases, dtype=np.int64)
    out["err1d_id"] = np.array(ids)
    np.savez_compressed(os.path.join(HERE, "ref_operators.npz"), **out)


def err_case_args(b, nrhs, bad):
    """Arguments of one error case (kept in step with tests/test_ref_operators.py)."""
    nt, nx = 3, 4
    Nz, Nq = nx * (nt - 1), nx * (nt - 1) + (nx - 1) * nt
    z, q = np.zeros((Nz, 6), order="F"), np.zeros(Nq)
    full = [z, q, nt, nx, 0.5, 0.25] if b == 0 else [q, z, nt, nx, 0.5]
    args = full[:nrhs]
    if bad >= 0:
        args[bad] = np.ones(2)
    return args


def trajectory(name, rho0, rho1, nt, K, weight=None, method="inPALM", **extra_opts):
    var, model, o = OD.make_level(rho0, rho1, nt, dict(tol=0.0, maxit=K, **extra_opts), method, weight)
    st = OD.make_state(var, o, model, method, weighted=weight is not None)
    st.run()
    hist, sigma = st.finish()
    extra = {} if weight is None else {"weight": weight}
    np.savez_compressed(os.path.join(HERE, name + ".npz"), rho0=rho0, rho1=rho1, nt=nt, K=K,
                        phi=var.phi, q=var.q, alpha=var.alpha, z=var.z, beta=var.beta, sigma=sigma,
                        kkt=hist["kkt"], iters=hist["iter"], pdGap=hist["pdGap"], cScale=var.cScale,
                        dScale=var.dScale, method=method, **{"opt_" + k: v for k, v in extra_opts.items()}, **extra)


if __name__ == "__main__":
    if not R.available():
        sys.exit("make_golden.py: oracle/_ref/ is incomplete; run oracle.ref_mex.build_ref() with a reference checkout")
    mexops.build()
    operators()
    ref_operators()
    r0, r1 = get_example_2d("example1", 17, 17)
    trajectory("traj_dot2d_17x17x9", r0, r1, 9, 40)
    r0, r1 = get_example_2d("example1", 16, 12)
    trajectory("traj_dot2d_alg2_16x12x8", r0, r1, 8, 25, method="ALG2")
    r0, r1 = get_example_1d("gaussian", 33)
    trajectory("traj_dot1d_33x17", r0, r1, 17, 40)
    r0, r1 = get_example_2d("example1", 16, 16)
    b = gene_barrier_of_circle_pillar()
    w = get_weight_by_barrier(16, 16, 8, b)
    r0, r1, _ = ensure_barrier_validity(r0, r1, b)
    trajectory("traj_wdot2d_16x16x8", r0, r1, 8, 30, weight=w)
    # loop variants
    r0, r1 = get_example_2d("example1", 16, 12)
    trajectory("traj_palm_16x12x8", r0, r1, 8, 25, method="PALM")
    trajectory("traj_accadmm_16x12x8", r0, r1, 8, 30, method="acc-ADMM", restart=7)
    trajectory("traj_accadmm_theta3_16x12x8", r0, r1, 8, 20, method="acc-ADMM", theta=3.0, restart=6)
    r0, r1 = get_example_2d("example1", 16, 16)
    r0, r1, _ = ensure_barrier_validity(r0, r1, b)
    trajectory("traj_waccadmm_16x16x8", r0, r1, 8, 25, weight=w, method="acc-ADMM")
    print("golden vectors written to", HERE)
