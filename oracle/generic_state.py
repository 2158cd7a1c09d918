"""One generic start for the loops: phi, q, z, alpha, beta with no vanishing term and all three
branches of the cone projection populated.

TEST INFRASTRUCTURE (see oracle/__init__.py).  The all-zero state of initialize.m is special: on an
`example1` trajectory started from it the polar branch of mexProjSoc (||x_bar|| <= -x_1, result 0) is
never taken and KKT column 5 stays at rounding noise.  The recipe here is the one of the random-state
tests (tests/test_gpu_solver.py::test_iterations_from_a_random_state) with one addition: each cone row
is drawn into one of three classes, and its first multiplier entry is pushed by +SHIFT (the row's
argument z2 - beta then lies in the polar cone), by -SHIFT (inside the cone) or left alone (mostly on
the surface branch).  tests/test_generic_state_conditions.py asserts, with the oracle alone, that the
free-running loops started here do visit every branch and keep every KKT column away from zero.
"""
import numpy as np

from . import mexops

FIELDS = ("phi", "q", "z", "alpha", "beta")
AMPLITUDES = {"phi": 1.0, "q": 0.3, "z": 0.6, "alpha": 0.5, "beta": 0.4}
SHIFT = 3.0
DEFAULT_SEED = 2357


def cone_holes(var, dims):
    """Boolean mask of the slots of z / beta that mexBFd (2-D: dims = (ny, nx, nt)) or mexBFd1d
    (dims = (nx, nt)) leaves unwritten: cone rows at the domain boundary have no edge there."""
    probe = np.full(np.shape(var.beta), np.nan, order="F")
    q = np.zeros(np.size(var.q))
    if len(dims) == 2:
        nx, nt = dims
        mexops.mexBFd1d(probe, q, nt, nx)
    else:
        ny, nx, nt = dims
        mexops.mexBFd(probe, q, nt, nx, ny)
    hole = np.isnan(probe)
    assert 0 < hole.sum() < probe.size // 4
    return hole


def generic_state(var, dims, seed=DEFAULT_SEED, amplitudes=None, shift=SHIFT):
    """The start as a dict of new arrays shaped like the fields of `var` (a level after InitialScaling).

    N(0,1) times the amplitude of each field; the row classes 0 / 1 / 2 with equal probability
    (1: beta[row, 0] += shift, 2: beta[row, 0] -= shift); z and beta zero in the slots mexBFd leaves
    unwritten -- the reference never makes them non-zero, and its KKT block reads what an earlier
    projection left in such slots of a shared temporary (tests/test_gpu_solver.py gives the lines)."""
    amp = dict(AMPLITUDES, **(amplitudes or {}))
    rng = np.random.default_rng(seed)
    start = {}
    for f in ("phi", "q", "alpha", "z", "beta"):
        shape = np.shape(getattr(var, f))
        start[f] = np.asfortranarray(amp[f] * rng.standard_normal(shape))
    rows = start["beta"].shape[0]
    cls = rng.integers(0, 3, size=rows)
    start["beta"][cls == 1, 0] += shift
    start["beta"][cls == 2, 0] -= shift
    hole = cone_holes(var, dims)
    start["z"][hole] = 0.0
    start["beta"][hole] = 0.0
    return start


def perturbed(start, seed=1, eps=2.0 ** -52):
    """Every entry times (1 + eps N(0,1)): the one-ulp perturbation the sensitivity check uses (zeros stay zero)."""
    rng = np.random.default_rng(seed)
    return {f: np.asfortranarray(a * (1.0 + eps * rng.standard_normal(a.shape))) for f, a in start.items()}


def set_state(var, start):
    """Copies of the start into the fields of `var` (an oracle level or a device-side one alike)."""
    for f in FIELDS:
        setattr(var, f, start[f].copy(order="F"))


# --------------------------------------------------------------------------------------------------
# The cases the generic-start tests run (tests/test_generic_state_conditions.py on the CPU asserts for each that the
# start does its job; tests/test_gpu_generic_state.py, tests/test_gpu_generic_accadmm.py and tests/test_gpu_generic_palm.py
# compare the device loops with the same oracle runs).
# shape: (ny, nx, nt), or (nx, nt) for the 1-D problem.  Every entry may carry seed / amplitudes / shift of its own, and
# solver options (restart, rho, theta, ifCheckStepByStep) under `opts`.
# --------------------------------------------------------------------------------------------------
CASES = {
    "inPALM-130x9x7": dict(method="inPALM", shape=(130, 9, 7), K=12),
    "inPALM-66x10x6": dict(method="inPALM", shape=(66, 10, 6), K=25),
    "inPALM-100x70x20": dict(method="inPALM", shape=(100, 70, 20), K=25),
    "inPALM-1d-150x7": dict(method="inPALM", shape=(150, 7), K=12),
    # The cases below miss a condition with the plain recipe (the polar rows die out within three iterations), so each
    # has amplitudes of its own; the thresholds of tests/test_generic_state_conditions.py are the same for all.
    # 13 layers: a wider class offset and a larger alpha keep polar rows alive through iterations 3..7
    "inPALM-40x12x13": dict(method="inPALM", shape=(40, 12, 13), K=12, shift=20.0, amplitudes=dict(alpha=2.5)),        # the time-slab grid
    # ny * nx = 4096 and ny % 16 == 0: unpitched rows and cone columns Nz + 48 apart on the device; the coarse level of the
    # padded transfer case (oracle/transfer_state.py)
    # (the inside rows nearly die out in iteration 2 on so few layers: the wide offset, and a small beta next to it)
    "inPALM-128x32x5": dict(method="inPALM", shape=(128, 32, 5), K=7, shift=20.0, amplitudes=dict(alpha=2.5, beta=0.1)),
    # 1e6 weights: with q of the plain size KKT column 5 moves by 3e-12 relative under one-ulp perturbations (w q
    # cancels against A phi in the alpha update); a smaller q brings that to 1e-13.  Past iteration 12 column 4 falls
    # to 1e-3.
    "inPALM-weighted-66x10x6": dict(method="inPALM", shape=(66, 10, 6), K=12, weighted=True, shift=20.0,
                                    amplitudes=dict(alpha=2.5, q=0.03)),
    # tau = 1: -beta lands in the cone after every multiplier step, so polar rows survive only behind a wide offset
    "ALG2-66x10x6": dict(method="ALG2", shape=(66, 10, 6), K=12, shift=20.0),
    # PALM and acc-ADMM recompute q from A phi before their first projection: a phi of size 1 makes q of size 30 and
    # every row a surface row; PALM's polar rows are gone after iteration 7
    "PALM-66x10x6": dict(method="PALM", shape=(66, 10, 6), K=7, shift=20.0, amplitudes=dict(phi=0.02, beta=0.1)),
    "acc-ADMM-66x10x6": dict(method="acc-ADMM", shape=(66, 10, 6), K=12, shift=20.0, amplitudes=dict(phi=0.02)),
    # --- acc-ADMM on every path of its device loop.  `opts` are solver options of the case (case_opts merges them).
    # The tile-crossing grids of the inPALM cases; on 100 x 70 x 20 the polar rows are gone by iteration 17 whatever the
    # amplitudes: K = 13
    # (130 x 9 x 7 with phi = 0.02 changes sigma at every check; a smaller phi and beta bring the residual ratio of the check
    # at iteration 1 to 1.02, inside the band (1/1.1, 1.1) that leaves sigma alone)
    "acc-ADMM-130x9x7": dict(method="acc-ADMM", shape=(130, 9, 7), K=12, shift=20.0,
                             amplitudes=dict(phi=0.002, beta=0.1)),
    "acc-ADMM-100x70x20": dict(method="acc-ADMM", shape=(100, 70, 20), K=13, shift=40.0,
                               amplitudes=dict(phi=0.02, alpha=2.5, z=2.0)),
    # a restart by count fires between checks only with restart <= 3: sigma changes at almost every check, which resets k
    # every three iterations
    "acc-ADMM-restart2-66x10x6": dict(method="acc-ADMM", shape=(66, 10, 6), K=12, shift=20.0, amplitudes=dict(phi=0.02),
                                      opts=dict(restart=2, rho=1.7)),
    # theta != 2: the extrapolation with its hatOld carry, no Halpern anchors
    "acc-ADMM-theta3-66x10x6": dict(method="acc-ADMM", shape=(66, 10, 6), K=12, shift=20.0, amplitudes=dict(phi=0.02),
                                    opts=dict(theta=3.0, restart=3)),
    "acc-ADMM-theta3-130x9x7": dict(method="acc-ADMM", shape=(130, 9, 7), K=12, shift=20.0,
                                    amplitudes=dict(phi=0.002, beta=0.1), opts=dict(theta=3.0, restart=3)),
    "acc-ADMM-theta5-66x10x6": dict(method="acc-ADMM", shape=(66, 10, 6), K=12, shift=20.0, amplitudes=dict(phi=0.02),
                                    opts=dict(theta=5.0, restart=8)),
    # a KKT check in every iteration
    "acc-ADMM-checkstep-66x10x6": dict(method="acc-ADMM", shape=(66, 10, 6), K=8, shift=20.0, amplitudes=dict(phi=0.02),
                                       opts=dict(ifCheckStepByStep=True)),
    "acc-ADMM-checkstep-theta3-66x10x6": dict(method="acc-ADMM", shape=(66, 10, 6), K=8, shift=20.0,
                                              amplitudes=dict(phi=0.02),
                                              opts=dict(ifCheckStepByStep=True, theta=3.0, restart=3)),
    # 1e6 barrier weights
    "acc-ADMM-weighted-66x10x6": dict(method="acc-ADMM", shape=(66, 10, 6), K=12, weighted=True, shift=20.0,
                                      amplitudes=dict(phi=0.02)),
    "acc-ADMM-weighted-130x9x7": dict(method="acc-ADMM", shape=(130, 9, 7), K=12, weighted=True, shift=20.0,
                                      amplitudes=dict(phi=0.02, alpha=2.5)),
    "acc-ADMM-weighted-theta3-66x10x6": dict(method="acc-ADMM", shape=(66, 10, 6), K=12, weighted=True, shift=20.0,
                                             amplitudes=dict(phi=0.02), opts=dict(theta=3.0, restart=3)),
    # the time-slab grid.  The inside branch of iteration 2 is the bottleneck of the Halpern cases: at rho = 2 it gets a
    # share of 0.0014 here, at rho = 1.5 (a regular option of the loop) 0.0052
    "acc-ADMM-40x12x13": dict(method="acc-ADMM", shape=(40, 12, 13), K=12, shift=20.0, amplitudes=dict(phi=0.02),
                              opts=dict(rho=1.5)),
    "acc-ADMM-theta3-40x12x13": dict(method="acc-ADMM", shape=(40, 12, 13), K=12, shift=20.0, amplitudes=dict(phi=0.02),
                                     opts=dict(theta=3.0, restart=3)),
    "acc-ADMM-weighted-40x12x13": dict(method="acc-ADMM", shape=(40, 12, 13), K=12, weighted=True, shift=20.0,
                                       amplitudes=dict(phi=0.02, alpha=2.5)),
    "acc-ADMM-checkstep-40x12x13": dict(method="acc-ADMM", shape=(40, 12, 13), K=8, shift=20.0, amplitudes=dict(phi=0.02),
                                        opts=dict(ifCheckStepByStep=True, rho=1.5)),
    "PALM-40x12x13": dict(method="PALM", shape=(40, 12, 13), K=7, shift=20.0, amplitudes=dict(phi=0.02, beta=0.1)),
    # --- PALM on the tile-crossing grids and with a check in every iteration (tests/test_gpu_generic_palm.py).  The polar
    # rows are gone after iteration 7 on every grid: K <= 7, checks at 1, 4, 7.
    # 130 x 9 x 7 with phi = 0.02 leaves the inside branch a share of 0.0016 (alpha = 2.5, beta = 0.4 and phi = 0.05 make it
    # smaller); phi = 0.01 gives 0.0037
    "PALM-130x9x7": dict(method="PALM", shape=(130, 9, 7), K=7, shift=20.0, amplitudes=dict(phi=0.01, beta=0.1)),
    "PALM-100x70x20": dict(method="PALM", shape=(100, 70, 20), K=7, shift=20.0, amplitudes=dict(phi=0.02, beta=0.1)),
    "PALM-checkstep-66x10x6": dict(method="PALM", shape=(66, 10, 6), K=6, shift=20.0, amplitudes=dict(phi=0.02, beta=0.1),
                                   opts=dict(ifCheckStepByStep=True)),
}

# KKT column 5 (index 4), sigma ||F*B*beta + D_w alpha||, is zero in exact arithmetic for the loops whose multiplier step
# has length 1 (ALG2: tau = 1, acc-ADMM): there the q-step's optimality condition diagQ q = A phi + alpha + F*B*(z + beta)
# and diagQ = I + F*B*BF give F*B*beta^+ + alpha^+ = 0 identically, whatever the data.  No start makes it generic; it is
# rounding noise (1e-16) that moves by O(1) relative under a one-ulp perturbation, and is held to an absolute bound instead.
# (Under 1e6 weights acc-ADMM leaves 1e-11 .. 3e-11 there, mostly systematic: a bound of its own,
# tests/test_generic_state_conditions.py: NOISE_WEIGHTED.)
CANCELLING_COLUMNS = {"ALG2": (4,), "acc-ADMM": (4,)}


def problem(case):
    """(rho0, rho1, nt, weight) of a case: `example1` / the 1-D Gaussians, the circle-pillar barrier when weighted."""
    from .examples import (ensure_barrier_validity, gene_barrier_of_circle_pillar, get_example_1d, get_example_2d,
                           get_weight_by_barrier)
    spec = CASES[case]
    shape = spec["shape"]
    if len(shape) == 2:
        rho0, rho1 = get_example_1d("gaussian", shape[0])
        return rho0, rho1, shape[1], None
    ny, nx, nt = shape
    rho0, rho1 = get_example_2d("example1", ny, nx)          # arrays of shape (ny, nx)
    weight = None
    if spec.get("weighted"):
        barrier = gene_barrier_of_circle_pillar()
        weight = get_weight_by_barrier(nx, ny, nt, barrier)
        rho0, rho1, _ = ensure_barrier_validity(rho0, rho1, barrier)
    return rho0, rho1, nt, weight


def case_opts(case):
    """tol = 0 and maxit = K, with the case's own solver options (restart, rho, theta, ifCheckStepByStep) over them."""
    return dict(dict(tol=0.0, maxit=CASES[case]["K"]), **CASES[case].get("opts", {}))


def case_start(case, var):
    spec = CASES[case]
    return generic_state(var, spec["shape"], seed=spec.get("seed", DEFAULT_SEED), amplitudes=spec.get("amplitudes"),
                         shift=spec.get("shift", SHIFT))


def branch_shares(inp):
    """Share of the rows of a mexProjSoc argument in each branch (oracle/mex_kernels.c: oracle_proj_soc):
    (polar: result 0, inside: the row itself, surface: the scaled row)."""
    n = np.sqrt(np.sum(inp[:, 1:] ** 2, axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (inp[:, 0] / n + 1.0) * 0.5
    polar, inside = np.mean(c <= 0.0), np.mean(c >= 1.0)
    return polar, inside, 1.0 - polar - inside


_runs = {}


def oracle_run(case, perturb=False):
    """The oracle's free-running loop of a case from its generic start, computed once per process and shared (treat
    the result as read-only).  Returns a dict: var (the finished level), start, hist, sigma, shares (one
    (polar, inside, surface) triple per z-step projection, the projection inside the KKT block not counted),
    weight, and the level's opts; for acc-ADMM and PALM also sigma_updates ((iteration, factor) of every check that
    changed sigma), for acc-ADMM restarts (the iterations whose extrapolation ended with the count back at 0) and
    interps ((iteration, k) of every extrapolation, k the count it ran with)."""
    key = (case, bool(perturb))
    if key in _runs:
        return _runs[key]
    from . import driver as OD
    spec = CASES[case]
    rho0, rho1, nt, weight = problem(case)
    var, model, o = OD.make_level(rho0, rho1, nt, case_opts(case), spec["method"], weight)
    start = case_start(case, var)
    if perturb:
        start = perturbed(start)
    set_state(var, start)
    st = OD.make_state(var, o, model, spec["method"], weighted=weight is not None)
    shares = []
    plain = mexops.mexProjSoc

    def counting(out, inp):
        if out is st.z:                      # the z-step; the KKT block projects into the temporary z2
            shares.append(branch_shares(inp))
        plain(out, inp)

    # acc-ADMM and PALM: the iterations at which a check changed sigma (with the factor); acc-ADMM: those at which the
    # extrapolation count returned to 0 inside _interpolate (a restart by count, as opposed to the reset a sigma update makes)
    sigma_updates, restarts, interps = [], [], []
    if hasattr(st, "_interpolate") or spec["method"] == "PALM":
        apply_factor = st._apply_sigma_factor

        def recording_factor(factor):
            sigma_updates.append((st.it, float(factor)))
            apply_factor(factor)

        st._apply_sigma_factor = recording_factor
    if hasattr(st, "_interpolate"):
        interpolate = st._interpolate

        def recording_interpolate():
            k = st.k
            interpolate()
            interps.append((st.it, k))
            if st.k == 0:
                restarts.append(st.it)

        st._interpolate = recording_interpolate

    mexops.mexProjSoc = counting
    try:
        st.run()
    finally:
        mexops.mexProjSoc = plain
    hist, sigma = st.finish()
    for f in FIELDS:
        getattr(var, f).flags.writeable = False
    _runs[key] = dict(var=var, start=start, hist=hist, sigma=sigma, shares=np.array(shares), weight=weight, opts=o,
                      sigma_updates=sigma_updates, restarts=restarts, interps=interps)
    return _runs[key]
