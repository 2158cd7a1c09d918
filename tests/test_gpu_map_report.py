"""The map report on the device (csrc/advect.hip: k_advect<., true>, k_map_final; dotsocp_map_report,
InPALMContext.map_report(), map_report= on the drivers) against the numpy twin advect.map_report applied to ctx.outputs()
of the SAME context: every field of the struct, the three per-particle arrays, the final positions and the clamp count bit
for bit (no contraction, a fixed summation tree: include/dotsocp.h fixes every operation), identical between two calls and
between slab splits.

States, contexts and particles are made as in tests/test_gpu_push.py (upload, begin(), no iteration, finish()): rho mostly
in [0.5, 1.5] with exact zeros and negative entries, E a smooth shear plus noise with |E / rho| up to about 0.5."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dotsocp_amd as D
from dotsocp_amd import advect as A
from dotsocp_amd import capi
from oracle.generic_state import generic_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (ny, nx, nt, weighted); 1-D: ny = None
CASES = {
    "2d_19x13x7": (19, 13, 7, False),
    "w_16x16x8": (16, 16, 8, True),
    "1d_33x9": (None, 33, 9, False),
    "2d_16x12x8": (16, 12, 8, False),
}
BLOCK = 256                                     # ADV_BLOCK of csrc/advect.hip: threads (particles) per workgroup
COUNTS = (63, BLOCK + 1)
SCALARS = ("n", "n_clamped", "n_still", "mass", "cost_map", "cost_length", "cost_action", "disp_mean", "len_mean", "disp_max",
           "len_max", "detour_max", "detour_over")
ARRAYS = ("detour_hist", "x", "y", "disp", "len", "action")


def _state(case):
    ny, nx, nt, weighted = CASES[case]
    rng = np.random.default_rng(sorted(CASES).index(case) + 1618)
    one_d = ny is None
    shape = (nx,) if one_d else (ny, nx)
    rho0, rho1 = rng.uniform(0.5, 1.5, shape), rng.uniform(0.5, 1.5, shape)
    var, model = D.initialize(rho0, rho1, nt)
    nq = var.q.size
    if weighted:
        model.weight = 0.5 + (1e6 - 0.5) * rng.uniform(0, 1, nq) ** 32       # as tests/test_gpu_report.py
    D.InitialScaling(var, model, not weighted, None, dim=1 if one_d else 2, weighted=weighted)
    my = 1 if one_d else ny
    a0 = rng.uniform(0.5, 1.5, (my, nx, nt - 1))
    for k, val in enumerate((0.0, 0.0, -0.3, -0.7)):                     # both cells around node 1 / node nt - 2
        p = rng.integers(0, my * nx)
        t = 0 if k % 2 == 0 else nt - 3
        a0[p % my, p // my, t:t + 2] = val
    gy = np.arange(my) / float(max(my - 1, 1))
    gx = np.arange(nx) / float(nx - 1)
    ends = np.ones(nt)
    ends[[0, -1]] = 0.5
    ax = (0.22 * np.sin(2 * np.pi * (gy if not one_d else 0 * gy) + 0.3)[:, None, None]
          + (0.22 * np.sin(4 * np.pi * gx[:-1] + 0.2)[None, :, None] if one_d else 0.0)
          + 0.05 * rng.uniform(-1, 1, (my, nx - 1, nt))) * ends
    ay = None
    if not one_d:
        ay = (0.22 * np.cos(2 * np.pi * gx + 0.1)[None, :, None] + 0.05 * rng.uniform(-1, 1, (ny - 1, nx, nt))) * ends
    target = np.concatenate([a.ravel(order="F") for a in (a0, ax, ay) if a is not None])
    assert target.size == nq
    var.alpha = target / (var.cScale * var.D) / (model.weight if weighted else 1.0)
    var.q = generic_state(var, (nx, nt) if one_d else (ny, nx, nt))["q"]
    return var, model, weighted


def _context(case, method="inPALM", **split):
    """A finished context on the state of `case` (no iteration)"""
    var, model, weighted = _state(case)
    opts = dict(tau=1.9, sigma=1.0, tol=0.0, maxit=1, ifCheckStepByStep=False, scaling=True)
    ctx = D.InPALMContext(var, opts, model, weighted=weighted, method=method, **split)
    ctx.finish(download=False)
    return ctx


def _particles(case, n, seed=0):
    """seeds on nodes, on cell borders, on the sides and corners of the square, outside it and anywhere (from 40 particles
    on; fewer: anywhere); masses in [0, 2) with exact zeros"""
    ny, nx, nt, _ = CASES[case]
    rng = np.random.default_rng(n + 7 * seed)
    one_d = ny is None
    gx = np.arange(nx) / float(nx - 1)
    gy = gx if one_d else np.arange(ny) / float(ny - 1)
    u = lambda k: rng.uniform(0, 1, k)                                    # noqa: E731
    xs = [rng.choice(gx, 12), rng.choice(gx, 8), u(8), np.array([0.0, 1.0, 0.0, 1.0, 1.0, -0.2, 1.5, 0.3])]
    ys = [rng.choice(gy, 12), u(8), rng.choice(gy, 8), np.array([0.0, 0.0, 1.0, 1.0, 0.5, 0.4, 0.5, 1.0])]
    x, y = np.concatenate(xs), np.concatenate(ys)
    if n >= x.size:
        x, y = np.concatenate([x, u(n - x.size)]), np.concatenate([y, u(n - y.size)])
    else:
        x, y = u(n), u(n)
    mass = rng.uniform(0.0, 2.0, n)
    if n > 8:
        mass[[3, n // 2]] = 0.0
    return x, (None if one_d else y), mass


def _strip(out):
    return {k: v for k, v in out.items() if k in ("rho", "Ex", "Ey")}


def _same(dev, twin, arrays=ARRAYS):
    """every field of the struct, the per-particle arrays and the final positions: the same bits"""
    assert set(dev) == set(twin) == set(SCALARS) | set(ARRAYS)
    for k in SCALARS:
        assert type(dev[k]) is type(twin[k]), k
        assert np.float64(dev[k]).tobytes() == np.float64(twin[k]).tobytes(), (k, dev[k], twin[k], dev[k] - twin[k])
    for k in arrays:
        if twin[k] is None:
            assert dev[k] is None, k
            continue
        d, t = np.asarray(dev[k]), np.asarray(twin[k])
        assert d.shape == t.shape and d.dtype == t.dtype, k
        if d.tobytes() != t.tobytes():
            raise AssertionError("%s differs in %d of %d entries, largest difference %.3e"
                                 % (k, np.count_nonzero(d != t), d.size, np.nanmax(np.abs(d - t))))


def _bytes(r):
    return b"".join(np.float64(r[k]).tobytes() for k in SCALARS) + \
        b"".join(np.asarray(r[k]).tobytes() for k in ARRAYS if r[k] is not None)


RUNS = [(direction, nsub, with_mass) for direction in (1, -1) for nsub in (1, 2) for with_mass in (True, False)]


def _check_context(ctx, case, counts=COUNTS):
    out = _strip(ctx.outputs())
    assert np.all(np.isfinite(out["rho"])) and np.count_nonzero(out["rho"] <= 0.0) >= 2
    raw = {}
    for n in counts:
        x, y, mass = _particles(case, n)
        for direction, nsub, with_mass in RUNS:
            kw = dict(mass=mass if with_mass else None, nsub=nsub, direction=direction, per_particle=True)
            dev = ctx.map_report(x, y, **kw)
            _same(dev, A.map_report(out, x, y, **kw))
            raw[(n, direction, nsub, with_mass)] = _bytes(dev)
            plain = ctx.advect(x, y, nsub=nsub, direction=direction)         # the trajectories are advect()'s
            assert plain["x"].tobytes() == dev["x"].tobytes() and plain["n_clamped"] == dev["n_clamped"]
            assert y is None or plain["y"].tobytes() == dev["y"].tobytes()
        again = ctx.map_report(x, y, mass=mass, nsub=2, per_particle=True)
        assert _bytes(again) == raw[(n, 1, 2, True)]                        # two calls: identical bytes
        lean = ctx.map_report(x, y, mass=mass, nsub=2)                      # without the arrays: the same report
        assert lean["disp"] is None and lean["len"] is None and lean["action"] is None
        assert all(np.float64(lean[k]).tobytes() == np.float64(again[k]).tobytes() for k in SCALARS)
        assert np.array_equal(lean["detour_hist"], again["detour_hist"])
    return raw


@pytest.mark.parametrize("case", ["2d_19x13x7", "w_16x16x8", "1d_33x9"])
def test_map_report_equals_the_twin(case):
    ctx = _context(case)
    try:
        _check_context(ctx, case)
    finally:
        ctx.close()


def test_ragged_reduction_ends():
    """one particle, full and ragged wavefronts and blocks; 4097 particles are 17 blocks, the last one with a single
    particle: the tree over the block sums has more than one level and an odd tail"""
    case = "2d_19x13x7"
    ctx = _context(case)
    try:
        out = _strip(ctx.outputs())
        for n in (1, 64, 65, 256, 257, 4097):
            x, y, mass = _particles(case, n)
            for m in (mass, None):
                dev = ctx.map_report(x, y, mass=m, nsub=1)
                twin = A.map_report(out, x, y, mass=m, nsub=1)
                _same(dev, twin)
                assert dev["n"] == n and dev["detour_hist"].sum() + dev["detour_over"] <= n
    finally:
        ctx.close()


_one_slab = {}


def _one_slab_bytes(case):
    if case not in _one_slab:
        ctx = _context(case)
        try:
            _one_slab[case] = _check_context(ctx, case, counts=(BLOCK + 1,))
        finally:
            ctx.close()
    return _one_slab[case]


@pytest.mark.parametrize("split", [dict(nslabs=2), dict(nslabs=3), dict(ngpu=3)], ids=["nslabs2", "nslabs3", "ngpu3"])
def test_time_slabs_give_the_same_bytes(split):
    case = "2d_16x12x8"
    raw = _one_slab_bytes(case)
    n = BLOCK + 1
    x, y, mass = _particles(case, n)
    ctx = _context(case, **split)
    try:
        for direction, nsub, with_mass in RUNS:
            dev = ctx.map_report(x, y, mass=mass if with_mass else None, nsub=nsub, direction=direction, per_particle=True)
            assert _bytes(dev) == raw[(n, direction, nsub, with_mass)], (direction, nsub, with_mass)
    finally:
        ctx.close()


@pytest.mark.parametrize("method", ["PALM", "acc-ADMM"])
def test_other_loops(method):
    case = "2d_19x13x7"
    ctx = _context(case, method=method)
    try:
        _check_context(ctx, case, counts=(63,))
    finally:
        ctx.close()


def _c_map(ctx, r0, r1, o, x, y, mass, rep, disp=None, length=None, action=None):
    ptr = lambda a: None if a is None else a.ctypes.data                    # noqa: E731
    rc = capi.lib().dotsocp_map_report(ctx._ctx, ptr(r0), ptr(r1), None if o is None else ctypes.byref(o), ptr(x), ptr(y),
                                       ptr(mass), None if rep is None else ctypes.byref(rep), ptr(disp), ptr(length), ptr(action))
    return rc, capi.lib().dotsocp_last_error()


def test_errors_name_the_call():
    ny, nx, nt = 9, 7, 4
    rng = np.random.default_rng(5)
    var, model = D.initialize(rng.uniform(0.5, 1.5, (ny, nx)), rng.uniform(0.5, 1.5, (ny, nx)), nt)
    D.InitialScaling(var, model, True, None, dim=2)
    ctx = D.InPALMContext(var, dict(tau=1.9, sigma=1.0, tol=0.0, maxit=1, scaling=True), model)
    n = 10
    x, y, mass = rng.uniform(0, 1, n), rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    try:
        with pytest.raises(capi.DotsocpError) as ei:
            ctx.map_report(x, y, mass=mass)
        assert ei.value.code == -4 and "map_report" in str(ei.value)                    # DOTSOCP_ESTATE
        ctx.finish(download=False)
        out = _strip(ctx.outputs())
        r0, r1 = np.asfortranarray(model.rho0), np.asfortranarray(model.rho1)

        def opts(n=n, nsub=1, direction=1):
            o = capi.AdvectOpts()
            o.n, o.nsub, o.direction, o.rho_floor = n, nsub, direction, 0.01
            return o

        def valid():
            xs, ys, rep, ln = x.copy(), y.copy(), capi.MapReport(), np.empty(n)
            rc, msg = _c_map(ctx, r0, r1, opts(), xs, ys, mass, rep, None, ln, None)     # disp and action may be NULL
            assert rc == 0, msg
            twin = A.map_report(out, x, y, mass=mass, rho_floor=0.01, per_particle=True)
            assert xs.tobytes() == twin["x"].tobytes() and ln.tobytes() == twin["len"].tobytes()
            assert rep.cost_action == twin["cost_action"] and rep.n == n

        def bad(i, v):
            m = mass.copy()
            m[i] = v
            return m

        R = capi.MapReport
        valid()
        for args in ((None, r1, opts(), x.copy(), y.copy(), mass, R()),                 # NULL rho0 / rho1 / opts / x / y / rep
                     (r0, None, opts(), x.copy(), y.copy(), mass, R()),
                     (r0, r1, None, x.copy(), y.copy(), mass, R()),
                     (r0, r1, opts(), None, y.copy(), mass, R()),
                     (r0, r1, opts(), x.copy(), None, mass, R()),
                     (r0, r1, opts(), x.copy(), y.copy(), mass, None),
                     (r0, r1, opts(n=0), x.copy(), y.copy(), mass, R()),
                     (r0, r1, opts(nsub=0), x.copy(), y.copy(), mass, R()),
                     (r0, r1, opts(direction=0), x.copy(), y.copy(), mass, R()),
                     (r0, r1, opts(direction=2), x.copy(), y.copy(), mass, R()),
                     (r0, r1, opts(), x.copy(), y.copy(), bad(4, -1e-300), R()),         # bad masses
                     (r0, r1, opts(), x.copy(), y.copy(), bad(4, np.nan), R()),
                     (r0, r1, opts(), x.copy(), y.copy(), bad(9, np.inf), R()),
                     (r0, r1, opts(), x.copy(), y.copy(), np.zeros(n), R()),
                     (r0, r1, opts(), np.full(n, np.nan), y.copy(), mass, R())):
            rc, msg = _c_map(ctx, *args)
            assert rc == -1 and b"map_report" in msg, (rc, msg)                         # DOTSOCP_EINVAL
            valid()                                                                     # a valid call still succeeds
        rc, msg = _c_map(ctx, r0, r1, opts(), x.copy(), y.copy(), None, R())            # a NULL mass is every mass 1.0
        assert rc == 0, msg
    finally:
        ctx.close()


def test_rccl_contexts_are_refused():
    from oracle.examples import get_example_2d
    rho0, rho1 = get_example_2d("example1", 16, 16)
    var, model = D.initialize_slab(rho0, rho1, 8, 0, 8)
    D.InitialScaling(var, model, True, None, dim=2)
    ctx = D.InPALMContext(var, dict(tau=1.9, sigma=1.0, tol=0.0, maxit=2, scaling=True), model,
                          rccl=(D.capi.rccl_unique_id(), 0, 1))
    try:
        ctx.run(-1)
        ctx.finish(download=False)
        x, y = A.seeds_on_nodes(16, 16, stride=4)
        with pytest.raises(capi.DotsocpError) as ei:
            ctx.map_report(x, y, mass=np.ones(x.size))
        assert ei.value.code == -1 and "map_report" in str(ei.value) and "RCCL" in str(ei.value)
    finally:
        ctx.close()


def _canary_child():
    """Runs in a fresh process with DOTSOCP_CANARY=1: particle blocks with the path sums, the seeds / masses / per-particle
    outputs / edges / sums / counters / block sums of the last slab lie between guard bands (the call fails with
    DOTSOCP_EHIP if a band was overwritten while its buffers are live)"""
    assert os.environ.get("DOTSOCP_CANARY") == "1"
    for case, split in (("2d_19x13x7", {}), ("1d_33x9", {}), ("2d_16x12x8", dict(nslabs=3))):
        ctx = _context(case, **split)
        try:
            out = _strip(ctx.outputs())
            x, y, mass = _particles(case, BLOCK + 1)
            for direction in (1, -1):
                for per in (True, False):
                    kw = dict(mass=mass if per else None, nsub=2, direction=direction, per_particle=per)
                    _same(ctx.map_report(x, y, **kw), A.map_report(out, x, y, **kw))
            assert capi.lib().dotsocp_canary_check() == 0, capi.lib().dotsocp_last_error().decode()
        finally:
            ctx.close()
    assert capi.lib().dotsocp_canary_check() == 0
    print("canary child ok")


def test_map_report_between_guard_bands():
    code = "import sys; sys.path.insert(0, sys.argv[1]); import test_gpu_map_report as T; T._canary_child()"
    env = dict(os.environ, DOTSOCP_CANARY="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "tests")], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("canary child ok"), out.stdout[-1000:] + out.stderr[-3000:]


# ---- real solves through the drivers: the anchor problems of tests/test_advect_host.py ----
def _after_solve(output, nsteps):
    dev = output["map_report"]
    out = _strip(output)
    one_d = "Ey" not in out
    shape = out["rho"].shape
    x, y = A.seeds_on_nodes(shape[0] if one_d else shape[1], None if one_d else shape[0])
    _same(dev, A.map_report(out, x, y, mass=A.masses_on_nodes(out["rho"][..., 0]), per_particle=True))
    eps = 4 * nsteps * 2.0 ** -52                                           # as tests/test_map_report_host.py: test_chain
    print("cost_map %.6f <= cost_length %.6f <= cost_action %.6f | detour_max %.3e, %d over 10 %%, %d still, %d clamped of %d"
          % (dev["cost_map"], dev["cost_length"], dev["cost_action"], dev["detour_max"], dev["detour_over"], dev["n_still"],
             dev["n_clamped"], dev["n"]))
    assert dev["cost_map"] <= dev["cost_length"] * (1 + eps) and dev["cost_length"] <= dev["cost_action"] * (1 + eps)
    return dev


def test_driver_1d_reports_the_map_after_a_real_solve():
    """N(0.3, 0.1^2) -> N(0.7, 0.05^2) on 129 x 33, tol 1e-5"""
    from test_advect_host import gaussian_1d_problem
    rho0, rho1, nt, _, _ = gaussian_1d_problem()
    output = D.solver_dotsocp1d(rho0, rho1, nt, 1, dict(tol=1e-5, maxit=8000), map_report=dict(stride=1, per_particle=True))[0]
    _after_solve(output, nt - 1)


def test_driver_2d_reports_the_map_after_a_real_solve():
    """The translation of a Gaussian by (0.2, 0.3) on 33 x 33 x 17, tol 1e-4: |T(x) - x| = sqrt(0.13) for every seed.
    tests/test_advect_host.py holds the end points of the anchor seeds (the nodes within two standard deviations of the
    start centre) to half a cell of T(x); so every such disp, and the root of their mass-weighted mean square, is within half
    a cell of sqrt(0.13) (triangle inequality)."""
    from test_advect_host import gaussian_2d_problem
    rho0, rho1, nt = gaussian_2d_problem()[:3]
    output = D.solver_dotsocp2d(rho0, rho1, nt, 1, dict(tol=1e-4, maxit=8000), map_report=dict(stride=1, per_particle=True))[0]
    dev = _after_solve(output, nt - 1)
    n = 33
    g = np.arange(n) / float(n - 1)
    Y, X = np.meshgrid(g, g, indexing="ij")
    anchors = (np.hypot(Y - 0.35, X - 0.4) <= 2 * 0.1).ravel(order="F")     # seeds_on_nodes' order: y fastest
    assert np.count_nonzero(anchors) == 129
    mass = A.masses_on_nodes(rho0)[anchors]
    disp = dev["disp"][anchors]
    cost_map = float(np.sum(mass * disp * disp) / np.sum(mass))
    print("anchor seeds: cost_map %.6f (W2^2 = 0.13), worst |disp - sqrt(0.13)| = %.3f cells"
          % (cost_map, np.max(np.abs(disp - np.sqrt(0.13))) * 32))
    assert abs(np.sqrt(cost_map) - np.sqrt(0.13)) <= 0.5 / 32


def test_map_report_needs_the_device_transfer():
    from test_advect_host import gaussian_1d_problem
    rho0, rho1, nt, _, _ = gaussian_1d_problem()
    with pytest.raises(ValueError):
        D.solver_dotsocp1d(rho0, rho1, nt, 1, dict(tol=1e-2, maxit=5), transfer="host", map_report=dict(stride=1))
