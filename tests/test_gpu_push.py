"""The mass push-forward on the device (csrc/advect.hip: k_deposit, k_frame_l1; dotsocp_push_mass,
InPALMContext.push_forward(), push= on the drivers) against the numpy twin advect.push_forward applied to ctx.outputs() of
the SAME context: frames, unit, final positions and the clamp count bit for bit (integer accumulation, no contraction:
include/dotsocp.h fixes every operation), l1 to rounding and identical between two calls and between slab splits.

States are made as in tests/test_gpu_advect.py (upload, begin(), no iteration, finish()): alpha so that rho lies mostly in
[0.5, 1.5] with exact zeros and negative entries and E is a smooth shear plus noise with |E / rho| up to about 0.5; q is
the q of oracle/generic_state.py (the push-forward does not read it)."""
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
    """seeds on nodes, on cell borders, on the sides and corners of the square, outside it and anywhere; masses in
    [0, 2) with exact zeros"""
    ny, nx, nt, _ = CASES[case]
    rng = np.random.default_rng(n + 7 * seed)
    one_d = ny is None
    gx = np.arange(nx) / float(nx - 1)
    gy = gx if one_d else np.arange(ny) / float(ny - 1)
    u = lambda k: rng.uniform(0, 1, k)                                    # noqa: E731
    xs = [rng.choice(gx, 12), rng.choice(gx, 8), u(8), np.array([0.0, 1.0, 0.0, 1.0, 1.0, -0.2, 1.5, 0.3])]
    ys = [rng.choice(gy, 12), u(8), rng.choice(gy, 8), np.array([0.0, 0.0, 1.0, 1.0, 0.5, 0.4, 0.5, 1.0])]
    x, y = np.concatenate(xs), np.concatenate(ys)
    x, y = np.concatenate([x, u(n - x.size)]), np.concatenate([y, u(n - y.size)])
    mass = rng.uniform(0.0, 2.0, n)
    mass[[3, n // 2]] = 0.0
    return x, (None if one_d else y), mass


def _strip(out):
    return {k: v for k, v in out.items() if k in ("rho", "Ex", "Ey")}


def _same(dev, twin):
    """frames, counts, unit, nodes, final positions, clamp count, units: the same bits; l1: to rounding"""
    assert set(dev) == set(twin)
    assert dev["unit"] == twin["unit"] and dev["n_clamped"] == twin["n_clamped"] and dev["total_units"] == twin["total_units"]
    assert np.array_equal(dev["nodes"], twin["nodes"])
    for k in ("frames", "counts", "x", "y"):
        if twin[k] is None:
            assert dev[k] is None, k
            continue
        d, t = np.asarray(dev[k]), np.asarray(twin[k])
        assert d.shape == t.shape and d.dtype == t.dtype, k
        if d.tobytes(order="F") != t.tobytes(order="F"):
            raise AssertionError("%s differs in %d of %d entries, largest difference %.3e"
                                 % (k, np.count_nonzero(d != t), d.size, np.nanmax(np.abs(d - t))))
    np.testing.assert_allclose(dev["l1"], twin["l1"], rtol=1e-12, atol=0.0)
    axes = tuple(range(dev["counts"].ndim - 1))
    assert np.all(dev["counts"].sum(axis=axes) == dev["total_units"])     # exact conservation, frame by frame


def _bytes(r):
    return b"".join(np.asarray(r[k]).tobytes(order="F") for k in ("frames", "l1", "x", "y") if r[k] is not None) + \
        int(r["n_clamped"]).to_bytes(8, "little") + np.float64(r["unit"]).tobytes()


def _runs(nt):
    """all nt nodes, then a sparse list without node 0 and the last node; both directions; nsub 1 and 2"""
    sparse = [1, 2, nt - 3, nt - 2] if nt >= 7 else [1, nt - 2]
    return [(frames, direction, nsub) for frames in (None, sorted(set(sparse))) for direction in (1, -1) for nsub in (1, 2)]


def _check_context(ctx, case, counts=COUNTS):
    out = _strip(ctx.outputs())
    assert np.all(np.isfinite(out["rho"])) and np.count_nonzero(out["rho"] <= 0.0) >= 2
    raw = {}
    for n in counts:
        x, y, mass = _particles(case, n)
        for frames, direction, nsub in _runs(CASES[case][2]):
            kw = dict(mass=mass, frames=frames, nsub=nsub, direction=direction)
            dev = ctx.push_forward(x, y, **kw)
            _same(dev, A.push_forward(out, x, y, **kw))
            raw[(n, None if frames is None else tuple(frames), direction, nsub)] = _bytes(dev)
        again = ctx.push_forward(x, y, mass=mass, nsub=2)
        assert _bytes(again) == raw[(n, None, 1, 2)]                        # two calls: identical bytes, l1 included
        plain = ctx.advect(x, y, nsub=2)                                    # the trajectories are advect()'s
        assert plain["x"].tobytes() == again["x"].tobytes() and plain["n_clamped"] == again["n_clamped"]
        assert y is None or plain["y"].tobytes() == again["y"].tobytes()
    return raw


@pytest.mark.parametrize("case", ["2d_19x13x7", "w_16x16x8", "1d_33x9"])
def test_push_equals_the_twin(case):
    ctx = _context(case)
    try:
        _check_context(ctx, case)
    finally:
        ctx.close()


def test_contention():
    """4096 particles on one point, and 4096 on one grid row: every atomic of a wavefront on the same four (two rows of)
    counters"""
    case = "2d_19x13x7"
    ny, nx, nt, _ = CASES[case]
    n = 4096
    rng = np.random.default_rng(99)
    mass = rng.uniform(0.0, 1.0, n)
    ctx = _context(case)
    try:
        out = _strip(ctx.outputs())
        for name, x, y in (("point", np.full(n, 0.37), np.full(n, 0.58)),
                           ("row", np.full(n, 5.0 / (nx - 1)), rng.uniform(0, 1, n)),
                           ("column", rng.uniform(0, 1, n), np.full(n, 7.25 / (ny - 1)))):
            dev = ctx.push_forward(x, y, mass=mass, frames=[0, 3, nt - 1])
            _same(dev, A.push_forward(out, x, y, mass=mass, frames=[0, 3, nt - 1]))
            touched = np.count_nonzero(dev["counts"][..., 0])
            print(name, ": counters touched at node 0:", touched)
            assert touched <= (4 if name == "point" else 2 * max(ny, nx))
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
        for frames, direction, nsub in _runs(CASES[case][2]):
            dev = ctx.push_forward(x, y, mass=mass, frames=frames, nsub=nsub, direction=direction)
            assert _bytes(dev) == raw[(n, None if frames is None else tuple(frames), direction, nsub)], (frames, direction, nsub)
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


def _c_push(ctx, r0, r1, o, x, y, mass, nodes, frames, l1=None):
    nc, unit = capi.i64(-7), capi.dbl(-1.0)
    ptr = lambda a: None if a is None else a.ctypes.data                    # noqa: E731
    rc = capi.lib().dotsocp_push_mass(ctx._ctx, ptr(r0), ptr(r1), None if o is None else ctypes.byref(o), ptr(x), ptr(y),
                                      ptr(mass), ptr(nodes), ptr(frames), ctypes.byref(nc), ctypes.byref(unit), ptr(l1))
    return rc, capi.lib().dotsocp_last_error()


def test_errors_name_the_call():
    L = capi.lib()
    ny, nx, nt = 9, 7, 4
    rng = np.random.default_rng(5)
    var, model = D.initialize(rng.uniform(0.5, 1.5, (ny, nx)), rng.uniform(0.5, 1.5, (ny, nx)), nt)
    D.InitialScaling(var, model, True, None, dim=2)
    ctx = D.InPALMContext(var, dict(tau=1.9, sigma=1.0, tol=0.0, maxit=1, scaling=True), model)
    n = 10
    x, y, mass = rng.uniform(0, 1, n), rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    try:
        with pytest.raises(capi.DotsocpError) as ei:
            ctx.push_forward(x, y, mass=mass)
        assert ei.value.code == -4 and "push_mass" in str(ei.value)                     # DOTSOCP_ESTATE
        ctx.finish(download=False)
        out = _strip(ctx.outputs())
        r0, r1 = np.asfortranarray(model.rho0), np.asfortranarray(model.rho1)
        nodes = np.array([0, 2, 3], dtype=np.int64)
        fr = np.empty((ny, nx, 3), order="F")

        def opts(n=n, nsub=1, direction=1, nf=3):
            o = capi.PushOpts()
            o.n, o.nsub, o.direction, o.rho_floor, o.nf = n, nsub, direction, 0.01, nf
            return o

        def valid():
            xs, ys, l1 = x.copy(), y.copy(), np.empty(3)
            rc, msg = _c_push(ctx, r0, r1, opts(), xs, ys, mass, nodes, fr, l1)
            assert rc == 0, msg
            twin = A.push_forward(out, x, y, mass=mass, frames=nodes, rho_floor=0.01)
            assert fr.tobytes(order="F") == twin["frames"].tobytes(order="F") and xs.tobytes() == twin["x"].tobytes()
            np.testing.assert_allclose(l1, twin["l1"], rtol=1e-12)

        def bad(i, v):
            m = mass.copy()
            m[i] = v
            return m

        I = lambda *v: np.array(v, dtype=np.int64)                          # noqa: E731,E741
        valid()
        for args in ((r0, r1, opts(), x.copy(), y.copy(), mass, nodes, None),           # NULL frames / mass / frame_nodes
                     (r0, r1, opts(), x.copy(), y.copy(), None, nodes, fr),
                     (r0, r1, opts(), x.copy(), y.copy(), mass, None, fr),
                     (None, r1, opts(), x.copy(), y.copy(), mass, nodes, fr),
                     (r0, r1, None, x.copy(), y.copy(), mass, nodes, fr),
                     (r0, r1, opts(), x.copy(), None, mass, nodes, fr),
                     (r0, r1, opts(nf=0), x.copy(), y.copy(), mass, nodes, fr),
                     (r0, r1, opts(nsub=0), x.copy(), y.copy(), mass, nodes, fr),
                     (r0, r1, opts(direction=0), x.copy(), y.copy(), mass, nodes, fr),
                     (r0, r1, opts(n=0), x.copy(), y.copy(), mass, nodes, fr),
                     (r0, r1, opts(), x.copy(), y.copy(), mass, I(0, 2, 2), fr),         # bad nodes
                     (r0, r1, opts(), x.copy(), y.copy(), mass, I(2, 1, 3), fr),
                     (r0, r1, opts(), x.copy(), y.copy(), mass, I(-1, 1, 3), fr),
                     (r0, r1, opts(), x.copy(), y.copy(), mass, I(0, 2, nt), fr),
                     (r0, r1, opts(), x.copy(), y.copy(), bad(4, -1e-300), nodes, fr),   # bad masses
                     (r0, r1, opts(), x.copy(), y.copy(), bad(4, np.nan), nodes, fr),
                     (r0, r1, opts(), x.copy(), y.copy(), bad(9, np.inf), nodes, fr),
                     (r0, r1, opts(), x.copy(), y.copy(), np.zeros(n), nodes, fr),
                     (r0, r1, opts(), np.full(n, np.nan), y.copy(), mass, nodes, fr)):
            rc, msg = _c_push(ctx, *args)
            assert rc == -1 and b"push_mass" in msg, (rc, msg)                          # DOTSOCP_EINVAL
            valid()                                                                     # a valid call still succeeds
        # n_clamped, unit and l1 may be NULL
        assert L.dotsocp_push_mass(ctx._ctx, r0.ctypes.data, r1.ctypes.data, ctypes.byref(opts()), x.copy().ctypes.data,
                                   y.copy().ctypes.data, mass.ctypes.data, nodes.ctypes.data, fr.ctypes.data, None, None, None) == 0
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
            ctx.push_forward(x, y, mass=np.ones(x.size))
        assert ei.value.code == -1 and "push_mass" in str(ei.value) and "RCCL" in str(ei.value)
    finally:
        ctx.close()


def _canary_child():
    """Runs in a fresh process with DOTSOCP_CANARY=1: particle blocks, count planes, tile sums and l1 slots lie between
    guard bands (the call fails with DOTSOCP_EHIP if a band was overwritten while its buffers are live)"""
    assert os.environ.get("DOTSOCP_CANARY") == "1"
    for case, split in (("2d_19x13x7", {}), ("1d_33x9", {}), ("2d_16x12x8", dict(nslabs=3))):
        ctx = _context(case, **split)
        try:
            out = _strip(ctx.outputs())
            x, y, mass = _particles(case, BLOCK + 1)
            for direction in (1, -1):
                dev = ctx.push_forward(x, y, mass=mass, nsub=2, direction=direction)
                _same(dev, A.push_forward(out, x, y, mass=mass, nsub=2, direction=direction))
            assert capi.lib().dotsocp_canary_check() == 0, capi.lib().dotsocp_last_error().decode()
        finally:
            ctx.close()
    assert capi.lib().dotsocp_canary_check() == 0
    print("canary child ok")


def test_push_between_guard_bands():
    code = "import sys; sys.path.insert(0, sys.argv[1]); import test_gpu_push as T; T._canary_child()"
    env = dict(os.environ, DOTSOCP_CANARY="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "tests")], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("canary child ok"), out.stdout[-1000:] + out.stderr[-3000:]


# ---- real solves through the drivers: the anchor problems of tests/test_advect_host.py ----
def _after_solve(output, bound):
    dev = output["push"]
    out = _strip(output)
    one_d = "Ey" not in out
    shape = out["rho"].shape
    x, y = A.seeds_on_nodes(shape[0] if one_d else shape[1], None if one_d else shape[0])
    _same(dev, A.push_forward(out, x, y, mass=A.masses_on_nodes(out["rho"][..., 0])))
    print("l1 of the pushed rho0: last frame %.4e (bound %.4e), middle %.4e, %d clamped"
          % (dev["l1"][-1], bound, dev["l1"][shape[-1] // 2], dev["n_clamped"]))
    assert dev["l1"][0] <= 0.5 * dev["unit"]                                # on their own nodes: rho0 rounded to whole units
    assert dev["l1"][-1] <= bound


def test_driver_1d_pushes_rho0_after_a_real_solve():
    """N(0.3, 0.1^2) -> N(0.7, 0.05^2) on 129 x 33, tol 1e-5.  The twin on the CPU oracle's solve of the same problem
    (oracle/driver.py: solve_single_level, same tolerance, one level) gives l1 = 2.3806e-02 at the last frame (mean
    density 1); allowed here: twice that -- the device trajectory differs from the oracle's by up to 1e-9 and the stop
    iteration by one check.  Measured on the device: 2.3806e-02."""
    from test_advect_host import gaussian_1d_problem
    rho0, rho1, nt, _, _ = gaussian_1d_problem()
    output = D.solver_dotsocp1d(rho0, rho1, nt, 1, dict(tol=1e-5, maxit=8000), push=dict(stride=1))[0]
    _after_solve(output, 2 * 2.3806e-02)


def test_driver_2d_pushes_rho0_after_a_real_solve():
    """The translation of a Gaussian on 33 x 33 x 17, tol 1e-4.  The twin on the CPU oracle's solve of the same problem
    gives l1 = 6.3310e-02 at the last frame (mean density 1); allowed here: twice that (as above).  Measured on the device: 6.3310e-02."""
    from test_advect_host import gaussian_2d_problem
    rho0, rho1, nt = gaussian_2d_problem()[:3]
    output = D.solver_dotsocp2d(rho0, rho1, nt, 1, dict(tol=1e-4, maxit=8000), push=dict(stride=1))[0]
    _after_solve(output, 2 * 6.3310e-02)


def test_push_needs_the_device_transfer():
    from test_advect_host import gaussian_1d_problem
    rho0, rho1, nt, _, _ = gaussian_1d_problem()
    with pytest.raises(ValueError):
        D.solver_dotsocp1d(rho0, rho1, nt, 1, dict(tol=1e-2, maxit=5), transfer="host", push=dict(stride=1))
