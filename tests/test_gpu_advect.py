"""Velocity and particle transport on the device (csrc/advect.hip, dotsocp_recover_velocity, dotsocp_advect_particles,
InPALMContext.velocity() / .advect()) against the numpy twins of dot-socp_amd/advect.py applied to ctx.outputs() of the
SAME context: bit for bit -- the kernels are built without contraction and include/dotsocp.h fixes every operation and its
order, so there is no tolerance here.

States are made here as in tests/test_gpu_report.py (upload, begin(), no iteration, finish()): alpha so that rho is mostly
in [0.5, 1.5] with exact zeros, negative entries and a NaN, E a smooth shear plus noise with |E / rho| up to about 0.5, and
next to every side of the square a node of low density (just above the floor) whose flux points at the wall.  Before a
device result is looked at, the outputs and the twin are checked to exercise what is compared (_conditions): particles
that cross several cells in each direction, particles clamped on each side, masked nodes with particles beside them.  (The
3 x 3 x 2 grid cannot meet that by counting, as in the report's test: it is compared with the twin only.)"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dotsocp_amd as D
from dotsocp_amd import advect as A
from dotsocp_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (ny, nx, nt, weighted, conditions asserted); 1-D: ny = None
CASES = {
    "2d_19x13x6": (19, 13, 6, False, True),
    "2d_3x3x2": (3, 3, 2, False, False),
    "1d_301x9": (None, 301, 9, False, True),
    "w_17x21x5": (17, 21, 5, True, True),
    "2d_19x13x7": (19, 13, 7, False, True),
}
N_PART = 2000
RUNS = [(nsub, direction, traj) for nsub in (1, 3) for direction in (1, -1) for traj in (False, True)]


def _density(rng, shape):
    r = rng.uniform(0.5, 1.5, shape)
    r.flat[rng.choice(r.size, 3, replace=False)] = 0.0
    return r


def _plants(ny, nx):
    """(y, x, axis, sign): a node one in from each side of the square whose flux points at that side"""
    if ny is None:
        return [(None, 1, 1, -1.0), (None, nx - 2, 1, 1.0)]
    if min(ny, nx) < 5:
        return []
    return [(ny // 2, 1, 1, -1.0), (ny // 2, nx - 2, 1, 1.0), (1, nx // 2, 0, -1.0), (ny - 2, nx // 2, 0, 1.0)]


def _state(case):
    """(var, model, weighted) of the generic state of `case`"""
    ny, nx, nt, weighted, _ = CASES[case]
    rng = np.random.default_rng(sorted(CASES).index(case) + 31415)
    one_d = ny is None
    shape = (nx,) if one_d else (ny, nx)
    rho0, rho1 = _density(rng, shape), _density(rng, shape)
    floor = A.default_rho_floor(rho0, rho1)
    for (y, x, axis, sign) in _plants(ny, nx):
        rho0[x if one_d else (y, x)] = 1.5 * floor
        rho1[x if one_d else (y, x)] = 1.5 * floor
    var, model = D.initialize(rho0, rho1, nt)
    nq = var.q.size
    if weighted:
        model.weight = 0.5 + (1e6 - 0.5) * rng.uniform(0, 1, nq) ** 32       # as tests/test_gpu_report.py
    D.InitialScaling(var, model, not weighted, None, dim=1 if one_d else 2, weighted=weighted)
    my = 1 if one_d else ny
    # a(.) of the outputs: the cells (density) ...
    a0 = rng.uniform(0.5, 1.5, (my, nx, nt - 1))
    if nt >= 3:
        for k, val in enumerate((0.0, 0.0, 0.0, -0.3, -0.7, np.nan)):    # both cells around node 1 / node nt - 2
            p = rng.integers(0, my * nx)
            t = 0 if k % 2 == 0 else nt - 3
            a0[p % my, p // my, t:t + 2] = val
    # ... and the edges (flux): a shear plus noise, halved on the end layers (which recover_RhoE doubles)
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
    for (y, x, axis, sign) in _plants(ny, nx):
        for t in (0, nt - 1):
            if axis == 1:
                ax[0 if one_d else y, x - 1:x + 1, t] = 0.25 * sign
            else:
                ay[y - 1:y + 1, x, t] = 0.25 * sign
    target = np.concatenate([a.ravel(order="F") for a in (a0, ax, ay) if a is not None])
    assert target.size == nq
    var.alpha = target / (var.cScale * var.D) / (model.weight if weighted else 1.0)
    var.q = rng.normal(0, 1, nq)
    return var, model, weighted


def _context(case, method="inPALM", **split):
    """A finished context on the generic state of `case` (no iteration)"""
    var, model, weighted = _state(case)
    opts = dict(tau=1.9, sigma=1.0, tol=0.0, maxit=1, ifCheckStepByStep=False, scaling=True)
    ctx = D.InPALMContext(var, opts, model, weighted=weighted, method=method, **split)
    ctx.finish(download=False)
    return ctx


def _seeds(case):
    ny, nx, nt, _, _ = CASES[case]
    rng = np.random.default_rng(sorted(CASES).index(case) + 27182)
    one_d = ny is None
    my = 1 if one_d else ny
    nodes_x, nodes_y = A.seeds_on_nodes(nx, ny)                           # every node of the first layer
    if one_d:
        nodes_y = np.zeros(nx)
    gx, gy = np.arange(nx) / float(nx - 1), np.arange(my) / float(max(my - 1, 1))
    u = lambda n: rng.uniform(0, 1, n)                                    # noqa: E731
    xs = [nodes_x, rng.choice(gx, 100), u(100),                           # on cell borders in x, in y
          np.zeros(25), np.ones(25), u(25), u(25),                        # the four sides
          np.array([0.0, 0.0, 1.0, 1.0]), np.array([-1e-3, 1 + 1e-3, -0.5, 1.5, 0.3, 0.6, -1e-3, 1.5])]     # corners, outside
    ys = [nodes_y, u(100), rng.choice(gy, 100),
          u(25), u(25), np.zeros(25), np.ones(25),
          np.array([0.0, 1.0, 0.0, 1.0]), np.array([0.2, 0.4, 0.5, 0.5, -1e-3, 1 + 1e-3, -0.7, 2.0])]
    for (y, x, axis, sign) in _plants(ny, nx):                            # beside the low-density nodes, on the side away from the wall
        px, py = x / float(nx - 1), (0.0 if one_d else y / float(ny - 1))
        d = -sign * rng.uniform(0.2, 0.8, 5)
        xs.append(px + (d / (nx - 1) if axis == 1 else 0.0) + np.zeros(5))
        ys.append(py + (d / (my - 1) if axis == 0 else 0.0) + np.zeros(5))
    x, y = np.concatenate(xs), np.concatenate(ys)
    assert x.size <= N_PART
    x, y = np.concatenate([x, u(N_PART - x.size)]), np.concatenate([y, u(N_PART - y.size)])
    return x, (None if one_d else y)


def _strip(out):
    return {k: v for k, v in out.items() if k in ("rho", "Ex", "Ey")}


def _conditions(case, out, x0, y0):
    """asserted on ctx.outputs() and the twin before any device result is looked at (module docstring)"""
    ny, nx, nt, _, _ = CASES[case]
    one_d = ny is None
    rho = out["rho"]
    floor = A.default_rho_floor(rho[..., 0], rho[..., -1])
    inside = (rho > 0.5) & (rho < 1.5)
    assert np.count_nonzero(inside) >= 0.9 * rho.size
    assert np.count_nonzero(rho == 0.0) >= 3 and np.count_nonzero(rho < 0.0) >= 2 and np.count_nonzero(np.isnan(rho)) >= 1
    v = A.velocity(out, floor)
    speed = np.abs(v["vx"]) if one_d else np.hypot(v["vx"], v["vy"])
    assert 0.3 <= np.quantile(speed, 0.95) <= 0.8, np.quantile(speed, 0.95)
    r = A.advect(out, x0, y0, trajectories=True)
    axes = [("x", x0, nx)] + ([] if one_d else [("y", y0, ny)])
    for name, s0, n in axes:
        cells = (r[name] - np.clip(s0, 0, 1)) * (n - 1)
        for sgn in (1, -1):
            share = np.count_nonzero(sgn * cells >= 2) / float(s0.size)
            print(case, name, "direction", sgn, ": share of particles crossing two or more cells", share)
            assert share >= 0.05
        tr = r["traj_" + name][:, 1:]
        began_inside = (s0 > 0) & (s0 < 1)
        for wall in (0.0, 1.0):
            hit = np.count_nonzero(began_inside & np.any(tr == wall, axis=1))
            print(case, name, "=", wall, ": particles clamped onto it", hit)
            assert hit >= 1
    assert r["n_clamped"] >= 2 * len(axes)
    masked = ~(rho[..., 0] > floor)
    assert np.count_nonzero(~(rho > floor)) >= 3 and np.count_nonzero(masked) >= 3
    i = np.minimum(np.floor(np.clip(x0, 0, 1) * (nx - 1)).astype(int), nx - 2)
    if one_d:
        beside = masked[i] | masked[i + 1]
    else:
        j = np.minimum(np.floor(np.clip(y0, 0, 1) * (ny - 1)).astype(int), ny - 2)
        beside = masked[j, i] | masked[j + 1, i] | masked[j, i + 1] | masked[j + 1, i + 1]
    assert np.count_nonzero(beside) >= 1


def _same(dev, twin):
    """positions, trajectories and the clamp count: the same bits"""
    assert dev["n_clamped"] == twin["n_clamped"], (dev["n_clamped"], twin["n_clamped"])
    for k in ("x", "y", "traj_x", "traj_y"):
        if twin[k] is None:
            assert dev[k] is None, k
            continue
        d, t = np.asarray(dev[k]), np.asarray(twin[k])
        if d.tobytes(order="F") != t.tobytes(order="F"):
            bad = np.flatnonzero(d.ravel(order="F").view(np.uint64) != t.ravel(order="F").view(np.uint64))
            raise AssertionError("%s differs in %d of %d entries, largest difference %.3e"
                                 % (k, bad.size, d.size, np.nanmax(np.abs(d - t))))


def _run_bytes(r):
    return b"".join(np.asarray(r[k]).tobytes(order="F") for k in ("x", "y", "traj_x", "traj_y") if r[k] is not None) + \
        int(r["n_clamped"]).to_bytes(8, "little")


def _check_context(ctx, case, conditions):
    """points 1 and 2 of the plan on one finished context; returns the bytes of every run"""
    x0, y0 = _seeds(case)
    out = _strip(ctx.outputs())
    floor = A.default_rho_floor(ctx.model.rho0, ctx.model.rho1)
    if conditions:
        _conditions(case, out, x0, y0)
    v, tv = ctx.velocity(), A.velocity(out, floor)
    assert set(v) == set(tv)
    for k in tv:
        assert v[k].shape == tv[k].shape and v[k].tobytes(order="F") == tv[k].tobytes(order="F"), k
    v2, tv2 = ctx.velocity(rho_floor=0.6), A.velocity(out, 0.6)            # another floor: a third of the nodes masked
    assert all(v2[k].tobytes(order="F") == tv2[k].tobytes(order="F") for k in tv2)
    raw = {}
    for nsub, direction, traj in RUNS:
        dev = ctx.advect(x0, y0, nsub=nsub, direction=direction, trajectories=traj)
        twin = A.advect(out, x0, y0, nsub=nsub, direction=direction, trajectories=traj)
        print(case, "nsub", nsub, "direction", direction, "trajectories", traj, "clamped", dev["n_clamped"], twin["n_clamped"])
        _same(dev, twin)
        raw[(nsub, direction, traj)] = _run_bytes(dev)
    return raw


_one_slab = {}


def _one_slab_run(case):
    """the bytes of every run on the one-slab context of `case` (checked against the twin), made once"""
    if case not in _one_slab:
        ctx = _context(case)
        try:
            raw = _check_context(ctx, case, CASES[case][4])
            x0, y0 = _seeds(case)
            again = _run_bytes(ctx.advect(x0, y0, nsub=3, direction=1, trajectories=True))
            assert again == raw[(3, 1, True)]                               # two consecutive calls: identical bytes
            _one_slab[case] = (raw, ctx.velocity())
        finally:
            ctx.close()
    return _one_slab[case]


@pytest.mark.parametrize("case", [c for c in CASES if c != "2d_19x13x7"])
def test_velocity_and_particles_equal_the_twin(case):
    _one_slab_run(case)


@pytest.mark.parametrize("split", [dict(nslabs=2), dict(nslabs=3), dict(ngpu=3)], ids=["nslabs2", "nslabs3", "ngpu3"])
def test_time_slabs_give_the_same_bytes(split):
    case = "2d_19x13x7"
    raw, vel = _one_slab_run(case)
    x0, y0 = _seeds(case)
    ctx = _context(case, **split)
    try:
        sv = ctx.velocity()
        assert all(sv[k].tobytes(order="F") == vel[k].tobytes(order="F") for k in vel)
        for nsub, direction, traj in RUNS:
            if nsub == 3 or traj:                                           # both directions, with and without trajectories
                assert _run_bytes(ctx.advect(x0, y0, nsub=nsub, direction=direction, trajectories=traj)) == raw[(nsub, direction, traj)], \
                    (nsub, direction, traj)
    finally:
        ctx.close()


@pytest.mark.parametrize("method", ["PALM", "acc-ADMM"])
def test_other_loops(method):
    case = "2d_19x13x6"
    ctx = _context(case, method=method)
    try:
        _check_context(ctx, case, True)
    finally:
        ctx.close()


def _c_advect(ctx, r0, r1, o, x, y, tx=None, ty=None):
    nc = capi.i64(-7)
    ptr = lambda a: None if a is None else capi.fptr(a)                     # noqa: E731
    rc = capi.lib().dotsocp_advect_particles(ctx._ctx, ptr(r0), ptr(r1), None if o is None else ctypes.byref(o), ptr(x), ptr(y),
                                             ptr(tx), ptr(ty), ctypes.byref(nc))
    return rc, capi.lib().dotsocp_last_error()


def test_errors_name_the_call():
    L = capi.lib()
    ny, nx, nt = 9, 7, 4
    rng = np.random.default_rng(5)
    var, model = D.initialize(_density(rng, (ny, nx)), _density(rng, (ny, nx)), nt)
    D.InitialScaling(var, model, True, None, dim=2)
    ctx = D.InPALMContext(var, dict(tau=1.9, sigma=1.0, tol=0.0, maxit=1, scaling=True), model)
    x, y = rng.uniform(0, 1, 10), rng.uniform(0, 1, 10)
    try:
        with pytest.raises(capi.DotsocpError) as ei:
            ctx.advect(x, y)
        assert ei.value.code == -4 and "advect_particles" in str(ei.value)              # DOTSOCP_ESTATE
        with pytest.raises(capi.DotsocpError) as ei:
            ctx.velocity()
        assert ei.value.code == -4 and "recover_velocity" in str(ei.value)
        ctx.finish(download=False)
        r0, r1 = np.asfortranarray(model.rho0), np.asfortranarray(model.rho1)

        def opts(n=10, nsub=1, direction=1):
            o = capi.AdvectOpts()
            o.n, o.nsub, o.direction, o.rho_floor = n, nsub, direction, 0.01
            return o

        nan_x = x.copy()
        nan_x[3] = np.nan
        inf_y = y.copy()
        inf_y[9] = np.inf
        for args in ((None, r1, opts(), x.copy(), y.copy()), (r0, None, opts(), x.copy(), y.copy()),
                     (r0, r1, None, x.copy(), y.copy()), (r0, r1, opts(), None, y.copy()), (r0, r1, opts(), x.copy(), None),
                     (r0, r1, opts(nsub=0), x.copy(), y.copy()), (r0, r1, opts(direction=0), x.copy(), y.copy()),
                     (r0, r1, opts(direction=2), x.copy(), y.copy()), (r0, r1, opts(n=0), x.copy(), y.copy()),
                     (r0, r1, opts(), nan_x, y.copy()), (r0, r1, opts(), x.copy(), inf_y)):
            rc, msg = _c_advect(ctx, *args)
            assert rc == -1 and b"advect_particles" in msg, (rc, msg)                   # DOTSOCP_EINVAL
        with pytest.raises(capi.DotsocpError) as ei:
            ctx.advect(np.empty(0), np.empty(0))
        assert ei.value.code == -1
        xs, ys = x.copy(), y.copy()
        rc, msg = _c_advect(ctx, r0, r1, opts(), xs, ys)
        assert rc == 0, msg
        twin = A.advect(_strip(ctx.outputs()), x, y, rho_floor=0.01)
        assert xs.tobytes() == twin["x"].tobytes() and ys.tobytes() == twin["y"].tobytes()
        assert L.dotsocp_advect_particles(ctx._ctx, capi.fptr(r0), capi.fptr(r1), ctypes.byref(opts()), capi.fptr(x.copy()),
                                          capi.fptr(y.copy()), None, None, None) == 0   # n_clamped may be NULL
        # recover_velocity: NULL densities are refused, vx and vy may each be NULL
        shp = (ny, nx, nt)
        vx, vy = np.empty(shp, order="F"), np.empty(shp, order="F")
        assert L.dotsocp_recover_velocity(ctx._ctx, None, capi.fptr(r1), 0.01, capi.fptr(vx), capi.fptr(vy)) == -1
        assert b"recover_velocity" in L.dotsocp_last_error()
        assert L.dotsocp_recover_velocity(ctx._ctx, capi.fptr(r0), capi.fptr(r1), 0.01, capi.fptr(vx), capi.fptr(vy)) == 0
        ax, ay = np.empty(shp, order="F"), np.empty(shp, order="F")
        assert L.dotsocp_recover_velocity(ctx._ctx, capi.fptr(r0), capi.fptr(r1), 0.01, capi.fptr(ax), None) == 0
        assert L.dotsocp_recover_velocity(ctx._ctx, capi.fptr(r0), capi.fptr(r1), 0.01, None, capi.fptr(ay)) == 0
        assert L.dotsocp_recover_velocity(ctx._ctx, capi.fptr(r0), capi.fptr(r1), 0.01, None, None) == 0
        assert ax.tobytes(order="F") == vx.tobytes(order="F") and ay.tobytes(order="F") == vy.tobytes(order="F")
    finally:
        ctx.close()


def _canary_child():
    """Runs in a fresh process with DOTSOCP_CANARY=1: the ring of velocity layers and the particle blocks lie between guard
    bands (both calls fail with DOTSOCP_EHIP if a band was overwritten while their buffers are live)"""
    assert os.environ.get("DOTSOCP_CANARY") == "1"
    case = "2d_19x13x6"
    ctx = _context(case)
    try:
        _check_context(ctx, case, False)
        assert capi.lib().dotsocp_canary_check() == 0, capi.lib().dotsocp_last_error().decode()   # the ring is live here
    finally:
        ctx.close()
    ctx = _context("2d_19x13x7", nslabs=3)
    try:
        x0, y0 = _seeds("2d_19x13x7")
        ctx.velocity()
        for direction in (1, -1):
            ctx.advect(x0, y0, nsub=2, direction=direction, trajectories=True)
        assert capi.lib().dotsocp_canary_check() == 0, capi.lib().dotsocp_last_error().decode()
    finally:
        ctx.close()
    assert capi.lib().dotsocp_canary_check() == 0
    print("canary child ok")


def test_advect_between_guard_bands():
    code = "import sys; sys.path.insert(0, sys.argv[1]); import test_gpu_advect as T; T._canary_child()"
    env = dict(os.environ, DOTSOCP_CANARY="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "tests")], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("canary child ok"), out.stdout[-1000:] + out.stderr[-3000:]


# ---- real solves: the anchors of tests/test_advect_host.py, now through the drivers ----
def _after_solve(output, plain, seeds, err, cell):
    dev = output["advect"]
    out = {k: v for k, v in output.items() if k != "advect"}
    _same(dev, A.advect(_strip(out), *seeds, trajectories=True))
    worst = err(dev)
    print("worst map error %.4f = %.2f cells, %d clamped" % (worst, worst / cell, dev["n_clamped"]))
    assert worst <= 0.5 * cell
    assert "advect" not in plain and set(plain) == set(out) and all(np.array_equal(plain[k], out[k]) for k in plain)


def test_driver_1d_carries_particles_after_a_real_solve():
    from test_advect_host import gaussian_1d_problem
    rho0, rho1, nt, x0, target = gaussian_1d_problem()
    o = dict(tol=1e-5, maxit=8000)
    output = D.solver_dotsocp1d(rho0, rho1, nt, 1, o, advect=dict(x=x0, trajectories=True))[0]
    plain = D.solver_dotsocp1d(rho0, rho1, nt, 1, o)[0]
    _after_solve(output, plain, (x0,), lambda r: np.max(np.abs(r["x"] - target)), 1.0 / (rho0.size - 1))


def test_driver_2d_carries_particles_after_a_real_solve():
    from test_advect_host import gaussian_2d_problem
    rho0, rho1, nt, x0, y0, tx, ty = gaussian_2d_problem()
    o = dict(tol=1e-4, maxit=8000)
    output = D.solver_dotsocp2d(rho0, rho1, nt, 1, o, advect=dict(x=x0, y=y0, trajectories=True))[0]
    plain = D.solver_dotsocp2d(rho0, rho1, nt, 1, o)[0]
    _after_solve(output, plain, (x0, y0), lambda r: np.max(np.hypot(r["x"] - tx, r["y"] - ty)), 1.0 / (rho0.shape[1] - 1))
