"""The numpy twin of the map report (dot-socp_amd/advect.py: map_report) on its own: fields whose paths are known in closed
form, the chain disp^2 <= len^2 <= action, walls and masked regions, independence of the particle order, and the two anchor
problems of tests/test_advect_host.py on the CPU oracle's solutions -- independent of the device code, which
tests/test_gpu_map_report.py holds to this twin bit for bit."""
import functools

import numpy as np
import pytest

import dotsocp_amd as D
from dotsocp_amd import advect as A
from dotsocp_amd import report as R
from oracle import driver as OD
from test_advect_host import (_const_out, _ring_seeds, _rk4_bound, _rotation_out, gaussian_1d_problem,
                              gaussian_2d_problem)

U = 2.0 ** -53
SUMS = ("mass", "cost_map", "cost_length", "cost_action", "disp_mean", "len_mean")


def test_exports():
    assert D.map_report is A.map_report


@pytest.mark.parametrize("nsub", [1, 2])
def test_constant_field(nsub):
    """straight paths at constant speed: disp^2 = len^2 = action = ex^2 + ey^2, up to the rounding of n_steps steps"""
    out = _const_out(9, 7, 5, 0.3, -0.2)
    rng = np.random.default_rng(1)
    x0, y0 = rng.uniform(0.05, 0.65, 200), rng.uniform(0.25, 0.95, 200)           # no clamp fires
    r = A.map_report(out, x0, y0, nsub=nsub, rho_floor=0.5, per_particle=True)
    n_steps = 4 * nsub
    want, bound = 0.3 ** 2 + 0.2 ** 2, 16 * n_steps * U
    worst = {k: np.max(np.abs(v / want - 1)) for k, v in (("disp2", r["disp"] ** 2), ("action", r["action"]), ("len2", r["len"] ** 2))}
    print("constant field, relative errors / 2^-53:", {k: v / U for k, v in worst.items()}, "allowed", 16 * n_steps,
          "| detour_max / 2^-53:", r["detour_max"] / U)
    assert r["n_clamped"] == 0 and r["n_still"] == 0 and r["n"] == 200
    assert all(v <= bound for v in worst.values())
    assert 0.0 <= r["detour_max"] <= bound
    for k in ("cost_map", "cost_length", "cost_action"):
        assert abs(r[k] / want - 1) <= bound + 200 * 2 * U                # the mean of 200 such values
    assert r["mass"] == 200.0 and r["detour_over"] == 0


def _rotation_errors(nt, nsub, direction):
    """The discrete path in a rigid rotation by theta = pi / 2 is (up to RK4's error) a regular polygon of N = (nt - 1) nsub
    chords on the circle of radius r"""
    out = _rotation_out(nt=nt)
    x0, y0 = _ring_seeds()
    r = np.hypot(x0 - 0.5, y0 - 0.5)
    rep = A.map_report(out, x0, y0, nsub=nsub, direction=direction, rho_floor=0.5, per_particle=True)
    N, th = (nt - 1) * nsub, np.pi / 2
    length = 2 * r * N * np.sin(th / (2 * N))
    err = dict(len=np.max(np.abs(rep["len"] - length)), action=np.max(np.abs(rep["action"] - length ** 2)),
               disp=np.max(np.abs(rep["disp"] - 2 * r * np.sin(th / 2))),
               detour=abs(rep["detour_max"] - (1 - np.sin(th / 2) / (N * np.sin(th / (2 * N))))))
    assert rep["n_clamped"] == 0 and rep["n_still"] == 0
    return err


@pytest.mark.parametrize("direction", [1, -1])
def test_rigid_rotation(direction):
    errs = {}
    for nt in (9, 17, 33):
        bound = _rk4_bound(nt, 1)
        errs[nt] = _rotation_errors(nt, 1, direction)
        print("rotation, direction %+d, nt %d:" % (direction, nt), {k: "%.2e" % v for k, v in errs[nt].items()}, "bound %.2e" % bound)
        assert all(v <= 2 * bound for v in errs[nt].values()), (nt, errs[nt], bound)
    print("len error nt 9 / nt 17: %.1f (fourth order: 16)" % (errs[9]["len"] / errs[17]["len"]))
    assert errs[9]["len"] > 8 * errs[17]["len"]
    e2 = _rotation_errors(9, 2, direction)
    assert all(v <= 2 * _rk4_bound(9, 2) for v in e2.values()), e2


def _rough_out(ny, nx, nt, seed):
    """rho mostly in [0.5, 1.5] with exact zeros and negative entries, E a smooth shear plus noise with |E / rho| up to
    about 0.5 (the kind of state tests/test_gpu_map_report.py uploads); ny None: 1-D"""
    rng = np.random.default_rng(seed)
    one_d = ny is None
    shp = (nx, nt) if one_d else (ny, nx, nt)
    rho = rng.uniform(0.5, 1.5, shp)
    flat = rho.reshape(-1)
    flat[rng.integers(0, flat.size, 4)] = (0.0, 0.0, -0.3, -0.7)
    gx = np.arange(nx) / float(nx - 1)
    if one_d:
        return dict(rho=rho, Ex=0.22 * np.sin(4 * np.pi * gx + 0.2)[:, None] + 0.05 * rng.uniform(-1, 1, shp))
    gy = np.arange(ny) / float(ny - 1)
    Ex = 0.22 * np.sin(2 * np.pi * gy + 0.3)[:, None, None] + 0.05 * rng.uniform(-1, 1, shp)
    Ey = 0.22 * np.cos(2 * np.pi * gx + 0.1)[None, :, None] + 0.05 * rng.uniform(-1, 1, shp)
    return dict(rho=rho, Ex=Ex, Ey=Ey)


def _seeds(n, one_d, seed=3):
    rng = np.random.default_rng(seed)
    x = np.concatenate([[0.0, 1.0, -0.2, 1.5, 0.5], rng.uniform(0, 1, n - 5)])
    return x, (None if one_d else np.concatenate([[0.0, 1.0, 0.4, 0.5, 1.0], rng.uniform(0, 1, n - 5)]))


@pytest.mark.parametrize("shape,nsub", [((19, 13, 7), 1), ((16, 12, 9), 4), ((None, 33, 9), 2), ((11, 9, 17), 2)])
@pytest.mark.parametrize("direction", [1, -1])
def test_chain(shape, nsub, direction):
    """disp^2 <= len^2 (triangle inequality) <= action (Cauchy-Schwarz over N steps of equal duration), particle by
    particle, up to the rounding of N additions: eps = 4 N 2^-52"""
    out = _rough_out(*shape, seed=11)
    x, y = _seeds(300, shape[0] is None)
    r = A.map_report(out, x, y, nsub=nsub, direction=direction, per_particle=True)
    N = (shape[2] - 1) * nsub
    eps = 4 * N * 2.0 ** -52
    d2, l2, act = r["disp"] ** 2, r["len"] ** 2, r["action"]
    with np.errstate(invalid="ignore", divide="ignore"):
        v1 = np.nanmax(np.where(l2 > 0, d2 / l2 - 1, 0.0))
        v2 = np.nanmax(np.where(act > 0, l2 / act - 1, 0.0))
    print("chain, N = %d: worst relative violation %.1e, %.1e (allowed %.1e); detour_max %.3f, %d still, %d clamped"
          % (N, max(v1, 0), max(v2, 0), eps, r["detour_max"], r["n_still"], r["n_clamped"]))
    assert np.all(d2 <= l2 * (1 + eps)) and np.all(l2 <= act * (1 + eps))
    assert r["cost_map"] <= r["cost_length"] * (1 + eps) and r["cost_length"] <= r["cost_action"] * (1 + eps)
    assert np.all(r["len"] >= 0) and 0.0 <= r["detour_max"] < 1.0
    assert r["detour_hist"].sum() + r["detour_over"] <= r["n"]
    edges = R.report_edges()
    det = np.where(r["len"] > 0, np.maximum(1 - r["disp"] / np.where(r["len"] > 0, r["len"], 1.0), 0.0), 0.0)
    assert r["detour_over"] == np.count_nonzero(det > edges[-1])
    assert r["detour_hist"].sum() == np.count_nonzero((det >= edges[0]) & (det <= edges[-1]))


def test_walls_and_masks():
    # a field pointing into the wall x = 1: every particle arrives (v = 2) and is held there
    out = _const_out(6, 5, 3, 2.0, 0.0)
    x0, y0 = np.linspace(0.3, 0.9, 50), np.linspace(0.0, 1.0, 50)
    for nsub in (1, 2):
        r = A.map_report(out, x0, y0, nsub=nsub, rho_floor=0.25, per_particle=True)
        n_steps = 2 * nsub
        assert r["n_clamped"] == 50 and np.all(r["x"] == 1.0)
        assert np.all(np.abs(r["disp"] - (1.0 - x0)) <= 4 * n_steps * U)
        assert np.all(np.abs(r["len"] - (1.0 - x0)) <= 4 * n_steps * U)     # pressed against the wall: nothing is added
        assert r["n_still"] == 0 and r["detour_max"] <= 8 * n_steps * U / 0.1 + 2 * U      # the shortest path is 0.1 long
    # rho <= floor everywhere: nothing moves
    out = _const_out(6, 5, 3, 2.0, -1.0)
    out["rho"][...] = 0.25
    r = A.map_report(out, x0, y0, rho_floor=0.25, per_particle=True)
    assert r["n_still"] == 50 and r["n_clamped"] == 0
    assert np.all(r["len"] == 0.0) and np.all(r["disp"] == 0.0) and np.all(r["action"] == 0.0)
    assert r["detour_max"] == 0.0 and r["detour_hist"].sum() == 0 and r["detour_over"] == 0
    assert r["cost_map"] == 0.0 and r["cost_action"] == 0.0
    # a masked patch holds the particles seeded in it, the others move
    out = _const_out(9, 9, 3, 0.1, 0.0)
    out["rho"][:, :3, :] = 0.0
    x, y = np.array([0.1, 0.2, 0.6]), np.array([0.5, 0.5, 0.5])
    r = A.map_report(out, x, y, rho_floor=0.25, per_particle=True)
    assert r["n_still"] == 2 and np.array_equal(r["len"] == 0.0, [True, True, False])


def test_masses_are_checked():
    out = _const_out(6, 5, 3, 0.1, 0.0)
    x, y = np.array([0.1, 0.2, 0.6]), np.array([0.5, 0.5, 0.5])
    for bad in ([1.0, -1e-300, 1.0], [1.0, np.nan, 1.0], [np.inf, 1.0, 1.0], [0.0, 0.0, 0.0], [1.0, 1.0]):
        with pytest.raises(ValueError):
            A.map_report(out, x, y, mass=bad, rho_floor=0.5)
    ones, none = A.map_report(out, x, y, mass=np.ones(3), rho_floor=0.5), A.map_report(out, x, y, rho_floor=0.5)
    assert all(ones[k] == none[k] for k in SUMS)
    # a zero mass takes its particle out of the means, not out of the maxima
    far = A.map_report(_const_out(6, 5, 3, 0.1, 0.0), x, y, mass=[1.0, 1.0, 0.0], rho_floor=0.5, per_particle=True)
    assert far["mass"] == 2.0 and far["disp_max"] == far["disp"].max()


def test_particle_order():
    out = _rough_out(19, 13, 7, seed=5)
    n = 700                                                                # three blocks, the last one ragged
    x, y = _seeds(n, False)
    rng = np.random.default_rng(8)
    mass = rng.uniform(0, 2, n)
    mass[[3, n // 2]] = 0.0
    a = A.map_report(out, x, y, mass=mass, nsub=2, per_particle=True)
    perm = rng.permutation(n)
    b = A.map_report(out, x[perm], y[perm], mass=mass[perm], nsub=2, per_particle=True)
    for k in ("disp", "len", "action", "x", "y"):
        assert a[k][perm].tobytes() == b[k].tobytes(), k
    for k in ("n", "n_clamped", "n_still", "detour_over", "disp_max", "len_max", "detour_max"):
        assert a[k] == b[k], k
    assert np.array_equal(a["detour_hist"], b["detour_hist"])
    terms = lambda r, m: (m, m * r["disp"] ** 2, m * r["len"] ** 2, m * r["action"], m * r["disp"], m * r["len"])   # noqa: E731
    for ta, tb in zip(terms(a, mass), terms(b, mass[perm])):
        sa, sb = A._tree_sum(ta), A._tree_sum(tb)
        assert abs(sa - sb) <= n * 2.0 ** -52 * sa
        assert abs(sa - float(np.sum(ta))) <= n * 2.0 ** -52 * sa       # and the tree is a sum
    assert a["mass"] == A._tree_sum(mass) and b["mass"] == A._tree_sum(mass[perm])
    assert a["len_mean"] == A._tree_sum(mass * a["len"]) / a["mass"]
    assert a["disp_mean"] == A._tree_sum(mass * a["disp"]) / a["mass"]
    assert a["cost_action"] == A._tree_sum(mass * a["action"]) / a["mass"]


@pytest.mark.parametrize("n", [1, 64, 65, 256, 257, 4097, 65537])
def test_tree_sum(n):
    """the fixed tree is a sum: exact on integers, whatever the raggedness of the last wavefront, block and row of blocks"""
    t = np.arange(1, n + 1, dtype=np.float64)
    assert A._tree_sum(t) == n * (n + 1) / 2


@functools.lru_cache(maxsize=None)
def _oracle_1d():
    rho0, rho1, nt, x0, target = gaussian_1d_problem()
    var, model, hist, sigma = OD.solve_single_level(rho0, rho1, nt, dict(tol=1e-5, maxit=8000))
    rho, Ex = OD.recover_RhoE_1d(var, model)
    return dict(rho=rho, Ex=Ex), rho0, x0, target


@functools.lru_cache(maxsize=None)
def _oracle_2d():
    rho0, rho1, nt, x0, y0, tx, ty = gaussian_2d_problem()
    var, model, hist, sigma = OD.solve_single_level(rho0, rho1, nt, dict(tol=1e-4, maxit=8000))
    rho, Ex, Ey = OD.recover_RhoE(var, model)
    return dict(rho=rho, Ex=Ex, Ey=Ey), rho0, x0, y0


def _eulerian_cost(out):
    cells = out["rho"].shape[:-1] + (out["rho"].shape[-1] - 1,)
    z = {k: np.zeros(cells) for k in (("q0", "bx") if "Ey" not in out else ("q0", "bx", "by"))}
    return R.solution_report(dict(out, **z))["cost"]


def _say(name, r, out):
    print("%s: cost_map %.6f <= cost_length %.6f <= cost_action %.6f | Eulerian cost %.6f | detour_max %.2e, %d clamped"
          % (name, r["cost_map"], r["cost_length"], r["cost_action"], _eulerian_cost(out), r["detour_max"], r["n_clamped"]))


def test_anchor_gaussians_on_the_line():
    """T(x) = 0.7 + 0.5 (x - 0.3): every seed's displacement is within half a cell of |T(x) - x| (the map error bound of
    tests/test_advect_host.py, by the triangle inequality)"""
    out, rho0, x0, target = _oracle_1d()
    cell = 1.0 / (rho0.size - 1)
    for nsub in (1, 2):
        mass = np.interp(x0, np.arange(rho0.size) * cell, rho0)
        r = A.map_report(out, x0, mass=mass, nsub=nsub, per_particle=True)
        err = np.max(np.abs(r["disp"] - np.abs(target - x0)))
        _say("1-D anchor, nsub %d, worst |disp - |T(x) - x|| = %.2f cells" % (nsub, err / cell), r, out)
        assert err <= 0.5 * cell
        eps = 4 * 32 * nsub * 2.0 ** -52
        assert r["cost_map"] <= r["cost_length"] * (1 + eps) and r["cost_length"] <= r["cost_action"] * (1 + eps)


def test_anchor_translation_in_the_plane():
    """the translation by (0.2, 0.3): |T(x) - x|^2 = 0.13 = W2^2 for every seed"""
    out, rho0, x0, y0 = _oracle_2d()
    cell = 1.0 / 32
    mass = rho0[np.rint(y0 * 32).astype(int), np.rint(x0 * 32).astype(int)]
    for nsub in (1, 2):
        r = A.map_report(out, x0, y0, mass=mass, nsub=nsub, per_particle=True)
        err = np.max(np.abs(r["disp"] - np.sqrt(0.13)))
        _say("2-D anchor, nsub %d, worst |disp - sqrt(0.13)| = %.2f cells" % (nsub, err / cell), r, out)
        assert err <= 0.5 * cell
        assert abs(np.sqrt(r["cost_map"]) - np.sqrt(0.13)) <= 0.5 * cell
        eps = 4 * 16 * nsub * 2.0 ** -52
        assert r["cost_map"] <= r["cost_length"] * (1 + eps) and r["cost_length"] <= r["cost_action"] * (1 + eps)
