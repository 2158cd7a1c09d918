"""The numpy twin of the particle transport (dot-socp_amd/advect.py) on its own: fields with known flows, the layout of
the trajectories, the masking rule, and two anchors on the CPU oracle's solutions whose transport maps are known in closed
form -- independent of the device code, which tests/test_gpu_advect.py holds to this twin bit for bit."""
import numpy as np
import pytest

import dotsocp_amd as D
from dotsocp_amd import advect as A
from oracle import driver as OD
from oracle.examples import get_example_1d

U = 2.0 ** -53


def _const_out(ny, nx, nt, ex, ey):
    shp = (ny, nx, nt)
    return dict(rho=np.ones(shp, order="F"), Ex=np.full(shp, ex, order="F"), Ey=np.full(shp, ey, order="F"))


def _rotation_out(n=17, nt=9, omega=np.pi / 2):
    g = np.arange(n) / float(n - 1)
    Y, X = np.meshgrid(g, g, indexing="ij")                              # arrays are (ny, nx)
    one = np.ones(nt)
    return dict(rho=np.ones((n, n, nt)), Ex=(-omega * (Y - 0.5))[:, :, None] * one, Ey=(omega * (X - 0.5))[:, :, None] * one)


def _ring_seeds():
    """within radius 0.3 of the centre (the largest radius is 0.29)"""
    r = np.repeat([0.05, 0.13, 0.21, 0.29], 16)
    th = np.tile(np.arange(16) * (2 * np.pi / 16) + 0.1, 4)
    return 0.5 + r * np.cos(th), 0.5 + r * np.sin(th)


def test_exports():
    assert D.advect is A and D.default_rho_floor is A.default_rho_floor and D.seeds_on_nodes is A.seeds_on_nodes
    assert A.default_rho_floor(np.array([1.0, 3.0]), np.array([2.0, 0.5])) == 3.0 / 100


@pytest.mark.parametrize("nsub", [1, 2])
def test_constant_field(nsub):
    out = _const_out(9, 7, 5, 0.3, -0.2)
    rng = np.random.default_rng(1)
    x0, y0 = rng.uniform(0.05, 0.65, 200), rng.uniform(0.25, 0.95, 200)           # no clamp fires
    r = A.advect(out, x0, y0, nsub=nsub, rho_floor=0.5)
    n_steps = 4 * nsub
    ex, ey = np.max(np.abs(r["x"] - (x0 + 0.3))), np.max(np.abs(r["y"] - (y0 - 0.2)))
    print("constant field: worst error / 2^-53 =", ex / U, ey / U, "allowed", 4 * n_steps)
    assert r["n_clamped"] == 0
    assert ex <= 4 * n_steps * U and ey <= 4 * n_steps * U


def _rk4_bound(nt, nsub, omega=np.pi / 2, r=0.3):
    """Bilinear interpolation of an affine field is exact, so the error is RK4's: per step the stability polynomial
    differs from exp(i omega dt) by (omega dt)^5 / 120 (relative to the radius), n_steps steps add up; plus the rounding
    of n_steps steps of about 40 operations each on numbers below 1."""
    n_steps = (nt - 1) * nsub
    dt = 1.0 / n_steps
    return n_steps * (omega * dt) ** 5 / 120 * r + 40 * n_steps * U


def test_rigid_rotation_and_its_inverse():
    out = _rotation_out()
    x0, y0 = _ring_seeds()
    assert np.max(np.hypot(x0 - 0.5, y0 - 0.5)) <= 0.3
    fwd = A.advect(out, x0, y0, nsub=4, rho_floor=0.5)
    bound = _rk4_bound(9, 4)
    xe, ye = 0.5 - (y0 - 0.5), 0.5 + (x0 - 0.5)                          # a quarter turn
    err = np.max(np.hypot(fwd["x"] - xe, fwd["y"] - ye))
    print("rotation: error %.3e, bound %.3e, ratio %.3f" % (err, bound, err / bound))
    assert fwd["n_clamped"] == 0 and err <= bound
    back = A.advect(out, fwd["x"], fwd["y"], nsub=4, direction=-1, rho_floor=0.5)
    err2 = np.max(np.hypot(back["x"] - x0, back["y"] - y0))
    print("there and back: error %.3e, bound %.3e, ratio %.3f" % (err2, 2 * bound, err2 / (2 * bound)))
    assert err2 <= 2 * bound


@pytest.mark.parametrize("direction", [1, -1])
def test_trajectory_layout(direction):
    out = _rotation_out()
    x0, y0 = _ring_seeds()
    x0, y0 = np.append(x0, [-0.25, 1.5]), np.append(y0, [0.5, 2.0])      # two seeds outside the square
    r = A.advect(out, x0, y0, nsub=2, direction=direction, rho_floor=0.5, trajectories=True)
    first, last = (0, -1) if direction > 0 else (-1, 0)
    assert r["traj_x"].shape == (x0.size, 9) and r["traj_y"].shape == (x0.size, 9)
    assert np.array_equal(r["traj_x"][:, first], np.clip(x0, 0, 1)) and np.array_equal(r["traj_y"][:, first], np.clip(y0, 0, 1))
    assert np.array_equal(r["traj_x"][:, last], r["x"]) and np.array_equal(r["traj_y"][:, last], r["y"])
    plain = A.advect(out, x0, y0, nsub=2, direction=direction, rho_floor=0.5)
    assert plain["traj_x"] is None and plain["traj_y"] is None
    assert plain["x"].tobytes() == r["x"].tobytes() and plain["y"].tobytes() == r["y"].tobytes()
    assert plain["n_clamped"] == r["n_clamped"]


def test_one_dimensional_outputs():
    nx, nt = 11, 4
    out = dict(rho=np.ones((nx, nt)), Ex=np.full((nx, nt), 0.25))
    x0 = np.linspace(0.0, 0.7, 15)
    r = A.advect(out, x0, nsub=3, rho_floor=0.5, trajectories=True)
    assert r["y"] is None and r["traj_y"] is None and r["traj_x"].shape == (15, nt)
    assert np.max(np.abs(r["x"] - (x0 + 0.25))) <= 4 * 9 * U and r["n_clamped"] == 0
    with pytest.raises(ValueError):
        A.advect(out, x0, x0)                                             # y on 1-D outputs
    assert set(A.velocity(out, 0.5)) == {"vx"}


def test_masking_and_clamp_count():
    out = _const_out(6, 5, 3, 2.0, 0.0)
    floor = 0.25
    out["rho"][1, 1, 0], out["rho"][2, 1, 0], out["rho"][3, 1, 0], out["rho"][4, 1, 0] = 0.0, np.nan, floor, -1.0
    out["rho"][1, 2, 1] = np.nextafter(floor, 1.0)
    out["Ex"][0, 0, 2], out["rho"][0, 0, 2] = np.inf, 1.0                 # a quotient that is not finite
    v = A.velocity(out, floor)
    assert np.all(np.isfinite(v["vx"])) and np.all(np.isfinite(v["vy"]))
    assert np.all(v["vx"][1:5, 1, 0] == 0.0) and v["vx"][0, 0, 2] == 0.0
    assert v["vx"][1, 2, 1] == 2.0 / np.nextafter(floor, 1.0)             # just above the floor: kept
    assert np.count_nonzero(v["vx"] == 0.0) == 5 and np.all(v["vy"] == 0.0)
    # every particle is pushed through x = 1 (v = 2 almost everywhere) and stays there for several steps: counted once
    x0, y0 = np.linspace(0.3, 0.9, 50), np.linspace(0.0, 1.0, 50)
    r = A.advect(out, x0, y0, nsub=2, rho_floor=floor)
    assert r["n_clamped"] == 50 and np.all(r["x"] == 1.0)
    still = A.advect(_const_out(6, 5, 3, 0.0, 0.0), x0, y0, rho_floor=floor)
    assert still["n_clamped"] == 0 and np.array_equal(still["x"], x0) and np.array_equal(still["y"], y0)
    half = A.advect(_const_out(6, 5, 3, 0.5, 0.0), x0, y0, rho_floor=floor)
    assert half["n_clamped"] == np.count_nonzero(x0 + 0.5 > 1.0 + 1e-12) == 33
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            A.advect(out, np.array([0.5, bad]), np.array([0.5, 0.5]), rho_floor=floor)
        with pytest.raises(ValueError):
            A.advect(out, np.array([0.5, 0.5]), np.array([bad, 0.5]), rho_floor=floor)
    for kw in (dict(nsub=0), dict(direction=0)):
        with pytest.raises(ValueError):
            A.advect(out, x0, y0, rho_floor=floor, **kw)


def test_seeds_on_nodes():
    x, y = A.seeds_on_nodes(5, 3)
    assert x.size == 15 and np.array_equal(y[:3], [0.0, 0.5, 1.0]) and np.all(x[:3] == 0.0)       # y fastest
    x, y = A.seeds_on_nodes(9, 5, stride=4)
    assert np.array_equal(x, [0, 0, 0.5, 0.5, 1, 1]) and np.array_equal(y, [0, 1, 0, 1, 0, 1])
    mask = np.zeros((5, 9), dtype=bool)
    mask[4, 8] = mask[1, 4] = True
    x, y = A.seeds_on_nodes(9, 5, stride=4, mask=mask)
    assert np.array_equal(x, [1.0]) and np.array_equal(y, [1.0])
    x, y = A.seeds_on_nodes(9, mask=np.arange(9) % 2 == 0, stride=2)
    assert y is None and np.array_equal(x, np.arange(0, 9, 2) / 8.0)


# ---- anchors: the oracle's solutions of two problems whose transport map is known ----
def gaussian_1d_problem():
    """the reference's 1-D example: N(0.3, 0.1^2) -> N(0.7, 0.05^2), T(x) = 0.7 + 0.5 (x - 0.3)"""
    rho0, rho1 = get_example_1d("gaussian", 129)
    x0 = np.linspace(0.1, 0.5, 41)
    return rho0, rho1, 33, x0, 0.7 + 0.5 * (x0 - 0.3)


def gaussian_2d_problem():
    """two equal Gaussians, s = 0.1, centres (cy, cx) = (0.35, 0.4) -> (0.65, 0.6): the map is the translation; seeds:
    the nodes within 2 s of the start centre"""
    n, s = 33, 0.1
    g = np.arange(n) / float(n - 1)
    Y, X = np.meshgrid(g, g, indexing="ij")

    def bump(cy, cx):
        b = np.exp(-0.5 * (((Y - cy) / s) ** 2 + ((X - cx) / s) ** 2))
        return b / b.mean()

    x0, y0 = A.seeds_on_nodes(n, n, mask=np.hypot(Y - 0.35, X - 0.4) <= 2 * s)
    return bump(0.35, 0.4), bump(0.65, 0.6), 17, x0, y0, x0 + 0.2, y0 + 0.3


def test_anchor_gaussians_on_the_line():
    rho0, rho1, nt, x0, target = gaussian_1d_problem()
    var, model, hist, sigma = OD.solve_single_level(rho0, rho1, nt, dict(tol=1e-5, maxit=8000))
    rho, Ex = OD.recover_RhoE_1d(var, model)
    cell = 1.0 / (rho0.size - 1)
    for nsub in (1, 2):
        r = A.advect(dict(rho=rho, Ex=Ex), x0, nsub=nsub)
        err = np.max(np.abs(r["x"] - target))
        print("1-D anchor, nsub %d: worst map error %.4f = %.2f cells, %d clamped" % (nsub, err, err / cell, r["n_clamped"]))
        assert err <= 0.5 * cell


def test_anchor_translation_in_the_plane():
    rho0, rho1, nt, x0, y0, tx, ty = gaussian_2d_problem()
    assert x0.size == 129
    var, model, hist, sigma = OD.solve_single_level(rho0, rho1, nt, dict(tol=1e-4, maxit=8000))
    rho, Ex, Ey = OD.recover_RhoE(var, model)
    cell = 1.0 / 32
    for nsub in (1, 2):
        r = A.advect(dict(rho=rho, Ex=Ex, Ey=Ey), x0, y0, nsub=nsub)
        err = np.max(np.hypot(r["x"] - tx, r["y"] - ty))
        print("2-D anchor, nsub %d: worst map error %.4f = %.2f cells, %d clamped" % (nsub, err, err / cell, r["n_clamped"]))
        assert err <= 0.5 * cell
