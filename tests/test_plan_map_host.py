"""The numpy twin of the plan's transport map (upper.barycentric_map, upper.plan_frames) on its own: against the dense
n x n plan it stands for, the identity upper = map cost + spread, a translation, a monotone 1-D map, and the frames.

The map is the barycentric projection T(x_i) = E[y | x_i] of the rounded plan P + er ec^T / fill of upper.sinkhorn_round:
the softmax weights of the last rounding transform f^ = S(lb - g') are the conditional law of the kept part, the rank-one
fill has closed-form moments."""
import functools

import numpy as np
import pytest

from dotsocp_amd import advect
from dotsocp_amd import upper as U


def _nodes(shape):
    """(x, y) of the nodes, flat, y fastest (a line: y = 0)"""
    if len(shape) == 1:
        return np.arange(shape[0]) / float(shape[0] - 1), np.zeros(shape[0])
    yy, xx = np.meshgrid(np.arange(shape[0]) / float(shape[0] - 1), np.arange(shape[1]) / float(shape[1] - 1), indexing="ij")
    return xx.ravel(order="F"), yy.ravel(order="F")


def dense_map(ub, rho0, rho1):
    """Dx, Dy, C, row of the n x n plan rebuilt from the arrays of an UpperBound (flat, y fastest); a line: Dy = 0"""
    shape = np.shape(rho0)
    P = U.plan_dense(ub["f"], ub["g"], ub["er"], ub["ec"], rho0, rho1, ub["eps"])
    x, y = _nodes(shape)
    row = P.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        Dx = np.where(row > 0, (P @ x) / row - x, 0.0)
        Dy = np.where(row > 0, (P @ y) / row - y, 0.0)
        C = np.where(row > 0, (P * U.pair_cost(shape)).sum(axis=1) / row, 0.0)
    return Dx, Dy, C, row


def check_against_dense(m, ub, rho0, rho1, tol=1e-11):
    shape = np.shape(rho0)
    Dx, Dy, C, row = dense_map(ub, rho0, rho1)
    flat = lambda t: np.ravel(t, order="F")                                          # noqa: E731
    pairs = [("C", C, m["C"]), ("row", row, m["row"])]
    pairs += [("Dx", Dx, m["Dx"])] if len(shape) == 1 else [("Dx", Dx, m["Dx"]), ("Dy", Dy, m["Dy"])]
    for name, want, got in pairs:
        d = float(np.max(np.abs(flat(got) - want)))
        print("  %-4s %s  max distance from the dense plan %.3e" % (name, shape, d))
        assert d <= tol, (name, d)


def check_identity(m, tol=1e-11):
    up = m["upper"]["upper"]
    print("  upper %.15g cost_rows %.15g map_cost + spread %.15g rows - 1 %.3e" %
          (up, m["cost_rows"], m["map_cost"] + m["spread"], m["rows"] - 1.0))
    assert abs(m["cost_rows"] - up) <= tol * up
    assert abs(m["map_cost"] + m["spread"] - m["cost_rows"]) <= tol * up
    assert abs(m["rows"] - 1.0) <= 1e-12


def _random_pair(shape, seed):
    rng = np.random.default_rng(seed)
    rho0, rho1 = rng.uniform(0.5, 1.5, shape), rng.uniform(0.5, 1.5, shape)
    rho0.flat[3] = 0.0
    rho1.flat[5] = 0.0
    eps = float(U._eps(shape, 0.25, np.float64))
    return rho0, rho1, eps * rng.uniform(-2.0, 2.0, shape), eps * rng.uniform(-2.0, 2.0, shape)


@pytest.mark.parametrize("shape", [(9, 9), (13, 17), (33,)], ids=str)
def test_against_the_dense_plan(shape):
    """random potentials f, g (no sweep): the rounding makes a feasible plan of any pair, the map is that plan's"""
    rho0, rho1, f, g = _random_pair(shape, 50 + sum(shape))
    ub = U.sinkhorn_round(rho0, rho1, f, 0.25, 0, g_start=g)
    m = U.barycentric_map(ub, rho0, rho1)
    assert ub["fill"] > 1e-3                    # the fill carries weight here: its closed-form moments are tested too
    check_against_dense(m, ub, rho0, rho1)
    check_identity(m)
    assert np.all(m["row"][rho0 == 0] == 0) and np.all(m["C"][rho0 == 0] == 0) and np.all(m["Dx"][rho0 == 0] == 0)
    # the value and the mean cost of the moment flavour carry the bits of the plain transform
    t = rho0 - rho1
    plain, mom = U.soft_transform(t, ub["eps"]), U._soft_moments(t, np.float64(ub["eps"]), np.float64)
    assert np.array_equal(plain[0], mom[0]) and np.array_equal(plain[1], mom[1])


def test_identity_after_sweeps():
    rho0, rho1, f, _ = _random_pair((17, 21), 7)
    ub = U.sinkhorn_round(rho0, rho1, f, 0.25, 10)
    check_identity(U.barycentric_map(ub, rho0, rho1))


def translation_case():
    """17 x 21: a cos^2 bump of radius 4.5 nodes plus 0.05 inside the radius, zero outside; rho1 the same bump shifted by
    (3, 7) nodes along (y, x)"""
    ny, nx, R, sy, sx = 17, 21, 4.5, 3, 7
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")

    def bump(cy, cx):
        r = np.hypot(yy - cy, xx - cx)
        return np.where(r < R, np.cos(0.5 * np.pi * r / R) ** 2 + 0.05, 0.0)
    return bump(6, 6), bump(6 + sy, 6 + sx), (sy / float(ny - 1), sx / float(nx - 1))


def check_translation(m, rho0, shift):
    """mass-weighted mean of |D - shift| <= 0.25 h per axis, maximum over the support <= 1 h, map_cost within 1 % of |s|^2"""
    ny, nx = rho0.shape
    a = rho0 / rho0.sum()
    on = rho0 > 0
    for name, D, s, h in (("y", m["Dy"], shift[0], 1.0 / (ny - 1)), ("x", m["Dx"], shift[1], 1.0 / (nx - 1))):
        err = np.abs(np.asarray(D, dtype=np.float64) - s)
        mean, worst = float((a * err).sum()) / h, float(err[on].max()) / h
        print("  translation along %s: mean |D - shift| %.3f h, max %.3f h" % (name, mean, worst))
        assert mean <= 0.25 and worst <= 1.0
    s2 = shift[0] ** 2 + shift[1] ** 2
    print("  map_cost %.9g |s|^2 %.9g relative %.2e" % (m["map_cost"], s2, abs(m["map_cost"] - s2) / s2))
    assert abs(m["map_cost"] - s2) <= 0.01 * s2


def test_translation():
    rho0, rho1, shift = translation_case()
    ub = U.sinkhorn_round(rho0, rho1, None, 0.25, 200)
    check_translation(U.barycentric_map(ub, rho0, rho1), rho0, shift)


@functools.lru_cache(maxsize=None)
def monotone_case():
    """129 nodes, Gaussians (0.3, 0.08) and (0.65, 0.12), each plus 0.01; T_exact: the barycentric map of the north-west-corner
    plan (the monotone, optimal one); the start: minus the integrated exact displacement (trapezoidal rule)"""
    n = 129
    x = np.arange(n) / float(n - 1)
    rho0 = np.exp(-0.5 * ((x - 0.3) / 0.08) ** 2) + 0.01
    rho1 = np.exp(-0.5 * ((x - 0.65) / 0.12) ** 2) + 0.01
    a, b = rho0 / rho0.sum(), rho1 / rho1.sum()
    T = np.zeros(n)
    i = j = 0
    ra, rb = a[0], b[0]
    moved = np.zeros(n)
    while i < n and j < n:
        t = min(ra, rb)
        T[i] += t * x[j]
        moved[i] += t
        ra, rb = ra - t, rb - t
        if ra <= 0.0:
            i += 1
            ra = a[i] if i < n else 0.0
        if rb <= 0.0:
            j += 1
            rb = b[j] if j < n else 0.0
    T = T / moved
    d = T - x
    f = -np.concatenate([[0.0], np.cumsum(0.5 * (d[1:] + d[:-1]))]) / float(n - 1)
    return rho0, rho1, f, T


def check_monotone(m, T_exact):
    n = T_exact.size
    x = np.arange(n) / float(n - 1)
    T = x + np.asarray(m["Dx"], dtype=np.float64)
    err = np.abs(T - T_exact) * (n - 1)
    print("  1-D: mean |T - T_exact| %.3f h, max %.3f h, smallest step of T %.3e" % (err.mean(), err.max(), np.diff(T).min()))
    assert np.all(np.diff(T) >= 0.0)
    assert err.mean() <= 0.1 and err.max() <= 1.0


def test_monotone_map_on_a_line():
    rho0, rho1, f, T_exact = monotone_case()
    assert abs(T_exact[0]) < 0.05 and abs(T_exact[-1] - 1.0) < 0.05 and np.all(np.diff(T_exact) >= -1e-15)
    ub = U.sinkhorn_round(rho0, rho1, f, 0.25, 100)
    check_monotone(U.barycentric_map(ub, rho0, rho1), T_exact)


def test_frames():
    rng = np.random.default_rng(3)
    shape = (11, 14)
    rho0 = rng.uniform(0.5, 1.5, shape)
    rho0[4, :] = 0.0
    rho0[7, 9] = 0.0
    Dx, Dy = rng.uniform(-0.2, 0.2, shape), rng.uniform(-0.2, 0.2, shape)
    fr = U.plan_frames(rho0, Dx, Dy, [0.0, 0.5, 1.0, 0.5])
    unit = advect.mass_unit(rho0.size, rho0.max())
    M = np.rint(rho0 / unit).astype(np.int64)
    assert fr["unit"] == unit and fr["total_units"] == int(M.sum())
    assert np.array_equal(fr["counts"][..., 0], M) and np.array_equal(fr["frames"][..., 0], M.astype(np.float64) * unit)
    assert all(int(fr["counts"][..., k].sum()) == int(M.sum()) for k in range(4))
    assert np.array_equal(fr["counts"][..., 1], fr["counts"][..., 3]) and not np.array_equal(fr["counts"][..., 1], fr["counts"][..., 2])
    # a node without mass moves nothing, however far its displacement points
    far = Dx.copy()
    far[7, 9] = 5.0
    again = U.plan_frames(rho0, far, Dy, [0.0, 0.5, 1.0, 0.5])
    assert np.array_equal(again["counts"], fr["counts"]) and again["n_clamped"] == fr["n_clamped"]
    # pushed against a wall: every node with mass in the last three columns is clamped, each counted once
    wall = np.full(shape, 0.2)
    got = U.plan_frames(rho0, wall, np.zeros(shape), [1.0, 0.0, 1.0])
    assert got["n_clamped"] == int(np.count_nonzero(rho0[:, -3:] > 0))
    assert int(got["counts"][..., 0].sum()) == int(M.sum())
    # a line
    line = U.plan_frames(rho0[:, 2], Dy[:, 2], None, [0.0, 1.0])
    assert np.array_equal(line["counts"][:, 0], np.rint(rho0[:, 2] / line["unit"]).astype(np.int64))
    assert int(line["counts"][:, 1].sum()) == line["total_units"]
    with pytest.raises(ValueError):
        U.plan_frames(rho0, Dx, Dy, [1.5])
