"""The numpy twin of the mass push-forward (dot-socp_amd/advect.py: push_forward, masses_on_nodes) on its own: exact
conservation, independence of the particle order, two closed forms (a constant field in exact arithmetic, a rigid
rotation that converges), the corner cases of the integer split and the refused arguments -- independent of the device
code, which tests/test_gpu_push.py holds to this twin bit for bit."""
import math

import numpy as np
import pytest

import dotsocp_amd as D
from dotsocp_amd import advect as A


def test_exports_and_masses_pair_with_seeds():
    assert D.push_forward is A.push_forward and D.masses_on_nodes is A.masses_on_nodes
    ny, nx = 5, 9
    rho = np.arange(ny * nx, dtype=np.float64).reshape(ny, nx)
    g = lambda n: np.arange(n) / float(n - 1)                             # noqa: E731
    at = lambda x, y: rho[np.rint(y * (ny - 1)).astype(int), np.rint(x * (nx - 1)).astype(int)]      # noqa: E731
    mask = (rho % 3 == 0)
    for kw in (dict(), dict(stride=2), dict(stride=4), dict(mask=mask), dict(stride=2, mask=mask)):
        x, y = A.seeds_on_nodes(nx, ny, **kw)
        m = A.masses_on_nodes(rho, **kw)
        assert m.shape == x.shape and x.size >= 1 and np.array_equal(m, at(x, y)), kw
    assert np.array_equal(A.masses_on_nodes(rho)[:ny], rho[:, 0])         # y fastest
    line = 10.0 + np.arange(9.0)
    for kw in (dict(), dict(stride=2), dict(stride=2, mask=np.arange(9) % 4 == 0)):
        x, y = A.seeds_on_nodes(9, **kw)
        assert y is None and np.array_equal(A.masses_on_nodes(line, **kw), line[np.rint(x * 8).astype(int)]), kw
    assert np.array_equal(g(9), A.seeds_on_nodes(9)[0])


def _random_out(rng, shape):
    """finite fluxes over a density with all three mask cases of the velocity: above the floor, below it, NaN"""
    rho = rng.uniform(0.5, 1.5, shape)
    flat = rng.choice(rho.size, 12, replace=False)
    rho.flat[flat[:4]] = 0.001
    rho.flat[flat[4:8]] = -0.4
    rho.flat[flat[8:]] = np.nan
    out = dict(rho=np.asfortranarray(rho), Ex=np.asfortranarray(rng.uniform(-0.6, 0.6, shape)))
    if len(shape) == 3:
        out["Ey"] = np.asfortranarray(rng.uniform(-0.6, 0.6, shape))
    floor = 0.05
    assert np.any(rho > floor) and np.any(rho <= floor) and np.any(np.isnan(rho))
    return out, floor


def _seed_sets(rng, nx, ny):
    on = A.seeds_on_nodes(nx, ny)
    n = on[0].size
    off = (rng.uniform(0, 1, n), None if ny is None else rng.uniform(0, 1, n))
    return [("on nodes", on), ("off nodes", off)]


@pytest.mark.parametrize("shape", [(17, 13, 5), (33, 5)], ids=["2d_17x13x5", "1d_33x5"])
def test_exact_conservation(shape):
    rng = np.random.default_rng(11)
    out, floor = _random_out(rng, shape)
    one_d = len(shape) == 2
    nx, ny = (shape[0], None) if one_d else (shape[1], shape[0])
    axes = (0,) if one_d else (0, 1)
    for name, (x, y) in _seed_sets(rng, nx, ny):
        mass = rng.uniform(0.0, 2.0, x.size)
        for direction in (1, -1):
            r = A.push_forward(out, x, y, mass=mass, nsub=2, direction=direction, rho_floor=floor)
            total = r["total_units"]
            assert isinstance(total, int) and 0 < total < 2 ** 51
            assert r["counts"].dtype == np.int64 and r["counts"].shape == shape and r["frames"].shape == shape
            assert np.array_equal(r["nodes"], np.arange(shape[-1]))
            sums = r["counts"].sum(axis=axes)
            print(shape, name, "direction", direction, "units", total, "plane sums - units", sums - total)
            assert np.all(sums == total)
            assert np.all(r["frames"].sum(axis=axes) == total * r["unit"])
            assert np.array_equal(r["frames"], r["counts"] * r["unit"])
            assert r["unit"] == math.ldexp(1.0, math.frexp(x.size * mass.max())[1] - 50)
            plain = A.advect(out, x, y, nsub=2, direction=direction, rho_floor=floor)
            assert r["n_clamped"] == plain["n_clamped"] and r["x"].tobytes() == plain["x"].tobytes()
            assert one_d or r["y"].tobytes() == plain["y"].tobytes()


@pytest.mark.parametrize("shape", [(17, 13, 5), (33, 5)], ids=["2d_17x13x5", "1d_33x5"])
def test_order_independence(shape):
    rng = np.random.default_rng(12)
    out, floor = _random_out(rng, shape)
    one_d = len(shape) == 2
    n = 300
    x, y = rng.uniform(0, 1, n), (None if one_d else rng.uniform(0, 1, n))
    mass = rng.uniform(0.0, 2.0, n)
    sel = lambda a, idx: None if a is None else a[idx]                    # noqa: E731
    kw = dict(nsub=1, rho_floor=floor, frames=[0, 2, 4])
    joint = A.push_forward(out, x, y, mass=mass, **kw)
    perm = rng.permutation(n)
    shuffled = A.push_forward(out, x[perm], sel(y, perm), mass=mass[perm], **kw)
    assert shuffled["frames"].tobytes(order="F") == joint["frames"].tobytes(order="F")
    assert shuffled["counts"].tobytes(order="F") == joint["counts"].tobytes(order="F")
    assert np.array_equal(shuffled["l1"], joint["l1"], equal_nan=True)
    # two calls that share the joint set's unit: their integer planes add up to the joint plane
    unit = A.mass_unit(n, mass.max())
    assert unit == joint["unit"]
    parts = [A.push_forward(out, x[idx], sel(y, idx), mass=mass[idx], unit=unit, **kw) for idx in (perm[:110], perm[110:])]
    assert all(p["unit"] == unit for p in parts)
    assert np.array_equal(parts[0]["counts"] + parts[1]["counts"], joint["counts"])
    assert parts[0]["total_units"] + parts[1]["total_units"] == joint["total_units"]


def _split_by_hand(M, fx, fy, n):
    """the units M of one particle at the cell coordinates (fx, fy) of an n x n grid -> {(j, i): units}, with Python's own
    arithmetic and rounding (round() rounds half to even)"""
    i, j = min(int(math.floor(fx)), n - 2), min(int(math.floor(fy)), n - 2)
    a, c = fx - i, fy - j
    d00, d10, d01 = round(((1 - c) * (1 - a)) * M), round((c * (1 - a)) * M), round(((1 - c) * a) * M)
    return {(j, i): d00, (j + 1, i): d10, (j, i + 1): d01, (j + 1, i + 1): M - d00 - d10 - d01}


def test_constant_field_in_exact_arithmetic():
    """vx = 0.25, vy = -0.125 on 17 x 17 x 9: per time interval a particle moves by half a cell in x and by minus a quarter
    of a cell in y, and every operation of the march is exact (checked below on the positions).  Frame k is the initial
    plane moved by (k / 2, -k / 4) cells: a pure shift at the nodes 0, 4 and 8 (at the nodes 2 and 6 the shift in y is half
    a cell), the bilinear split worked out by hand at every node."""
    n, nt = 17, 9
    shp = (n, n, nt)
    out = dict(rho=np.ones(shp, order="F"), Ex=np.full(shp, 0.25, order="F"), Ey=np.full(shp, -0.125, order="F"))
    g = np.arange(n) / float(n - 1)
    Y, X = np.meshgrid(g, g, indexing="ij")
    blob = np.exp(-0.5 * (((Y - 0.6) / 0.08) ** 2 + ((X - 0.3) / 0.08) ** 2))
    support = (np.abs(Y - 0.6) <= 0.2) & (np.abs(X - 0.3) <= 0.2)        # rows 7 .. 12, columns 2 .. 8: stays inside
    x0, y0 = A.seeds_on_nodes(n, n, mask=support)
    mass = A.masses_on_nodes(blob, mask=support)
    assert x0.size == 42 and np.all(mass > 0)
    r = A.push_forward(out, x0, y0, mass=mass, rho_floor=0.5)
    assert r["n_clamped"] == 0
    assert np.array_equal(r["x"], x0 + 0.25) and np.array_equal(r["y"], y0 - 0.125)       # the march was exact
    M = np.rint(mass / r["unit"]).astype(np.int64)
    first = np.zeros((n, n), dtype=np.int64)
    first[np.rint(y0 * (n - 1)).astype(int), np.rint(x0 * (n - 1)).astype(int)] = M
    assert np.array_equal(r["counts"][..., 0], first) and r["total_units"] == int(M.sum())
    for k in range(nt):
        want = np.zeros((n, n), dtype=np.int64)
        for p in range(x0.size):
            for node, d in _split_by_hand(int(M[p]), x0[p] * (n - 1) + 0.5 * k, y0[p] * (n - 1) - 0.25 * k, n).items():
                want[node] += d
        assert np.array_equal(r["counts"][..., k], want), k
        if k % 4 == 0:
            shifted = np.zeros_like(first)
            shifted[:n - k // 4, k // 2:] = first[k // 4:, :n - k // 2]
            assert np.array_equal(r["counts"][..., k], shifted), k
        assert np.array_equal(r["frames"][..., k], want * r["unit"])
    back = A.push_forward(out, r["x"], r["y"], mass=mass, frames=[0], direction=-1, rho_floor=0.5)
    assert np.array_equal(back["counts"][..., 0], first)
    assert np.array_equal(back["x"], x0) and np.array_equal(back["y"], y0)


def _rotation_out(n=17, nt=9, omega=np.pi / 2):
    """_rotation_out of tests/test_advect_host.py: a rigid quarter turn about the centre of the square"""
    g = np.arange(n) / float(n - 1)
    Y, X = np.meshgrid(g, g, indexing="ij")                              # arrays are (ny, nx)
    one = np.ones(nt)
    return dict(rho=np.ones((n, n, nt)), Ex=(-omega * (Y - 0.5))[:, :, None] * one, Ey=(omega * (X - 0.5))[:, :, None] * one)


# l1 of the pushed Gaussian against the analytically rotated one, measured with this twin (x86-64, glibc, 2026-10-19);
# the bound asserted is 1.5 times these: the margin covers differences between maths libraries only.  The values fall
# with n towards a plateau, not towards zero: one particle per node on a lattice turned against the grid leaves a moire
# of a few per cent of the density in the bilinear sums (the mean of the density is 0.03), whatever the spacing.
ROTATION_L1 = {17: 3.3031e-03, 33: 1.8298e-03, 65: 1.5644e-03}


def test_rotated_gaussian_converges():
    s, th = 0.07, np.pi / 3            # (a quarter turn would take nodes to nodes: no split to look at)
    got = {}
    for n in (17, 33, 65):
        out = _rotation_out(n, omega=th)
        g = np.arange(n) / float(n - 1)
        Y, X = np.meshgrid(g, g, indexing="ij")
        blob = lambda cy, cx: np.exp(-0.5 * (((Y - cy) / s) ** 2 + ((X - cx) / s) ** 2))      # noqa: E731
        inside = np.hypot(Y - 0.5, X - 0.5) <= 0.45                       # these stay in the square
        x0, y0 = A.seeds_on_nodes(n, n, mask=inside)
        r = A.push_forward(out, x0, y0, mass=A.masses_on_nodes(blob(0.5, 0.7), mask=inside), frames=[8], nsub=4, rho_floor=0.5)
        assert r["n_clamped"] == 0
        # the turn by th about the centre of the square takes the blob's centre (x, y) = (0.7, 0.5) to 0.5 + 0.2 (cos, sin)
        got[n] = float(np.mean(np.abs(r["frames"][..., 0] - blob(0.5 + 0.2 * np.sin(th), 0.5 + 0.2 * np.cos(th)))))
        print("rotation n = %d: l1 %.4e (recorded %.4e)" % (n, got[n], ROTATION_L1[n]))
    assert got[17] > got[33] > got[65]
    for n in got:
        assert got[n] <= 1.5 * ROTATION_L1[n], (n, got[n])


def _still_out(n=6, nt=3):
    shp = (n, n, nt)
    return dict(rho=np.ones(shp, order="F"), Ex=np.zeros(shp, order="F"), Ey=np.zeros(shp, order="F"))


def test_border_and_zero_mass():
    n = 6
    out = _still_out(n)
    #            last column      last row         the far corner   inside, without mass
    x = np.array([1.0,            0.4,             1.0,             0.5])
    y = np.array([0.4,            1.0,             1.0,             0.5])
    mass = np.array([1.0, 0.5, 0.25, 0.0])
    r = A.push_forward(out, x, y, mass=mass, rho_floor=0.5)
    c = r["counts"][..., -1]
    M = np.rint(mass / r["unit"]).astype(np.int64)
    assert np.array_equal(r["counts"][..., 0], c)
    assert c[2, n - 1] == M[0] and c[n - 1, 2] == M[1] and c[n - 1, n - 1] == M[2]        # (i = n - 2, a = 1): all on the border node
    assert np.count_nonzero(c) == 3 and c.sum() == r["total_units"] == int(M.sum())
    line = dict(rho=np.ones((n, 3)), Ex=np.zeros((n, 3)))
    r1 = A.push_forward(line, np.array([1.0, 0.5, 0.3]), mass=np.array([1.0, 0.0, 0.0]), rho_floor=0.5)
    assert r1["counts"][n - 1, 0] == r1["total_units"] and np.count_nonzero(r1["counts"][..., 0]) == 1


def test_negative_remainder_on_the_last_corner():
    """d11 = M - d00 - d10 - d01 = -1 when the three rounded corners take one unit too many; found here by search over
    small M and cell offsets.  With other particles on that node the count stays >= 0; alone, the count is the signed
    value itself (include/dotsocp.h: the counts are signed)."""
    n = 6
    found = None
    for M in range(1, 40):
        for ka in range(1, 32):
            for kc in range(1, 32):
                a, c = ka / 32.0, kc / 32.0
                d = [round(((1 - c) * (1 - a)) * M), round((c * (1 - a)) * M), round(((1 - c) * a) * M)]
                if M - sum(d) == -1 and found is None:
                    found = (M, a, c, d)
    assert found is not None
    M, a, c, d = found
    print("d11 = -1 for M = %d at a = %g, c = %g: corners %s" % (M, a, c, d))
    out = _still_out(n)
    j, i = 2, 3
    big = 1.0
    for others in (True, False):
        # a heavy particle far away fixes the unit; `others`: two more sit exactly on the node that takes the remainder
        x = [0.0, (i + a) / (n - 1)] + ([(i + 1) / (n - 1)] * 2 if others else [])
        y = [0.0, (j + c) / (n - 1)] + ([(j + 1) / (n - 1)] * 2 if others else [])
        unit = A.mass_unit(len(x), big)
        mass = [big, M * unit] + ([3 * unit, 5 * unit] if others else [])
        r = A.push_forward(out, np.array(x), np.array(y), mass=np.array(mass), frames=[1], rho_floor=0.5)
        assert r["unit"] == unit
        cnt = r["counts"][..., 0]
        assert [cnt[j, i], cnt[j + 1, i], cnt[j, i + 1]] == d
        assert cnt[j + 1, i + 1] == (7 if others else -1)
        assert cnt.sum() == r["total_units"] == int(round(big / unit)) + M + (8 if others else 0)
        assert (np.all(cnt >= 0) and np.all(r["frames"] >= 0)) if others else r["frames"][j + 1, i + 1, 0] == -unit


def test_refused_arguments():
    out = _still_out()
    x, y = np.array([0.2, 0.4, 0.6]), np.array([0.3, 0.3, 0.3])
    ok = np.array([1.0, 2.0, 0.0])
    A.push_forward(out, x, y, mass=ok, rho_floor=0.5)
    for bad in ([1.0, -1e-300, 1.0], [1.0, np.nan, 1.0], [1.0, np.inf, 1.0], [0.0, 0.0, 0.0], [1.0, 1.0], None):
        with pytest.raises(ValueError):
            A.push_forward(out, x, y, mass=bad, rho_floor=0.5)
    for frames in ([], [1, 1], [2, 1], [-1, 0], [0, 3], [3]):
        with pytest.raises(ValueError):
            A.push_forward(out, x, y, mass=ok, frames=frames, rho_floor=0.5)
    line = dict(rho=np.ones((6, 3)), Ex=np.zeros((6, 3)))
    A.push_forward(line, x, mass=ok, rho_floor=0.5)
    with pytest.raises(ValueError):
        A.push_forward(line, x, y, mass=ok, rho_floor=0.5)                 # y on 1-D outputs
    with pytest.raises(ValueError):
        A.push_forward(out, x, mass=ok, rho_floor=0.5)                     # no y on 2-D outputs
    for kw in (dict(nsub=0), dict(direction=0)):
        with pytest.raises(ValueError):
            A.push_forward(out, x, y, mass=ok, rho_floor=0.5, **kw)
