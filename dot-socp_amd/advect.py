"""Where the mass goes: the velocity v = E / rho of a solved flow and particles carried along it (the transport map).

Host twins (numpy) of dotsocp_recover_velocity and dotsocp_advect_particles (include/dotsocp.h states the semantics once;
csrc/advect.hip and this module follow them operation by operation -- no fused multiply-add on either side -- so
InPALMContext.velocity() / .advect() and velocity(ctx.outputs(), floor) / advect(ctx.outputs(), ...) agree bit for bit).
The velocity is the one utils/show_movement_2d.m draws: arrows of E, masked where rho is small.
push_forward is the twin of dotsocp_push_mass: the masses the particles carry, deposited on the grid at chosen time nodes
in whole units (int64 planes, np.add.at), so that every frame conserves the mass exactly and no bit depends on the order
of the particles; InPALMContext.push_forward() returns the same bits.
map_report is the twin of dotsocp_map_report: displacement, path length and kinetic action of every particle and their
mass-weighted means, added in the device's order; InPALMContext.map_report() returns the same bits.

Coordinates: the unit square and t in [0, 1]; x runs along the SECOND array index of the outputs (nx columns, node i at
i / (nx - 1)), y along the first (ny rows); 1-D outputs (nx, nt) have x alone.  E = +rho v.
"""
import math

import numpy as np


def default_rho_floor(rho0, rho1):
    """max(rho0.max(), rho1.max()) / 100: the mask rule of show_movement_2d.m:31 (rho < max(rho) / 100 draws no arrow),
    with the maximum taken over the two GIVEN densities instead of over all of rho, so that it needs no pass over rho (and
    is known before the solve)."""
    return max(float(np.max(rho0)), float(np.max(rho1))) / 100


def _quot(E, rho, floor):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = E / rho
        return np.where((rho > floor) & np.isfinite(q), q, 0.0)


def velocity(out, rho_floor):
    """Twin of dotsocp_recover_velocity on the outputs dict (rho, Ex[, Ey]): dict(vx=..., [vy=...]) of the outputs'
    shapes; v = E / rho where rho > rho_floor and the quotient is finite, else 0 (a NaN density gives 0)."""
    rho = np.asarray(out["rho"], dtype=np.float64)
    floor = float(rho_floor)
    v = dict(vx=_quot(np.asarray(out["Ex"], dtype=np.float64), rho, floor))
    if "Ey" in out:
        v["vy"] = _quot(np.asarray(out["Ey"], dtype=np.float64), rho, floor)
    return v


def _clamp(u):
    return np.where(u < 0.0, 0.0, np.where(u > 1.0, 1.0, u))


def _cell(u, n):
    f = u * float(n - 1)
    i = np.minimum(np.floor(f).astype(np.int64), n - 2)
    return i, f - i.astype(np.float64)


class _Field:
    """The node velocity, interpolated: bilinear in a layer, linear between the two layers of a time interval"""

    def __init__(self, v):
        self.vx, self.vy = v["vx"], v.get("vy")
        self.one_d = self.vy is None
        self.nx = self.vx.shape[0 if self.one_d else 1]
        self.ny = None if self.one_d else self.vx.shape[0]

    def _layer(self, F, i, a, j, c):
        if self.one_d:
            return (1.0 - a) * F[i] + a * F[i + 1]
        f0 = (1.0 - c) * F[j, i] + c * F[j + 1, i]
        f1 = (1.0 - c) * F[j, i + 1] + c * F[j + 1, i + 1]
        return (1.0 - a) * f0 + a * f1

    def __call__(self, x, y, k, b):
        i, a = _cell(x, self.nx)
        j, c = (None, None) if self.one_d else _cell(y, self.ny)
        at = lambda V: (1.0 - b) * self._layer(V[..., k], i, a, j, c) + b * self._layer(V[..., k + 1], i, a, j, c)  # noqa: E731
        return at(self.vx), (None if self.one_d else at(self.vy))


def advect(out, x, y=None, nsub=1, direction=+1, rho_floor=None, trajectories=False):
    """Twin of dotsocp_advect_particles on the outputs dict: classical RK4 along v = E / rho, nsub steps per time interval,
    from t = 0 to 1 (direction=+1) or from 1 to 0 (-1).  x, y: seeds (y None for 1-D outputs); rho_floor None:
    default_rho_floor of the first and last layer of rho (which are rho0 and rho1).  Returns dict(x, y, traj_x, traj_y,
    n_clamped): final positions; with trajectories=True the (n, nt) positions at every time node, indexed by node in
    both directions (else None); the number of particles that the clamp at the end of some step moved."""
    return _march(out, x, y, nsub, direction, rho_floor, trajectories, False)


def _march(out, x, y, nsub, direction, rho_floor, trajectories, path):
    """advect(); path=True (map_report): the result also holds x0, y0 (the clamped seeds), sq and len -- the sums of
    |step|^2 and |step| over all steps, each step taken between the position before it and the one after its end clamp --
    and steps = (nt - 1) * nsub"""
    rho = np.asarray(out["rho"], dtype=np.float64)
    one_d = "Ey" not in out
    if one_d != (y is None):
        raise ValueError("advect(): y is given for 2-D outputs and only for them")
    nsub, direction = int(nsub), int(direction)
    if nsub < 1 or direction not in (1, -1):
        raise ValueError("advect(): nsub >= 1 and direction +1 or -1")
    if rho_floor is None:
        rho_floor = default_rho_floor(rho[..., 0], rho[..., -1])
    nt = rho.shape[-1]
    x = np.array(x, dtype=np.float64).ravel()
    y = None if one_d else np.array(y, dtype=np.float64).ravel()
    if x.size < 1 or (y is not None and y.size != x.size):
        raise ValueError("advect(): x and y hold the same number (>= 1) of seeds")
    if not (np.all(np.isfinite(x)) and (one_d or np.all(np.isfinite(y)))):
        raise ValueError("advect(): a seed is not finite")
    V = _Field(velocity(out, rho_floor))
    dt = direction / float((nt - 1) * nsub)
    hh, h6 = 0.5 * dt, dt / 6.0
    den = float(2 * nsub)
    x = _clamp(x)
    y = None if one_d else _clamp(y)
    moved = np.zeros(x.size, dtype=bool)
    step = lambda p, h, k: None if p is None else _clamp(p + h * k)          # noqa: E731
    final = lambda p, k1, k2, k3, k4: p + h6 * (((k1 + 2.0 * k2) + 2.0 * k3) + k4)   # noqa: E731
    tx = np.empty((x.size, nt), order="F") if trajectories else None
    ty = np.empty((x.size, nt), order="F") if trajectories and not one_d else None

    def record(node):
        if trajectories:
            tx[:, node] = x
            if not one_d:
                ty[:, node] = y

    record(0 if direction > 0 else nt - 1)
    x0, y0 = x, y
    sq, length = np.zeros(x.size), np.zeros(x.size)
    for it in range(nt - 1):
        k = it if direction > 0 else nt - 2 - it
        for s in range(nsub):
            e0 = 2 * s if direction > 0 else 2 * (nsub - s)
            b0, b1, b2 = e0 / den, (e0 + direction) / den, (e0 + 2 * direction) / den
            k1x, k1y = V(x, y, k, b0)
            k2x, k2y = V(step(x, hh, k1x), step(y, hh, k1y), k, b1)
            k3x, k3y = V(step(x, hh, k2x), step(y, hh, k2y), k, b1)
            k4x, k4y = V(step(x, dt, k3x), step(y, dt, k3y), k, b2)
            xo, yo = x, y
            ux = final(x, k1x, k2x, k3x, k4x)
            moved |= (ux < 0.0) | (ux > 1.0)
            x = _clamp(ux)
            if not one_d:
                uy = final(y, k1y, k2y, k3y, k4y)
                moved |= (uy < 0.0) | (uy > 1.0)
                y = _clamp(uy)
            if path:
                ex = x - xo
                s2 = ex * ex if one_d else ex * ex + (y - yo) * (y - yo)
                sq = sq + s2
                length = length + np.sqrt(s2)
        record(k + 1 if direction > 0 else k)
    r = dict(x=x, y=y, traj_x=tx, traj_y=ty, n_clamped=int(np.count_nonzero(moved)))
    if path:
        r.update(x0=x0, y0=y0, sq=sq, len=length, steps=(nt - 1) * nsub)
    return r


def _tree_sum(t):
    """The sum of the terms t (all >= 0) in the order dotsocp_map_report adds them (include/dotsocp.h, "Sums"): blocks of 256
    consecutive particles, padded with +0.0; in a block the four wavefronts of 64 by the halving tree, then ((w0 + w1) + w2)
    + w3; the blocks by k_report_final's tree: 256 running sums over every 256th block, then the halving tree."""
    t = np.asarray(t, dtype=np.float64)
    blocks = -(-t.size // 256)
    v = np.zeros(blocks * 256)
    v[:t.size] = t
    v = v.reshape(blocks, 4, 64)
    off = 32
    while off >= 1:
        v = v[..., :off] + v[..., off:2 * off]
        off //= 2
    w = v[..., 0]
    part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    rows = -(-blocks // 256)
    p = np.zeros(rows * 256)
    p[:blocks] = part
    p = p.reshape(rows, 256)
    red = np.zeros(256)
    for k in range(rows):
        red = red + p[k]
    off = 128
    while off >= 1:
        red = red[:off] + red[off:2 * off]
        off //= 2
    return float(red[0])


def map_report(out, x, y=None, mass=None, nsub=1, direction=+1, rho_floor=None, per_particle=False):
    """Twin of dotsocp_map_report on the outputs dict: how good the flow of v = E / rho is as a transport map.  The particles
    of advect() (same seeds, nsub, direction, rho_floor: same trajectories) each give the displacement disp = |end - start|,
    the path length len = sum |step| and the kinetic action = sum |step|^2 / |dt|; over the march of total time 1,
    disp^2 <= len^2 <= action, with equality iff the path is straight resp. the speed constant.  mass: one per particle,
    finite, >= 0, not all zero; None: all 1.  Returns dict(n, n_clamped, n_still, mass, cost_map, cost_length, cost_action,
    disp_mean, len_mean, disp_max, len_max, detour_max, detour_hist, detour_over, x, y, disp, len, action): the
    mass-weighted means of disp^2, len^2, action, disp, len (summed in the device's order, which depends on n alone: the same
    bits); maxima over all particles; detour = 1 - disp / len (0 for a particle that did not move) counted over the edges
    of report.report_edges() with the solution report's bin rule, detour_over = the count above the last edge (0.1);
    n_still = particles with len == 0; final positions; the per-particle arrays with per_particle=True, else None."""
    from .report import _bin_counts, report_edges
    n = np.asarray(x).size
    if mass is None:
        m = np.ones(n)
    else:
        m = np.array(mass, dtype=np.float64).ravel()
        if m.size != n:
            raise ValueError("map_report(): one mass per seed")
        if not np.all(np.isfinite(m)) or np.any(m < 0.0):
            raise ValueError("map_report(): a mass is negative or not finite")
        if not np.any(m > 0.0):
            raise ValueError("map_report(): all masses are zero")
    r = _march(out, x, y, nsub, direction, rho_floor, False, True)
    dx = r["x"] - r["x0"]
    disp2 = dx * dx if r["y"] is None else dx * dx + (r["y"] - r["y0"]) * (r["y"] - r["y0"])
    disp, length = np.sqrt(disp2), r["len"]
    action = r["sq"] * float(r["steps"])
    len2 = length * length
    with np.errstate(invalid="ignore", divide="ignore"):
        q = 1.0 - disp / length
        detour = np.where((length > 0.0) & (q > 0.0), q, 0.0)
    edges = report_edges()
    hist = _bin_counts(detour, edges)
    total = _tree_sum(m)
    mean = lambda t: _tree_sum(m * t) / total                               # noqa: E731
    return dict(n=int(n), n_clamped=r["n_clamped"], n_still=int(np.count_nonzero(length == 0.0)), mass=total,
                cost_map=mean(disp2), cost_length=mean(len2), cost_action=mean(action), disp_mean=mean(disp),
                len_mean=mean(length), disp_max=float(disp.max()), len_max=float(length.max()),
                detour_max=float(detour.max()), detour_hist=hist, detour_over=int(np.count_nonzero(detour > edges[-1])),
                x=r["x"], y=r["y"], disp=disp if per_particle else None, len=length if per_particle else None,
                action=action if per_particle else None)


def mass_unit(n, mass_max):
    """The unit of dotsocp_push_mass: 2^(e - 50) with frexp(n * mass_max) = (f, e), so that n particles of at most
    mass_max stay below 2^51 units in total."""
    top = float(n) * float(mass_max)
    if not (math.isfinite(top) and top > 0.0):
        raise ValueError("push_forward(): n * max(mass) must be positive and finite")
    unit = math.ldexp(1.0, math.frexp(top)[1] - 50)
    if unit < 2.2250738585072014e-308:
        raise ValueError("push_forward(): the unit 2^(e-50) of n * max(mass) is not a normal double")
    return unit


def _deposit(counts, x, y, M):
    """counts (int64 plane) += the bilinear split of the units M of the particles at (x, y): three corners rounded half
    to even, the fourth takes the remainder (include/dotsocp.h)"""
    Md = M.astype(np.float64)
    rnd = lambda w: np.rint(w * Md).astype(np.int64)                        # noqa: E731
    if y is None:
        i, a = _cell(x, counts.shape[0])
        d0 = rnd(1.0 - a)
        np.add.at(counts, i, d0)
        np.add.at(counts, i + 1, M - d0)
        return
    i, a = _cell(x, counts.shape[1])
    j, c = _cell(y, counts.shape[0])
    d00, d10, d01 = rnd((1.0 - c) * (1.0 - a)), rnd(c * (1.0 - a)), rnd((1.0 - c) * a)
    np.add.at(counts, (j, i), d00)
    np.add.at(counts, (j + 1, i), d10)
    np.add.at(counts, (j, i + 1), d01)
    np.add.at(counts, (j + 1, i + 1), M - d00 - d10 - d01)


def push_forward(out, x, y=None, mass=None, frames=None, nsub=1, direction=+1, rho_floor=None, unit=None):
    """Twin of dotsocp_push_mass on the outputs dict: the particles of advect() carry `mass` (n values, finite, >= 0, not
    all zero) and deposit it at the time nodes `frames` (strictly ascending indices; None: every node) by integer
    accumulation -- exact conservation, no dependence on the particle order (include/dotsocp.h).  unit (twin only): a
    unit fixed by the caller, mass_unit(n, max) of a larger particle set this call deposits a part of.  Returns
    dict(frames, counts, nodes, unit, l1, x, y, n_clamped, total_units): frames (ny, nx, nf) (1-D: (nx, nf)) =
    counts * unit, counts the signed int64 planes, l1[k] = mean |frames[..., k] - rho[..., nodes[k]]|, final positions and
    n_clamped as advect() returns them, total_units = sum of the particles' units = counts[..., k].sum() for every k."""
    rho = np.asarray(out["rho"], dtype=np.float64)
    one_d = "Ey" not in out
    nt = rho.shape[-1]
    if mass is None:
        raise ValueError("push_forward(): mass is needed")
    mass = np.array(mass, dtype=np.float64).ravel()
    n = np.asarray(x).size
    if mass.size != n:
        raise ValueError("push_forward(): one mass per seed")
    if not np.all(np.isfinite(mass)) or np.any(mass < 0.0):
        raise ValueError("push_forward(): a mass is negative or not finite")
    if not np.any(mass > 0.0):
        raise ValueError("push_forward(): all masses are zero")
    nodes = np.arange(nt, dtype=np.int64) if frames is None else np.array(frames, dtype=np.int64).ravel()
    if nodes.size < 1 or nodes[0] < 0 or nodes[-1] >= nt or np.any(np.diff(nodes) <= 0):
        raise ValueError("push_forward(): frames must be strictly ascending node indices in [0, nt)")
    unit = mass_unit(n, mass.max()) if unit is None else float(unit)
    M = np.rint(mass / unit).astype(np.int64)
    adv = advect(out, x, y, nsub=nsub, direction=direction, rho_floor=rho_floor, trajectories=True)
    counts = np.zeros(rho.shape[:-1] + (nodes.size,), dtype=np.int64, order="F")
    for k, node in enumerate(nodes):
        plane = np.zeros(rho.shape[:-1], dtype=np.int64)
        _deposit(plane, adv["traj_x"][:, node], None if one_d else adv["traj_y"][:, node], M)
        counts[..., k] = plane
    fr = np.asfortranarray(counts.astype(np.float64) * unit)
    l1 = np.array([np.mean(np.abs(fr[..., k] - rho[..., node])) for k, node in enumerate(nodes)])
    return dict(frames=fr, counts=counts, nodes=nodes, unit=unit, l1=l1, x=adv["x"], y=adv["y"], n_clamped=adv["n_clamped"],
                total_units=int(M.sum()))


def masses_on_nodes(rho, stride=1, mask=None):
    """The companion of seeds_on_nodes: the values of a 2-D (ny, nx) or 1-D (nx,) density at the same nodes, in the same
    order -- the masses of the particles seeded there."""
    rho = np.asarray(rho, dtype=np.float64)
    if rho.ndim == 1:
        i = np.arange(0, rho.shape[0], int(stride))
        keep = np.ones(i.size, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)[i]
        return rho[i][keep]
    j = np.arange(0, rho.shape[0], int(stride))
    i = np.arange(0, rho.shape[1], int(stride))
    jj, ii = np.meshgrid(j, i, indexing="ij")
    jj, ii = jj.ravel(order="F"), ii.ravel(order="F")
    keep = np.ones(jj.size, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)[jj, ii]
    return rho[jj, ii][keep]


def seeds_on_nodes(nx, ny=None, stride=1, mask=None):
    """Seeds on every stride-th node: (x, y) of the nodes (j, i), j = 0, stride, .. < ny and i = 0, stride, .. < nx, in
    the grid's own order (y fastest: neighbouring particles then gather from neighbouring memory); 1-D (ny None): (x, None).
    mask: boolean (ny, nx) array (1-D: (nx,)); only the nodes where it is true are kept."""
    i = np.arange(0, int(nx), int(stride))
    if ny is None:
        keep = np.ones(i.size, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)[i]
        return (i / float(nx - 1))[keep], None
    j = np.arange(0, int(ny), int(stride))
    jj, ii = np.meshgrid(j, i, indexing="ij")
    jj, ii = jj.ravel(order="F"), ii.ravel(order="F")
    keep = np.ones(jj.size, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)[jj, ii]
    return (ii / float(nx - 1))[keep], (jj / float(ny - 1))[keep]
