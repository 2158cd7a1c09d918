"""An upper bound on the transport cost: soft Hopf-Lax (log-domain Sinkhorn) sweeps rounded to a feasible plan.

For the cost c(x, y) = |x - y|^2 / 2 between the nodes and ANY pair of functions f, g on the nodes, the matrix
P_ij = a_i b_j exp((f_i + g_j - c_ij) / eps) can be scaled down (f' = min(f, f~), g' = min(g, g~): Altschuler, Weed and
Rigollet) until its row sums stay below a and its column sums below b; what is missing, er = a - rows and ec = b - columns,
is filled by the rank-one plan er ec^T / delta.  The sum has the marginals a = rho0 / sum(rho0) and b = rho1 / sum(rho1)
exactly, so 2 sum P c >= W2^2(a, b) whatever f and g are -- the counterpart of dual.dual_bound(), which certifies from below.
A few Sinkhorn sweeps at a temperature eps of a fraction of h^2, started from the solve's own potential, make the bound
tight.  The Gaussian kernel factorises over the axes: one update is the soft-min version of the two min-plus passes of
dual.hopf_lax, and the row masses, column masses and the cost sum P c are node sums of such transforms -- no n x n object.

The plan also names a map: barycentric_map() gives T(x_i) = E[y | x_i] of that plan, its cost and the spread around it
(map_cost + spread = upper), plan_frames() the displacement interpolant -- twins of dotsocp_plan_map / dotsocp_upper_map.

Host twins (numpy) of dotsocp_plan_bound / dotsocp_upper_bound: include/dotsocp.h states the arithmetic once;
csrc/softlax.hip and this module follow it operation by operation.  The device's exp and log are the only operations numpy
does not reproduce bit for bit, so device and twin agree to a few ulp of the largest entry, not to the bit.  Every function
has a `dtype`: np.longdouble runs the same operations in extended precision (the yardstick of tests/test_gpu_upper.py).

Arrays: 2-D layers (ny, nx) -- x runs along the second index --, 1-D layers (nx,).  Flat node indices are y fastest.
"""
import numpy as np

FIELDS = ("n_nodes", "sweeps", "zero0", "zero1", "nonfinite", "eps", "mass0", "mass1", "upper", "cost_kept", "cost_fill",
          "kept", "fill", "defect_first", "defect_last")
_INT_FIELDS = ("n_nodes", "sweeps", "zero0", "zero1", "nonfinite")
ARRAYS = ("f", "g", "E", "er", "ec", "defects")
# exp(x) is exactly +0.0 for every x below (the device skips such terms: include/dotsocp.h)
_EXP_ZERO = {"float64": -746.0, np.dtype(np.longdouble).name: -746.0 if np.finfo(np.longdouble).bits == 64 else -11400.0}


def _tree_sum(t, dtype=np.float64):
    """The sum of t in the order of dotsocp_map_report ("Sums"; advect._tree_sum), in `dtype`"""
    t = np.asarray(t, dtype=dtype).ravel()
    blocks = -(-t.size // 256)
    v = np.zeros(blocks * 256, dtype=dtype)
    v[:t.size] = t
    v = v.reshape(blocks, 4, 64)
    off = 32
    while off >= 1:
        v = v[..., :off] + v[..., off:2 * off]
        off //= 2
    w = v[..., 0]
    part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    rows = -(-blocks // 256)
    p = np.zeros(rows * 256, dtype=dtype)
    p[:blocks] = part
    p = p.reshape(rows, 256)
    red = np.zeros(256, dtype=dtype)
    for k in range(rows):
        red = red + p[k]
    off = 128
    while off >= 1:
        red = red[:off] + red[off:2 * off]
        off //= 2
    return red[0]


def _soft_axis(a, pm, eps, dtype, pb=None, moments=False):
    """One soft pass over the lines a[l, :] (no NaN, missing entries +Inf): (out, mean) with, for output j over the
    candidates c_i = a[l, i] + (double)((i - j)^2) * w:  m = min_i c_i,  s = sum_i exp((m - c_i) * ieps),
    q = sum_i exp((m - c_i) * ieps) * ((double)((i - j)^2) * w + pm[l, i]),  both added in ascending i from 0.0;
    out = m - eps * log(s), mean = q / s; a line without a finite entry: out = +Inf, mean = 0.
    moments=True (the moment flavour of the pass, dotsocp_plan_map): two more accumulators of the same kind,
    qa = sum_i e_i * ((double)(i - j) * h) and qb = sum_i e_i * pb[l, i] (pb None: zeros); returns (out, mean, qa / s, qb / s),
    the two quotients 0 on a dead line.  out and mean carry the bits of the plain pass."""
    lines, n = a.shape
    one = dtype(1.0)
    h = one / dtype(n - 1)
    w = (dtype(0.5) * h) * h
    ieps = one / eps
    j = np.arange(n, dtype=np.int64)
    m = np.full((lines, n), np.inf, dtype=dtype)
    for i in range(n):
        d = ((i - j) ** 2).astype(dtype) * w
        m = np.minimum(m, a[:, i:i + 1] + d[None, :])
    s = np.zeros((lines, n), dtype=dtype)
    q = np.zeros((lines, n), dtype=dtype)
    qa = np.zeros((lines, n), dtype=dtype) if moments else None
    qb = np.zeros((lines, n), dtype=dtype) if moments else None
    if moments and pb is None:
        pb = np.zeros((lines, n), dtype=dtype)
    dead = ~np.isfinite(m)
    zero = _EXP_ZERO[np.dtype(dtype).name]
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for i in range(n):
            d = ((i - j) ** 2).astype(dtype) * w
            x = (m - (a[:, i:i + 1] + d[None, :])) * ieps
            cols = np.flatnonzero((x >= zero).any(axis=0))      # elsewhere exp(x) is exactly +0.0: s and q stay as they are
            if cols.size == 0:
                continue
            e = np.exp(x[:, cols])
            e[dead[:, cols]] = 0.0
            s[:, cols] = s[:, cols] + e
            q[:, cols] = q[:, cols] + e * (d[None, cols] + pm[:, i:i + 1])
            if moments:
                qa[:, cols] = qa[:, cols] + e * ((i - j[cols]).astype(dtype) * h)[None, :]
                qb[:, cols] = qb[:, cols] + e * pb[:, i:i + 1]
        out = m - eps * np.log(s)
        mean = q / s
        if moments:
            da, db = qa / s, qb / s
    out[dead] = np.inf
    mean[dead] = 0.0
    if not moments:
        return out, mean
    da[dead] = 0.0
    db[dead] = 0.0
    return out, mean, da, db


def soft_transform(f, eps, dtype=np.float64):
    """Twin of the transform S of dotsocp_plan_bound.  f: a layer (ny, nx) or a line (n,); eps: the temperature (absolute).
    value(y) = -eps log sum_x exp(-(f(x) + |x - y|^2 / 2) / eps), along x first, then along y; mean(y) = the mean of
    |x - y|^2 / 2 under those weights.  Non-finite entries of f count as +Inf: such a node drops out.  Returns (value, mean)."""
    f = np.asarray(f, dtype=dtype)
    if f.ndim not in (1, 2) or min(f.shape) < 2:
        raise ValueError("soft_transform(): a layer (ny, nx) or a line (n,) with two nodes along every axis")
    eps = dtype(eps)
    if not (np.isfinite(eps) and eps > 0):
        raise ValueError("soft_transform(): eps must be positive and finite")
    a = np.where(np.isfinite(f), f, dtype(np.inf)).astype(dtype)
    if f.ndim == 1:
        v, mean = _soft_axis(a[None, :], np.zeros((1, a.size), dtype=dtype), eps, dtype)
        return v[0], mean[0]
    t, mx = _soft_axis(a, np.zeros(a.shape, dtype=dtype), eps, dtype)                       # rows: along x
    v, mean = _soft_axis(np.ascontiguousarray(t.T), np.ascontiguousarray(mx.T), eps, dtype)     # columns: along y
    return np.asfortranarray(v.T), np.asfortranarray(mean.T)


class UpperBound(dict):
    """The result of upper_bound() / sinkhorn_round(): the fields of the C struct dotsocp_upper (FIELDS) and, where asked
    for, the arrays f, g (the scaled-down potentials f', g'), E, er, ec, defects."""

    def __str__(self):
        return ("upper: W2^2 of the node histograms <= %.10g (kept %.10g of the mass at cost %.10g, fill %.3e at cost %.3e) | "
                "eps %.3e, %d sweeps, defect %.3e -> %.3e | zero mass %d / %d | %d non-finite"
                % (self["upper"], self["kept"], self["cost_kept"], self["fill"], self["cost_fill"], self["eps"],
                   self["sweeps"], self["defect_first"], self["defect_last"], self["zero0"], self["zero1"], self["nonfinite"]))


def _check_opts(eps_h2, max_sweeps, start, f_start, stateless):
    if not (np.isfinite(eps_h2) and eps_h2 > 0):
        raise ValueError("upper bound: eps_h2 must be positive and finite")
    if int(max_sweeps) < 0:
        raise ValueError("upper bound: max_sweeps must not be negative")
    if start not in (0, 1, 2):
        raise ValueError("upper bound: start is 0 (zeros), 1 (the potential) or 2 (f_start)")
    if start == 2 and f_start is None:
        raise ValueError("upper bound: start = 2 needs f_start")
    if start == 1 and stateless:
        raise ValueError("upper bound: start = 1 needs a potential")


def _masses(rho0, rho1, dtype):
    for r in (rho0, rho1):
        if not np.all(np.isfinite(r)) or np.any(r < 0):
            raise ValueError("upper bound: rho0 and rho1 must be finite and not negative")
    m0, m1 = _tree_sum(np.ravel(rho0, order="F"), dtype), _tree_sum(np.ravel(rho1, order="F"), dtype)
    if not (np.isfinite(m0) and m0 > 0 and np.isfinite(m1) and m1 > 0):
        raise ValueError("upper bound: the sum of rho0 or of rho1 is not a positive finite number")
    return m0, m1


def _eps(shape, eps_h2, dtype):
    one = dtype(1.0)
    if len(shape) == 1:
        h = one / dtype(shape[0] - 1)
        return (dtype(eps_h2) * h) * h
    return (dtype(eps_h2) * (one / dtype(shape[1] - 1))) * (one / dtype(shape[0] - 1))


def sinkhorn_round(rho0, rho1, f_start=None, eps_h2=0.25, max_sweeps=50, defect_tol=0.0, dtype=np.float64, g_start=None):
    """Twin of dotsocp_plan_bound: the sweeps from f_start (None: zeros; its non-finite entries are counted and count as
    0.0), the rounding and the sums.  Returns an UpperBound with all arrays.  g_start (host only, finite): the rounding
    takes this g in the place of S(la - f) -- it makes a feasible plan of ANY pair (f, g), which the tests use."""
    _check_opts(eps_h2, max_sweeps, 0 if f_start is None else 2, f_start, False)
    rho0, rho1 = np.asarray(rho0, dtype=dtype), np.asarray(rho1, dtype=dtype)
    if rho0.shape != rho1.shape or rho0.ndim not in (1, 2) or min(rho0.shape) < 2:
        raise ValueError("upper bound: rho0 and rho1 are layers (ny, nx) or lines (n,) of one shape, two nodes along every axis")
    shape = rho0.shape
    f = np.zeros(shape, dtype=dtype) if f_start is None else np.array(f_start, dtype=dtype)
    if f.shape != shape:
        raise ValueError("upper bound: the start potential has the shape of rho0")
    m0, m1 = _masses(rho0, rho1, dtype)
    total = lambda t: _tree_sum(np.ravel(t, order="F"), dtype)                       # noqa: E731
    eps = _eps(shape, eps_h2, dtype)
    ieps = dtype(1.0) / eps
    S = lambda t: soft_transform(t, eps, dtype)                                      # noqa: E731
    a, b = rho0 / m0, rho1 / m1
    bad = ~np.isfinite(f)
    f = np.where(bad, dtype(0.0), f)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        la, lb = -(eps * np.log(a)), -(eps * np.log(b))
        defects = np.full(int(max_sweeps), np.nan, dtype=dtype)
        sweeps = 0
        while sweeps < int(max_sweeps):
            g = S(la - f)[0]
            fn = S(lb - g)[0]
            defects[sweeps] = total(np.where(a > 0, a * np.abs(np.exp((f - fn) * ieps) - dtype(1.0)), dtype(0.0)))
            f = fn
            sweeps += 1
            if defects[sweeps - 1] <= defect_tol:
                break
        g = S(la - f)[0] if g_start is None else np.array(g_start, dtype=dtype)
        ft = S(lb - g)[0]
        f1 = np.where(ft < f, ft, f)
        gt, E = S(la - f1)
        g1 = np.where(gt < g, gt, g)
        fh = S(lb - g1)[0]
        r = np.where(a > 0, a * np.exp((f1 - fh) * ieps), dtype(0.0))
        k = np.where(b > 0, b * np.exp((g1 - gt) * ieps), dtype(0.0))
        er, ec = np.maximum(a - r, dtype(0.0)), np.maximum(b - k, dtype(0.0))
        if len(shape) == 1:
            px = np.zeros(shape, dtype=dtype)
            py = np.arange(shape[0]).astype(dtype) * (dtype(1.0) / dtype(shape[0] - 1))
        else:
            yy, xx = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
            px = xx.astype(dtype) * (dtype(1.0) / dtype(shape[1] - 1))
            py = yy.astype(dtype) * (dtype(1.0) / dtype(shape[0] - 1))
        p2 = px * px + py * py
        kept, cost_kept = total(k), total(k * E)
        R0, R1x, R1y, R2 = total(er), total(er * px), total(er * py), total(er * p2)
        C0, C1x, C1y, C2 = total(ec), total(ec * px), total(ec * py), total(ec * p2)
    delta = R0 if R0 < C0 else C0
    cost_fill = dtype(0.5) * ((R2 * C0 + R0 * C2) - dtype(2.0) * (R1x * C1x + R1y * C1y)) / delta if delta > 0 else dtype(0.0)
    as_f = (lambda v: v) if dtype is not np.float64 else float
    return UpperBound(n_nodes=int(rho0.size), sweeps=sweeps, zero0=int(np.count_nonzero(rho0 == 0)),
                      zero1=int(np.count_nonzero(rho1 == 0)), nonfinite=int(np.count_nonzero(bad)), eps=as_f(eps),
                      mass0=as_f(m0), mass1=as_f(m1), upper=as_f(dtype(2.0) * (cost_kept + cost_fill)),
                      cost_kept=as_f(cost_kept), cost_fill=as_f(cost_fill), kept=as_f(kept), fill=as_f(delta),
                      defect_first=as_f(defects[0]) if sweeps else float("nan"),
                      defect_last=as_f(defects[sweeps - 1]) if sweeps else float("nan"),
                      f=f1, g=g1, E=E, er=er, ec=ec, defects=defects)


def upper_bound(phi0, rho0, rho1, eps_h2=0.25, max_sweeps=50, defect_tol=0.0, start=1, f_start=None, dtype=np.float64):
    """Twin of dotsocp_upper_bound.  phi0: the first node layer of phi in original units (recoverOrgVar), or None with
    start 0 / 2; start = 1: the sweeps begin at f = -phi0, 2: at f_start, 0: at zeros.  Returns an UpperBound."""
    _check_opts(eps_h2, max_sweeps, start, f_start, phi0 is None)
    if start == 1:
        f_start = -np.asarray(phi0, dtype=dtype)
    elif start == 0:
        f_start = None
    return sinkhorn_round(rho0, rho1, f_start, eps_h2, max_sweeps, defect_tol, dtype)


def pair_cost(shape, dtype=np.float64):
    """c[i, j] = |x_i - y_j|^2 / 2 between all pairs of the nodes of a layer `shape` = (ny, nx) or a line (n,); nodes flat,
    y fastest"""
    if len(shape) == 1:
        t = np.arange(shape[0]).astype(dtype) / dtype(shape[0] - 1)
        return dtype(0.5) * (t[:, None] - t[None, :]) ** 2
    yy, xx = np.meshgrid(np.arange(shape[0]).astype(dtype) / dtype(shape[0] - 1),
                         np.arange(shape[1]).astype(dtype) / dtype(shape[1] - 1), indexing="ij")
    y, x = yy.ravel(order="F"), xx.ravel(order="F")
    return dtype(0.5) * ((x[:, None] - x[None, :]) ** 2 + (y[:, None] - y[None, :]) ** 2)


def plan_dense(f, g, er, ec, rho0, rho1, eps, dtype=np.float64):
    """The n x n plan the bound stands for, P[i, j] = a_i b_j exp((f_i + g_j - c_ij) / eps) + er_i ec_j / delta with
    c = pair_cost() and delta = min(sum er, sum ec); nodes flat, y fastest.  Host only, for small n (the tests)."""
    rho0, rho1 = np.asarray(rho0, dtype=dtype), np.asarray(rho1, dtype=dtype)
    flat = lambda t: np.ravel(np.asarray(t, dtype=dtype), order="F")               # noqa: E731
    a, b = flat(rho0) / flat(rho0).sum(), flat(rho1) / flat(rho1).sum()
    c = pair_cost(rho0.shape, dtype)
    f, g, er, ec = flat(f), flat(g), flat(er), flat(ec)
    with np.errstate(under="ignore"):
        P = (a[:, None] * b[None, :]) * np.exp(((f[:, None] + g[None, :]) - c) / dtype(eps))
    delta = min(er.sum(), ec.sum())
    if delta > 0:
        P = P + er[:, None] * ec[None, :] / delta
    return P


MAP_FIELDS = ("rows", "map_cost", "spread", "cost_rows", "disp_mean", "disp_max", "n_clamped", "unit")
MAP_ARRAYS = ("Dx", "Dy", "C", "row", "spread_nodes")


class PlanMap(dict):
    """The result of barycentric_map() / plan_map(): the fields of the C struct dotsocp_plan_map_t (MAP_FIELDS; the twin
    has n_clamped and unit only with frames), the node arrays Dx, Dy (a line: Dx alone), C, row, spread_nodes, `upper` (the
    UpperBound the map belongs to) and, where asked for, frames (ny, nx, nf)."""

    def __str__(self):
        return ("plan map: cost of the barycentric map %.10g + spread %.10g = %.10g (upper %.10g) | rows %.15g | "
                "displacement mean %.4g max %.4g" % (self["map_cost"], self["spread"], self["cost_rows"],
                                                     self["upper"]["upper"], self["rows"], self["disp_mean"], self["disp_max"]))


def _soft_moments(f, eps, dtype):
    """The transform S in its moment flavour: (value, mean cost, mean displacement along x, along y) of the softmax
    weights of every output node; a line: (value, mean cost, None, displacement).  value and mean cost carry the bits of
    soft_transform()."""
    a = np.where(np.isfinite(f), f, dtype(np.inf)).astype(dtype)
    if a.ndim == 1:
        v, mean, d, _ = _soft_axis(a[None, :], np.zeros((1, a.size), dtype=dtype), eps, dtype, moments=True)
        return v[0], mean[0], None, d[0]
    t, mx, ax, _ = _soft_axis(a, np.zeros(a.shape, dtype=dtype), eps, dtype, moments=True)          # rows: along x
    v, mean, dy, dx = _soft_axis(np.ascontiguousarray(t.T), np.ascontiguousarray(mx.T), eps, dtype,
                                 pb=np.ascontiguousarray(ax.T), moments=True)                       # columns: along y
    return tuple(np.asfortranarray(t.T) for t in (v, mean, dx, dy))


def barycentric_map(ub, rho0, rho1, dtype=np.float64):
    """Twin of the map part of dotsocp_plan_map.  ub: the UpperBound of sinkhorn_round(rho0, rho1, ..., dtype=dtype) with
    its arrays f, g, er, ec.  The last transform of the rounding, f^ = S(lb - g'), is made again with the moment
    accumulators: its softmax weights at source node i are the conditional law of the kept plan.  Returns a PlanMap
    (without n_clamped, unit and frames: plan_frames())."""
    rho0, rho1 = np.asarray(rho0, dtype=dtype), np.asarray(rho1, dtype=dtype)
    shape = rho0.shape
    m0, m1 = _masses(rho0, rho1, dtype)
    total = lambda t: _tree_sum(np.ravel(t, order="F"), dtype)                       # noqa: E731
    eps = dtype(ub["eps"])
    ieps = dtype(1.0) / eps
    zero, half, two = dtype(0.0), dtype(0.5), dtype(2.0)
    a, b = rho0 / m0, rho1 / m1
    f1, g1, er, ec = (np.asarray(ub[k], dtype=dtype) for k in ("f", "g", "er", "ec"))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        lb = -(eps * np.log(b))
        fh, kc, kdx, kdy = _soft_moments(lb - g1, eps, dtype)
        r = np.where(a > 0, a * np.exp((f1 - fh) * ieps), zero)
        if len(shape) == 1:
            px = np.zeros(shape, dtype=dtype)
            py = np.arange(shape[0]).astype(dtype) * (dtype(1.0) / dtype(shape[0] - 1))
            kdx = np.zeros(shape, dtype=dtype)
        else:
            yy, xx = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
            px = xx.astype(dtype) * (dtype(1.0) / dtype(shape[1] - 1))
            py = yy.astype(dtype) * (dtype(1.0) / dtype(shape[0] - 1))
        p2 = px * px + py * py
        R0 = total(er)
        C0, C1x, C1y, C2 = total(ec), total(ec * px), total(ec * py), total(ec * p2)
        fill = R0 if R0 < C0 else C0
        kappa = C0 / fill if fill > 0 else zero
        mx, my, m2 = (C1x / C0, C1y / C0, C2 / C0) if C0 > 0 else (zero, zero, zero)
        wk, wf = r, er * kappa
        row = wk + wf
        fdx, fdy = mx - px, my - py
        fc = half * ((m2 - two * (px * mx + py * my)) + p2)
        some = row != 0
        Dx = np.where(some, (wk * kdx + wf * fdx) / row, zero)
        Dy = np.where(some, (wk * kdy + wf * fdy) / row, zero)
        C = np.where(some, (wk * kc + wf * fc) / row, zero)
        d2 = Dx * Dx + Dy * Dy
        spread = np.where(some, two * C - d2, zero)
        disp = np.sqrt(d2)
        sums = dict(rows=total(row), map_cost=total(row * d2), spread=total(row * spread), cost_rows=two * total(row * C),
                    disp_mean=total(row * disp), disp_max=disp.max())
    as_f = (lambda v: v) if dtype is not np.float64 else float
    out = PlanMap((k, as_f(v)) for k, v in sums.items())
    out.update(upper=ub, C=C, row=row, spread_nodes=spread)
    if len(shape) == 1:
        out["Dx"] = Dy                  # a line lives along y in the library; its displacement comes back in Dx
    else:
        out.update(Dx=Dx, Dy=Dy)
    return out


def plan_frames(rho0, Dx, Dy, taus):
    """Twin of the frames of dotsocp_plan_map (float64: the deposit is integer arithmetic on float64 positions): every node
    carries M = rint(rho0 / unit) units, unit = advect.mass_unit(nodes, max rho0), to clamp(p + tau * D) and splits them over
    the corners of its cell as dotsocp_push_mass does.  A line: Dy = None.  Returns dict(frames (ny, nx, nf), counts, unit,
    n_clamped, total_units); n_clamped: the nodes with M > 0 that a clamp moved in some frame."""
    from . import advect
    rho0 = np.asarray(rho0, dtype=np.float64)
    shape = rho0.shape
    taus = np.asarray(taus, dtype=np.float64).ravel()
    if not np.all(np.isfinite(taus)) or np.any(taus < 0.0) or np.any(taus > 1.0):
        raise ValueError("plan_frames(): every tau is finite and in [0, 1]")
    unit = advect.mass_unit(rho0.size, rho0.max())
    M = np.rint(rho0 / unit).astype(np.int64)
    flat = lambda t: np.ravel(t, order="F")                                          # noqa: E731
    if len(shape) == 1:
        px = None
        py = np.arange(shape[0]).astype(np.float64) * (1.0 / float(shape[0] - 1))
        Dx, Dy = None, np.asarray(Dx, dtype=np.float64)
    else:
        yy, xx = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
        px = xx.astype(np.float64) * (1.0 / float(shape[1] - 1))
        py = yy.astype(np.float64) * (1.0 / float(shape[0] - 1))
        Dx, Dy = np.asarray(Dx, dtype=np.float64), np.asarray(Dy, dtype=np.float64)
    counts = np.zeros(shape + (taus.size,), dtype=np.int64, order="F")
    moved = np.zeros(shape, dtype=bool)
    for k, tau in enumerate(taus):
        plane = np.zeros(shape, dtype=np.int64)
        uy = py + tau * Dy
        Y = advect._clamp(uy)
        moved |= Y != uy
        if px is None:
            advect._deposit(plane, Y, None, M)
        else:
            ux = px + tau * Dx
            X = advect._clamp(ux)
            moved |= X != ux
            advect._deposit(plane, flat(X), flat(Y), flat(M))
        counts[..., k] = plane
    return dict(frames=np.asfortranarray(counts.astype(np.float64) * unit), counts=counts, unit=unit,
                n_clamped=int(np.count_nonzero(moved & (M > 0))), total_units=int(M.sum()))


def device_call(call, rho0, rho1, shape, eps_h2, max_sweeps, defect_tol, start, f_start, arrays):
    """Shared by plan_bound() and InPALMContext.upper_bound(): `call` takes the arguments of dotsocp_upper_bound behind the
    context (rho0, rho1, f_start, opts, res and the six optional arrays); rho0, rho1: contiguous float64 in memory order"""
    import ctypes
    from . import capi
    _check_opts(eps_h2, max_sweeps, start, f_start, False)
    if f_start is not None:
        f_start = np.asfortranarray(f_start, dtype=np.float64)
        if f_start.shape != tuple(shape):
            raise ValueError("upper bound: the start potential has the shape of rho0")
    o = capi.UpperOpts(float(eps_h2), int(max_sweeps), float(defect_tol), int(start))
    res = capi.Upper()
    out = {k: np.empty(shape, order="F") for k in ARRAYS[:5]} if arrays else {}
    if arrays:
        out["defects"] = np.empty(int(max_sweeps))
    ptr = lambda k: out[k].ctypes.data if k in out and out[k].size else None     # noqa: E731
    capi.check(call(capi.fptr(rho0), capi.fptr(rho1), None if f_start is None else capi.fptr(f_start), ctypes.byref(o),
                    ctypes.byref(res), *[ptr(k) for k in ARRAYS]))
    return from_struct(res, **out)


def plan_bound(rho0, rho1, f_start=None, eps_h2=0.25, max_sweeps=50, defect_tol=0.0, arrays=False, device=0):
    """dotsocp_plan_bound: sinkhorn_round() on HIP device `device` -- the stateless call, for densities without a solve (or
    with a potential from elsewhere: f_start = -phi0).  Returns an UpperBound; arrays=True adds f, g, E, er, ec, defects."""
    from . import capi
    r0, r1 = np.asfortranarray(rho0, dtype=np.float64), np.asfortranarray(rho1, dtype=np.float64)
    if r0.shape != r1.shape or r0.ndim not in (1, 2):
        raise ValueError("upper bound: rho0 and rho1 are layers (ny, nx) or lines (n,) of one shape")
    ny, nx = (1, r0.shape[0]) if r0.ndim == 1 else r0.shape
    call = lambda a, b, fs, o, res, *arr: capi.lib().dotsocp_plan_bound(a, b, ny, nx, fs, o, res, *arr, int(device))   # noqa: E731
    return device_call(call, r0, r1, r0.shape, eps_h2, max_sweeps, defect_tol, 0 if f_start is None else 2, f_start, arrays)


def device_map_call(call, rho0, rho1, shape, eps_h2, max_sweeps, defect_tol, start, f_start, arrays, times, int_times=False):
    """Shared by plan_map() and InPALMContext.plan_map(): `call` takes the arguments of dotsocp_plan_map behind ny, nx (rho0
    ... defects, map_res, Dx, Dy, C, row, spread, times, nf, frames).  times: the taus (int_times: the frame nodes) or None"""
    import ctypes
    from . import capi
    _check_opts(eps_h2, max_sweeps, start, f_start, False)
    if f_start is not None:
        f_start = np.asfortranarray(f_start, dtype=np.float64)
        if f_start.shape != tuple(shape):
            raise ValueError("upper bound: the start potential has the shape of rho0")
    o = capi.UpperOpts(float(eps_h2), int(max_sweeps), float(defect_tol), int(start))
    res, mres = capi.Upper(), capi.PlanMap()
    out = {k: np.empty(shape, order="F") for k in ARRAYS[:5]} if arrays else {}
    if arrays:
        out["defects"] = np.empty(int(max_sweeps))
    ptr = lambda k: out[k].ctypes.data if k in out and out[k].size else None     # noqa: E731
    names = MAP_ARRAYS if len(shape) == 2 else tuple(k for k in MAP_ARRAYS if k != "Dy")
    marr = {k: np.empty(shape, order="F") for k in names}
    nf = 0 if times is None else int(np.size(times))
    times = None if nf == 0 else np.ascontiguousarray(times, dtype=np.int64 if int_times else np.float64).ravel()
    frames = np.empty(tuple(shape) + (nf,), order="F") if nf else None
    capi.check(call(capi.fptr(rho0), capi.fptr(rho1), None if f_start is None else capi.fptr(f_start), ctypes.byref(o),
                    ctypes.byref(res), *[ptr(k) for k in ARRAYS], ctypes.byref(mres),
                    *[marr[k].ctypes.data if k in marr else None for k in MAP_ARRAYS],
                    None if nf == 0 else times.ctypes.data, nf, None if nf == 0 else frames.ctypes.data))
    got = PlanMap((k, (int if k == "n_clamped" else float)(getattr(mres, k))) for k in MAP_FIELDS)
    got.update(marr, upper=from_struct(res, **out))
    if nf:
        got["frames"] = frames
    return got


def plan_map(rho0, rho1, f_start=None, eps_h2=0.25, max_sweeps=50, defect_tol=0.0, arrays=False, taus=None, device=0):
    """dotsocp_plan_map: plan_bound() and the barycentric map of its plan on HIP device `device` -- barycentric_map() and
    plan_frames() of the twin.  Returns a PlanMap: the numbers, Dx, Dy (a line: Dx alone), C, row, spread_nodes, `upper` (the
    UpperBound, with its arrays if arrays=True) and, with taus (values in [0, 1]), frames (ny, nx, len(taus))."""
    from . import capi
    r0, r1 = np.asfortranarray(rho0, dtype=np.float64), np.asfortranarray(rho1, dtype=np.float64)
    if r0.shape != r1.shape or r0.ndim not in (1, 2):
        raise ValueError("upper bound: rho0 and rho1 are layers (ny, nx) or lines (n,) of one shape")
    ny, nx = (1, r0.shape[0]) if r0.ndim == 1 else r0.shape
    call = lambda a, b, fs, *rest: capi.lib().dotsocp_plan_map(a, b, ny, nx, fs, *rest, int(device))   # noqa: E731
    return device_map_call(call, r0, r1, r0.shape, eps_h2, max_sweeps, defect_tol, 0 if f_start is None else 2, f_start, arrays, taus)


def map_gap(x0, y0, x1, y1, dx, dy, mass):
    """How far the flow's particles end from the static map: with gap2_p = |X_p(1) - (x_p + D(x_p))|^2 of the particles seeded
    at (x0, y0) (a line: y0 = y1 = dy = None) that ended at (x1, y1), map_gap = sum mass * gap2 / sum mass (both sums by
    _tree_sum) and map_gap_max = max gap2.  Host arithmetic."""
    ex = np.asarray(x1, dtype=np.float64) - (np.asarray(x0, dtype=np.float64) + np.asarray(dx, dtype=np.float64))
    gap2 = ex * ex
    if y0 is not None:
        ey = np.asarray(y1, dtype=np.float64) - (np.asarray(y0, dtype=np.float64) + np.asarray(dy, dtype=np.float64))
        gap2 = gap2 + ey * ey
    mass = np.asarray(mass, dtype=np.float64)
    return dict(map_gap=float(_tree_sum(mass * gap2) / _tree_sum(mass)), map_gap_max=float(gap2.max()), n=int(gap2.size))


def from_struct(res, **arrays):
    """UpperBound from a capi.Upper filled by the library and the arrays that were asked for"""
    out = UpperBound((k, (int if k in _INT_FIELDS else float)(getattr(res, k))) for k in FIELDS)
    out.update({k: v for k, v in arrays.items() if v is not None})
    return out
