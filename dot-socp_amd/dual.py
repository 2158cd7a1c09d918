"""A lower bound on the transport cost from the potential: the Hopf-Lax transform of phi and the Kantorovich dual.

For ANY function psi0 on the nodes, psi1(y) = min_x psi0(x) + |x - y|^2 / 2 satisfies psi1(y) - psi0(x) <= |x - y|^2 / 2 for
every pair of nodes, so 2 (sum psi1 b - sum psi0 a) <= W2^2(a, b) between the node histograms a = rho0 / sum(rho0) and
b = rho1 / sum(rho1), whatever state the solve is in.  With psi0 = phi(t = 0) that is the Hopf-Lax transform of the potential
to t = 1 (`bound_fwd`); the mirror transform of phi(t = 1) back to t = 0 gives `bound_bwd`.  Certified is the discrete static
cost between the node histograms, which differs from the continuous W2^2 by O(h).

Host twins (numpy) of dotsocp_dual_bound: include/dotsocp.h states the arithmetic once; csrc/hopflax.hip and this module
follow it operation by operation -- no fused multiply-add on either side -- so InPALMContext.dual_bound() and
dual_bound(phi0, phi1, rho0, rho1) of the downloaded, recovered layers agree bit for bit.

Arrays: 2-D layers (ny, nx) -- x runs along the second index --, 1-D layers (nx,).  Flat node indices are y fastest.
"""
import numpy as np

from .advect import _tree_sum

_TEMP = 1 << 22          # candidates formed at a time (doubles)


def _axis_pass(a, sign):
    """One pass over the lines a[l, :]: (values, winners), out[l, j] = min_i a[l, i] + (double)((i - j)^2) * w (sign > 0) or
    max_i a[l, i] - ... (sign < 0), w = (0.5 * h) * h, h = 1 / (n - 1); the smallest index wins a tie, the value is the winning
    candidate.  The lines hold no NaN (hopf_lax replaces them)."""
    lines, n = a.shape
    h = 1.0 / float(n - 1)
    w = (0.5 * h) * h
    i = np.arange(n, dtype=np.int64)
    val = np.empty((lines, n))
    idx = np.empty((lines, n), dtype=np.int32)
    jb = max(1, _TEMP // (lines * n))
    with np.errstate(over="ignore"):
        for j0 in range(0, n, jb):
            j = i[j0:j0 + jb]
            d = ((i[None, :] - j[:, None]) ** 2).astype(np.float64) * w
            cand = a[:, None, :] + d[None] if sign > 0 else a[:, None, :] - d[None]
            k = cand.argmin(axis=2) if sign > 0 else cand.argmax(axis=2)       # the first of equal candidates
            val[:, j0:j0 + jb] = np.take_along_axis(cand, k[..., None], axis=2)[..., 0]
            idx[:, j0:j0 + jb] = k
    return val, idx


def hopf_lax(f, sign=+1):
    """Twin of the transform of dotsocp_dual_bound.  f: a layer (ny, nx) or a line (n,).  sign=+1: forward,
    H(y) = min_x f(x) + |x - y|^2 / 2; sign=-1: backward, B(x) = max_y f(y) - |x - y|^2 / 2; along x first, then along y.
    Non-finite entries of f count as +Inf (forward) / -Inf (backward).  Returns (values, winners, nonfinite): winners int32,
    the flat node index (y fastest) whose candidate won, the smallest on ties; nonfinite: the entries replaced."""
    f = np.asarray(f, dtype=np.float64)
    if f.ndim not in (1, 2) or min(f.shape) < 2:
        raise ValueError("hopf_lax(): a layer (ny, nx) or a line (n,) with two nodes along every axis")
    if sign not in (1, -1):
        raise ValueError("hopf_lax(): sign +1 (forward) or -1 (backward)")
    ok = np.isfinite(f)
    a = np.where(ok, f, np.inf if sign > 0 else -np.inf)
    bad = int(f.size - np.count_nonzero(ok))
    if f.ndim == 1:
        val, idx = _axis_pass(a[None, :], sign)
        return val[0], idx[0], bad
    ny, nx = f.shape
    t, ix = _axis_pass(a, sign)                    # rows: along x
    v, iy = _axis_pass(np.ascontiguousarray(t.T), sign)         # columns: along y
    val, iy = v.T, iy.T
    win = iy.astype(np.int64) + ny * ix[iy, np.arange(nx)[None, :]].astype(np.int64)
    return np.asfortranarray(val), np.asfortranarray(win.astype(np.int32)), bad


FIELDS = ("n_nodes", "nonfinite", "mass0", "mass1", "dual_raw", "bound_fwd", "bound_bwd", "bound", "gap1_max", "gap1_min",
          "gap1_mean", "gap0_max", "gap0_min", "gap0_mean", "map_cost_bwd")


class DualBound(dict):
    """The result of dual_bound(): the fields of the C struct dotsocp_dual (FIELDS) and, where asked for, the arrays H, B,
    arg_fwd, arg_bwd."""

    def __str__(self):
        return ("dual: bound %.10g (fwd %.10g, bwd %.10g) <= W2^2 of the node histograms | raw dual %.10g | gap at t=1 "
                "[%.3e, %.3e], at t=0 [%.3e, %.3e] | map cost %.10g | %d non-finite"
                % (self["bound"], self["bound_fwd"], self["bound_bwd"], self["dual_raw"], self["gap1_min"], self["gap1_max"],
                   self["gap0_min"], self["gap0_max"], self["map_cost_bwd"], self["nonfinite"]))


def _extrema(g):
    ok = np.isfinite(g)
    if not ok.any():
        return float("-inf"), float("inf")
    return float(g[ok].max() + 0.0), float(g[ok].min() + 0.0)


def dual_bound(phi0, phi1, rho0, rho1):
    """Twin of dotsocp_dual_bound.  phi0, phi1: the first and last node layer of phi in original units (recoverOrgVar);
    rho0, rho1: the given densities; all (ny, nx) or (nx,).  Returns a DualBound with the arrays."""
    phi0, phi1 = np.asarray(phi0, dtype=np.float64), np.asarray(phi1, dtype=np.float64)
    rho0, rho1 = np.asarray(rho0, dtype=np.float64), np.asarray(rho1, dtype=np.float64)
    if not (phi0.shape == phi1.shape == rho0.shape == rho1.shape):
        raise ValueError("dual_bound(): phi0, phi1, rho0 and rho1 have one shape")
    H, af, bad0 = hopf_lax(phi0, +1)
    B, ab, bad1 = hopf_lax(phi1, -1)
    total = lambda t: _tree_sum(np.ravel(t, order="F"))                     # noqa: E731
    m0, m1 = total(rho0), total(rho1)
    if not (np.isfinite(m0) and m0 > 0.0 and np.isfinite(m1) and m1 > 0.0):
        raise ValueError("dual_bound(): the sum of rho0 or of rho1 is not a positive finite number")
    with np.errstate(invalid="ignore", over="ignore"):
        a0, a1 = total(phi0 * rho0) / m0, total(phi1 * rho1) / m1
        fwd = 2.0 * (total(H * rho1) / m1 - a0)
        bwd = 2.0 * (a1 - total(B * rho0) / m0)
        g1, g0 = phi1 - H, phi0 - B
        gap1, gap0 = total(np.abs(g1) * rho1) / m1, total(np.abs(g0) * rho0) / m0
    if phi0.ndim == 1:
        n = phi0.shape[0]
        e = (np.arange(n) - ab).astype(np.float64) * (1.0 / float(n - 1))
        d2 = e * e
    else:
        ny, nx = phi0.shape
        y, x = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
        ex = (x - ab // ny).astype(np.float64) * (1.0 / float(nx - 1))
        ey = (y - ab % ny).astype(np.float64) * (1.0 / float(ny - 1))
        d2 = ex * ex + ey * ey
    g1max, g1min = _extrema(g1)
    g0max, g0min = _extrema(g0)
    return DualBound(n_nodes=int(phi0.size), nonfinite=bad0 + bad1, mass0=m0, mass1=m1, dual_raw=2.0 * (a1 - a0),
                     bound_fwd=fwd, bound_bwd=bwd, bound=bwd if bwd > fwd else fwd, gap1_max=g1max, gap1_min=g1min,
                     gap1_mean=gap1, gap0_max=g0max, gap0_min=g0min, gap0_mean=gap0, map_cost_bwd=total(rho0 * d2) / m0,
                     H=H, B=B, arg_fwd=af, arg_bwd=ab)


def from_struct(res, H=None, B=None, arg_fwd=None, arg_bwd=None):
    """DualBound from a capi.Dual filled by dotsocp_dual_bound and the arrays that were asked for"""
    out = DualBound((k, (int if k in ("n_nodes", "nonfinite") else float)(getattr(res, k))) for k in FIELDS)
    out.update({k: v for k, v in dict(H=H, B=B, arg_fwd=arg_fwd, arg_bwd=arg_bwd).items() if v is not None})
    return out
