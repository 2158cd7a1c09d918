"""The geodesic's profile: what separates a geodesic from a curve that merely joins rho0 to rho1, per time node.

On an exact W2 geodesic the kinetic energy of every time layer equals W2^2 (constant speed), the centre of mass moves on
a straight line at constant momentum, the second moment is a parabola in t, the entropy is convex in t (displacement
convexity) and the density's maximum stays below the larger of its ends.  include/dotsocp.h (dotsocp_geodesic_profile)
states the eleven layer sums and csrc/geodesic_summary.h the scalars made of them; the device forms the sums in one pass
over the resident alpha (InPALMContext.geodesic(), the drivers' geodesic=True).  Here:

  layer_sums(output, dtype)            the numpy twin of the kernel, from the `output` dict of the drivers / outputs()
  summarize(sums, rho_max, n_support, n_layer_nodes)     the twin of geodesic_summary.h, operation for operation
  geodesic_profile(output, dtype)      summarize(*layer_sums(output, dtype))
  from_struct(...)                     the same GeodesicProfile from what the C call filled

A GeodesicProfile is a dict: the fields of the C struct (nt, n_nodes, cost, energy_min, energy_max, speed_spread,
com_defect, momentum_defect, entropy_defect, peak_excess, nonfinite), one array of nt layer means per name in NAMES (each
layer sum divided by ny*nx), cx, cy (the centre of mass), rho_max, n_support, and `sums`, the (nt, 11) layer sums as they
were added; methods summary() and table().

NaN rule (geodesic_summary.h): every maximum / minimum is `(d > m or d != d) ? d : m` -- it takes a NaN when it meets one
and keeps it; a guard `c > 0 ? a : b` takes b for a NaN c."""
import numpy as np

from . import capi

NAMES = ("mass", "mx", "my", "mxx", "myy", "mxy", "px", "py", "kin", "ent", "sq")
RHO_FLOOR = capi.REPORT_RHO_FLOOR
SCALARS = ("cost", "energy_min", "energy_max", "speed_spread", "com_defect", "momentum_defect", "entropy_defect", "peak_excess")
KIN = NAMES.index("kin")


def _layers(a, N):
    return np.asarray(a).reshape((N, -1), order="F")


def layer_terms(output):
    """The eleven terms of include/dotsocp.h at every node, in float64 without contraction: a list of arrays of the shape
    of output["rho"].  X runs along the second array index (1-D: the only one), Y along the first."""
    rho = np.asarray(output["rho"], dtype=np.float64)
    Ex = np.asarray(output["Ex"], dtype=np.float64)
    one_d = "Ey" not in output
    zero = np.zeros(rho.shape)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if one_d:
            nx = rho.shape[0]
            X = (np.arange(nx, dtype=np.float64) / np.float64(nx - 1))[:, None]
            E2 = Ex * Ex
            rX = rho * X
            moments = [rX, zero, rX * X, zero, zero, Ex, zero]
        else:
            ny, nx = rho.shape[:2]
            Ey = np.asarray(output["Ey"], dtype=np.float64)
            X = (np.arange(nx, dtype=np.float64) / np.float64(nx - 1))[None, :, None]
            Y = (np.arange(ny, dtype=np.float64) / np.float64(ny - 1))[:, None, None]
            E2 = Ex * Ex + Ey ** 2
            rX, rY = rho * X, rho * Y
            moments = [rX, rY, rX * X, rY * Y, rX * Y, Ex, Ey]
        kin = np.where(rho > RHO_FLOOR, E2 / rho, 0.0)                  # the report twin's cost term
        pos = rho > 0
        ent = np.where(pos, rho * np.log(np.where(pos, rho, 1.0)), 0.0)
        return [rho] + moments + [kin, ent, rho * rho]


def layer_sums(output, dtype=np.float64):
    """(sums, rho_max, n_support, n_layer_nodes): the (nt, 11) layer sums of layer_terms() accumulated in `dtype` (the terms
    themselves are always float64; np.longdouble gives the reference the tests compare with), the largest finite rho of
    every layer (-Inf if there is none, a -0.0 counted as +0.0) and the number of its nodes with rho > RHO_FLOOR."""
    rho = np.asarray(output["rho"], dtype=np.float64)
    nt = rho.shape[-1]
    N = rho.size // nt
    sums = np.empty((nt, len(NAMES)), dtype=dtype, order="F")
    for q, term in enumerate(layer_terms(output)):
        t2 = _layers(term, N)
        sums[:, q] = (t2 if dtype == np.float64 else t2.astype(dtype)).sum(axis=0)
    r2 = _layers(rho, N)
    with np.errstate(invalid="ignore"):
        rho_max = np.where(np.isfinite(r2), r2, -np.inf).max(axis=0) + 0.0
        n_support = np.count_nonzero(r2 > RHO_FLOOR, axis=0).astype(np.int64)
    return sums, rho_max, n_support, N


def _keep_max(m, d):
    return d if (d > m or d != d) else m


def _keep_min(m, d):
    return d if (d < m or d != d) else m


class GeodesicProfile(dict):
    """The profile of one solution (module docstring)."""

    def summary(self):
        return ("geodesic: cost %.10g | energy per layer in [%.6g, %.6g], spread / cost %.3e | centre off its line %.3e, momentum off "
                "its constant %.3e | entropy concave by %.3e | peak above its ends by %.3e | %d non-finite layer(s)"
                % (self["cost"], self["energy_min"], self["energy_max"], self["speed_spread"], self["com_defect"],
                   self["momentum_defect"], self["entropy_defect"], self["peak_excess"], self["nonfinite"]))

    def table(self, bracket=None):
        """One line per time node: energy (bracket = (lower, upper): and whether it lies inside), centre of mass, second
        moment about the origin, entropy, maximum, support."""
        head = "%4s %14s %s%10s %10s %12s %14s %12s %9s" % ("t", "energy", "" if bracket is None else "%-8s" % "bracket", "cx", "cy",
                                                           "mxx + myy", "entropy", "rho max", "support")
        rows = [head]
        for t in range(int(self["nt"])):
            e = float(self["kin"][t])
            where = "" if bracket is None else "%-8s" % ("inside" if bracket[0] <= e <= bracket[1] else ("below" if e < bracket[0] else "above"))
            rows.append("%4d %14.8g %s%10.6f %10.6f %12.8f %14.8g %12.6g %9d"
                        % (t, e, where, self["cx"][t], self["cy"][t], self["mxx"][t] + self["myy"][t], self["ent"][t],
                           self["rho_max"][t], self["n_support"][t]))
        return "\n".join(rows)


def summarize(sums, rho_max, n_support, n_layer_nodes):
    """csrc/geodesic_summary.h restated with numpy float64 scalars, operation for operation: the same bits.  sums: (nt, 11)
    layer sums as added (not divided); rho_max, n_support: nt each; n_layer_nodes = ny * nx."""
    sums = np.asfortranarray(sums, dtype=np.float64)
    rho_max = np.asarray(rho_max, dtype=np.float64)
    nt = sums.shape[0]
    N = np.float64(n_layer_nodes)
    f = np.float64
    with np.errstate(all="ignore"):
        mean = sums / N
        a = {k: mean[:, q] for q, k in enumerate(NAMES)}
        n_nodes = int(n_layer_nodes) * nt
        cost = f(0.0)
        for s in sums[:, KIN]:                                          # the report's formula, its order
            cost = cost + s
        cost = cost / f(n_nodes)
        emin = emax = a["kin"][0]
        for t in range(1, nt):
            emin, emax = _keep_min(emin, a["kin"][t]), _keep_max(emax, a["kin"][t])
        spread = (emax - emin) / cost if cost > 0 else f(0.0)
        e = nt - 1
        cx, cy = a["mx"] / a["mass"], a["my"] / a["mass"]
        gx, gy = a["mx"][e] - a["mx"][0], a["my"][e] - a["my"][0]
        com, mom, peak, bad = f(0.0), f(0.0), rho_max[0], 0
        for t in range(nt):
            s = f(t) / f(nt - 1)
            dx = cx[t] - ((1 - s) * cx[0] + s * cx[e])
            dy = cy[t] - ((1 - s) * cy[0] + s * cy[e])
            com = _keep_max(com, np.sqrt(dx * dx + dy * dy))
            ex, ey = a["px"][t] - gx, a["py"][t] - gy
            mom = _keep_max(mom, np.sqrt(ex * ex + ey * ey))
            peak = _keep_max(peak, rho_max[t])
            bad += not np.isfinite(a["mass"][t])
        ent = f(0.0)
        for t in range(1, nt - 1):
            ent = _keep_max(ent, -((a["ent"][t - 1] + a["ent"][t + 1]) - 2 * a["ent"][t]))
        excess = _keep_max(f(0.0), peak - _keep_max(rho_max[0], rho_max[e]))
    out = GeodesicProfile(nt=nt, n_nodes=n_nodes, cost=float(cost), energy_min=float(emin), energy_max=float(emax),
                          speed_spread=float(spread), com_defect=float(com), momentum_defect=float(mom), entropy_defect=float(ent),
                          peak_excess=float(excess), nonfinite=int(bad), cx=cx, cy=cy, rho_max=rho_max,
                          n_support=np.asarray(n_support, dtype=np.int64), sums=sums)
    out.update(a)
    return out


def geodesic_profile(output, dtype=np.float64):
    """numpy twin of dotsocp_geodesic_profile, from the `output` dict of the drivers / InPALMContext.outputs() (rho, Ex[, Ey];
    other keys are not read).  Its `cost` has the bits of report.solution_report(output)["cost"], its `mass` those of that
    report's layer_mass."""
    return summarize(*layer_sums(output, dtype))


def from_struct(res, sums, rho_max, n_support, n_layer_nodes):
    """GeodesicProfile from a capi.Geodesic filled by dotsocp_geodesic_profile and its three arrays: the arrays of the summary
    restated here, the scalars as the library formed them"""
    out = summarize(sums, rho_max, n_support, n_layer_nodes)
    out.update(nt=int(res.nt), n_nodes=int(res.n_nodes), nonfinite=int(res.nonfinite), **{k: float(getattr(res, k)) for k in SCALARS})
    return out
