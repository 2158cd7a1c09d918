"""Judging a solution: mass conservation, negative densities, violation of f(q) <= 0, transport cost.

Host twins (numpy, no plotting) of what the reference's demos run on the outputs of a solve --
utils/check_massConservation.m:16-27, utils/hist_positive_value.m:28-55, utils/hist_negative_density.m:14,
utils/hist_violation_q_1d.m:4, utils/hist_violation_q_2d.m:4 -- and the dict form of the device-side report
(include/dotsocp.h: dotsocp_solution_report; InPALMContext.report(), the drivers' report=True), which forms the same
numbers in one pass over the device-resident state instead of downloading six grid-sized arrays.

Both `solution_report(output)` and `InPALMContext.report()` return a SolutionReport: a dict with the fields of the C
struct (n_nodes, n_cells, mass_err, neg_err, rho_min, rho_neg, rho_hist, fq_max, fq_pos, fq_hist, cost, nonfinite) plus
layer_mass and layer_neg, and the methods mass_ok(tol) and summary().
"""
import numpy as np

from . import capi

BINS = capi.REPORT_BINS
RHO_FLOOR = capi.REPORT_RHO_FLOOR


def report_edges():
    """The 50 bin edges 10.^linspace(-8, -1, 50) of hist_positive_value.m:28-30, as the library computes them once on the
    host (dotsocp_report_edges; no device needed): the device kernel and the twins below bin against the same doubles."""
    e = np.empty(BINS + 1)
    capi.check(capi.lib().dotsocp_report_edges(capi.fptr(e)))
    return e


def _bin_counts(y, edges):
    """MATLAB histcounts(y, edges): bin j counts edges[j] <= y < edges[j+1], the last bin also y == edges[-1]; values
    outside [edges[0], edges[-1]] and non-finite ones are in no bin.  Compared on y itself, not on log10(y)."""
    y = np.asarray(y, dtype=np.float64).ravel()
    with np.errstate(invalid="ignore"):
        y = y[(y >= edges[0]) & (y <= edges[-1])]              # (a NaN fails both comparisons)
    j = np.minimum(np.searchsorted(edges, y, side="right") - 1, len(edges) - 2)
    return np.bincount(j, minlength=len(edges) - 1).astype(np.int64)


def hist_positive_value(y):
    """hist_positive_value.m:30-55 without the figure: counts per bin, proportion = counts / numel(y) (histcounts'
    'probability' normalisation counts the values outside the bins too), cumulative = cumsum(proportion, 'reverse'),
    levels = the bin midpoints on the log10 axis (movmean(levels, 2, 'Endpoints', 'discard'))."""
    y = np.asarray(y, dtype=np.float64)
    edges = report_edges()
    counts = _bin_counts(y, edges)
    proportion = counts / float(y.size)
    lv = np.log10(edges)
    return dict(counts=counts, proportion=proportion, cumulative=np.cumsum(proportion[::-1])[::-1],
                levels=(lv[:-1] + lv[1:]) / 2)


def hist_negative_density(rho):
    """hist_negative_density.m:14: the histogram of -rho"""
    return hist_positive_value(-np.asarray(rho, dtype=np.float64))


def violation_q(q0, bx, by=None):
    """f(q) of hist_violation_q_2d.m:4, or of hist_violation_q_1d.m:4 when there is no by"""
    q0, bx = np.asarray(q0, dtype=np.float64), np.asarray(bx, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if by is None:
            return (q0 + .5 * bx ** 2) / (1 + np.abs(q0) + np.abs(bx))
        by = np.asarray(by, dtype=np.float64)
        return (q0 + .5 * (bx ** 2 + by ** 2)) / (1 + np.abs(q0) + np.sqrt(bx ** 2 + by ** 2))


def hist_violation_q_1d(q0, bx):
    return hist_positive_value(violation_q(q0, bx))


def hist_violation_q_2d(q0, bx, by):
    return hist_positive_value(violation_q(q0, bx, by))


class SolutionReport(dict):
    """The report of one solution (module docstring)."""

    def mass_ok(self, tol=1e-2):
        """check_massConservation.m:27-34: max(mass_err, neg_err) <= tol (False if either is a NaN)"""
        return bool(self["mass_err"] <= tol and self["neg_err"] <= tol)

    def summary(self):
        return ("report: mass err %.3e, negative mass %.3e | rho min %.3e, %d of %d nodes < 0 | f(q) max %.3e, %d of %d "
                "cells > 0 | cost %.10g | %d non-finite"
                % (self["mass_err"], self["neg_err"], self["rho_min"], self["rho_neg"], self["n_nodes"], self["fq_max"],
                   self["fq_pos"], self["n_cells"], self["cost"], self["nonfinite"]))


def solution_report(output):
    """numpy twin of dotsocp_solution_report, from the `output` dict of the drivers / InPALMContext.outputs()
    (rho, Ex[, Ey], q0, bx[, by]; 1-D outputs have no Ey / by)."""
    rho = np.asarray(output["rho"], dtype=np.float64)
    nt = rho.shape[-1]
    N = rho.size // nt
    one_d = "Ey" not in output
    edges = report_edges()
    layers = lambda a: np.asarray(a).reshape((N, -1), order="F")         # noqa: E731
    r2 = layers(rho)
    with np.errstate(invalid="ignore"):
        neg = r2 < 0
    layer_mass = r2.sum(axis=0) / N
    layer_neg = np.where(neg, r2, 0.0).sum(axis=0) / N
    Ex = np.asarray(output["Ex"], dtype=np.float64)
    E2 = Ex * Ex if one_d else Ex * Ex + np.asarray(output["Ey"], dtype=np.float64) ** 2
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        term = np.where(rho > RHO_FLOOR, E2 / rho, 0.0)
    cost = 0.0
    for s in layers(term).sum(axis=0):                                   # layer sums, added in layer order
        cost += float(s)
    fq = violation_q(output["q0"], output["bx"], None if one_d else output["by"])
    rho_ok, fq_ok = np.isfinite(rho), np.isfinite(fq)
    with np.errstate(invalid="ignore"):
        fq_pos = int(np.count_nonzero(fq > 0))
    return SolutionReport(
        n_nodes=int(rho.size), n_cells=int(fq.size),
        mass_err=float(np.max(np.abs(layer_mass - 1))), neg_err=float(np.max(np.abs(layer_neg))),     # (np.max keeps a NaN)
        rho_min=float(rho[rho_ok].min() + 0.0) if rho_ok.any() else float("inf"), rho_neg=int(np.count_nonzero(neg)),
        rho_hist=_bin_counts(-rho, edges),
        fq_max=float(fq[fq_ok].max() + 0.0) if fq_ok.any() else float("-inf"), fq_pos=fq_pos,
        fq_hist=_bin_counts(fq, edges),
        cost=cost / rho.size, nonfinite=int(rho.size - np.count_nonzero(rho_ok) + fq.size - np.count_nonzero(fq_ok)),
        layer_mass=layer_mass, layer_neg=layer_neg)


def from_struct(rep, layer_mass, layer_neg):
    """SolutionReport from a capi.Report filled by dotsocp_solution_report and its two layer arrays"""
    return SolutionReport(
        n_nodes=int(rep.n_nodes), n_cells=int(rep.n_cells), mass_err=float(rep.mass_err), neg_err=float(rep.neg_err),
        rho_min=float(rep.rho_min), rho_neg=int(rep.rho_neg), rho_hist=np.array(rep.rho_hist[:], dtype=np.int64),
        fq_max=float(rep.fq_max), fq_pos=int(rep.fq_pos), fq_hist=np.array(rep.fq_hist[:], dtype=np.int64),
        cost=float(rep.cost), nonfinite=int(rep.nonfinite), layer_mass=layer_mass, layer_neg=layer_neg)
