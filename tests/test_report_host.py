"""Host side of the solution report (dot-socp_amd/report.py, include/dotsocp.h: dotsocp_solution_report): the exported
symbols, the bin edges, the bin semantics of MATLAB's histcounts, the numpy twin on a hand-made output, mass_ok against
check_massConservation, the 1-D formula of f(q), and the drivers' argument check.  No GPU."""
import ctypes

import numpy as np
import pytest

import dotsocp_amd as D
from dotsocp_amd import capi
from dotsocp_amd import report as R


def test_library_exports_the_report_calls():
    L = capi.lib()
    assert hasattr(L, "dotsocp_solution_report") and hasattr(L, "dotsocp_report_edges")
    assert ctypes.sizeof(capi.Report) == 8 * (10 + 2 * capi.REPORT_BINS)       # ten scalars + two 49-bin histograms
    assert L.dotsocp_report_edges(None) == -1 and b"report_edges" in L.dotsocp_last_error()


def test_edges():
    e = D.report_edges()
    ref = 10.0 ** np.linspace(-8, -1, 50)
    assert e.shape == (50,) and np.all(np.diff(e) > 0)
    assert np.all(np.abs(e - ref) <= 4 * np.spacing(ref))
    assert e[0] <= 1e-8 * (1 + 1e-15) and e[-1] >= 1e-1 * (1 - 1e-15)


def test_bin_semantics():
    e = D.report_edges()
    inner = e[17]
    y = np.array([inner,                       # an inner edge: upper bin
                  e[49],                       # the last edge: last bin
                  e[0],                        # the first edge: bin 0
                  0.0, -3e-4, np.nextafter(e[0], 0), np.nextafter(e[49], 1), np.nan, np.inf, -np.inf,      # no bin
                  np.nextafter(inner, 0),      # just below the inner edge: lower bin
                  3e-5, 3e-5])
    h = D.hist_positive_value(y)
    want = np.zeros(49, dtype=np.int64)
    want[17] += 1
    want[48] += 1
    want[0] += 1
    want[16] += 1
    j = [k for k in range(49) if e[k] <= 3e-5 < e[k + 1]]
    assert len(j) == 1
    want[j[0]] += 2
    assert h["counts"].dtype == np.int64 and np.array_equal(h["counts"], want)
    assert np.array_equal(h["proportion"], want / y.size)                       # normalised by numel(y), not by the binned ones
    assert np.allclose(h["cumulative"], np.cumsum((want / y.size)[::-1])[::-1], rtol=0, atol=1e-15)
    assert h["cumulative"][0] == pytest.approx(6 / y.size)
    assert h["levels"].shape == (49,) and np.allclose(h["levels"], -8 + (np.arange(49) + .5) / 7, rtol=0, atol=1e-12)
    # hist_negative_density bins -rho
    assert np.array_equal(D.hist_negative_density(-y)["counts"], want)


def _hand_output():
    ny, nx, nt = 5, 4, 3
    rho = np.ones((ny, nx, nt), order="F")
    rho[:, :, 2] = 1.25
    rho[0, 0, 1] = -0.5
    rho[3, 0, 1] = -2e-3
    rho[1, 0, 1] = 5e-9                  # <= floor: no cost term
    rho[2, 0, 1] = 4.502 - 5e-9          # layer 1 sums to 20 exactly up to rounding
    Ex = np.full((ny, nx, nt), 2.0, order="F")
    Ey = np.zeros((ny, nx, nt), order="F")
    Ex[2, 0, 1] = 0.0
    Ex[1, 0, 1] = 7.0                    # at the floor node: must not count
    Ey[4, 3, 0] = 1.0
    q0 = np.full((ny, nx, nt - 1), -1.0, order="F")
    bx = np.zeros((ny, nx, nt - 1), order="F")
    by = np.zeros((ny, nx, nt - 1), order="F")
    q0[1, 1, 0], bx[1, 1, 0], by[1, 1, 0] = 0.0, 0.3, 0.4
    q0[2, 2, 1] = np.nan
    return dict(rho=rho, Ex=Ex, Ey=Ey, q0=q0, bx=bx, by=by)


def _bin_of(v):
    e = D.report_edges()
    j = [k for k in range(49) if e[k] <= v < e[k + 1]]
    assert len(j) == 1
    return j[0]


def test_solution_report_by_hand():
    out = _hand_output()
    r = D.solution_report(out)
    assert isinstance(r, dict) and r["n_nodes"] == 60 and r["n_cells"] == 40
    assert np.allclose(r["layer_mass"], [1.0, 1.0, 1.25], rtol=0, atol=1e-15)
    assert np.allclose(r["layer_neg"], [0.0, -0.502 / 20, 0.0], rtol=0, atol=1e-17)
    assert r["mass_err"] == pytest.approx(0.25, abs=1e-15) and r["neg_err"] == pytest.approx(0.0251, abs=1e-17)
    assert r["rho_min"] == -0.5 and r["rho_neg"] == 2
    want = np.zeros(49, dtype=np.int64)
    want[_bin_of(2e-3)] = 1                                           # 0.5 lies above the last edge
    assert np.array_equal(r["rho_hist"], want)
    # cost: layer 0: 19 * 4 + 5, layer 1: 16 * 4 (two negative nodes, the floor node and the E = 0 node add nothing), layer 2: 20 * 4 / 1.25
    assert r["cost"] == pytest.approx((81 + 64 + 64) / 60, rel=1e-15)
    fq = (.5 * (0.3 ** 2 + 0.4 ** 2)) / (1 + np.sqrt(0.3 ** 2 + 0.4 ** 2))
    assert r["fq_max"] == pytest.approx(fq, rel=1e-15) and r["fq_pos"] == 1 and r["nonfinite"] == 1
    want = np.zeros(49, dtype=np.int64)
    want[_bin_of(fq)] = 1
    assert np.array_equal(r["fq_hist"], want)
    assert "mass err" in r.summary()


@pytest.mark.parametrize("tol", [1e-2, 1e-6])
def test_mass_ok_agrees_with_check_massConservation(tol):
    out = _hand_output()
    assert D.solution_report(out).mass_ok(tol) == D.check_massConservation(out["rho"], tol) is False
    good = dict(out, rho=np.ones((5, 4, 3), order="F"))
    good["rho"][1, 1, 1] -= 1e-5                                      # layer mean off by 5e-7: passes 1e-2 and 1e-6
    good["rho"][2, 2, 2] += 1e-3                                      # 5e-5: passes 1e-2 only
    r = D.solution_report(good)
    assert r.mass_ok(tol) == D.check_massConservation(good["rho"], tol) == (tol == 1e-2)
    assert r.mass_ok() is True                                        # default tolerance 1e-2
    bad = dict(out, rho=out["rho"].copy(order="F"))
    bad["rho"][0, 1, 1] = np.nan                                      # a NaN layer is not a conserved one
    r = D.solution_report(bad)
    assert r.mass_ok(tol) is False and D.check_massConservation(bad["rho"], tol) is False
    assert r["nonfinite"] == 2 and r["rho_min"] == -0.5


def test_fq_1d_uses_abs_not_sqrt():
    q0 = np.array([[-1.0, 0.25], [0.0, -3.0]])
    bx = np.array([[-0.5, 3e-170], [2.0, 1e-3]])
    got = R.violation_q(q0, bx)
    assert np.array_equal(got, (q0 + .5 * bx * bx) / (1 + np.abs(q0) + np.abs(bx)))
    assert got[0, 1] == 0.25 / (1.25 + 3e-170)                        # sqrt(bx^2) would have lost the 3e-170
    out = dict(rho=np.ones((2, 3)), Ex=np.zeros((2, 3)), q0=q0, bx=bx)
    r = D.solution_report(out)
    assert r["n_cells"] == 4 and r["fq_max"] == got.max() and r["fq_pos"] == int((got > 0).sum())
    assert np.array_equal(D.hist_violation_q_1d(q0, bx)["counts"], r["fq_hist"])


@pytest.mark.parametrize("driver", ["solver_dotsocp2d", "solver_dotsocp1d", "solver_wdotsocp2d"])
def test_report_needs_the_device_transfer(driver):
    """ValueError before any device call (on a box without a GPU a device call would raise a DotsocpError instead)"""
    if driver == "solver_dotsocp1d":
        rho0, rho1 = D.get_example_1d("gaussian", 17)
    else:
        rho0, rho1 = D.get_example_2d("example1", 9, 9)
    opts = dict(tol=1e-3, maxit=5)
    if driver == "solver_wdotsocp2d":
        opts["weight"] = np.ones(9 * 9 * 4 + 9 * 8 * 5 + 8 * 9 * 5)
    with pytest.raises(ValueError, match="report"):
        getattr(D, driver)(rho0, rho1, 5, 1, opts, transfer="host", report=True)
