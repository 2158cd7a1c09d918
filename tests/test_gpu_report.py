"""The solution report on the device (csrc/report.hip, dotsocp_solution_report, InPALMContext.report()) against its numpy
twin (report.solution_report) applied to ctx.outputs() of the SAME context.

States are made here: alpha and q entries s * 10^u (s = +-1, u uniform in [-10, 1], seeded), rho0 / rho1 positive with a
few exact zeros; uploaded, begin(), no iteration, finish().  Before a device report is looked at, the recovered fields are
checked to exercise the binning: nearly every bin of both histograms occupied, values below the first and above the last
edge, a density at or below the cost floor.  (The 3 x 3 x 2 grid cannot meet that by counting -- 18 nodes, all of them on
the first or last layer, 9 cells -- so it is compared with the twin only.)

Integer fields, histograms, min(rho) and max(fq) must agree exactly; the layer means and the cost within the classical
bound for summing N terms in any order, taken once for each side: 2 N 2^-53 mean|term|."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dotsocp_amd as D
from dotsocp_amd import capi
from dotsocp_amd import report as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53

# name: (ny, nx, nt, weighted, least number of occupied bins per histogram or None); 1-D: ny = None
CASES = {
    "2d_19x13x6": (19, 13, 6, False, 45),
    "2d_33x17x9": (33, 17, 9, False, 45),
    "2d_3x3x2": (3, 3, 2, False, None),
    "1d_301x9": (None, 301, 9, False, 40),
    "w_17x21x5": (17, 21, 5, True, 45),
    "2d_19x13x7": (19, 13, 7, False, 45),
}
INTS = ("n_nodes", "n_cells", "rho_neg", "fq_pos", "nonfinite")


def _signed_pow(rng, n):
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-10, 1, n)


def _density(rng, shape):
    r = rng.uniform(0.5, 1.5, shape)
    r.flat[rng.choice(r.size, 3, replace=False)] = 0.0
    return r


def _context(case, nan=False, **split):
    """A finished context on the generic state of `case` (no iteration)"""
    ny, nx, nt, weighted, _ = CASES[case]
    rng = np.random.default_rng(sorted(CASES).index(case) + 20260)
    shape = (nx,) if ny is None else (ny, nx)
    var, model = D.initialize(_density(rng, shape), _density(rng, shape), nt)
    nq = var.q.size
    if weighted:
        # in [0.5, 1e6], most entries of order one, a few huge (a weight that is large everywhere lifts every density of
        # this small grid above the first bins)
        model.weight = 0.5 + (1e6 - 0.5) * rng.uniform(0, 1, nq) ** 32
    # (and the weighted state stays unscaled, for the same reason: its D follows the mean of log10(weight))
    D.InitialScaling(var, model, not weighted, None, dim=1 if ny is None else 2, weighted=weighted)
    var.q, var.alpha = _signed_pow(rng, nq), _signed_pow(rng, nq)
    if nan:
        plane = nx * (ny or 1)
        var.alpha[plane * (nt // 2) + plane // 2] = np.nan              # an alpha0 entry of an inner cell layer
        var.q[var.qInd.bx + plane // 3] = np.nan                        # an edge entry of q
    opts = dict(tau=1.9, sigma=1.0, tol=0.0, maxit=1, ifCheckStepByStep=False, scaling=True)
    ctx = D.InPALMContext(var, opts, model, weighted=weighted, **split)
    ctx.finish(download=False)
    return ctx


def _raw_report(ctx):
    """(SolutionReport, bytes of the struct and of both layer arrays) straight from the C call"""
    m = ctx.model
    r0, r1 = np.asfortranarray(m.rho0, dtype=np.float64), np.asfortranarray(m.rho1, dtype=np.float64)
    rep, mass, neg = capi.Report(), np.empty(int(m.nt)), np.empty(int(m.nt))
    capi.check(capi.lib().dotsocp_solution_report(ctx._ctx, capi.fptr(r0), capi.fptr(r1), ctypes.byref(rep),
                                                  capi.fptr(mass), capi.fptr(neg)))
    return R.from_struct(rep, mass, neg), bytes(rep) + mass.tobytes() + neg.tobytes()


def _layers(a):
    return np.asarray(a).reshape((-1, a.shape[-1]), order="F")


def _conditions(out, min_bins):
    """The recovered fields exercise the binning (module docstring); asserted before the device report is read"""
    e = D.report_edges()
    rho = out["rho"]
    fq = R.violation_q(out["q0"], out["bx"], out.get("by"))
    for name, y, counts in (("rho", -rho, D.hist_negative_density(rho)["counts"]), ("fq", fq, D.hist_positive_value(fq)["counts"])):
        assert np.count_nonzero(counts) >= min_bins, (name, np.count_nonzero(counts))
        assert np.count_nonzero((y > 0) & (y < e[0])) >= 1, name
        assert np.count_nonzero(y > e[-1]) >= 1, name
    assert np.count_nonzero(rho <= R.RHO_FLOOR) >= 1


def _cost_terms(out):
    E2 = out["Ex"] ** 2 + (out["Ey"] ** 2 if "Ey" in out else 0.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.where(out["rho"] > R.RHO_FLOOR, E2 / out["rho"], 0.0)


def _same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _assert_matches(dev, out, sums=True):
    twin = D.solution_report(out)
    for k in INTS:
        print(k, dev[k], twin[k])
        assert dev[k] == twin[k], k
    assert np.array_equal(dev["rho_hist"], twin["rho_hist"]) and np.array_equal(dev["fq_hist"], twin["fq_hist"])
    assert dev["rho_hist"].sum() <= dev["rho_neg"] and dev["fq_hist"].sum() <= dev["fq_pos"]
    print("rho_min", dev["rho_min"], twin["rho_min"], "fq_max", dev["fq_max"], twin["fq_max"])
    assert _same_bits(dev["rho_min"], twin["rho_min"]) and _same_bits(dev["fq_max"], twin["fq_max"])
    if not sums:
        return twin
    rho2 = _layers(out["rho"])
    N = rho2.shape[0]
    bound = 2 * N * U * np.abs(rho2).mean(axis=0)
    for k in ("layer_mass", "layer_neg"):
        d = np.abs(dev[k] - twin[k])
        print(k, "worst difference / bound", np.max(d / bound))
        assert np.all(d <= bound), k
    assert _same_bits(dev["mass_err"], np.max(np.abs(dev["layer_mass"] - 1)))
    assert _same_bits(dev["neg_err"], np.max(np.abs(dev["layer_neg"])))
    cbound = 2 * dev["n_nodes"] * U * np.abs(_cost_terms(out)).mean()
    print("cost", dev["cost"], twin["cost"], "difference / bound", abs(dev["cost"] - twin["cost"]) / cbound)
    assert abs(dev["cost"] - twin["cost"]) <= cbound
    assert dev.mass_ok() == twin.mass_ok() == D.check_massConservation(out["rho"], 1e-2)
    return twin


_one_slab = {}


def _one_slab_run(case):
    """(report, its bytes, the bytes of a second call, outputs) of the one-slab context of `case`, made once"""
    if case not in _one_slab:
        ctx = _context(case)
        try:
            out = ctx.outputs()
            dev, raw = _raw_report(ctx)
            _one_slab[case] = (dev, raw, _raw_report(ctx)[1], out, ctx.report())
        finally:
            ctx.close()
    return _one_slab[case]


@pytest.mark.parametrize("case", [c for c in CASES if c != "2d_19x13x7"])
def test_report_equals_the_twin(case):
    dev, raw, again, out, via_method = _one_slab_run(case)
    if CASES[case][4] is not None:
        _conditions(out, CASES[case][4])
    _assert_matches(dev, out)
    assert raw == again                                             # two consecutive calls: identical bytes
    assert _same_bits(via_method["cost"], dev["cost"]) and np.array_equal(via_method["layer_mass"], dev["layer_mass"])


@pytest.mark.parametrize("nslabs", [2, 3])
def test_time_slabs_give_the_same_bytes(nslabs):
    case = "2d_19x13x7"
    dev, raw, again, out, _ = _one_slab_run(case)
    _conditions(out, CASES[case][4])
    _assert_matches(dev, out)
    assert raw == again
    ctx = _context(case, nslabs=nslabs)
    try:
        sdev, sraw = _raw_report(ctx)
        sout = ctx.outputs()
    finally:
        ctx.close()
    for k in out:
        assert np.array_equal(out[k], sout[k]), k
    assert sraw == raw
    _assert_matches(sdev, sout)


def test_slabs_on_their_own_streams_give_the_same_bytes():
    """dotsocp_create_multi (every slab with its own pair of streams)"""
    case = "2d_19x13x7"
    raw = _one_slab_run(case)[1]
    ctx = _context(case, ngpu=3)
    try:
        assert _raw_report(ctx)[1] == raw
    finally:
        ctx.close()


def test_planted_nans():
    ctx = _context("2d_19x13x6", nan=True)
    try:
        out = ctx.outputs()
        dev, _ = _raw_report(ctx)
    finally:
        ctx.close()
    n_bad = np.count_nonzero(~np.isfinite(out["rho"])) + np.count_nonzero(~np.isfinite(R.violation_q(out["q0"], out["bx"], out["by"])))
    assert np.count_nonzero(~np.isfinite(out["rho"])) >= 1 and n_bad >= 2
    twin = _assert_matches(dev, out, sums=False)
    assert dev["nonfinite"] == n_bad == twin["nonfinite"]
    assert np.isfinite(dev["rho_min"]) and np.isfinite(dev["fq_max"])
    clean = _one_slab_run("2d_19x13x6")[0]                         # same seed without the NaNs: a NaN moved counts out of bins only
    assert np.all(dev["rho_hist"] <= clean["rho_hist"]) and np.all(dev["fq_hist"] <= clean["fq_hist"])
    assert not dev.mass_ok()                                        # a layer with a NaN in it is not a conserved one


def test_errors_name_the_call():
    L = capi.lib()
    ny, nx, nt = 9, 7, 4
    rng = np.random.default_rng(5)
    var, model = D.initialize(_density(rng, (ny, nx)), _density(rng, (ny, nx)), nt)
    D.InitialScaling(var, model, True, None, dim=2)
    ctx = D.InPALMContext(var, dict(tau=1.9, sigma=1.0, tol=0.0, maxit=1, scaling=True), model)
    try:
        with pytest.raises(capi.DotsocpError) as ei:
            ctx.report()
        assert ei.value.code == -4 and "solution_report" in str(ei.value)          # DOTSOCP_ESTATE
        ctx.finish(download=False)
        r0, r1 = np.asfortranarray(model.rho0), np.asfortranarray(model.rho1)
        rep = capi.Report()
        assert L.dotsocp_solution_report(ctx._ctx, None, capi.fptr(r1), ctypes.byref(rep), None, None) == -1
        assert b"solution_report" in L.dotsocp_last_error()
        assert L.dotsocp_solution_report(ctx._ctx, capi.fptr(r0), capi.fptr(r1), None, None, None) == -1
        assert b"solution_report" in L.dotsocp_last_error()
        assert L.dotsocp_solution_report(ctx._ctx, capi.fptr(r0), capi.fptr(r1), ctypes.byref(rep), None, None) == 0   # layer arrays may be NULL
        assert rep.n_nodes == ny * nx * nt
    finally:
        ctx.close()


def _after_solve(output):
    dev = output["report"]
    assert isinstance(dev, R.SolutionReport)
    out = {k: v for k, v in output.items() if k != "report"}
    twin = _assert_matches(dev, out)
    assert dev["nonfinite"] == 0 and twin["nonfinite"] == 0
    assert dev.mass_ok() == D.check_massConservation(out["rho"])


def test_driver_2d_reports_after_a_real_solve():
    rho0, rho1 = D.get_example_2d("example1", 33, 33)
    output = D.solver_dotsocp2d(rho0, rho1, 9, 2, dict(tol=1e-4, maxit=60), report=True)[0]
    _after_solve(output)
    plain = D.solver_dotsocp2d(rho0, rho1, 9, 2, dict(tol=1e-4, maxit=60))[0]          # the default path has no report and the same outputs
    assert "report" not in plain and all(np.array_equal(plain[k], output[k]) for k in plain)


def test_driver_1d_reports_after_a_real_solve():
    rho0, rho1 = D.get_example_1d("gaussian", 129)
    _after_solve(D.solver_dotsocp1d(rho0, rho1, 17, 2, dict(tol=1e-4, maxit=60), report=True)[0])


def test_driver_weighted_reports_after_a_real_solve():
    rho0, rho1 = D.get_example_2d("example1", 33, 33)
    weight = D.gene_space_weight_circleInv(33, 33)
    assert isinstance(weight, D.SpaceWeight)
    output = D.solver_wdotsocp2d(rho0, rho1, 9, 2, dict(tol=1e-4, maxit=60, weight=weight), weights="device", report=True)[0]
    _after_solve(output)


def _canary_child():
    """Runs in a fresh process with DOTSOCP_CANARY=1: the report's buffers lie between guard bands"""
    assert os.environ.get("DOTSOCP_CANARY") == "1"
    ctx = _context("2d_19x13x6")
    try:
        out = ctx.outputs()
        dev, _ = _raw_report(ctx)             # fails with DOTSOCP_EHIP if a band was overwritten
        assert capi.lib().dotsocp_canary_check() == 0, capi.lib().dotsocp_last_error().decode()   # the report's buffers are live here
    finally:
        ctx.close()
    _assert_matches(dev, out)
    assert capi.lib().dotsocp_canary_check() == 0
    print("canary child ok")


def test_report_between_guard_bands():
    code = "import sys; sys.path.insert(0, sys.argv[1]); import test_gpu_report as T; T._canary_child()"
    env = dict(os.environ, DOTSOCP_CANARY="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "tests")], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("canary child ok"), out.stdout[-1000:] + out.stderr[-3000:]
