"""The early cone pass: the q-step of an iteration whose own cone pass left gamma also runs the NEXT iteration's
gamma-reading pass, in one kernel, on the q it holds in registers (qstep_march.hip: k_qcone; Solver::step schedules it,
solver.h).  The steady form does not store q at all, the exit form stores q and beta for the readers behind it.

Every entry gets the arithmetic of the unfused pair of kernels in the same order, so DOTSOCP_QCONE=1 (fuse wherever
the schedule allows, whatever the grid size) must reproduce DOTSOCP_QCONE=0 (the two kernels, a launch each) TO THE
BIT: the five fields, sigma, cScale / dScale and the whole KKT history -- for every chunk length of the fused march
(DOTSOCP_QCONE_TC), across rescales, norm checks, run() calls in pieces and the time limit.  Weighted problems and time
slabs keep the two kernels.  With the switch unset only grids of at least 2048 tiles fuse: none of these."""
import numpy as np
import pytest

import dotsocp_amd as D
from oracle import driver as OD
from oracle.examples import (ensure_barrier_validity, gene_barrier_of_circle_pillar, get_example_1d,
                             get_example_2d, get_weight_by_barrier)
from oracle.inpalm import InPALMState

pytestmark = pytest.mark.gpu
FIELDS = ("phi", "q", "z", "alpha", "beta")
SWITCH = "DOTSOCP_QCONE"


def _run(rho0, rho1, nt, opts, weight=None, method="inPALM", nslabs=1, pieces=(-1,), profiling=False):
    dim = 2 if np.ndim(rho0) == 2 else 1
    var, model = D.initialize(rho0, rho1, nt)
    if weight is not None:
        model.weight = np.asarray(weight, dtype=np.float64)
    o = OD.default_opts(opts, method, weight is not None)
    D.InitialScaling(var, model, o["scaling"], None, dim=dim, weighted=weight is not None)
    ctx = D.InPALMContext(var, o, model, weighted=weight is not None, nslabs=nslabs, z_unread=True, profiling=profiling)
    try:
        for n in pieces:
            ctx.run(n)
        hist, sigma = ctx.finish()
        counts = {k: ctx.kernel_time(k)[1] for k in ("cone_fused_a", "cone_fused_b", "cone_carry", "qcone", "qstep")} \
            if profiling else None
    finally:
        ctx.close()
    return var, hist, sigma, counts


def _identical(monkeypatch, *args, **kw):
    monkeypatch.setenv(SWITCH, "0")
    ref, h0, s0, _ = _run(*args, **kw)
    monkeypatch.setenv(SWITCH, "1")
    got, h1, s1, counts = _run(*args, **kw)
    assert s1 == s0
    assert h1["len"] == h0["len"] and h0["len"] >= 1
    np.testing.assert_array_equal(h1["iter"], h0["iter"])
    np.testing.assert_array_equal(h1["kkt"], h0["kkt"])
    np.testing.assert_array_equal(h1["pdGap"], h0["pdGap"])
    assert got.cScale == ref.cScale and got.dScale == ref.dScale
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(got, f), getattr(ref, f), err_msg=f)
    return got, h1, s1, counts


SHAPES = [(32, 32, 16, 40), (100, 70, 20, 30), (65, 129, 33, 25), (63, 5, 7, 20), (5, 3, 4, 12), (2, 2, 2, 6),
          (129, 3, 5, 15)]


def _densities(ny, nx):
    if ny * nx <= 6:
        rho0 = np.ones((ny, nx))
        rho1 = np.ones((ny, nx))
        rho1.flat[0] = 1.5
        rho1 /= rho1.mean()
        return rho0, rho1
    return get_example_2d("example1", ny, nx)


@pytest.mark.parametrize("ny,nx,nt,K", SHAPES)
def test_fusion_changes_no_bit(ny, nx, nt, K, monkeypatch):
    """Tile borders in y and x, pitched rows, widths that are no multiple of the tile, one cell in t."""
    rho0, rho1 = _densities(ny, nx)
    _identical(monkeypatch, rho0, rho1, nt, dict(tol=0.0, maxit=K))


def test_fusion_changes_no_bit_1d(monkeypatch):
    r0, r1 = get_example_1d("gaussian", 129)
    _identical(monkeypatch, r0, r1, 33, dict(tol=0.0, maxit=60))


@pytest.mark.parametrize("tc", ["3", "8"])
@pytest.mark.parametrize("ny,nx,nt,K", [(100, 70, 20, 30), (65, 129, 33, 25)])
def test_chunk_length_changes_no_bit(tc, ny, nx, nt, K, monkeypatch):
    """Several chunk fronts per tile (with 3 layers per chunk one front lies two layers behind the next chunk's first
    stored layer): each chunk recomputes, without storing, the two layers in front of it."""
    monkeypatch.setenv("DOTSOCP_QCONE_TC", tc)
    rho0, rho1 = get_example_2d("example1", ny, nx)
    _identical(monkeypatch, rho0, rho1, nt, dict(tol=0.0, maxit=K))


def test_fusion_changes_no_bit_alg2_step_by_step_unscaled(monkeypatch):
    rho0, rho1 = get_example_2d("example1", 24, 40)
    _identical(monkeypatch, rho0, rho1, 12, dict(tol=0.0, maxit=40), method="ALG2")            # tau = 1
    _identical(monkeypatch, rho0, rho1, 12, dict(tol=0.0, maxit=15, ifCheckStepByStep=True))   # never fuses
    _identical(monkeypatch, rho0, rho1, 12, dict(tol=0.0, maxit=20, scaling=False, sigma=0.1))


def test_weighted_problems_and_time_slabs_keep_the_two_kernels(monkeypatch):
    rho0, rho1 = get_example_2d("example1", 33, 47)
    barrier = gene_barrier_of_circle_pillar()
    weight = get_weight_by_barrier(47, 33, 13, barrier)
    rho0, rho1, _ = ensure_barrier_validity(rho0, rho1, barrier)
    counts = _identical(monkeypatch, rho0, rho1, 13, dict(tol=0.0, maxit=25), weight=weight, profiling=True)[3]
    assert counts["qcone"] == 0 and counts["qstep"] == 25
    rho0, rho1 = get_example_2d("example1", 64, 48)
    counts = _identical(monkeypatch, rho0, rho1, 24, dict(tol=0.0, maxit=30), nslabs=2, profiling=True)[3]
    assert counts["qcone"] == 0


@pytest.mark.parametrize("ny,nx,nt,K,sigma0", [(32, 32, 16, 230, 1.0), (16, 16, 8, 320, 0.01)])
def test_fusion_changes_no_bit_across_rescales_and_norm_checks(ny, nx, nt, K, sigma0, monkeypatch):
    """Both rescales and the norm checks of iterations 100, 200, 300: the iteration in front of each of them takes the
    exit form at the latest, so beta and q are in memory for them."""
    rho0, rho1 = get_example_2d("example1", ny, nx)
    _identical(monkeypatch, rho0, rho1, nt, dict(tol=0.0, maxit=K, sigma=sigma0))


def test_run_in_pieces_is_one_run(monkeypatch):
    """run(7); run(5); run(-1): no early pass crosses the end of a run() call, and the trajectory is that of one run(-1)."""
    rho0, rho1 = get_example_2d("example1", 40, 24)
    opts = dict(tol=0.0, maxit=40)
    whole = _identical(monkeypatch, rho0, rho1, 12, opts)
    parts = _identical(monkeypatch, rho0, rho1, 12, opts, pieces=(7, 5, -1))
    assert parts[2] == whole[2]
    np.testing.assert_array_equal(parts[1]["kkt"], whole[1]["kkt"])
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(parts[0], f), getattr(whole[0], f), err_msg=f)


def test_time_limit_with_the_fusion_on(monkeypatch):
    """The time-out predicate is evaluated in front of the q-step as well: iteration 6 (the entry pass, which leaves
    gamma) sees the limit passed and issues no early pass, iteration 7 checks and stops -- as without the fusion."""
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.setenv("DOTSOCP_TEST_TIMEOUT_AT", "6")
    rho0, rho1 = get_example_2d("example1", 32, 32)
    var, hist, _, _ = _run(rho0, rho1, 16, dict(tol=0.0, maxit=50))
    assert list(hist["iter"]) == [1, 4, 7]
    for f in FIELDS:
        assert np.all(np.isfinite(getattr(var, f))), f


def test_fused_launches_are_a_phase_of_their_own(monkeypatch):
    """Profiling: a fused launch is the phase "qcone" and neither "qstep" nor "cone_carry", so one cone phase and one
    q-step phase are counted per iteration either way.  Unset, the switch leaves a grid of 16 tiles alone."""
    K = 40
    rho0, rho1 = get_example_2d("example1", 64, 64)
    monkeypatch.setenv(SWITCH, "1")
    c = _run(rho0, rho1, 16, dict(tol=0.0, maxit=K), profiling=True)[3]
    print("forced:", c)
    assert c["cone_fused_a"] + c["cone_fused_b"] + c["cone_carry"] + c["qcone"] == K
    assert c["qstep"] + c["qcone"] == K
    assert c["qcone"] >= 1
    monkeypatch.delenv(SWITCH)
    c = _run(rho0, rho1, 16, dict(tol=0.0, maxit=K), profiling=True)[3]
    assert c["qcone"] == 0 and c["qstep"] == K


def test_schedule_alone_with_the_two_kernels_back_to_back(monkeypatch):
    """DOTSOCP_QCONE=2: the same host schedule, the early pass as the unfused kernels launched one behind the other."""
    rho0, rho1 = get_example_2d("example1", 100, 70)
    opts = dict(tol=0.0, maxit=30)
    monkeypatch.setenv(SWITCH, "0")
    ref, h0, s0, _ = _run(rho0, rho1, 20, opts)
    monkeypatch.setenv(SWITCH, "2")
    got, h1, s1, _ = _run(rho0, rho1, 20, opts)
    assert s1 == s0
    np.testing.assert_array_equal(h1["kkt"], h0["kkt"])
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(got, f), getattr(ref, f), err_msg=f)


def test_forced_fusion_against_the_oracle(monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    ny, nx, nt, K = 64, 64, 32, 120
    rho0, rho1 = get_example_2d("example1", ny, nx)
    opts = dict(tol=0.0, maxit=K)
    ovar, omodel, oo = OD.make_level(rho0, rho1, nt, opts, "inPALM", None)
    st = InPALMState(ovar, oo, omodel)
    st.run()
    o_hist, o_sigma = st.finish()
    gvar, g_hist, g_sigma, _ = _run(rho0, rho1, nt, opts)
    assert g_hist["len"] == o_hist["len"]
    np.testing.assert_array_equal(g_hist["iter"], o_hist["iter"])
    assert abs(g_sigma - o_sigma) <= 1e-12 * abs(o_sigma)
    np.testing.assert_allclose(g_hist["kkt"], o_hist["kkt"], rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(g_hist["pdGap"], o_hist["pdGap"], rtol=1e-6, atol=1e-14)
    errs = {f: np.max(np.abs(getattr(gvar, f) - getattr(ovar, f))) / np.max(np.abs(getattr(ovar, f))) for f in FIELDS}
    print("relative errors against the oracle:", errs)
    assert max(errs.values()) <= 1e-9, errs
    assert abs(gvar.cScale - ovar.cScale) <= 1e-12 * ovar.cScale and abs(gvar.dScale - ovar.dScale) <= 1e-12 * ovar.dScale

