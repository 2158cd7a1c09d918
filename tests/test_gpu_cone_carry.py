"""The gamma form of the cone pass and the zero interior of c.

Between two plain inPALM / ALG2 iterations the fused cone pass stores gamma^k = beta^k + tau z^{k+1} where it used to
store beta^k, and the next pass forms beta^{k+1} = gamma^k - tau (BF q^{k+1} + d) without reading q^k or projecting a
second time (fused.hip, flavours CONE_GIN / CONE_GOUT of mode 1; Solver::step schedules them).  gamma is stored as the
exact double mult_carry() returns, so a run with the flavours must reproduce the run without them
(DOTSOCP_CONE_CARRY=0: every deferred pass reads and writes beta) TO THE BIT: fields, sigma, the whole KKT history.

model.c is zero off its first and last time layer; when the device test at upload confirms that (Slab::c_ends), the
q-step, k_rhs and the sigma fix leave the interior alone.  They keep every arithmetic use of the value, so
DOTSOCP_C_ENDS=0 (load everything) must agree to the bit as well -- also for a c with a non-zero interior entry, where
the detection says no and the switch changes nothing.

One trajectory against the oracle proves the default path itself, at the tolerances of tests/test_gpu_solver.py."""
import numpy as np
import pytest

import dotsocp_amd as D
from oracle import driver as OD
from oracle.examples import (ensure_barrier_validity, gene_barrier_of_circle_pillar, get_example_1d,
                             get_example_2d, get_weight_by_barrier)
from oracle.inpalm import InPALMState

pytestmark = pytest.mark.gpu
FIELDS = ("phi", "q", "z", "alpha", "beta")


def _run(rho0, rho1, nt, opts, weight=None, method="inPALM", nslabs=1, ngpu=None, pieces=(-1,), poke_c=None):
    dim = 2 if np.ndim(rho0) == 2 else 1
    var, model = D.initialize(rho0, rho1, nt)
    if weight is not None:
        model.weight = np.asarray(weight, dtype=np.float64)
    o = OD.default_opts(opts, method, weight is not None)
    D.InitialScaling(var, model, o["scaling"], None, dim=dim, weighted=weight is not None)
    if poke_c is not None:               # one entry of an interior layer of c (after the scaling, which may replace model.c)
        c = np.array(model.c, dtype=np.float64, copy=True).reshape(-1)
        c[poke_c(c.size)] = 1e-3 * np.max(np.abs(c))
        model.c = c
        if hasattr(model, "_c_ends"):
            model._c_ends = None
    ctx = D.InPALMContext(var, o, model, weighted=weight is not None, nslabs=nslabs, ngpu=ngpu, z_unread=True)
    try:
        for n in pieces:
            ctx.run(n)
        hist, sigma = ctx.finish()
    finally:
        ctx.close()
    return var, hist, sigma


def _identical(monkeypatch, switch, *args, **kw):
    monkeypatch.setenv(switch, "0")
    ref, h0, s0 = _run(*args, **kw)
    monkeypatch.setenv(switch, "1")
    got, h1, s1 = _run(*args, **kw)
    assert s1 == s0
    assert h1["len"] == h0["len"] and h0["len"] >= 1
    np.testing.assert_array_equal(h1["iter"], h0["iter"])
    np.testing.assert_array_equal(h1["kkt"], h0["kkt"])
    np.testing.assert_array_equal(h1["pdGap"], h0["pdGap"])
    assert got.cScale == ref.cScale and got.dScale == ref.dScale
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(got, f), getattr(ref, f), err_msg=f)
    return got, h1, s1


SHAPES = [(32, 32, 16, 40), (100, 70, 20, 30), (65, 129, 33, 25), (63, 5, 7, 20), (5, 3, 4, 12), (2, 2, 2, 6),
          (129, 3, 5, 15), (256, 256, 64, 30)]


def _densities(ny, nx):
    if ny * nx <= 6:
        rho0 = np.ones((ny, nx))
        rho1 = np.ones((ny, nx))
        rho1.flat[0] = 1.5
        rho1 /= rho1.mean()
        return rho0, rho1
    return get_example_2d("example1", ny, nx)


@pytest.mark.parametrize("switch", ["DOTSOCP_CONE_CARRY", "DOTSOCP_C_ENDS"])
@pytest.mark.parametrize("ny,nx,nt,K", SHAPES)
def test_switch_changes_no_bit(switch, ny, nx, nt, K, monkeypatch):
    rho0, rho1 = _densities(ny, nx)
    _identical(monkeypatch, switch, rho0, rho1, nt, dict(tol=0.0, maxit=K))


@pytest.mark.parametrize("switch", ["DOTSOCP_CONE_CARRY", "DOTSOCP_C_ENDS"])
def test_switch_changes_no_bit_1d_alg2_weighted_step_by_step(switch, monkeypatch):
    r0, r1 = get_example_1d("gaussian", 129)
    _identical(monkeypatch, switch, r0, r1, 33, dict(tol=0.0, maxit=60))
    rho0, rho1 = get_example_2d("example1", 24, 40)
    _identical(monkeypatch, switch, rho0, rho1, 12, dict(tol=0.0, maxit=40), method="ALG2")            # tau = 1
    _identical(monkeypatch, switch, rho0, rho1, 12, dict(tol=0.0, maxit=15, ifCheckStepByStep=True))
    _identical(monkeypatch, switch, rho0, rho1, 12, dict(tol=0.0, maxit=20, scaling=False, sigma=0.1))
    rho0, rho1 = get_example_2d("example1", 33, 47)
    barrier = gene_barrier_of_circle_pillar()
    weight = get_weight_by_barrier(47, 33, 13, barrier)
    rho0, rho1, _ = ensure_barrier_validity(rho0, rho1, barrier)
    _identical(monkeypatch, switch, rho0, rho1, 13, dict(tol=0.0, maxit=25), weight=weight)


@pytest.mark.parametrize("switch", ["DOTSOCP_CONE_CARRY", "DOTSOCP_C_ENDS"])
@pytest.mark.parametrize("ny,nx,nt,K,sigma0", [(32, 32, 16, 230, 1.0), (16, 16, 8, 320, 0.01)])
def test_switch_changes_no_bit_across_rescales_and_norm_checks(switch, ny, nx, nt, K, sigma0, monkeypatch):
    """Both rescales and the norm checks of iterations 100, 200, 300 (solver_socp_inPALM.m:139-149); with sigma0 = 0.01
    a check past iteration 100 does rescale.  The iteration in front of each of them has to leave beta behind."""
    rho0, rho1 = get_example_2d("example1", ny, nx)
    _identical(monkeypatch, switch, rho0, rho1, nt, dict(tol=0.0, maxit=K, sigma=sigma0))


@pytest.mark.parametrize("switch", ["DOTSOCP_CONE_CARRY", "DOTSOCP_C_ENDS"])
@pytest.mark.parametrize("nslabs,ngpu", [(2, None), (3, None), (1, 2)])
def test_switch_changes_no_bit_on_time_slabs(switch, nslabs, ngpu, monkeypatch):
    rho0, rho1 = get_example_2d("example1", 64, 48)
    _identical(monkeypatch, switch, rho0, rho1, 24, dict(tol=0.0, maxit=45), nslabs=nslabs, ngpu=ngpu)


def test_run_in_pieces_is_one_run(monkeypatch):
    """run(7); run(5); run(-1): the last iteration of each call leaves beta (the caller may download anything), and the
    trajectory is that of one run(-1) -- with the flavours and without."""
    rho0, rho1 = get_example_2d("example1", 40, 24)
    opts = dict(tol=0.0, maxit=40)
    whole = _identical(monkeypatch, "DOTSOCP_CONE_CARRY", rho0, rho1, 12, opts)
    parts = _identical(monkeypatch, "DOTSOCP_CONE_CARRY", rho0, rho1, 12, opts, pieces=(7, 5, -1))
    assert parts[2] == whole[2]
    np.testing.assert_array_equal(parts[1]["kkt"], whole[1]["kkt"])
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(parts[0], f), getattr(whole[0], f), err_msg=f)


def test_nonzero_interior_of_c_is_detected(monkeypatch):
    """One non-zero entry in an interior layer of c: the device test at upload says no, every layer is loaded, and
    DOTSOCP_C_ENDS changes nothing.  The entry does matter: the solve differs from the one with the plain c."""
    rho0, rho1 = get_example_2d("example1", 40, 24)
    opts = dict(tol=0.0, maxit=30)
    plane = 40 * 24
    poked = _identical(monkeypatch, "DOTSOCP_C_ENDS", rho0, rho1, 12, opts, poke_c=lambda n: 5 * plane + 7 * 40 + 3)
    plain, _, _ = _run(rho0, rho1, 12, opts)
    assert np.max(np.abs(poked[0].phi - plain.phi)) > 1e-6 * np.max(np.abs(plain.phi))
    # the plain c is what the detection is made for: all-zero bits between its end layers
    var, model = D.initialize(rho0, rho1, 12)
    D.InitialScaling(var, model, True, None, dim=2)
    inner = np.ascontiguousarray(np.asarray(model.c, dtype=np.float64).reshape(-1)[plane:-plane])
    assert not inner.view(np.uint64).any()


@pytest.mark.parametrize("ny,nx,nt,K", [(64, 64, 32, 120), (65, 129, 33, 25)])
def test_default_path_against_the_oracle(ny, nx, nt, K):
    rho0, rho1 = get_example_2d("example1", ny, nx)
    opts = dict(tol=0.0, maxit=K)
    ovar, omodel, oo = OD.make_level(rho0, rho1, nt, opts, "inPALM", None)
    st = InPALMState(ovar, oo, omodel)
    st.run()
    o_hist, o_sigma = st.finish()
    gvar, g_hist, g_sigma = _run(rho0, rho1, nt, opts)
    assert g_hist["len"] == o_hist["len"]
    np.testing.assert_array_equal(g_hist["iter"], o_hist["iter"])
    assert abs(g_sigma - o_sigma) <= 1e-12 * abs(o_sigma)
    np.testing.assert_allclose(g_hist["kkt"], o_hist["kkt"], rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(g_hist["pdGap"], o_hist["pdGap"], rtol=1e-6, atol=1e-14)
    errs = {f: np.max(np.abs(getattr(gvar, f) - getattr(ovar, f))) / np.max(np.abs(getattr(ovar, f))) for f in FIELDS}
    print("relative errors against the oracle:", errs)
    assert max(errs.values()) <= 1e-9, errs
    assert abs(gvar.cScale - ovar.cScale) <= 1e-12 * ovar.cScale and abs(gvar.dScale - ovar.dScale) <= 1e-12 * ovar.dScale


def test_time_limit_in_a_plain_iteration_stops_at_a_check():
    """The time limit is read after the iteration body.  If that iteration left gamma behind, the unscheduled KKT check
    cannot read it: the next iteration is a checking one and the loop stops there.  Either way the run ends with a check
    of its last iteration, on a state every reader accepts."""
    rho0, rho1 = get_example_2d("example1", 64, 64)
    var, model = D.initialize(rho0, rho1, 16)
    o = OD.default_opts(dict(tol=0.0, maxit=1000000, time_limit=0.5), "inPALM", False)
    D.InitialScaling(var, model, o["scaling"], None, dim=2)
    ctx = D.InPALMContext(var, o, model, z_unread=True)
    try:
        done = ctx.run(-1)
        hist, _ = ctx.finish()
        stopped, iters = ctx.result.stopped, ctx.result.iters
    finally:
        ctx.close()
    assert stopped == 1 and 1 < done == iters < 1000000
    assert hist["iter"][-1] == iters
    for f in FIELDS:
        assert np.all(np.isfinite(getattr(var, f))), f


@pytest.mark.parametrize("carry,stop_at", [("1", 7), ("0", 6)])
def test_time_limit_in_a_gamma_iteration_is_honoured_one_iteration_later(carry, stop_at, monkeypatch):
    """The same branch, taken at a chosen iteration (DOTSOCP_TEST_TIMEOUT_AT: the limit counts as passed from that
    iteration on).  Iterations 1 and 4 end in a check, 5 runs without a pending step, 6 is the entry pass and leaves
    gamma (7 is the next check, 6 has none): the time-out seen after iteration 6 is remembered, iteration 7 is a
    scheduled checking iteration and the loop stops there.  Without the gamma form the unscheduled check stops it at 6."""
    monkeypatch.setenv("DOTSOCP_CONE_CARRY", carry)
    monkeypatch.setenv("DOTSOCP_TEST_TIMEOUT_AT", "6")
    rho0, rho1 = get_example_2d("example1", 32, 32)
    var, hist, _ = _run(rho0, rho1, 16, dict(tol=0.0, maxit=50))
    assert list(hist["iter"]) == [1, 4, stop_at]
    for f in FIELDS:
        assert np.all(np.isfinite(getattr(var, f))), f


def _phase_counts(K):
    rho0, rho1 = get_example_2d("example1", 64, 64)
    var, model = D.initialize(rho0, rho1, 16)
    o = OD.default_opts(dict(tol=0.0, maxit=K), "inPALM", False)
    D.InitialScaling(var, model, o["scaling"], None, dim=2)
    ctx = D.InPALMContext(var, o, model, profiling=True, z_unread=True)
    try:
        ctx.run(-1)
        ctx.finish()
        return [ctx.kernel_time(k) for k in ("cone_fused_a", "cone_fused_b", "cone_carry")]
    finally:
        ctx.close()


def test_steady_passes_are_timed_as_their_own_phase(monkeypatch):
    """Profiling: the passes that read gamma and no q^{k-1} are the phase "cone_carry"; "cone_fused_b" keeps the passes
    that move 8 (20 Nz + 3 Nq) bytes (flavours (0,0) and (0,1)); "cone_fused_a" the passes without a pending multiplier
    step (the first one, and the one after every KKT check or materialising rescale, which execute that step
    themselves).  In one run(-1) of 40 iterations (no norm check before iteration 100) a beta-form state with a
    pending step arises only behind a mode-A pass, so at most one beta-reading deferred pass follows each of them and
    every other deferred pass reads gamma.  With DOTSOCP_CONE_CARRY=0 the same passes all read beta."""
    K = 40
    monkeypatch.setenv("DOTSOCP_CONE_CARRY", "1")
    (ms_a, n_a), (ms_b, n_b), (ms_c, n_c) = _phase_counts(K)
    print("carry on: cone_fused_a %d, cone_fused_b %d, cone_carry %d launches" % (n_a, n_b, n_c))
    assert n_a + n_b + n_c == K and n_a >= 1
    assert 1 <= n_b <= n_a and n_c >= 1
    assert ms_b > 0 and ms_c > 0
    monkeypatch.setenv("DOTSOCP_CONE_CARRY", "0")
    (_, m_a), (_, m_b), (_, m_c) = _phase_counts(K)
    assert m_c == 0 and m_a == n_a and m_b == n_b + n_c
