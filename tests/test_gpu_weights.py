"""The device-resident weight pyramid (include/dotsocp.h: dotsocp_weights_*, csrc/weights.hip) against the oracle's
restatement of downSample_q.m / downSample_barrier.m, and the weighted multilevel driver with weights="device"."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import dotsocp_amd as D
from dotsocp_amd import capi
from oracle import multilevel as OM
from oracle.driver import recover_RhoE
from oracle.examples import (ensure_barrier_validity, gene_barrier_of_circle_pillar, get_example_2d,
                             get_weight_by_barrier)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = -1, -4

# fine grids (ny, nx, nt): coarse axes of two points and edge axes of one; three different lengths; a row longer than a
# wave; the longest row
GRIDS = [(3, 3, 3), (5, 3, 3), (17, 9, 5), (9, 33, 17), (129, 5, 5), (1025, 3, 3)]
# the bars tests/test_multilevel.py::test_downsample_weights holds the two host implementations to
LOG_RTOL, LIN_ATOL = 1e-13, 1e-14


def nq(ny, nx, nt):
    return ny * nx * (nt - 1) + ny * (nx - 1) * nt + (ny - 1) * nx * nt


def make_weight(kind, ny, nx, nt, seed=0):
    rng = np.random.default_rng(1000 * seed + ny + 7 * nx + 31 * nt)
    if kind == "barrier":
        return get_weight_by_barrier(nx, ny, nt, gene_barrier_of_circle_pillar())
    if kind == "loguniform":
        return 10.0 ** rng.uniform(-3.0, 6.0, nq(ny, nx, nt))
    return rng.uniform(0.0, 1.0, nq(ny, nx, nt))


def check_restriction(dev, ref, log_mean, what):
    err = np.abs(dev - ref)
    print(f"{what}: max abs err {err.max():.3e}, max rel err {(err / np.abs(ref).clip(1e-300)).max():.3e}")
    if log_mean:
        np.testing.assert_allclose(dev, ref, rtol=LOG_RTOL, atol=0)
    else:
        np.testing.assert_allclose(dev, ref, rtol=0, atol=LIN_ATOL)


@pytest.mark.parametrize("kind", ["barrier", "loguniform", "uniform"])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_restriction_against_oracle(grid, kind):
    ny, nx, nt = grid
    log_mean = kind != "uniform"
    w = make_weight(kind, ny, nx, nt)
    pyr = D.WeightPyramid(ny, nx, nt, 2)
    try:
        pyr.set(w)
        pyr.restrict(log_mean)
        np.testing.assert_array_equal(pyr.download(1), w)
        dev = pyr.download(0)
    finally:
        pyr.close()
    ref = OM.downSample_barrier(nt, nx, ny, w) if log_mean else OM.downSample_q(nt, nx, ny, w)
    assert dev.shape == ref.shape
    check_restriction(dev, ref, log_mean, f"{grid} {kind}")


@pytest.mark.parametrize("log_mean", [True, False])
def test_three_level_pyramid(log_mean):
    """Level 1 and level 0 of a pyramid from (33, 17, 9): each against the oracle applied to the device's own previous
    level, so that errors do not compound inside the comparison -- and against the oracle applied once and twice to the
    input, which a level wired to the wrong source would miss.  Bar of the second step there: a restriction step is a
    convex combination (of the logarithms in log-mean mode), so it passes on at most the error of its input and adds its
    own -- twice the bar of one step."""
    ny, nx, nt = 33, 17, 9
    w = make_weight("barrier" if log_mean else "uniform", ny, nx, nt)
    pyr = D.WeightPyramid(ny, nx, nt, 3)
    try:
        pyr.set(w)
        pyr.restrict(log_mean)
        l2, l1, l0 = pyr.download(2), pyr.download(1), pyr.download(0)
    finally:
        pyr.close()
    np.testing.assert_array_equal(l2, w)
    down = OM.downSample_barrier if log_mean else OM.downSample_q
    assert l1.size == nq(17, 9, 5) and l0.size == nq(9, 5, 3)
    check_restriction(l1, down(nt, nx, ny, l2), log_mean, "level 1")
    check_restriction(l0, down(5, 9, 17, l1), log_mean, "level 0")
    once = down(nt, nx, ny, w)
    twice = down(5, 9, 17, once)
    check_restriction(l1, once, log_mean, "level 1 against the oracle applied once")
    err = np.abs(l0 - twice)
    print(f"level 0 against the oracle applied twice: max abs err {err.max():.3e}, max rel err {(err / np.abs(twice)).max():.3e}")
    if log_mean:
        np.testing.assert_allclose(l0, twice, rtol=2 * LOG_RTOL, atol=0)
    else:
        np.testing.assert_allclose(l0, twice, rtol=0, atol=2 * LIN_ATOL)


def test_set_space_equals_get_weight_by_barrier():
    ny, nx, nt = 9, 17, 5
    barrier = gene_barrier_of_circle_pillar()
    ref = get_weight_by_barrier(nx, ny, nt, barrier)
    sw = D.get_space_weight_by_barrier(nx, ny, barrier)
    np.testing.assert_array_equal(sw.expand(nt), ref)
    pyr = D.WeightPyramid(ny, nx, nt, 1)
    try:
        pyr.set(sw)
        np.testing.assert_array_equal(pyr.download(0), ref)
    finally:
        pyr.close()


@pytest.mark.parametrize("kind", ["barrier", "loguniform", "uniform"])
def test_log10_mean(kind):
    """mean(log10(w + 1e-10)): terms in [-10, 6], Nq <= 2e5 -- the fixed-order sum is the only difference to numpy"""
    ny, nx, nt = 65, 33, 29
    w = make_weight(kind, ny, nx, nt)
    assert w.size <= 200000
    pyr = D.WeightPyramid(ny, nx, nt, 2)
    try:
        pyr.set(w)
        pyr.restrict(kind != "uniform")
        for lv in (1, 0):
            a, b = pyr.log10_mean(lv), pyr.log10_mean(lv)
            ref = np.mean(np.log10(pyr.download(lv) + 1e-10))
            print(f"{kind} level {lv}: device {a!r} numpy {ref!r} diff {abs(a - ref):.3e}")
            assert a == b                                 # equal bits
            np.testing.assert_allclose(a, ref, rtol=0, atol=1e-13)
    finally:
        pyr.close()


def _create(ny, nx, nt, weighted=1, dim=2, nslabs=1, ngpu=None):
    L = capi.lib()
    p = capi.Problem()
    p.dim, p.weighted, p.ny, p.nx, p.nt = dim, weighted, ny, nx, nt
    p.D = p.E = p.cScale = p.dScale = p.normc = p.normd = 1.0
    ctx = (L.dotsocp_create_multi(ctypes.byref(p), 0, ngpu) if ngpu else L.dotsocp_create(ctypes.byref(p), 0, nslabs))
    assert ctx, L.dotsocp_last_error().decode()
    return ctx


def _upload_roundtrip(ny, nx, nt, **kw):
    """model.weight of a context filled from both levels of a pyramid, then downloaded: bit-equal to the pyramid's own
    download (rows py / pyb apart on the device, reference layout on both ends)"""
    L = capi.lib()
    w = make_weight("loguniform", ny, nx, nt)
    pyr = D.WeightPyramid(ny, nx, nt, 2)
    try:
        pyr.set(w)
        pyr.restrict(True)
        for lv, (a, b, c) in ((1, (ny, nx, nt)), (0, ((ny + 1) // 2, (nx + 1) // 2, (nt + 1) // 2))):
            if c < 2 * max(kw.get("nslabs", 1), kw.get("ngpu") or 1):
                continue                                  # too few time nodes for that many slabs
            ctx = _create(a, b, c, **kw)
            try:
                pyr.upload_to(ctx, lv)
                got = np.empty(nq(a, b, c))
                capi.check(L.dotsocp_download(ctx, capi.F_WEIGHT, capi.fptr(got)))
            finally:
                L.dotsocp_destroy(ctx)
            np.testing.assert_array_equal(got, pyr.download(lv))
    finally:
        pyr.close()


@pytest.mark.parametrize("ny", [9, 17, 129])
def test_upload_weight_from_one_slab(ny):
    """ny = 9: unpitched rows; 17 and 129: rows padded to 32 / 144 doubles"""
    _upload_roundtrip(ny, 5, 5)


def test_upload_weight_from_uneven_slabs():
    _upload_roundtrip(9, 5, 9, nslabs=3)


def test_upload_weight_from_create_multi():
    _upload_roundtrip(9, 5, 9, ngpu=2)


@pytest.mark.parametrize("kw", [dict(nslabs=3), dict(ngpu=2)], ids=["nslabs3", "ngpu2"])
@pytest.mark.parametrize("ny", [17, 33])
def test_upload_weight_from_pitched_slabs(ny, kw):
    """Time slabs are pitched like the single slab (rows of 17 / 33 doubles stored 32 / 48 apart): every slab spreads its
    layers with its own 2-D copies (level 0 of the ngpu = 2 case has ny = 9 or 17)"""
    _upload_roundtrip(ny, 5, 9, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(nslabs=3), dict(ngpu=2)], ids=["one_slab", "nslabs3", "ngpu2"])
def test_upload_weight_from_staged(kw, monkeypatch):
    """DOTSOCP_WEIGHT_STAGE=1: every slab first takes its three layer ranges of [q0; bx; by] as peer copies into a staging
    buffer and spreads the rows from there -- the form a pitched slab on ANOTHER device than the pyramid takes.  (Copies
    between different devices themselves cannot run on a one-GPU box.)"""
    monkeypatch.setenv("DOTSOCP_WEIGHT_STAGE", "1")
    _upload_roundtrip(17, 5, 9, **kw)
    _upload_roundtrip(9, 5, 9, **kw)


CANARY_CHILD = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, {root!r})
import dotsocp_amd as D
from dotsocp_amd import capi
L = capi.lib()
ny, nx, nt = 17, 9, 5
w = D.get_weight_by_barrier(nx, ny, nt, D.gene_barrier_of_circle_pillar())
pyr = D.WeightPyramid(ny, nx, nt, 2)
pyr.set(D.get_space_weight_by_barrier(nx, ny, D.gene_barrier_of_circle_pillar()))
pyr.restrict(True)
assert np.array_equal(pyr.download(1), w)
pyr.log10_mean(0)
p = capi.Problem()
p.dim, p.weighted, p.ny, p.nx, p.nt = 2, 1, ny, nx, nt
p.D = p.E = p.cScale = p.dScale = p.normc = p.normd = 1.0
ctx = L.dotsocp_create(ctypes.byref(p), 0, 1)
assert ctx
pyr.upload_to(ctx, 1)
got = np.empty(w.size)
capi.check(L.dotsocp_download(ctx, capi.F_WEIGHT, capi.fptr(got)))
assert np.array_equal(got, w)
bad = L.dotsocp_canary_check()
print("canary_check", bad, L.dotsocp_last_error().decode() if bad else "")
L.dotsocp_destroy(ctx)
pyr.close()
sys.exit(0 if bad == 0 else 3)
"""


def test_pyramid_under_guard_bands():
    """A child process with DOTSOCP_CANARY=1: the pyramid's buffers come from the guarded allocator, and no kernel or
    copy of the feature writes outside them"""
    env = dict(os.environ, DOTSOCP_CANARY="1")
    r = subprocess.run([sys.executable, "-c", CANARY_CHILD.format(root=ROOT)], env=env, capture_output=True, text=True,
                       timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "canary_check 0" in r.stdout


# ---------------------------------------------------------------------------------------------------------------------
# solver level: the configuration of tests/test_multilevel.py::test_multilevel_wdot2d_with_barrier_against_oracle
N, NT = 33, 17
OPTS = dict(tol=1e-3, maxit=400)


def _problem():
    barrier = gene_barrier_of_circle_pillar()
    rho0, rho1 = get_example_2d("example1", N, N)
    rho0, rho1, _ = ensure_barrier_validity(rho0, rho1, barrier)
    return rho0, rho1, barrier, get_weight_by_barrier(N, N, NT, barrier)


@functools.lru_cache(maxsize=None)
def _oracle(method):
    rho0, rho1, barrier, weight = _problem()
    ovar, omodel, ohists, _ = OM.solve_multilevel(rho0, rho1, NT, 2, OPTS, method, weight=weight, barrier=barrier,
                                                  ensure_barrier=ensure_barrier_validity)
    rho_o, _, _ = recover_RhoE(ovar, omodel, weighted=True)
    return [int(h["iter"][-1]) for h in ohists], rho_o


@pytest.mark.parametrize("form", ["ndarray", "SpaceWeight"])
def test_driver_with_device_weights_against_oracle(form):
    """Per-level iteration counts equal the oracle's and rho within 1e-5 of it: that test's own bars"""
    rho0, rho1, barrier, weight = _problem()
    iters_o, rho_o = _oracle("inPALM")
    w = weight if form == "ndarray" else D.get_space_weight_by_barrier(N, N, barrier)
    out, timeML, histML, hist = D.solver_wdotsocp2d(rho0, rho1, NT, 2, dict(OPTS, weight=w), "inPALM", barrier,
                                                    weights="device")
    print("iterations", [int(t["Iters"]) for t in timeML[:2]], iters_o, "max |rho - rho_o|", np.abs(out["rho"] - rho_o).max())
    assert [int(t["Iters"]) for t in timeML[:2]] == iters_o
    np.testing.assert_allclose(out["rho"], rho_o, atol=1e-5)


def test_driver_acc_admm_with_device_weights_against_oracle():
    """The acc-ADMM loop through the same driver path (same problem and options), held to what
    test_multilevel_loop_variants_against_oracle asks of the unweighted level loop: the oracle's iteration counts, rho
    within 1e-7, mass conservation, the method name."""
    rho0, rho1, barrier, weight = _problem()
    iters_o, rho_o = _oracle("acc-ADMM")
    sw = D.get_space_weight_by_barrier(N, N, barrier)
    out, timeML, histML, hist = D.solver_wdotsocp2d(rho0, rho1, NT, 2, dict(OPTS, weight=sw), "acc-ADMM", barrier)
    print("iterations", [int(t["Iters"]) for t in timeML[:2]], iters_o, "max |rho - rho_o|", np.abs(out["rho"] - rho_o).max())
    assert [int(t["Iters"]) for t in timeML[:2]] == iters_o
    np.testing.assert_allclose(out["rho"], rho_o, atol=1e-7)
    assert D.check_massConservation(out["rho"], 1e-2)
    assert hist["method"] == "Multilevel-acc-ADMM for Weighted-DOT-SOCP"


# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = capi.lib()
    with pytest.raises(capi.DotsocpError) as e:           # an even length with levels > 1
        D.WeightPyramid(9, 8, 5, 2)
    assert e.value.code == EINVAL
    assert L.dotsocp_weights_create(0, 9, 9, 6, 2) is None
    pyr = D.WeightPyramid(9, 9, 5, 2)
    ctxs = []
    try:
        with pytest.raises(capi.DotsocpError) as e:       # restrict before set
            pyr.restrict(True)
        assert e.value.code == ESTATE
        pyr.set(make_weight("loguniform", 9, 9, 5))
        pyr.restrict(True)
        m = capi.dbl()
        for lv in (-1, 2):                                # a level out of range
            assert L.dotsocp_weights_log10_mean(pyr._w, lv, ctypes.byref(m)) == EINVAL
            assert L.dotsocp_weights_download(pyr._w, lv, capi.fptr(np.empty(4))) == EINVAL
        fine = _create(9, 9, 5)
        ctxs.append(fine)
        assert L.dotsocp_upload_weight_from(fine, pyr._w, 2) == EINVAL
        assert L.dotsocp_upload_weight_from(fine, pyr._w, 0) == EINVAL            # a level of another grid
        unweighted = _create(9, 9, 5, weighted=0)
        ctxs.append(unweighted)
        assert L.dotsocp_upload_weight_from(unweighted, pyr._w, 1) == EINVAL
        one_d = _create(1, 9, 5, weighted=1, dim=1)
        ctxs.append(one_d)
        assert L.dotsocp_upload_weight_from(one_d, pyr._w, 1) == EINVAL
        assert L.dotsocp_upload_weight_from(fine, pyr._w, 1) == 0
        o = capi.Opts()
        o.tau, o.sigma, o.tol, o.maxit, o.checkPrimDualFeas, o.time_limit = 1.9, 1.0, 1e-3, 5, -1, 3600.0
        capi.check(L.dotsocp_begin(fine, ctypes.byref(o)))
        assert L.dotsocp_upload_weight_from(fine, pyr._w, 1) == ESTATE           # after begin()
    finally:
        for c in ctxs:
            L.dotsocp_destroy(c)
        pyr.close()
