"""The transport map of the rounded plan on the device (csrc/softlax.hip: the moment flavour of the soft passes, k_sl_map,
the frame kernels; csrc/solver_upper.hip; dotsocp_plan_map, dotsocp_upper_map, upper.plan_map(), InPALMContext.plan_map())
against its numpy twin (upper.barycentric_map, upper.plan_frames).

The rule is that of tests/test_gpu_upper.py, restated in _near_map: the yardstick is the twin in long double; every new array
and double of the device may lie as far from it as four times the float64 twin's own distance, at least 16 ulp of the array's
largest entry.  spread = 2 C - |D|^2 is a difference: its floor is taken on the largest entry of 2 C (the double `spread`: on
cost_rows, the same sum of 2 C), which is what the operands of the subtraction carry.  What the fixed order of the sums and
the integer deposit promise IS compared as bits: the bound against dotsocp_plan_bound, a second call, another chunk length,
the frames against plan_frames fed the device's own displacement, the context call against the stateless call."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import dotsocp_amd as D
from dotsocp_amd import capi
from dotsocp_amd import upper as U
import test_gpu_upper as TU
from test_gpu_upper import EINVAL, ESTATE, _bits, _env, _generic_context, _phi0, _problem, _solved_context
from test_plan_map_host import (check_against_dense, check_identity, check_monotone, check_translation, monotone_case,
                                translation_case)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_DOUBLES = ("rows", "map_cost", "spread", "cost_rows", "disp_mean", "disp_max")
TAUS = (0.0, 0.5, 1.0)


def _mbytes(d):
    """every number and array of a PlanMap, the bound's included, as bytes"""
    out = []
    for k in sorted(d):
        out.append(TU._bytes(d[k]) if k == "upper" else np.asarray(d[k]).tobytes(order="F"))
    return b"".join(out)


def _arrays(shape):
    return tuple(k for k in U.MAP_ARRAYS if len(shape) == 2 or k != "Dy")


@functools.lru_cache(maxsize=None)
def _map_case(shape, seed, sweeps, start=2):
    """the problem of test_gpu_upper._case (shared with that file's tests) and the two twins of its map, computed once"""
    rho0, rho1, f, u64, uld = TU._case(shape, seed, sweeps, start)
    return rho0, rho1, f, U.barycentric_map(u64, rho0, rho1), U.barycentric_map(uld, rho0, rho1, dtype=np.longdouble)


def _near_map(dev, m64, mld, what):
    worst = 0.0
    shape = np.shape(dev["C"])
    for k in _arrays(shape) + MAP_DOUBLES:
        ref = np.atleast_1d(np.asarray(mld[k], dtype=np.longdouble))
        got, own = np.atleast_1d(np.asarray(dev[k], dtype=np.float64)), np.atleast_1d(np.asarray(m64[k], dtype=np.float64))
        assert got.shape == ref.shape, k
        assert np.all(np.isfinite(ref)) and np.all(np.isfinite(got)) and np.all(np.isfinite(own)), k
        top = float(np.max(np.abs(ref)))
        if k == "spread_nodes":
            top = float(np.max(np.abs(2.0 * np.asarray(mld["C"], dtype=np.longdouble))))
        elif k == "spread":
            top = float(abs(mld["cost_rows"]))
        floor = 16.0 * float(np.spacing(np.float64(top)))
        d_own, d_dev = float(np.max(np.abs(own - ref))), float(np.max(np.abs(got - ref)))
        tol = max(4.0 * d_own, floor)
        print("  %-12s %-22s device %.3e  twin %.3e  allowed %.3e  (largest %.3e)  ratio %.3f" % (k, what, d_dev, d_own, tol, top, d_dev / tol))
        assert d_dev <= tol, (k, what, d_dev, tol)
        worst = max(worst, d_dev / tol)
    return worst


def _check_frames(dev, rho0, taus):
    """frames, unit and n_clamped of the device: the bits of plan_frames fed the device's own displacement"""
    tw = U.plan_frames(rho0, dev["Dx"], dev.get("Dy"), taus)
    assert dev["unit"] == tw["unit"] and dev["n_clamped"] == tw["n_clamped"]
    assert np.array_equal(_bits(dev["frames"]), _bits(tw["frames"]))
    counts = np.rint(dev["frames"] / dev["unit"]).astype(np.int64)
    assert all(int(counts[..., k].sum()) == tw["total_units"] for k in range(len(taus)))
    return tw


def _check(shape, seed, sweeps):
    rho0, rho1, f, m64, mld = _map_case(tuple(shape), seed, sweeps)
    dev = U.plan_map(rho0, rho1, f, 0.25, sweeps, arrays=True, taus=TAUS)
    again = U.plan_map(rho0, rho1, f, 0.25, sweeps, arrays=True, taus=TAUS)
    print(shape, "sweeps", sweeps, str(dev))
    worst = _near_map(dev, m64, mld, str(shape))
    print("  worst device / allowed: %.3f" % worst)
    assert _mbytes(dev) == _mbytes(again)                       # two calls: identical bytes
    bound = U.plan_bound(rho0, rho1, f, 0.25, sweeps, arrays=True)
    assert TU._bytes(dev["upper"]) == TU._bytes(bound)          # the bound is untouched, bit for bit
    assert set(U.plan_map(rho0, rho1, f, 0.25, sweeps)["upper"]) == set(U.FIELDS)
    _check_frames(dev, rho0, TAUS)
    return dev


@pytest.mark.parametrize("n,sweeps", [(2, 3), (33, 3), (1023, 2), (1024, 2), (1025, 2), (2049, 2)], ids=str)
def test_1d_against_the_long_double_twin(n, sweeps):
    _check((n,), seed=n, sweeps=sweeps)


@pytest.mark.parametrize("ny,nx", [(13, 17), (33, 31), (64, 32), (65, 33), (257, 40)], ids=str)
def test_2d_against_the_long_double_twin(ny, nx):
    _check((ny, nx), seed=ny + nx, sweeps=3)


def test_the_chunk_length_changes_no_bit():
    line = _problem((33,), 78)
    whole = U.plan_map(*line, 0.25, 3, arrays=True, taus=TAUS)
    for chunk in (1, 2, 7, 32):                                 # 33, 17, 5 and 2 chunks
        with _env(DOTSOCP_HL_CHUNK=chunk):
            assert _mbytes(U.plan_map(*line, 0.25, 3, arrays=True, taus=TAUS)) == _mbytes(whole), chunk
    rho0, rho1, f = _problem((40, 37), 77)
    whole = U.plan_map(rho0, rho1, f, 0.25, 4, arrays=True, taus=TAUS)
    with _env(DOTSOCP_HL_CHUNK=5):
        assert _mbytes(U.plan_map(rho0, rho1, f, 0.25, 4, arrays=True, taus=TAUS)) == _mbytes(whole)


def _near_twin(rho0, rho1, f, sweeps, what):
    dev = U.plan_map(rho0, rho1, f, 0.25, sweeps, arrays=True, taus=TAUS)
    m64 = U.barycentric_map(U.sinkhorn_round(rho0, rho1, f, 0.25, sweeps), rho0, rho1)
    mld = U.barycentric_map(U.sinkhorn_round(rho0, rho1, f, 0.25, sweeps, dtype=np.longdouble), rho0, rho1, dtype=np.longdouble)
    _near_map(dev, m64, mld, what)
    assert TU._bytes(dev["upper"]) == TU._bytes(U.plan_bound(rho0, rho1, f, 0.25, sweeps, arrays=True))
    _check_frames(dev, rho0, TAUS)
    return dev


def test_zero_mass_rows_columns_and_nodes():
    rho0, rho1, f = _problem((24, 19), 5, zeros=0)
    rho0[7, :] = 0.0
    rho0[:, 3] = 0.0
    rho0[12, 11] = 0.0
    rho1[0, 0] = rho1[23, 18] = rho1[11, 9] = 0.0
    rho1[:, 17] = 0.0
    dev = _near_twin(rho0, rho1, f, 3, "zero mass")
    for k in U.MAP_ARRAYS:
        assert np.all(dev[k][rho0 == 0] == 0.0), k
    assert np.all(dev["row"][rho0 > 0] > 0.0)
    assert np.array_equal(dev["frames"][..., 0] == 0.0, rho0 == 0)          # tau = 0: every node keeps its own units
    line = _problem((40,), 6, zeros=0)
    line[0][:9] = 0.0
    line[1][-11:] = 0.0
    dev = _near_twin(*line, 3, "zero mass 1-D")
    assert np.all(dev["Dx"][:9] == 0.0) and np.all(dev["row"][:9] == 0.0) and np.all(dev["row"][9:] > 0.0)


def test_non_finite_start_entries_at_a_chunk_boundary():
    n, at = 24, 8
    rho0, rho1, f = _problem((n,), 9, zeros=0)
    f[at - 1], f[at], f[at + 1] = np.nan, np.inf, -np.inf
    with _env(DOTSOCP_HL_CHUNK=8):
        dev = _near_twin(rho0, rho1, f, 2, "non-finite start 1-D")
        clean = f.copy()
        clean[at - 1:at + 2] = 0.0          # ... they count as 0.0
        same = U.plan_map(rho0, rho1, clean, 0.25, 2, arrays=True, taus=TAUS)
    assert dev["upper"]["nonfinite"] == 3 and same["upper"]["nonfinite"] == 0
    dev["upper"]["nonfinite"] = 0
    assert _mbytes(dev) == _mbytes(same)
    rho0, rho1, f = _problem((24, 24), 10, zeros=0)
    f[5, at - 1:at + 2] = np.nan
    f[at - 1:at + 2, 17] = np.inf
    with _env(DOTSOCP_HL_CHUNK=8):
        dev = _near_twin(rho0, rho1, f, 2, "non-finite start 2-D")
    assert dev["upper"]["nonfinite"] == 6


def test_frames_out_of_order_and_against_a_wall():
    rho0, rho1, f = _problem((21, 18), 31)
    taus = (1.0, 0.0, 0.5, 1.0, 0.25)
    dev = U.plan_map(rho0, rho1, f, 0.25, 3, taus=taus)
    _check_frames(dev, rho0, taus)
    fr = dev["frames"]
    assert np.array_equal(_bits(fr[..., 0]), _bits(fr[..., 3])) and not np.array_equal(fr[..., 0], fr[..., 2])
    M = np.rint(rho0 / dev["unit"]).astype(np.int64)
    assert np.array_equal(_bits(fr[..., 1]), _bits(M.astype(np.float64) * dev["unit"]))     # tau = 0: M unit, node by node
    assert "frames" not in U.plan_map(rho0, rho1, f, 0.25, 3) and U.plan_map(rho0, rho1, f, 0.25, 3)["n_clamped"] == 0
    # all of rho1 on the right wall and the bottom wall's corner: T(x) lies on the wall, where rounding may step over it; the
    # clamp then moves the node, and the count is that of the twin
    wall = np.zeros((21, 18))
    wall[:, -1] = 1.0
    dev = U.plan_map(rho0, rho1 * 0.0 + wall, None, 0.25, 5, taus=(1.0, 0.5, 1.0))
    tw = _check_frames(dev, rho0, (1.0, 0.5, 1.0))
    print("against the wall: %d nodes clamped, largest x + Dx - 1 = %.3e" % (dev["n_clamped"], float((np.arange(18) / 17.0 + dev["Dx"]).max() - 1.0)))
    # at tau = 1 the mass stands in the wall's column (a position one ulp short of the wall leaves the rounding of its few
    # units to the column before)
    assert int(tw["counts"][:, -1, 0].sum()) >= (1.0 - 1e-9) * tw["total_units"] and np.all(tw["counts"][:, :-2, 0] == 0)
    assert 0 <= dev["n_clamped"] <= int(np.count_nonzero(rho0 > 0))


@pytest.mark.parametrize("shape", [(9, 9), (13, 17)], ids=str)
def test_the_device_map_is_the_dense_plans(shape):
    """the n x n plan rebuilt on the host from the device's f, g, er, ec -- no twin involved -- has this map"""
    rho0, rho1, f = _problem(shape, 20 + sum(shape))
    dev = U.plan_map(rho0, rho1, f, 0.25, 20, arrays=True)
    check_against_dense(dev, dev["upper"], rho0, rho1)
    check_identity(dev)


def test_translation_on_the_device():
    rho0, rho1, shift = translation_case()
    dev = U.plan_map(rho0, rho1, None, 0.25, 200)
    check_translation(dev, rho0, shift)
    check_identity(dev)


def test_monotone_map_on_a_line_on_the_device():
    rho0, rho1, f, T_exact = monotone_case()
    check_monotone(U.plan_map(rho0, rho1, f, 0.25, 100), T_exact)


@pytest.mark.parametrize("dim,method,split", [(2, "inPALM", {}), (2, "PALM", {}), (2, "acc-ADMM", {}), (2, "inPALM", dict(nslabs=2)),
                                              (1, "inPALM", {})], ids=["inPALM", "PALM", "acc-ADMM", "nslabs2", "1d"])
def test_context_call_after_a_real_solve(dim, method, split):
    ctx = _solved_context(dim, method, **split)
    nt = int(ctx.model.nt)
    nodes = [nt - 1, 0, nt // 2, nt // 2 + 1]
    try:
        got = ctx.plan_map(max_sweeps=10, arrays=True, frames=nodes, compare=dict(stride=2, nsub=2))
        phi0 = _phi0(ctx)
        rho = ctx.outputs()["rho"]
        mask = np.asarray(ctx.model.rho0) > 0
        x, y = D.advect.seeds_on_nodes(int(ctx.model.nx), int(ctx.model.ny) if dim == 2 else None, stride=2, mask=mask)
        end = ctx.advect(x, y, nsub=2)
    finally:
        ctx.close()
    rho0 = np.asarray(ctx.model.rho0)
    free = U.plan_map(rho0, ctx.model.rho1, -phi0, 0.25, 10, arrays=True, taus=np.array(nodes) / float(nt - 1))
    print(method, split, str(got), "l1", got["l1"], "map_gap %.4e max %.4e" % (got["map_gap"], got["map_gap_max"]))
    own = ("l1", "nodes", "map_gap", "map_gap_max", "n")
    assert _mbytes({k: v for k, v in got.items() if k not in own}) == _mbytes(free)
    l1 = [np.mean(np.abs(got["frames"][..., k] - rho[..., node])) for k, node in enumerate(nodes)]
    np.testing.assert_allclose(got["l1"], l1, rtol=1e-12, atol=0.0)
    at = lambda t: D.advect.masses_on_nodes(t, stride=2, mask=mask)         # noqa: E731
    want = U.map_gap(x, y, end["x"], end["y"], at(got["Dx"]), at(got["Dy"]) if dim == 2 else None, at(rho0))
    assert np.isfinite(got["map_gap"]) and np.isfinite(got["map_gap_max"]) and got["map_gap"] <= got["map_gap_max"]
    assert (got["map_gap"], got["map_gap_max"], got["n"]) == (want["map_gap"], want["map_gap_max"], want["n"])
    assert got["l1"][1] <= 0.5 * got["unit"]                    # node 0: rho0 rounded to whole units, on its own nodes


def _child():
    """Runs in a fresh process with DOTSOCP_CANARY=1 (the calls' buffers lie between guard bands) and DOTSOCP_POISON=1 (what no
    kernel has written is a NaN)"""
    assert os.environ.get("DOTSOCP_CANARY") == "1" and os.environ.get("DOTSOCP_POISON") == "1"
    for shape, chunk in (((37, 29), None), ((300,), 7)):
        with _env(DOTSOCP_HL_CHUNK=chunk):
            _check(shape, seed=sum(shape), sweeps=2)            # fails with DOTSOCP_EHIP if a band was overwritten
        assert capi.lib().dotsocp_canary_check() == 0, capi.lib().dotsocp_last_error().decode()
    for shape in ((19, 13), (70,)):
        ctx = _generic_context(shape, 5, nslabs=2)
        try:
            got = ctx.plan_map(max_sweeps=2, arrays=True, frames=[4, 0, 2])
            free = U.plan_map(ctx.model.rho0, ctx.model.rho1, -_phi0(ctx), 0.25, 2, arrays=True, taus=[1.0, 0.0, 0.5])
        finally:
            ctx.close()
        assert _mbytes({k: v for k, v in got.items() if k not in ("l1", "nodes")}) == _mbytes(free)
        assert np.all(np.isfinite(got["l1"]))
        assert capi.lib().dotsocp_canary_check() == 0, capi.lib().dotsocp_last_error().decode()
    print("child ok")


def test_between_guard_bands_and_on_poisoned_memory():
    code = "import sys; sys.path.insert(0, sys.argv[1]); import test_gpu_plan_map as T; T._child()"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), DOTSOCP_CANARY="1", DOTSOCP_POISON="1")
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "tests")], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("child ok"), out.stdout[-1000:] + out.stderr[-3000:]


def _sentinels(shape, sweeps, nf):
    res, mres = capi.Upper(), capi.PlanMap()
    ctypes.memset(ctypes.byref(res), 0x5a, ctypes.sizeof(res))
    ctypes.memset(ctypes.byref(mres), 0x5a, ctypes.sizeof(mres))
    arrs = [np.full(shape, 7.5, order="F") for _ in range(5)] + [np.full(sweeps, 7.5)]
    marrs = [np.full(shape, 7.5, order="F") for _ in range(5)]
    return res, mres, arrs, marrs, np.full(tuple(shape) + (nf,), 7.5, order="F"), np.full(nf, 7.5)


def _refused(code, word, ctx, r0, r1, o, shape, times, nf, with_map=True, with_frames=True, ny=None, nx=None):
    """the call returns `code`, its message holds `word`, and no struct and no array was written"""
    p = lambda a: None if a is None else a.ctypes.data         # noqa: E731
    res, mres, arrs, marrs, frames, l1 = _sentinels(shape, 4, 3)
    marks = bytes(res), bytes(mres)
    head = (p(r0), p(r1))
    tail = (None, None if o is None else ctypes.byref(o), ctypes.byref(res)) + tuple(p(a) for a in arrs) + \
        (ctypes.byref(mres) if with_map else None,) + tuple(p(a) for a in marrs) + (p(times), nf, p(frames) if with_frames else None)
    if ctx is None:
        rc = capi.lib().dotsocp_plan_map(*head, ny, nx, *tail, 0)
    else:
        rc = capi.lib().dotsocp_upper_map(ctx._ctx, *head, *tail, p(l1))
    assert rc == code, (word, rc)
    msg = capi.lib().dotsocp_last_error()
    assert word.encode() in msg, msg
    assert (bytes(res), bytes(mres)) == marks and all(np.all(a == 7.5) for a in arrs + marrs + [frames, l1]), word


def test_argument_errors_leave_the_outputs_untouched():
    ny, nx, nt = 9, 7, 4
    good = lambda **kw: capi.UpperOpts(**dict(dict(eps_h2=0.25, max_sweeps=4, defect_tol=0.0, start=0), **kw))     # noqa: E731
    ctx = _generic_context((ny, nx), nt, finish=False)
    r0, r1 = np.asfortranarray(ctx.model.rho0), np.asfortranarray(ctx.model.rho1)
    taus, nodes = np.array([0.0, 0.5, 1.0]), np.array([0, 1, 3], dtype=np.int64)
    try:
        _refused(ESTATE, "upper_map() needs finish()", ctx, r0, r1, good(), (ny, nx), nodes, 3)
        with pytest.raises(capi.DotsocpError) as ei:
            ctx.plan_map()
        assert ei.value.code == ESTATE
        ctx.finish(download=False)
        for c, dims, times in ((ctx, {}, nodes), (None, dict(ny=ny, nx=nx), taus)):
            ref = lambda word, a=r0, b=r1, o=good(), t=times, nf=3, **kw: _refused(EINVAL, word, c, a, b, o, (ny, nx), t, nf, **dict(dims, **kw))   # noqa: E731
            # what the bound's calls refuse
            ref("NULL", a=None)
            ref("NULL", b=None)
            ref("opts is NULL", o=None)
            ref("positive finite", a=np.zeros((ny, nx), order="F"))
            bad = r1.copy(order="F")
            for v in (np.inf, np.nan, -0.5):
                bad[2, 3] = v
                ref("negative or not finite", b=bad)
            for v in (0.0, -0.25, np.inf, np.nan):
                ref("eps_h2", o=good(eps_h2=v))
            ref("max_sweeps", o=good(max_sweeps=-1))
            ref("start is", o=good(start=3))
            ref("needs f_start", o=good(start=2))
            # the map's own
            ref("map_res is NULL", with_map=False)
            ref("nf must not be negative", nf=-1)
            ref("needs its times", t=None)
            ref("needs its times", with_frames=False)
            huge = r0.copy(order="F")
            huge[1, 1] = 1e307                              # the sum is finite, nodes * max(rho0) is not
            ref("unit", a=huge)
        for v in (np.nan, np.inf, -0.25, 1.0 + 2.0 ** -52):
            _refused(EINVAL, "every tau", None, r0, r1, good(), (ny, nx), np.array([0.0, v, 1.0]), 3, ny=ny, nx=nx)
        for v in (-1, nt):
            _refused(EINVAL, "frame node", ctx, r0, r1, good(), (ny, nx), np.array([0, v, 1], dtype=np.int64), 3)
        _refused(EINVAL, "needs a context", None, r0, r1, good(start=1), (ny, nx), taus, 3, ny=ny, nx=nx)
        _refused(EINVAL, "two nodes", None, r0, r1, good(), (ny, nx), taus, 3, ny=ny * nx, nx=1)
        # nf = 0 with both NULL is allowed, and so is any subset of the optional arrays
        res, mres = capi.Upper(), capi.PlanMap()
        p = lambda a: a.ctypes.data                         # noqa: E731
        o = good(start=1)
        assert capi.lib().dotsocp_upper_map(ctx._ctx, p(r0), p(r1), None, ctypes.byref(o), ctypes.byref(res), *([None] * 6),
                                            ctypes.byref(mres), *([None] * 5), None, 0, None, None) == 0
        full = ctx.plan_map(max_sweeps=4)
        assert _bits(mres.map_cost)[0] == _bits(full["map_cost"])[0] and mres.n_clamped == 0 and mres.unit == full["unit"]
        C = np.full((ny, nx), 7.5, order="F")
        assert capi.lib().dotsocp_upper_map(ctx._ctx, p(r0), p(r1), None, ctypes.byref(o), ctypes.byref(res), *([None] * 6),
                                            ctypes.byref(mres), None, None, p(C), None, None, None, 0, None, None) == 0
        assert np.array_equal(_bits(C), _bits(full["C"]))
    finally:
        ctx.close()
    ctx = _generic_context((ny, nx), nt, weighted=True)     # a weighted context: its cost is not the Euclidean one
    try:
        _refused(EINVAL, "weighted", ctx, r0, r1, good(), (ny, nx), nodes, 3)
    finally:
        ctx.close()


def test_interleaved_with_the_other_calls():
    """plan_map() between upper_bound(), dual_bound(), report() and push_from_nodes() on one context (2 time slabs): each
    result equals the same call made first on a fresh context"""
    rep = lambda r: b"".join(np.asarray(r[k]).tobytes() for k in sorted(r))            # noqa: E731
    push = lambda r: b"".join(np.asarray(r[k]).tobytes(order="F") for k in ("frames", "l1", "x", "y", "n_clamped"))   # noqa: E731
    raw = {"report": rep, "dual_bound": TU._bytes, "upper_bound": TU._bytes, "plan_map": _mbytes, "push": push}
    call = {"report": lambda c: c.report(), "dual_bound": lambda c: c.dual_bound(arrays=True),
            "upper_bound": lambda c: c.upper_bound(max_sweeps=3, arrays=True),
            "plan_map": lambda c: c.plan_map(max_sweeps=3, arrays=True, frames=[6, 0, 3], compare=dict(stride=3)),
            "push": lambda c: c.push_from_nodes(stride=2, frames=[0, 3, 6])}
    order = ["plan_map", "report", "upper_bound", "plan_map", "push", "dual_bound", "plan_map", "report", "push", "upper_bound"]
    ctx = _generic_context((19, 13), 7, seed=7, nslabs=2)
    try:
        mixed = [raw[k](call[k](ctx)) for k in order]
    finally:
        ctx.close()
    first = {}
    for k in call:
        fresh = _generic_context((19, 13), 7, seed=7, nslabs=2)
        try:
            first[k] = raw[k](call[k](fresh))
        finally:
            fresh.close()
    for k, got in zip(order, mixed):
        assert got == first[k], "%s differs from the same call made first on a fresh context" % k


def test_drivers_take_the_keyword():
    rho0, rho1 = D.get_example_2d("example1", 17, 17)
    with pytest.raises(ValueError, match="plan_map= needs transfer='device'"):
        D.solver_dotsocp2d(rho0, rho1, 5, 1, dict(tol=1e-2, maxit=5), transfer="host", plan_map=dict(max_sweeps=2))
    out = D.solver_dotsocp2d(rho0, rho1, 9, 1, dict(tol=1e-3, maxit=200), upper=dict(max_sweeps=20),
                             plan_map=dict(max_sweeps=20, frames=[0, 4, 8], compare=dict(stride=2)))[0]
    m = out["plan_map"]
    assert isinstance(m, U.PlanMap) and TU._bytes(m["upper"]) == TU._bytes(out["upper"])
    assert m["frames"].shape == (17, 17, 3) and m["l1"].shape == (3,) and np.isfinite(m["map_gap"])
    check_identity(m)
    assert "plan_map" not in D.solver_dotsocp2d(rho0, rho1, 5, 1, dict(tol=1e-2, maxit=5))[0]
