"""The geodesic's profile on the device (csrc/geodesic.hip, dotsocp_geodesic_profile, InPALMContext.geodesic()) against its
numpy twin (geodesic.geodesic_profile) applied to ctx.outputs() of the SAME context.

States are made by the recipe of tests/test_gpu_report.py, restated here: alpha and q entries s * 10^u (s = +-1, u uniform
in [-10, 1], seeded), rho0 / rho1 in [0.5, 1.5] with three exact zeros each; uploaded, begin(), no iteration, finish().
Before a device result is read, the recovered density is checked to hold a node with rho < 0, one with 0 <= rho <= floor
and one above the floor.  (A grid of two time nodes has end layers only, which are rho0 and rho1 themselves: it cannot
hold a negative node, and is asked for the other two.)

Rules.  The layer sums are compared as the layer means the profile holds (sum / (ny nx)), by the rule of
tests/test_gpu_report.py for its layer means: |device - twin| <= 2 N 2^-53 mean|term| per layer, N = ny nx, the classical
bound for summing N terms in any order, taken once for each side.  The entropy alone gets 8 * 2^-53 mean|term| on top: its
logarithm is the one operation that is not bit for bit the twin's (device within 1 ulp, libm within 1 ulp, the product's
rounding on both sides: 3 ulp = 6 * 2^-53 per term, rounded up).  rho_max, n_support: exact.  The struct must equal
geodesic.summarize() of the device's own arrays bit for bit; the mass row must carry the bits of the report's layer_mass
and `cost` those of its cost; two calls, time slabs, slabs on their own streams and DOTSOCP_PITCH=0 give identical bytes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dotsocp_amd as D
from dotsocp_amd import capi
from dotsocp_amd import geodesic as G
from dotsocp_amd import report as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
EINVAL, ESTATE = -1, -4

# name: (ny, nx, nt, weighted); 1-D: ny = None
CASES = {
    "2d_19x13x6": (19, 13, 6, False),
    "2d_33x17x9": (33, 17, 9, False),
    "2d_3x3x2": (3, 3, 2, False),
    "2d_64x4x2": (64, 4, 2, False),          # exactly one tile, end layers only
    "2d_65x5x3": (65, 5, 3, False),          # one past the tile both ways, one inner layer
    "2d_129x9x4": (129, 9, 4, False),
    "1d_301x9": (None, 301, 9, False),
    "1d_64x2": (None, 64, 2, False),
    "w_17x21x5": (17, 21, 5, True),
}


def _signed_pow(rng, n):
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-10, 1, n)


def _density(rng, shape):
    r = rng.uniform(0.5, 1.5, shape)
    r.flat[rng.choice(r.size, 3, replace=False)] = 0.0
    return r


def _context(case, nan=False, **split):
    """A finished context on the generic state of `case` (no iteration)"""
    ny, nx, nt, weighted = CASES[case]
    rng = np.random.default_rng(sorted(CASES).index(case) + 31070)
    shape = (nx,) if ny is None else (ny, nx)
    var, model = D.initialize(_density(rng, shape), _density(rng, shape), nt)
    nq = var.q.size
    if weighted:
        model.weight = 0.5 + (1e6 - 0.5) * rng.uniform(0, 1, nq) ** 32          # in [0.5, 1e6], most entries of order one
    D.InitialScaling(var, model, not weighted, None, dim=1 if ny is None else 2, weighted=weighted)
    var.q, var.alpha = _signed_pow(rng, nq), _signed_pow(rng, nq)
    if nan:
        plane = nx * (ny or 1)
        var.alpha[plane * (nt // 2) + plane // 2] = np.nan                      # an alpha0 entry of an inner cell layer
    opts = dict(tau=1.9, sigma=1.0, tol=0.0, maxit=1, ifCheckStepByStep=False, scaling=True)
    ctx = D.InPALMContext(var, opts, model, weighted=weighted, **split)
    ctx.finish(download=False)
    return ctx


def _raw(ctx):
    """(GeodesicProfile, struct, bytes of the struct and of the three arrays) straight from the C call"""
    m = ctx.model
    nt = int(m.nt)
    r0, r1 = np.asfortranarray(m.rho0, dtype=np.float64), np.asfortranarray(m.rho1, dtype=np.float64)
    res, sums = capi.Geodesic(), np.empty((nt, capi.GEO_SUMS), order="F")
    rho_max, n_support = np.empty(nt), np.empty(nt, dtype=np.int64)
    capi.check(capi.lib().dotsocp_geodesic_profile(ctx._ctx, capi.fptr(r0), capi.fptr(r1), ctypes.byref(res), capi.fptr(sums),
                                                   capi.fptr(rho_max), n_support.ctypes.data))
    return (G.from_struct(res, sums, rho_max, n_support, r0.size), res,
            bytes(res) + sums.tobytes(order="F") + rho_max.tobytes() + n_support.tobytes())


def _conditions(out, nt):
    """The recovered density exercises every branch of the terms (module docstring); asserted before the device is read"""
    rho = out["rho"]
    if nt > 2:
        assert np.count_nonzero(rho < 0) >= 1
    assert np.count_nonzero((rho >= 0) & (rho <= R.RHO_FLOOR)) >= 1 and np.count_nonzero(rho > R.RHO_FLOOR) >= 1


def _bits(v):
    return np.float64(v).tobytes()


def _assert_matches(dev, res, out, summary=True):
    """the device's profile `dev` (and struct `res`) against the twin of `out`, by the rules of the module docstring"""
    twin = G.geodesic_profile(out)
    N = out["rho"].size // out["rho"].shape[-1]
    for name, term in zip(G.NAMES, G.layer_terms(out)):
        with np.errstate(invalid="ignore"):
            mean_abs = np.abs(term.reshape((N, -1), order="F")).mean(axis=0)
        bound = 2 * N * U * mean_abs + (8 * U * mean_abs if name == "ent" else 0.0)
        ok = np.isfinite(twin[name])
        assert np.array_equal(np.isnan(dev[name]), np.isnan(twin[name])), name
        d = np.abs(dev[name][ok] - twin[name][ok])
        print(name, "worst difference / bound", np.max(d / np.where(bound[ok] > 0, bound[ok], 1.0)) if d.size else None)
        assert np.all(d <= bound[ok]), name
    assert dev["rho_max"].tobytes() == twin["rho_max"].tobytes() and np.array_equal(dev["n_support"], twin["n_support"])
    if summary:
        own = G.summarize(dev["sums"], dev["rho_max"], dev["n_support"], N)
        assert (res.nt, res.n_nodes, res.nonfinite) == (own["nt"], own["n_nodes"], own["nonfinite"]) == (twin["nt"], twin["n_nodes"], twin["nonfinite"])
        for k in G.SCALARS:
            print(k, getattr(res, k), own[k], twin[k])
            assert _bits(getattr(res, k)) == _bits(own[k]), k
    return twin


_one_slab = {}


def _one_slab_run(case):
    """(profile, struct, its bytes, the bytes of a second call, outputs, the report, geodesic()) of the one-slab context of `case`"""
    if case not in _one_slab:
        ctx = _context(case)
        try:
            out = ctx.outputs()
            dev, res, raw = _raw(ctx)
            _one_slab[case] = (dev, res, raw, _raw(ctx)[2], out, ctx.report(), ctx.geodesic())
        finally:
            ctx.close()
    return _one_slab[case]


@pytest.mark.parametrize("case", sorted(CASES))
def test_profile_equals_the_twin(case):
    dev, res, raw, again, out, rep, via_method = _one_slab_run(case)
    _conditions(out, CASES[case][2])
    _assert_matches(dev, res, out)
    assert raw == again                                             # two consecutive calls: identical bytes
    N = out["rho"].size // out["rho"].shape[-1]
    # the report's order: its layer means and its cost, bit for bit
    assert (dev["sums"][:, 0] / N).tobytes() == dev["mass"].tobytes() == rep["layer_mass"].tobytes()
    assert _bits(res.cost) == _bits(rep["cost"]) == _bits(dev["cost"])
    assert via_method["sums"].tobytes(order="F") == dev["sums"].tobytes(order="F") and _bits(via_method["cost"]) == _bits(dev["cost"])
    assert isinstance(via_method, G.GeodesicProfile) and via_method.summary().startswith("geodesic: cost ")
    assert len(via_method.table().splitlines()) == CASES[case][2] + 1


@pytest.mark.parametrize("split", [dict(nslabs=2), dict(nslabs=3), dict(ngpu=3)], ids=["nslabs2", "nslabs3", "multi3"])
@pytest.mark.parametrize("case", ["2d_19x13x6", "1d_301x9"])
def test_time_slabs_give_the_same_bytes(case, split):
    raw = _one_slab_run(case)[2]
    ctx = _context(case, **split)
    try:
        assert _raw(ctx)[2] == raw
    finally:
        ctx.close()


def test_planted_nan():
    case = "2d_19x13x6"
    nt = CASES[case][2]
    ctx = _context(case, nan=True)
    try:
        out = ctx.outputs()
        dev, res, _ = _raw(ctx)
    finally:
        ctx.close()
    hit = np.isnan(out["rho"]).reshape((-1, nt), order="F").any(axis=0)
    assert list(np.flatnonzero(hit)) == [nt // 2, nt // 2 + 1]      # the two node layers around the cell layer
    twin = _assert_matches(dev, res, out)                           # NaN where the twin has one, the rest within the bounds
    assert np.array_equal(np.isnan(dev["mass"]), hit) and np.array_equal(np.isnan(dev["sq"]), hit)
    assert np.all(np.isfinite(dev["rho_max"])) and res.nonfinite == 2 == twin["nonfinite"]
    clean = _one_slab_run(case)[0]                                  # same seed without the NaN
    for name in G.NAMES:
        assert dev[name][~hit].tobytes() == clean[name][~hit].tobytes(), name


@pytest.mark.parametrize("method", ["PALM", "acc-ADMM"])
def test_other_loops(method):
    rng = np.random.default_rng(77)
    var, model = D.initialize(_density(rng, (19, 13)), _density(rng, (19, 13)), 6)
    D.InitialScaling(var, model, True, None, dim=2)
    ctx = D.InPALMContext(var, dict(tau=1.9, sigma=1.0, tol=0.0, maxit=3, scaling=True), model, method=method)
    try:
        ctx.run(-1)
        ctx.finish(download=False)
        out = ctx.outputs()
        dev, res, _ = _raw(ctx)
    finally:
        ctx.close()
    _assert_matches(dev, res, out)


def _gaussians(n):
    """a Gaussian translated along the diagonal, on a small floor; mean 1"""
    X, Y = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n))
    g = lambda cx, cy: np.exp(-((X - cx) ** 2 + (Y - cy) ** 2) / (2 * 0.1 ** 2)) + 0.05          # noqa: E731
    rho0, rho1 = g(.35, .4), g(.65, .6)
    return rho0 / rho0.mean(), rho1 / rho1.mean()


def _solved():
    rho0, rho1 = _gaussians(33)
    var, model = D.initialize(rho0, rho1, 17)
    D.InitialScaling(var, model, True, None, dim=2)
    ctx = D.InPALMContext(var, dict(tau=1.9, sigma=1.0, tol=0.0, maxit=60, scaling=True), model)
    ctx.run(-1)
    ctx.finish(download=False)
    return ctx


def _flat(v):
    """the bytes of a result of geodesic(), report(), dual_bound(), outputs() or render()"""
    return b"".join(k.encode() + (np.ascontiguousarray(v[k]).tobytes() if isinstance(v[k], np.ndarray) else repr(v[k]).encode())
                    for k in sorted(v))


def test_real_solve_and_interleaved_calls():
    calls = dict(geodesic=lambda c: c.geodesic(), report=lambda c: c.report(), dual=lambda c: c.dual_bound(),
                 outputs=lambda c: c.outputs(), render=lambda c: c.render(num_frame=3))
    first = {}
    for name, call in calls.items():                                # every call made first on a fresh context
        ctx = _solved()
        try:
            first[name] = _flat(call(ctx))
        finally:
            ctx.close()
    ctx = _solved()
    try:
        out = ctx.outputs()
        dev, res, raw = _raw(ctx)
        rep = ctx.report()
        for name in ("geodesic", "report", "geodesic", "dual", "geodesic", "outputs", "render", "geodesic", "report", "dual", "render"):
            assert _flat(calls[name](ctx)) == first[name], name
        assert _raw(ctx)[2] == raw
    finally:
        ctx.close()
    twin = _assert_matches(dev, res, out)
    print(dev.summary())
    print(dev.table())
    assert _bits(res.cost) == _bits(rep["cost"]) and dev["mass"].tobytes() == rep["layer_mass"].tobytes()
    assert res.nonfinite == 0 and twin["nonfinite"] == 0


def _sentinels(nt):
    res = capi.Geodesic()
    ctypes.memset(ctypes.byref(res), 0x5a, ctypes.sizeof(res))
    return res, np.full((nt, capi.GEO_SUMS), 7.5, order="F"), np.full(nt, 7.5), np.full(nt, -3, dtype=np.int64)


def _refused(code, word, ctx, r0, r1, nt, with_res=True):
    """the call returns `code`, its message holds `word`, and neither the struct nor the three arrays were written"""
    res, sums, rho_max, n_support = _sentinels(nt)
    mark = bytes(res)
    p = lambda a: None if a is None else a.ctypes.data         # noqa: E731
    assert capi.lib().dotsocp_geodesic_profile(ctx._ctx, p(r0), p(r1), ctypes.byref(res) if with_res else None, p(sums), p(rho_max),
                                               p(n_support)) == code
    msg = capi.lib().dotsocp_last_error()
    assert word.encode() in msg, msg
    assert bytes(res) == mark and np.all(sums == 7.5) and np.all(rho_max == 7.5) and np.all(n_support == -3)


def test_refusals_leave_the_outputs_untouched():
    ny, nx, nt = 9, 7, 4
    rng = np.random.default_rng(5)
    var, model = D.initialize(_density(rng, (ny, nx)), _density(rng, (ny, nx)), nt)
    D.InitialScaling(var, model, True, None, dim=2)
    ctx = D.InPALMContext(var, dict(tau=1.9, sigma=1.0, tol=0.0, maxit=1, scaling=True), model)
    r0, r1 = np.asfortranarray(model.rho0), np.asfortranarray(model.rho1)
    try:
        _refused(ESTATE, "geodesic_profile() needs finish()", ctx, r0, r1, nt)
        with pytest.raises(capi.DotsocpError) as ei:
            ctx.geodesic()
        assert ei.value.code == ESTATE and "geodesic_profile" in str(ei.value)
        ctx.finish(download=False)
        _refused(EINVAL, "geodesic_profile", ctx, None, r1, nt)
        _refused(EINVAL, "geodesic_profile", ctx, r0, None, nt)
        _refused(EINVAL, "geodesic_profile", ctx, r0, r1, nt, with_res=False)
        # null optional arrays are accepted, any subset of them
        full, _, _ = _raw(ctx)
        res, sums, rho_max, n_support = _sentinels(nt)
        assert capi.lib().dotsocp_geodesic_profile(ctx._ctx, capi.fptr(r0), capi.fptr(r1), ctypes.byref(res), None, None, None) == 0
        assert res.n_nodes == ny * nx * nt and res.nt == nt and _bits(res.cost) == _bits(full["cost"])
        assert capi.lib().dotsocp_geodesic_profile(ctx._ctx, capi.fptr(r0), capi.fptr(r1), ctypes.byref(res), None, capi.fptr(rho_max),
                                                   None) == 0
        assert rho_max.tobytes() == full["rho_max"].tobytes() and np.all(sums == 7.5) and np.all(n_support == -3)
    finally:
        ctx.close()


def test_rccl_contexts_are_refused():
    from oracle.examples import get_example_2d
    rho0, rho1 = get_example_2d("example1", 16, 16)
    var, model = D.initialize_slab(rho0, rho1, 8, 0, 8)
    D.InitialScaling(var, model, True, None, dim=2)
    ctx = D.InPALMContext(var, dict(tau=1.9, sigma=1.0, tol=0.0, maxit=2, scaling=True), model, rccl=(D.capi.rccl_unique_id(), 0, 1))
    try:
        ctx.run(-1)
        ctx.finish(download=False)
        with pytest.raises(capi.DotsocpError) as ei:
            ctx.geodesic()
        assert ei.value.code == EINVAL and "RCCL" in str(ei.value)
        _refused(EINVAL, "RCCL", ctx, np.asfortranarray(rho0), np.asfortranarray(rho1), 8)
    finally:
        ctx.close()


def _child(what):
    """Runs in a fresh process with DOTSOCP_CANARY=1 (the call's buffers lie between guard bands), DOTSOCP_POISON=1 (what no
    kernel has written is a NaN) or DOTSOCP_PITCH=0 (rows as long as the grid's; read once per process): prints the bytes
    of the raw results of three contexts"""
    env = dict(canary="DOTSOCP_CANARY", poison="DOTSOCP_POISON", pitch0="DOTSOCP_PITCH")[what]
    assert os.environ.get(env) == ("0" if what == "pitch0" else "1")
    for case, split in (("2d_19x13x6", {}), ("2d_19x13x6", dict(nslabs=3)), ("w_17x21x5", {}), ("1d_301x9", {})):
        ctx = _context(case, **split)
        try:
            raw = _raw(ctx)[2]                   # fails with DOTSOCP_EHIP if a band was overwritten
            assert capi.lib().dotsocp_canary_check() == 0, capi.lib().dotsocp_last_error().decode()   # the buffers are live here
        finally:
            ctx.close()
        print("raw", case, raw.hex())
    assert capi.lib().dotsocp_canary_check() == 0
    print("child ok")


@pytest.mark.parametrize("what,env", [("canary", dict(DOTSOCP_CANARY="1")), ("poison", dict(DOTSOCP_POISON="1")),
                                      ("pitch0", dict(DOTSOCP_PITCH="0"))], ids=["canary", "poison", "pitch0"])
def test_guard_bands_poison_and_no_pitch_give_the_same_bytes(what, env):
    code = "import sys; sys.path.insert(0, sys.argv[1]); import test_gpu_geodesic as T; T._child(sys.argv[2])"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "tests"), what], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("child ok"), out.stdout[-1000:] + out.stderr[-3000:]
    got = [ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith("raw ")]
    want = [_one_slab_run(c)[2].hex() for c in ("2d_19x13x6", "2d_19x13x6", "w_17x21x5", "1d_301x9")]
    assert [g[1] for g in got] == want


def _after_solve(output):
    dev = output["geodesic"]
    assert isinstance(dev, G.GeodesicProfile)
    out = {k: v for k, v in output.items() if k != "geodesic"}
    N = out["rho"].size // out["rho"].shape[-1]
    twin = _assert_matches(dev, None, out, summary=False)
    own = G.summarize(dev["sums"], dev["rho_max"], dev["n_support"], N)
    for k in G.SCALARS:
        assert _bits(dev[k]) == _bits(own[k]), k
    assert dev["nonfinite"] == 0 and twin["nonfinite"] == 0
    print(dev.summary())


def test_driver_2d_profiles_after_a_real_solve():
    rho0, rho1 = D.get_example_2d("example1", 17, 17)
    output = D.solver_dotsocp2d(rho0, rho1, 9, 2, dict(tol=1e-4, maxit=60), geodesic=True)[0]
    _after_solve(output)
    plain = D.solver_dotsocp2d(rho0, rho1, 9, 2, dict(tol=1e-4, maxit=60))[0]          # the default path has no profile and the same outputs
    assert "geodesic" not in plain and all(np.array_equal(plain[k], output[k]) for k in plain)
    with pytest.raises(ValueError, match="geodesic=True needs transfer='device'"):
        D.solver_dotsocp2d(rho0, rho1, 9, 2, dict(tol=1e-2, maxit=5), transfer="host", geodesic=True)


def test_driver_1d_profiles_after_a_real_solve():
    rho0, rho1 = D.get_example_1d("gaussian", 65)
    _after_solve(D.solver_dotsocp1d(rho0, rho1, 9, 2, dict(tol=1e-4, maxit=60), geodesic=True)[0])


def test_driver_weighted_profiles_after_a_real_solve():
    rho0, rho1 = D.get_example_2d("example1", 17, 17)
    weight = D.gene_space_weight_circleInv(17, 17)
    _after_solve(D.solver_wdotsocp2d(rho0, rho1, 9, 2, dict(tol=1e-4, maxit=60, weight=weight), weights="device", geodesic=True)[0])
