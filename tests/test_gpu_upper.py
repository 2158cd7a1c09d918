"""The upper bound on the device (csrc/softlax.hip, csrc/solver_upper.hip; dotsocp_plan_bound, dotsocp_upper_bound,
upper.plan_bound(), InPALMContext.upper_bound()) against its numpy twin (upper.sinkhorn_round).

The device's exp and log are not numpy's, so nothing is compared as bits against the twin.  The yardstick is the twin run in
long double: an array of the device may lie as far from it as four times the float64 twin's own distance (the maximum over
the array), at least 16 ulp of the array's largest finite entry.  What the fixed order of the sums promises IS compared as
bits: another chunk length, a second call, the context call against the stateless call fed the downloaded phi(t = 0).

Sizes: a line of 2 nodes; lines below, at and above HL_YOUT = 1024 outputs of a workgroup of the y pass (= its chunk) and
one of two workgroups and chunks; layers that are ragged, exact, and one below / above the 64 lines, 32 outputs and 32
inputs of a workgroup of the x pass; 257 x 40 with two slices of the y pass."""
import contextlib
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = -1, -4
OPTS = dict(tau=1.9, sigma=1.0, tol=0.0, maxit=1, ifCheckStepByStep=False, scaling=True)
DOUBLES = tuple(k for k in U.FIELDS if k not in U._INT_FIELDS)


@contextlib.contextmanager
def _env(**kw):
    """environment variables around the calls of the block (DOTSOCP_HL_CHUNK and DOTSOCP_POISON are read at every call)"""
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items() if v is not None})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel(order="F")).view(np.uint64)


def _bytes(d):
    return b"".join(np.asarray(d[k]).tobytes(order="F") for k in sorted(d))


def _problem(shape, seed, zeros=3):
    """(rho0, rho1, f_start): densities in [0.5, 1.5] with a few exact zeros, a start of a few eps"""
    rng = np.random.default_rng(4100 + seed)
    rho = []
    for _ in range(2):
        r = rng.uniform(0.5, 1.5, shape)
        if zeros and r.size > zeros + 1:
            r.flat[rng.choice(r.size, zeros, replace=False)] = 0.0
        rho.append(r)
    eps = float(U._eps(shape, 0.25, np.float64))
    return rho[0], rho[1], eps * rng.uniform(-2.0, 2.0, shape)


@functools.lru_cache(maxsize=None)
def _case(shape, seed, sweeps, start, eps_h2=0.25):
    """the problem and its two twins (float64, long double), computed once and left alone"""
    rho0, rho1, f = _problem(shape, seed)
    f = f if start == 2 else None
    return rho0, rho1, f, U.sinkhorn_round(rho0, rho1, f, eps_h2, sweeps), \
        U.sinkhorn_round(rho0, rho1, f, eps_h2, sweeps, dtype=np.longdouble)


def _near(dev, u64, uld, what):
    """every array and every double of the device within 4 x the float64 twin's distance from the long double twin, floor 16
    ulp of the largest finite entry; non-finite entries in the same places; the integers equal"""
    worst = 0.0
    for k in U.ARRAYS + DOUBLES:
        ref = np.atleast_1d(np.asarray(uld[k], dtype=np.longdouble))
        got, own = np.atleast_1d(np.asarray(dev[k], dtype=np.float64)), np.atleast_1d(np.asarray(u64[k], dtype=np.float64))
        assert got.shape == ref.shape, k
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(got)) and np.array_equal(fin, np.isfinite(own)), k
        assert np.array_equal(got[~fin], own[~fin], equal_nan=True), k
        if not fin.any():
            continue
        top = float(np.max(np.abs(ref[fin])))
        floor = 16.0 * float(np.spacing(np.float64(top)))
        d_own = float(np.max(np.abs(own[fin] - ref[fin])))
        d_dev = float(np.max(np.abs(got[fin] - ref[fin])))
        tol = max(4.0 * d_own, floor)
        print("  %-12s %-22s device %.3e  twin %.3e  allowed %.3e  (largest %.3e)" % (k, what, d_dev, d_own, tol, top))
        assert d_dev <= tol, (k, what, d_dev, tol)
        worst = max(worst, d_dev / tol)
    for k in U._INT_FIELDS:
        assert dev[k] == u64[k] == uld[k], (k, dev[k], u64[k])
    return worst


def _check(shape, seed=0, sweeps=3, start=2, eps_h2=0.25):
    rho0, rho1, f, u64, uld = _case(tuple(shape), seed, sweeps, start, eps_h2)
    dev = U.plan_bound(rho0, rho1, f, eps_h2, sweeps, arrays=True)
    again = U.plan_bound(rho0, rho1, f, eps_h2, sweeps, arrays=True)
    print(shape, "sweeps", sweeps, "start", start, str(dev))
    _near(dev, u64, uld, str(shape))
    assert _bytes(dev) == _bytes(again)                         # two calls: identical bytes
    assert dev["n_nodes"] == int(np.prod(shape)) and dev["sweeps"] == sweeps and dev["nonfinite"] == 0
    assert set(U.plan_bound(rho0, rho1, f, eps_h2, sweeps)) == set(U.FIELDS)        # arrays=False: the numbers alone
    return dev


@pytest.mark.parametrize("n,sweeps", [(2, 3), (33, 3), (1023, 2), (1024, 2), (1025, 2), (2049, 2)], ids=str)
def test_1d_against_the_long_double_twin(n, sweeps):
    _check((n,), seed=n, sweeps=sweeps)


@pytest.mark.parametrize("ny,nx", [(13, 17), (33, 31), (64, 32), (65, 33), (257, 40)], ids=str)
def test_2d_against_the_long_double_twin(ny, nx):
    _check((ny, nx), seed=ny + nx, sweeps=3)


def test_the_chunk_length_changes_no_bit():
    rho0, rho1, f = _problem((40, 37), 77)
    whole = U.plan_bound(rho0, rho1, f, 0.25, 4, arrays=True)
    with _env(DOTSOCP_HL_CHUNK=5):
        chunks = U.plan_bound(rho0, rho1, f, 0.25, 4, arrays=True)
    assert _bytes(chunks) == _bytes(whole)
    line = _problem((300,), 78)
    whole = U.plan_bound(*line, 0.25, 3, arrays=True)
    with _env(DOTSOCP_HL_CHUNK=7):
        chunks = U.plan_bound(*line, 0.25, 3, arrays=True)
    assert _bytes(chunks) == _bytes(whole)


def _near_twin(rho0, rho1, f, sweeps, what, **kw):
    dev = U.plan_bound(rho0, rho1, f, 0.25, sweeps, arrays=True, **kw)
    u64 = U.sinkhorn_round(rho0, rho1, f, 0.25, sweeps)
    uld = U.sinkhorn_round(rho0, rho1, f, 0.25, sweeps, dtype=np.longdouble)
    _near(dev, u64, uld, what)
    return dev


def test_zero_mass_rows_columns_and_nodes():
    rho0, rho1, f = _problem((24, 19), 5, zeros=0)
    rho0[7, :] = 0.0                    # a row and a column of rho0 without mass, single nodes of rho1
    rho0[:, 3] = 0.0
    rho1[0, 0] = rho1[23, 18] = rho1[11, 9] = 0.0
    rho1[:, 17] = 0.0
    dev = _near_twin(rho0, rho1, f, 3, "zero mass")
    assert dev["zero0"] == 24 + 19 - 1 and dev["zero1"] == 3 + 24
    assert np.all(dev["er"][rho0 == 0] == 0.0) and np.all(dev["ec"][rho1 == 0] == 0.0)
    assert np.all(np.isfinite(dev["f"])) and np.all(np.isfinite(dev["g"])) and np.isfinite(dev["upper"])
    line = _problem((40,), 6, zeros=0)
    line[0][:9] = 0.0
    line[1][-11:] = 0.0
    dev = _near_twin(*line, 3, "zero mass 1-D")
    assert dev["zero0"] == 9 and dev["zero1"] == 11


def test_non_finite_start_entries_at_a_chunk_boundary():
    n, at = 24, 8
    rho0, rho1, f = _problem((n,), 9, zeros=0)
    f[at - 1], f[at], f[at + 1] = np.nan, np.inf, -np.inf
    with _env(DOTSOCP_HL_CHUNK=8):
        dev = _near_twin(rho0, rho1, f, 2, "non-finite start 1-D")
    assert dev["nonfinite"] == 3 and np.isfinite(dev["upper"])
    clean = f.copy()
    clean[at - 1:at + 2] = 0.0          # ... they count as 0.0
    with _env(DOTSOCP_HL_CHUNK=8):
        assert _bytes({k: v for k, v in U.plan_bound(rho0, rho1, clean, 0.25, 2, arrays=True).items() if k != "nonfinite"}) == \
            _bytes({k: v for k, v in dev.items() if k != "nonfinite"})
    rho0, rho1, f = _problem((24, 24), 10, zeros=0)
    f[5, at - 1:at + 2] = np.nan
    f[at - 1:at + 2, 17] = np.inf
    with _env(DOTSOCP_HL_CHUNK=8):
        dev = _near_twin(rho0, rho1, f, 2, "non-finite start 2-D")
    assert dev["nonfinite"] == 6


def test_stop_rule_and_starts():
    rho0, rho1, f = _problem((33, 31), 12)
    full = U.plan_bound(rho0, rho1, f, 0.25, 6, arrays=True)
    d = full["defects"]
    assert full["sweeps"] == 6 and d[2] < d[1] < d[0] and full["defect_first"] == d[0] and full["defect_last"] == d[5]
    early = U.plan_bound(rho0, rho1, f, 0.25, 6, defect_tol=0.5 * (d[1] + d[2]), arrays=True)
    assert early["sweeps"] == 3 and np.array_equal(_bits(early["defects"][:3]), _bits(d[:3])) and np.all(np.isnan(early["defects"][3:]))
    assert early["defect_last"] == d[2]
    three = U.plan_bound(rho0, rho1, f, 0.25, 3, arrays=True)
    assert _bytes({k: v for k, v in three.items() if k != "defects"}) == _bytes({k: v for k, v in early.items() if k != "defects"})
    # no sweep at all: the rounding of the start alone
    none = _near_twin(rho0, rho1, f, 0, "max_sweeps = 0")
    assert none["sweeps"] == 0 and np.isnan(none["defect_first"]) and np.isnan(none["defect_last"]) and none["defects"].size == 0
    assert none["upper"] > full["upper"]
    # start = 0: zeros
    cold = _near_twin(rho0, rho1, None, 3, "start = 0")
    assert _bytes(cold) == _bytes(U.plan_bound(rho0, rho1, np.zeros((33, 31)), 0.25, 3, arrays=True))


@pytest.mark.parametrize("shape", [(9, 9), (13, 17)], ids=str)
def test_the_device_certifies_itself(shape):
    """the n x n plan rebuilt on the host from the device's arrays -- no twin involved -- has the marginals and the cost"""
    rho0, rho1, f = _problem(shape, 20 + sum(shape))
    dev = U.plan_bound(rho0, rho1, f, 0.25, 20, arrays=True)
    P = U.plan_dense(dev["f"], dev["g"], dev["er"], dev["ec"], rho0, rho1, dev["eps"])
    a, b = rho0.ravel(order="F") / rho0.sum(), rho1.ravel(order="F") / rho1.sum()
    rows, cols = np.max(np.abs(P.sum(axis=1) - a)), np.max(np.abs(P.sum(axis=0) - b))
    cost = 2.0 * float((P * U.pair_cost(shape)).sum())
    print(shape, "rows %.2e columns %.2e plan cost %.12g upper %.12g" % (rows, cols, cost, dev["upper"]))
    assert rows <= 1e-12 and cols <= 1e-12
    assert abs(cost - dev["upper"]) <= 1e-11 * abs(cost)


def _solved_context(dim, method="inPALM", **split):
    """a real solve of example1 at 17 x 17 x 9 (1-D: the Gaussian pair at 65 x 9)"""
    if dim == 2:
        rho0, rho1 = D.get_example_2d("example1", 17, 17)
    else:
        rho0, rho1 = D.get_example_1d("gaussian", 65)
    var, model = D.initialize(rho0, rho1, 9)
    D.InitialScaling(var, model, True, None, dim=dim)
    ctx = D.InPALMContext(var, dict(OPTS, tol=1e-4, maxit=400), model, method=method, **split)
    ctx.run(-1)
    ctx.finish(download=False)
    return ctx


def _phi0(ctx):
    """phi(t = 0) in original units out of the download (recoverOrgVar: dScale * phi)"""
    m = ctx.model
    shape = (int(m.nx),) if not hasattr(m, "ny") else (int(m.ny), int(m.nx))
    phi = ctx.download(capi.F_PHI, np.empty(int(np.prod(shape)) * int(m.nt)))
    return (ctx.var.dScale * phi).reshape(shape + (int(m.nt),), order="F")[..., 0]


@pytest.mark.parametrize("dim,method,split", [(2, "inPALM", {}), (2, "PALM", {}), (2, "acc-ADMM", {}), (2, "inPALM", dict(nslabs=2)),
                                              (1, "inPALM", {})], ids=["inPALM", "PALM", "acc-ADMM", "nslabs2", "1d"])
def test_context_call_after_a_real_solve(dim, method, split):
    ctx = _solved_context(dim, method, **split)
    try:
        up = ctx.upper_bound(max_sweeps=10, arrays=True)
        lo = ctx.dual_bound()
        phi0 = _phi0(ctx)
        given = ctx.upper_bound(max_sweeps=10, start=2, f_start=-phi0, arrays=True)
    finally:
        ctx.close()
    free = U.plan_bound(ctx.model.rho0, ctx.model.rho1, -phi0, 0.25, 10, arrays=True)
    print(method, split, "bound %.9g <= upper %.9g" % (lo["bound"], up["upper"]), str(up))
    assert _bytes(up) == _bytes(free) and _bytes(given) == _bytes(free)
    assert lo["bound"] <= up["upper"]
    assert up["nonfinite"] == 0 and up["sweeps"] == 10 and up["defect_last"] < up["defect_first"]


def _child():
    """Runs in a fresh process with DOTSOCP_CANARY=1 (read once per process: the calls' buffers lie between guard bands) and
    DOTSOCP_POISON=1 (what no kernel has written is a NaN)"""
    assert os.environ.get("DOTSOCP_CANARY") == "1" and os.environ.get("DOTSOCP_POISON") == "1"
    for shape, chunk in (((37, 29), None), ((300,), 7)):
        with _env(DOTSOCP_HL_CHUNK=chunk):
            _check(shape, seed=sum(shape), sweeps=2)            # fails with DOTSOCP_EHIP if a band was overwritten
        assert capi.lib().dotsocp_canary_check() == 0, capi.lib().dotsocp_last_error().decode()
    for shape in ((19, 13), (70,)):
        ctx = _generic_context(shape, 5, nslabs=2)
        try:
            up = ctx.upper_bound(max_sweeps=2, arrays=True)
            free = U.plan_bound(ctx.model.rho0, ctx.model.rho1, -_phi0(ctx), 0.25, 2, arrays=True)
        finally:
            ctx.close()
        assert _bytes(up) == _bytes(free) and np.isfinite(up["upper"])
        assert capi.lib().dotsocp_canary_check() == 0, capi.lib().dotsocp_last_error().decode()
    print("child ok")


def test_between_guard_bands_and_on_poisoned_memory():
    code = "import sys; sys.path.insert(0, sys.argv[1]); import test_gpu_upper as T; T._child()"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), DOTSOCP_CANARY="1", DOTSOCP_POISON="1")
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "tests")], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("child ok"), out.stdout[-1000:] + out.stderr[-3000:]


def _generic_context(shape, nt, seed=0, finish=True, weighted=False, **split):
    """a context (no iteration) on a smooth potential of the size of a few eps"""
    rho0, rho1, f = _problem(shape, 300 + seed)
    var, model = D.initialize(rho0, rho1, nt)
    if weighted:
        model.weight = np.ones(var.q.size)
    D.InitialScaling(var, model, True, None, dim=len(shape), weighted=weighted)
    rng = np.random.default_rng(seed)
    var.phi = np.concatenate([f.ravel(order="F") * s for s in rng.uniform(0.5, 1.5, nt)])
    ctx = D.InPALMContext(var, OPTS, model, weighted=weighted, **split)
    if finish:
        ctx.finish(download=False)
    return ctx


def _sentinels(shape, sweeps):
    res = capi.Upper()
    ctypes.memset(ctypes.byref(res), 0x5a, ctypes.sizeof(res))
    return res, [np.full(shape, 7.5, order="F") for _ in range(5)] + [np.full(sweeps, 7.5)]


def _raw(ctx, r0, r1, fs, o, res, arrs, ny=None, nx=None):
    p = lambda a: None if a is None else a.ctypes.data         # noqa: E731
    tail = (p(fs), None if o is None else ctypes.byref(o), None if res is None else ctypes.byref(res)) + tuple(p(a) for a in arrs)
    if ctx is None:
        return capi.lib().dotsocp_plan_bound(p(r0), p(r1), ny, nx, *tail, 0)
    return capi.lib().dotsocp_upper_bound(ctx._ctx, p(r0), p(r1), *tail)


def _refused(code, word, ctx, r0, r1, fs, o, shape, with_res=True, **dims):
    """the call returns `code`, its message holds `word`, and neither the struct nor the six arrays were written"""
    res, arrs = _sentinels(shape, 4)
    mark = bytes(res)
    assert _raw(ctx, r0, r1, fs, o, res if with_res else None, arrs, **dims) == code, word
    msg = capi.lib().dotsocp_last_error()
    assert word.encode() in msg, msg
    assert bytes(res) == mark and all(np.all(a == 7.5) for a in arrs), word


def test_argument_errors_leave_the_outputs_untouched():
    ny, nx = 9, 7
    good = lambda **kw: capi.UpperOpts(**dict(dict(eps_h2=0.25, max_sweeps=4, defect_tol=0.0, start=0), **kw))     # noqa: E731
    ctx = _generic_context((ny, nx), 4, finish=False)
    r0, r1 = np.asfortranarray(ctx.model.rho0), np.asfortranarray(ctx.model.rho1)
    fs = np.zeros((ny, nx), order="F")
    try:
        _refused(ESTATE, "upper_bound() needs finish()", ctx, r0, r1, None, good(), (ny, nx))
        with pytest.raises(capi.DotsocpError) as ei:
            ctx.upper_bound()
        assert ei.value.code == ESTATE
        ctx.finish(download=False)
        for c, dims in ((ctx, {}), (None, dict(ny=ny, nx=nx))):
            ref = lambda word, a=r0, b=r1, f=None, o=good(), **kw: _refused(EINVAL, word, c, a, b, f, o, (ny, nx), **dict(dims, **kw))   # noqa: E731
            ref("NULL", a=None)
            ref("NULL", b=None)
            ref("NULL", with_res=False)
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
            ref("start is", o=good(start=-1))
            ref("needs f_start", o=good(start=2))
        _refused(EINVAL, "needs a context", None, r0, r1, fs, good(start=1), (ny, nx), ny=ny, nx=nx)
        _refused(EINVAL, "two nodes", None, r0, r1, None, good(), (ny, nx), ny=ny * nx, nx=1)
        _refused(EINVAL, "2^20", None, r0, r1, None, good(), (ny, nx), ny=1, nx=(1 << 20) + 1)
        # null optional outputs are accepted, any subset of them
        res = capi.Upper()
        assert _raw(ctx, r0, r1, None, good(start=1), res, [None] * 6) == 0
        full = ctx.upper_bound(max_sweeps=4, arrays=True)
        assert res.n_nodes == ny * nx and _bits(res.upper)[0] == _bits(full["upper"])[0]
        _, arrs = _sentinels((ny, nx), 4)
        assert _raw(ctx, r0, r1, None, good(start=1), res, [None, arrs[1], None, None, arrs[4], arrs[5]]) == 0
        assert np.array_equal(_bits(arrs[1]), _bits(full["g"])) and np.array_equal(_bits(arrs[4]), _bits(full["ec"]))
        assert np.array_equal(_bits(arrs[5]), _bits(full["defects"]))
        with pytest.raises(ValueError):
            ctx.upper_bound(eps_h2=0.0)
        with pytest.raises(ValueError):
            ctx.upper_bound(start=2)
    finally:
        ctx.close()
    ctx = _generic_context((ny, nx), 4, weighted=True)     # a weighted context: its cost is not the Euclidean one
    try:
        _refused(EINVAL, "weighted", ctx, r0, r1, None, good(), (ny, nx))
    finally:
        ctx.close()


def test_rccl_contexts_are_refused():
    rho0, rho1 = D.get_example_2d("example1", 16, 16)
    var, model = D.initialize_slab(rho0, rho1, 8, 0, 8)
    D.InitialScaling(var, model, True, None, dim=2)
    ctx = D.InPALMContext(var, dict(OPTS, maxit=2), model, rccl=(D.capi.rccl_unique_id(), 0, 1))
    try:
        ctx.run(-1)
        ctx.finish(download=False)
        with pytest.raises(capi.DotsocpError) as ei:
            ctx.upper_bound()
        assert ei.value.code == EINVAL and "RCCL" in str(ei.value)
        _refused(EINVAL, "RCCL", ctx, np.asfortranarray(rho0), np.asfortranarray(rho1), None, capi.UpperOpts(0.25, 4, 0.0, 1), (16, 16))
    finally:
        ctx.close()


def test_drivers_take_the_keyword():
    rho0, rho1 = D.get_example_2d("example1", 17, 17)
    with pytest.raises(ValueError, match="upper= needs transfer='device'"):
        D.solver_dotsocp2d(rho0, rho1, 5, 1, dict(tol=1e-2, maxit=5), transfer="host", upper=dict(max_sweeps=2))
    out = D.solver_dotsocp2d(rho0, rho1, 9, 1, dict(tol=1e-3, maxit=200), dual=True, upper=dict(eps_h2=0.25, max_sweeps=20, defect_tol=0.0))[0]
    assert isinstance(out["upper"], U.UpperBound) and out["upper"]["sweeps"] == 20
    assert out["dual"]["bound"] <= out["upper"]["upper"]
    assert "upper" not in D.solver_dotsocp2d(rho0, rho1, 5, 1, dict(tol=1e-2, maxit=5))[0]


def test_interleaved_with_the_other_calls():
    """upper_bound() between dual_bound() and report() on one context (2 time slabs): each result equals the same call made
    first on a fresh context"""
    raw = {"report": lambda r: b"".join(np.asarray(r[k]).tobytes() for k in sorted(r)), "dual_bound": _bytes, "upper_bound": _bytes}
    call = {"report": lambda c: c.report(), "dual_bound": lambda c: c.dual_bound(arrays=True),
            "upper_bound": lambda c: c.upper_bound(max_sweeps=3, arrays=True)}
    order = ["report", "upper_bound", "dual_bound", "upper_bound", "report", "upper_bound", "dual_bound"]
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


def test_kernel_times_are_fed():
    ctx = _generic_context((65, 33), 3, seed=3)
    try:
        capi.check(capi.lib().dotsocp_set_profiling(ctx._ctx, 1))
        ctx.upper_bound(max_sweeps=2)
        t = {k: ctx.kernel_time(k) for k in ("sl_pass_x", "sl_pass_y", "sl_node")}
    finally:
        ctx.close()
    print(t)
    assert t["sl_pass_x"][1] == 2 * 2 + 4 and t["sl_pass_y"][1] == 2 * 2 + 4 and t["sl_node"][1] == 1 + 1 + 2 * 2 + 4
    assert all(ms > 0.0 for ms, _ in t.values())
