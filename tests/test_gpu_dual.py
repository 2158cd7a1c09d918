"""The dual lower bound on the device (csrc/hopflax.hip, csrc/solver_dual.hip, dotsocp_dual_bound,
InPALMContext.dual_bound()) against its numpy twin (dual.dual_bound) on the downloaded, recovered phi of the SAME context:
every float as bits, every index exactly.

Potentials are made here: phi entries s * 10^u (s normal, u uniform in [-4, -1], seeded) -- from far below to far above
the distance table's entries (0.5 h)^2 d^2, so near and far nodes win --, rho0 / rho1 positive with a few exact zeros;
uploaded, begin(), no iteration, finish().  Sizes: ragged and exact shapes in 2-D and 1-D, and one length below, at and above every size
the kernels have (hopflax.hip / kernels.h): the wavefront (64), the 256 outputs of a slice and the HL_YOUT = 1024 outputs
of a workgroup of the y pass, its chunk HL_CHUNK_MAX = 1024; the 64 lines, HL_XOUT = 32 outputs and HL_XCHUNK_MAX = 32
inputs of a workgroup of the x pass; with DOTSOCP_HL_CHUNK=7 also the chunk itself, and lines of many chunks."""
import contextlib
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dotsocp_amd as D
from dotsocp_amd import capi
from dotsocp_amd import dual as DU

from test_dual_host import asymmetric_problem, exact_w2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = -1, -4
OPTS = dict(tau=1.9, sigma=1.0, tol=0.0, maxit=1, ifCheckStepByStep=False, scaling=True)


@contextlib.contextmanager
def _chunk(n):
    """DOTSOCP_HL_CHUNK=n around the calls of the block (the library reads it at every call)"""
    old = os.environ.get("DOTSOCP_HL_CHUNK")
    if n is not None:
        os.environ["DOTSOCP_HL_CHUNK"] = str(n)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("DOTSOCP_HL_CHUNK", None)
        else:
            os.environ["DOTSOCP_HL_CHUNK"] = old


def _density(rng, shape):
    r = rng.uniform(0.5, 1.5, shape)
    r.flat[rng.choice(r.size, 3, replace=False)] = 0.0
    return r


def _potential(rng, n):
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-4, -1, n)


def _context(shape, nt, seed=0, phi=None, scaling=True, method="inPALM", opts=OPTS, **split):
    """A finished context (no iteration) on a generic potential, or on `phi` (shape + (nt,))"""
    rng = np.random.default_rng(20270 + seed)
    var, model = D.initialize(_density(rng, shape), _density(rng, shape), nt)
    D.InitialScaling(var, model, scaling, None, dim=len(shape))
    var.phi = _potential(rng, var.phi.size) if phi is None else np.asarray(phi, dtype=np.float64).ravel(order="F")
    ctx = D.InPALMContext(var, opts, model, method=method, **split)
    ctx.finish(download=False)
    return ctx


def _twin(ctx):
    """dual.dual_bound of the downloaded phi in original units (recoverOrgVar: dScale * phi)"""
    m = ctx.model
    shape = (int(m.nx),) if not hasattr(m, "ny") else (int(m.ny), int(m.nx))
    phi = ctx.download(capi.F_PHI, np.empty(int(np.prod(shape)) * int(m.nt)))
    phi = (ctx.var.dScale * phi).reshape(shape + (int(m.nt),), order="F")
    return DU.dual_bound(phi[..., 0], phi[..., -1], m.rho0, m.rho1)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel(order="F")).view(np.uint64)


def _bytes(d):
    return b"".join(np.asarray(d[k]).tobytes(order="F") for k in sorted(d))


def _same(dev, twin, arrays=True):
    for k in DU.FIELDS:
        print("  %-13s %-24r %r" % (k, dev[k], twin[k]))
    for k in DU.FIELDS:
        assert _bits(dev[k])[0] == _bits(twin[k])[0] if isinstance(twin[k], float) else dev[k] == twin[k], k
    if not arrays:
        return
    for k in ("H", "B"):
        assert dev[k].shape == twin[k].shape and np.array_equal(_bits(dev[k]), _bits(twin[k])), k
    for k in ("arg_fwd", "arg_bwd"):
        assert dev[k].dtype == np.int32 and dev[k].shape == twin[k].shape and np.array_equal(dev[k], twin[k]), k


def _check(shape, nt, seed=0, chunk=None, **kw):
    ctx = _context(shape, nt, seed, **kw)
    try:
        with _chunk(chunk):
            dev = ctx.dual_bound(arrays=True)
            again = ctx.dual_bound(arrays=True)
        twin = _twin(ctx)
    finally:
        ctx.close()
    print(shape, nt, "chunk", chunk, kw)
    _same(dev, twin)
    assert _bytes(dev) == _bytes(again)                        # two consecutive calls: identical bytes
    assert dev["n_nodes"] == int(np.prod(shape)) and dev["nonfinite"] == 0
    assert len(set(np.unique(dev["arg_fwd"]))) > 1              # the potential moves the winners about
    return dev


# ragged and exact shapes; one below / at / above the x pass's 64 lines with its 32 outputs and inputs; the y pass's wavefront,
# slice and workgroup (= its chunk); both passes with several workgroups per line
SHAPES_2D = [(37, 29, 3), (64, 64, 3), (67, 131, 2), (63, 31, 2), (65, 33, 2), (255, 3, 2), (256, 3, 2), (257, 3, 2),
             (1023, 3, 2), (1024, 3, 2), (1025, 3, 2), (1025, 33, 2)]
SHAPES_1D = [(300, 3), (5000, 2), (63, 2), (64, 2), (65, 2), (255, 2), (256, 2), (257, 2), (1023, 2), (1024, 2), (1025, 2)]


@pytest.mark.parametrize("ny,nx,nt", SHAPES_2D, ids=lambda v: str(v))
def test_2d_equals_the_twin(ny, nx, nt):
    _check((ny, nx), nt, seed=ny + nx)


@pytest.mark.parametrize("n,nt", SHAPES_1D, ids=lambda v: str(v))
def test_1d_equals_the_twin(n, nt):
    _check((n,), nt, seed=n)


@pytest.mark.parametrize("shape,nt", [((300,), 3), ((6,), 2), ((7,), 2), ((8,), 2), ((15,), 2), ((37, 29), 3), ((65, 33), 2),
                                      ((9, 8), 2)], ids=lambda v: str(v))
def test_small_chunks_equal_the_twin(shape, nt):
    """DOTSOCP_HL_CHUNK=7: the 300-node line takes 43 chunks; lengths below, at and above the chunk; both passes in 2-D"""
    dev = _check(shape, nt, seed=sum(shape), chunk=7)
    ctx = _context(shape, nt, seed=sum(shape))
    try:
        assert _bytes(ctx.dual_bound(arrays=True)) == _bytes(dev)           # the chunk length changes no bit
    finally:
        ctx.close()


def test_row_length_that_takes_the_second_padding():
    """ny = 512: rows of 528 doubles (DOTSOCP_PITCH2); nt reduced to stay small"""
    _check((512, 5), 2, seed=512)


def _special_line(n, at, w):
    """10.0 everywhere but: w * [0, 1, 0] from `at` - 1 on (the middle output has three equal candidates, the first of them in
    the chunk before `at`), -0.0 / +0.0 behind it, then NaN, +Inf, -Inf"""
    f = np.full(n, 10.0)
    f[at - 1:at + 2] = [0.0, w, 0.0]
    f[at + 3:at + 5] = [-0.0, 0.0]
    f[at + 6:at + 9] = [np.nan, np.inf, -np.inf]
    return f


def test_ties_zeros_and_non_finite_entries_at_a_chunk_boundary():
    n, at, nt = 24, 8, 2
    w = (0.5 * (1.0 / (n - 1))) * (1.0 / (n - 1))
    line = _special_line(n, at, w)
    # 1-D, unscaled (dScale = 1: the device sees these very doubles); both layers carry the line
    ctx = _context((n,), nt, phi=np.stack([line, -line], axis=1), scaling=False)
    try:
        with _chunk(8):
            dev = ctx.dual_bound(arrays=True)
        twin = _twin(ctx)
    finally:
        ctx.close()
    _same(dev, twin)
    assert dev["nonfinite"] == 6
    assert dev["arg_fwd"][at] == at - 1 and dev["H"][at] == w          # three equal candidates: the one of the chunk before wins
    assert dev["arg_bwd"][at] == at - 1 and dev["B"][at] == -w
    assert dev["arg_fwd"][at + 3] == at + 3 and dev["H"][at + 3] == 0.0 and not np.signbit(dev["H"][at + 3])     # -0.0 + 0.0 w
    assert dev["arg_bwd"][at + 4] == at + 4 and dev["B"][at + 4] == 0.0 and np.signbit(dev["B"][at + 4])         # -0.0 - 0.0 w
    assert np.all(np.isfinite(dev["H"])) and np.all(np.isfinite(dev["B"]))
    # 2-D: the line along x in one row and along y in one column, a row without a finite entry, chunks of 8 in both passes
    ny, nx = 24, 24
    lay = np.full((ny, nx), 10.0)
    lay[5, :] = line
    lay[:, 17] = line
    lay[20, :] = np.nan
    ctx = _context((ny, nx), nt, phi=np.stack([lay, -lay], axis=2), scaling=False)
    try:
        with _chunk(8):
            dev = ctx.dual_bound(arrays=True)
        twin = _twin(ctx)
    finally:
        ctx.close()
    _same(dev, twin)
    assert dev["nonfinite"] == 2 * np.count_nonzero(~np.isfinite(lay))
    # every node of both layers non-finite: index 0 everywhere, the bound is not a number
    ctx = _context((9, 7), nt, phi=np.full((9, 7, nt), np.nan), scaling=False)
    try:
        dev = ctx.dual_bound(arrays=True)
        twin = _twin(ctx)
    finally:
        ctx.close()
    _same(dev, twin)
    assert np.all(dev["arg_fwd"] == 0) and np.all(dev["arg_bwd"] == 0) and np.all(dev["H"] == np.inf) and np.all(dev["B"] == -np.inf)
    assert dev["nonfinite"] == 2 * 63 and np.isnan(dev["bound"]) and dev["gap1_max"] == -np.inf and dev["gap1_min"] == np.inf


def test_scaled_context_after_real_iterations():
    """scaling=True and 12 iterations (the in-loop rescale block has run): the units are dScale * phi of the download"""
    rho0, rho1 = asymmetric_problem()
    var, model = D.initialize(rho0, rho1, 9)
    D.InitialScaling(var, model, True, None, dim=2)
    ctx = D.InPALMContext(var, dict(OPTS, maxit=12), model)
    try:
        ctx.run(-1)
        ctx.finish(download=False)
        assert var.dScale != 1.0
        dev = ctx.dual_bound(arrays=True)
        twin = _twin(ctx)
    finally:
        ctx.close()
    _same(dev, twin)


@pytest.mark.parametrize("split", [dict(nslabs=2), dict(nslabs=3), dict(ngpu=3)], ids=lambda s: "%s%d" % next(iter(s.items())))
def test_time_slabs_give_the_same_bytes(split):
    one = _check((19, 13), 7, seed=7)
    assert _bytes(_check((19, 13), 7, seed=7, **split)) == _bytes(one)


def test_time_slabs_1d():
    assert _bytes(_check((301,), 9, seed=9, nslabs=3)) == _bytes(_check((301,), 9, seed=9))


@pytest.mark.parametrize("method", ["PALM", "acc-ADMM"])
def test_other_loops(method):
    opts = dict(OPTS, maxit=3)
    rho0, rho1 = asymmetric_problem()
    var, model = D.initialize(rho0, rho1, 5)
    D.InitialScaling(var, model, True, None, dim=2)
    ctx = D.InPALMContext(var, opts, model, method=method)
    try:
        ctx.run(-1)
        ctx.finish(download=False)
        dev = ctx.dual_bound(arrays=True)
        twin = _twin(ctx)
    finally:
        ctx.close()
    _same(dev, twin)


def _child(what):
    """Runs in a fresh process: DOTSOCP_CANARY=1 (the call's buffers lie between guard bands) or DOTSOCP_PITCH=0 (rows as
    long as the grid's; both are read once per process)"""
    if what == "canary":
        assert os.environ.get("DOTSOCP_CANARY") == "1"
    else:
        assert os.environ.get("DOTSOCP_PITCH") == "0"
    for shape, nt, chunk in (((37, 29), 3, None), ((65, 33), 2, 7), ((300,), 3, 7), ((67, 131), 2, None)):
        _check(shape, nt, seed=sum(shape), chunk=chunk)        # fails with DOTSOCP_EHIP if a band was overwritten
        assert capi.lib().dotsocp_canary_check() == 0, capi.lib().dotsocp_last_error().decode()
    _check((19, 13), 7, seed=7, nslabs=3)
    assert capi.lib().dotsocp_canary_check() == 0
    print("child ok")


@pytest.mark.parametrize("what,env", [("canary", dict(DOTSOCP_CANARY="1")), ("pitch0", dict(DOTSOCP_PITCH="0"))], ids=["canary", "pitch0"])
def test_between_guard_bands_and_without_pitch(what, env):
    code = "import sys; sys.path.insert(0, sys.argv[1]); import test_gpu_dual as T; T._child(sys.argv[2])"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "tests"), what], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("child ok"), out.stdout[-1000:] + out.stderr[-3000:]


def _raw_call(ctx, r0, r1, res, H, B, af, ab):
    p = lambda a: None if a is None else a.ctypes.data         # noqa: E731
    return capi.lib().dotsocp_dual_bound(ctx._ctx, p(r0), p(r1), None if res is None else ctypes.byref(res), p(H), p(B), p(af), p(ab))


def _sentinels(shape):
    res = capi.Dual()
    ctypes.memset(ctypes.byref(res), 0x5a, ctypes.sizeof(res))
    return res, np.full(shape, 7.5, order="F"), np.full(shape, 7.5, order="F"), \
        np.full(shape, -3, dtype=np.int32, order="F"), np.full(shape, -3, dtype=np.int32, order="F")


def _refused(code, word, ctx, r0, r1, shape, with_res=True):
    """the call returns `code`, its message holds `word`, and neither the struct nor the four arrays were written"""
    res, H, B, af, ab = _sentinels(shape)
    mark = bytes(res)
    assert _raw_call(ctx, r0, r1, res if with_res else None, H, B, af, ab) == code
    msg = capi.lib().dotsocp_last_error()
    assert word.encode() in msg, msg
    assert bytes(res) == mark and np.all(H == 7.5) and np.all(B == 7.5) and np.all(af == -3) and np.all(ab == -3)


def test_argument_errors_leave_the_outputs_untouched():
    L = capi.lib()
    ny, nx, nt = 9, 7, 4
    rng = np.random.default_rng(5)
    var, model = D.initialize(_density(rng, (ny, nx)), _density(rng, (ny, nx)), nt)
    D.InitialScaling(var, model, True, None, dim=2)
    ctx = D.InPALMContext(var, OPTS, model)
    r0, r1 = np.asfortranarray(model.rho0), np.asfortranarray(model.rho1)

    def refused(code, word, c, a, b, with_res=True):
        _refused(code, word, c, a, b, (ny, nx), with_res)

    try:
        refused(ESTATE, "dual_bound() needs finish()", ctx, r0, r1)
        with pytest.raises(capi.DotsocpError) as ei:
            ctx.dual_bound()
        assert ei.value.code == ESTATE and "dual_bound" in str(ei.value)
        ctx.finish(download=False)
        refused(EINVAL, "dual_bound", ctx, None, r1)
        refused(EINVAL, "dual_bound", ctx, r0, None)
        refused(EINVAL, "dual_bound", ctx, r0, r1, with_res=False)
        refused(EINVAL, "positive finite", ctx, np.zeros((ny, nx), order="F"), r1)
        bad = r1.copy(order="F")
        bad[2, 3] = np.inf
        refused(EINVAL, "positive finite", ctx, r0, bad)
        bad[2, 3] = np.nan
        refused(EINVAL, "positive finite", ctx, r0, bad)
        refused(EINVAL, "positive finite", ctx, -r0, r1)
        # null optional outputs are accepted, any subset of them
        res = capi.Dual()
        assert _raw_call(ctx, r0, r1, res, None, None, None, None) == 0
        full = ctx.dual_bound(arrays=True)
        assert res.n_nodes == ny * nx and _bits(res.bound)[0] == _bits(full["bound"])[0]
        _, H, B, af, ab = _sentinels((ny, nx))
        assert _raw_call(ctx, r0, r1, res, None, B, af, None) == 0
        assert np.array_equal(_bits(B), _bits(full["B"])) and np.array_equal(af, full["arg_fwd"])
        assert set(ctx.dual_bound()) == set(DU.FIELDS)             # arrays=False: the numbers alone
        assert str(full).startswith("dual: bound ")
    finally:
        ctx.close()
    # a weighted context: its cost is not the Euclidean one
    var, model = D.initialize(r0, r1, nt)
    model.weight = np.ones(var.q.size)
    D.InitialScaling(var, model, True, None, dim=2, weighted=True)
    ctx = D.InPALMContext(var, OPTS, model, weighted=True)
    try:
        ctx.finish(download=False)
        refused(EINVAL, "weighted", ctx, r0, r1)
    finally:
        ctx.close()


def test_rccl_contexts_are_refused():
    from oracle.examples import get_example_2d
    rho0, rho1 = get_example_2d("example1", 16, 16)
    var, model = D.initialize_slab(rho0, rho1, 8, 0, 8)
    D.InitialScaling(var, model, True, None, dim=2)
    ctx = D.InPALMContext(var, dict(OPTS, maxit=2), model, rccl=(D.capi.rccl_unique_id(), 0, 1))
    try:
        ctx.run(-1)
        ctx.finish(download=False)
        with pytest.raises(capi.DotsocpError) as ei:
            ctx.dual_bound()
        assert ei.value.code == EINVAL and "RCCL" in str(ei.value)
        _refused(EINVAL, "RCCL", ctx, np.asfortranarray(rho0), np.asfortranarray(rho1), (16, 16))
    finally:
        ctx.close()


def test_drivers_refuse_what_they_cannot_serve():
    rho0, rho1 = D.get_example_2d("example1", 17, 17)
    with pytest.raises(ValueError, match="dual=True needs transfer='device'"):
        D.solver_dotsocp2d(rho0, rho1, 5, 1, dict(tol=1e-2, maxit=5), transfer="host", dual=True)
    weight = D.gene_space_weight_circleInv(17, 17)
    with pytest.raises(capi.DotsocpError) as ei:
        D.solver_wdotsocp2d(rho0, rho1, 5, 1, dict(tol=1e-2, maxit=5, weight=weight), dual=True)
    assert ei.value.code == EINVAL and "weighted" in str(ei.value)
    x0, x1 = D.get_example_1d("gaussian", 65)
    out = D.solver_dotsocp1d(x0, x1, 9, 1, dict(tol=1e-3, maxit=40), dual=True)[0]
    assert isinstance(out["dual"], DU.DualBound) and out["dual"]["n_nodes"] == 65 and np.isfinite(out["dual"]["bound"])
    assert "dual" not in D.solver_dotsocp1d(x0, x1, 9, 1, dict(tol=1e-3, maxit=40))[0]


def test_one_real_solve():
    """The asymmetric 13 x 17 x 9 problem at tol 1e-4 through the driver: the bits of the twin, the certificate against the LP,
    the raw dual against the oracle's"""
    from oracle import driver as OD
    rho0, rho1 = asymmetric_problem()
    nt, opts = 9, dict(tol=1e-4)
    output = D.solver_dotsocp2d(rho0, rho1, nt, 1, opts, dual=True)[0]
    d = output["dual"]
    assert isinstance(d, DU.DualBound)
    # the same solve on a context of our own (the driver's steps; the loop is deterministic): its phi, the twin on it
    from dotsocp_amd.solvers import _driver_opts
    var, model = D.initialize(rho0, rho1, nt, lazy_zeros=True)
    D.InitialScaling(var, model, True, None, dim=2)
    ctx = D.InPALMContext(var, _driver_opts(opts, "inPALM", False), model)
    try:
        ctx.run(-1)
        ctx.finish(download=False)
        dev = ctx.dual_bound(arrays=True)
        twin = _twin(ctx)
    finally:
        ctx.close()
    _same(dev, twin)
    _same(d, twin, arrays=False)
    exact = exact_w2(rho0, rho1)
    ovar = OD.solve_single_level(rho0, rho1, nt, opts)[0]
    ophi = ovar.phi.reshape((13, 17, nt), order="F")
    oracle = DU.dual_bound(ophi[:, :, 0], ophi[:, :, -1], rho0, rho1)
    print("bound %.9g (fwd %.9g, bwd %.9g)  exact %.9g  raw %.12g  oracle's raw %.12g" %
          (d["bound"], d["bound_fwd"], d["bound_bwd"], exact, d["dual_raw"], oracle["dual_raw"]))
    assert d["bound"] <= exact + 1e-12 and d["bound"] >= 0.95 * exact
    assert abs(d["dual_raw"] - oracle["dual_raw"]) <= 1e-6 * abs(oracle["dual_raw"])


def test_interleaved_with_the_other_calls():
    """dual_bound() between outputs(), report() and render() on one context (3 time slabs): each result equals the same
    call made first on a fresh context"""
    raw = {"outputs": _bytes, "report": lambda r: b"".join(np.asarray(r[k]).tobytes() for k in sorted(r)), "dual_bound": _bytes,
           "render": lambda r: r["image"].tobytes() + np.float64(r["vmax"]).tobytes()}
    call = {"outputs": lambda c: c.outputs(), "report": lambda c: c.report(), "dual_bound": lambda c: c.dual_bound(arrays=True),
            "render": lambda c: c.render(num_frame=3)}
    order = ["report", "dual_bound", "outputs", "dual_bound", "render", "dual_bound", "report", "outputs", "render"]
    ctx = _context((19, 13), 7, seed=7, nslabs=3)
    try:
        mixed = [raw[k](call[k](ctx)) for k in order]
        twin = _twin(ctx)
        _same(ctx.dual_bound(arrays=True), twin)
    finally:
        ctx.close()
    first = {}
    for k in call:
        fresh = _context((19, 13), 7, seed=7, nslabs=3)
        try:
            first[k] = raw[k](call[k](fresh))
        finally:
            fresh.close()
    for k, got in zip(order, mixed):
        assert got == first[k], "%s differs from the same call made first on a fresh context" % k
