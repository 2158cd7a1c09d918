"""The two-level DCT for power-of-two lines that do not fit the LDS (csrc/dct_long.hip: 4096 .. 2^20 along y, 16384 .. 2^20
along x / t) on the GPU: against scipy along every axis, in batches through the bounded scratch array, against the in-LDS
kernels it extends (DOTSOCP_DCT_LONG_MIN=256), against the oracle's Poisson solve, inside the inPALM loop against the
oracle and across time slabs, between guard bands, and the refusal of 2^21 points.  The switches are read once per
process, hence the subprocesses."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import scipy.fft as sfft

import dotsocp_amd as D
from dotsocp_amd import capi
from oracle import driver as OD
from oracle.examples import get_example_1d, get_example_2d
from oracle.inpalm import InPALMState
from oracle.model import initialize_FFTkernel, oper_poisson

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("phi", "q", "z", "alpha", "beta")
rng = np.random.default_rng(4096)


def _sub(code, env, *args, timeout=900):
    e = {k: v for k, v in os.environ.items() if k not in ("DOTSOCP_DCT_LONG_MIN", "DOTSOCP_PITCH", "DOTSOCP_TSOLVE")}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", code] + list(args), env=e, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def _relerr(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _long_axes(shape):
    return [ax for ax, n in enumerate(shape) if D.dct_levels(n, ax) == 2]


def _check_against_scipy(shape):
    a = np.asfortranarray(rng.standard_normal(shape))
    np.testing.assert_allclose(D.mirt_dctn(a), sfft.dctn(a, norm="ortho"), rtol=0, atol=2e-12)
    np.testing.assert_allclose(D.mirt_idctn(a), sfft.idctn(a, norm="ortho"), rtol=0, atol=2e-12)
    np.testing.assert_allclose(D.mirt_idctn(D.mirt_dctn(a)), a, rtol=0, atol=2e-12)


@pytest.mark.parametrize("shape,axis", [((4096, 3, 2), 0), ((8192, 1, 1), 0), ((2, 16384, 3), 1), ((3, 2, 16384), 2),
                                        ((32768, 1, 1), 0), ((65536, 2, 1), 0), ((4096, 5, 1), 0)])
def test_dctn_matches_scipy_beyond_the_lds(shape, axis):
    """Odd line counts, a single line, an uneven split (8192 = 128 x 64, 32768 = 256 x 128) and both kinds of strided
    axes; atol = 2e-12, the bar of the in-LDS power-of-two lengths."""
    assert _long_axes(shape) == [axis] and D.dct_algorithm(shape[axis]) == "fft"
    _check_against_scipy(shape)


@pytest.mark.parametrize("shape,axis", [((4096, 2100, 1), 0), ((6, 16384, 100), 1)])
def test_passes_larger_than_the_scratch_array_run_in_batches(shape, axis):
    """The scratch array of a (plan, stream) pair is bounded by 64 MB (LONG_SCRATCH_BYTES) = 1024 tiles of one pair of
    4096-point lines resp. 16 (forward) / 8 (inverse) tiles of 16 / 32 pairs of 16384-point lines: 1050 resp. 300
    pairs need a second batch, and its last tile is partial."""
    src = open(os.path.join(ROOT, "dot-socp_amd", "csrc", "dct_long.hip")).read()
    assert "#define LONG_SCRATCH_BYTES ((size_t)64 << 20)" in src
    assert 2 * np.prod(shape) * 8 > 64 << 20 and _long_axes(shape) == [axis]
    _check_against_scipy(shape)


SWITCH_SHAPES = [(256, 6, 3), (10, 512, 3), (5, 3, 2048), (2048, 7, 2), (512, 512, 16)]


def test_the_switch_against_the_in_lds_kernels():
    """DOTSOCP_DCT_LONG_MIN=256 sends lengths the LDS holds through the two-level path: two algorithms for one transform
    agree to rounding and are never bit-identical on random data -- which is what shows that the new kernels ran."""
    code = (
        "import sys, numpy as np, dotsocp_amd as D\n"
        "rng = np.random.default_rng(256)\n"
        "shapes = %r\n"
        "out = {'lev': np.array([[D.dct_levels(n, ax) for ax, n in enumerate(s)] for s in shapes])}\n"
        "for i, shape in enumerate(shapes):\n"
        "    a = np.asfortranarray(rng.standard_normal(shape))\n"
        "    out['f%%d' %% i] = D.mirt_dctn(a); out['i%%d' %% i] = D.mirt_idctn(a)\n"
        "    out['p%%d' %% i] = D.oper_poisson3dim(0.37 ** 2, a)\n"
        "np.savez(sys.argv[1], **out)\n" % (SWITCH_SHAPES,))
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, env in (("lds", {}), ("long", dict(DOTSOCP_DCT_LONG_MIN="256"))):
            path = os.path.join(tmp, name + ".npz")
            _sub(code, env, path)
            with np.load(path) as z:
                res[name] = {k: z[k].copy() for k in z.files}
    assert set(res["lds"].pop("lev").ravel().tolist()) == {1}
    lev = res["long"].pop("lev")
    for s, row in zip(SWITCH_SHAPES, lev):
        assert [int(v) for v in row] == [2 if n >= 256 else 1 for n in s], (s, row)
    for k, ref in res["lds"].items():
        got = res["long"][k]
        np.testing.assert_allclose(got, ref, rtol=0, atol=2e-13 * max(1.0, np.abs(ref).max()) * np.sqrt(ref.size), err_msg=k)
        if k[0] in "fi":
            assert not np.array_equal(got, ref), k


POISSON_SHAPES = [(4096, 1, 33), (4096, 6, 5), (8, 16384, 3), (8192, 1, 16), (3, 2, 16384)]


def _check_poisson(ny, nx, nt):
    Dsc = 0.37
    rhs = np.asfortranarray(rng.standard_normal((ny, nx, nt)))
    ref = oper_poisson(Dsc ** 2 * initialize_FFTkernel(nt, nx, ny), rhs).ravel(order="F")
    got = D.oper_poisson3dim(Dsc ** 2, rhs)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * np.abs(ref).max())


@pytest.mark.parametrize("ny,nx,nt", POISSON_SHAPES)
def test_oper_poisson_beyond_the_lds(ny, nx, nt, monkeypatch):
    assert len(_long_axes((ny, nx, nt))) == 1
    monkeypatch.delenv("DOTSOCP_TSOLVE", raising=False)
    _check_poisson(ny, nx, nt)


def test_oper_poisson_three_pass_t_step(monkeypatch):
    """nt = 16384 has no fused t pass: forward pass, division, inverse pass -- also when DOTSOCP_TSOLVE=dct rules the
    tridiagonal solve out"""
    monkeypatch.setenv("DOTSOCP_TSOLVE", "dct")
    _check_poisson(3, 2, 16384)


@pytest.mark.parametrize("ny,nx,nt", [(5, 3, 2048), (5, 3, 1024), (1, 1, 2048), (3, 1, 64)])
def test_fused_t_solve_with_an_odd_number_of_columns(ny, nx, nt, monkeypatch):
    """The reference side of the switch test above: the in-LDS fused t pass (k_dct_strided<2>) on an odd number of
    (y, x) columns -- the last column has no partner and must be divided by ITS OWN eigenvalues (it took its left
    neighbour's: 6e-3 off at (5, 3, 2048), found by the comparison with the two-level path)."""
    monkeypatch.setenv("DOTSOCP_TSOLVE", "dct")
    assert D.dct_levels(nt, 2) == 1
    _check_poisson(ny, nx, nt)


def test_oper_poisson_beyond_the_lds_unpitched():
    code = (
        "import numpy as np, dotsocp_amd as D\n"
        "from oracle.model import initialize_FFTkernel, oper_poisson\n"
        "rng = np.random.default_rng(3)\n"
        "for ny, nx, nt in [(4096, 6, 5)]:\n"
        "    rhs = np.asfortranarray(rng.standard_normal((ny, nx, nt)))\n"
        "    ref = oper_poisson(0.37 ** 2 * initialize_FFTkernel(nt, nx, ny), rhs).ravel(order='F')\n"
        "    got = D.oper_poisson3dim(0.37 ** 2, rhs)\n"
        "    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * np.abs(ref).max())\n"
        "print('ok')\n")
    assert "ok" in _sub(code, dict(DOTSOCP_PITCH="0"))


def _gpu_level(rho0, rho1, nt, opts):
    dim = 2 if np.ndim(rho0) == 2 else 1
    var, model = D.initialize(rho0, rho1, nt)
    o = OD.default_opts(opts, "inPALM", False)
    D.InitialScaling(var, model, o["scaling"], None, dim=dim, weighted=False)
    return var, model, o


def _compare_run(rho0, rho1, nt, K):
    """_compare_run of tests/test_gpu_solver.py: fields <= 1e-9, `iter` equal, sigma / cScale / dScale <= 1e-12,
    KKT rtol 1e-6 / atol 1e-10"""
    opts = dict(tol=0.0, maxit=K)
    ovar, omodel, oo = OD.make_level(rho0, rho1, nt, opts, "inPALM", None)
    st = InPALMState(ovar, oo, omodel, weighted=False)
    st.run()
    o_hist, o_sigma = st.finish()
    gvar, gmodel, go = _gpu_level(rho0, rho1, nt, opts)
    assert gvar.D == ovar.D and gvar.E == ovar.E
    g_hist, g_sigma = D.solver_socp_inPALM(gvar, go, gmodel)
    assert g_hist["len"] == o_hist["len"] and g_hist["len"] >= 1
    np.testing.assert_array_equal(g_hist["iter"], o_hist["iter"])
    assert abs(g_sigma - o_sigma) <= 1e-12 * abs(o_sigma)
    np.testing.assert_allclose(g_hist["kkt"], o_hist["kkt"], rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(g_hist["pdGap"], o_hist["pdGap"], rtol=1e-6, atol=1e-14)
    errs = {f: _relerr(getattr(gvar, f), getattr(ovar, f)) for f in FIELDS}
    assert max(errs.values()) <= 1e-9, errs
    assert abs(gvar.cScale - ovar.cScale) <= 1e-12 * ovar.cScale
    assert abs(gvar.dScale - ovar.dScale) <= 1e-12 * ovar.dScale


@pytest.mark.parametrize("nx,nt,K", [(4096, 32, 12), (8192, 16, 12)])
def test_inpalm_1d_against_the_oracle(nx, nt, K):
    """1-D problems run as ny = nx1d, nx = 1: their space axis is the contiguous one"""
    assert D.dct_levels(nx, 0) == 2
    rho0, rho1 = get_example_1d("gaussian", nx)
    _compare_run(rho0, rho1, nt, K)


@pytest.mark.parametrize("ny,nx,nt,K", [(4096, 6, 5, 8), (8, 16384, 3, 6)])
def test_inpalm_2d_against_the_oracle(ny, nx, nt, K):
    assert len(_long_axes((ny, nx, nt))) == 1
    rho0, rho1 = get_example_2d("example1", ny, nx)
    assert rho0.shape == (ny, nx)
    _compare_run(rho0, rho1, nt, K)


def test_two_time_slabs_match_one():
    """4096 x 6 x 8 as two in-process time slabs against one: fields <= 1e-10, KKT rtol 1e-7 (the slab tests' bounds); the
    per-device plan of the y axis serves both slabs, each on its own stream with its own scratch array"""
    rho0, rho1 = get_example_2d("example1", 4096, 6)
    res = []
    for nslabs in (1, 2):
        var, model = D.initialize(rho0, rho1, 8)
        o = OD.default_opts(dict(tol=0.0, maxit=12), "inPALM", False)
        D.InitialScaling(var, model, o["scaling"], None, dim=2)
        hist, sigma = D.solver_socp_inPALM(var, o, model, nslabs=nslabs)
        res.append((var, hist, sigma))
    (a, ha, sa), (b, hb, sb) = res
    np.testing.assert_array_equal(hb["iter"], ha["iter"])
    np.testing.assert_allclose(hb["kkt"], ha["kkt"], rtol=1e-7, atol=1e-10)
    assert abs(sb - sa) <= 1e-12 * sa
    errs = {f: _relerr(getattr(b, f), getattr(a, f)) for f in FIELDS}
    assert max(errs.values()) <= 1e-10, errs


def _solve(rho0, rho1, nt, K, **kw):
    var, model = D.initialize(rho0, rho1, nt)
    o = OD.default_opts(dict(tol=0.0, maxit=K), "inPALM", False)
    D.InitialScaling(var, model, o["scaling"], None, dim=2)
    ctx = D.InPALMContext(var, o, model, **kw)
    ctx.run(-1)
    hist, sigma = ctx.finish(download=True)        # raises DotsocpError when a guard band was overwritten
    outs = ctx.outputs()
    ctx.close()
    assert capi.lib().dotsocp_canary_check() == 0, capi.lib().dotsocp_last_error().decode()
    return var, hist, sigma, outs


@pytest.mark.parametrize("kw", [{}, {"ngpu": 2}], ids=["one_slab", "two_slabs"])
def test_scratch_array_between_guard_bands(kw, monkeypatch):
    """DOTSOCP_CANARY=1: the scratch array comes from the guarded allocator like every device buffer of a context"""
    rho0, rho1 = get_example_2d("example1", 4096, 6)
    monkeypatch.delenv("DOTSOCP_CANARY", raising=False)
    ref, h0, s0, o0 = _solve(rho0, rho1, 5, 6, **kw)
    monkeypatch.setenv("DOTSOCP_CANARY", "1")
    got, h1, s1, o1 = _solve(rho0, rho1, 5, 6, **kw)
    assert s0 == s1 and np.array_equal(h0["kkt"], h1["kkt"])
    for f in FIELDS:
        a = getattr(got, f)
        assert np.all(np.isfinite(a)), f
        assert np.array_equal(a, getattr(ref, f)), f
    for k in o0:
        assert np.array_equal(o0[k], o1[k]), k


def test_a_2_to_the_21_point_axis_is_refused_before_anything_runs():
    L = capi.lib()
    n = 1 << 21
    assert D.dct_levels(n, 0) < 0 and D.dct_levels(1 << 20, 0) == 2
    a = np.zeros((n, 1, 1), order="F")
    for call in (lambda: D.mirt_dctn(a), lambda: D.mirt_idctn(a), lambda: D.oper_poisson3dim(1.0, a)):
        with pytest.raises(capi.DotsocpError) as e:
            call()
        assert e.value.code == -1 and "1048576" in str(e.value), str(e.value)
    assert not np.any(a)
    for ny, nx, nt, dim in [(n, 4, 4, 2), (4, n, 4, 2), (4, 4, n, 2), (1, n, 4, 1)]:
        p = capi.Problem()
        p.dim, p.weighted, p.ny, p.nx, p.nt = dim, 0, ny, nx, nt
        p.D = p.E = p.cScale = p.dScale = p.normc = p.normd = 1.0
        assert not L.dotsocp_create(ctypes.byref(p), 0, 1)
        assert b"1048576" in L.dotsocp_last_error(), L.dotsocp_last_error()
