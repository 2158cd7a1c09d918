"""The two-level Bluestein DCT (csrc/cdft_long.hip: lengths that are no powers of two, from 4101 -- or from
DOTSOCP_CDFT_LONG_MIN >= 129 -- up to 2^19 - 1) on the GPU: against scipy along every axis and in batches through the
bounded scratch array, against the in-LDS convolution and the dense product it extends, against the oracle's Poisson
solve, inside the inPALM loop and the multilevel driver against the oracle, across time slabs, between guard bands, and
the refusal of longer lines.  The switches are read once per process, hence the subprocesses."""
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
SWITCHES = ("DOTSOCP_CDFT", "DOTSOCP_CDFT_MIN", "DOTSOCP_CDFT_LONG_MIN")
rng = np.random.default_rng(4101)


def _sub(code, env, *args, timeout=900):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", code] + list(args), env=e, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def _relerr(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _against_scipy(a, what=""):
    """Bar: 5e-14 * max(1, max |ref|) per entry.  Two M-point FFTs and six complex multiplications give about
    eps * (2 log2 M + 8) = 5e-15 relative to the largest value, values reach about 5: 2.6e-14 at M = 2^20, doubled."""
    for name, got, ref in (("dctn", D.mirt_dctn(a), sfft.dctn(a, norm="ortho")),
                           ("idctn", D.mirt_idctn(a), sfft.idctn(a, norm="ortho")),
                           ("round trip", D.mirt_idctn(D.mirt_dctn(a)), a)):
        err = np.abs(got - ref).max()
        bar = 5e-14 * max(1.0, np.abs(ref).max())
        print(what, a.shape, name, "max error %.3e, bar %.3e" % (err, bar))
        assert err <= bar, (a.shape, name, err, bar)


@pytest.mark.parametrize("shape", [(4101, 3, 2), (3, 4101, 2), (2, 3, 4101), (4101, 1, 1), (4101, 5, 1), (65537, 3, 1),
                                   (524287, 10, 1)])
def test_dctn_matches_scipy(shape):
    """each axis; one line without a partner; an odd line count; the 512 x 512 split; the 1024 x 1024 split, whose ten
    lines exceed the 64 MB bound of the scratch array (16 MB per pair of lines): two batches"""
    assert [D.cdft_levels(n) for n in shape if n > 100] == [2]
    assert [D.dct_algorithm(n) for n in shape if n > 100] == ["bluestein"]
    _against_scipy(np.asfortranarray(rng.standard_normal(shape)))


LOW_SHAPES = [(130, 7, 3), (5, 300, 3), (3, 2, 1000), (1536, 3, 1), (1537, 2, 2), (2049, 9, 2)]

_LOW_CODE = (
    "import sys, numpy as np, scipy.fft as sfft, dotsocp_amd as D\n"
    "rng = np.random.default_rng(129)\n"
    "shapes = %r\n"
    "out = {'levels': np.array([max(D.cdft_levels(n) for n in s) for s in shapes])}\n"
    "for i, shape in enumerate(shapes):\n"
    "    a = np.asfortranarray(rng.standard_normal(shape))\n"
    "    out['a%%d' %% i] = a\n"
    "    out['f%%d' %% i] = D.mirt_dctn(a); out['i%%d' %% i] = D.mirt_idctn(a); out['r%%d' %% i] = D.mirt_idctn(out['f%%d' %% i])\n"
    "np.savez(sys.argv[1], **out)\n" % (LOW_SHAPES,))


def test_lowered_switch_against_scipy_and_the_other_families():
    """DOTSOCP_CDFT_LONG_MIN=129: the 32 x 16 (uneven), 32 x 32, 64 x 32, 64 x 64 and 128 x 64 splits, a strided axis, the
    t axis, n a multiple of m2 (column 0 is its own mirror) and n = 1 mod m2 -- against scipy at the bar of
    _against_scipy, and against the same process with the switch unset (in-LDS Bluestein at 1000, the dense product
    elsewhere): two algorithms for one transform agree to rounding (2e-13 max sqrt(size), the bar of
    test_convolution_dct_against_the_dense_product) and are never bit-identical on random data, which shows that the new
    kernels ran."""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for key, env in (("long", dict(DOTSOCP_CDFT_LONG_MIN="129")), ("ref", {})):
            path = os.path.join(tmp, key + ".npz")
            _sub(_LOW_CODE, env, path)
            with np.load(path) as z:
                res[key] = {k: z[k].copy() for k in z.files}
    assert res["long"].pop("levels").tolist() == [2] * len(LOW_SHAPES)
    assert res["ref"].pop("levels").tolist() == [0, 0, 1, 0, 0, 0]
    for i, shape in enumerate(LOW_SHAPES):
        a = res["long"]["a%d" % i]
        assert np.array_equal(a, res["ref"]["a%d" % i])
        for k, ref in (("f", sfft.dctn(a, norm="ortho")), ("i", sfft.idctn(a, norm="ortho")), ("r", a)):
            got = res["long"]["%s%d" % (k, i)]
            err, bar = np.abs(got - ref).max(), 5e-14 * max(1.0, np.abs(ref).max())
            print(shape, k, "against scipy: max error %.3e, bar %.3e" % (err, bar))
            assert err <= bar, (shape, k, err, bar)
            other = res["ref"]["%s%d" % (k, i)]
            np.testing.assert_allclose(got, other, rtol=0, atol=2e-13 * max(1.0, np.abs(other).max()) * np.sqrt(other.size),
                                       err_msg="%s %s" % (shape, k))
            assert not np.array_equal(got, other), (shape, k)


def _check_poisson(ny, nx, nt):
    Dsc = 0.37
    rhs = np.asfortranarray(rng.standard_normal((ny, nx, nt)))
    ref = oper_poisson(Dsc ** 2 * initialize_FFTkernel(nt, nx, ny), rhs).ravel(order="F")
    got = D.oper_poisson3dim(Dsc ** 2, rhs)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * np.abs(ref).max())


@pytest.mark.parametrize("ny,nx,nt", [(4101, 6, 5), (6, 4101, 3)])
def test_oper_poisson(ny, nx, nt, monkeypatch):
    monkeypatch.delenv("DOTSOCP_TSOLVE", raising=False)
    _check_poisson(ny, nx, nt)


def test_oper_poisson_with_the_transform_along_t(monkeypatch):
    """nt = 4101 has no fused t pass: with DOTSOCP_TSOLVE=dct the solve crosses axis 2 of the new path forward and back"""
    monkeypatch.setenv("DOTSOCP_TSOLVE", "dct")
    assert D.cdft_levels(4101) == 2
    _check_poisson(5, 3, 4101)


def test_oper_poisson_unpitched():
    code = (
        "import numpy as np, dotsocp_amd as D\n"
        "from oracle.model import initialize_FFTkernel, oper_poisson\n"
        "rng = np.random.default_rng(3)\n"
        "for ny, nx, nt in [(4101, 6, 5), (6, 4101, 3)]:\n"
        "    rhs = np.asfortranarray(rng.standard_normal((ny, nx, nt)))\n"
        "    ref = oper_poisson(0.37 ** 2 * initialize_FFTkernel(nt, nx, ny), rhs).ravel(order='F')\n"
        "    got = D.oper_poisson3dim(0.37 ** 2, rhs)\n"
        "    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * np.abs(ref).max())\n"
        "print('ok')\n")
    assert "ok" in _sub(code, dict(DOTSOCP_PITCH="0"))


def _compare_run(rho0, rho1, nt, K):
    """the bars of test_inpalm_loop_against_the_oracle_on_a_bluestein_grid: fields <= 1e-9, `iter` equal, sigma <= 1e-12,
    KKT rtol 1e-6 / atol 1e-10"""
    dim = 2 if np.ndim(rho0) == 2 else 1
    opts = dict(tol=0.0, maxit=K)
    ovar, omodel, oo = OD.make_level(rho0, rho1, nt, opts, "inPALM", None)
    st = InPALMState(ovar, oo, omodel, weighted=False)
    st.run()
    o_hist, o_sigma = st.finish()
    gvar, gmodel = D.initialize(rho0, rho1, nt)
    go = OD.default_opts(opts, "inPALM", False)
    D.InitialScaling(gvar, gmodel, go["scaling"], None, dim=dim, weighted=False)
    assert gvar.D == ovar.D and gvar.E == ovar.E
    g_hist, g_sigma = D.solver_socp_inPALM(gvar, go, gmodel)
    assert g_hist["len"] == o_hist["len"] and g_hist["len"] >= 1
    np.testing.assert_array_equal(g_hist["iter"], o_hist["iter"])
    assert abs(g_sigma - o_sigma) <= 1e-12 * abs(o_sigma)
    np.testing.assert_allclose(g_hist["kkt"], o_hist["kkt"], rtol=1e-6, atol=1e-10)
    errs = {f: _relerr(getattr(gvar, f), getattr(ovar, f)) for f in FIELDS}
    assert max(errs.values()) <= 1e-9, errs


def test_inpalm_1d_against_the_oracle():
    """nx = 4101, nt = 9, K = 10 from the driver's start with KKT checks on the way (1-D problems run as ny = nx1d,
    nx = 1: their space axis is the contiguous one)"""
    assert D.cdft_levels(4101) == 2
    rho0, rho1 = get_example_1d("gaussian", 4101)
    _compare_run(rho0, rho1, 9, 10)


def test_inpalm_2d_against_the_oracle():
    rho0, rho1 = get_example_2d("example1", 4101, 40)
    assert rho0.shape == (4101, 40)
    _compare_run(rho0, rho1, 5, 6)


def test_multilevel_1d_against_the_oracle():
    """solver_dotsocp1d on the gaussian at 8193 points, nt = 17, three levels (2049, 4097, 8193 points), tol = 1e-3, with
    DOTSOCP_CDFT_LONG_MIN=1026 so that every level takes the new path; the assertions of
    test_multilevel_dot1d_against_oracle: per-level iteration counts equal, rho within 1e-6.  The oracle stops at
    [339, 239, 129]; its last KKT maxima are 6 - 76 % below the level tolerances and the values before them 9 - 38 % above:
    rounding cannot move a stop."""
    code = (
        "import numpy as np, dotsocp_amd as D\n"
        "from oracle import multilevel as OM\n"
        "from oracle.examples import get_example_1d\n"
        "from oracle.driver import recover_RhoE_1d\n"
        "assert [D.cdft_levels(n) for n in (2049, 4097, 8193)] == [2, 2, 2]\n"
        "rho0, rho1 = get_example_1d('gaussian', 8193)\n"
        "ovar, omodel, ohists, osigma = OM.solve_multilevel(rho0, rho1, 17, 3, dict(tol=1e-3))\n"
        "out, timeML, histML, hist = D.solver_dotsocp1d(rho0, rho1, 17, 3, dict(tol=1e-3), 'inPALM')\n"
        "assert out['rho'].shape == (8193, 17)\n"
        "print([int(t['Iters']) for t in timeML[:3]], [int(h['iter'][-1]) for h in ohists])\n"
        "assert [int(t['Iters']) for t in timeML[:3]] == [int(h['iter'][-1]) for h in ohists]\n"
        "rho_o, _ = recover_RhoE_1d(ovar, omodel)\n"
        "np.testing.assert_allclose(out['rho'], rho_o, atol=1e-6)\n"
        "print('ok')\n")
    assert "ok" in _sub(code, dict(DOTSOCP_CDFT_LONG_MIN="1026"))


def test_two_time_slabs_match_one(monkeypatch):
    """4101 x 12 x 9 with DOTSOCP_TSOLVE=dct as two in-process time slabs against one: fields <= 1e-10, KKT rtol 1e-7 (the
    bounds of test_two_time_slabs_match_one_on_257); the per-device plan of the y axis serves both slabs, each on its own
    stream with its own scratch array"""
    monkeypatch.setenv("DOTSOCP_TSOLVE", "dct")
    rho0, rho1 = get_example_2d("example1", 4101, 12)
    res = []
    for nslabs in (1, 2):
        var, model = D.initialize(rho0, rho1, 9)
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
    rho0, rho1 = get_example_2d("example1", 4101, 9)
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


def test_a_longer_line_that_is_no_power_of_two_is_refused_before_anything_runs():
    L = capi.lib()
    n = (1 << 19) + 3
    assert D.cdft_levels(n) == 0 and D.cdft_levels((1 << 19) - 1) == 2
    a = np.zeros((n, 1, 1), order="F")
    for call in (lambda: D.mirt_dctn(a), lambda: D.mirt_idctn(a), lambda: D.oper_poisson3dim(1.0, a)):
        with pytest.raises(capi.DotsocpError) as e:
            call()
        assert e.value.code == -1 and "524287" in str(e.value), str(e.value)
    assert not np.any(a)
    for ny, nx, nt, dim in [(n, 4, 4, 2), (4, n, 4, 2), (4, 4, n, 2), (1, n, 4, 1)]:
        p = capi.Problem()
        p.dim, p.weighted, p.ny, p.nx, p.nt = dim, 0, ny, nx, nt
        p.D = p.E = p.cScale = p.dScale = p.normc = p.normd = 1.0
        assert not L.dotsocp_create(ctypes.byref(p), 0, 1)
        assert b"524287" in L.dotsocp_last_error(), L.dotsocp_last_error()
