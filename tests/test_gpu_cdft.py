"""The convolution-based DCT (csrc/cdft.hip: Rader for 257, Bluestein for the other lengths up to 1024) on the GPU:
against scipy along every axis, against the dense product it replaces (DOTSOCP_CDFT=0), against the oracle's Poisson
solve, inside the inPALM loop against the oracle and across time slabs, and between guard bands.  The switches are read
once per process, hence the subprocesses."""
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
from oracle.examples import get_example_2d
from oracle.inpalm import InPALMState
from oracle.model import initialize_FFTkernel, oper_poisson

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("phi", "q", "z", "alpha", "beta")
rng = np.random.default_rng(257)


def _sub(code, env, *args, timeout=900):
    e = {k: v for k, v in os.environ.items() if k not in ("DOTSOCP_CDFT", "DOTSOCP_CDFT_MIN")}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", code] + list(args), env=e, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def _relerr(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


@pytest.mark.parametrize("shape", [(257, 3, 2), (7, 257, 3), (3, 5, 257), (257, 257, 5), (257, 1, 1), (1000, 6, 3),
                                   (10, 1000, 3), (4, 3, 1000), (769, 11, 2), (1, 769, 1), (1023, 2, 2), (600, 600, 4)])
def test_dctn_matches_scipy_on_the_new_lengths(shape):
    a = np.asfortranarray(rng.standard_normal(shape))
    tol = 2e-13 * np.sqrt(np.prod(shape))
    np.testing.assert_allclose(D.mirt_dctn(a), sfft.dctn(a, norm="ortho"), atol=tol)
    np.testing.assert_allclose(D.mirt_idctn(a), sfft.idctn(a, norm="ortho"), atol=tol)
    np.testing.assert_allclose(D.mirt_idctn(D.mirt_dctn(a)), a, atol=tol)


def test_dctn_matches_scipy_with_a_lowered_crossover():
    """DOTSOCP_CDFT_MIN=48: Bluestein with 128 .. 1024-point convolutions along every axis."""
    code = (
        "import numpy as np, scipy.fft as sfft, dotsocp_amd as D\n"
        "rng = np.random.default_rng(48)\n"
        "for shape in [(97, 100, 49), (193, 50, 7), (66, 385, 3)]:\n"
        "    assert all(D.dct_algorithm(n) == 'bluestein' for n in shape if n >= 48), shape\n"
        "    a = np.asfortranarray(rng.standard_normal(shape))\n"
        "    tol = 2e-13 * np.sqrt(np.prod(shape))\n"
        "    np.testing.assert_allclose(D.mirt_dctn(a), sfft.dctn(a, norm='ortho'), atol=tol)\n"
        "    np.testing.assert_allclose(D.mirt_idctn(a), sfft.idctn(a, norm='ortho'), atol=tol)\n"
        "    np.testing.assert_allclose(D.mirt_idctn(D.mirt_dctn(a)), a, atol=tol)\n"
        "print('ok')\n")
    assert "ok" in _sub(code, dict(DOTSOCP_CDFT_MIN="48"))


def test_convolution_dct_against_the_dense_product():
    """DOTSOCP_CDFT=0 sends the same lengths through the dense DCT-matrix product: two algorithms for one transform agree
    to rounding and are never bit-identical on random data -- which is what shows that the new kernels ran.  One exception:
    the Poisson solve of (5, 3, 257) has its only new length along t, where the default solve is tridiagonal and crosses no
    transform at all (p2 is bit-identical, measured); that shape is solved a second time with DOTSOCP_TSOLVE=dct (pdct2),
    which does cross axis 2 of the new path and must differ in bits like the rest."""
    code = (
        "import os, sys, numpy as np, dotsocp_amd as D\n"
        "rng = np.random.default_rng(12)\n"
        "out = {'alg': np.array([D.dct_algorithm(257), D.dct_algorithm(1000), D.dct_algorithm(769), D.dct_algorithm(300)])}\n"
        "for i, shape in enumerate([(257, 6, 3), (10, 257, 3), (5, 3, 257), (257, 257, 65), (1000, 9, 17), (18, 769, 5), (300, 1000, 9)]):\n"
        "    a = np.asfortranarray(rng.standard_normal(shape))\n"
        "    out['f%d' % i] = D.mirt_dctn(a); out['i%d' % i] = D.mirt_idctn(a)\n"
        "    out['p%d' % i] = D.oper_poisson3dim(0.37 ** 2, a)\n"
        "    if shape[2] == 257:\n"
        "        os.environ['DOTSOCP_TSOLVE'] = 'dct'\n"
        "        out['pdct%d' % i] = D.oper_poisson3dim(0.37 ** 2, a)\n"
        "        del os.environ['DOTSOCP_TSOLVE']\n"
        "np.savez(sys.argv[1], **out)\n")
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for flag in ("0", "1"):
            path = os.path.join(tmp, f"cdft{flag}.npz")
            _sub(code, dict(DOTSOCP_CDFT=flag), path)
            with np.load(path) as z:
                res[flag] = {k: z[k].copy() for k in z.files}
    assert set(res["0"].pop("alg").tolist()) == {"dense"}
    assert res["1"].pop("alg").tolist()[:2] == ["rader", "bluestein"]
    for k in res["0"]:
        ref = res["0"][k]
        np.testing.assert_allclose(res["1"][k], ref, rtol=0, atol=2e-13 * max(1.0, np.abs(ref).max()) * np.sqrt(ref.size), err_msg=k)
        if k != "p2":
            assert not np.array_equal(res["1"][k], ref), k


POISSON_SHAPES = [(257, 257, 65), (257, 129, 33), (769, 40, 17), (1000, 64, 128), (300, 1000, 9)]


@pytest.mark.parametrize("ny,nx,nt", POISSON_SHAPES)
def test_oper_poisson_on_the_new_lengths(ny, nx, nt):
    Dsc = 0.37
    rhs = np.asfortranarray(rng.standard_normal((ny, nx, nt)))
    ref = oper_poisson(Dsc ** 2 * initialize_FFTkernel(nt, nx, ny), rhs).ravel(order="F")
    got = D.oper_poisson3dim(Dsc ** 2, rhs)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * np.abs(ref).max())


def test_oper_poisson_on_the_new_lengths_unpitched():
    code = (
        "import numpy as np, dotsocp_amd as D\n"
        "from oracle.model import initialize_FFTkernel, oper_poisson\n"
        "rng = np.random.default_rng(3)\n"
        "for ny, nx, nt in %r:\n"
        "    rhs = np.asfortranarray(rng.standard_normal((ny, nx, nt)))\n"
        "    ref = oper_poisson(0.37 ** 2 * initialize_FFTkernel(nt, nx, ny), rhs).ravel(order='F')\n"
        "    got = D.oper_poisson3dim(0.37 ** 2, rhs)\n"
        "    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * np.abs(ref).max())\n"
        "print('ok')\n" % (POISSON_SHAPES,))
    assert "ok" in _sub(code, dict(DOTSOCP_PITCH="0"))


def test_inpalm_loop_against_the_oracle_on_a_bluestein_grid():
    """769 x 1000 x 9 (Bluestein along y and x, pitched rows), K = 10 iterations from the driver's start state with KKT
    checks on the way, all five state arrays <= 1e-9 as in test_parity_gate_config2."""
    ny, nx, nt, K = 769, 1000, 9, 10
    assert D.dct_algorithm(ny) == "bluestein" and D.dct_algorithm(nx) == "bluestein"
    rho0, rho1 = get_example_2d("example1", ny, nx)
    opts = dict(tol=0.0, maxit=K)
    ovar, omodel, oo = OD.make_level(rho0, rho1, nt, opts, "inPALM", None)
    st = InPALMState(ovar, oo, omodel)
    st.run()
    o_hist, o_sigma = st.finish()
    var, model = D.initialize(rho0, rho1, nt)
    D.InitialScaling(var, model, True, None, dim=2)
    assert var.D == ovar.D and var.E == ovar.E
    g_hist, g_sigma = D.solver_socp_inPALM(var, oo, model)
    assert g_hist["len"] == o_hist["len"] and g_hist["len"] >= 1
    np.testing.assert_array_equal(g_hist["iter"], o_hist["iter"])
    assert abs(g_sigma - o_sigma) <= 1e-12 * abs(o_sigma)
    np.testing.assert_allclose(g_hist["kkt"], o_hist["kkt"], rtol=1e-6, atol=1e-10)
    errs = {f: _relerr(getattr(var, f), getattr(ovar, f)) for f in FIELDS}
    assert max(errs.values()) <= 1e-9, errs


_SLAB_CODE = (
    "import numpy as np, dotsocp_amd as D\n"
    "from oracle import driver as OD\n"
    "from oracle.examples import get_example_2d\n"
    "import sys\n"
    "ny, nx, nt = [int(v) for v in sys.argv[1:4]]\n"
    "assert D.dct_algorithm(ny) == 'rader' and D.dct_algorithm(nt) == sys.argv[4], D.dct_algorithm(nt)\n"
    "rho0, rho1 = get_example_2d('example1', ny, nx)\n"
    "res = []\n"
    "for nslabs in (1, 2):\n"
    "    var, model = D.initialize(rho0, rho1, nt)\n"
    "    o = OD.default_opts(dict(tol=0.0, maxit=12), 'inPALM', False)\n"
    "    D.InitialScaling(var, model, o['scaling'], None, dim=2)\n"
    "    hist, sigma = D.solver_socp_inPALM(var, o, model, nslabs=nslabs)\n"
    "    res.append((var, hist, sigma))\n"
    "(a, ha, sa), (b, hb, sb) = res\n"
    "np.testing.assert_array_equal(hb['iter'], ha['iter'])\n"
    "np.testing.assert_allclose(hb['kkt'], ha['kkt'], rtol=1e-7, atol=1e-10)\n"
    "assert abs(sb - sa) <= 1e-12 * sa\n"
    "errs = {f: np.max(np.abs(getattr(b, f) - getattr(a, f))) / np.max(np.abs(getattr(a, f))) for f in ('phi', 'q', 'z', 'alpha', 'beta')}\n"
    "print(errs)\n"
    "assert max(errs.values()) <= 1e-10, errs\n"
    "print('ok')\n")


@pytest.mark.parametrize("nt,env,talg", [(17, {}, "pfa"), (17, {"DOTSOCP_TSOLVE": "dct"}, "pfa"),
                                         (49, {"DOTSOCP_TSOLVE": "dct", "DOTSOCP_CDFT_MIN": "48"}, "bluestein")])
def test_two_time_slabs_match_one_on_257(nt, env, talg):
    """257 x 257 x nt as two in-process time slabs against one slab, <= 1e-10 (the slab tests' bound): the partitioned
    tridiagonal t-solve, the transposes around the t-axis transform, and (nt = 49 with the crossover lowered) that transform
    through axis 2 of the new path."""
    assert "ok" in _sub(_SLAB_CODE, env, "257", "257", str(nt), talg)


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


@pytest.mark.parametrize("ny,nx,nt", [(257, 70, 9), (1000, 50, 5)])
@pytest.mark.parametrize("kw", [{}, {"ngpu": 2}], ids=["one_slab", "two_slabs"])
def test_new_lengths_between_guard_bands(ny, nx, nt, kw, monkeypatch):
    rho0, rho1 = get_example_2d("example1", ny, nx)
    monkeypatch.delenv("DOTSOCP_CANARY", raising=False)
    ref, h0, s0, o0 = _solve(rho0, rho1, nt, 6, **kw)
    monkeypatch.setenv("DOTSOCP_CANARY", "1")
    got, h1, s1, o1 = _solve(rho0, rho1, nt, 6, **kw)
    assert s0 == s1 and np.array_equal(h0["kkt"], h1["kkt"])
    for f in FIELDS:
        a = getattr(got, f)
        assert np.all(np.isfinite(a)), f
        assert np.array_equal(a, getattr(ref, f)), f
    for k in o0:
        assert np.array_equal(o0[k], o1[k]), k
