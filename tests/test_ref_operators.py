"""The oracle's five MEX operators (oracle/mex_kernels.c) against the reference's prebuilt binaries, bit for bit.

Two checks, neither marked gpu:
  * tests/golden/ref_operators.npz holds inputs and the outputs the binaries gave for them (recorded by
    tests/golden/make_golden.py): the SOC projection at K = 2, 3, 6, 10, 13 with rows from 1e-3 to 30, rows next
    to the apex and the edge rows (zero, x1 = +-||xbar||, 1e-200, 1e150, +-inf, NaN); B F q + d and its adjoint in
    2-D and 1-D at small shapes with a sentinel in the unwritten slots, every argument count the binaries handle,
    non-integer dimension doubles; the 1-D binaries' error identifiers.  Runs everywhere, never skips.
  * A seeded comparison with the live binaries in oracle/_ref/ (filled by oracle.ref_mex.build_ref()) at larger
    shapes.  Skips only when oracle/_ref/ is absent.
Through the HIP kernels' bit-exact tests against the oracle (tests/test_gpu_operators.py) this pins the kernels to
the reference too."""
import os
import sys

import numpy as np
import pytest

from oracle import mexops as O, ref_mex as R

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden import ERR_BINARIES, SENTINEL, err_case_args  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "ref_operators.npz"), allow_pickle=False)
PROJ_K = (2, 3, 6, 10, 13)
N2D = len([k for k in G.files if k.startswith("bfd") and k.endswith("_sdF") and not k.startswith("bfd1d")])
N1D = len([k for k in G.files if k.startswith("bfd1d") and k.endswith("_sdF")])


def same_bits(a, b, nan_bits=True):
    """Equal bit for bit, signed zeros included.  nan_bits=False: a NaN matches any NaN (the GPU's 0/0 is the
    positive quiet NaN, x86's the negative one)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    ia, ib = a.view(np.int64), b.view(np.int64)
    if nan_bits:
        return np.array_equal(ia, ib)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(ia[~na], ib[~nb])


def fixture_cases(M):
    """Every operator case of the fixture run through module M (oracle.mexops or dotsocp_amd): yields
    (label, got, expected)."""
    for K in PROJ_K:
        x = G["proj%d_in" % K]
        p = np.full_like(x, SENTINEL, order="F")
        M.mexProjSoc(p, x)
        yield "proj K=%d" % K, p, G["proj%d_out" % K]
    for c in range(N2D):
        dims, (s, dF) = G["bfd%d_dims" % c], G["bfd%d_sdF" % c]
        nt, nx, ny = (int(v) for v in dims)
        z = np.full(G["bfd%d_z" % c].shape, SENTINEL, order="F")
        M.mexBFd(z, G["bfd%d_q" % c], nt, nx, ny, s, dF)
        yield "mexBFd %s" % dims, z, G["bfd%d_z" % c]
        q = np.full(G["bfdc%d_q" % c].shape, SENTINEL)
        M.mexBFdConj(q, G["bfdc%d_w" % c], nt, nx, ny, s)
        yield "mexBFdConj %s" % dims, q, G["bfdc%d_q" % c]
    for c in range(N1D):
        dims, sdF = G["bfd1d%d_dims" % c], [float(v) for v in G["bfd1d%d_sdF" % c]]
        nt, nx = (int(v) for v in dims)
        z = np.full(G["bfd1d%d_z" % c].shape, SENTINEL, order="F")
        M.mexBFd1d(z, G["bfd1d%d_q" % c], nt, nx, *sdF)
        yield "mexBFd1d %s %s" % (dims, sdF), z, G["bfd1d%d_z" % c]
        q = np.full(G["bfdc1d%d_q" % c].shape, SENTINEL)
        M.mexBFdConj1d(q, G["bfdc1d%d_w" % c], nt, nx, *sdF[:1])
        yield "mexBFdConj1d %s %s" % (dims, sdF[:1]), q, G["bfdc1d%d_q" % c]


def test_fixture_covers_the_cases():
    """The fixture holds what the comparisons below rely on: edge rows, apex rows, sentinels, every arity."""
    for K in PROJ_K:
        x, p = G["proj%d_in" % K], G["proj%d_out" % K]
        assert np.isnan(p).any() and np.isinf(x).any() and (np.abs(x) == 1e-200).any() and (x == 1e150).any()
        assert not (p == SENTINEL).any()
    assert N2D >= 6 and N1D >= 5
    assert any((G["bfd%d_z" % c] == SENTINEL).any() for c in range(N2D))           # unwritten slots recorded
    assert {len(G["bfd1d%d_sdF" % c]) for c in range(N1D)} == {0, 1, 2}
    assert {"mexBFd:invalidNumInputs", "mexBFd:invalidNumOutputs", "mexBFd:invalidInput",
            "oper_BFd_c:invalidInput"} <= set(G["err1d_id"].tolist())


def test_oracle_reproduces_the_reference_fixture():
    bad = [label for label, got, exp in fixture_cases(O) if not same_bits(got, exp)]
    assert not bad, "oracle differs from the reference binaries' recorded outputs: %s" % bad


# ---------------------------------------------------------------------------------------------------------------
# live binaries (oracle/_ref/)
# ---------------------------------------------------------------------------------------------------------------
live = pytest.mark.skipif(not R.available(), reason="oracle/_ref/ is absent (no reference checkout when "
                                                    "oracle.ref_mex.build_ref() ran): live comparison skipped")


def _rows(rng, M, K):
    x = rng.standard_normal((M, K)) * np.geomspace(1e-3, 30.0, M)[rng.permutation(M)][:, None]
    k = M // 4
    xb = x[:k, 1:]
    x[:k, 0] = -np.sqrt((xb * xb).sum(1)) * (1.0 - np.geomspace(1e-16, 1e-4, k))     # next to the apex
    return np.asfortranarray(x)


@live
@pytest.mark.parametrize("M,K", [(777, 10), (100000, 10), (4096, 6), (3000, 2), (3000, 3), (3000, 13), (2000, 21)])
def test_proj_soc_matches_the_binary(M, K):
    x = _rows(np.random.default_rng(M * 31 + K), M, K)
    ref, got = np.full_like(x, SENTINEL, order="F"), np.full_like(x, SENTINEL, order="F")
    R.mexProjSoc(ref, x)
    O.mexProjSoc(got, x)
    assert same_bits(got, ref), "%d of %d rows differ" % ((got != ref).any(1).sum(), M)


@live
@pytest.mark.parametrize("nt,nx,ny", [(2, 1, 1), (2, 2, 2), (4, 6, 5), (3, 70, 130), (9, 17, 64), (5, 1, 100),
                                      (5, 100, 1), (9, 64, 64)])
def test_bfd_and_conj_match_the_binaries(nt, nx, ny):
    rng = np.random.default_rng(nt * 10007 + nx * 101 + ny)
    Nz = ny * nx * (nt - 1)
    Nq = Nz + ny * (nx - 1) * nt + (ny - 1) * nx * nt
    s, dF = 0.731, 1.37
    q = rng.standard_normal(Nq)
    z0 = np.asfortranarray(rng.standard_normal((Nz, 10)))      # sentinels in the unwritten slots
    ref, got = z0.copy(order="F"), z0.copy(order="F")
    R.mexBFd(ref, q, nt + 0.9, nx, ny, s, dF)
    O.mexBFd(got, q, nt, nx, ny, s, dF)
    assert same_bits(got, ref)
    w = np.asfortranarray(rng.standard_normal((Nz, 10)))
    qr, qg = np.full(Nq, SENTINEL), np.full(Nq, SENTINEL)
    R.mexBFdConj(qr, w, nt, nx, ny + 0.5, s)
    O.mexBFdConj(qg, w, nt, nx, ny, s)
    assert same_bits(qg, qr)


@live
@pytest.mark.parametrize("nt,nx", [(2, 1), (2, 2), (4, 9), (33, 129), (5, 300), (300, 33)])
@pytest.mark.parametrize("nopt", [0, 1, 2])
def test_bfd1d_and_conj1d_match_the_binaries(nt, nx, nopt):
    rng = np.random.default_rng(nt * 1009 + nx * 7 + nopt)
    Nz, Nq = nx * (nt - 1), nx * (nt - 1) + (nx - 1) * nt
    sdF = [1.21, 0.6][:nopt]
    q = rng.standard_normal(Nq)
    z0 = np.asfortranarray(rng.standard_normal((Nz, 6)))
    ref, got = z0.copy(order="F"), z0.copy(order="F")
    R.mexBFd1d(np.zeros((1, 6), order="F"), np.zeros(1), 2, 1, 1.0, 1.0)    # omitted arguments: last value passed
    R.mexBFd1d(ref, q, nt + 0.5, nx, *sdF)
    O.mexBFd1d(got, q, nt, nx, *sdF)
    assert same_bits(got, ref)
    w = np.asfortranarray(rng.standard_normal((Nz, 6)))
    qr, qg = np.full(Nq, SENTINEL), np.full(Nq, SENTINEL)
    R.mexBFdConj1d(np.zeros(1), np.zeros((1, 6), order="F"), 2, 1, 1.0)
    R.mexBFdConj1d(qr, w, nt, nx + 0.25, *sdF[:1])
    O.mexBFdConj1d(qg, w, nt, nx, *sdF[:1])
    assert same_bits(qg, qr)


@live
def test_fixture_matches_the_live_binaries():
    """The committed fixture is what the binaries in oracle/_ref/ give (outputs and 1-D error identifiers)."""
    class Ref:
        mexProjSoc = staticmethod(R.mexProjSoc)
        mexBFd = staticmethod(R.mexBFd)
        mexBFdConj = staticmethod(R.mexBFdConj)
        mexBFdConj1d = staticmethod(R.mexBFdConj1d)

        @staticmethod
        def mexBFd1d(*a):
            R.mexBFd1d(np.zeros((1, 6), order="F"), np.zeros(1), 2, 1, 1.0, 1.0)
            R.mexBFdConj1d(np.zeros(1), np.zeros((1, 6), order="F"), 2, 1, 1.0)
            R.mexBFd1d(*a)

    bad = [label for label, got, exp in fixture_cases(Ref) if not same_bits(got, exp)]
    assert not bad, bad
    for (b, nrhs, nlhs, badpos), ident in zip(G["err1d_case"].tolist(), G["err1d_id"].tolist()):
        assert (R.call(ERR_BINARIES[b], err_case_args(b, nrhs, badpos), nlhs=nlhs) or "") == ident
