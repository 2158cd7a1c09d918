"""The convolution-based DCT of csrc/cdft.hip -- Rader for 257, Bluestein for the other lengths up to 1024 -- as its
numpy prototype (tools/cdft_proto.py) against scipy's orthonormal DCT-II / DCT-III, the tables the kernels are built on,
and the selection of the transform per length through the C ABI (dotsocp_dct_algorithm) under its three switches.  CPU
only: the kernels follow the prototype step by step and are held against scipy, the dense product and the oracle on
the GPU (tests/test_gpu_cdft.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.fft as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cdft_proto import Cdft, chirp  # noqa: E402

PFA = {1025, 513, 129, 65, 33, 17, 9, 5, 3}
NMAX = 4100


@pytest.mark.parametrize("n", [257, 49, 97, 100, 193, 300, 385, 769, 1000, 1023])
def test_prototype_matches_scipy(n):
    rng = np.random.default_rng(n)
    P = Cdft(n)
    assert P.rader == (n == 257) and P.M == (256 if n == 257 else 1 << int(np.ceil(np.log2(2 * n - 1))))
    xa, xb = rng.standard_normal(n), rng.standard_normal(n)
    fa, fb = P.dct2(xa, xb)
    np.testing.assert_allclose(fa, sf.dct(xa, norm="ortho"), atol=1e-13)
    np.testing.assert_allclose(fb, sf.dct(xb, norm="ortho"), atol=1e-13)
    ia, ib = P.dct3(xa, xb)
    np.testing.assert_allclose(ia, sf.idct(xa, norm="ortho"), atol=1e-13)
    np.testing.assert_allclose(ib, sf.idct(xb, norm="ortho"), atol=1e-13)


def test_rader_tables():
    P = Cdft(257)
    assert sorted(P.pw.tolist()) == list(range(1, 257)) and sorted(P.ipw.tolist()) == list(range(1, 257))
    assert np.all((P.pw * P.ipw) % 257 == 1)                       # g^q * g^-q = 1 mod 257
    for pos in (P.pos_in, P.pos_out):
        assert pos[0] == -1 and sorted(pos[1:].tolist()) == list(range(256))
    # input p = g^q goes to q, output k = g^-q is found at q
    assert np.array_equal(P.pw[P.pos_in[1:]], np.arange(1, 257))
    assert np.array_equal(P.ipw[P.pos_out[1:]], np.arange(1, 257))


def test_chirp_exponent_is_reduced_exactly():
    n = 1023
    j = np.arange(n, dtype=np.int64)
    ld = np.longdouble
    t = -(ld(np.pi) + ld(1.2246467991473532e-16)) * ((j * j) % (2 * n)).astype(ld) / ld(n)     # pi to long-double accuracy
    ref = np.cos(t).astype(float) + 1j * np.sin(t).astype(float)
    # double arithmetic on an exponent below 2 pi: two roundings of the argument (<= 2 * 6.29 * 2^-53 = 1.4e-15) and one of
    # each of cos / sin
    assert np.abs(chirp(n) - ref).max() <= 2e-15
    naive = np.exp(-1j * np.pi * (j * j).astype(float) / n)       # what a loose GPU tolerance would still let through
    assert np.abs(naive - ref).max() > 1e-13
    # and the kernel's table is built the same way
    src = open(os.path.join(ROOT, "dot-socp_amd", "csrc", "cdft.hip")).read()
    assert "(j * j) % (2 * n)" in src


def _selection(**env):
    code = ("import json, dotsocp_amd as D\n"
            "L = D.capi.lib()\n"
            "print(json.dumps([L.dotsocp_dct_algorithm(n) for n in range(%d)] + [D.dct_algorithm(257), D.dct_algorithm(7)]))\n"
            % (NMAX + 1))
    e = {k: v for k, v in os.environ.items() if k not in ("DOTSOCP_CDFT", "DOTSOCP_CDFT_MIN", "DOTSOCP_PFA")}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", code], env=e, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    return out[:NMAX + 1], out[NMAX + 1:]


def _pow2(n):
    return n & (n - 1) == 0


def _eligible(n):
    return 48 <= n <= 1024 and not _pow2(n) and n not in PFA and n != 257


def test_selection_default():
    alg, names = _selection()
    assert names == ["rader", "dense"]
    assert alg[0] == 0 and alg[1] == 0
    for n in range(2, NMAX + 1):
        if _pow2(n):
            assert alg[n] == 1, n
        elif n in PFA:
            assert alg[n] == 2, n
        elif n == 257:
            assert alg[n] == 3
        elif not _eligible(n):
            assert alg[n] == 5, n
    assert alg[1000] == 4 and alg[1023] == 4
    el = [n for n in range(48, 1025) if _eligible(n)]
    nb = min(n for n in el if alg[n] == 4)                 # the crossover is measured, not fixed here
    for n in el:
        assert alg[n] == (4 if n >= nb else 5), (n, nb)


def test_selection_with_a_lowered_crossover():
    alg, _ = _selection(DOTSOCP_CDFT_MIN="48")
    for n in range(2, NMAX + 1):
        if _eligible(n):
            assert alg[n] == 4, n
        elif n == 257:
            assert alg[n] == 3
        else:
            assert alg[n] in (1, 2, 5), n


def test_selection_switched_off():
    alg, names = _selection(DOTSOCP_CDFT="0")
    assert 3 not in alg and 4 not in alg and names == ["dense", "dense"]
    assert alg[257] == 5 and alg[1000] == 5 and alg[1025] == 2 and alg[1024] == 1


def test_selection_without_the_prime_factor_transform():
    alg, _ = _selection(DOTSOCP_PFA="0")
    for n in PFA:
        assert alg[n] == 5, n
    assert alg[257] == 3 and alg[1000] == 4


def test_readme_names_the_switches():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "`DOTSOCP_CDFT=0`" in readme and "`DOTSOCP_CDFT_MIN=n`" in readme
