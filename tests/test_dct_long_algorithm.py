"""The two-level DCT for power-of-two lines beyond the LDS (csrc/dct_long.hip), without a GPU: the numpy model the
kernels follow (tools/dct_long_proto.py) against scipy, and dotsocp_dct_levels -- which lengths take the two-level path
along which axis, by default, with DOTSOCP_DCT_LONG_MIN, and above the limit of 2^20."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.fft as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dct_long_proto as proto  # noqa: E402

LENGTHS = [0, 1, 2, 3, 16, 255, 256, 257, 512, 1000, 1024, 1025, 2048, 4095, 4096, 4097, 4100, 8192, 16383, 16384, 16385,
           32768, 65536, 1 << 19, 1 << 20, (1 << 20) + 1, 1 << 21, 1 << 22, 1 << 30]


@pytest.mark.parametrize("n,split", [(256, (16, 16)), (512, (32, 16)), (4096, (64, 64)), (8192, (128, 64)), (65536, (256, 256))])
def test_model_matches_scipy(n, split):
    """Forward and inverse on two lines travelling as one complex line.  Bar: 2e-14 absolute on orthonormal transforms of
    standard-normal data (values of order one, at most 5 in magnitude): an n-point FFT in double precision errs by
    about eps * log2(n) = 3.6e-15 at n = 65536 relative to the largest value, the factored tables add two roundings."""
    P = proto.DctLong(n)
    assert (P.n1, P.n2) == split
    rng = np.random.default_rng(n)
    xa, xb = rng.standard_normal(n), rng.standard_normal(n)
    fa, fb = P.dct2(xa, xb)
    np.testing.assert_allclose(fa, sf.dct(xa, norm="ortho"), rtol=0, atol=2e-14)
    np.testing.assert_allclose(fb, sf.dct(xb, norm="ortho"), rtol=0, atol=2e-14)
    ia, ib = P.dct3(xa, xb)
    np.testing.assert_allclose(ia, sf.idct(xa, norm="ortho"), rtol=0, atol=2e-14)
    np.testing.assert_allclose(ib, sf.idct(xb, norm="ortho"), rtol=0, atol=2e-14)
    ra, rb = P.dct3(fa, fb)
    np.testing.assert_allclose(ra, xa, rtol=0, atol=2e-14)
    np.testing.assert_allclose(rb, xb, rtol=0, atol=2e-14)


def test_model_tables_reduce_their_indices_in_integers():
    """exp(-2 pi i m / n) as hi[m // n2] * lo[m % n2] stays within three roundings of the long-double value for every
    m = j2 * k1 of the largest length"""
    P = proto.DctLong(1 << 20)
    rng = np.random.default_rng(5)
    m = rng.integers(0, 1 << 20, 4096)
    got = P.hi[m // P.n2] * P.lo[m % P.n2]
    assert np.abs(got - proto.unit(m, 1 << 20)).max() <= 4e-16
    src = open(os.path.join(ROOT, "dot-socp_amd", "csrc", "dct_long.hip")).read()
    assert "(num % den)" in src and "sincos" not in src


def _levels(**env):
    code = ("import json, dotsocp_amd as D\n"
            "print(json.dumps([[D.dct_levels(n, ax) for ax in (0, 1, 2, 3, -1)] for n in %r]))\n" % (LENGTHS,))
    e = {k: v for k, v in os.environ.items() if k != "DOTSOCP_DCT_LONG_MIN"}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", code], env=e, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _expected(n, axis, first):
    if n <= 1:
        return 0
    if n & (n - 1) or n < first:
        return 1
    return 2 if n <= 1 << 20 else -1


def test_levels_default():
    got = _levels()
    for n, row in zip(LENGTHS, got):
        assert row[3] < 0 and row[4] < 0, n                    # no such axis
        for axis in (0, 1, 2):
            want = _expected(n, axis, 4096 if axis == 0 else 16384)
            assert (row[axis] == want) if want >= 0 else (row[axis] < 0), (n, axis, row)
            assert proto.levels(n, axis) == want
    assert got[LENGTHS.index(2048)][:3] == [1, 1, 1] and got[LENGTHS.index(4096)][:3] == [2, 1, 1]
    assert got[LENGTHS.index(8192)][:3] == [2, 1, 1] and got[LENGTHS.index(16384)][:3] == [2, 2, 2]
    assert got[LENGTHS.index(1 << 20)][:3] == [2, 2, 2] and all(v < 0 for v in got[LENGTHS.index(1 << 21)][:3])
    assert got[LENGTHS.index(4100)][:3] == [1, 1, 1]           # not a power of two: the dense product, one pass


@pytest.mark.parametrize("value,first", [("256", 256), ("1", 256), ("300", 512), ("65536", 65536)])
def test_levels_with_DOTSOCP_DCT_LONG_MIN(value, first):
    """the switch names the smallest power of two that takes the two-level path on EVERY axis; never below 256, and never
    above the first length that leaves the LDS anyway (a value above that changes nothing)"""
    got = _levels(DOTSOCP_DCT_LONG_MIN=value)
    for n, row in zip(LENGTHS, got):
        for axis in (0, 1, 2):
            want = _expected(n, axis, min(first, 4096 if axis == 0 else 16384))
            assert (row[axis] == want) if want >= 0 else (row[axis] < 0), (n, axis, row)
            assert proto.levels(n, axis, int(value)) == want


def test_algorithm_keeps_answering_fft_and_the_readme_names_the_switch():
    code = "import dotsocp_amd as D\nprint([D.dct_algorithm(1 << k) for k in range(1, 23)])\n"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert set(eval(r.stdout.strip().splitlines()[-1])) == {"fft"}
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "`DOTSOCP_DCT_LONG_MIN=n`" in readme and "csrc/dct_long.hip" in readme
