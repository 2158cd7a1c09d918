"""The two-level Bluestein DCT for the lengths whose convolution does not fit the LDS (csrc/cdft_long.hip), without a GPU:
the numpy model the kernels follow (tools/cdft_long_proto.py) against scipy, the tables it shares with the kernels, and
dotsocp_cdft_levels -- which lengths take the two-level convolution, by default, with DOTSOCP_CDFT_LONG_MIN and with
DOTSOCP_CDFT=0.  The kernels themselves are held against scipy, the other families and the oracle on the GPU
(tests/test_gpu_cdft_long.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.fft as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cdft_long_proto as proto  # noqa: E402

PFA = {1025, 513, 129, 65, 33, 17, 9, 5, 3}
MAX_N = (1 << 19) - 1
SPLITS = [(129, 512, (32, 16)), (130, 512, (32, 16)), (300, 1024, (32, 32)), (1000, 2048, (64, 32)), (1026, 4096, (64, 64)),
          (1536, 4096, (64, 64)), (1537, 4096, (64, 64)), (2049, 8192, (128, 64)), (4097, 16384, (128, 128)),
          (4101, 16384, (128, 128)), (16385, 65536, (256, 256)), (65537, 262144, (512, 512)),
          (524287, 1 << 20, (1024, 1024))]


@pytest.mark.parametrize("n,M,split", SPLITS)
def test_model_matches_scipy(n, M, split):
    """Forward, inverse and round trip on two lines riding as one complex line.  Bar: 2e-14 absolute on orthonormal
    transforms of standard-normal data, the bar of test_dct_long_algorithm.py: two M-point FFTs and six complex
    multiplications give about eps * (2 log2 M + 8) = 5e-15 relative to the largest value (at most 5); the model's worst
    error over these lengths is 7.1e-15."""
    P = proto.CdftLong(n)
    assert P.M == M and (P.m1, P.m2) == split
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


@pytest.mark.parametrize("n", [129, 130, 1536, 1537, 2049, 4101])
def test_every_column_of_the_last_pass_meets_its_mirror_once(n):
    """odd and even n mod m2, n a multiple of m2 (column 0 mirrors itself) and n = 1 mod m2: the (primary, mirror) pairs
    of the forward last pass cover every column exactly once and sum to n mod m2"""
    P = proto.CdftLong(n)
    pairs = P.mirror_columns()
    assert len(pairs) == P.m2 // 2
    cols = [c for pr in pairs for c in pr]
    selfm = [c for c in range(P.m2) if (n - c) % P.m2 == c]
    assert sorted(cols) == list(range(P.m2))
    for a, b in pairs:
        assert (a + b) % P.m2 == n % P.m2 or (a in selfm and b in selfm)
    assert len(selfm) == (0 if n % 2 else 2)


def test_factored_twiddles_and_tables():
    """exp(-2 pi i m / M) as hi[m >> lg m2] * lo[m mod m2] stays within 4e-16 of the long-double value for every kind of
    m = j2 * k1 of the largest convolution; the chirp's exponent is reduced in integers, in the model and in the kernel
    file, which has no device sincos"""
    P = proto.CdftLong(MAX_N)
    rng = np.random.default_rng(5)
    m = rng.integers(0, 1 << 20, 4096)
    assert np.abs(P.twiddle(m) - proto.unit(m, 1 << 20)).max() <= 4e-16
    n = 4101
    j = np.arange(n, dtype=np.int64)
    ld = np.longdouble
    t = -(ld(np.pi) + ld(1.2246467991473532e-16)) * ((j * j) % (2 * n)).astype(ld) / ld(n)     # pi to long-double accuracy
    ref = np.cos(t).astype(float) + 1j * np.sin(t).astype(float)
    assert np.abs(proto.CdftLong(n).chirp - ref).max() <= 4e-16
    src = open(os.path.join(ROOT, "dot-socp_amd", "csrc", "cdft_long.hip")).read()
    assert "(j * j) % (2 * n)" in src and "sincos" not in src


LENGTHS = sorted(set(list(range(0, 4200)) + [8192, 8193, 16385, 32769, 65536, 65537, 100000, 1 << 19, MAX_N - 1, MAX_N,
                                            MAX_N + 2, (1 << 19) + 3, (1 << 20) + 1, 1 << 20]))


def _levels(**env):
    code = ("import json, dotsocp_amd as D\n"
            "L = D.capi.lib()\n"
            "print(json.dumps([[L.dotsocp_cdft_levels(n), L.dotsocp_dct_algorithm(n), D.cdft_levels(n)] for n in %r]))\n"
            % (LENGTHS,))
    e = {k: v for k, v in os.environ.items()
         if k not in ("DOTSOCP_CDFT", "DOTSOCP_CDFT_MIN", "DOTSOCP_CDFT_LONG_MIN", "DOTSOCP_PFA")}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", code], env=e, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(a == c for a, _, c in out)                  # the Python wrapper answers what the C ABI answers
    return {n: (a, alg) for n, (a, alg, _) in zip(LENGTHS, out)}


def _served_elsewhere(n):
    return n <= 1 or n & (n - 1) == 0 or n in PFA


def _check(got, first, default=False):
    """2 exactly for the lengths from `first` up to 2^19 - 1 that are neither powers of two nor prime-factor lengths; below
    `first`, 1 for 257 and the in-LDS Bluestein range (whose start is measured: read from the answers), 0 elsewhere"""
    el = [n for n in LENGTHS if 48 <= n <= 1024 and n < first and not _served_elsewhere(n) and n != 257]
    ones = [n for n in el if got[n][0] == 1]
    nb = min(ones) if ones else 1025
    for n in LENGTHS:
        lv, alg = got[n]
        if _served_elsewhere(n):
            assert lv == 0 and alg in (0, 1, 2), n
        elif first <= n <= MAX_N:
            assert lv == 2 and alg == 4, n
        elif n == 257:
            assert lv == 1 and alg == 3
        elif n in el and n >= nb:
            assert lv == 1 and alg == 4, n
        else:
            assert lv == 0 and alg == 5, n
        assert proto.levels(n, long_min=None if default else first, cdft_min=nb) == lv, n


def test_levels_default():
    got = _levels()
    first = min(n for n in LENGTHS if n > 4100 and got[n][0] == 2)      # the measured default: never below 4101
    assert first >= 4101
    _check(got, first, default=True)
    assert got[1000][0] == 1 and got[257][0] == 1 and got[4100][0] == 0 and got[1026][0] == 0
    assert got[65537] == (2, 4) and got[MAX_N] == (2, 4) and got[(1 << 19) + 3][0] == 0 and got[1 << 19][0] == 0
    assert proto.DEFAULT_MIN == first


@pytest.mark.parametrize("value,first", [("129", 129), ("1026", 1026), ("1", 129)])
def test_levels_with_DOTSOCP_CDFT_LONG_MIN(value, first):
    """the switch names the smallest length that takes the two-level convolution on every axis, never below 129 -- also
    where the LDS convolution (257, 1000) or the dense product (1026 .. 4100) would serve it"""
    got = _levels(DOTSOCP_CDFT_LONG_MIN=value)
    _check(got, first)
    assert got[128][0] == 0 and got[130][0] == (2 if first == 129 else 0)
    assert got[257][0] == (2 if first <= 257 else 1) and got[1000][0] == (2 if first <= 1000 else 1)
    assert got[2049] == (2, 4) and got[4097] == (2, 4) and got[1025] == (0, 2) and got[129] == (0, 2)


def test_levels_switched_off():
    for env in (dict(DOTSOCP_CDFT="0"), dict(DOTSOCP_CDFT="0", DOTSOCP_CDFT_LONG_MIN="129")):
        got = _levels(**env)
        assert all(lv == 0 for lv, _ in got.values())
        assert got[4101][1] == 5 and got[65537][1] == 5 and got[1025][1] == 2 and got[4096][1] == 1


def test_readme_names_the_switch():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "`DOTSOCP_CDFT_LONG_MIN=n`" in readme and "csrc/cdft_long.hip" in readme
