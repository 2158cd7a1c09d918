"""Every DCT family entry by entry: one pass along one axis (dotsocp_dct_axis, the launch_dct_axis call of dotsocp_dctn for
that axis) on the probes of tests/dct_probes.py -- impulses (A), impulses beside a partner 2^30 times larger (A'), and
two modes 2^20 apart (B) -- against long-double references, forward and inverse.  Bound: 4 x the larger of scipy's and of
the family's numpy model's error on the same arrays, computed at run time; the dense family: 1 ulp on (A) / (A').  Every
case prints E_device, the CPU figures and E_device / bound per direction and probe (DESIGN.md section 5 has the table).

A shape (ny, nx, nt) with the transform along axis a has the lines of the other two extents; line l and l + 1 (memory
order) share a complex line in every FFT family.  Which kernel instance the shapes take on the 256 CUs of an MI355X
(LineMap of launch_dct_axis; `vec`: the lines per row, the row distance and the element distance are all even):

in-LDS powers of two (dct_pow2.hip, pow2_launch_axis0 / launch_strided; lp = log2 of the staged pairs)
  (8, 9, 1), (64, 9, 1), (128, 9, 1) axis 0     k_dct_axis0, one row per wave: (n / 2) 2^lp < 1024
  (1024, 1, 1) axis 0                           k_dct_axis0 on a single line (lp = 0)
  (64, 65, 1) axis 0                            k_dct_axis0_wg, 32 rows per workgroup: 32 * 2^5 = 1024
  (512, 9, 1), (1024, 9, 1), (2048, 9, 1) axis 0  k_dct_axis0_wg, four rows (2048: 139 KB of LDS); five pairs: the second
                                                workgroup holds one line
  (9, 8, 1), (9, 64, 1), (9, 1024, 1) axis 1; (3, 3, 8), (3, 3, 1024) axis 2     k_dct_strided<., false>: odd n0 resp. n0 n1
  (10, 8, 1), (10, 64, 1) axis 1; (2, 5, 64) axis 2                              k_dct_strided<., true>: n 2^lp < 1024
  (32, 64, 1), (10, 1024, 1) axis 1             k_dct_strided_wg<., 512>: n 2^lp >= 1024, and 2 x the tile <= 80 KB (64) resp.
                                                fewer than 4 * 2^lp = 16 lines (1024)
  (16, 1024, 1), (10, 2048, 1) axis 1; (2, 8, 1024) axis 2                       k_dct_strided_wg<., 1024>: 2 x the tile in
                                                (80 KB, 160 KB] and at least 4 * 2^lp lines
pipelined powers of two (lg 7 .. 11; whole tiles of 8192 doubles, 512 = 2 x 256 of them, the fewest the launchers take;
every line is checked; test_power_of_two_pipelined ASSERTS the instance through dotsocp_dct_pass_kernel)
  (128, 32768, 1), (512, 8192, 1), (2048, 2048, 1) axis 0      k_dct_axis0_pipe<., 7 / 9 / 11>, 64 / 16 / 4 lines per tile;
                                                               2048: the quarter / half tables TwQuarter, WwHalf
  (256, 16384, 1), (1024, 4096, 1) axis 0                      k_dct_axis0_pipe<., 8 / 10>, 32 / 8 lines per tile: the y
                                                               lengths of the parity-gate grid and of the benchmark grid
  (512, 128, 64), (512, 512, 16), (2048, 2048, 1) axis 1       k_dct_strided_pipe<., 7 / 9 / 11>: n0 a multiple of the tile
  (512, 256, 32), (512, 1024, 8) axis 1                        k_dct_strided_pipe<., 8 / 10>, 16 / 4 pairs per tile
  with DOTSOCP_DCT_PIPE=0 the same shapes: k_dct_axis0_wg (32 / 16 / 8 / 4 / 4 rows) resp. k_dct_strided_wg<., 1024>
  (asserted too: "pow2-wg")
two-level powers of two (dct_long.hip: k_long_cols + k_long_rows through the scratch array; n = n1 x n2)
  (4096, 9, 1), (8192, 9, 1) axis 0             64 x 64, 128 x 64: one pair per tile (lP = 0)
  (33, 16384, 1) axis 1                         128 x 128, 17 pairs: lP = 4, two tiles, the second holds one line
  (3, 3, 16384) axis 2                          five pairs: lP = 2
  (65536, 5, 1), (2^19, 5, 1), (2^20, 5, 1)     256 x 256, 1024 x 512, 1024 x 1024, three pairs; 15, 9 and 9 positions
  with DOTSOCP_DCT_LONG_MIN=256: 256 = 16 x 16, 512 = 32 x 16, 2048 = 64 x 32 along y, x and t
prime-factor (pfa.hip; 1025 = 25 x 41, 513 = 27 x 19, 129 = 3 x 43, 17, 3)
  (n, 9, 1) axis 0                              k_pfa_axis0<PfaDims, P0, T0, .>: 4 / 8 / 16 / 32 / 32 pairs per workgroup
  (9, n, 1) axis 1, (3, 3, n) axis 2            k_pfa_strided<., false>: an odd number of lines per row and no pad behind it
  (10, n, 1) axis 1, (2, 5, 129) axis 2         k_pfa_strided<., true>
Rader (257) and Bluestein inside the LDS (cdft.hip: M = 1024 for 500, 2048 for 1000 and 1023)
  (n, 9, 1) axis 0                              k_cdft<256, true, ., rader?>: 4 rows (257 and 500: five pairs), 2 (1000, 1023)
  (9, n, 1) axis 1, (3, 3, n) axis 2            k_cdft<256, false, ., .>; M = 2048: k_cdft<512, false, ., false>, four rows
  with DOTSOCP_CDFT_MIN=48: 48 (M = 128), 100 (M = 256) through the same kernels
two-level Bluestein (cdft_long.hip: k_clong_cols, k_clong_rows, k_clong_back; M = m1 x m2)
  (4101, 9, 1), (9, 4101, 1), (3, 3, 4101)      M = 16384 = 128 x 128; lP = 0 along y, 2 along x and t (five pairs)
  (65537, 5, 1), (524287, 5, 1)                 M = 2^18 = 512 x 512, 2^20 = 1024 x 1024; 15 and 5 positions (524287: one
                                                batch per probe -- its plan takes half a second to make)
  with DOTSOCP_CDFT_LONG_MIN=129: 130 (32 x 16), 1000 (64 x 32), 1536 and 1537 (64 x 64: n a multiple of m2 -- column
  0 is its own mirror -- and n = 1 mod m2), 2049 (128 x 64)
dense (dct_dense.hip)
  (47, 31, 1) axis 0, (31, 47, 1) axis 1        k_dct_dense<false> / <true>, TL = 1 line per workgroup
  (47, 515, 1), (515, 47, 1)                    TL = 8, the last tile holds three lines
  (n, 63, 1), (63, n, 1), n = 48, 96, 1026      63 < 64 lines: k_dct_dense, TL = 1
  (n, 130, 1), (130, n, 1), n = 48, 96, 99, 1026; (5, 26, 96) axis 2     k_dct_mfma_split<axis 0?, 8, inverse?>: two line
                                                tiles of 128 (the second holds two lines), ragged k tiles of 64 per parity,
                                                odd n: the middle element goes with the even part
  with DOTSOCP_PFA=0 DOTSOCP_CDFT=0: 1025 and 257 through the same two kernels, under the 1-ulp bound

Measured on an MI355X (E_device against the larger CPU figure): powers of two 0.6 .. 5.4 against 0.8 .. 4.6, prime-factor
0.2 .. 2.1 against 0.8 .. 7.3, Rader 3.6 against 5.7, Bluestein 2.1 .. 8.4 against 3.7 .. 12.7; worst E_device / bound 0.53
except on the forward (B) of the in-LDS powers of two, which have no model: scipy's figure there is the luck of one
rounding at the bin of size one (0.26 at n = 2048) and the device's one-ulp error at that bin is 0.96 of four times it.
Dense product: every entry within 0.49 ulp on (A) / (A'), (B) at most 0.30 of the bound."""
import os
import subprocess
import sys
import tempfile

import pytest

import dct_probes as P
import dotsocp_amd as D

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _judge(rows):
    print()
    for r in rows:
        print(P.format_row(r))
    bad = [P.format_row(r) for r in rows if not P.passes(r)]
    assert not bad, "\n" + "\n".join(bad)


def _run(case):
    family, shape, axis, _ = P.case_shape(case)
    assert P.family_on_device(D, shape[axis], axis) == family
    _judge(P.measure(case, D.dct_axis))


@pytest.mark.parametrize("case", P.cases_of("fft1"), ids=P.case_id)
def test_power_of_two_inside_the_lds(case):
    _run(case)


@pytest.mark.parametrize("case", P.cases_of("fft1-pipe"), ids=P.case_id)
def test_power_of_two_pipelined(case):
    """asserts the instance: the library's own launch decision for this pass on this device (dotsocp_dct_pass_kernel)"""
    family, shape, axis, _ = P.case_shape(case)
    kernel = P.kernel_on_device(D, shape, axis)
    assert kernel == "pow2-pipe", "%s: this device runs the %s kernel along axis %d, not the pipelined one" % (
        P.case_id(case), kernel, axis)
    _run(case)


@pytest.mark.parametrize("case", P.cases_of("fft2"), ids=P.case_id)
def test_power_of_two_two_level(case):
    _run(case)


@pytest.mark.parametrize("case", P.cases_of("pfa"), ids=P.case_id)
def test_prime_factor(case):
    _run(case)


@pytest.mark.parametrize("case", P.cases_of("rader") + P.cases_of("bluestein1"), ids=P.case_id)
def test_rader_and_bluestein_inside_the_lds(case):
    _run(case)


@pytest.mark.parametrize("case", P.cases_of("bluestein2"), ids=P.case_id)
def test_bluestein_two_level(case):
    _run(case)


@pytest.mark.parametrize("case", P.cases_of("dense"), ids=P.case_id)
def test_dense_product(case):
    _run(case)


@pytest.mark.parametrize("name", sorted(P.SWITCHED))
def test_with_a_switch_of_the_dispatcher(name):
    """the switch is read once per process: the probe module runs the cases in a child and writes the figures"""
    env, family, cases = P.SWITCHED[name]
    e = {k: v for k, v in os.environ.items() if k not in P.SWITCHES}
    e.update(env)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "figures.npz")
        r = subprocess.run([sys.executable, "-m", "dct_probes", path] + [P.spec_of((family,) + c) for c in cases], env=e,
                           cwd=HERE, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        rows, extra = P.load_rows(path)
    assert extra["families"] == [family] * len(cases)
    if name.startswith("dct_pipe_off"):          # the workgroup-wide counterparts of the pipelined instances
        assert extra["kernels"] == ["pow2-wg"] * len(cases)
    assert len(rows) == 6 * len(cases)
    _judge(rows)
