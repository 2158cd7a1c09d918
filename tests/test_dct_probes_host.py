"""(No device needed.)  What tests/test_gpu_dct_probes.py rests on: the long-double references of tests/dct_probes.py
against scipy at every probe length, the numpy models of the families (tools/*_proto.py) on the same probes, and the
probes themselves -- boundary positions present, odd batches, the exact scaling of (A')."""
import math
import os
import re

import numpy as np
import pytest

import dct_probes as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# E = error / (eps * scale) of the CPU baselines, measured over all probes below (columns: fwd A, A', B, inv A, A', B):
#   scipy    0.3 .. 4.6 for powers of two, 0.4 .. 5.5 up to n = 1026, 6.5 .. 7.7 at 4101, 10 .. 12.7 at 65537, 8 .. 11.3 at
#            524287 (pocketfft takes Bluestein there)
#   models   DctLong 0.9 .. 4.3, Pfa 0.6 .. 7.3, Cdft 0.5 .. 10.7, CdftLong 1.6 .. 10.6, DctDense 0.3 .. 0.7 but 2.5 .. 3.1 on the
#            forward (B) from 96 points on (n roundings of a sum of size one)
SCIPY_MAX = 16.0
MODEL_MAX = {"fft2": 6.0, "pfa": 10.0, "rader": 8.0, "bluestein1": 14.0, "bluestein2": 14.0, "dense": 5.0}


def _lengths():
    """one CPU case per (family, n, positions): the CPU figures do not depend on the axis or on how many lines cycle"""
    seen = {}
    for c in P.all_cases():
        family, shape, axis, npos = P.case_shape(c)
        n = shape[axis]
        seen.setdefault((family, n, npos), min(int(np.prod(shape)) // n, 9))
    return [(f, (n, L, 1), 0) + ((npos,) if npos else ()) for (f, n, npos), L in sorted(seen.items())]


@pytest.mark.parametrize("case", _lengths(), ids=P.case_id)
def test_references_against_scipy_and_the_models(case):
    rows = P.measure(case)
    print()
    for r in rows:
        print(P.format_row(r))
    assert len(rows) == 6 and [r["kind"] for r in rows] == ["A", "A'", "B"] * 2
    for r in rows:
        # scipy and the references are independent computations of the same entries: both are right, or neither bound holds
        assert 0 < r["E_scipy"] <= SCIPY_MAX, P.format_row(r)
        if P.model_for(r["family"], r["n"]) is not None:
            assert 0 < r["E_model"] <= MODEL_MAX[r["family"]], P.format_row(r)
        else:
            assert r["family"] == "fft1" or r["n"] > P.MODEL_MAX_N
        assert r["bound"] >= P.MARGIN * max(r["E_scipy"], r["E_model"])


def test_reference_is_the_dct_matrix():
    """matrix_columns and basis_rows are the two readings of one orthonormal matrix"""
    for n in (3, 8, 17, 47, 64):
        C = P.basis_rows(n, np.arange(n))                       # C[k, j]
        assert np.array_equal(P.matrix_columns(n, np.arange(n)), C.T)
        assert float(np.max(np.abs(C @ C.T - np.eye(n)))) < 5e-18
    assert abs(float(P.PI) - math.pi) < 2e-16 and float(abs(np.sin(P.PI))) < 5e-18


def test_boundary_positions_are_probed():
    pfa = re.findall(r"case (\d+): n1 = (\d+); n2 = (\d+); return true;",
                     open(os.path.join(ROOT, "dot-socp_amd", "csrc", "pfa.hip")).read())
    assert {int(n): (int(a), int(b)) for n, a, b in pfa} == P.PFA_FACTORS
    from cdft_long_proto import conv_length, split as csplit
    from dct_long_proto import split as dsplit
    for case in P.all_cases():
        family, shape, axis, npos = P.case_shape(case)
        n = shape[axis]
        pos = P.positions(family, n, npos)
        assert len(pos) % 2 == 1 and (len(set(pos)) == len(pos) or n < 16) and all(0 <= p < n for p in pos)
        want = set(P.boundaries(family, n)[:npos])
        if family == "fft2":
            n1, n2 = dsplit(n)
            assert (n1, n2) == P.split2(n) and {n2 - 1, n2, n2 + 1, n - n2 - 1, n - n2} <= want
        if family == "bluestein2":
            m1, m2 = csplit(conv_length(n))
            assert (m1, m2) == P.split2(P.conv_length(n)) and {m2 - 1, m2, m2 + 1, n - m2 - 1, n - m2} <= want
        if family == "pfa" and n > 17:
            N1, N2 = P.PFA_FACTORS[n]
            assert {N1, N2, n - N1, n - N2} <= want
        if family in ("bluestein1", "rader"):
            assert n - 1 in want
        if family == "bluestein1":
            s = math.isqrt(2 * n)
            assert s * s < 2 * n <= (s + 1) ** 2 and {s, s + 1} <= want       # j^2 passes 2n between the two
        assert want <= set(pos)
        if npos is None:
            assert set(P.generic_positions(n)) <= set(pos) and len(pos) >= min(n, 20) and (n > 32 or set(pos) == set(range(n)))


def test_batches_are_odd_and_cover_every_probe_line():
    even = 0
    for case in P.all_cases():
        family, shape, axis, npos = P.case_shape(case)
        n = shape[axis]
        L = int(np.prod(shape)) // n
        vec = (axis == 1 and shape[0] % 2 == 0) or (axis == 2 and (shape[0] * shape[1]) % 2 == 0)
        whole = L >= 2048 or L == 130
        assert L % 2 == 1 or vec or whole, (case, P.EVEN)
        even += L % 2 == 0
        for m in (len(P.positions(family, n, npos)), len(P.b_modes(n))):
            assert m % 2 == 1
            bs = P.batches(m, L)
            assert all(len(b) == L for b in bs) and set(np.concatenate(bs).tolist()) == set(range(m))
    assert 0 < even < len(P.all_cases()) / 2


def test_unequal_partners_are_scaled_exactly():
    s = P.line_factors("A'", 9)
    assert s.tolist() == [1, P.SMALL] * 4 + [1] and np.all(P.line_factors("A", 9) == 1) and np.all(P.line_factors("B", 9) == 1)
    assert math.frexp(P.SMALL) == (0.5, -29) and math.frexp(P.TINY) == (0.5, -19)          # powers of two
    for inverse in (0, 1):
        pr = P.probes("pfa", 129, None, inverse)[1]
        assert pr.kind == "A'" and set(np.unique(pr.U).tolist()) == {0.0, 1.0} and np.all(pr.U.sum(axis=1) == 1)
        ref = pr.ref[:3]
        scaled = ref * np.longdouble(P.SMALL)
        assert np.array_equal(scaled / np.longdouble(P.SMALL), ref)                       # no rounding either way
    # the lines travel through the layout unchanged, in the order in which the kernels pair them
    X = np.arange(9 * 4, dtype=np.float64).reshape(9, 4)
    for shape, axis in (((4, 9, 1), 0), ((9, 4, 1), 1), ((3, 3, 4), 2)):
        a = P.lines_to_array(X, shape, axis)
        assert a.shape == shape and a.flags.f_contiguous and np.array_equal(P.array_to_lines(a, axis), X)
    assert np.array_equal(P.lines_to_array(X, (3, 3, 4), 2)[1, 2, :], X[1 + 3 * 2])
    assert np.array_equal(P.lines_to_array(X, (9, 4, 1), 1)[5, :, 0], X[5])


def test_case_specs_round_trip():
    for case in P.all_cases():
        assert P.parse_case(P.spec_of(case)) == tuple(case)
