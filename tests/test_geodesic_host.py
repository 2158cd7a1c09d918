"""Host side of the geodesic's profile (dot-socp_amd/geodesic.py, dot-socp_amd/csrc/geodesic_summary.h); no device.

The numpy twin of the kernel against the same float64 terms accumulated in long double -- every one of the eleven layer
means of every layer within the classical bound for summing N terms, 2 N 2^-53 mean|term| (the rule of
tests/test_gpu_report.py for its layer means) --, closed forms on exactly representable
data (grids of 2^k + 1 nodes: every coordinate is a dyadic fraction), the summary's corner cases, one solve with the oracle
(cost and layer masses must carry the bits of report.solution_report; the defects are printed, not judged), and the
summary header itself: built into an ordinary program with g++ under AddressSanitizer + UBSan
(tests/san/geodesic_summary_check.cpp), it must print the bits that geodesic.summarize() returns."""
import os
import struct
import subprocess

import numpy as np
import pytest

from dotsocp_amd import geodesic as G
from dotsocp_amd import report as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "san", "_build")
U = 2.0 ** -53


def _random_output(rng, shape):
    """rho in [0.5, 1.5] with a few negative entries, exact zeros and values at and below the cost floor; E of order one"""
    names = ("rho", "Ex", "Ey") if len(shape) == 3 else ("rho", "Ex")
    out = {k: np.asfortranarray(rng.standard_normal(shape)) for k in names}
    out["rho"] = np.asfortranarray(rng.uniform(0.5, 1.5, shape))
    flat = out["rho"].reshape(-1, order="F")
    flat[rng.choice(flat.size, 6, replace=False)] = [0.0, -0.0, R.RHO_FLOOR, 1e-9, -0.25, -1.0]
    return out


def _with_cells(out):
    cells = out["rho"].shape[:-1] + (out["rho"].shape[-1] - 1,)
    return dict(out, **{k: np.zeros(cells) for k in (("q0", "bx") if "Ey" not in out else ("q0", "bx", "by"))})


@pytest.mark.parametrize("shape", [(19, 13, 6), (301, 9), (3, 3, 2)], ids=["2d_19x13x6", "1d_301x9", "2d_3x3x2"])
def test_twin_against_long_double(shape):
    out = _random_output(np.random.default_rng(len(shape) * 100 + shape[0]), shape)
    sums, rho_max, n_support, N = G.layer_sums(out)
    ref = G.layer_sums(out, np.longdouble)[0]
    assert sums.dtype == np.float64 and ref.dtype == np.longdouble and N == int(np.prod(shape[:-1]))
    for q, (name, term) in enumerate(zip(G.NAMES, G.layer_terms(out))):
        bound = 2 * N * U * np.abs(term.reshape((N, -1), order="F")).mean(axis=0)
        d = np.abs((sums[:, q] / N - ref[:, q] / N).astype(np.float64))           # the layer means, as the report's test compares them
        print(name, "worst difference / bound", np.max(d / np.where(bound > 0, bound, 1.0)))
        assert np.all(d <= bound), name
    rho = out["rho"].reshape((N, -1), order="F")
    assert np.array_equal(rho_max, rho.max(axis=0) + 0.0) and np.array_equal(n_support, (rho > R.RHO_FLOOR).sum(axis=0))
    if len(shape) == 2:                                     # 1-D: every Y / Ey term is an exact zero
        for name in ("my", "myy", "mxy", "py"):
            assert not sums[:, G.NAMES.index(name)].any()
    # the report's numbers, bit for bit
    p, r = G.geodesic_profile(out), R.solution_report(_with_cells(out))
    assert np.float64(p["cost"]).tobytes() == np.float64(r["cost"]).tobytes()
    assert p["mass"].tobytes() == r["layer_mass"].tobytes()


def test_uniform_density_in_closed_form():
    for shape in ((9, 17, 5), (33, 3)):
        out = {k: np.zeros(shape, order="F") for k in (("rho", "Ex", "Ey") if len(shape) == 3 else ("rho", "Ex"))}
        out["rho"] += 1.0
        p = G.geodesic_profile(out)
        one = np.ones(shape[-1])
        assert np.array_equal(p["mass"], one) and np.array_equal(p["sq"], one) and not p["ent"].any() and not p["kin"].any()
        assert np.array_equal(p["cx"], 0.5 * one) and np.array_equal(p["cy"], (0.5 if len(shape) == 3 else 0.0) * one)
        assert np.array_equal(p["rho_max"], one) and np.array_equal(p["n_support"], int(np.prod(shape[:-1])) * one)
        for k in G.SCALARS:
            assert p[k] == 0.0, k
        assert p["nonfinite"] == 0 and p["nt"] == shape[-1] and p["n_nodes"] == int(np.prod(shape))


@pytest.mark.parametrize("dim", [1, 2])
def test_translated_block_in_closed_form(dim):
    """A block of nodes with rho = 2 that moves `step` nodes per time layer (2-D: along the diagonal) with E = rho v: a
    curve of constant speed and constant shape.  Everything but the divisions by N and the logarithm is exact here, so the
    bound is the one for summing N terms, 2 N 2^-53 times the size of the quantity."""
    n, nt, step, width, first = 33, 5, 3, 6, 4
    v = step * (nt - 1) / (n - 1)                          # nodes per layer -> domain lengths per unit time: 3 * 4 / 32
    shape = (n, nt) if dim == 1 else (n, n, nt)
    rho, E = np.zeros(shape, order="F"), np.zeros(shape, order="F")
    for t in range(nt):
        sl = slice(first + step * t, first + step * t + width)
        rho[(sl,) * dim + (t,)] = 2.0
        E[(sl,) * dim + (t,)] = 2.0 * v
    out = dict(rho=rho, Ex=E) if dim == 1 else dict(rho=rho, Ex=E, Ey=E.copy(order="F"))
    p = G.geodesic_profile(out)
    N = n ** dim
    tol = 2 * N * U
    mass = 2.0 * width ** dim / N
    speed2 = dim * v * v
    print(p.summary())
    print(p.table())
    assert np.all(np.abs(p["mass"] - mass) <= tol * mass)
    assert np.all(np.abs(p["kin"] - speed2 * p["mass"]) <= tol * speed2 * mass)
    assert np.all(np.abs(p["ent"] - p["mass"] * np.log(2.0)) <= tol * mass)
    assert abs(p["cost"] - speed2 * mass) <= tol * speed2 * mass
    assert p["com_defect"] <= tol and p["entropy_defect"] <= tol * mass and p["speed_spread"] <= tol
    assert p["momentum_defect"] <= tol * 2.0 * v * mass
    assert p["peak_excess"] == 0.0 and np.array_equal(p["rho_max"], np.full(nt, 2.0)) and np.all(p["n_support"] == width ** dim)
    centre = (first + step * np.arange(nt) + (width - 1) / 2) / (n - 1)
    assert np.all(np.abs(p["cx"] - centre) <= tol) and np.all(np.abs(p["cy"] - (centre if dim == 2 else 0.0)) <= tol)


def _sums(nt, **rows):
    s = np.zeros((nt, len(G.NAMES)), order="F")
    s[:, 0] = 1.0
    for k, v in rows.items():
        s[:, G.NAMES.index(k)] = v
    return s


def test_summarize_corner_cases():
    N = 4                                                   # a power of two: the means are exact
    # two layers: no inner node, the centre's line is the centre itself
    p = G.summarize(_sums(2, mass=N, mx=[N * .25, N * .75], px=[N * .5, N * .5], ent=[1.0, 5.0]), [1.0, 2.0], [N, N], N)
    assert p["com_defect"] == 0.0 and p["entropy_defect"] == 0.0 and p["momentum_defect"] == 0.0 and p["peak_excess"] == 0.0
    # a planted concave entropy comes back as planted: -((0 + 0) - 2 * 0.375)
    p = G.summarize(_sums(4, mass=N, ent=[0.0, N * .375, 0.0, 0.0]), np.ones(4), [N] * 4, N)
    assert p["entropy_defect"] == 0.75
    # a centre on multiples of 1/8: every operation of the defect is exact
    nt = 5
    p = G.summarize(_sums(nt, mass=N, mx=N * np.arange(nt) / 8.0, my=N * (1 - np.arange(nt) / 8.0)), np.ones(nt), [N] * nt, N)
    assert p["com_defect"] == 0.0 and np.array_equal(p["cx"], np.arange(nt) / 8.0)
    # a peak between the ends
    p = G.summarize(_sums(3, mass=N), [1.0, 1.75, 1.5], [N] * 3, N)
    assert p["peak_excess"] == 0.25
    # constant speed: spread 0; cost = the mean of the layers' energies
    p = G.summarize(_sums(3, mass=N, kin=[N * 2.0, N * 2.0, N * 2.0]), np.ones(3), [N] * 3, N)
    assert p["cost"] == 2.0 and p["energy_min"] == p["energy_max"] == 2.0 and p["speed_spread"] == 0.0


def test_summarize_propagates_nans():
    N, nt = 4, 4
    nan = float("nan")
    p = G.summarize(_sums(nt, mass=N, kin=[1.0, nan, 2.0, 3.0]), np.ones(nt), [N] * nt, N)
    assert np.isnan(p["cost"]) and np.isnan(p["energy_min"]) and np.isnan(p["energy_max"])
    assert p["speed_spread"] == 0.0 and p["nonfinite"] == 0              # (`cost > 0` is false for a NaN cost)
    for first in (True, False):                            # a NaN is kept wherever it stands, the first layer included
        kin = [nan, 1.0, 2.0, 3.0] if first else [1.0, 2.0, 3.0, nan]
        p = G.summarize(_sums(nt, mass=N, kin=kin), np.ones(nt), [N] * nt, N)
        assert np.isnan(p["energy_min"]) and np.isnan(p["energy_max"])
    p = G.summarize(_sums(nt, mass=[N, nan, N, N], mx=N * .5, ent=[0.0, 0.0, nan, 0.0]), [1.0, nan, 1.0, 1.0], [N] * nt, N)
    assert p["nonfinite"] == 1 and np.isnan(p["com_defect"]) and np.isnan(p["entropy_defect"]) and np.isnan(p["peak_excess"])
    assert p["momentum_defect"] == 0.0
    p = G.summarize(_sums(nt, mass=[N, np.inf, N, N]), [1.0, -np.inf, 1.0, 1.0], [N] * nt, N)
    assert p["nonfinite"] == 1 and p["peak_excess"] == 0.0               # a layer without a finite density raises no peak


def _oracle_output():
    from oracle import driver as OD
    from oracle.examples import get_example_2d
    rho0, rho1 = get_example_2d("example1", 9, 9)
    var, model, _, _ = OD.solve_single_level(rho0, rho1, 9, dict(tol=1e-4))
    rho, Ex, Ey = OD.recover_RhoE(var, model)
    return {k: np.asfortranarray(v) for k, v in dict(rho=rho, Ex=Ex, Ey=Ey).items()}


def test_oracle_solve_carries_the_reports_bits():
    out = _oracle_output()
    p, r = G.geodesic_profile(out), R.solution_report(_with_cells(out))
    print(p.summary())
    print(p.table())
    assert np.float64(p["cost"]).tobytes() == np.float64(r["cost"]).tobytes()
    assert p["mass"].tobytes() == r["layer_mass"].tobytes()
    assert p["nonfinite"] == 0 and p["nt"] == 9 and p["n_nodes"] == 9 * 9 * 9


def _case_bytes(sums, rho_max, N):
    sums = np.asfortranarray(sums, dtype=np.float64)
    return struct.pack("qq", sums.shape[0], N) + sums.tobytes(order="F") + np.asarray(rho_max, dtype=np.float64).tobytes()


def _hex(v):
    return "%016x" % struct.unpack("Q", struct.pack("d", float(v)))[0]


def test_summary_header_under_sanitizers_equals_summarize():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "geodesic_summary_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "dot-socp_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "san", "geodesic_summary_check.cpp"), "-o", exe])
    rng = np.random.default_rng(11)
    cases = []
    for shape in ((19, 13, 6), (301, 9), (3, 3, 2), (17, 9, 3)):
        s, m, c, N = G.layer_sums(_random_output(rng, shape))
        cases.append((s, m, c, N))
    s, m, c, N = cases[0]
    bad = s.copy(order="F")
    bad[2, G.NAMES.index("mass")], bad[4, G.NAMES.index("kin")], bad[1, G.NAMES.index("ent")] = np.nan, np.inf, np.nan
    cases.append((bad, np.where(np.arange(m.size) == 3, -np.inf, m), c, N))
    cases.append((rng.uniform(0.5, 1.5, (40, len(G.NAMES))) * 97, rng.uniform(1, 2, 40), np.zeros(40), 97))     # all positive: cost > 0
    path = os.path.join(OUT, "geodesic_summary_cases.bin")
    with open(path, "wb") as f:
        for s, m, _, N in cases:
            f.write(_case_bytes(s, m, N))
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "%d cases" % len(cases)
    for k, ((s, m, c, N), line) in enumerate(zip(cases, lines)):
        p = G.summarize(s, m, c, N)
        want = ["%d" % p["nt"], "%d" % p["n_nodes"]] + [_hex(p[name]) for name in G.SCALARS] + ["%d" % p["nonfinite"]]
        if k & 1:
            want.append(_hex(p["sq"][-1]))
        print(k, line)
        assert line.split() == want, (k, dict(zip(G.SCALARS, line.split()[2:])), p.summary())
    assert any(G.summarize(*c)["speed_spread"] > 0 for c in cases)
