"""The generic start of oracle/generic_state.py does its job: with the oracle alone (no device), for every case that
tests/test_gpu_generic_state.py runs, the free-running loop started there

  * sends rows into each of the three branches of the cone projection (polar: result 0, inside: the row itself, surface)
    in EVERY z-step projection of iterations 1..min(K, 25) -- at least 0.2 % of the rows per branch (half of the smallest
    share measured when the recipe was chosen).  On an `example1` trajectory from the all-zero start the polar branch
    gets no row at all.  Only the z-step's projection counts, not the one inside the KKT block;
  * keeps every KKT column at every check >= 1e-3 (from the zero start column 5 is 2e-16: any error in it is invisible
    behind an absolute floor).  The one exception is mathematical, not a matter of the start: with a multiplier step of
    length 1 (ALG2, acc-ADMM) column 5 is zero in exact arithmetic (oracle/generic_state.py: CANCELLING_COLUMNS), and is
    asserted here to BE rounding noise;
  * takes every kind of iteration of the device schedule: entry (a plain iteration after a check: its cone pass leaves
    gamma), steady (plain after plain: gamma in, gamma out) and exit (a check after a plain one: gamma in, beta out);
  * is not rounding-sensitive: a second run from the start perturbed by relative 2^-52 N(0,1) moves the fields by
    <= 1e-12 of their max-abs and the KKT history by <= 1e-12 relative -- so the 1e-11 / 1e-8 bounds of the GPU
    comparison are 10x and 1e4x what rounding alone can explain.

A later change of the recipe, of a case or of the oracle that empties one of these fails here, on the CPU."""
import numpy as np
import pytest

from oracle import generic_state as G

MIN_SHARE = 2e-3
KKT_FLOOR = 1e-3
SENSITIVITY = 1e-12
NOISE = 1e-13          # a relative residual whose terms cancel exactly: a few roundings per entry, 450 eps is generous


def _kinds(checks, K):
    checks = set(int(i) for i in checks)
    kinds = set()
    for it in range(2, K + 1):
        prev_plain = (it - 1) not in checks
        if it not in checks:
            kinds.add("steady" if prev_plain else "entry")
        elif prev_plain:
            kinds.add("exit")
    return kinds


@pytest.mark.parametrize("case", list(G.CASES))
def test_the_generic_start_populates_every_branch_and_kkt_column(case):
    spec = G.CASES[case]
    K = spec["K"]
    assert K <= 25          # the polar share decays after about 30 iterations
    run = G.oracle_run(case)
    hist = run["hist"]
    # --- the projection branches
    shares = run["shares"]
    assert shares.shape == (K, 3)
    low = shares[:min(K, 25)].min(axis=0)
    print("\n%s: smallest share per z-step projection  polar %.4f  inside %.4f  surface %.4f" % (case, *low))
    assert low.min() >= MIN_SHARE, dict(polar=shares[:, 0], inside=shares[:, 1], surface=shares[:, 2])
    # --- the KKT columns
    kkt = hist["kkt"]
    assert kkt.shape == (hist["len"], 7) and hist["len"] >= 3
    cancelling = G.CANCELLING_COLUMNS.get(spec["method"], ())
    generic = [c for c in range(7) if c not in cancelling]
    print("%s: smallest KKT entry per column %s" % (case, " ".join("%.2e" % v for v in kkt.min(axis=0))))
    assert kkt[:, generic].min() >= KKT_FLOOR, kkt
    for c in cancelling:
        assert np.all(kkt[:, c] <= NOISE), kkt[:, c]
    # --- the schedule
    assert hist["iter"][-1] == K
    assert _kinds(hist["iter"], K) == {"entry", "steady", "exit"}, list(hist["iter"])
    # --- the weights are the barrier's
    if spec.get("weighted"):
        assert (run["weight"] == 1e6).sum() > 0
    # --- sensitivity to one-ulp perturbations of the start
    twin = G.oracle_run(case, perturb=True)
    np.testing.assert_array_equal(twin["hist"]["iter"], hist["iter"])
    moved = {f: np.max(np.abs(getattr(twin["var"], f) - getattr(run["var"], f))) / np.max(np.abs(getattr(run["var"], f)))
             for f in G.FIELDS}
    kmoved = np.max(np.abs(twin["hist"]["kkt"] - kkt)[:, generic] / kkt[:, generic])
    smoved = abs(twin["sigma"] - run["sigma"]) / run["sigma"]
    print("%s: one-ulp perturbation moves the fields by %s, the KKT history by %.1e, sigma by %.1e"
          % (case, " ".join("%s %.1e" % kv for kv in moved.items()), kmoved, smoved))
    assert any(np.any(twin["start"][f] != run["start"][f]) for f in G.FIELDS)
    assert max(moved.values()) <= SENSITIVITY, moved
    assert kmoved <= SENSITIVITY
    for c in cancelling:
        assert np.all(twin["hist"]["kkt"][:, c] <= NOISE)


def test_the_recipe():
    """Amplitudes, classes and holes as stated: the fields have the stated spread, a third of the rows is shifted each
    way, and z / beta are zero exactly in the slots mexBFd leaves unwritten."""
    run = G.oracle_run("inPALM-66x10x6")
    start = run["start"]
    ny, nx, nt = G.CASES["inPALM-66x10x6"]["shape"]
    assert start["beta"].shape == (ny * nx * (nt - 1), 10)
    for f in ("phi", "q", "alpha"):
        assert abs(np.std(start[f]) / G.AMPLITUDES[f] - 1.0) < 0.1, f
    b0 = start["beta"][:, 0]
    up, down = np.mean(b0 > 0.5 * G.SHIFT), np.mean(b0 < -0.5 * G.SHIFT)
    assert abs(up - 1 / 3) < 0.03 and abs(down - 1 / 3) < 0.03
    hole = G.cone_holes(run["var"], (ny, nx, nt))
    assert not hole[:, 0].any() and not hole[:, 9].any()
    assert np.all(start["z"][hole] == 0.0) and np.all(start["beta"][hole] == 0.0)
    assert np.all(start["z"][~hole] != 0.0) and np.all(start["beta"][~hole] != 0.0)
    # the same seed gives the same start; another seed another
    again = G.generic_state(run["var"], (ny, nx, nt))
    other = G.generic_state(run["var"], (ny, nx, nt), seed=G.DEFAULT_SEED + 1)
    assert all(np.array_equal(again[f], start[f]) for f in G.FIELDS)
    assert not np.array_equal(other["phi"], start["phi"])
