"""The generic start of oracle/generic_state.py does its job: with the oracle alone (no device), for every case that
tests/test_gpu_generic_state.py runs, the free-running loop started there

  * sends rows into each of the three branches of the cone projection (polar: result 0, inside: the row itself, surface)
    in EVERY z-step projection of iterations 1..min(K, 25) -- at least 0.2 % of the rows per branch (half of the smallest
    share measured when the recipe was chosen).  On an `example1` trajectory from the all-zero start the polar branch
    gets no row at all.  Only the z-step's projection counts, not the one inside the KKT block;
  * keeps every KKT column at every check >= 1e-3 (from the zero start column 5 is 2e-16: any error in it is invisible
    behind an absolute floor).  The one exception is mathematical, not a matter of the start: with a multiplier step of
    length 1 (ALG2, acc-ADMM) column 5 is zero in exact arithmetic (oracle/generic_state.py: CANCELLING_COLUMNS), and is
    asserted here to BE rounding noise (below NOISE; with 1e6 weights below NOISE_WEIGHTED, see there);
  * takes every kind of iteration of the device schedule: entry (a plain iteration after a check: its cone pass leaves
    gamma), steady (plain after plain: gamma in, gamma out) and exit (a check after a plain one: gamma in, beta out) --
    or, with ifCheckStepByStep, a check in every iteration;
  * is not rounding-sensitive: a second run from the start perturbed by relative 2^-52 N(0,1) moves the fields by
    <= 1e-12 of their max-abs and the KKT history by <= 1e-12 relative -- so the 1e-11 / 1e-8 bounds of the GPU
    comparison are 10x and 1e4x what rounding alone can explain.

For the acc-ADMM cases the schedule of the extrapolation is asserted as well (test_the_accadmm_cases_...): which checks
change sigma, where the count restarts, which branches of the theta != 2 interpolation run.  For the PALM cases (test_the_palm_cases_take_every_path): a check that changes sigma and one that
leaves it alone, each followed by further iterations, and a case that checks in every iteration.

A later change of the recipe, of a case or of the oracle that empties one of these fails here, on the CPU."""
import numpy as np
import pytest

from oracle import generic_state as G

MIN_SHARE = 2e-3
KKT_FLOOR = 1e-3
SENSITIVITY = 1e-12
NOISE = 1e-13          # a relative residual whose terms cancel exactly: a few roundings per entry, 450 eps is generous
# The same column of acc-ADMM with 1e6 barrier weights: 10x the largest entry of the oracle runs and their perturbed twins
# over all weighted acc-ADMM cases, 3.10e-11 (acc-ADMM-weighted-40x12x13; the others 2.0e-11 .. 2.8e-11) -- the margin
# NOISE has over its own measured 6e-16 .. 1e-15.  Run and twin differ by 2 % .. 14 % of it, not by O(1): at these weights
# the quantity is systematic, not rounding noise.  test_column_5_of_the_weighted_accadmm_cases holds
# the oracle below it; the device is held to the same figure, which is not taken from it.
NOISE_WEIGHTED = 3.1e-10
ACC_CASES = [c for c, spec in G.CASES.items() if spec["method"] == "acc-ADMM"]
WEIGHTED_ACC_CASES = [c for c in ACC_CASES if G.CASES[c].get("weighted")]


def noise_bound(case):
    spec = G.CASES[case]
    return NOISE_WEIGHTED if spec["method"] == "acc-ADMM" and spec.get("weighted") else NOISE


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
        assert np.all(kkt[:, c] <= noise_bound(case)), kkt[:, c]
    # --- the schedule
    assert hist["iter"][-1] == K
    if spec.get("opts", {}).get("ifCheckStepByStep"):
        np.testing.assert_array_equal(hist["iter"], np.arange(1, K + 1))
    else:
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
        assert np.all(twin["hist"]["kkt"][:, c] <= noise_bound(case))


# With 1e6 barrier weights the ratio of the primal to the dual residual is 0.02 .. 0.2 at every check of the first twelve
# iterations, whatever the amplitudes of the start (scanned by factors 1/4 .. 4 per field): every check changes sigma.
# The pass after a check that leaves sigma alone reads no weight (k_acc_cone mode 1 takes none), so the unweighted
# cases cover it.
EVERY_CHECK_CHANGES_SIGMA = WEIGHTED_ACC_CASES


@pytest.mark.parametrize("case", ACC_CASES)
def test_the_accadmm_cases_take_every_path_of_the_extrapolation(case):
    """What the device loop does differently from one iteration to the next (Solver::acc_step) hangs on the check before
    it: a check that changed sigma is followed by the restart pass (k_acc_cone mode 3, k_acc_restart: divide by the
    factor, store the anchors), one that left sigma alone by the plain extrapolating pass (mode 1).  Both kinds must
    occur at a check that is not the last one, or the pass after it never runs.  With restart <= 3 the count also
    returns to 0 between two checks (acc_set_anchors while the gather stays valid), and for theta != 2 the
    interpolation takes its k == 0 and k > 0 branches, with and without the hatOld store."""
    spec = G.CASES[case]
    opts = spec.get("opts", {})
    run = G.oracle_run(case)
    checks = [int(i) for i in run["hist"]["iter"]]
    factors = dict(run["sigma_updates"])
    changed = [i for i in checks[:-1] if i in factors]
    alone = [i for i in checks[:-1] if i not in factors]
    print("\n%s: checks %s  sigma factors %s  left alone at %s  restarts by count at %s"
          % (case, checks, {i: round(f, 3) for i, f in factors.items()}, alone, run["restarts"]))
    assert set(factors) <= set(checks) and all(f != 1.0 for f in factors.values())
    assert len(changed) >= 1
    if case in EVERY_CHECK_CHANGES_SIGMA:
        assert alone == []          # if this ever fails the case has gained the path: take it off the list
    else:
        assert len(alone) >= 1
    # one extrapolation per iteration (tol = 0: no check stops the run), the count back at 0 after a sigma update
    interps = run["interps"]
    assert [i for i, _ in interps] == list(range(1, spec["K"] + 1))
    assert all(k == 0 for i, k in interps if i in factors)
    restart = int(opts.get("restart", 100))
    theta = float(opts.get("theta", 2.0))
    assert set(run["restarts"]) == set(i for i, k in interps if k + 1 >= restart)
    if restart <= 3:
        by_count = run["restarts"] if opts.get("ifCheckStepByStep") else [i for i in run["restarts"] if i not in checks]
        assert len(by_count) >= 2, run["restarts"]
    if theta != 2.0:
        ks = [k for _, k in interps]
        assert 0 in ks and max(ks) > 0
        if restart <= 3:
            stores = set(k + 1 < restart for k in ks)          # solver_socp_accADMM.m:417-421
            assert stores == {True, False}
            # ... and both for k == 0 and for k > 0 where the count allows it (k + 1 < restart needs k <= 1)
            assert any(k > 0 and k + 1 < restart for k in ks) and any(k > 0 and k + 1 >= restart for k in ks)


PALM_CASES = [c for c, spec in G.CASES.items() if spec["method"] == "PALM"]


def test_the_palm_cases_take_every_path():
    """What Solver::palm_step does in the iteration after a check hangs on that check: the multiplier step is executed and
    z regenerated either way, but a check that changed sigma has divided alpha, beta and c by the factor in between, one
    that left it alone has not.  Over the PALM cases together both kinds occur at a check that is not the last one (the
    pass after the last check never runs), and the checkstep case checks in every iteration, so that none of its
    iterations ever takes the one-pass form (k_cone_fused mode 5).  PALM-130x9x7 is the case whose first check leaves
    sigma alone; in the other cases every check changes it."""
    assert len(PALM_CASES) >= 5
    changed, alone = {}, {}
    for case in PALM_CASES:
        spec = G.CASES[case]
        run = G.oracle_run(case)
        checks = [int(i) for i in run["hist"]["iter"]]
        factors = dict(run["sigma_updates"])
        assert set(factors) <= set(checks) and all(f != 1.0 for f in factors.values())
        changed[case] = [i for i in checks[:-1] if i in factors]
        alone[case] = [i for i in checks[:-1] if i not in factors]
        print("\n%s: checks %s  sigma factors %s  left alone at %s"
              % (case, checks, {i: round(f, 3) for i, f in factors.items()}, alone[case]))
        if spec.get("opts", {}).get("ifCheckStepByStep"):
            assert checks == list(range(1, spec["K"] + 1))
            # sigma may change only where the schedule of IfAdjustSigma says so: the other checks all leave it alone
            assert len(alone[case]) >= 2 and len(changed[case]) >= 1
        else:
            assert len(checks) < spec["K"]
    assert any(G.CASES[c].get("opts", {}).get("ifCheckStepByStep") for c in PALM_CASES)
    free = [c for c in PALM_CASES if not G.CASES[c].get("opts", {}).get("ifCheckStepByStep")]
    assert sum(1 for c in free if changed[c]) >= 2
    assert alone["PALM-130x9x7"] == [1] and changed["PALM-130x9x7"] == [4]
    assert any(alone[c] for c in free)


def test_column_5_of_the_weighted_accadmm_cases():
    """KKT column 5 of acc-ADMM under 1e6 weights is not below NOISE: the oracle gives 2.0e-11 .. 3.1e-11, in the run and in
    its perturbed twin alike.  Both stay below NOISE_WEIGHTED, which is 10x the largest of them; the relative difference
    between run and twin is printed -- small throughout, so the quantity is systematic and not noise."""
    assert len(WEIGHTED_ACC_CASES) >= 3
    largest = 0.0
    for case in WEIGHTED_ACC_CASES:
        c5 = G.oracle_run(case)["hist"]["kkt"][:, 4]
        t5 = G.oracle_run(case, perturb=True)["hist"]["kkt"][:, 4]
        print("\n%s: column 5 run %.3e .. %.3e  twin %.3e .. %.3e  run against twin %.1e relative"
              % (case, c5.min(), c5.max(), t5.min(), t5.max(), np.max(np.abs(c5 - t5) / c5)))
        assert np.all(c5 > NOISE) and np.all(t5 > NOISE)
        assert np.all(c5 <= NOISE_WEIGHTED) and np.all(t5 <= NOISE_WEIGHTED)
        largest = max(largest, c5.max(), t5.max())
    print("largest %.3e, NOISE_WEIGHTED / largest = %.2f" % (largest, NOISE_WEIGHTED / largest))
    assert 5.0 <= NOISE_WEIGHTED / largest <= 20.0          # the constant is still 10x what the oracle gives, give or take 2x


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
