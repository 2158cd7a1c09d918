"""The schedule of the cone pass's gamma form (solver.h: "The gamma form"), as pure host arithmetic through the C ABI:
no device.  Between two plain inPALM iterations the cone pass leaves gamma = beta + tau z where it would leave beta, and
only the next cone pass can read that -- so the pass of an iteration that is followed by any other reader of beta or z
(a KKT check at its end, the caller after run() returns, the rescale block of the next iteration) must write beta.
The loop below replays Solver::step()'s decisions for iterations 1..600 with the reference's check cadence
(IfAdjustSigma, solver_socp_inPALM.m:361-379, restated here) and a rescale history as a solve produces it.  What carries
the test is the comparison of the library's predicate with the three reasons restated here, as an "if and only if";
the one reader that looks at what the PREVIOUS iteration left, the rescale block, is checked against the carried state."""
import itertools

import pytest

from dotsocp_amd import capi


def if_adjust_sigma(it, last):
    passed = it - last
    if it < 20 and passed >= 3:
        return True
    if it < 50 and passed >= 6:
        return True
    if it < 100 and passed >= 10:
        return True
    if it < 200 and passed >= 15:
        return True
    if it < 500 and passed >= 25:
        return True
    return passed >= 40


def rescale_due(it, rescale, max_feas, rel_gap):
    """solver_socp_inPALM.m:139-149: the iterations whose rescale block reads the state."""
    if rescale >= 3 and it % 100 == 0:
        return True
    if rescale == 1 and max_feas < 2e-2 and it >= 10 and rel_gap < 5e-2:
        return True
    return rescale == 2 and max_feas < 5e-3 and it >= 50 and rel_gap < 1e-2


def _splits(kind, maxit):
    """lengths of the run(n) calls; the last call runs to the end"""
    if kind == "one":
        return []
    if kind == "7-5":
        return [7, 5]
    if kind == "ones":
        return [1] * 30
    if kind == "mixed":
        return [2, 3, 1, 40, 1, 1, 99, 100, 57]
    raise ValueError(kind)


@pytest.mark.parametrize("step_by_step", [False, True])
@pytest.mark.parametrize("kind", ["one", "7-5", "ones", "mixed"])
@pytest.mark.parametrize("scaling,feas_at", [(False, None), (True, (7, 33)), (True, (3, 58)), (True, (64, 64)), (True, (9, None))])
def test_every_reader_of_beta_finds_beta(step_by_step, kind, scaling, feas_at):
    L = capi.lib()
    maxit = 600
    # the iterations at which a run() call ends
    ends, acc = set(), 0
    for n in _splits(kind, maxit):
        acc += n
        ends.add(acc)
    last_sigma = float("-inf")
    rescale = 1 if scaling else 0
    max_feas = rel_gap = float("inf")
    form = "beta"                       # what the multiplier array holds between two iterations
    n_gamma = n_checks = 0
    for it in range(1, maxit + 1):
        # ---- the rescale block at the start of iteration `it`
        due = rescale_due(it, rescale, max_feas, rel_gap)
        assert L.dotsocp_rescale_due(it, rescale, max_feas, rel_gap) == int(due)
        if due:
            assert form == "beta", ("rescale block", it)
            if rescale in (1, 2) or it % 200 == 0:       # a rescale (every second norm check fires one here)
                rescale += 1
        # ---- the decision step() takes in front of the cone pass
        check = step_by_step or if_adjust_sigma(it, last_sigma) or it == maxit
        last_of_run = it in ends
        next_due = rescale_due(it + 1, rescale, max_feas, rel_gap)
        must = check or last_of_run or next_due
        got = L.dotsocp_cone_writes_beta(it, last_sigma, maxit, int(step_by_step), int(last_of_run), rescale, max_feas, rel_gap)
        # exactly the iterations with a reader behind them write beta: none of them may write gamma, and the others do
        assert got == int(must), (it, check, last_of_run, next_due)
        deferred = it >= 2               # the first pass has no multiplier step to carry
        writes_gamma = deferred and not got
        # the pass of this iteration was the one reader of what the last one left; this is what the next iteration finds
        form = "gamma" if writes_gamma else "beta"
        n_gamma += writes_gamma
        # ---- the end of the iteration (its check and the caller after run() read what this pass wrote: `must` above)
        if check:
            n_checks += 1
            if if_adjust_sigma(it, last_sigma):
                last_sigma = it
            if rescale > 0 and feas_at is not None:
                # the feasibility and gap thresholds of the two rescales are met from these iterations on
                if rescale == 1 and it >= feas_at[0]:
                    max_feas, rel_gap = 1e-2, 1e-2
                if rescale == 2 and feas_at[1] is not None and it >= feas_at[1]:
                    max_feas, rel_gap = 1e-3, 1e-3
    if not step_by_step:
        assert n_checks < 60 and n_gamma > 450       # the cadence leaves most passes in the steady flavour
    else:
        assert n_gamma == 0


def test_rescale_predicate_matches_the_reference_conditions():
    L = capi.lib()
    for it, rescale, (mf, rg) in itertools.product((1, 9, 10, 49, 50, 99, 100, 101, 200, 300, 555),
                                                   (0, 1, 2, 3, 4, 7),
                                                   ((float("inf"), float("inf")), (1.9e-2, 4.9e-2), (2e-2, 1e-3), (1e-3, 5e-2),
                                                    (4.9e-3, 0.99e-2), (5e-3, 1e-3), (1e-3, 1e-2), (1e-9, 1e-9))):
        assert L.dotsocp_rescale_due(it, rescale, mf, rg) == int(rescale_due(it, rescale, mf, rg)), (it, rescale, mf, rg)
