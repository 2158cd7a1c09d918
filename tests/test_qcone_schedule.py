"""The schedule of the early cone pass (solver.h: "The early cone pass"), as pure host arithmetic through the C ABI: no
device.  The q-step of an iteration whose own cone pass left gamma may run the NEXT iteration's gamma-reading pass in
the same kernel: in the steady form (gamma out, q never stored) or in the exit form (beta and q stored), as the
schedule of the gamma form (tests/test_cone_carry_schedule.py) asks of that next pass.

The loop below replays Solver::step() for iterations 1..400 over the parameter grid of that test -- check cadence, maxit,
step-by-step checks, run() calls in pieces, the rescale and norm-check triggers -- with the fusion taken wherever
dotsocp_qcone_form allows, and follows what is in memory: the form of the multiplier array and whether q was stored."""
import pytest

from dotsocp_amd import capi

NONE, STEADY, EXIT = 0, 1, 2


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
    if rescale >= 3 and it % 100 == 0:
        return True
    if rescale == 1 and max_feas < 2e-2 and it >= 10 and rel_gap < 5e-2:
        return True
    return rescale == 2 and max_feas < 5e-3 and it >= 50 and rel_gap < 1e-2


def _splits(kind):
    return {"one": [], "7-5": [7, 5], "ones": [1] * 30, "mixed": [2, 3, 1, 40, 1, 1, 99, 100, 57]}[kind]


@pytest.mark.parametrize("maxit", [400, 37])
@pytest.mark.parametrize("step_by_step", [False, True])
@pytest.mark.parametrize("kind", ["one", "7-5", "ones", "mixed"])
@pytest.mark.parametrize("scaling,feas_at", [(False, None), (True, (7, 33)), (True, (3, 58)), (True, (64, 64)), (True, (9, None))])
def test_every_reader_of_q_and_beta_finds_them(maxit, step_by_step, kind, scaling, feas_at):
    L = capi.lib()
    ends, acc = set(), 0
    for n in _splits(kind):
        acc += n
        ends.add(acc)
    last_sigma = float("-inf")
    rescale = 1 if scaling else 0
    max_feas = rel_gap = float("inf")
    form = "beta"            # what the multiplier array holds between two iterations
    q_stored = True          # the last q-step stored q
    early = NONE             # the form in which the last q-step ran this iteration's cone pass
    n_steady = n_exit = 0
    for it in range(1, min(maxit, 400) + 1):
        # ---- the rescale block at the start of iteration `it` reads q and beta
        if rescale_due(it, rescale, max_feas, rel_gap):
            assert form == "beta" and q_stored and early in (NONE, EXIT), ("rescale block", it)
            if rescale in (1, 2) or it % 200 == 0:
                rescale += 1
        check = step_by_step or if_adjust_sigma(it, last_sigma) or it == maxit
        last_of_run, next_last = it in ends, (it + 1) in ends
        args = (last_sigma, maxit, int(step_by_step))
        state = (rescale, max_feas, rel_gap)
        writes_beta = bool(L.dotsocp_cone_writes_beta(it, *args, int(last_of_run), *state))
        deferred = it >= 2
        gamma_out = deferred and not writes_beta
        # ---- the cone pass: run by the last q-step, or launched now (it then reads q from memory)
        if early != NONE:
            assert form == "gamma", it                     # an early pass is a gamma-reading one
            assert (early == STEADY) == gamma_out, (it, early, gamma_out)
        else:
            assert q_stored, ("cone pass", it)
        form = "gamma" if gamma_out else "beta"
        # ---- the q-step
        fuse = L.dotsocp_qcone_form(it, *args, int(last_of_run), int(next_last), *state)
        if writes_beta:
            assert fuse == NONE, it                        # never in an iteration whose pass writes beta
        else:
            nxt_writes_beta = bool(L.dotsocp_cone_writes_beta(it + 1, *args, int(next_last), *state))
            assert fuse == (EXIT if nxt_writes_beta else STEADY), (it, fuse)
        if not deferred or form != "gamma":
            fuse = NONE                                    # the solver's own conditions (Solver::qcone_decide)
        early = fuse
        q_stored = fuse != STEADY
        n_steady += fuse == STEADY
        n_exit += fuse == EXIT
        # ---- readers behind this iteration: its KKT check, the caller after run(), the next rescale block
        reader = check or last_of_run or rescale_due(it + 1, rescale, max_feas, rel_gap)
        if reader:
            assert form == "beta" and q_stored and early == NONE, ("reader behind", it)
        if check:
            if if_adjust_sigma(it, last_sigma):
                last_sigma = it
            if rescale > 0 and feas_at is not None:
                if rescale == 1 and it >= feas_at[0]:
                    max_feas, rel_gap = 1e-2, 1e-2
                if rescale == 2 and feas_at[1] is not None and it >= feas_at[1]:
                    max_feas, rel_gap = 1e-3, 1e-3
    assert early == NONE                                   # nothing is pending at the end
    if step_by_step:
        assert n_steady == n_exit == 0
    elif maxit == 400 and kind == "one":
        assert n_steady > 200 and n_exit >= 10             # most iterations of a plain run take the steady form
