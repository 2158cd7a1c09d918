"""The proximal ALM loop (csrc/solver_palm.hip) on GENERIC data against the oracle.

The PALM oracle is PARITY UNPINNED (oracle/palm.py): the device-against-oracle comparison is the only thing that holds
this loop, and tests/test_gpu_palm.py makes it on `example1` from the all-zero start, where no row takes the polar branch
of the projection and KKT column 5 is rounding noise, at rtol 1e-6 over an absolute floor.  Here every run starts from
the generic state of oracle/generic_state.py and follows its usual schedule; tests/test_generic_state_conditions.py asserts
on the CPU, with the oracle alone, that every cone pass sees all three branches, that no KKT entry is small, and that the
PALM cases together take the paths named below.  The helpers and the bounds are those of tests/test_gpu_generic_state.py,
part (a): same `iter` history, sigma / cScale / dScale to 1e-12, every KKT column to rtol 1e-8 with NO absolute floor,
pdGap to 1e-8, the five fields to 1e-11 of their max-abs.  PALM's multiplier step has length tau = 1.9: no column cancels.

What is under test is PALM's own code.  The one-pass dataflow rests on
    F*B*(z^k + beta^k) = F*B*((1 + tau) z^k + beta^{k-1}) - tau F*B*(BF q^k + d):
the cone pass emits the first term as a second gather p2 (k_cone_fused modes 5 / 6), the first q-step of the next iteration
subtracts the second, element-wise (k_qstep_rhs VAR 3 with qk).  Where z^k = 0 (polar rows) or nothing is generic an error
in that algebra can vanish; here it cannot.

(a) one slab, default switches, every one-slab PALM case: 66 x 10 x 6, the tile-crossing 130 x 9 x 7 (three y tiles, rows
    pitched to 144, a 1-column remainder in x; its check at iteration 1 leaves sigma alone, so the iteration behind it
    runs launch_acc_cone(2) and mode 6 on multipliers no scaling has touched) and 100 x 70 x 20 (every check changes
    sigma), and a check in every iteration (no iteration ever runs mode 5).  The launch counts are those Solver::palm_step
    gives for the `iter` history of the run: they show that mode 5 ran, and how often.
(b) DOTSOCP_PALM_FAST=0 (modes 4 + 0, two passes over beta) against =1, and against the oracle.
(c) DOTSOCP_KKT_FOLD=0 (k_qstep_fused and the unfolded KKT block) against =1, and against the oracle.
(d) the switches that must change no bit.  palm_step and its launchers read DOTSOCP_NT (launch_cone_fused,
    launch_acc_cone), DOTSOCP_QTX (launch_qstep_rhs_var reads it for every variant, and must keep the wide tile away from
    VAR 3 and from the KKT flavour) and DOTSOCP_C_ENDS (begin() runs detect_c_ends; no launch of PALM's may take the
    flag).  Left out: DOTSOCP_QCONE, DOTSOCP_QCONE_TC and DOTSOCP_CONE_CARRY are used by the inPALM planner (plan_step)
    and launch_qcone only, which palm_step never reaches; DOTSOCP_ACC_POST is read by acc_begin alone; DOTSOCP_FUSED=0 is
    an error for PALM (palm_begin); DOTSOCP_TSOLVE selects another t solve and changes bits -- it is held against the
    oracle in (e); DOTSOCP_KKT_FOLD and DOTSOCP_PALM_FAST are (b) and (c).
(e) time slabs, 40 x 12 x 13 in two and three slabs: on a stream pair per slab, under both t solves, the two-pass dataflow
    (the middle of three slabs is neither first nor last: ptail_* and send_p* are both live in the one-pass run and absent
    in the other) and the unfolded check.

Measured errors are recorded in DESIGN.md (section 5, "PALM from a generic start")."""
import numpy as np
import pytest

from oracle import generic_state as G
from test_gpu_generic_state import FIELDS, _against_the_oracle, _gpu_run, _identical, _relerr

pytestmark = pytest.mark.gpu

SLAB_CASE = "PALM-40x12x13"
ONE_SLAB_CASES = [c for c, spec in G.CASES.items() if spec["method"] == "PALM" and c != SLAB_CASE]
CHECKSTEP = "PALM-checkstep-66x10x6"
GRID_CASES = ["PALM-130x9x7", "PALM-100x70x20", "PALM-66x10x6"]
_cache = {}


def _run(monkeypatch, case, env=None, **split):
    """_gpu_run with profiling on one slab, once per (case, switches, split) and process (read-only)."""
    key = (case, tuple(sorted((env or {}).items())), tuple(sorted(split.items())))
    if key not in _cache:
        _cache[key] = _gpu_run(monkeypatch, case, env, profiling=not split, **split)
    return _cache[key]


def _expected_counts(case, fast=True):
    """The launches of one slab that Solver::palm_step makes for the `iter` history of the oracle run.  Every iteration
    has one first q-step (qstep_first: with the cone pass in front of it where there is one), one cone pass in front of
    the second q-step and that q-step (qstep).  The cone pass is mode 5 (cone_fused_b) where the one-pass dataflow is on,
    the multiplier step is pending and the pass before left p2 -- from iteration 2 on, unless the iteration before ended
    in a KKT check, which executes the multiplier step -- and mode 6, or 0 without the one-pass dataflow, otherwise
    (cone_fused_a).  The folded or unfolded check changes none of these counts; no other cone or gather phase runs."""
    K = G.CASES[case]["K"]
    checks = set(int(i) for i in G.oracle_run(case)["hist"]["iter"])
    three = sum(1 for it in range(2, K + 1) if (it - 1) not in checks) if fast else 0
    return dict(cone_fused_a=K - three, cone_fused_b=three, qstep_first=K, qstep=K, cone_carry=0, qcone=0, acc_cone=0,
                acc_gather=0)


def _assert_counts(case, counts, **kw):
    want = _expected_counts(case, **kw)
    got = {k: counts[k] for k in want}
    print("\n%s: launches %s" % (case, got))
    assert got == want


def _close(tag, case, a, b, field_tol):
    """Two device runs of one case that differ in the order of summation only: same `iter` history, sigma to 1e-13, the KKT
    history to rtol 1e-9 with no absolute floor, pdGap to rtol 1e-9, the fields to field_tol of their max-abs (b is the
    reference)."""
    (va, ha, sa, _), (vb, hb, sb, _) = a, b
    errs = {f: _relerr(getattr(va, f), getattr(vb, f)) for f in FIELDS}
    same_len = ha["len"] == hb["len"]
    print("\n%s: %s, KKT history %.1e, pdGap %.1e, sigma %.1e, fields %.1e (%s)"
          % (case, tag, np.max(np.abs(ha["kkt"] - hb["kkt"]) / hb["kkt"]) if same_len else np.nan,
             np.max(np.abs(ha["pdGap"] - hb["pdGap"]) / np.abs(hb["pdGap"])) if same_len else np.nan,
             abs(sa - sb) / abs(sb), max(errs.values()), "  ".join("%s %.1e" % kv for kv in errs.items())))
    assert same_len and ha["len"] >= 3
    np.testing.assert_array_equal(ha["iter"], hb["iter"])
    assert abs(sa - sb) <= 1e-13 * abs(sb)
    np.testing.assert_allclose(ha["kkt"], hb["kkt"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(ha["pdGap"], hb["pdGap"], rtol=1e-9, atol=0)
    assert max(errs.values()) <= field_tol, errs


# --------------------------------------------------------------------------------------------------
# (a) one slab, default switches
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ONE_SLAB_CASES)
def test_palm_from_the_generic_start(case, monkeypatch):
    got = _run(monkeypatch, case)
    _against_the_oracle(case, "default", got)
    counts = got[3]
    _assert_counts(case, counts)
    assert counts["qstep_first"] == G.CASES[case]["K"]
    if case == CHECKSTEP:
        assert counts["cone_fused_b"] == 0                      # a check in every iteration: mode 6 throughout
    else:
        # checks at 1, 4, 7: iterations 3, 4, 6, 7 follow a plain one (mode 5), 1, 2, 5 a check or the start (mode 6)
        assert counts["cone_fused_b"] == 4 and counts["cone_fused_a"] == 3


# --------------------------------------------------------------------------------------------------
# (b) the two-pass dataflow
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GRID_CASES)
def test_one_pass_dataflow_equals_two_pass_on_generic_data(case, monkeypatch):
    """tests/test_gpu_palm.py::test_one_pass_dataflow_equals_two_pass (fields to 1e-11) on data where the rows of z^k that
    are zero, those that are the argument itself and those on the surface all occur in every pass; the KKT history at the
    bar of the folded / unfolded tests, with no absolute floor.  The two-pass run is held against the oracle as well: it
    shares the q-steps, the Poisson solve and the KKT block with the one-pass run, but none of the algebra of p2."""
    two = _run(monkeypatch, case, {"DOTSOCP_PALM_FAST": "0"})
    one = _run(monkeypatch, case, {"DOTSOCP_PALM_FAST": "1"})
    _assert_counts(case, one[3])
    _assert_counts(case, two[3], fast=False)
    assert two[3]["cone_fused_b"] == 0 and one[3]["cone_fused_b"] >= 1
    _close("one pass against two", case, one, two, 1e-11)
    _against_the_oracle(case, "palm_fast=0", two)


# --------------------------------------------------------------------------------------------------
# (c) the unfolded KKT check
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GRID_CASES + [CHECKSTEP])
def test_folded_kkt_equals_unfolded_on_generic_data(case, monkeypatch):
    """The bounds of tests/test_gpu_generic_state.py::test_folded_kkt_equals_unfolded_on_generic_data (fields to 1e-12), with
    no absolute floor anywhere.  With DOTSOCP_KKT_FOLD=0 the second q-step of an iteration that ends in a check is
    k_qstep_fused and the block takes all its sums itself; that run is held against the oracle."""
    unfolded = _run(monkeypatch, case, {"DOTSOCP_KKT_FOLD": "0"})
    folded = _run(monkeypatch, case, {"DOTSOCP_KKT_FOLD": "1"})
    _assert_counts(case, folded[3])
    _assert_counts(case, unfolded[3])
    _close("folded against unfolded", case, folded, unfolded, 1e-12)
    _against_the_oracle(case, "kkt_fold=0", unfolded)


# --------------------------------------------------------------------------------------------------
# (d) the switches that change no bit
# --------------------------------------------------------------------------------------------------
VARIANTS = {"nt=0": {"DOTSOCP_NT": "0"}, "nt=1": {"DOTSOCP_NT": "1"}, "qtx=4": {"DOTSOCP_QTX": "4"},
            "qtx=8": {"DOTSOCP_QTX": "8"}, "c_ends=0": {"DOTSOCP_C_ENDS": "0"}, "c_ends=1": {"DOTSOCP_C_ENDS": "1"}}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_switches_change_no_bit_for_palm(variant, monkeypatch):
    """Every value of every switch PALM's launchers read gives the bits of the run with all switches unset (the module
    docstring names the switches left out, and why)."""
    case = "PALM-130x9x7"
    got = _run(monkeypatch, case, VARIANTS[variant])
    _assert_counts(case, got[3])
    _identical(got, _run(monkeypatch, case))


# --------------------------------------------------------------------------------------------------
# (e) time slabs
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nslabs", [2, 3])
def test_palm_on_time_slabs_from_the_generic_start(nslabs, monkeypatch):
    case = "PALM-40x12x13"
    _against_the_oracle(case, "nslabs=%d" % nslabs, _gpu_run(monkeypatch, case, nslabs=nslabs))


def test_a_stream_pair_per_slab_from_the_generic_start(monkeypatch):
    _against_the_oracle(SLAB_CASE, "ngpu=2", _run(monkeypatch, SLAB_CASE, ngpu=2))


@pytest.mark.parametrize("nslabs", [2, 3])
@pytest.mark.parametrize("tsolve", ["dct", "tridiag"])
def test_time_slabs_under_both_t_solves(tsolve, nslabs, monkeypatch):
    _against_the_oracle(SLAB_CASE, "tsolve=%s, nslabs=%d" % (tsolve, nslabs),
                        _run(monkeypatch, SLAB_CASE, {"DOTSOCP_TSOLVE": tsolve}, nslabs=nslabs))


def test_one_pass_dataflow_equals_two_pass_on_three_slabs(monkeypatch):
    """The second pair of tail layers (launch_tail_finalize on p2 / sxp / syp, send_pbx / send_pby -> ptail_bx / ptail_by)
    and q~^k in q3 (its halo, the u0 tail) exist in the one-pass run only; the middle slab sends and receives both."""
    two = _run(monkeypatch, SLAB_CASE, {"DOTSOCP_PALM_FAST": "0"}, nslabs=3)
    one = _run(monkeypatch, SLAB_CASE, {"DOTSOCP_PALM_FAST": "1"}, nslabs=3)
    _close("one pass against two, nslabs=3", SLAB_CASE, one, two, 1e-11)
    _against_the_oracle(SLAB_CASE, "palm_fast=0, nslabs=3", two)
    _against_the_oracle(SLAB_CASE, "palm_fast=1, nslabs=3", one)


def test_folded_kkt_equals_unfolded_on_three_slabs(monkeypatch):
    unfolded = _run(monkeypatch, SLAB_CASE, {"DOTSOCP_KKT_FOLD": "0"}, nslabs=3)
    folded = _run(monkeypatch, SLAB_CASE, {"DOTSOCP_KKT_FOLD": "1"}, nslabs=3)
    _close("folded against unfolded, nslabs=3", SLAB_CASE, folded, unfolded, 1e-12)
    _against_the_oracle(SLAB_CASE, "kkt_fold=0, nslabs=3", unfolded)
