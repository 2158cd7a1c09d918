"""The accelerated ADMM loop (csrc/acc.hip, csrc/solver_acc.hip) on GENERIC data against the oracle.

The acc-ADMM oracle is PARITY UNPINNED (oracle/accadmm.py): the device-against-oracle comparison is the only thing that
holds this loop, and tests/test_gpu_accadmm.py makes it on `example1` from the all-zero start, where no row takes the
polar branch of the projection and KKT column 5 is 2e-16.  Here every run starts from the generic state of
oracle/generic_state.py and follows its usual schedule; tests/test_generic_state_conditions.py asserts on the CPU, with
the oracle alone, that every cone pass sees all three branches and that the cases take the paths named below.  The
helpers and the bounds are those of tests/test_gpu_generic_state.py, part (a): same `iter` history, sigma / cScale /
dScale to 1e-12, the generic KKT columns to rtol 1e-8 with NO absolute floor, pdGap to 1e-8, the five fields to 1e-11
of their max-abs.  Column 5 cancels exactly (oracle/generic_state.py: CANCELLING_COLUMNS) and is held absolutely on both
sides: below 1e-13, and below 3.1e-10 under 1e6 weights (tests/test_generic_state_conditions.py: NOISE_WEIGHTED).

(a) one slab, default switches, every one-slab case: Halpern on the tile-crossing grids (130 x 9 x 7: 1-column remainder,
    rows pitched to 144; 100 x 70 x 20: many tiles both ways), restart by count between checks (restart = 2: the
    anchors re-set by acc_set_anchors while the gather stays valid), theta = 3 and 5 (k_acc_interp modes 1 and 2, with
    and without write_aux), a check in every iteration, 1e6 weights (the WEIGHTED flavours of k_acc_cone<RAW, ., KKT>
    and of the q-step).  In every Halpern case a check that changed sigma is followed by k_acc_cone mode 3 and
    k_acc_restart, and -- except under weights, where every check changes sigma -- one that left it alone by mode 1.
    The launch counts are those Solver::acc_step gives for the `iter` history of the run.
(b) the switches DOTSOCP_ACC_POST and DOTSOCP_NT to the bit, DOTSOCP_KKT_FOLD at the bounds of
    tests/test_gpu_accadmm.py::test_folded_kkt_equals_unfolded without its absolute floor; the runs with a path
    switched off are held against the oracle too.
(c) time slabs (ship_tails, the raw q^+ halo, the u0 tail with launch_rhs_fixup, the phi^+ head in front of the unfolded
    KKT block): 40 x 12 x 13 in two and three slabs, on a stream pair per slab, under both t solves; DOTSOCP_ACC_POST
    to the bit on three slabs.
PALM from the generic start, on one slab and on time slabs, is in tests/test_gpu_generic_palm.py.

Measured errors are recorded in DESIGN.md (section 5, "acc-ADMM from a generic start")."""
import numpy as np
import pytest

from oracle import generic_state as G
from test_generic_state_conditions import noise_bound
from test_gpu_generic_state import FIELDS, _against_the_oracle, _gpu_run, _identical, _relerr

pytestmark = pytest.mark.gpu

ONE_SLAB_CASES = [c for c, spec in G.CASES.items() if spec["method"] == "acc-ADMM" and c != "acc-ADMM-checkstep-40x12x13"]
SLAB_CASES = ["acc-ADMM-40x12x13", "acc-ADMM-theta3-40x12x13", "acc-ADMM-weighted-40x12x13", "acc-ADMM-checkstep-40x12x13"]
_cache = {}


def _run(monkeypatch, case, env=None, **split):
    """_gpu_run with profiling on one slab, once per (case, switches, split) and process (read-only)."""
    key = (case, tuple(sorted((env or {}).items())), tuple(sorted(split.items())))
    if key not in _cache:
        _cache[key] = _gpu_run(monkeypatch, case, env, profiling=not split, **split)
    return _cache[key]


def _expected_counts(case, fold=True, post=True):
    """The launches of one slab that Solver::acc_step makes for the `iter` history of the oracle run: the cone pass of an
    iteration with a KKT check is the folded flavour (cone_fused_a) unless DOTSOCP_KKT_FOLD=0, every other one is
    acc_cone (the pass AFTER a check runs inside the extrapolation phase and is not counted).  The gather is a launch of
    its own in iteration 1, and later wherever the pass before did not emit it: never for Halpern (the folded pass and
    the pass after a check both do), after every check with DOTSOCP_ACC_POST=0, in every iteration for theta != 2."""
    spec = G.CASES[case]
    K = spec["K"]
    checks = [int(i) for i in G.oracle_run(case)["hist"]["iter"]]
    halpern = float(spec.get("opts", {}).get("theta", 2.0)) == 2.0
    if not halpern:
        gathers = K
    elif post:
        gathers = 1
    else:
        gathers = 1 + sum(1 for c in checks if c < K)
    return dict(cone_fused_a=len(checks) if fold else 0, acc_cone=K - len(checks) if fold else K, acc_gather=gathers)


def _assert_counts(case, counts, **kw):
    want = _expected_counts(case, **kw)
    got = {k: counts[k] for k in want}
    print("\n%s: launches %s" % (case, got))
    assert got == want


# --------------------------------------------------------------------------------------------------
# (a) one slab, default switches
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ONE_SLAB_CASES)
def test_accadmm_from_the_generic_start(case, monkeypatch):
    got = _run(monkeypatch, case)
    _against_the_oracle(case, "default", got)
    counts = got[3]
    _assert_counts(case, counts)
    spec = G.CASES[case]
    halpern = float(spec.get("opts", {}).get("theta", 2.0)) == 2.0
    assert counts["cone_fused_a"] >= 1                         # the folded KKT cone pass
    if not spec.get("opts", {}).get("ifCheckStepByStep"):      # (with a check in every iteration every pass is the folded one)
        assert counts["acc_cone"] >= 1
    if halpern:
        assert counts["acc_gather"] == 1                       # the pass after a check emits the next gather
    else:
        assert counts["acc_gather"] > 1
    assert counts["cone_fused_b"] == counts["cone_carry"] == counts["qcone"] == 0


# --------------------------------------------------------------------------------------------------
# (b) the switches on generic data
# --------------------------------------------------------------------------------------------------
SWITCH_CASES = ["acc-ADMM-130x9x7", "acc-ADMM-restart2-66x10x6", "acc-ADMM-checkstep-66x10x6", "acc-ADMM-weighted-66x10x6"]


@pytest.mark.parametrize("case", SWITCH_CASES)
def test_the_pass_after_a_check_changes_no_bit_on_generic_data(case, monkeypatch):
    """tests/test_gpu_accadmm.py::test_post_kkt_cone_pass_changes_nothing on data where every branch of the projection is
    taken: k_acc_cone modes 1 / 3 and k_acc_restart against two scalings, the anchor copies, the extrapolation passes and
    a gather pass of its own (DOTSOCP_ACC_POST=0)."""
    off = _run(monkeypatch, case, {"DOTSOCP_ACC_POST": "0"})
    on = _run(monkeypatch, case, {"DOTSOCP_ACC_POST": "1"})
    _identical(on, off)
    _assert_counts(case, on[3])
    _assert_counts(case, off[3], post=False)
    assert off[3]["acc_gather"] > 1
    _against_the_oracle(case, "acc_post=0", off)


@pytest.mark.parametrize("case", SWITCH_CASES)
def test_nontemporal_stores_change_no_bit_on_generic_data(case, monkeypatch):
    _identical(_run(monkeypatch, case, {"DOTSOCP_NT": "1"}), _run(monkeypatch, case, {"DOTSOCP_NT": "0"}))


@pytest.mark.parametrize("case", SWITCH_CASES + ["acc-ADMM-theta3-66x10x6"])
def test_folded_kkt_equals_unfolded_on_generic_data(case, monkeypatch):
    """The bounds of tests/test_gpu_accadmm.py::test_folded_kkt_equals_unfolded, with no absolute floor under the generic
    columns; column 5, which cancels, absolutely on both sides."""
    unfolded = _run(monkeypatch, case, {"DOTSOCP_KKT_FOLD": "0"})
    folded = _run(monkeypatch, case, {"DOTSOCP_KKT_FOLD": "1"})
    (ref, h0, s0, c0), (got, h1, s1, c1) = unfolded, folded
    _assert_counts(case, c1)
    _assert_counts(case, c0, fold=False)
    assert c0["cone_fused_a"] == 0
    np.testing.assert_array_equal(h1["iter"], h0["iter"])
    assert abs(s1 - s0) <= 1e-13 * abs(s0)
    generic = [c for c in range(7) if c != 4]
    errs = {f: _relerr(getattr(got, f), getattr(ref, f)) for f in FIELDS}
    print("\n%s: folded against unfolded, KKT history %.1e, column 5 %.2e / %.2e, fields %.1e"
          % (case, np.max(np.abs(h1["kkt"] - h0["kkt"])[:, generic] / h0["kkt"][:, generic]), np.max(h1["kkt"][:, 4]),
             np.max(h0["kkt"][:, 4]), max(errs.values())))
    np.testing.assert_allclose(h1["kkt"][:, generic], h0["kkt"][:, generic], rtol=1e-9, atol=0)
    assert np.all(np.abs(h1["kkt"][:, 4]) <= noise_bound(case)) and np.all(np.abs(h0["kkt"][:, 4]) <= noise_bound(case))
    np.testing.assert_allclose(h1["pdGap"], h0["pdGap"], rtol=1e-9, atol=1e-15)
    assert max(errs.values()) <= (1e-9 if G.CASES[case].get("weighted") else 1e-11), errs
    _against_the_oracle(case, "kkt_fold=0", unfolded)


# --------------------------------------------------------------------------------------------------
# (c) time slabs
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", ["nslabs=2", "nslabs=3"])
@pytest.mark.parametrize("case", SLAB_CASES)
def test_time_slabs_from_the_generic_start(case, split, monkeypatch):
    kind, n = split.split("=")
    _against_the_oracle(case, split, _run(monkeypatch, case, **{kind: int(n)}))


def test_a_stream_pair_per_slab_from_the_generic_start(monkeypatch):
    _against_the_oracle("acc-ADMM-40x12x13", "ngpu=2", _run(monkeypatch, "acc-ADMM-40x12x13", ngpu=2))


@pytest.mark.parametrize("nslabs", [2, 3])
@pytest.mark.parametrize("tsolve", ["dct", "tridiag"])
def test_time_slabs_under_both_t_solves(tsolve, nslabs, monkeypatch):
    case = "acc-ADMM-40x12x13"
    _against_the_oracle(case, "tsolve=%s, nslabs=%d" % (tsolve, nslabs),
                        _run(monkeypatch, case, {"DOTSOCP_TSOLVE": tsolve}, nslabs=nslabs))


@pytest.mark.parametrize("case", ["acc-ADMM-40x12x13", "acc-ADMM-weighted-40x12x13", "acc-ADMM-checkstep-40x12x13"])
def test_the_pass_after_a_check_changes_no_bit_on_three_slabs(case, monkeypatch):
    off = _run(monkeypatch, case, {"DOTSOCP_ACC_POST": "0"}, nslabs=3)
    _identical(_run(monkeypatch, case, {"DOTSOCP_ACC_POST": "1"}, nslabs=3), off)
    _against_the_oracle(case, "acc_post=0, nslabs=3", off)
