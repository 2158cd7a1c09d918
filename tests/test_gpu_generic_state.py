"""The free-running loops on GENERIC data against the oracle.

The trajectories of `example1` from the all-zero start never enter the polar branch of the cone projection and keep KKT
column 5 at rounding noise; the random-state tests always check step by step on a one-tile grid, so no iteration leaves
gamma behind and k_qcone never launches.  Here every loop starts from the generic state of oracle/generic_state.py --
every term of every sum generic, all three projection branches populated in every cone pass of the run
(tests/test_generic_state_conditions.py asserts that on the CPU) -- and runs its usual schedule: checks at 1, 4, 7, ...,
so iteration 2 writes gamma, 3 is steady, 4 exits into a check, and from 19 on the steady stretch is five long.

(a) against oracle/: same `iter` history, sigma / cScale / dScale to 1e-12, the KKT history to rtol 1e-8 with NO absolute
    floor, pdGap to 1e-8, the five fields to 1e-11 of their max-abs (100x the oracle's own sensitivity to one-ulp
    perturbations of the start, <= 1.1e-13, which is the size of effect another summation order has).  Shapes that cross
    every tile border; 1-D; 1e6 barrier weights; ALG2; PALM; acc-ADMM.  inPALM / ALG2 under the default switches, with
    the early cone pass forced (DOTSOCP_QCONE=1, also in 3-layer chunks) and on the unfused dataflow.
    KKT column 5 of ALG2 and acc-ADMM is zero in exact arithmetic (oracle/generic_state.py: CANCELLING_COLUMNS): there it
    is held below 1e-13 on both sides instead (tests/test_generic_state_conditions.py: noise_bound).
    The accelerated ADMM loop has a file of its own, tests/test_gpu_generic_accadmm.py, which reuses the helpers here:
    _gpu_run clears every switch of the library, DOTSOCP_ACC_POST and DOTSOCP_TSOLVE included, and counts the launches
    of the acc-ADMM phases as well.
    The proximal ALM loop likewise: tests/test_gpu_generic_palm.py (tile-crossing grids, a check in every iteration,
    DOTSOCP_PALM_FAST, DOTSOCP_KKT_FOLD, the bit-exact switches, time slabs); here PALM runs once, on 66 x 10 x 6 under the
    default switches.  _gpu_run clears DOTSOCP_PALM_FAST and counts PALM's first q-step (qstep_first) too.
(b) the switches of the library, on the same data: bit-identical, or (DOTSOCP_KKT_FOLD) at the bounds of
    tests/test_gpu_kkt_fold.py without the absolute floor.
(c) time slabs against the oracle, and DOTSOCP_CONE_CARRY to the bit on them.

Measured errors are recorded in DESIGN.md (section 5, "Free-running loops from a generic start")."""
import numpy as np
import pytest

import dotsocp_amd as D
from oracle import driver as OD
from oracle import generic_state as G
from test_generic_state_conditions import noise_bound          # NOISE, or NOISE_WEIGHTED for acc-ADMM under 1e6 weights

pytestmark = pytest.mark.gpu
FIELDS = G.FIELDS
SWITCHES = ("DOTSOCP_QCONE", "DOTSOCP_QCONE_TC", "DOTSOCP_FUSED", "DOTSOCP_CONE_CARRY", "DOTSOCP_C_ENDS", "DOTSOCP_QTX",
            "DOTSOCP_NT", "DOTSOCP_KKT_FOLD", "DOTSOCP_ACC_POST", "DOTSOCP_TSOLVE", "DOTSOCP_PALM_FAST")
SETTINGS = {"default": {}, "qcone": {"DOTSOCP_QCONE": "1"}, "qcone-tc3": {"DOTSOCP_QCONE": "1", "DOTSOCP_QCONE_TC": "3"},
            "unfused": {"DOTSOCP_FUSED": "0"}}
PHASES = ("cone_fused_a", "cone_fused_b", "cone_carry", "qcone", "qstep", "acc_cone", "acc_gather", "qstep_first")


def _gpu_run(monkeypatch, case, env=None, profiling=False, **split):
    """The device loop of a case from the start the oracle run of that case used, under exactly the switches in env."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    spec = G.CASES[case]
    rho0, rho1, nt, weight = G.problem(case)
    var, model = D.initialize(rho0, rho1, nt)
    if weight is not None:
        model.weight = np.asarray(weight, dtype=np.float64)
    o = OD.default_opts(G.case_opts(case), spec["method"], weight is not None)
    D.InitialScaling(var, model, o["scaling"], None, dim=len(spec["shape"]) - 1, weighted=weight is not None)
    G.set_state(var, G.oracle_run(case)["start"])
    ctx = D.InPALMContext(var, o, model, weighted=weight is not None, method=spec["method"], profiling=profiling, **split)
    try:
        ctx.run(-1)
        hist, sigma = ctx.finish()
        counts = {k: ctx.kernel_time(k)[1] for k in PHASES} if profiling else None
    finally:
        ctx.close()
    return var, hist, sigma, counts


def _relerr(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b))


def _against_the_oracle(case, tag, got):
    gvar, g_hist, g_sigma, _ = got
    run = G.oracle_run(case)
    ovar, o_hist, o_sigma = run["var"], run["hist"], run["sigma"]
    errs = {f: _relerr(getattr(gvar, f), getattr(ovar, f)) for f in FIELDS}
    cancelling = G.CANCELLING_COLUMNS.get(G.CASES[case]["method"], ())
    generic = [c for c in range(7) if c not in cancelling]
    same_len = g_hist["len"] == o_hist["len"]
    kerr = np.max(np.abs(g_hist["kkt"] - o_hist["kkt"])[:, generic] / o_hist["kkt"][:, generic]) if same_len else np.nan
    print("\n%s [%s]: errors against the oracle  %s  kkt %.1e  (largest field error %.1e)"
          % (case, tag, "  ".join("%s %.1e" % kv for kv in errs.items()), kerr, max(errs.values())))
    assert same_len
    np.testing.assert_array_equal(g_hist["iter"], o_hist["iter"])
    assert abs(g_sigma - o_sigma) <= 1e-12 * abs(o_sigma)
    assert abs(gvar.cScale - ovar.cScale) <= 1e-12 * ovar.cScale and abs(gvar.dScale - ovar.dScale) <= 1e-12 * ovar.dScale
    np.testing.assert_allclose(g_hist["kkt"][:, generic], o_hist["kkt"][:, generic], rtol=1e-8, atol=0)
    for c in cancelling:
        print("%s [%s]: cancelling column %d  device %.2e  oracle %.2e  (bound %.1e)"
              % (case, tag, c + 1, np.max(np.abs(g_hist["kkt"][:, c])), np.max(o_hist["kkt"][:, c]), noise_bound(case)))
        assert np.all(np.abs(g_hist["kkt"][:, c]) <= noise_bound(case)) and np.all(o_hist["kkt"][:, c] <= noise_bound(case))
    np.testing.assert_allclose(g_hist["pdGap"], o_hist["pdGap"], rtol=1e-8, atol=0)
    assert max(errs.values()) <= 1e-11, errs
    # the run did move the state, and away from the structure of the start
    assert _relerr(gvar.q, run["start"]["q"]) > 1e-2 and _relerr(gvar.beta, run["start"]["beta"]) > 1e-2


def _identical(a, b):
    (va, ha, sa, _), (vb, hb, sb, _) = a, b
    assert sa == sb
    assert ha["len"] == hb["len"] >= 3
    np.testing.assert_array_equal(ha["iter"], hb["iter"])
    np.testing.assert_array_equal(ha["kkt"], hb["kkt"])
    np.testing.assert_array_equal(ha["pdGap"], hb["pdGap"])
    assert va.cScale == vb.cScale and va.dScale == vb.dScale
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(va, f), getattr(vb, f), err_msg=f)


# --------------------------------------------------------------------------------------------------
# (a) the free-running loop against the oracle
# --------------------------------------------------------------------------------------------------
INPALM_CASES = ["inPALM-130x9x7", "inPALM-66x10x6", "inPALM-100x70x20", "inPALM-1d-150x7", "inPALM-weighted-66x10x6",
                "ALG2-66x10x6"]


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("case", INPALM_CASES)
def test_inpalm_from_the_generic_start(case, setting, monkeypatch):
    """130 x 9 x 7: three tiles in y with a 2-row remainder, three 4-wide x tiles with a 1-column remainder, rows pitched
    to 144.  66 x 10 x 6: two y tiles with a 2-row remainder, three x tiles with a 2-column remainder.  100 x 70 x 20: the
    five-iteration steady stretch (K = 25).  The launch counts show that the paths under test ran: under the default
    switches the gamma-reading passes are launches of their own (cone_carry >= 1, qcone == 0: no grid here is large
    enough to fuse); with the early pass forced every gamma-reading pass of these schedules runs inside a q-step
    (qcone >= 1, cone_carry == 0).  Weighted problems keep the two kernels whatever the switch
    (tests/test_gpu_qcone.py), the unfused dataflow has neither phase."""
    got = _gpu_run(monkeypatch, case, SETTINGS[setting], profiling=True)
    counts = got[3]
    print("\n%s [%s]: launches %s" % (case, setting, counts))
    _against_the_oracle(case, setting, got)
    if setting == "unfused":
        assert counts["cone_carry"] == counts["qcone"] == 0
    elif setting == "default" or G.CASES[case].get("weighted"):
        assert counts["cone_carry"] >= 1 and counts["qcone"] == 0
    else:
        assert counts["qcone"] >= 1 and counts["cone_carry"] == 0


@pytest.mark.parametrize("case", ["PALM-66x10x6", "acc-ADMM-66x10x6"])
def test_palm_and_accadmm_from_the_generic_start(case, monkeypatch):
    _against_the_oracle(case, "default", _gpu_run(monkeypatch, case))


# --------------------------------------------------------------------------------------------------
# (b) the switches on generic data
# --------------------------------------------------------------------------------------------------
SWITCH_CASES = ["inPALM-130x9x7", "inPALM-100x70x20"]
VARIANTS = {"qcone=0": {"DOTSOCP_QCONE": "0"}, "qcone=1": {"DOTSOCP_QCONE": "1"}, "qcone=2": {"DOTSOCP_QCONE": "2"},
            "qcone=0,tc=3": {"DOTSOCP_QCONE": "0", "DOTSOCP_QCONE_TC": "3"},
            "qcone=1,tc=3": {"DOTSOCP_QCONE": "1", "DOTSOCP_QCONE_TC": "3"},
            "qcone=2,tc=3": {"DOTSOCP_QCONE": "2", "DOTSOCP_QCONE_TC": "3"},
            "cone_carry=0": {"DOTSOCP_CONE_CARRY": "0"}, "cone_carry=1": {"DOTSOCP_CONE_CARRY": "1"},
            "c_ends=0": {"DOTSOCP_C_ENDS": "0"}, "c_ends=1": {"DOTSOCP_C_ENDS": "1"},
            "qtx=4": {"DOTSOCP_QTX": "4"}, "qtx=8": {"DOTSOCP_QTX": "8"},
            "nt=0": {"DOTSOCP_NT": "0"}, "nt=1": {"DOTSOCP_NT": "1"}}
_plain = {}


def _plain_run(monkeypatch, case):
    """The run with every switch unset, once per case (read-only)."""
    if case not in _plain:
        _plain[case] = _gpu_run(monkeypatch, case)
    return _plain[case]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", SWITCH_CASES)
def test_switches_change_no_bit_on_generic_data(case, variant, monkeypatch):
    """Every value of every switch gives the bits of the run with all switches unset, hence of every other value: the
    claim of tests/test_gpu_qcone.py, test_gpu_cone_carry.py and test_gpu_kkt_fold.py, on data where no term vanishes."""
    ref = _plain_run(monkeypatch, case)
    _identical(_gpu_run(monkeypatch, case, VARIANTS[variant]), ref)


@pytest.mark.parametrize("case", SWITCH_CASES)
def test_folded_kkt_equals_unfolded_on_generic_data(case, monkeypatch):
    """The bounds of tests/test_gpu_kkt_fold.py::_both, with no absolute floor under the KKT history: every column is
    generic here, the border-edge share of column 5 included."""
    ref, h0, s0, _ = _gpu_run(monkeypatch, case, {"DOTSOCP_KKT_FOLD": "0"})
    got, h1, s1, _ = _gpu_run(monkeypatch, case, {"DOTSOCP_KKT_FOLD": "1"})
    np.testing.assert_array_equal(h1["iter"], h0["iter"])
    assert abs(s1 - s0) <= 1e-13 * abs(s0)
    print("\n%s: folded against unfolded, KKT history %.1e" % (case, np.max(np.abs(h1["kkt"] - h0["kkt"]) / h0["kkt"])))
    np.testing.assert_allclose(h1["kkt"], h0["kkt"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(h1["pdGap"], h0["pdGap"], rtol=1e-9, atol=1e-15)
    for f in FIELDS:
        assert _relerr(getattr(got, f), getattr(ref, f)) <= 1e-12, f


# --------------------------------------------------------------------------------------------------
# (c) time slabs
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", ["nslabs=2", "nslabs=3", "ngpu=2"])
def test_time_slabs_from_the_generic_start(split, monkeypatch):
    """40 x 12 x 13 in two and three time slabs (sharing the device's stream pair, or with a pair per slab): against the
    oracle at the bounds of (a), and the gamma form of the cone pass to the bit against the beta form."""
    case = "inPALM-40x12x13"
    kind, n = split.split("=")
    kw = {kind: int(n)}
    carry = _gpu_run(monkeypatch, case, {"DOTSOCP_CONE_CARRY": "1"}, **kw)
    _against_the_oracle(case, split, carry)
    plain = _gpu_run(monkeypatch, case, {"DOTSOCP_CONE_CARRY": "0"}, **kw)
    _identical(carry, plain)
