"""The staging that outputs(), report(), velocity() and the three particle marches share (csrc/solver_io.hip:
stage_left_tail, stage_rho_ends; csrc/solver_particles.hip: velocity_stage with the reset of the velocity rings) does not
depend on what ran before: on one finished context the calls are made interleaved, in both directions, and every result is

  * what the numpy twin makes of outputs() of the same context -- bit for bit, as tests/test_gpu_advect.py,
    tests/test_gpu_push.py (l1 at its rtol=1e-12) and tests/test_gpu_map_report.py compare it; the report as
    tests/test_gpu_report.py compares it (counts, histograms and extrema bit for bit; the layer sums and the cost, which
    the twin adds in another order, within that file's summation bound);
  * byte for byte what the same call returns as the FIRST call on a fresh context (report and l1 included).

Contexts, states and particles are those of tests/test_gpu_map_report.py: 2d_16x12x8 cut into 3 time slabs (a0_prev and the
copies between the velocity rings are in play) and 1d_33x9; BLOCK + 1 particles, nsub=2."""
import numpy as np
import pytest

from dotsocp_amd import advect as A

import test_gpu_advect as TA
import test_gpu_map_report as TM
import test_gpu_push as TP
import test_gpu_report as TR

pytestmark = pytest.mark.gpu
N = TM.BLOCK + 1
NSUB = 2


def _report_bytes(r):
    return b"".join(np.asarray(r[k]).tobytes() for k in sorted(r))


def _array_bytes(d):
    return b"".join(np.asarray(d[k]).tobytes(order="F") for k in sorted(d))


# (name, the call on a context, its bytes, the comparison with the twin on `out`), in the interleaved order
def _calls(case):
    x, y, mass = TM._particles(case, N)
    strip = TM._strip

    def twin_velocity(dev, out, ctx):
        tv = A.velocity(strip(out), A.default_rho_floor(ctx.model.rho0, ctx.model.rho1))
        assert set(dev) == set(tv)
        for k in tv:
            assert dev[k].shape == tv[k].shape and dev[k].tobytes(order="F") == tv[k].tobytes(order="F"), k

    def twin_outputs(dev, out, ctx):
        assert _array_bytes(dev) == _array_bytes(out)

    push = lambda d: dict(mass=mass, nsub=NSUB, direction=d)                                    # noqa: E731
    mapr = dict(mass=mass, nsub=NSUB, direction=+1, per_particle=True)
    adv = dict(nsub=NSUB, direction=-1, trajectories=True)
    return [
        ("report", lambda c: c.report(), _report_bytes, lambda dev, out, ctx: TR._assert_matches(dev, out)),
        ("push_forward -1", lambda c: c.push_forward(x, y, **push(-1)), TP._bytes,
         lambda dev, out, ctx: TP._same(dev, A.push_forward(strip(out), x, y, **push(-1)))),
        ("outputs", lambda c: c.outputs(), _array_bytes, twin_outputs),
        ("map_report +1", lambda c: c.map_report(x, y, **mapr), TM._bytes,
         lambda dev, out, ctx: TM._same(dev, A.map_report(strip(out), x, y, **mapr))),
        ("velocity", lambda c: c.velocity(), _array_bytes, twin_velocity),
        ("advect -1", lambda c: c.advect(x, y, **adv), TA._run_bytes,
         lambda dev, out, ctx: TA._same(dev, A.advect(strip(out), x, y, **adv))),
        ("push_forward +1", lambda c: c.push_forward(x, y, **push(+1)), TP._bytes,
         lambda dev, out, ctx: TP._same(dev, A.push_forward(strip(out), x, y, **push(+1)))),
    ]


@pytest.mark.parametrize("case,split", [("2d_16x12x8", dict(nslabs=3)), ("1d_33x9", {})], ids=["2d_16x12x8_nslabs3", "1d_33x9"])
def test_interleaved_calls_equal_the_twin_and_a_first_call(case, split):
    calls = _calls(case)
    ctx = TM._context(case, **split)
    try:
        mixed = [call(ctx) for _, call, _, _ in calls]
        out = ctx.outputs()                                     # (the third call made these already: twin_outputs compares)
        for (name, _, _, twin), dev in zip(calls, mixed):
            print(case, name, "against the twin")
            twin(dev, out, ctx)
    finally:
        ctx.close()
    for (name, call, raw, _), dev in zip(calls, mixed):
        fresh = TM._context(case, **split)
        try:
            first = call(fresh)
        finally:
            fresh.close()
        assert raw(first) == raw(dev), "%s: %s differs from the same call made first on a fresh context" % (case, name)
