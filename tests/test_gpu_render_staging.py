"""render() shares its staging with outputs(), report(), velocity() and advect() (csrc/solver_io.hip: stage_left_tail,
stage_rho_ends): on one finished context the calls are made interleaved, render() between every two of the others, and each
result is byte for byte what the same call returns as the FIRST call on a fresh context; the pictures and arrows also equal
the numpy twin on outputs() of the interleaved context.

Contexts and particles are those of tests/test_gpu_map_report.py: 2d_16x12x8 cut into 3 time slabs (a0_prev is in play) and
1d_33x9.  (tests/test_gpu_staging_order.py does the same for the older calls among themselves.)"""
import numpy as np
import pytest

from dotsocp_amd import render as R

import test_gpu_advect as TA
import test_gpu_map_report as TM
import test_gpu_render as TG

pytestmark = pytest.mark.gpu


def _report_bytes(r):
    return b"".join(np.asarray(r[k]).tobytes() for k in sorted(r))


def _array_bytes(d):
    """arrays in their own memory order (both sides of a comparison come from the same call), then the scalars"""
    arrays = b"".join(d[k].tobytes(order="A") for k in sorted(d) if isinstance(d[k], np.ndarray))
    return arrays + repr(sorted((k, v) for k, v in d.items() if not isinstance(v, np.ndarray))).encode()


def _calls(case):
    x, y, _ = TM._particles(case, 63)
    nt = TM.CASES[case][2]
    adv = dict(nsub=2, direction=-1, trajectories=True)
    pictures = dict(frames=[nt - 1, 0, 3, 3, 1], mode="levels", lut=TG.LUT, arrows=dict(skip_y=2, skip_x=3))
    gray = dict(num_frame=4, mode="inverted", arrows=dict(skip_y=1, skip_x=1, mask_frac=0.05))
    return [
        ("render levels", lambda c: c.render(**pictures), _array_bytes),
        ("report", lambda c: c.report(), _report_bytes),
        ("render inverted", lambda c: c.render(**gray), _array_bytes),
        ("outputs", lambda c: c.outputs(), _array_bytes),
        ("render levels again", lambda c: c.render(**pictures), _array_bytes),
        ("velocity", lambda c: c.velocity(), _array_bytes),
        ("render inverted again", lambda c: c.render(**gray), _array_bytes),
        ("advect -1", lambda c: c.advect(x, y, **adv), TA._run_bytes),
        ("render after the march", lambda c: c.render(**pictures), _array_bytes),
    ], pictures, gray


@pytest.mark.parametrize("case,split", [("2d_16x12x8", dict(nslabs=3)), ("1d_33x9", {})], ids=["2d_16x12x8_nslabs3", "1d_33x9"])
def test_render_interleaved_with_the_other_readers(case, split):
    calls, pictures, gray = _calls(case)
    ctx = TM._context(case, **split)
    try:
        mixed = [call(ctx) for _, call, _ in calls]
        out = TM._strip(ctx.outputs())
    finally:
        ctx.close()
    for (name, _, _), dev in zip(calls, mixed):
        if not name.startswith("render"):
            continue
        kw = dict(pictures if "levels" in name or "march" in name else gray)
        a = kw.pop("arrows")
        TG._same_picture(dev, R.render(out, **kw))
        TG._same_arrows(dev, out, a["skip_y"], a["skip_x"], a.get("mask_frac", R.MASK_FRAC))
    seen = {}
    for (name, call, raw), dev in zip(calls, mixed):
        key = name.replace(" again", "").replace("render after the march", "render levels")
        if key not in seen:
            fresh = TM._context(case, **split)
            try:
                seen[key] = raw(call(fresh))
            finally:
                fresh.close()
        assert seen[key] == raw(dev), "%s: %s differs from the same call made first on a fresh context" % (case, name)
