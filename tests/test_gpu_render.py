"""Pictures of the density evolution on the device (csrc/render.hip: k_rho_range, k_render, k_movement;
dotsocp_render_evolution, InPALMContext.render(), render= on the drivers) against the numpy twin (render.render,
render.movement) applied to ctx.outputs() of the SAME context.  Every comparison is exact: uint8 pictures equal, doubles
equal as bytes.

States are made as in tests/test_gpu_report.py: alpha and q entries s * 10^u (s = +-1, u uniform in [-10, 1], seeded), rho0 /
rho1 positive with a few exact zeros; uploaded, begin(), no iteration, finish().  Shapes: 70 x 37 x 9 (two y tiles, the second
ragged; rows pitched 70 -> 80; ragged x), 64 x 4 x 2 (one exact tile; both layers are given data), 3 x 3 x 2, 1-D 130 x 17,
weighted 17 x 21 x 5.  Before a device picture of the 70 x 37 x 9 state is read, the twin's pictures of all nt layers are
checked to exercise the index: 0 and 255 present, at least 100 distinct linear indices and 100 of the 129 level indices, and
an arrow mask that removes between 20 % and 80 % of the nodes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dotsocp_amd as D
from dotsocp_amd import capi
from dotsocp_amd import render as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (ny, nx, nt, weighted); 1-D: ny = None
CASES = {
    "2d_70x37x9": (70, 37, 9, False),
    "2d_64x4x2": (64, 4, 2, False),
    "2d_3x3x2": (3, 3, 2, False),
    "1d_130x17": (None, 130, 17, False),
    "w_17x21x5": (17, 21, 5, True),
    "2d_19x13x7": (19, 13, 7, False),
}
BIG = "2d_70x37x9"
LUT = R.ramp_lut([(0, 0, 40), (30, 200, 255), (255, 255, 0), (200, 0, 0)])
EINVAL, ESTATE = -1, -4


def _signed_pow(rng, n):
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-10, 1, n)


def _density(rng, shape):
    r = rng.uniform(0.5, 1.5, shape)
    r.flat[rng.choice(r.size, 3, replace=False)] = 0.0
    return r


def _shape(case):
    ny, nx, _, _ = CASES[case]
    return (nx,) if ny is None else (ny, nx)


def _context(case, method="inPALM", finish=True, **split):
    """A finished context on the generic state of `case` (no iteration)"""
    ny, nx, nt, weighted = CASES[case]
    rng = np.random.default_rng(sorted(CASES).index(case) + 4242)
    shape = _shape(case)
    var, model = D.initialize(_density(rng, shape), _density(rng, shape), nt)
    nq = var.q.size
    if weighted:
        model.weight = 0.5 + (1e6 - 0.5) * rng.uniform(0, 1, nq) ** 32
    D.InitialScaling(var, model, not weighted, None, dim=1 if ny is None else 2, weighted=weighted)
    var.q, var.alpha = _signed_pow(rng, nq), _signed_pow(rng, nq)
    opts = dict(tau=1.9, sigma=1.0, tol=0.0, maxit=1, ifCheckStepByStep=False, scaling=True)
    ctx = D.InPALMContext(var, opts, model, weighted=weighted, method=method, **split)
    if finish:
        ctx.finish(download=False)
    return ctx


def _barrier(case):
    """a seeded mask over about a tenth of the nodes of a layer"""
    rng = np.random.default_rng(sorted(CASES).index(case) + 99)
    return rng.uniform(0, 1, _shape(case)) < 0.1


def _bits(a):
    return np.asarray(a, dtype=np.float64).tobytes(order="F")


def _same_picture(dev, twin):
    assert dev["image"].dtype == np.uint8 and dev["image"].shape == twin["image"].shape and dev["image"].flags.c_contiguous
    diff = np.count_nonzero(dev["image"] != twin["image"])
    print("  pixels that differ: %d of %d; vmax %r / %r; rho_min %r / %r" % (diff, twin["image"].size, dev["vmax"], twin["vmax"],
                                                                        dev["rho_min"], twin["rho_min"]))
    assert diff == 0
    assert np.array_equal(dev["nodes"], twin["nodes"])
    assert _bits(dev["vmax"]) == _bits(twin["vmax"]) and _bits(dev["rho_min"]) == _bits(twin["rho_min"])
    assert dev["nonfinite"] == twin["nonfinite"] and dev["masked"] == twin["masked"]


def _same_arrows(dev, out, skip_y, skip_x, mask_frac=R.MASK_FRAC):
    mv = R.movement(out, dev["nodes"], dev["vmax"], skip_y, skip_x, mask_frac)
    assert set(mv) <= set(dev)
    for k in mv:
        assert dev[k].shape == mv[k].shape, (k, dev[k].shape, mv[k].shape)
        assert _bits(dev[k]) == _bits(mv[k]), k
    return mv


def _check(ctx, out, arrows=None, **kw):
    """ctx.render(**kw) equals the twin on `out`; arrows = (skip_y, skip_x[, mask_frac])"""
    a = {} if arrows is None else dict(arrows=dict(zip(("skip_y", "skip_x", "mask_frac"), arrows)))
    dev = ctx.render(**kw, **a)
    _same_picture(dev, R.render(out, **kw))
    if arrows is not None:
        _same_arrows(dev, out, *arrows)
    return dev


def _conditions(out):
    """The pictures of all layers of the 70 x 37 x 9 state exercise the index (module docstring); asserted on the twin alone"""
    nt = out["rho"].shape[-1]
    every = list(range(nt))
    lin = R.render(out, frames=every)
    lev = R.render(out, frames=every, mode="levels", nlevels=128)
    n_lin, n_lev = len(np.unique(lin["image"])), len(np.unique(lev["image"]))
    with np.errstate(invalid="ignore"):
        gone = np.count_nonzero(out["rho"] < lin["vmax"] * R.MASK_FRAC) / out["rho"].size
    print("coverage: %d linear indices, %d level indices, %.1f %% of the arrows masked" % (n_lin, n_lev, 100 * gone))
    assert lin["image"].min() == 0 and lin["image"].max() == 255
    assert n_lin >= 100 and n_lev >= 100 and lev["image"].max() <= 128
    assert 0.2 <= gone <= 0.8


@pytest.mark.parametrize("case", ["2d_70x37x9", "2d_64x4x2", "2d_3x3x2", "1d_130x17", "w_17x21x5"])
def test_render_equals_the_twin(case):
    nt = CASES[case][2]
    one_d = CASES[case][0] is None
    ctx = _context(case)
    try:
        out = ctx.outputs()
        if case == BIG:
            _conditions(out)
        every = list(range(nt))
        for barrier in (None, _barrier(case)):
            for mode in ("imshow", "inverted", "levels"):
                for lut in (None, LUT):
                    print(case, mode, "rgb" if lut is not None else "gray", "barrier" if barrier is not None else "")
                    dev = _check(ctx, out, frames=every, mode=mode, lut=lut, barrier=barrier)
                    assert dev["image"].shape == (nt,) + _shape(case) + (() if lut is None else (3,))
            assert dev["masked"] == (0 if barrier is None else nt * np.count_nonzero(barrier))
        for skips in ((1, 1), (3, 2), (1000, 1000)):
            dev = _check(ctx, out, arrows=skips, frames=every)
            assert ("Ey" in dev) == (not one_d)
        _check(ctx, out, arrows=(2, 2, 0.3), frames=[nt - 1], barrier=_barrier(case), barrier_index=0)
        _check(ctx, out, num_frame=2, mode="levels", nlevels=1)
        _check(ctx, out, num_frame=2, mode="levels", nlevels=254, lut=LUT)
        _check(ctx, out, num_frame=1, mode="levels", levels=[0.5, 2.0, 2.5, 300.0])
    finally:
        ctx.close()


def test_frames_in_any_order_and_a_given_scale():
    nt = CASES[BIG][2]
    ctx = _context(BIG)
    try:
        out = ctx.outputs()
        _conditions(out)
        nodes = [nt - 1, 0, 4, 4, 1]
        dev = _check(ctx, out, arrows=(3, 2), frames=nodes, lut=LUT)
        assert dev["nodes"].tolist() == nodes and np.array_equal(dev["image"][2], dev["image"][3])
        own = dev["vmax"]
        for scale in (0.37 * own, 3.0 * own):
            fixed = _check(ctx, out, arrows=(1, 1), frames=nodes, vmax=scale, mode="levels")
            assert fixed["vmax"] == scale and fixed["rho_min"] == dev["rho_min"]
        assert _check(ctx, out, frames=nodes, vmax=0.37 * own)["image"].max() == 255
        assert _check(ctx, out, frames=nodes, vmax=-1.0)["vmax"] == own          # not > 0: the maximum found
        default = ctx.render(arrows=True)                                        # six frames, the reference's skips and mask
        assert default["nodes"].tolist() == R.frame_nodes(nt, 6).tolist()
        _same_picture(default, R.render(out))
        _same_arrows(default, out, *R.movement_skips(70, 37))
    finally:
        ctx.close()


def test_pinned_boundaries_in_rho0():
    """Frame 0 is rho0 verbatim: a rho0 that holds the global maximum P (a power of two), the exact boundaries P j / 256 of
    the linear index and the values one ulp below them, the exact level values divided by k = 255 / P and their neighbours,
    zeros of both signs, a negative value and the arrow threshold P / 100 with its lower neighbour"""
    ny, nx, nt, _ = CASES[BIG]
    ctx = _context(BIG)
    try:
        first = ctx.outputs()["rho"]
        P = 2.0 ** np.ceil(np.log2(2 * first[np.isfinite(first)].max()))
        lv = R.log_levels(128)
        k = 255.0 / P
        j = np.arange(257)
        bounds = P * j / 256
        thr = P * R.MASK_FRAC
        pinned = np.concatenate([bounds, np.nextafter(bounds[1:], 0), lv / k, np.nextafter(lv / k, 0), np.nextafter(lv / k, np.inf),
                                 [0.0, -0.0, -1.0, thr, np.nextafter(thr, 0), np.nextafter(thr, np.inf)]])
        rng = np.random.default_rng(8)
        flat = rng.uniform(0, P, ny * nx)
        assert pinned.size < flat.size
        where = rng.choice(flat.size, pinned.size, replace=False)
        flat[where] = pinned
        rho0 = flat.reshape(ny, nx)
        ctx.model.rho0, ctx._ends = rho0, None
        out = ctx.outputs()
        assert np.array_equal(out["rho"][:, :, 0], rho0) and R.rho_range(out)["vmax"] == P
        for mode in ("imshow", "inverted", "levels"):
            dev = _check(ctx, out, arrows=(1, 1), frames=[0], mode=mode, lut=None)
            got = dev["image"][0].ravel()[where]
            if mode == "imshow":
                assert dev["vmax"] == P
                assert got[:257].tolist() == np.minimum(j, 255).tolist()                     # on a boundary: the upper index
                assert got[257:513].tolist() == (j[1:] - 1).tolist()                         # one ulp below: the lower one
            if mode == "levels":
                on = (lv / k) * k == lv                                                      # s lands on the level itself
                print("levels met exactly by rho * k: %d of 128" % np.count_nonzero(on))
                assert np.array_equal(got[513:641][on], (np.arange(128) + 1)[on])
        for k in ("Ex", "Ey"):                                        # at the threshold, one ulp below it, one ulp above it
            kept, full = dev[k][:, :, 0].ravel()[where[-3:]], out[k][:, :, 0].ravel()[where[-3:]]
            assert _bits(kept[[0, 2]]) == _bits(full[[0, 2]]) and _bits(kept[1]) == _bits(0.0)
        _check(ctx, out, frames=[0, 1], lut=LUT, mode="levels")
    finally:
        ctx.close()


def _slab_ends(nt, world):
    nodes = []
    for r in range(world):
        t0, t1 = capi.slab_range(nt, world, r)
        nodes += [t0, t1 - 1]
    return nodes


@pytest.mark.parametrize("split", [dict(nslabs=3), dict(ngpu=3)], ids=["nslabs3", "create_multi3"])
def test_time_slabs_give_the_same_bytes(split):
    """frames on every slab's first and last layer (the first needs the left neighbour's last cell); dotsocp_create_multi puts
    slab r on device r mod #devices, with its own streams also where only one device is visible"""
    nt = CASES[BIG][2]
    nodes = _slab_ends(nt, 3)
    assert len(set(nodes)) == 6
    nodes = nodes[::-1] + [4]
    kw = dict(frames=nodes, mode="levels", lut=LUT, barrier=_barrier(BIG), arrows=dict(skip_y=3, skip_x=2))
    one = _context(BIG)
    try:
        out = one.outputs()
        ref = one.render(**kw)
    finally:
        one.close()
    ctx = _context(BIG, **split)
    try:
        dev = ctx.render(**kw)
        sout = ctx.outputs()
    finally:
        ctx.close()
    assert np.array_equal(out["rho"], sout["rho"])
    _same_picture(dev, ref)
    _same_picture(dev, R.render(out, **{k: v for k, v in kw.items() if k != "arrows"}))
    for k in ("Ex", "Ey"):
        assert _bits(dev[k]) == _bits(ref[k])
    _same_arrows(dev, out, 3, 2)


@pytest.mark.parametrize("method", ["PALM", "acc-ADMM"])
def test_other_loops(method):
    case = "2d_19x13x7"
    ctx = _context(case, method=method)
    try:
        out = ctx.outputs()
        for mode in ("imshow", "levels"):
            _check(ctx, out, arrows=(2, 3), frames=list(range(7)), mode=mode, lut=LUT, barrier=_barrier(case))
    finally:
        ctx.close()


def _canary_child():
    """Runs in a fresh process with DOTSOCP_CANARY=1: the pictures' buffers lie between guard bands"""
    assert os.environ.get("DOTSOCP_CANARY") == "1"
    for case, split in ((BIG, {}), (BIG, dict(nslabs=3)), ("1d_130x17", {})):
        ctx = _context(case, **split)
        try:
            out = ctx.outputs()
            for lut in (None, LUT):
                _check(ctx, out, arrows=(3, 2), frames=list(range(CASES[case][2])), mode="levels", lut=lut, barrier=_barrier(case))
            assert capi.lib().dotsocp_canary_check() == 0, capi.lib().dotsocp_last_error().decode()
        finally:
            ctx.close()
    assert capi.lib().dotsocp_canary_check() == 0
    print("canary child ok")


def test_render_between_guard_bands():
    code = "import sys; sys.path.insert(0, sys.argv[1]); import test_gpu_render as T; T._canary_child()"
    env = dict(os.environ, DOTSOCP_CANARY="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "tests")], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("canary child ok"), out.stdout[-1000:] + out.stderr[-3000:]


def test_errors_write_nothing():
    L = capi.lib()
    case = "2d_19x13x7"
    ny, nx, nt, _ = CASES[case]
    ctx = _context(case, finish=False)
    try:
        m = ctx.model
        r0, r1 = np.asfortranarray(m.rho0, dtype=np.float64), np.asfortranarray(m.rho1, dtype=np.float64)
        nodes = np.array([0, 3, 6], dtype=np.int64)
        lv = R.log_levels(8)
        image = np.full((3, ny, nx, 3), 0xA5, dtype=np.uint8)
        mvx, mvy = np.full((ny, nx, 3), -7.25, order="F"), np.full((ny, nx, 3), -7.25, order="F")
        info = capi.RenderInfo()
        info.vmax, info.masked = -3.0, 12345

        def opts(**kw):
            o = capi.RenderOpts()
            o.mode, o.channels, o.nf, o.nlevels, o.barrier_index, o.vmax = capi.RENDER_LEVELS, 3, 3, 8, 255, 0.0
            o.skip_y, o.skip_x, o.mask_frac = 1, 1, 0.01
            for k, v in kw.items():
                setattr(o, k, v)
            return o

        def call(o=None, **kw):
            a = dict(rho0=capi.fptr(r0), rho1=capi.fptr(r1), opts=ctypes.byref(o if o is not None else opts()),
                     nodes=nodes.ctypes.data, levels=lv.ctypes.data, lut=LUT.ctypes.data, barrier=None, image=image.ctypes.data,
                     mvx=mvx.ctypes.data, mvy=mvy.ctypes.data)
            a.update(kw)
            rc = L.dotsocp_render_evolution(ctx._ctx, a["rho0"], a["rho1"], a["opts"], a["nodes"], a["levels"], a["lut"], a["barrier"],
                                            a["image"], a["mvx"], a["mvy"], ctypes.byref(info))
            assert np.all(image == 0xA5) and np.all(mvx == -7.25) and np.all(mvy == -7.25), "an output was written"
            assert info.vmax == -3.0 and info.masked == 12345
            if rc:
                assert b"render_evolution" in L.dotsocp_last_error()
            return rc

        assert call() == ESTATE                                       # before finish()
        ctx.finish(download=False)
        for kw in (dict(image=None), dict(opts=None), dict(nodes=None), dict(rho0=None), dict(rho1=None),
                   dict(lut=None),                                    # three channels without a table
                   dict(levels=None), dict(mvx=None), dict(mvy=None)):
            assert call(**kw) == EINVAL, kw
        up, flat, nan = lv.copy(), lv.copy(), lv.copy()
        up[[3, 4]] = up[[4, 3]]
        flat[5] = flat[4]
        nan[2] = np.nan
        for bad in (up, flat, nan):
            assert call(levels=bad.ctypes.data) == EINVAL
        for bad_nodes in ([0, nt, 1], [0, -1, 1]):
            assert call(nodes=np.array(bad_nodes, dtype=np.int64).ctypes.data) == EINVAL, bad_nodes
        for kw in (dict(nlevels=0), dict(nlevels=255), dict(channels=2), dict(channels=0), dict(channels=4), dict(mode=3), dict(mode=-1),
                   dict(nf=0), dict(barrier_index=256), dict(barrier_index=-1), dict(skip_y=-1), dict(skip_x=-2),
                   dict(skip_y=0), dict(skip_x=0),                    # exactly one skip zero
                   dict(vmax=float("inf"))):                          # a scale that is not finite
            assert call(opts(**kw)) == EINVAL, kw
        with pytest.raises(capi.DotsocpError) as ei:                  # no finite positive density: no scale
            ctx.render(barrier=np.ones((ny, nx), dtype=bool))
        assert ei.value.code == EINVAL and "scale" in str(ei.value)
        # the same arguments, valid: everything is written
        rc = L.dotsocp_render_evolution(ctx._ctx, capi.fptr(r0), capi.fptr(r1), ctypes.byref(opts()), nodes.ctypes.data, lv.ctypes.data,
                                        LUT.ctypes.data, None, image.ctypes.data, mvx.ctypes.data, mvy.ctypes.data, ctypes.byref(info))
        assert rc == 0 and info.vmax > 0 and info.masked == 0 and (info.my, info.mx) == (ny, nx)
        out = ctx.outputs()
        assert np.array_equal(image, R.render(out, frames=nodes, mode="levels", nlevels=8, lut=LUT)["image"])
        assert _bits(mvx) == _bits(R.movement(out, nodes, info.vmax)["Ex"])
        rc = L.dotsocp_render_evolution(ctx._ctx, capi.fptr(r0), capi.fptr(r1), ctypes.byref(opts(skip_y=0, skip_x=0, channels=1, mode=0)),
                                        nodes.ctypes.data, None, None, None, image.ctypes.data, None, None, None)
        assert rc == 0                                                # no arrows, no levels, no table, no info
    finally:
        ctx.close()


def test_rccl_contexts_are_refused():
    from oracle.examples import get_example_2d
    rho0, rho1 = get_example_2d("example1", 16, 16)
    var, model = D.initialize_slab(rho0, rho1, 8, 0, 8)
    D.InitialScaling(var, model, True, None, dim=2)
    ctx = D.InPALMContext(var, dict(tau=1.9, sigma=1.0, tol=0.0, maxit=2, scaling=True), model, rccl=(D.capi.rccl_unique_id(), 0, 1))
    try:
        ctx.run(-1)
        ctx.finish(download=False)
        with pytest.raises(capi.DotsocpError) as ei:
            ctx.render()
        assert ei.value.code == EINVAL and "RCCL" in str(ei.value)
    finally:
        ctx.close()


def test_driver_renders_after_a_real_solve():
    rho0, rho1 = D.get_example_2d("example1", 33, 33)
    opts = dict(tol=1e-4, maxit=60)
    output = D.solver_dotsocp2d(rho0, rho1, 9, 2, opts, render=dict(num_frame=6, arrows=True))[0]
    r = output["render"]
    out = {k: v for k, v in output.items() if k != "render"}
    assert r["nodes"].tolist() == R.frame_nodes(9, 6).tolist() == [0, 2, 3, 5, 6, 8]
    assert r["image"].shape == (6, 33, 33) and r["image"].dtype == np.uint8
    assert r["Ex"].shape == (33, 33, 6) and r["Ey"].shape == (33, 33, 6)       # 33 <= 40 nodes: every node keeps its arrow
    assert r["nonfinite"] == 0 and r["masked"] == 0 and r["vmax"] == out["rho"].max()
    assert np.array_equal(r["image"][0], R.indices(np.asarray(rho0, dtype=np.float64), r["vmax"]))
    _same_picture(r, R.render(out, num_frame=6))
    _same_arrows(r, out, 1, 1)
    with pytest.raises(ValueError, match="render= needs transfer='device'"):
        D.solver_dotsocp2d(rho0, rho1, 9, 2, opts, transfer="host", render=dict(num_frame=6))


def test_weighted_driver_masks_its_barrier():
    n = 33
    barrier = D.gene_barrier_of_circle_pillar()
    rho0, rho1 = D.get_example_2d("example1", n, n)
    rho0, rho1, mask = D.ensure_barrier_validity(rho0, rho1, barrier)
    weight = D.get_space_weight_by_barrier(n, n, barrier)
    output = D.solver_wdotsocp2d(rho0, rho1, 9, 1, dict(tol=1e-3, maxit=30, weight=weight), barrier=barrier,
                                 render=dict(num_frame=3, mode="levels", lut=LUT))[0]
    r = output["render"]
    out = {k: v for k, v in output.items() if k != "render"}
    assert r["masked"] == 9 * np.count_nonzero(mask) > 0
    assert np.all(r["image"][:, mask] == LUT[255])
    _same_picture(r, R.render(out, num_frame=3, mode="levels", lut=LUT, barrier=barrier))
