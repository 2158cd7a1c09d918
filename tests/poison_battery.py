"""The scenarios of tests/test_gpu_poison.py, run in a child process: `run_group(name)` runs the scenarios of one group
and prints one JSON object per scenario -- {"scenario", "sha256": {array: digest}, "nonfinite": {array: count},
"launches": {phase: count}} -- on a line of its own.  The parent runs every group twice, plain and under
DOTSOCP_POISON=1, and compares the lines: the same launches on the same inputs, only the contents of never-written device
memory differ, so every digest must be the same.

A scenario is (name, function); the function returns a (nested) dict / sequence of arrays and numbers, and optionally the
launch counts of the phases that show which path ran.  Everything is deterministic: seeded generators, fixed orders."""
import contextlib
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = os.path.join(ROOT, "tests", "golden", "images")
FIELDS = ("phi", "q", "z", "alpha", "beta")
PHASES = ("cone_fused_a", "cone_fused_b", "cone_carry", "qcone", "qstep", "acc_cone", "acc_gather", "transpose", "comm",
          "poisson")
# the one scenario that feeds NaNs in on purpose (tests/test_gpu_dual.py's 24 x 24 special layer): its results may hold
# non-finite values, its digests must still match
NAN_ON_PURPOSE = "post:nan-layer-24x24"


class _Env:
    """what tests/test_gpu_generic_state.py::_gpu_run asks of pytest's monkeypatch; a child process needs no undo"""

    @staticmethod
    def delenv(name, raising=True):
        os.environ.pop(name, None)

    @staticmethod
    def setenv(name, value):
        os.environ[name] = value


@contextlib.contextmanager
def _environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _flatten(obj, prefix, out):
    if obj is None or isinstance(obj, (str, bytes)):
        return
    if hasattr(obj, "keys"):
        for k in sorted(obj.keys()):
            _flatten(obj[k], "%s.%s" % (prefix, k) if prefix else str(k), out)
    elif isinstance(obj, (tuple, list)):
        for i, v in enumerate(obj):
            _flatten(v, "%s[%d]" % (prefix, i), out)
    else:
        a = np.asarray(obj)
        if a.dtype != object:
            out[prefix] = a


def emit(name, result, launches=None, seconds=None, **extra):
    arrays = {}
    _flatten(result, "", arrays)
    assert arrays, name
    line = {"scenario": name,
            "sha256": {k: hashlib.sha256(a.tobytes(order="F")).hexdigest() for k, a in arrays.items()},
            "nonfinite": {k: int(np.count_nonzero(~np.isfinite(a))) if a.dtype.kind == "f" else 0 for k, a in arrays.items()},
            # where to look when a digest differs: the first entry that is not finite (Fortran order)
            "first_nonfinite": {k: int(np.flatnonzero(~np.isfinite(a.ravel(order="F")))[0]) for k, a in arrays.items()
                                if a.dtype.kind == "f" and not np.all(np.isfinite(a))},
            "launches": launches or {}, "seconds": seconds}
    line.update(extra)
    print(json.dumps(line, sort_keys=True), flush=True)


def _loop_result(var, hist, sigma):
    res = {f: getattr(var, f) for f in FIELDS}
    res.update(kkt=hist["kkt"], pdGap=hist["pdGap"], sigma=sigma, cScale=var.cScale, dScale=var.dScale)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# loops
# ---------------------------------------------------------------------------------------------------------------------
def _generic(case, env=None, **split):
    """a case of oracle/generic_state.py from its generic start, as tests/test_gpu_generic_state.py runs it"""
    from oracle import generic_state as G
    import test_gpu_generic_state as T

    def run():
        # (the launch counts: this file's phases, the pencil passes and messages of time slabs among them)
        T.PHASES = PHASES
        var, hist, sigma, counts = T._gpu_run(_Env, case, env, profiling=True, **split)
        return _loop_result(var, hist, sigma), counts
    assert case in G.CASES, case
    tag = ",".join("%s=%s" % kv for kv in sorted({**(env or {}), **{k: str(v) for k, v in split.items()}}.items()))
    return ("%s[%s]" % (case, tag or "default"), run)


def _zero_start(shape, method, K=25, env=None, weighted=False, **split):
    """`example1` from the all-zero start (the circle-pillar barrier when weighted)"""
    ny, nx, nt = shape

    def run():
        import dotsocp_amd as D
        from oracle import driver as OD
        from oracle.examples import (ensure_barrier_validity, gene_barrier_of_circle_pillar, get_example_2d,
                                     get_weight_by_barrier)
        rho0, rho1 = get_example_2d("example1", ny, nx)
        weight = None
        if weighted:
            barrier = gene_barrier_of_circle_pillar()
            weight = get_weight_by_barrier(nx, ny, nt, barrier)
            rho0, rho1, _ = ensure_barrier_validity(rho0, rho1, barrier)
        var, model = D.initialize(rho0, rho1, nt)
        if weight is not None:
            model.weight = np.asarray(weight, dtype=np.float64)
        o = OD.default_opts(dict(tol=0.0, maxit=K), method, weighted)
        D.InitialScaling(var, model, o["scaling"], None, dim=2, weighted=weighted)
        with _environ(env or {}):
            ctx = D.InPALMContext(var, o, model, weighted=weighted, method=method, profiling=True, **split)
            try:
                ctx.run(-1)
                hist, sigma = ctx.finish()
                counts = {k: ctx.kernel_time(k)[1] for k in PHASES}
            finally:
                ctx.close()
        return _loop_result(var, hist, sigma), counts
    tag = ",".join("%s=%s" % kv for kv in sorted({**(env or {}), **{k: str(v) for k, v in split.items()}}.items()))
    return ("zero-%s%s-%dx%dx%d[%s]" % (method, "-weighted" if weighted else "", ny, nx, nt, tag or "default"), run)


def group_loops_generic():
    cases = ["inPALM-130x9x7", "inPALM-128x32x5", "inPALM-1d-150x7", "inPALM-weighted-66x10x6", "ALG2-66x10x6", "PALM-66x10x6",
             "acc-ADMM-66x10x6", "acc-ADMM-theta3-66x10x6", "acc-ADMM-weighted-66x10x6"]
    out = [_generic(c) for c in cases]
    for env in ({"DOTSOCP_FUSED": "0"}, {"DOTSOCP_QCONE": "1"}, {"DOTSOCP_KKT_FOLD": "0"}, {"DOTSOCP_TSOLVE": "dct"}):
        out.append(_generic("inPALM-130x9x7", env))
    return out


def group_loops_unpitched():
    """ny % 16 == 0 and ny * nx < 4096: rows unpitched, columns unpadded -- w0, w1 and beta2 are not zeroed"""
    out = []
    for shape in ((32, 20, 6), (16, 9, 5), (64, 40, 9)):
        for method in ("inPALM", "PALM", "acc-ADMM"):
            out.append(_zero_start(shape, method))
        out.append(_zero_start(shape, "inPALM", env={"DOTSOCP_FUSED": "0"}))
    out.append(_zero_start((48, 30, 13), "inPALM"))
    out.append(_zero_start((48, 30, 13), "inPALM", nslabs=3))
    out.append(_zero_start((48, 30, 13), "inPALM", ngpu=2))
    out.append(_zero_start((32, 20, 6), "inPALM", weighted=True))
    return out


def group_loops_pitch0():
    """DOTSOCP_PITCH=0 in the child's environment (read once per process)"""
    assert os.environ.get("DOTSOCP_PITCH") == "0"
    return [_generic("inPALM-130x9x7"), _generic("PALM-66x10x6"), _generic("acc-ADMM-66x10x6"),
            _generic("inPALM-40x12x13", nslabs=3)]


def _slab_group(tsolve):
    out = []
    for case in ("inPALM-40x12x13", "PALM-40x12x13", "acc-ADMM-40x12x13", "acc-ADMM-weighted-40x12x13"):
        for split in (dict(nslabs=2), dict(nslabs=3), dict(ngpu=2)):
            out.append(_generic(case, {"DOTSOCP_TSOLVE": tsolve}, **split))
    return out


def group_slabs_tri():
    return _slab_group("tri")


def group_slabs_dct():
    return _slab_group("dct")


# ---------------------------------------------------------------------------------------------------------------------
# post-solve calls
# ---------------------------------------------------------------------------------------------------------------------
def _particles(ny, nx, n=40, seed=0):
    """seeds on nodes, on cell borders, on the sides and corners of the square, outside it and anywhere; masses in [0, 2)
    with exact zeros (the recipe of tests/test_gpu_push.py)"""
    rng = np.random.default_rng(n + 7 * seed)
    gx, gy = np.arange(nx) / float(nx - 1), np.arange(ny) / float(ny - 1)
    u = lambda k: rng.uniform(0, 1, k)                                    # noqa: E731
    xs = [rng.choice(gx, 12), rng.choice(gx, 8), u(8), np.array([0.0, 1.0, 0.0, 1.0, 1.0, -0.2, 1.5, 0.3])]
    ys = [rng.choice(gy, 12), u(8), rng.choice(gy, 8), np.array([0.0, 0.0, 1.0, 1.0, 0.5, 0.4, 0.5, 1.0])]
    x, y = np.concatenate(xs), np.concatenate(ys)
    x, y = np.concatenate([x, u(n - x.size)]), np.concatenate([y, u(n - y.size)])
    mass = rng.uniform(0.0, 2.0, n)
    mass[[3, n // 2]] = 0.0
    return x, y, mass


def _post_solve(shape, **split):
    ny, nx, nt = shape

    def run():
        import dotsocp_amd as D
        from oracle import driver as OD
        from oracle.examples import get_example_2d
        rho0, rho1 = get_example_2d("example1", ny, nx)
        var, model = D.initialize(rho0, rho1, nt)
        o = OD.default_opts(dict(tol=0.0, maxit=12), "inPALM", False)
        D.InitialScaling(var, model, o["scaling"], None, dim=2)
        ctx = D.InPALMContext(var, o, model, profiling=True, **split)
        res = {}
        try:
            ctx.run(-1)
            ctx.finish(download=False)
            call = [("outputs", lambda: ctx.outputs()), ("report", lambda: ctx.report()),
                    ("render", lambda: ctx.render(num_frame=3)), ("dual_bound", lambda: ctx.dual_bound(arrays=True))]
            for i, (k, f) in enumerate(call + call[::-1]):
                res["%d-%s" % (i, k)] = f()
            x, y, mass = _particles(ny, nx)
            res["velocity"] = ctx.velocity()
            res["render-arrows"] = ctx.render(num_frame=3, arrows=True)
            for direction in (1, -1):
                res["advect%+d" % direction] = ctx.advect(x, y, nsub=2, direction=direction, trajectories=True)
                res["push%+d" % direction] = ctx.push_forward(x, y, mass=mass, frames=[0, nt // 2, nt - 1], nsub=2,
                                                               direction=direction)
                res["map%+d" % direction] = ctx.map_report(x, y, mass=mass, nsub=2, direction=direction, per_particle=True)
            res["map-lean"] = ctx.map_report(x, y, nsub=1)
            counts = {k: ctx.kernel_time(k)[1] for k in ("velocity_layer", "advect", "deposit", "frame_l1", "advect_path",
                                                         "map_final", "hl_pass_x", "hl_pass_y", "hl_reduce")}
        finally:
            ctx.close()
        return res, counts
    tag = ",".join("%s=%s" % kv for kv in sorted(split.items()))
    return ("post:%dx%dx%d[%s]" % (ny, nx, nt, tag or "one-slab"), run)


def _nan_layer():
    """tests/test_gpu_dual.py::test_ties_zeros_and_non_finite_entries_at_a_chunk_boundary, its 2-D layer"""
    def run():
        import test_gpu_dual as T
        n, at, nt = 24, 8, 2
        w = (0.5 * (1.0 / (n - 1))) * (1.0 / (n - 1))
        line = T._special_line(n, at, w)
        lay = np.full((n, n), 10.0)
        lay[5, :] = line
        lay[:, 17] = line
        lay[20, :] = np.nan
        ctx = T._context((n, n), nt, phi=np.stack([lay, -lay], axis=2), scaling=False)
        try:
            with T._chunk(8):
                dev = ctx.dual_bound(arrays=True)
        finally:
            ctx.close()
        assert dev["nonfinite"] == 2 * np.count_nonzero(~np.isfinite(lay))
        return dev
    return (NAN_ON_PURPOSE, run)


def group_post_solve():
    return [_post_solve((19, 13, 7)), _post_solve((19, 13, 7), nslabs=3), _post_solve((32, 20, 6)),
            _post_solve((32, 20, 6), nslabs=3), _nan_layer()]


# ---------------------------------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------------------------------
def _driver_result(ret):
    out, timeML, histML, hist = ret
    res = {k: out[k] for k in sorted(out) if isinstance(out[k], np.ndarray)}
    res["kkt"] = np.asarray(hist["kkt"])
    res["iters"] = np.array([int(t["Iters"]) for t in timeML if "Iters" in t])
    return res


def group_drivers():
    def two_levels():
        import dotsocp_amd as D
        rho0, rho1 = D.get_example_2d("example1", 33, 33)
        return _driver_result(D.solver_dotsocp2d(rho0, rho1, 9, 2, dict(tol=1e-12, maxit=40), "inPALM", transfer="device"))

    def device_weights():
        import dotsocp_amd as D
        from oracle.examples import (ensure_barrier_validity, gene_barrier_of_circle_pillar, get_example_2d)
        n, nt = 33, 17
        barrier = gene_barrier_of_circle_pillar()
        rho0, rho1 = get_example_2d("example1", n, n)
        rho0, rho1, _ = ensure_barrier_validity(rho0, rho1, barrier)
        w = D.get_space_weight_by_barrier(n, n, barrier)
        return _driver_result(D.solver_wdotsocp2d(rho0, rho1, nt, 2, dict(tol=1e-12, maxit=40, weight=w), "inPALM", barrier,
                                                  weights="device"))

    def imresize():
        from dotsocp_amd import images as I
        import test_gpu_images as T
        res = {}
        for shape_in, shape_out in (((5, 7), (9, 13)), ((9, 13), (5, 7)), ((37, 29), (9, 16))):
            for dtype in (np.uint8, np.float64):
                a = T._input("random", shape_in, dtype)
                res["%dx%d-%dx%d-%s" % (shape_in + shape_out + (np.dtype(dtype).name,))] = I.imresize_device(a, shape_out)
        return res

    def image_example():
        import dotsocp_amd as D
        rho0, rho1 = D.get_example_2d("example5", 33, 33, resources=RES, device=0)
        res = _driver_result(D.solver_dotsocp2d(rho0, rho1, 9, 2, dict(tol=1e-12, maxit=40), "inPALM"))
        res.update(rho0=rho0, rho1=rho1)
        return res

    return [("driver:dot2d-17-to-33", two_levels), ("driver:wdot2d-device-weights-33x33x17", device_weights),
            ("driver:imresize", imresize), ("driver:example5-33x33x9", image_example)]


# ---------------------------------------------------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------------------------------------------------
def _mex_operators():
    def run():
        import dotsocp_amd as D
        rng = np.random.default_rng(99)
        res = {}
        for M, K in ((777, 10), (513, 6), (300, 13)):
            x = np.asfortranarray(rng.standard_normal((M, K)) * rng.choice([0.1, 1, 30], size=(M, 1)))
            got = np.full_like(x, -7.0, order="F")
            D.mexProjSoc(got, x)
            res["proj-%dx%d" % (M, K)] = got
        for nt, nx, ny in ((2, 2, 2), (4, 6, 5), (3, 70, 130)):
            Nz = ny * nx * (nt - 1)
            Nq = Nz + ny * (nx - 1) * nt + (ny - 1) * nx * nt
            q = rng.standard_normal(Nq)
            z = np.asfortranarray(rng.standard_normal((Nz, 10)))            # sentinels in the slots mexBFd leaves unwritten
            D.mexBFd(z, q, nt, nx, ny, 0.731, 1.37)
            w = np.asfortranarray(rng.standard_normal((Nz, 10)))
            qg = np.full(Nq, 5.0)
            D.mexBFdConj(qg, w, nt, nx, ny, 0.731)
            res["bfd-%dx%dx%d" % (nt, nx, ny)], res["bfdconj-%dx%dx%d" % (nt, nx, ny)] = z, qg
        for nt, nx in ((2, 2), (4, 9), (5, 300)):
            Nz = nx * (nt - 1)
            Nq = Nz + (nx - 1) * nt
            q = rng.standard_normal(Nq)
            z = np.asfortranarray(rng.standard_normal((Nz, 6)))
            D.mexBFd1d(z, q, nt, nx, 1.21, 0.6)
            w = np.asfortranarray(rng.standard_normal((Nz, 6)))
            qg = np.zeros(Nq)
            D.mexBFdConj1d(qg, w, nt, nx, 1.21)
            res["bfd1d-%dx%d" % (nt, nx)], res["bfdconj1d-%dx%d" % (nt, nx)] = z, qg
        return res
    return ("operators:mex", run)


def _transforms(n, want_levels=None):
    """dctn, idctn and the Poisson solve with the length n on each of the three axes in turn"""
    def run():
        import dotsocp_amd as D
        rng = np.random.default_rng(n)
        res = {}
        for axis in range(3):
            shape = [3, 2, 2]
            shape[axis] = n
            a = np.asfortranarray(rng.standard_normal(shape))
            res["dctn-axis%d" % axis] = D.mirt_dctn(a)
            res["idctn-axis%d" % axis] = D.mirt_idctn(a)
            res["poisson-axis%d" % axis] = D.oper_poisson3dim(0.37, a)
        reach = {"dct_levels_axis%d" % ax: D.dct_levels(n, ax) for ax in range(3)}
        reach["cdft_levels"] = D.cdft_levels(n)
        if want_levels is not None:
            assert want_levels(reach), (n, reach)
        return res, dict(reach, algorithm=D.dct_algorithm(n))
    return ("operators:transforms-%d" % n, run)


def group_operators():
    import dotsocp_amd as D
    want = {64: "fft", 65: "pfa", 257: "rader", 600: "bluestein", 100: "dense"}
    for n, alg in want.items():
        assert D.dct_algorithm(n) == alg, (n, D.dct_algorithm(n))
    return [_mex_operators()] + [_transforms(n) for n in want]


def group_operators_long():
    """the two two-level transforms at their smallest lengths: DOTSOCP_DCT_LONG_MIN=256 and DOTSOCP_CDFT_LONG_MIN=129 in the
    child's environment (read once per process), as tests/test_gpu_dct_long.py and tests/test_gpu_cdft_long.py lower them"""
    assert os.environ.get("DOTSOCP_DCT_LONG_MIN") == "256" and os.environ.get("DOTSOCP_CDFT_LONG_MIN") == "129"
    return [_transforms(256, lambda r: all(r["dct_levels_axis%d" % ax] == 2 for ax in range(3))),
            _transforms(130, lambda r: r["cdft_levels"] == 2)]


GROUPS = {"loops-generic": group_loops_generic, "loops-unpitched": group_loops_unpitched, "loops-pitch0": group_loops_pitch0,
          "slabs-tri": group_slabs_tri, "slabs-dct": group_slabs_dct, "post-solve": group_post_solve, "drivers": group_drivers,
          "operators": group_operators, "operators-long": group_operators_long}
# what the child of a group finds in its environment in BOTH runs
GROUP_ENV = {"loops-pitch0": {"DOTSOCP_PITCH": "0"},
             "operators-long": {"DOTSOCP_DCT_LONG_MIN": "256", "DOTSOCP_CDFT_LONG_MIN": "129"}}


def run_group(name):
    t_group = time.perf_counter()
    for scenario, fn in GROUPS[name]():
        t0 = time.perf_counter()
        got = fn()
        result, launches = got if isinstance(got, tuple) else (got, None)
        emit(scenario, result, launches, round(time.perf_counter() - t0, 3))
    print(json.dumps({"group": name, "seconds": round(time.perf_counter() - t_group, 3),
                      "poison": os.environ.get("DOTSOCP_POISON", "")}), flush=True)


def cache_cap_child(what):
    """tests/test_gpu_poison.py, the cap of the device block cache (DOTSOCP_DEVICE_CACHE_GB is read once per process).
    "solve": 40 x 40 x 12 twice, as tests/test_gpu_errors.py::test_device_buffers_of_destroyed_contexts_are_reused solves
    it, and what the cache then gave back.  "two_devices": one 32 x 32 x 8 context on device 0, then one on device 1,
    and what the cache held per device in between and afterwards."""
    import dotsocp_amd as D
    from dotsocp_amd import capi
    from oracle import driver as OD
    from oracle.examples import get_example_2d
    L = capi.lib()
    L.dotsocp_release_cache()

    def solve(n, nt, device=0):
        o = OD.default_opts(dict(tol=0.0, maxit=25), "inPALM")
        rho0, rho1 = get_example_2d("example1", n, n)
        var, model = D.initialize(rho0, rho1, nt)
        D.InitialScaling(var, model, True, None, dim=2)
        hist, sigma = D.solver_socp_inPALM(var, o, model, device=device)
        return _loop_result(var, hist, sigma)

    if what == "solve":
        res = {"solve%d" % i: solve(40, 12) for i in range(2)}
        held = int(L.dotsocp_debug_cache_held(-1))
        released = int(L.dotsocp_release_cache())
        assert held == released and L.dotsocp_release_cache() == 0
        emit("cache-cap", res, released=released)
    else:
        res = {"dev0": solve(32, 8, 0)}
        held0 = int(L.dotsocp_debug_cache_held(0))
        res["dev1"] = solve(32, 8, 1)
        emit("cache-per-device", res, held0=held0, held0_after=int(L.dotsocp_debug_cache_held(0)),
             held1=int(L.dotsocp_debug_cache_held(1)), held_all=int(L.dotsocp_debug_cache_held(-1)))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    run_group(sys.argv[1])
