"""Solver-level boundary B1 and the drivers above it, with the reference's names and option
structs:

    [runHist, sigma] = solver_socp_inPALM(var, opts, model)        socp/dot2d|dot1d/algorithms/solver_socp_inPALM.m:1
    [runHist, sigma] = solver_wsocp_inPALM(var, opts, model)       socp/wdot2d/algorithms/solver_wsocp_inPALM.m:1
    [output, timeML, runHistML, runHist] = solver_dotsocp2d(rho0, rho1, nt, levelN, opts, method)
                                                                   socp/dot2d/solver_dotsocp2d.m:1
    ... solver_dotsocp1d (socp/dot1d/solver_dotsocp1d.m:1), solver_wdotsocp2d (socp/wdot2d/solver_wdotsocp2d.m:1)

The whole iteration loop runs on the GPU inside libdotsocp (dot-socp_amd/csrc/solver.hip);
this module only marshals VarHandle / ModelHandle fields across the C ABI.
"""
import ctypes
import time

import numpy as np

from . import capi
from .examples import SpaceWeight
from .model import (InitialScaling, ModelHandle, VarHandle, check_massConservation, initialize,
                    recover_q, recover_RhoE, recoverOrgVar)
from .weights import WeightPyramid

TIME_NAMES = ['Step_1_1_FFT', 'Step_1_2_ProjSOC', 'Step_2_Q_Step', 'Step_3_Multiplier', 'KKT',
              'Total_Time', 'Iters']
# solver_socp_accADMM.m:438-439 (the weighted file lists 'Step_4_Interp' before 'KKT', :443-444)
ACC_TIME_NAMES = ['Step_1_Q_Step', 'Step_2_Multiplier', 'Step_3_1_FFT', 'Step_3_2_ProjSOC', 'KKT', 'Interp',
                  'Total_Time', 'Iters']
WACC_TIME_NAMES = ['Step_1_Q_Step', 'Step_2_Multiplier', 'Step_3_1_FFT', 'Step_3_2_ProjSOC', 'Step_4_Interp', 'KKT',
                   'Total_Time', 'Iters']
PALM_TIME_NAMES = ['Step_1_Q_Step', 'Step_2_1_FFT', 'Step_2_2_ProjSOC', 'Step_3_Q_Step', 'Step_4_Multiplier', 'KKT',
                   'Total_Time', 'Iters']      # solver_socp_PALM.m:351-352
METHODS = {"inPALM": capi.METHOD_INPALM, "ALG2": capi.METHOD_INPALM, "PALM": capi.METHOD_PALM,
           "acc-ADMM": capi.METHOD_ACCADMM}


def _get(opts, name, default=None):
    if isinstance(opts, dict):
        return opts.get(name, default)
    return getattr(opts, name, default)


def _has(opts, name):
    return (name in opts) if isinstance(opts, dict) else hasattr(opts, name)


def _ptr(a):
    return None if a is None else capi.fptr(a)


class InPALMContext:
    """Stateful handle on one device-resident loop (create -> upload -> begin -> run* -> finish)."""

    def __init__(self, var, opts, model, weighted=False, device=0, nslabs=1, profiling=False, rccl=None,
                 method="inPALM", warm_from=None, ngpu=None, z_unread=False, weight_from=None):
        """rccl = (unique_id_bytes, rank, world): one process per GPU, this process owns time slab
        `rank`; var / model then hold the LOCAL slab of every field (model.nt stays the global nt).
        method: which loop file of the reference runs ("inPALM"/"ALG2" by opts.tau, "PALM", "acc-ADMM").
        warm_from: the finished context of the previous (coarser) multilevel level: phi, q, alpha, z, beta are
        then produced on the device by jump_nextLevel.m's transfer instead of being uploaded from `var`.
        ngpu: single-process multi-GPU (dotsocp_create_multi): that many time slabs, slab r on device
        (device + r) mod #devices; nslabs (diagnostic) keeps all slabs on `device`.
        z_unread: the caller will run at least one iteration of the inPALM / ALG2 loop, which overwrites z before its first
        use (solver_socp_inPALM.m:199; the rescale block, the only other reader, needs it >= 10): var.z is not uploaded --
        10 of the 27 N doubles of the state (tests/test_gpu_solver.py::test_iterations_from_a_random_state).
        weight_from = (WeightPyramid, level): model.weight is that level of the pyramid, copied device to device
        (dotsocp_upload_weight_from); model.weight itself is not read."""
        L = capi.lib()
        self.method = method
        one_d = not hasattr(model, "ny")
        p = capi.Problem()
        p.dim = 1 if one_d else 2
        p.weighted = 1 if weighted else 0
        p.ny = 1 if one_d else int(model.ny)
        p.nx, p.nt = int(model.nx), int(model.nt)
        p.D, p.E, p.cScale, p.dScale = float(var.D), float(var.E), float(var.cScale), float(var.dScale)
        p.normc, p.normd = float(model.normc), float(model.normd)
        self.var, self.model, self.weighted = var, model, weighted
        if ngpu is not None and int(ngpu) > 1:
            self._ctx = L.dotsocp_create_multi(ctypes.byref(p), int(device), int(ngpu))
        else:
            self._ctx = L.dotsocp_create(ctypes.byref(p), int(device), int(nslabs))
        if not self._ctx:
            raise capi.DotsocpError(-1, L.dotsocp_last_error().decode())
        try:
            if rccl is not None:
                uid, rk, wd = rccl
                buf = (ctypes.c_ubyte * 128).from_buffer_copy(bytes(uid))
                capi.check(L.dotsocp_attach_rccl(self._ctx, buf, int(rk), int(wd)))
            # a field left as None keeps the device default (zeros), e.g. z, beta, q, alpha of a cold start
            skip_z = z_unread and METHODS[method] == capi.METHOD_INPALM and int(_get(opts, "maxit")) >= 1
            state = () if warm_from is not None else ((capi.F_PHI, var.phi), (capi.F_Q, var.q), (capi.F_ALPHA, var.alpha),
                                                      (capi.F_Z, None if skip_z else var.z), (capi.F_BETA, var.beta))
            for f, a in state:
                if a is not None:
                    self.upload(f, a)
            ends = getattr(model, "_c_ends", None)
            if ends is not None and model.c.size > 2 * ends and rccl is None:
                # initialize(lazy_zeros=True): c is zero between its first and last layer, as the device array is
                nlay = model.c.size // ends
                for t, part in ((0, model.c[:ends]), (nlay - 1, model.c[model.c.size - ends:])):
                    capi.check(L.dotsocp_upload_layers(self._ctx, capi.F_C, capi.fptr(np.ascontiguousarray(part)), t, 1))
            else:
                self.upload(capi.F_C, model.c)
            if weighted and weight_from is not None:
                weight_from[0].upload_to(self, weight_from[1])
            elif weighted:
                self.upload(capi.F_WEIGHT, model.weight)
            if warm_from is not None:
                capi.check(L.dotsocp_jump_next_level(warm_from._ctx, self._ctx))
            if profiling:
                capi.check(L.dotsocp_set_profiling(self._ctx, 1))
            o = capi.Opts()
            # required fields (solver_socp_inPALM.m:33-37)
            o.tau = float(_get(opts, "tau", 1.0) if method == "acc-ADMM" else _get(opts, "tau"))
            o.sigma, o.tol = float(_get(opts, "sigma")), float(_get(opts, "tol"))
            o.maxit = int(_get(opts, "maxit"))
            o.ifCheckStepByStep = int(bool(_get(opts, "ifCheckStepByStep", False)))
            # optional fields (:20-30,64-68)
            o.checkPrimDualFeas = int(bool(_get(opts, "checkPrimDualFeas"))) if _has(opts, "checkPrimDualFeas") else -1
            o.scaling = int(bool(_get(opts, "scaling", False)))
            o.time_limit = float(_get(opts, "time_limit", 3600))
            if METHODS[method] == capi.METHOD_INPALM:
                capi.check(L.dotsocp_begin(self._ctx, ctypes.byref(o)))
            else:
                a = capi.AccOpts()                  # solver_socp_accADMM.m:12-28; 0 = reference default
                a.restart = int(_get(opts, "restart", 0) or 0)
                a.rho = float(_get(opts, "rho", 0) or 0)
                a.theta = float(_get(opts, "theta", 0) or 0)
                capi.check(L.dotsocp_begin_method(self._ctx, ctypes.byref(o), METHODS[method], ctypes.byref(a)))
        except Exception:
            self.close()
            raise

    def upload(self, field, arr):
        a = np.asfortranarray(arr, dtype=np.float64)
        capi.check(capi.lib().dotsocp_upload(self._ctx, field, capi.fptr(a)))

    def download(self, field, like):
        out = np.empty(like.shape, dtype=np.float64, order="F")
        capi.check(capi.lib().dotsocp_download(self._ctx, field, capi.fptr(out)))
        return out

    def run(self, n_iters=-1):
        done = capi.i64()
        capi.check(capi.lib().dotsocp_run(self._ctx, int(n_iters), ctypes.byref(done)))
        return done.value

    def synchronize(self):
        capi.check(capi.lib().dotsocp_synchronize(self._ctx))

    def kernel_time(self, name):
        ms, n = capi.dbl(), capi.i64()
        capi.check(capi.lib().dotsocp_kernel_time(self._ctx, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def finish(self, download=True):
        """solver_socp_inPALM.m:329-357: write iterates and scaling factors back into `var`."""
        L = capi.lib()
        res = capi.Result()
        capi.check(L.dotsocp_finish(self._ctx, ctypes.byref(res)))
        var = self.var
        var.name = {"acc-ADMM": 'Accelerated ADMM', "PALM": 'Proximal ALM'}.get(self.method, 'Inexact Proximal ALM')
        if download:
            var.phi = self.download(capi.F_PHI, var.phi)
            var.q = self.download(capi.F_Q, var.q)
            var.z = self.download(capi.F_Z, var.z)
            var.alpha = self.download(capi.F_ALPHA, var.alpha)       # = sigma * alpha
            var.beta = self.download(capi.F_BETA, var.beta)          # = sigma * beta
        t = list(res.times)
        if self.method == "acc-ADMM":
            tm = dict(Step_1_Q_Step=t[2], Step_2_Multiplier=t[3], Step_3_1_FFT=t[0], Step_3_2_ProjSOC=t[1], KKT=t[4],
                      Interp=res.time_extra, Step_4_Interp=res.time_extra, Total_Time=t[5], Iters=t[6])
            var.time = {k: tm[k] for k in (WACC_TIME_NAMES if self.weighted else ACC_TIME_NAMES)}
        elif self.method == "PALM":
            var.time = dict(zip(PALM_TIME_NAMES, [res.time_extra] + t))
        else:
            var.time = dict(zip(TIME_NAMES, t))
        var.cScale, var.dScale = res.cScale, res.dScale
        n = int(res.hist_len)
        kkt = np.empty((n, 7), order="F")
        tm, itr, gap = np.empty(n), np.empty(n), np.empty(n)
        capi.check(L.dotsocp_get_history(self._ctx, capi.fptr(kkt) if n else None, capi.fptr(tm) if n else None,
                                         capi.fptr(itr) if n else None, capi.fptr(gap) if n else None))
        runHist = dict(kkt=kkt, time=tm, iter=itr, pdGap=gap, len=n)
        self.result = res
        return runHist, res.sigma

    def _rho_ends(self):
        """model.rho0 / rho1 in the column-major layout the library reads, converted once per context (10 ms for a pair of
        row-major 1024 x 1024 arrays: several times what the whole device report takes)"""
        if getattr(self, "_ends", None) is None:
            self._ends = (np.asfortranarray(self.model.rho0, dtype=np.float64), np.asfortranarray(self.model.rho1, dtype=np.float64))
        return self._ends

    def outputs(self):
        """solver_dotsocp2d.m:262-281 on the device (recoverOrgVar + recover_RhoE + recover_q): dict with rho, Ex,
        [Ey,] q0, bx[, by]; call after finish()."""
        m = self.model
        one_d = not hasattr(m, "ny")
        nt = int(m.nt)
        shp = (int(m.nx),) if one_d else (int(m.ny), int(m.nx))
        names = ("rho", "Ex", "q0", "bx") if one_d else ("rho", "Ex", "Ey", "q0", "bx", "by")
        out = {k: np.empty(shp + ((nt - 1,) if k in ("q0", "bx", "by") else (nt,)), order="F") for k in names}
        r0, r1 = self._rho_ends()
        ptr = lambda k: capi.fptr(out[k]) if k in out else None      # noqa: E731
        capi.check(capi.lib().dotsocp_recover_outputs(self._ctx, capi.fptr(r0), capi.fptr(r1), ptr("rho"), ptr("Ex"),
                                                      ptr("Ey"), ptr("q0"), ptr("bx"), ptr("by")))
        return out

    def report(self):
        """The solution report on the device (dotsocp_solution_report; report.py): mass conservation, negative densities,
        violation of f(q) <= 0 and the transport cost of the finished solve, from one pass over the device-resident alpha
        and q -- no output array is made or downloaded.  Call after finish(); same numbers as
        report.solution_report(self.outputs())."""
        from .report import from_struct
        m = self.model
        nt = int(m.nt)
        r0, r1 = self._rho_ends()
        rep, mass, neg = capi.Report(), np.empty(nt), np.empty(nt)
        capi.check(capi.lib().dotsocp_solution_report(self._ctx, capi.fptr(r0), capi.fptr(r1), ctypes.byref(rep),
                                                      capi.fptr(mass), capi.fptr(neg)))
        return from_struct(rep, mass, neg)

    def geodesic(self):
        """The geodesic's profile on the device (dotsocp_geodesic_profile; geodesic.py): per time node the mass, the moments,
        the momentum, the kinetic energy, the entropy, the largest density and the support of the finished solve, and what
        they say about it as a geodesic (constant speed, straight centre line, convex entropy, bounded peak), from one pass
        over the device-resident alpha -- no output array is made or downloaded.  Call after finish(); the numbers of
        geodesic.geodesic_profile(self.outputs()), the sums to rounding."""
        from .geodesic import from_struct
        m = self.model
        nt = int(m.nt)
        r0, r1 = self._rho_ends()
        res, sums = capi.Geodesic(), np.empty((nt, capi.GEO_SUMS), order="F")
        rho_max, n_support = np.empty(nt), np.empty(nt, dtype=np.int64)
        capi.check(capi.lib().dotsocp_geodesic_profile(self._ctx, capi.fptr(r0), capi.fptr(r1), ctypes.byref(res), capi.fptr(sums),
                                                       capi.fptr(rho_max), n_support.ctypes.data))
        return from_struct(res, sums, rho_max, n_support, r0.size)

    def dual_bound(self, arrays=False):
        """A lower bound on W2^2 between the node histograms of rho0 and rho1, on the device (dotsocp_dual_bound; dual.py):
        the Hopf-Lax transform of phi(t = 0) forward to t = 1 and of phi(t = 1) back to t = 0, and the Kantorovich dual of
        each pair -- valid whatever state the solve is in.  Returns a dual.DualBound (bound, bound_fwd, bound_bwd, dual_raw,
        the Hopf-Lax gaps at both ends, map_cost_bwd, ...); arrays=True adds H, B (the transforms) and arg_fwd, arg_bwd (int32,
        the flat winning node of every node, y fastest).  Same bits as dual.dual_bound() of the downloaded, recovered layers.
        Call after finish(); unweighted contexts only."""
        from .dual import from_struct
        m = self.model
        shp = (int(m.nx),) if not hasattr(m, "ny") else (int(m.ny), int(m.nx))
        r0, r1 = self._rho_ends()
        res = capi.Dual()
        arr = [np.empty(shp, order="F", dtype=t) if arrays else None for t in (np.float64, np.float64, np.int32, np.int32)]
        ptr = lambda a: None if a is None else a.ctypes.data         # noqa: E731
        capi.check(capi.lib().dotsocp_dual_bound(self._ctx, capi.fptr(r0), capi.fptr(r1), ctypes.byref(res), *[ptr(a) for a in arr]))
        return from_struct(res, *arr)

    def upper_bound(self, eps_h2=0.25, max_sweeps=50, defect_tol=0.0, start=1, f_start=None, arrays=False):
        """An upper bound on W2^2 between the node histograms of rho0 and rho1, on the device (dotsocp_upper_bound; upper.py):
        log-domain Sinkhorn sweeps at the temperature eps_h2 hx hy from f = -phi(t = 0) (start=1), f_start (start=2) or zeros
        (start=0), rounded to an exactly feasible plan -- valid whatever state the solve is in; with dual_bound() the bracket
        bound <= W2^2 <= upper.  Returns an upper.UpperBound (upper, cost_kept, cost_fill, kept, fill, sweeps, the defects of
        the first and last sweep, ...); arrays=True adds f, g (the scaled-down potentials), E, er, ec and defects.  Call after
        finish(); unweighted contexts only."""
        from . import upper as U
        m = self.model
        shp = (int(m.nx),) if not hasattr(m, "ny") else (int(m.ny), int(m.nx))
        r0, r1 = self._rho_ends()
        return U.device_call(lambda *a: capi.lib().dotsocp_upper_bound(self._ctx, *a), r0, r1, shp, eps_h2, max_sweeps,
                             defect_tol, start, f_start, arrays)

    def plan_map(self, eps_h2=0.25, max_sweeps=50, defect_tol=0.0, start=1, f_start=None, arrays=False, frames=None, compare=None):
        """upper_bound() and the transport map of its plan, on the device (dotsocp_upper_map; upper.py): the barycentric map
        T(x) = x + (Dx, Dy) of the rounded plan -- a second, static map beside the one the flow realises; a projection, not
        measure preserving --, its cost and the spread around it (map_cost + spread = cost_rows = upper, to rounding).
        frames: time nodes (any order) at which the displacement interpolant ((1 - tau) Id + tau T)# rho0, tau = node / (nt - 1),
        is deposited; l1[k] = mean |frames[..., k] - rho(node)|.  compare = dict(stride=1, nsub=1): particles seeded on every
        stride-th node of positive mass are marched by advect(); map_gap = the mass-weighted mean of |X(1) - T(x)|^2,
        map_gap_max its maximum (upper.map_gap).  Returns an upper.PlanMap (+ frames, l1, nodes; + map_gap, map_gap_max).
        Call after finish(); unweighted contexts only."""
        from . import upper as U
        from .advect import masses_on_nodes, seeds_on_nodes
        m = self.model
        one_d = not hasattr(m, "ny")
        shp = (int(m.nx),) if one_d else (int(m.ny), int(m.nx))
        r0, r1 = self._rho_ends()
        nodes = None if frames is None else np.array(frames, dtype=np.int64).ravel()
        l1 = np.empty(0 if nodes is None else nodes.size)
        call = lambda *a: capi.lib().dotsocp_upper_map(self._ctx, *a, l1.ctypes.data if l1.size else None)   # noqa: E731
        out = U.device_map_call(call, r0, r1, shp, eps_h2, max_sweeps, defect_tol, start, f_start, arrays, nodes, int_times=True)
        if nodes is not None and nodes.size:
            out.update(l1=l1, nodes=nodes)
        if compare is not None:
            stride, nsub = int(compare.get("stride", 1)), int(compare.get("nsub", 1))
            mask = np.asarray(m.rho0) > 0
            x, y = seeds_on_nodes(int(m.nx), None if one_d else int(m.ny), stride=stride, mask=mask)
            at = lambda t: masses_on_nodes(t, stride=stride, mask=mask)             # noqa: E731
            end = self.advect(x, y, nsub=nsub)
            out.update(U.map_gap(x, y, end["x"], end["y"], at(out["Dx"]), None if one_d else at(out["Dy"]), at(m.rho0)))
        return out

    def render(self, frames=None, num_frame=6, mode="imshow", nlevels=128, lut=None, barrier=None, vmax=None, arrows=False,
               barrier_index=255, levels=None):
        """Pictures of the density evolution on the device (dotsocp_render_evolution; render.py): uint8 frames at the nodes
        `frames` (any order, repeats allowed; None: render.frame_nodes(nt, num_frame)) in mode "imshow", "inverted" or
        "levels" (nlevels log-spaced levels, or `levels`), as indices or -- lut: a (256, 3) uint8 table -- as RGB; barrier:
        a mask (ny, nx) or a barrier function of the examples; vmax > 0 fixes the scale.  arrows: False, True (the reference's
        skips, render.movement_skips, and mask 0.01) or dict(skip_y=, skip_x=, mask_frac=).  Returns dict(image, nodes, vmax,
        rho_min, nonfinite, masked[, Ex[, Ey]]): image (nf, ny, nx[, 3]) C-ordered (1-D: (nf, nx[, 3])), Ex / Ey
        (my, mx, nf) Fortran-ordered (1-D: Ex (mx, nf)); the same bytes as render.render / render.movement of
        self.outputs().  Call after finish(); only the pictures cross PCIe."""
        from . import render as R
        m = self.model
        one_d = not hasattr(m, "ny")
        nt = int(m.nt)
        shp = (int(m.nx),) if one_d else (int(m.ny), int(m.nx))
        if mode not in R.MODES:
            raise ValueError("render(): mode must be one of %s" % sorted(R.MODES))
        nodes = R.frame_nodes(nt, num_frame) if frames is None else np.array(frames, dtype=np.int64).ravel()
        o = capi.RenderOpts()
        o.mode, o.channels, o.nf = R.MODES[mode], 1 if lut is None else 3, int(nodes.size)
        o.barrier_index, o.vmax = int(barrier_index), float(vmax) if vmax is not None else 0.0
        lv = None
        if mode == "levels":
            lv = np.ascontiguousarray(R.log_levels(nlevels) if levels is None else levels, dtype=np.float64).ravel()
            o.nlevels = int(lv.size)
        table = None if lut is None else R.check_lut(lut)
        b = R.barrier_mask(barrier, shp)
        mask = None if b is None else np.asfortranarray(b, dtype=np.uint8)
        Ex = Ey = None
        if arrows:
            a = dict(arrows) if isinstance(arrows, dict) else {}
            sy, sx = R.movement_skips(1 if one_d else shp[0], shp[-1])
            o.skip_y, o.skip_x = (1 if one_d else int(a.get("skip_y", sy))), int(a.get("skip_x", sx))
            o.mask_frac = float(a.get("mask_frac", R.MASK_FRAC))
            if o.skip_y >= 1 and o.skip_x >= 1:
                cut = tuple(-(-n // s) for n, s in zip(shp, (o.skip_x,) if one_d else (o.skip_y, o.skip_x)))
                Ex = np.empty(cut + (nodes.size,), order="F")
                Ey = None if one_d else np.empty(cut + (nodes.size,), order="F")
        image = np.empty((nodes.size,) + shp + (() if lut is None else (3,)), dtype=np.uint8)
        info = capi.RenderInfo()
        r0, r1 = self._rho_ends()
        ptr = lambda a: None if a is None else a.ctypes.data         # noqa: E731
        capi.check(capi.lib().dotsocp_render_evolution(self._ctx, capi.fptr(r0), capi.fptr(r1), ctypes.byref(o), nodes.ctypes.data,
                                                       ptr(lv), ptr(table), ptr(mask), image.ctypes.data, ptr(Ex), ptr(Ey),
                                                       ctypes.byref(info)))
        out = dict(image=image, nodes=nodes, vmax=float(info.vmax), rho_min=float(info.rho_min), nonfinite=int(info.nonfinite),
                   masked=int(info.masked))
        if Ex is not None:
            out["Ex"] = Ex
        if Ey is not None:
            out["Ey"] = Ey
        return out

    def _rho_floor(self, rho_floor):
        from .advect import default_rho_floor
        return default_rho_floor(self.model.rho0, self.model.rho1) if rho_floor is None else float(rho_floor)

    def velocity(self, rho_floor=None):
        """v = E / rho at the nodes on the device (dotsocp_recover_velocity; advect.py): dict(vx[, vy]) of the shapes of
        outputs()["rho"]; zero where rho <= rho_floor (None: advect.default_rho_floor(rho0, rho1)) or the quotient is not
        finite.  Call after finish(); same bits as advect.velocity(self.outputs(), rho_floor)."""
        m = self.model
        one_d = not hasattr(m, "ny")
        shp = ((int(m.nx),) if one_d else (int(m.ny), int(m.nx))) + (int(m.nt),)
        v = {k: np.empty(shp, order="F") for k in (("vx",) if one_d else ("vx", "vy"))}
        r0, r1 = self._rho_ends()
        capi.check(capi.lib().dotsocp_recover_velocity(self._ctx, capi.fptr(r0), capi.fptr(r1), self._rho_floor(rho_floor),
                                                       capi.fptr(v["vx"]), None if one_d else capi.fptr(v["vy"])))
        return v

    def _march_inputs(self, who, x, y, mass, nsub, direction, rho_floor):
        """What advect(), push_forward() and map_report() (`who`, named in every ValueError) hand to the library alike: one_d,
        the seed arrays (copies: the end positions are written there), the masses or None, the opts, rho0 / rho1."""
        one_d = not hasattr(self.model, "ny")
        if one_d != (y is None):
            raise ValueError("%s(): y is given on a 2-D context and only there" % who)
        if who == "push_forward" and mass is None:
            raise ValueError("%s(): mass is needed" % who)
        px = np.array(x, dtype=np.float64).ravel()
        py = None if one_d else np.array(y, dtype=np.float64).ravel()
        ms = None if mass is None else np.array(mass, dtype=np.float64).ravel()
        if (py is not None and py.size != px.size) or (ms is not None and ms.size != px.size):
            raise ValueError("%s(): %s" % (who, "x and y hold the same number of seeds" if who == "advect" else
                                           "x, y and mass hold one entry per seed"))
        o = capi.PushOpts() if who == "push_forward" else capi.AdvectOpts()
        o.n, o.nsub, o.direction, o.rho_floor = int(px.size), int(nsub), int(direction), self._rho_floor(rho_floor)
        return (one_d, px, py, ms, o) + tuple(capi.fptr(r) for r in self._rho_ends())

    def advect(self, x, y=None, nsub=1, direction=+1, rho_floor=None, trajectories=False):
        """Particles along the solved flow on the device (dotsocp_advect_particles; advect.py): RK4 along v = E / rho from
        the seeds x, y (y None on a 1-D context) over t = 0 -> 1 (direction=+1) or 1 -> 0 (-1), nsub steps per time
        interval.  Returns dict(x, y, traj_x, traj_y, n_clamped) as advect.advect does, with the same bits as
        advect.advect(self.outputs(), ...).  Call after finish()."""
        one_d, px, py, _, o, r0, r1 = self._march_inputs("advect", x, y, None, nsub, direction, rho_floor)
        nt = int(self.model.nt)
        tx = np.empty((px.size, nt), order="F") if trajectories else None
        ty = np.empty((px.size, nt), order="F") if trajectories and not one_d else None
        nc = capi.i64()
        capi.check(capi.lib().dotsocp_advect_particles(self._ctx, r0, r1, ctypes.byref(o), _ptr(px), _ptr(py), _ptr(tx), _ptr(ty),
                                                       ctypes.byref(nc)))
        return dict(x=px, y=py, traj_x=tx, traj_y=ty, n_clamped=int(nc.value))

    def push_forward(self, x, y=None, mass=None, frames=None, nsub=1, direction=+1, rho_floor=None):
        """The mass the particles carry, deposited on the grid at the time nodes `frames` (None: every node) on the device
        (dotsocp_push_mass; advect.py): the particles of advect() with one mass each (finite, >= 0, not all zero), integer
        accumulation -- exact conservation, the same bits for any particle order and slab split.  Returns dict(frames,
        counts, nodes, unit, l1, x, y, n_clamped, total_units) as advect.push_forward does, with the same bits as
        advect.push_forward(self.outputs(), ...) (l1: to rounding; identical between two calls).  Call after finish()."""
        one_d, px, py, ms, o, r0, r1 = self._march_inputs("push_forward", x, y, mass, nsub, direction, rho_floor)
        m = self.model
        nodes = np.arange(int(m.nt), dtype=np.int64) if frames is None else np.array(frames, dtype=np.int64).ravel()
        o.nf = int(nodes.size)
        shp = (int(m.nx),) if one_d else (int(m.ny), int(m.nx))
        fr = np.empty(shp + (nodes.size,), order="F")
        l1 = np.empty(nodes.size)
        nc, unit = capi.i64(), capi.dbl()
        capi.check(capi.lib().dotsocp_push_mass(self._ctx, r0, r1, ctypes.byref(o), _ptr(px), _ptr(py), capi.fptr(ms),
                                                nodes.ctypes.data, capi.fptr(fr), ctypes.byref(nc), ctypes.byref(unit), capi.fptr(l1)))
        u = unit.value
        counts = (fr / u).astype(np.int64)                 # exact: the frames are whole multiples of a power of two
        return dict(frames=fr, counts=counts, nodes=nodes, unit=u, l1=l1, x=px, y=py, n_clamped=int(nc.value),
                    total_units=int(np.rint(ms / u).astype(np.int64).sum()))

    def _node_particles(self, stride, direction):
        """x, y, mass of the given density itself: a particle on every stride-th node (advect.seeds_on_nodes) with the value
        of rho0 there as its mass (direction=-1: of rho1, carried back from t = 1)"""
        from .advect import masses_on_nodes, seeds_on_nodes
        m = self.model
        dens = np.asarray(m.rho0 if int(direction) > 0 else m.rho1, dtype=np.float64)
        x, y = seeds_on_nodes(int(m.nx), int(m.ny) if hasattr(m, "ny") else None, stride=stride)
        return x, y, masses_on_nodes(dens, stride=stride)

    def push_from_nodes(self, stride=1, frames=None, nsub=1, direction=+1, rho_floor=None):
        """push_forward() of the given density itself (_node_particles).  With stride=1, l1 at the far end is the defect of
        the transport map: how far the pushed rho0 is from rho1."""
        x, y, mass = self._node_particles(stride, direction)
        return self.push_forward(x, y, mass=mass, frames=frames, nsub=nsub, direction=direction, rho_floor=rho_floor)

    def map_report(self, x, y=None, mass=None, nsub=1, direction=+1, rho_floor=None, per_particle=False):
        """How good the flow is as a transport map, on the device (dotsocp_map_report; advect.py): the particles of
        advect() each give their displacement, path length and kinetic action (disp^2 <= len^2 <= action, equal for
        straight paths at constant speed); returned are their mass-weighted means (mass None: all 1), maxima, the
        histogram of the detour 1 - disp / len, the final positions and -- per_particle=True -- the three arrays.  Same
        keys and same bits as advect.map_report(self.outputs(), ...).  Call after finish()."""
        _, px, py, ms, o, r0, r1 = self._march_inputs("map_report", x, y, mass, nsub, direction, rho_floor)
        arr = [np.empty(px.size) if per_particle else None for _ in range(3)]
        rep = capi.MapReport()
        capi.check(capi.lib().dotsocp_map_report(self._ctx, r0, r1, ctypes.byref(o), _ptr(px), _ptr(py), _ptr(ms), ctypes.byref(rep),
                                                 _ptr(arr[0]), _ptr(arr[1]), _ptr(arr[2])))
        out = {k: (int if t is capi.i64 else float)(getattr(rep, k)) for k, t in capi.MapReport._fields_ if k != "detour_hist"}
        out.update(detour_hist=np.array(rep.detour_hist[:], dtype=np.int64), x=px, y=py, disp=arr[0], len=arr[1], action=arr[2])
        return out

    def map_report_from_nodes(self, stride=1, nsub=1, direction=+1, rho_floor=None, per_particle=False):
        """map_report() of the given density itself, seeded as push_from_nodes() seeds it (_node_particles): cost_map is then
        the cost of the map the flow realises, to set beside report()["cost"]."""
        x, y, mass = self._node_particles(stride, direction)
        return self.map_report(x, y, mass=mass, nsub=nsub, direction=direction, rho_floor=rho_floor, per_particle=per_particle)

    def close(self):
        if getattr(self, "_ctx", None):
            capi.lib().dotsocp_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        self.close()


def solver_socp_inPALM(var, opts, model, device=0, nslabs=1):
    """[runHist, sigma] = solver_socp_inPALM(var, opts, model); `var` is mutated in place.
    nslabs > 1 runs the multi-GPU time-slab algorithm with all slabs on this one device."""
    ctx = InPALMContext(var, opts, model, weighted=False, device=device, nslabs=nslabs, z_unread=True)
    try:
        ctx.run(-1)
        return ctx.finish()
    finally:
        ctx.close()


def solver_wsocp_inPALM(var, opts, model, device=0, nslabs=1):
    """[runHist, sigma] = solver_wsocp_inPALM(var, opts, model) (model.weight required)."""
    ctx = InPALMContext(var, opts, model, weighted=True, device=device, nslabs=nslabs, z_unread=True)
    try:
        ctx.run(-1)
        return ctx.finish()
    finally:
        ctx.close()


def solver_socp_PALM(var, opts, model, device=0, nslabs=1):
    """[runHist, sigma] = solver_socp_PALM(var, opts, model)   socp/dot2d/algorithms/solver_socp_PALM.m:1
    nslabs > 1: the time-slab algorithm with all slabs on this one device (as for solver_socp_inPALM)."""
    ctx = InPALMContext(var, opts, model, weighted=False, device=device, method="PALM", nslabs=nslabs)
    try:
        ctx.run(-1)
        return ctx.finish()
    finally:
        ctx.close()


def solver_socp_accADMM(var, opts, model, device=0, nslabs=1):
    """[runHist, sigma] = solver_socp_accADMM(var, opts, model)   socp/dot2d/algorithms/solver_socp_accADMM.m:1
    opts: sigma, maxit, tol, ifCheckStepByStep (+ restart, rho, theta, checkPrimDualFeas, time_limit, scaling)."""
    ctx = InPALMContext(var, opts, model, weighted=False, device=device, method="acc-ADMM", nslabs=nslabs)
    try:
        ctx.run(-1)
        return ctx.finish()
    finally:
        ctx.close()


def solver_wsocp_accADMM(var, opts, model, device=0, nslabs=1):
    """socp/wdot2d/algorithms/solver_wsocp_accADMM.m:1"""
    ctx = InPALMContext(var, opts, model, weighted=True, device=device, method="acc-ADMM", nslabs=nslabs)
    try:
        ctx.run(-1)
        return ctx.finish()
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------
# drivers
# --------------------------------------------------------------------------------------
def _driver_opts(opts, method, weighted, dim=2):
    """solver_dotsocp2d.m:76-151 / solver_dotsocp1d.m / solver_wdotsocp2d.m:85-162."""
    ok = method in ("inPALM", "ALG2") or (method == "acc-ADMM" and dim == 2) or (
        method == "PALM" and dim == 2 and not weighted)                   # solver_dotsocp2d.m:205-226
    if not ok:
        raise ValueError("Invalid input at position 6 (Solving method)")
    o = dict(opts) if isinstance(opts, dict) else dict(vars(opts))
    o.setdefault("ifCheckStepByStep", False)
    o.setdefault("scaling", True)
    o.setdefault("maxit", 10000 if weighted else 3000)
    if method != "acc-ADMM":
        o["tau"] = 1.0 if method == "ALG2" else 1.9                       # :133-137
    o.setdefault("sigma", 1.0)
    o.setdefault("time_limit", 3600)
    return o


def _weights_mode(weight, weights, transfer, weighted=True):
    """Where the levels' weights of a weighted multilevel solve are made: the `weights` argument of solver_wdotsocp2d,
    or its default -- "device" for a SpaceWeight whose state stays on the device, else "host" (today's path)."""
    if weights is None:
        weights = "device" if isinstance(weight, SpaceWeight) and transfer == "device" else "host"
    if weights not in ("device", "host"):
        raise ValueError("weights must be 'device' or 'host'")
    if weights == "device" and (transfer != "device" or not weighted):
        raise ValueError("weights='device' needs a weighted driver and transfer='device'")
    return weights


def _solve_levels(rho0, rho1, nt, levelN, opts, method, dim, weighted, device, barrier=None, transfer="device",
                  weights=None, report=False, advect=None, push=None, map_report=None, render=None, dual=False, upper=None, plan_map=None,
                  geodesic=False):
    """The level loop of solver_dotsocp2d.m:154-250 (dot1d / wdot2d twins): restrict the data to
    levelN grids, solve coarse to fine with warm starts; every solve runs on the device.
    transfer = "device": the state never leaves the GPU -- jump_nextLevel and the output recovery run there
    (dotsocp_jump_next_level / dotsocp_recover_outputs); "host": download, numpy twins of jump_nextLevel.m /
    recover_RhoE.m / recover_q.m, upload (the two agree to rounding, tests/test_multilevel.py).
    weights (weighted drivers) = "host": every level's weight is restricted with numpy (multilevel.downSample_q /
    downSample_barrier) and uploaded; "device": one WeightPyramid holds the weights of all levels -- the finest is uploaded
    once (an Nq array, or the two 2-D arrays of a SpaceWeight), the others are restricted on the GPU, every level's
    context takes its weight device to device and InitialScaling its log10 mean from the pyramid; needs
    transfer="device".  None: "device" for a SpaceWeight with transfer="device", else "host" (a SpaceWeight is then
    expanded on the host).
    report = True: the last level's context is asked for its solution report (InPALMContext.report(), report.py) before it
    is closed; output["report"] holds it.  Needs transfer="device".
    geodesic = True: the last level's context is asked for the geodesic's profile (InPALMContext.geodesic(), geodesic.py) in
    the same way; output["geodesic"] holds it.  Needs transfer="device".
    advect = dict(x=..., y=..., nsub=..., direction=..., rho_floor=..., trajectories=...): the keyword arguments of
    InPALMContext.advect(), which is asked of the last level's context in the same way; output["advect"] holds its
    result.  Needs transfer="device".
    push = dict(stride=..., frames=..., nsub=..., direction=..., rho_floor=...): the keyword arguments of
    InPALMContext.push_from_nodes() -- the given density carried along the solved flow and deposited at the frame nodes --
    asked of the last level's context; output["push"] holds its result.  Needs transfer="device".
    map_report = dict(stride=..., nsub=..., direction=..., rho_floor=...): the keyword arguments of
    InPALMContext.map_report_from_nodes() -- what the map realised by the flow costs and how straight and steady its paths
    are -- asked of the last level's context; output["map_report"] holds its result.  Needs transfer="device".
    dual = True: the last level's context is asked for the dual lower bound on W2^2 (InPALMContext.dual_bound(), dual.py);
    output["dual"] holds it.  Needs transfer="device"; a weighted context refuses (capi.DotsocpError).
    upper = dict(eps_h2=..., max_sweeps=..., defect_tol=...): the keyword arguments of InPALMContext.upper_bound() -- the
    upper end of the bracket around W2^2 -- asked of the last level's context; output["upper"] holds its result.  Needs
    transfer="device"; a weighted context refuses.
    plan_map = dict(eps_h2=..., max_sweeps=..., frames=..., compare=dict(stride=..., nsub=...)): the keyword arguments of
    InPALMContext.plan_map() -- the static transport map of the rounded plan, its frames and its distance from the flow's
    own map -- asked of the last level's context; output["plan_map"] holds its result.  Needs transfer="device"; a weighted
    context refuses."""
    from . import multilevel as ML
    from .examples import ensure_barrier_validity
    if not (isinstance(levelN, (int, np.integer)) and levelN >= 1):
        raise ValueError("Invalid input at position 4 (Number of levels in multilevel strategy)")
    if transfer not in ("device", "host"):
        raise ValueError("transfer must be 'device' or 'host'")
    if report and transfer != "device":
        raise ValueError("report=True needs transfer='device' (the report is taken from the device-resident state)")
    if geodesic and transfer != "device":
        raise ValueError("geodesic=True needs transfer='device' (the profile is taken from the device-resident state)")
    if advect is not None and transfer != "device":
        raise ValueError("advect= needs transfer='device' (the particles move through the device-resident state)")
    if push is not None and transfer != "device":
        raise ValueError("push= needs transfer='device' (the mass moves through the device-resident state)")
    if map_report is not None and transfer != "device":
        raise ValueError("map_report= needs transfer='device' (the particles move through the device-resident state)")
    if dual and transfer != "device":
        raise ValueError("dual=True needs transfer='device' (the bound is taken from the device-resident potential)")
    if upper is not None and transfer != "device":
        raise ValueError("upper= needs transfer='device' (the sweeps start from the device-resident potential)")
    if plan_map is not None and transfer != "device":
        raise ValueError("plan_map= needs transfer='device' (the sweeps start from the device-resident potential)")
    if render is not None and transfer != "device":
        raise ValueError("render= needs transfer='device' (the pictures are made from the device-resident state)")
    wopt = _get(opts, "weight") if weighted else None
    weights = _weights_mode(wopt, weights, transfer, weighted)
    wdev = weights == "device"
    if isinstance(wopt, SpaceWeight) and not wdev:
        wopt = wopt.expand(nt)
    o = _driver_opts(opts, method, weighted, dim)
    t_all = time.perf_counter()
    tolFactor = -1.0 if o["tol"] > 0.99e-3 else -0.5                     # :124-128
    tolLB = 1e-4 if dim == 2 else 1e-5                                   # :130, solver_dotsocp1d.m:121
    L = int(levelN)
    rho0s, rho1s, nts, tols, ws = [None] * L, [None] * L, [None] * L, [None] * L, [None] * L
    rho0s[-1], rho1s[-1] = np.asarray(rho0, dtype=np.float64), np.asarray(rho1, dtype=np.float64)
    nts[-1], tols[-1] = int(nt), o["tol"]
    if weighted and not wdev:
        ws[-1] = np.asarray(wopt, dtype=np.float64)
    for lv in range(L - 2, -1, -1):                                      # :166-178
        if (nts[lv + 1] - 1) % 2 or any((n - 1) % 2 for n in rho0s[lv + 1].shape):
            raise ValueError("multilevel needs 2^k*m+1 grid sizes on every level (solver_dotsocp2d.m:167)")
        nts[lv] = (nts[lv + 1] - 1) // 2 + 1
        tols[lv] = max(tols[lv + 1] * 2 ** tolFactor, tolLB)
        rho0s[lv], rho1s[lv] = ML.downSample_phi(rho0s[lv + 1]), ML.downSample_phi(rho1s[lv + 1])
        if weighted:
            nyf, nxf = rho0s[lv + 1].shape
            if barrier is not None:                                      # solver_wdotsocp2d.m:186-189
                rho0s[lv], rho1s[lv], _ = ensure_barrier_validity(rho0s[lv], rho1s[lv], barrier)
                if not wdev:
                    ws[lv] = ML.downSample_barrier(nts[lv + 1], nxf, nyf, ws[lv + 1])
                continue
            if not wdev:
                ws[lv] = ML.downSample_q(nts[lv + 1], nxf, nyf, ws[lv + 1])
        N = rho0s[lv].size
        rho0s[lv] = rho0s[lv] / (rho0s[lv].sum() / N)
        rho1s[lv] = rho1s[lv] / (rho1s[lv].sum() / N)
    on_device = transfer == "device"
    # opts.ngpu (extension, as in the MEX gateway): every level is cut into time slabs on that many devices of this one
    # process (a level with few time nodes gets fewer slabs: at least two nodes per slab)
    ngpu = int(_get(opts, "ngpu", 1) or 1)
    var, model = initialize(rho0s[0], rho1s[0], nts[0], lazy_zeros=on_device)
    timeML, runHistML, runHist, last = [], None, None, None
    ctx = prev = pyr = None

    def level_weight(model, lv):
        if wdev:                          # no Nq host array: InitialScaling reads the mean, the context the pyramid level
            model.weight_log10_mean = pyr.log10_mean(lv)
        elif weighted:
            model.weight = ws[lv]

    try:
        if wdev:
            pyr = WeightPyramid(rho0s[-1].shape[0], rho0s[-1].shape[1], nts[-1], L, device=device)
            pyr.set(wopt)
            pyr.restrict(log_mean=barrier is not None)                   # solver_wdotsocp2d.m:186-191
        level_weight(model, 0)
        for lv in range(L):
            InitialScaling(var, model, o["scaling"], last, dim=dim, weighted=weighted)
            ctx = InPALMContext(var, dict(o, tol=tols[lv]), model, weighted=weighted, device=device, method=method,
                                warm_from=prev, ngpu=max(1, min(ngpu, nts[lv] // 2)),
                                weight_from=(pyr, lv) if wdev else None)
            if wdev and lv == L - 1:
                pyr.close()                                              # the last level has its weight
            if prev is not None:
                prev.close()
                prev = None
            ctx.run(-1)
            last_level = lv == L - 1
            runHist, sigma = ctx.finish(download=not on_device)
            timeML.append(var.time)
            if runHistML is None:                                        # catRunHist, :389-407
                runHistML = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in runHist.items()}
            else:
                runHist["time"] = runHistML["time"][-1] + runHist["time"]
                runHistML["kkt"] = np.concatenate([runHistML["kkt"], runHist["kkt"]], axis=0)
                runHistML["pdGap"] = np.concatenate([runHistML["pdGap"], runHist["pdGap"]])
                runHistML["time"] = np.concatenate([runHistML["time"], runHist["time"]])
                runHistML["iter"] = np.concatenate([runHistML["iter"], runHistML["iter"][-1] + runHist["iter"]])
                runHistML["len"] = runHistML["len"] + runHist["len"]
            if on_device and last_level:
                output = ctx.outputs()
                if report:
                    output["report"] = ctx.report()
                if geodesic:
                    output["geodesic"] = ctx.geodesic()
                if dual:
                    output["dual"] = ctx.dual_bound()
                if upper is not None:
                    output["upper"] = ctx.upper_bound(**upper)
                if plan_map is not None:
                    output["plan_map"] = ctx.plan_map(**plan_map)
                if advect is not None:
                    output["advect"] = ctx.advect(**advect)
                if push is not None:
                    output["push"] = ctx.push_from_nodes(**push)
                if map_report is not None:
                    output["map_report"] = ctx.map_report_from_nodes(**map_report)
                if render is not None:
                    asked = [render] if isinstance(render, dict) else list(render)
                    made = [ctx.render(**(dict(r) if barrier is None else dict(dict(barrier=barrier), **r))) for r in asked]
                    output["render"] = made[0] if isinstance(render, dict) else made
            if not on_device:
                ctx.close()
                recoverOrgVar(var)
            if not last_level:
                o["time_limit"] = o["time_limit"] - var.time["Total_Time"]   # :244
                o["sigma"] = 10 ** (np.log10(o["sigma"] * sigma) / 2)         # :245
                last = runHist["kkt"][-1]
                wf = ws[lv + 1] if weighted else None
                if on_device:
                    E2 = var.E2
                    var, model = initialize(rho0s[lv + 1], rho1s[lv + 1], nts[lv + 1], lazy_zeros=True, phi=False)
                    var.E2 = E2                         # the state comes from the coarse level on the device
                    level_weight(model, lv + 1)
                    prev = ctx
                else:
                    var, model = ML.jump_nextLevel(var, model, rho0s[lv + 1], rho1s[lv + 1], nts[lv + 1], wf)
        if not on_device:
            rho_E = recover_RhoE(var, model, weighted=weighted)
            qs = recover_q(var, model)
            if dim == 2:
                output = dict(rho=rho_E[0], Ex=rho_E[1], Ey=rho_E[2], q0=qs[0], bx=qs[1], by=qs[2])
            else:
                output = dict(rho=rho_E[0], Ex=rho_E[1], q0=qs[0], bx=qs[1])
    finally:
        for c in (ctx, prev, pyr):
            if c is not None:
                c.close()
    timeML.append({"ML_Time": time.perf_counter() - t_all})
    name = ("Weighted-" if weighted else "") + "DOT-SOCP"
    mname = (f"{method} for {name}") if L == 1 else (f"Multilevel-{method} for {name}")
    runHist["method"] = runHistML["method"] = mname
    return output, timeML, runHistML, runHist


def solver_dotsocp2d(rho0, rho1, nt, levelN, opts, method="inPALM", device=0, transfer="device", report=False,
                     advect=None, push=None, map_report=None, render=None, dual=False, upper=None, plan_map=None,
                     geodesic=False):
    """[output, timeML, runHistML, runHist] = solver_dotsocp2d(rho0, rho1, nt, levelN, opts, method)
    socp/dot2d/solver_dotsocp2d.m:1.  report=True: output["report"] = the device-side solution report; advect=dict(x=..., y=...,
    ...): output["advect"] = the particles carried along the solved flow; push=dict(stride=..., frames=..., ...):
    output["push"] = the given density carried along it and deposited at the frame nodes; map_report=dict(stride=..., ...):
    output["map_report"] = cost, straightness and steadiness of the map the flow realises; render=dict(num_frame=..., mode=...,
    arrows=..., ...): output["render"] = uint8 pictures of the density evolution and the arrows of the flux; dual=True:
    output["dual"] = the dual lower bound on W2^2 from the potential; upper=dict(eps_h2=..., max_sweeps=..., defect_tol=...):
    output["upper"] = the upper bound on it from Sinkhorn sweeps rounded to a plan; geodesic=True: output["geodesic"] = the
    profile of the solution per time node (energy, moments, entropy; geodesic.py) (all of them: _solve_levels)."""
    output, timeML, runHistML, runHist = _solve_levels(rho0, rho1, nt, levelN, opts, method, 2, False, device,
                                                       transfer=transfer, report=report, advect=advect, push=push, map_report=map_report,
                                                       render=render, dual=dual, upper=upper, plan_map=plan_map, geodesic=geodesic)
    if not check_massConservation(output["rho"], 1e-2):
        print("Warning: The mass conservation constraint violation exceeds 0.01")
    return output, timeML, runHistML, runHist


def solver_dotsocp1d(rho0, rho1, nt, levelN, opts, method="inPALM", device=0, transfer="device", report=False,
                     advect=None, push=None, map_report=None, render=None, dual=False, upper=None, plan_map=None,
                     geodesic=False):
    """socp/dot1d/solver_dotsocp1d.m:1.  report, advect, push, map_report, render, dual, upper, geodesic: as for solver_dotsocp2d."""
    output, timeML, runHistML, runHist = _solve_levels(rho0, rho1, nt, levelN, opts, method, 1, False, device,
                                                       transfer=transfer, report=report, advect=advect, push=push, map_report=map_report,
                                                       render=render, dual=dual, upper=upper, plan_map=plan_map, geodesic=geodesic)
    if not check_massConservation(output["rho"], 1e-2):
        print("Warning: The mass conservation constraint violation exceeds 0.01")
    return output, timeML, runHistML, runHist


def solver_wdotsocp2d(rho0, rho1, nt, levelN, opts, method="inPALM", barrier=None, device=0, transfer="device",
                      weights=None, report=False, advect=None, push=None, map_report=None, render=None, dual=False, upper=None, plan_map=None,
                      geodesic=False):
    """socp/wdot2d/solver_wdotsocp2d.m:1.  opts["weight"]: the Nq array, or a SpaceWeight (examples.py); weights:
    where the levels' weights are made, "host" or "device" (_solve_levels); report, geodesic, advect, push, map_report, render: as for
    solver_dotsocp2d (render: `barrier` is the default mask of the pictures; dual=True and upper= raise the library's refusal:
    the weighted cost is not the Euclidean one)."""
    output, timeML, runHistML, runHist = _solve_levels(rho0, rho1, nt, levelN, opts, method, 2, True, device,
                                                       barrier=barrier, transfer=transfer, weights=weights, report=report,
                                                       advect=advect, push=push, map_report=map_report, render=render, dual=dual, upper=upper, plan_map=plan_map, geodesic=geodesic)
    if not check_massConservation(output["rho"], 1e-2):
        print("Warning: The tolerance of mass conservation constraint is under 0.01")
    return output, timeML, runHistML, runHist


def poisson_on_slabs(rhs, D, nslabs=1, ngpu=None, dim=2, device=0, repeat=None):
    """Test support: idctn(dctn(rhs) ./ (D^2 * initialize_FFTkernel)) by the loop's own Poisson solve
    (dotsocp_poisson_phi: Solver::poisson_all) on a context cut into `nslabs` time slabs on one device, or `ngpu` slabs
    with their own streams (dotsocp_create_multi).  rhs: (ny, nx, nt) Fortran array; dim=1: the 1-D grid nx1d x nt as
    (nx1d, 1, nt).  The context is built from the shape and D alone -- no densities.
    Two arguments beyond that: `device`, the HIP device (ngpu: the first one); and `repeat`, a list of further
    right-hand sides of the same shape solved one after the other on the SAME context (the mode probes solve several
    bands per layout and would otherwise create the slabs once per band).  Without `repeat` the result is the solved
    array; WITH it the return type changes: a list, [solution of rhs] + [solutions of repeat], in that order."""
    L = capi.lib()
    rhs = np.asfortranarray(rhs, dtype=np.float64)
    if rhs.ndim != 3 or (dim == 1 and rhs.shape[1] != 1) or dim not in (1, 2):
        raise ValueError("rhs must be an (ny, nx, nt) array (dim=1: (nx1d, 1, nt))")
    ny, nx, nt = rhs.shape
    p = capi.Problem()
    p.dim, p.weighted = int(dim), 0
    p.ny, p.nx, p.nt = (1, ny, nt) if dim == 1 else (ny, nx, nt)
    p.D, p.E, p.cScale, p.dScale, p.normc, p.normd = float(D), 1.0, 1.0, 1.0, 1.0, 1.0
    if ngpu is not None and int(ngpu) > 1:
        ctx = L.dotsocp_create_multi(ctypes.byref(p), int(device), int(ngpu))
    else:
        ctx = L.dotsocp_create(ctypes.byref(p), int(device), int(nslabs))
    if not ctx:
        raise capi.DotsocpError(-1, L.dotsocp_last_error().decode())
    try:
        out = []
        for r in [rhs] + [np.asfortranarray(a, dtype=np.float64) for a in (repeat or [])]:
            if r.shape != rhs.shape:
                raise ValueError("every right-hand side must have the shape of the first")
            res = np.empty(rhs.shape, dtype=np.float64, order="F")
            capi.check(L.dotsocp_upload(ctx, capi.F_PHI, capi.fptr(r)))
            capi.check(L.dotsocp_poisson_phi(ctx))
            capi.check(L.dotsocp_download(ctx, capi.F_PHI, capi.fptr(res)))
            out.append(res)
    finally:
        L.dotsocp_destroy(ctx)
    return out[0] if repeat is None else out
