"""The multilevel transfer (dotsocp_jump_next_level: Solver::jump_from, k_prolong_phi, k_prolong_beta, k_scale_div) and the
output kernels (k_outputs, k_out_tail) on GENERIC states against the oracle, isolated from the loop.

The end-to-end multilevel tests start from the all-zero state on square grids and look at the converged output, which the
loop reaches from any reasonable warm start.  Here the coarse level is a free-running device loop from the generic start
of oracle/generic_state.py; its finished state is downloaded, and

(1) the oracle alone takes copies of those arrays through recoverOrgVar, jump_nextLevel and InitialScaling
    (oracle/transfer_state.expected), while the device jumps from the still open coarse context into a fine context that
    was created through the C API and never begun.  Both start from the same bits, so what is compared is the transfer
    and nothing else: the scale factors to 1e-15, z == 0, beta == 0 in the slots mexBFd leaves unwritten (asserted on the
    oracle first), and phi, q, alpha, beta within c u M, u = 2^-53 -- c counts the roundings of the two chains and M is
    the magnitude they act on; the derivation is the module docstring of oracle/transfer_state.py, and
    tests/test_transfer_conditions.py shows on the CPU that wrong transfers miss these bounds by >= 1e3.
    Cases: 66x10x6 -> 131x19x11 (non-square, both levels pitched, tile remainders in y and x), 1-D 150x7 -> 299x13,
    1e6 barrier weights, 128x32x5 -> 255x63x9 (cone columns Nz + 48 apart on both levels, coarse rows unpitched, fine rows
    pitched), 3x2x2 -> 5x3x3, and 40x12x13 -> 79x23x25 on time slabs: 1 -> 1, 1 -> 3 (a pitched coarse level feeding an
    unpitched fine one), 2 -> 3, 3 -> 2 and, because in none of these a fine slab STARTS at a node whose coarse
    neighbours tc, tc + 1 lie in different coarse slabs (the slab ranges are asserted), 2 -> 2 and 3 -> 3, where one does.
    Time slabs change no bit: every split gives the bits of one slab -> one slab.  For that comparison the coarse slabs
    must hold the same state, and free-running loops on different splits do not; a `carrier` holds the downloaded state of
    the one-slab run on any split (begin with sigma = 1 and no iteration, then finish: alpha and beta are uploaded
    already times sigma, and a product with 1.0 is exact).  This comparison found alpha on the first edge layer of every
    non-first fine slab one bit off in a quarter of its entries -- the left neighbour's share of the adjoint sum entered
    as one term -- and is the regression test of k_conj_first_layer (csrc/transfer.hip), which sums in one slab's order.
(2) the fine loop's first 7 iterations after the jump (begin() exchanges the halos of q and phi) against the oracle's loop
    from the oracle's own transfer, with the assertions of tests/test_gpu_generic_state.py; the field tolerance is 100 x
    the oracle's one-ulp sensitivity (oracle/transfer_state.WARM_SENSITIVITY).  KKT column 5 is rounding noise after a
    jump (WARM_CANCELLING) and held below 1e-13 on both sides.
(3) the guard bands: the jump and outputs() between NaN bands (DOTSOCP_CANARY=1), no band touched, same bits.
(4) outputs() of the finished coarse contexts against recover_RhoE of the oracle, and q0 / bx / by against plain loops
    written from the definition (include/dotsocp.h, csrc/transfer.hip: the x resp. y mean of the two edges around a
    node, 0 on the boundary, then the mean of the two node layers of a cell).  Roundings per side: a = [w *] (cD (sigma
    alpha)) has the product with sigma, the factor cD, its product [and the weight's]: 3 [4]; rho and Ex / Ey add one
    sum (the halving and the doubling on the end layers are exact): c = 8 [10] against max|a| (2 max|a| for the doubled
    layers of Ex / Ey) -- the size of the terms, not of a sum that may cancel.  b = dD q: the factor and its product, 2:
    q0 c = 4; bx / by add two sums: c = 8, against max|b|.  Boundary entries are exactly 0.

Measured errors are recorded in DESIGN.md (section 5, "The multilevel transfer on generic states")."""
import ctypes

import numpy as np
import pytest

import dotsocp_amd as D
from dotsocp_amd import capi
from oracle import driver as OD
from oracle import generic_state as G
from oracle import transfer_state as T

pytestmark = pytest.mark.gpu
FOUR = ("phi", "q", "alpha", "beta")
FIELD_IDS = {"phi": capi.F_PHI, "q": capi.F_Q, "z": capi.F_Z, "alpha": capi.F_ALPHA, "beta": capi.F_BETA}
SWITCHES = ("DOTSOCP_QCONE", "DOTSOCP_QCONE_TC", "DOTSOCP_FUSED", "DOTSOCP_CONE_CARRY", "DOTSOCP_C_ENDS", "DOTSOCP_QTX",
            "DOTSOCP_NT", "DOTSOCP_KKT_FOLD", "DOTSOCP_CANARY")
SLAB_CASE = "40x12x13"


def _split_kw(split):
    """"nslabs=3" -> dict(nslabs=3); None -> one slab"""
    if not split:
        return {}
    kind, n = split.split("=")
    return {kind: int(n)}


def _world(split):
    return int(split.split("=")[1]) if split else 1


def _create(p, split):
    L = capi.lib()
    kw = _split_kw(split)
    ctx = (L.dotsocp_create_multi(ctypes.byref(p), 0, kw["ngpu"]) if "ngpu" in kw
           else L.dotsocp_create(ctypes.byref(p), 0, kw.get("nslabs", 1)))
    if not ctx:
        raise capi.DotsocpError(-1, L.dotsocp_last_error().decode())
    return ctx


def _problem(shape, weighted, scal, normc=1.0, normd=1.0):
    p = capi.Problem()
    one_d = len(shape) == 2
    p.dim, p.weighted = (1 if one_d else 2), (1 if weighted else 0)
    p.ny, p.nx, p.nt = (1, shape[0], shape[1]) if one_d else shape
    p.D, p.E, p.cScale, p.dScale = scal["D"], scal["E"], scal["cScale"], scal["dScale"]
    p.normc, p.normd = float(normc), float(normd)
    return p


class _Coarse:
    """A finished coarse level on the device, context open: the free-running loop of the case from the generic start,
    built as tests/test_gpu_generic_state.py::_gpu_run builds it."""

    def __init__(self, monkeypatch, name, split=None, env=None):
        for sw in SWITCHES:
            monkeypatch.delenv(sw, raising=False)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        spec = T.spec(name)
        rho0, rho1, nt, weight = T.coarse_problem(name)
        var, model = D.initialize(rho0, rho1, nt)
        if weight is not None:
            model.weight = np.asarray(weight, dtype=np.float64)
        o = OD.default_opts(dict(tol=0.0, maxit=spec["K"]), spec["method"], weight is not None)
        D.InitialScaling(var, model, o["scaling"], None, dim=len(spec["shape"]) - 1, weighted=weight is not None)
        G.set_state(var, T.coarse_start(name, var))
        self.name, self.var, self.model, self.weight = name, var, model, weight
        self.ctx = D.InPALMContext(var, o, model, weighted=weight is not None, method=spec["method"], **_split_kw(split))
        try:
            self.ctx.run(-1)
            self.hist, self.sigma = self.ctx.finish(download=True)
        except Exception:
            self.ctx.close()
            raise
        self.fields, self.scalars = T.finished(var)
        self.handle = self.ctx._ctx

    def close(self):
        self.ctx.close()


class _Carrier:
    """The downloaded state of a finished level on any split, finished without an iteration (module docstring)."""

    def __init__(self, src, split):
        L = capi.lib()
        shape = T.spec(src.name)["shape"]
        self.handle = _create(_problem(shape, False, src.scalars), split)
        try:
            for f, a in src.fields.items():
                capi.check(L.dotsocp_upload(self.handle, FIELD_IDS[f], capi.fptr(np.asfortranarray(a))))
            o = capi.Opts()
            o.tau, o.sigma, o.tol, o.maxit = 1.9, 1.0, 0.0, 0
            o.ifCheckStepByStep, o.checkPrimDualFeas, o.scaling, o.time_limit = 0, -1, 1, 3600.0
            capi.check(L.dotsocp_begin(self.handle, ctypes.byref(o)))
            res = capi.Result()
            capi.check(L.dotsocp_finish(self.handle, ctypes.byref(res)))
            assert res.sigma == 1.0 and res.cScale == src.scalars["cScale"] and res.dScale == src.scalars["dScale"]
        except Exception:
            self.close()
            raise

    def close(self):
        if self.handle:
            capi.lib().dotsocp_destroy(self.handle)
            self.handle = None


def _fine_level(name, coarse):
    """The fine level as solvers.py builds it between two levels: no state on the host, E2 carried over."""
    rho0, rho1, nt, weight = T.fine_problem(name)
    var, model = D.initialize(rho0, rho1, nt, lazy_zeros=True, phi=False)
    var.E2 = coarse.scalars["E2"]
    if weight is not None:
        model.weight = np.asarray(weight, dtype=np.float64)
    D.InitialScaling(var, model, True, coarse.hist["kkt"][-1], dim=len(T.fine_shape(name)) - 1, weighted=weight is not None)
    return var, model, weight


def _jump(name, coarse, handle, split=None, like=None, check_canary=False):
    """dotsocp_jump_next_level from the coarse context `handle` into a fresh fine context on `split`, never begun:
    the five downloaded fields and the fine level's scalars."""
    L = capi.lib()
    var, model, weight = _fine_level(name, coarse)
    scal = {k: float(getattr(var, k)) for k in ("cScale", "dScale", "D", "E")}
    fine = _create(_problem(T.fine_shape(name), weight is not None, scal, model.normc, model.normd), split)
    try:
        capi.check(L.dotsocp_upload(fine, capi.F_C, capi.fptr(np.ascontiguousarray(model.c))))
        if weight is not None:
            capi.check(L.dotsocp_upload(fine, capi.F_WEIGHT, capi.fptr(np.ascontiguousarray(model.weight))))
        capi.check(L.dotsocp_jump_next_level(handle, fine))
        if check_canary:
            assert L.dotsocp_canary_check() == 0, L.dotsocp_last_error().decode()
        got = {}
        for f in G.FIELDS:
            got[f] = np.full(like[f].shape, np.nan, order="F")
            capi.check(L.dotsocp_download(fine, FIELD_IDS[f], capi.fptr(got[f])))
    finally:
        L.dotsocp_destroy(fine)
    return got, scal


def _oracle(name, coarse):
    var, model, raw = T.expected(name, coarse.fields, coarse.scalars, coarse.hist["kkt"][-1])
    return var, model, raw, {f: getattr(var, f) for f in G.FIELDS}


def _against_the_oracle(name, tag, coarse, got, scal, ovar, raw):
    weight = T.fine_problem(name)[3]
    # --- the scale factors of the two sides, and what they differ by in units of u
    slack = 0.0
    for k in ("D", "E", "cScale", "dScale"):
        rel = abs(scal[k] - getattr(ovar, k)) / abs(getattr(ovar, k))
        assert rel <= 1e-15, (k, scal[k], getattr(ovar, k))
        slack += rel / T.U
    # --- z, and the holes of beta (the oracle's first)
    hole = T.holes(ovar.beta.shape, T.fine_shape(name))
    assert np.all(ovar.beta[hole] == 0.0) and np.all(ovar.beta[~hole] != 0.0)
    assert np.all(got["beta"][hole] == 0.0)
    assert np.all(got["z"] == 0.0) and np.all(ovar.z == 0.0)
    # --- the four fields
    bounds = T.bounds(name, ovar, raw, weight, scale_slack=slack)
    kap = T.kappa(name, ovar, bounds, weight)
    share, in_u = {}, {}
    for f in FOUR:
        assert got[f].shape == getattr(ovar, f).shape and np.all(np.isfinite(got[f])), f
        err = got[f] - getattr(ovar, f)
        share[f] = T.worst(err, bounds[f])
        in_u[f] = np.max(np.abs(err)) / (T.U * np.max(np.abs(getattr(ovar, f))))
    print("\n%s [%s]: max|device - oracle| in u max|field|  %s ; as a share of the bound  %s ; kappa_q %.1f kappa_alpha %.2f, "
          "scale factors differ by %.1f u" % (name, tag, "  ".join("%s %.2f" % kv for kv in in_u.items()),
                                           "  ".join("%s %.3f" % kv for kv in share.items()), kap["q"], kap["alpha"], slack))
    assert max(share.values()) <= 1.0, share


def _same_bits(a, b):
    for f in G.FIELDS:
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)


# --------------------------------------------------------------------------------------------------
# (1) the transfer against the oracle
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["66x10x6", "1d-150x7", "weighted-66x10x6", "128x32x5", "3x2x2"])
def test_the_transfer_against_the_oracle(name, monkeypatch):
    coarse = _Coarse(monkeypatch, name)
    try:
        ovar, _, raw, like = _oracle(name, coarse)
        got, scal = _jump(name, coarse, coarse.handle, like=like)
    finally:
        coarse.close()
    _against_the_oracle(name, "one slab", coarse, got, scal, ovar, raw)


def _ranges(nt, split):
    w = _world(split)
    return [capi.slab_range(nt, w, r) for r in range(w)]


def _owner(ranges, t):
    return [i for i, (a, b) in enumerate(ranges) if a <= t < b][0]


# coarse split, fine split, and whether a fine slab must START between two coarse slabs
SPLITS = [(None, None, False), (None, "nslabs=3", False), (None, "ngpu=3", False), ("nslabs=2", "ngpu=3", False),
          ("ngpu=2", "nslabs=3", False), ("ngpu=3", "nslabs=2", False), ("nslabs=3", "ngpu=2", False),
          ("nslabs=2", "ngpu=2", True), ("ngpu=3", "nslabs=3", True)]
_one_slab = {}


def _one_slab_state(monkeypatch):
    """The finished one-slab coarse run of the slab case and its one slab -> one slab transfer (once; read-only)."""
    if not _one_slab:
        coarse = _Coarse(monkeypatch, SLAB_CASE)
        try:
            ovar, _, raw, like = _oracle(SLAB_CASE, coarse)
            got, scal = _jump(SLAB_CASE, coarse, coarse.handle, like=like)
        finally:
            coarse.close()
        _one_slab.update(coarse=coarse, ovar=ovar, raw=raw, like=like, got=got, scal=scal)
    return _one_slab


@pytest.mark.parametrize("csplit,fsplit,starts_between", SPLITS)
def test_the_transfer_on_time_slabs(csplit, fsplit, starts_between, monkeypatch):
    name = SLAB_CASE
    ntc, ntf = T.spec(name)["shape"][-1], T.fine_shape(name)[-1]
    cr, fr = _ranges(ntc, csplit), _ranges(ntf, fsplit)
    # --- what the split covers, from the slab bounds
    odd_starts = [a for a, _ in fr if a & 1]
    if len(fr) > 1:
        assert odd_starts                                     # a slab whose first node needs the coarse nodes tc and tc + 1
    if len(cr) > 1:
        # some odd fine node reads its two coarse nodes from two coarse slabs: the gather assembles w0 from both owners
        assert any(_owner(cr, t >> 1) != _owner(cr, (t >> 1) + 1) for t in range(1, ntf, 2))
    if starts_between:
        assert any(_owner(cr, a >> 1) != _owner(cr, (a >> 1) + 1) for a in odd_starts)
    if csplit is None and fsplit is not None:
        nyc, nyf = T.spec(name)["shape"][0], T.fine_shape(name)[0]
        assert nyc > 16 and nyc % 16 != 0 and nyf % 16 != 0   # the one coarse slab pitches its rows, fine slabs never do
    one = _one_slab_state(monkeypatch)
    tag = "%s -> %s" % (csplit or "one slab", fsplit or "one slab")
    # --- against the oracle: the free-running coarse loop on this split (one slab: the closed run's state in a carrier)
    if csplit is None:
        coarse, src = one["coarse"], _Carrier(one["coarse"], None)
    else:
        coarse = src = _Coarse(monkeypatch, name, csplit)
    try:
        ovar, _, raw, like = _oracle(name, coarse)
        got, scal = _jump(name, coarse, src.handle, fsplit, like=like)
    finally:
        src.close()
    _against_the_oracle(name, tag, coarse, got, scal, ovar, raw)
    # --- the same state on this split: the bits of one slab -> one slab
    carrier = _Carrier(one["coarse"], csplit)
    try:
        again, scal2 = _jump(name, one["coarse"], carrier.handle, fsplit, like=one["like"])
    finally:
        carrier.close()
    assert scal2 == one["scal"]
    _same_bits(again, one["got"])


# --------------------------------------------------------------------------------------------------
# (2) the warm start
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,csplit,fsplit", [("66x10x6", None, None), (SLAB_CASE, "nslabs=2", "ngpu=3"),
                                                (SLAB_CASE, "ngpu=2", "nslabs=3")])
def test_the_fine_loop_from_the_transferred_state(name, csplit, fsplit, monkeypatch):
    spec = T.spec(name)
    coarse = _Coarse(monkeypatch, name, csplit)
    try:
        var, model, weight = _fine_level(name, coarse)
        o = T.warm_opts(name, coarse.sigma)
        fine = D.InPALMContext(var, o, model, weighted=weight is not None, method=spec["method"], warm_from=coarse.ctx,
                               **_split_kw(fsplit))
        try:
            fine.run(-1)
            hist, sigma = fine.finish(download=False)
            ovar, ohist, osigma = T.warm_run(name, coarse.fields, coarse.scalars, coarse.hist["kkt"][-1], coarse.sigma)
            got = {f: fine.download(FIELD_IDS[f], getattr(ovar, f)) for f in G.FIELDS}
        finally:
            fine.close()
    finally:
        coarse.close()
    errs = {f: np.max(np.abs(got[f] - getattr(ovar, f))) / np.max(np.abs(getattr(ovar, f))) for f in G.FIELDS}
    generic = [c for c in range(7) if c not in T.WARM_CANCELLING]
    same_len = hist["len"] == ohist["len"]
    kerr = np.max((np.abs(hist["kkt"] - ohist["kkt"]) / ohist["kkt"])[:, generic]) if same_len else np.nan
    print("\n%s [%s -> %s]: %d fine iterations, errors against the oracle  %s  kkt %.1e  (bound %.1e)"
          % (name, csplit or "one slab", fsplit or "one slab", T.WARM_K, "  ".join("%s %.1e" % kv for kv in errs.items()), kerr,
             100 * T.WARM_SENSITIVITY))
    assert same_len
    np.testing.assert_array_equal(hist["iter"], ohist["iter"])
    np.testing.assert_array_equal(hist["iter"], [1, 4, 7])
    assert abs(sigma - osigma) <= 1e-12 * abs(osigma)
    assert abs(var.cScale - ovar.cScale) <= 1e-12 * ovar.cScale and abs(var.dScale - ovar.dScale) <= 1e-12 * ovar.dScale
    np.testing.assert_allclose(hist["kkt"][:, generic], ohist["kkt"][:, generic], rtol=1e-8, atol=0)
    for c in T.WARM_CANCELLING:
        assert np.all(np.abs(hist["kkt"][:, c]) <= T.NOISE) and np.all(ohist["kkt"][:, c] <= T.NOISE)
    np.testing.assert_allclose(hist["pdGap"], ohist["pdGap"], rtol=1e-8, atol=0)
    assert max(errs.values()) <= 100 * T.WARM_SENSITIVITY, errs


# --------------------------------------------------------------------------------------------------
# (4) the outputs  (helpers first: (3) uses them)
# --------------------------------------------------------------------------------------------------
def _q_means(q, shape):
    """q0, bx[, by] at the cells, index by index from the definition: the mean of the two x (y) edges around a node,
    0 on the boundary, then the mean of the cell's two node layers."""
    one_d = len(shape) == 2
    ny, nx, nt = (shape[0], 1, shape[1]) if one_d else shape
    ncell = ny * nx * (nt - 1)
    q0 = q[:ncell].reshape((ny, nx, nt - 1), order="F").copy(order="F")
    # the first space axis of a 1-D problem is its x
    e0 = q[ncell:ncell + (ny - 1) * nx * nt].reshape((ny - 1, nx, nt), order="F") if one_d else \
        q[ncell + ny * (nx - 1) * nt:].reshape((ny - 1, nx, nt), order="F")
    m0 = np.zeros((ny, nx, nt - 1), order="F")
    for t in range(nt - 1):
        for x in range(nx):
            for y in range(1, ny - 1):
                lo = (e0[y - 1, x, t] + e0[y, x, t]) / 2
                hi = (e0[y - 1, x, t + 1] + e0[y, x, t + 1]) / 2
                m0[y, x, t] = (lo + hi) / 2
    if one_d:
        return dict(q0=q0[:, 0, :], bx=m0[:, 0, :])
    e1 = q[ncell:ncell + ny * (nx - 1) * nt].reshape((ny, nx - 1, nt), order="F")
    m1 = np.zeros((ny, nx, nt - 1), order="F")
    for t in range(nt - 1):
        for x in range(1, nx - 1):
            for y in range(ny):
                lo = (e1[y, x - 1, t] + e1[y, x, t]) / 2
                hi = (e1[y, x - 1, t + 1] + e1[y, x, t + 1]) / 2
                m1[y, x, t] = (lo + hi) / 2
    return dict(q0=q0, bx=m1, by=m0)


def _outputs_against_the_oracle(name, tag, coarse, outs):
    shape = T.spec(name)["shape"]
    one_d = len(shape) == 2
    weighted = coarse.weight is not None
    # the oracle's level with the downloaded iterates, recovered
    rho0, rho1, nt, _ = T.coarse_problem(name)
    from oracle.model import initialize
    ovar, omodel = initialize(rho0, rho1, nt)
    for f in G.FIELDS:
        setattr(ovar, f, coarse.fields[f].copy(order="F"))
    for k, v in coarse.scalars.items():
        setattr(ovar, k, v)
    OD.recoverOrgVar(ovar)
    if weighted:
        omodel.weight = np.asarray(coarse.weight, dtype=np.float64)
    want = dict(zip(("rho", "Ex"), OD.recover_RhoE_1d(ovar, omodel))) if one_d else \
        dict(zip(("rho", "Ex", "Ey"), OD.recover_RhoE(ovar, omodel, weighted=weighted)))
    want.update(_q_means(ovar.q, shape))
    amax = np.max(np.abs(ovar.alpha * (omodel.weight if weighted else 1.0)))
    bmax = np.max(np.abs(ovar.q))
    cw = 2 if weighted else 0
    bound = {"rho": (8 + cw) * T.U * amax, "Ex": (8 + cw) * T.U * 2 * amax, "Ey": (8 + cw) * T.U * 2 * amax,
             "q0": 4 * T.U * bmax, "bx": 8 * T.U * bmax, "by": 8 * T.U * bmax}
    assert set(outs) == set(want)
    share = {}
    for k in want:
        assert outs[k].shape == want[k].shape and np.all(np.isfinite(outs[k])), k
        share[k] = float(np.max(np.abs(outs[k] - want[k])) / bound[k])
    print("\n%s [%s]: outputs, max|device - oracle| as a share of the bound  %s"
          % (name, tag, "  ".join("%s %.3f" % kv for kv in share.items())))
    assert max(share.values()) <= 1.0, share
    # the boundary, exactly; the interior is not zero
    for k in ("Ex", "bx"):
        a = outs[k] if one_d else np.moveaxis(outs[k], 1, 0)      # the x axis first
        assert np.all(a[0] == 0.0) and np.all(a[-1] == 0.0), k
        if a.shape[0] > 2:
            assert np.all(a[1:-1] != 0.0), k
    if not one_d:
        for k in ("Ey", "by"):
            assert np.all(outs[k][0] == 0.0) and np.all(outs[k][-1] == 0.0) and np.all(outs[k][1:-1] != 0.0), k
    # the ends of the density are the given ones
    np.testing.assert_array_equal(outs["rho"][..., 0], np.asarray(rho0).reshape(outs["rho"][..., 0].shape))
    np.testing.assert_array_equal(outs["rho"][..., -1], np.asarray(rho1).reshape(outs["rho"][..., -1].shape))


@pytest.mark.parametrize("name,split", [("66x10x6", None), ("1d-150x7", None), ("weighted-66x10x6", None), ("128x32x5", None),
                                        ("3x2x2", None), (SLAB_CASE, None), (SLAB_CASE, "nslabs=2"), (SLAB_CASE, "ngpu=3")])
def test_the_outputs_against_an_independent_reference(name, split, monkeypatch):
    coarse = _Coarse(monkeypatch, name, split)
    try:
        outs = coarse.ctx.outputs()
    finally:
        coarse.close()
    _outputs_against_the_oracle(name, split or "one slab", coarse, outs)


# --------------------------------------------------------------------------------------------------
# (3) between guard bands
# --------------------------------------------------------------------------------------------------
def _jump_and_outputs(monkeypatch, name, fsplit, guarded):
    L = capi.lib()
    coarse = _Coarse(monkeypatch, name, env={"DOTSOCP_CANARY": "1"} if guarded else None)
    try:
        like = {f: np.empty(s, order="F") for f, s in _fine_shapes(name).items()}
        got, _ = _jump(name, coarse, coarse.handle, fsplit, like=like, check_canary=guarded)
        outs = coarse.ctx.outputs()
        if guarded:
            assert L.dotsocp_canary_check() == 0, L.dotsocp_last_error().decode()
    finally:
        coarse.close()
    assert L.dotsocp_canary_check() == 0
    return got, outs, coarse.fields


def _fine_shapes(name):
    shape = T.fine_shape(name)
    one_d = len(shape) == 2
    nt = shape[-1]
    plane = int(np.prod(shape[:-1]))
    nq = plane * (nt - 1) + sum(plane // n * (n - 1) * nt for n in shape[:-1])
    zshape = (plane * (nt - 1), 6 if one_d else 10)
    return {"phi": (plane * nt,), "q": (nq,), "z": zshape, "alpha": (nq,), "beta": zshape}


@pytest.mark.parametrize("name,fsplit", [("66x10x6", None), (SLAB_CASE, "nslabs=3"), ("128x32x5", None), ("3x2x2", None)])
def test_the_jump_and_the_outputs_between_guard_bands(name, fsplit, monkeypatch):
    plain, pouts, pfields = _jump_and_outputs(monkeypatch, name, fsplit, False)
    guard, gouts, gfields = _jump_and_outputs(monkeypatch, name, fsplit, True)
    for f in G.FIELDS:
        assert np.all(np.isfinite(guard[f])), f
        np.testing.assert_array_equal(gfields[f], pfields[f], err_msg="coarse " + f)
    _same_bits(guard, plain)
    assert set(gouts) == set(pouts)
    for k in pouts:
        assert np.all(np.isfinite(gouts[k])), k
        np.testing.assert_array_equal(gouts[k], pouts[k], err_msg=k)
