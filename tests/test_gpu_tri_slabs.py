"""The Poisson solve of the loop on time slabs (Solver::poisson_all through dotsocp_poisson_phi), probed mode by mode.

A Poisson solution is dominated by its low modes -- the highest (ky, kx) modes are about 1e-6 of it -- so a comparison of
whole fields at 1e-10 of their max-abs cannot see an error of 1e-6 of a high mode.  Here the right-hand side is a handful
of (ky, kx) modes, rhs = sum_j amp_j u_ky (x) v_kx (x) g_j(t) with seeded normal columns g_j, scaled so that every component
of the SOLUTION is O(1); the device result is projected back onto u_ky (x) v_kx (long-double dot products over y and x; the
other modes are orthogonal and drop out) and compared, per mode, with the literal definition of the operation along t,
    x_j = C' diag(1 / (D^2 (CY[ky] + CX[kx] + CT))) C g_j       (C: the nt x nt orthonormal DCT-II matrix, long double,
                                                                  the zero eigenvalue replaced by 1: initialize_FFTkernel)
which shares nothing with the tridiagonal algebra of tri.hip.  CY and CX are the float64 tables of initialize_FFTkernel
taken to long double (_eig_table: the numbers the operator divides by), CT the eigenvalues along t in long double.  Modes
whose amplitudes differ by more than a factor of 16 go into separate solves: otherwise the rounding of the y / x transforms
of the large components leaks into the small ones, which is the conditioning of the problem and not the kernel's doing.

Bound per mode: 1e-12 max(1, 1e-2 / a'), a' = (CY[ky] + CX[kx]) / (nt-1)^2; 1e-12 for the singular (0, 0) mode.  It comes
from the CPU model of the partitioned solve (tests/test_tri_closed_form.py) against the same long-double reference: <= 3e-14
where a' >= 1e-2 and rho^(n-1) stays normal, growing like 1 / a' below (1e-13 .. 1e-12 at a' = 1e-4), <= 1.4e-13 for the
zero-mode recurrence at nt = 512.  The shapes are the smallest grids that reach every kernel instance and regime:

  1 (130, 9, 40)    pitched rows; nslabs 1: k_tsolve_single; 2: k_tri_final_reg<32>; 3: slabs of 14 / 13 / 13 nodes,
                    k_tri_final_reg<16>, k_tri_reduced<4>; 12: k_tri_reduced<16>; 20: two-node slabs, the scratch-array
                    instance k_tri_reduced<DS_MAX_WORLD>; ngpu 2: a pair of streams per slab
  2 (66, 10, 80)    40 nodes per slab: k_tri_final_reg<64>
  3 (66, 10, 140)   70 nodes per slab: the generic k_tri_final
  4 (34, 6, 512)    2 slabs of 256 = TRI_EXTRA nodes (tiny a': no underflow); the same grid on 1 and 4 slabs
  5 (34, 6, 514)    257 nodes per slab: the solve must fall back to the slab <-> pencil transposes
  6 (2048, 1, 512)  1-D; 2 slabs: n = 256, a' up to 64, rho^255 underflows; 4 slabs: n = 128, it does not
  7 (2048, 4, 340)  n = 170, a' up to 146: underflow
  8 (2048, 4, 262)  2048^2 x 256 on two GPUs in miniature: n = 131, r = 248, rho^130 = 1e-311 (denormal)
  9 (3, 4096, 505)  ONE slab (the 4096-point axis along x: the y transform stops at 2048): pieces of 64 rows, a' up to 264, rho^63 < TRI_PW_SAFE: k_tsolve_single, which walks its
                    powers up from rho^(n-1), must not be launched (tsolve_tri_safe) -- the transform passes along t run
  10 .. 18 (66, 5, nt) on ONE slab, one shape per k_tsolve_single<R, NSUB> instance (two pitched rows per tile; the tile
                    solve is the one k_tsolve_pipe shares, tri_sweep.h): nt = 5 <8, 1> (no reduced sweep), 12 <8, 2>,
                    23 <16, 2> (pieces of 12 / 11 rows), 49 <16, 4> (13 / 12 / 12 / 12), 100 <32, 4>, 133 <34, 4>
                    (34 / 33 / 33 / 33: n == R on wave 0 only), 200 <32, 8>, 270 <34, 8>, 500 <64, 8>
  19 (514, 3, 200)  ONE slab, small but legal powers: a' up to 27, rho^24 = 1e-35
  20 (2048, 1, 505) 1-D, ONE slab: pieces of 64 / 63 rows, rho^63 = 4e-116, dotsocp_tsolve_tri_safe = 1
  21 .. 29 ONE slab, nt = 12 (k_tsolve_single<8, 2> along t): the y / x transforms of the other DCT families under the
                    pitched rows of a context (py = ny rounded up to 16 doubles), every output bin paired with its
                    eigenvalue at the highest modes: along y 21 (257, 5, 12) Rader, 22 (1000, 3, 12) Bluestein inside the
                    LDS, 23 (1025, 3, 12) prime-factor, 24 (96, 5, 12) dense product, 25 (4096, 1, 12) 1-D, the two-level
                    power of two, 26 (4101, 1, 12) 1-D, the two-level Bluestein; along x 27 (6, 257, 12), 28 (6, 1000, 12),
                    29 (6, 1025, 12)
  30 (66, 5, 64)    a power of two along t that k_tsolve_pipe does not take (it starts above 64 nodes): the fused transform
                    pass along t (k_dct_strided<2, true>: DCT-II, division, DCT-III in one kernel, rows 80 doubles apart)
  31 (66, 5, 33)    with DOTSOCP_TSOLVE=dct only: the fused prime-factor pass along t (k_pfa_strided<., 2, .>)
  32 .. 41 ONE slab, the pipelined fused transform pass along t, k_dct_tsolve_pipe<LG> (persistent workgroups, tiles of
                    L = 4096 / nt lines of one x by LDS-DMA, CY and CT in LDS, CX one scalar load per tile).  The launcher
                    takes it once the grid has two tiles per resident workgroup -- 1024 tiles on 256 CUs while two
                    workgroups fit a CU (nt <= 256), 512 beyond -- so each shape is the smallest grid of 1024 tiles,
                    4.2 M nodes (at nt = 512 and 1024 that is four tiles per workgroup: first, two steady, last).
                    test_modes_through_the_pipelined_t_pass ASSERTS the kernels named here (PIPE_KERNELS) through the
                    library's own launch decision (capi.poisson_kernels: dotsocp_tsolve_kernel, dotsocp_dct_pass_kernel)
                    before it measures.  <n>: log2 of the line length of the pipelined y / x pass.
                      32 (256, 512, 32)   LG 5, L = 128; y pass k_dct_axis0_pipe<., 8>, x pass k_dct_strided_pipe<., 9>
                      33 (256, 256, 64)   LG 6, L = 64; y and x pipelined <8>: the parity-gate grid
                      34 (256, 288, 64)   LG 6; 1152 tiles on 512 workgroups: two and three tiles (first / steady / last
                                          wait counts); y pipelined <8> (x: 288 points, the dense product)
                      35 (128, 256, 128)  LG 7, L = 32; the plane is below the k_tsolve_pipe threshold, so the transform
                                          pass runs and not the tridiagonal kernel
                      36 (128, 128, 256)  LG 8, L = 16
                      37 (64, 128, 512)   LG 9, L = 8 (one workgroup per CU: the image is 80.5 KB)
                      38 (64, 64, 1024)   LG 10, L = 4; a' down to 9e-6
                      39 (1024, 64, 64)   LG 6; y pass k_dct_axis0_pipe<., 10> on rows pitched to 1040
                      40 (64, 1024, 64)   LG 6; x pass k_dct_strided_pipe<., 10>
                      41 (4096, 1, 512)   1-D, LG 9: the two-level y transform in front of the pipelined t pass, rows
                                          pitched to 4112.  (65536, 1, 64) does NOT take the kernel: CY sits in LDS whole,
                                          which needs ny <= 12032 at nt = 64, and a 1-D grid of ny <= 8192 has 512 tiles
                                          only from nt = 256 (ny = 8192) resp. 512 (ny = 4096) on; this is the smaller ny.
                    Modes: _pipe_modes -- those of _modes and ky = L - 1, L, 2 L - 1, 2 L times kx = nx / 2 besides 0, 1,
                    nx - 1; every one is checked.  Bound per mode: max(the bound above, 4 e_cpu), e_cpu the error of the
                    same operation along t in plain float64 on the CPU (_cpu_error) against the same long-double
                    reference, computed at run time.  The right-hand sides are built band by band (_rhs_separable) and
                    projected by contracting y, then x (_project_separable).  Measured on an MI355X: e_device / e_cpu
                    0.88 .. 1.13 at the worst mode of every shape (2.3 on shape 34, at 3.9e-15); worst e_device 4.7e-15 ..
                    1.7e-14 up to nt = 128, 1.8e-13 (256), 4.0e-13 (512), 2.3e-12 (1024, at (0, 1), a' = 9e-6); worst
                    e_device / bound 0.25, at (0, 0) of shapes 38 and 41, where the float64 table CT alone puts plain
                    float64 at 1.8e-12 and 1.3e-12 -- outside the fixed 1e-12 -- and the device with it (DESIGN.md
                    section 5 has the table).
The CPU model on the pieces of shapes 10 .. 20 (the left interface as xl N_0 rho^t, the power walked up from rho^(n-1)) stays
below 1e-2 of the bound at every probed mode.

Before the backward sweeps of k_tri_final / k_tri_final_reg resumed rho^t from the last row at which it was still safely
normal (TRI_PW_SAFE), rows 6 (two slabs: 3.0e-6 at ky = 1024) and 7 (9.6e-8 at ky = 2046) missed the bound by five to six
orders of magnitude."""
import functools

import numpy as np
import pytest
import scipy.fft as sfft

import dotsocp_amd as D
from dotsocp_amd import capi

gpu = pytest.mark.gpu

LD = np.longdouble
PI = 4 * np.arctan(LD(1))           # np.pi would leave the reference itself good to 1e-14 only at nt = 512
DSC = 0.37

SHAPES = {1: ((130, 9, 40), 2), 2: ((66, 10, 80), 2), 3: ((66, 10, 140), 2), 4: ((34, 6, 512), 2), 5: ((34, 6, 514), 2),
          6: ((2048, 1, 512), 1), 7: ((2048, 4, 340), 2), 8: ((2048, 4, 262), 2), 9: ((3, 4096, 505), 2),
          10: ((66, 5, 5), 2), 11: ((66, 5, 12), 2), 12: ((66, 5, 23), 2), 13: ((66, 5, 49), 2), 14: ((66, 5, 100), 2),
          15: ((66, 5, 133), 2), 16: ((66, 5, 200), 2), 17: ((66, 5, 270), 2), 18: ((66, 5, 500), 2),
          19: ((514, 3, 200), 2), 20: ((2048, 1, 505), 1),
          21: ((257, 5, 12), 2), 22: ((1000, 3, 12), 2), 23: ((1025, 3, 12), 2), 24: ((96, 5, 12), 2), 25: ((4096, 1, 12), 1),
          26: ((4101, 1, 12), 1), 27: ((6, 257, 12), 2), 28: ((6, 1000, 12), 2), 29: ((6, 1025, 12), 2), 30: ((66, 5, 64), 2),
          31: ((66, 5, 33), 2)}
# the pipelined fused transform pass along t, k_dct_tsolve_pipe<LG> (module docstring): shape -> the kernels that
# dotsocp_dct_pass_kernel / dotsocp_tsolve_kernel must name for (y pass, x pass, t step); None: not claimed
PIPE_SHAPES = {32: ((256, 512, 32), 2), 33: ((256, 256, 64), 2), 34: ((256, 288, 64), 2), 35: ((128, 256, 128), 2),
               36: ((128, 128, 256), 2), 37: ((64, 128, 512), 2), 38: ((64, 64, 1024), 2), 39: ((1024, 64, 64), 2),
               40: ((64, 1024, 64), 2), 41: ((4096, 1, 512), 1)}
PIPE_KERNELS = {32: ("pow2-pipe", "pow2-pipe", "fused-pipe"), 33: ("pow2-pipe", "pow2-pipe", "fused-pipe"),
                34: ("pow2-pipe", None, "fused-pipe"), 35: (None, None, "fused-pipe"), 36: (None, None, "fused-pipe"),
                37: (None, None, "fused-pipe"), 38: (None, None, "fused-pipe"), 39: ("pow2-pipe", None, "fused-pipe"),
                40: (None, "pow2-pipe", "fused-pipe"), 41: ("pow2-long", "none", "fused-pipe")}
SHAPES.update(PIPE_SHAPES)
TS_TILE = 4096                      # doubles per tile of k_dct_tsolve_pipe (TS_LG_CPLX = 11 complex pairs of lines)
LAYOUTS = [(1, dict(nslabs=1)), (1, dict(nslabs=2)), (1, dict(nslabs=3)), (1, dict(nslabs=12)), (1, dict(nslabs=20)),
           (1, dict(ngpu=2)), (2, dict(nslabs=2)), (3, dict(nslabs=2)), (4, dict(nslabs=1)), (4, dict(nslabs=2)),
           (4, dict(nslabs=4)), (5, dict(nslabs=2)), (6, dict(nslabs=2)), (6, dict(nslabs=4)), (7, dict(nslabs=2)),
           (8, dict(nslabs=2)), (9, dict(nslabs=1))] + [(no, dict(nslabs=1)) for no in range(10, 31)]


def _id(case):
    shape, kw = case
    return "shape%d-%s" % (shape, "-".join("%s%d" % kv for kv in kw.items()))


def _basis(n, k):
    """the k-th orthonormal DCT-II basis vector of length n"""
    i = np.arange(n, dtype=LD)
    return np.sqrt(LD(1 if k == 0 else 2) / n) * np.cos(PI * k * (2 * i + 1) / (2 * n))


def _eig(n):
    """initialize_FFTkernel.m:6-8"""
    return 2 * LD(n - 1) ** 2 * (1 - np.cos(PI * np.arange(n, dtype=LD) / n))


def _eig_table(n):
    """the same eigenvalues as the operator holds them: the float64 table of initialize_FFTkernel.m:6-8, which the
    reference and the device alike evaluate as 2 (n-1)^2 (1 - cos(pi k / n)) in doubles.  They are the operator's data
    along y and x -- the t solve divides by these numbers -- and 1 - cos cancels at the low modes of a long axis: at
    n = 4096 the entry k = 1 is good to 3e-11 only, which a solution at nt = 12 shows in full (1.6e-11 at (1, 0) against
    the eigenvalues in long double, on the device and in numpy alike)"""
    return ((2.0 * (n - 1) ** 2) * (1.0 - np.cos(np.pi * np.arange(n) / n))).astype(LD)


def _modes(ny, nx):
    kys = sorted({0, 1, 2, ny // 8, ny // 2, ny - 2, ny - 1} & set(range(ny)))
    kxs = sorted({0, 1, nx - 1} & set(range(nx)))
    return [(ky, kx) for ky in kys for kx in kxs]


def _pipe_modes(ny, nx, nt):
    """_modes(ny, nx) and what k_dct_tsolve_pipe can get wrong beside them.  A tile holds L = 4096 / nt consecutive
    lines ky of one kx and reads CY from LDS by the line's index: ky = L - 1 and L (the last line of one tile, the first
    of the next), 2 L - 1 and 2 L (one tile further on), where they exist.  CX arrives once per tile, and a persistent
    workgroup walks tiles that are G apart in ky + ny kx: kx = nx / 2 besides 0 and nx - 1 puts probes into its first,
    a middle and its last tile.  The full product of the two lists, the modes of _modes first and in their order."""
    base = _modes(ny, nx)
    L = TS_TILE // nt
    kys = sorted({ky for ky, _ in base} | ({L - 1, L, 2 * L - 1, 2 * L} & set(range(ny)) if L < ny else set()))
    kxs = sorted({kx for _, kx in base} | ({nx // 2} if 0 < nx // 2 < nx - 1 else set()))
    return base + [(ky, kx) for ky in kys for kx in kxs if (ky, kx) not in base]


def _cpu_error(g, amp, x, cyk, cxk, nt, zero):
    """e_cpu of a mode: the same operation along t in plain float64 -- scipy's DCT-II of amp g, division by the float64
    D^2 (CY[ky] + CX[kx] + CT) with the float64 table CT the device holds, scipy's DCT-III -- against the long-double x"""
    lam = (float(cyk) + float(cxk)) + _eig_table(nt).astype(np.float64)
    if zero:
        lam[0] = 1.0
    y = sfft.idct(sfft.dct((amp * g).astype(np.float64), type=2, norm="ortho") / (DSC * DSC * lam), type=2, norm="ortho")
    return float(np.max(np.abs(y.astype(LD) - x)))


@functools.lru_cache(maxsize=4)
def _solved_modes(shape_no):
    """Per shape, computed once and read-only: the modes with their long-double solutions, amplitudes and bounds (the
    shapes of PIPE_SHAPES: with e_cpu, and the bound max(the project's, 4 e_cpu)), and the bands."""
    (ny, nx, nt), _ = SHAPES[shape_no]
    pipe = shape_no in PIPE_SHAPES
    rng = np.random.default_rng(1000 + shape_no)
    C = np.stack([_basis(nt, k) for k in range(nt)])            # C[k, t]
    cy, cx, ct = _eig_table(ny), _eig_table(nx), _eig(nt)
    modes = []
    for ky, kx in (_pipe_modes(ny, nx, nt) if pipe else _modes(ny, nx)):
        g = rng.standard_normal(nt).astype(LD)
        lam = cy[ky] + cx[kx] + ct
        if ky == 0 and kx == 0:
            lam[0] = 1                                           # kernel(kernel == 0) = 1 (initialize_FFTkernel.m:15)
        x = C.T @ ((C @ g) / (LD(DSC) ** 2 * lam))
        amp = 1 / np.max(np.abs(x))
        ap = float((cy[ky] + cx[kx]) / LD(nt - 1) ** 2)
        bound = 1e-12 if (ky, kx) == (0, 0) else 1e-12 * max(1.0, 1e-2 / ap)
        m = dict(k=(ky, kx), g=g, x=amp * x, amp=amp, ap=ap, bound=bound, u=_basis(ny, ky), v=_basis(nx, kx))
        if pipe:
            m["e_cpu"] = _cpu_error(g, amp, m["x"], cy[ky], cx[kx], nt, (ky, kx) == (0, 0))
            m["bound"] = max(bound, 4 * m["e_cpu"])
        modes.append(m)
    # bands: (0, 0) alone -- the singular column travels whole and is solved by recurrence -- then by amplitude
    bands = [[m for m in modes if m["k"] == (0, 0)]]
    for m in sorted((m for m in modes if m["k"] != (0, 0)), key=lambda m: float(m["amp"])):
        if len(bands) == 1 or m["amp"] > 16 * bands[-1][0]["amp"]:
            bands.append([])
        bands[-1].append(m)
    return modes, bands


def _plane(m):
    """b[y + ny x] = u(y) v(x)"""
    return np.outer(m["v"], m["u"]).ravel()


@functools.lru_cache(maxsize=2)
def _probe(shape_no):
    """The bands of _solved_modes and their right-hand sides (float64, Fortran (ny, nx, nt)), the dense way: every mode
    with its plane b, one outer product per mode."""
    (ny, nx, nt), _ = SHAPES[shape_no]
    modes, bands = _solved_modes(shape_no)
    for m in modes:
        m.setdefault("b", _plane(m))
    rhs = []
    for band in bands:
        r = np.zeros((ny * nx, nt), dtype=LD)
        for m in band:
            r += np.outer(m["b"], m["amp"] * m["g"])
        r = np.asfortranarray(r.astype(np.float64)).reshape((ny, nx, nt), order="F")
        r.setflags(write=False)
        rhs.append(r)
    return bands, rhs


def _rhs_separable(band, shape):
    """sum over the band of u(y) v(x) (amp g(t)) by broadcasting into one accumulator and one scratch array; the products
    are taken in the order of _probe, (u v) (amp g), so the float64 array has the same bits"""
    ny, nx, nt = shape
    r = np.zeros((ny * nx, nt), dtype=LD)
    tmp = np.empty_like(r)
    for m in band:
        np.multiply(_plane(m)[:, None], (m["amp"] * m["g"])[None, :], out=tmp)
        r += tmp
    r = np.asfortranarray(r.astype(np.float64)).reshape(shape, order="F")
    r.setflags(write=False)
    return r


def _project_separable(band, sol):
    """[mode of the band] -> sum_x v(x) sum_y u(y) sol[y, x, :] in long double: y is contracted once per distinct ky"""
    ny, nx, nt = sol.shape
    kys = sorted({m["k"][0] for m in band})
    W = sol.reshape((ny, nx * nt), order="F").astype(LD)
    Y = (np.stack([_basis(ny, ky) for ky in kys]) @ W).reshape((len(kys), nx, nt), order="F")
    return [m["v"] @ Y[kys.index(m["k"][0])] for m in band]


def _errors(shape_no, kw):
    """[(mode, e_j, bound_j)] over all bands of the shape, one context, one solve per band"""
    (ny, nx, nt), dim = SHAPES[shape_no]
    bands, rhs = _probe(shape_no)
    sols = D.poisson_on_slabs(rhs[0], DSC, dim=dim, repeat=rhs[1:], **kw)
    out = []
    for band, sol in zip(bands, sols):
        assert np.all(np.isfinite(sol))
        W = sol.reshape((ny * nx, nt), order="F").astype(LD)
        P = np.stack([m["b"] for m in band]) @ W
        for m, p in zip(band, P):
            out.append((m, float(np.max(np.abs(p - m["x"]))), m["bound"]))
    return out


def _report(tag, errs):
    m, e, b = max(errs, key=lambda r: r[1])
    mr, er, br = max(errs, key=lambda r: r[1] / r[2])
    print("\n%s: worst e_j %.2e at (ky, kx) = %s, a' = %.3g; worst e_j / bound %.2e at %s, a' = %.3g"
          % (tag, e, m["k"], m["ap"], er / br, mr["k"], mr["ap"]))


def _check(tag, errs):
    _report(tag, errs)
    bad = ["(ky, kx) = %s, a' = %.3g: e = %.2e > %.2e" % (m["k"], m["ap"], e, b) for m, e, b in errs if not e <= b]
    assert not bad, tag + ": " + "; ".join(bad)


def _assert_bands(bands, least):
    assert [m["k"] for m in bands[0]] == [(0, 0)] and len(bands) >= least
    for band in bands:
        amps = [float(m["amp"]) for m in band]
        assert max(amps) <= 16 * min(amps)
        for m in band:
            assert abs(float(np.max(np.abs(m["x"]))) - 1) < 1e-15


def test_bands_of_the_probes():
    """(No device needed.)  What the probes rest on: three or more bands per shape besides (0, 0), amplitudes within a
    factor of 16 inside a band, every component of the solution of unit size.  The shapes of the pipelined t pass (38:
    nt = 1024, a' down to 4e-5 -- the worst conditioned; 41: 1-D, a' up to 257) besides: every mode of _pipe_modes is
    there, the tile borders included, and its own float64 model is worth something -- e_cpu finite and below 1e-6,
    or 4 e_cpu would bound nothing."""
    for shape_no in (1, 6):
        bands, rhs = _probe(shape_no)
        _assert_bands(bands, 4)
        assert len(rhs) == len(bands)
    for shape_no in (38, 41):
        (ny, nx, nt), _ = SHAPES[shape_no]
        modes, bands = _solved_modes(shape_no)
        _assert_bands(bands, 2)       # (64, 64, 1024): a' = 4e-5 .. 0.03, two bands besides (0, 0)
        L = TS_TILE // nt
        ks = [m["k"] for m in modes]
        assert ks[:len(_modes(ny, nx))] == _modes(ny, nx) and len(set(ks)) == len(ks)
        assert sorted(m["k"] for band in bands for m in band) == sorted(ks)
        assert {(ky, kx) for ky in (L - 1, L, 2 * L - 1, 2 * L) for kx in {0, nx // 2, nx - 1}} <= set(ks)
        for m in modes:
            assert np.isfinite(m["e_cpu"]) and m["e_cpu"] < 1e-6, (m["k"], m["e_cpu"])
            assert m["bound"] == max(1e-12 if m["k"] == (0, 0) else 1e-12 * max(1.0, 1e-2 / m["ap"]), 4 * m["e_cpu"])


def test_separable_probe_is_the_dense_probe():
    """(No device needed.)  Shape 1 both ways: the right-hand sides built by broadcasting have the bits of _probe's, and
    the projection that contracts y, then x, is the dense long-double product up to the rounding of long-double sums of
    1170 terms of size <= 1 (another order of summation: 1170 * 2^-64 = 6e-17)."""
    shape, _ = SHAPES[1]
    bands, rhs = _probe(1)
    sol = np.asfortranarray(np.random.default_rng(1).standard_normal(shape))
    W = sol.reshape((shape[0] * shape[1], shape[2]), order="F").astype(LD)
    for band, r in zip(bands, rhs):
        assert np.array_equal(_rhs_separable(band, shape), r)
        dense = np.stack([m["b"] for m in band]) @ W
        for p, q in zip(_project_separable(band, sol), dense):
            assert float(np.max(np.abs(p - q))) <= 6e-17


def _pipe_errors(shape_no):
    """[(mode, e_device, bound)] of a shape of PIPE_SHAPES on one slab: one context, one solve per band, the right-hand side
    of a band built when its turn comes (4.2 M nodes: one band at a time in memory)"""
    shape, dim = SHAPES[shape_no]
    _, bands = _solved_modes(shape_no)
    sols = D.poisson_on_slabs(_rhs_separable(bands[0], shape), DSC, dim=dim,
                              repeat=[_rhs_separable(band, shape) for band in bands[1:]])
    out = []
    for band, sol in zip(bands, sols):
        assert np.all(np.isfinite(sol))
        for m, p in zip(band, _project_separable(band, sol)):
            out.append((m, float(np.max(np.abs(p - m["x"]))), m["bound"]))
    return out


def _pipe_report(tag, errs):
    for what, (m, e, b) in (("worst e_device", max(errs, key=lambda r: r[1])),
                            ("worst e_device / bound", max(errs, key=lambda r: r[1] / r[2]))):
        print("\n%s: %s at (ky, kx) = %s, a' = %.3g: e_device %.2e, e_cpu %.2e, e_device / e_cpu %.2f, bound %.2e"
              % (tag, what, m["k"], m["ap"], e, m["e_cpu"], e / m["e_cpu"] if m["e_cpu"] > 0 else float("inf"), b), end="")
    print()


@gpu
@pytest.mark.parametrize("shape_no", sorted(PIPE_SHAPES))
def test_modes_through_the_pipelined_t_pass(shape_no):
    """Shapes 32 .. 41 on one slab.  First the instance: what the library's own launch decision (dotsocp_tsolve_kernel,
    dotsocp_dct_pass_kernel: the functions the launchers switch on) names for this grid on this device must be what the
    table of the module docstring claims -- on a device with another CU count this fails and says what runs instead.
    Then every mode of _pipe_modes against the long-double reference, bound max(the project's, 4 e_cpu)."""
    (ny, nx, nt), dim = SHAPES[shape_no]
    found = capi.poisson_kernels(ny, nx, nt)
    for what, want, got in zip(("y pass", "x pass", "t step"), PIPE_KERNELS[shape_no], found):
        assert want is None or got == want, "shape %d %s: the %s of this device is '%s', not '%s' (all: %s)" % (
            shape_no, (ny, nx, nt), what, got, want, found)
    errs = _pipe_errors(shape_no)
    assert [m["k"] for m, _, _ in errs] == [m["k"] for band in _solved_modes(shape_no)[1] for m in band]
    _pipe_report("shape%d" % shape_no, errs)
    bad = ["(ky, kx) = %s, a' = %.3g: e_device = %.2e > %.2e (e_cpu %.2e)" % (m["k"], m["ap"], e, b, m["e_cpu"])
           for m, e, b in errs if not e <= b]
    assert not bad, "shape%d: " % shape_no + "; ".join(bad)


@gpu
@pytest.mark.parametrize("case", LAYOUTS, ids=_id)
def test_modes_on_slabs(case):
    shape_no, kw = case
    _check(_id(case), _errors(shape_no, kw))


@gpu
@pytest.mark.parametrize("case", [(1, dict(nslabs=2)), (1, dict(nslabs=3)), (3, dict(nslabs=2)), (31, dict(nslabs=1))],
                         ids=_id)
def test_modes_through_the_transposes(case, monkeypatch):
    """DOTSOCP_TSOLVE=dct: the slab <-> pencil transposes around the t-axis transform, same probes, same bounds; on one
    slab (shape 31) the fused transform pass along t instead of the tridiagonal kernel"""
    monkeypatch.setenv("DOTSOCP_TSOLVE", "dct")
    shape_no, kw = case
    _check(_id(case) + "-dct", _errors(shape_no, kw))


def _slab_nodes(nt, nslabs):
    return [b - a for a, b in (capi.slab_range(nt, nslabs, r) for r in range(nslabs))]


@gpu
@pytest.mark.parametrize("shape_no,nslabs,tri", [(1, 2, True), (3, 2, True), (4, 2, True), (5, 2, False)])
def test_which_t_solve_ran(shape_no, nslabs, tri, monkeypatch):
    """The slab runs above took the tridiagonal path, shape 5 (257 nodes per slab > TRI_EXTRA) the transposes: with
    DOTSOCP_TSOLVE=dct every context transposes, so the bits of the default run differ from that run's exactly where the
    default is another algorithm for the same systems, and are the same bits where it is the same launches."""
    (ny, nx, nt), dim = SHAPES[shape_no]
    assert (max(_slab_nodes(nt, nslabs)) <= 256) == tri
    rhs = np.asfortranarray(np.random.default_rng(shape_no).standard_normal((ny, nx, nt)))
    a = D.poisson_on_slabs(rhs, DSC, nslabs=nslabs, dim=dim)
    monkeypatch.setenv("DOTSOCP_TSOLVE", "dct")
    b = D.poisson_on_slabs(rhs, DSC, nslabs=nslabs, dim=dim)
    # the same operation: each run within the bound of its worst-conditioned mode (the smallest a') of the field
    ap = min(float(v) for v in (_eig(ny)[1:2].tolist() + _eig(nx)[1:2].tolist())) / (nt - 1) ** 2
    np.testing.assert_allclose(a, b, rtol=0, atol=2e-12 * max(1.0, 1e-2 / ap) * np.abs(b).max())
    assert np.array_equal(a, b) == (not tri)


@gpu
@pytest.mark.parametrize("nx,safe", [(2048, True), (4096, False)])
def test_single_slab_t_solve_and_the_guard(nx, safe, monkeypatch):
    """3 x nx x 505 on one slab: at nx = 2048 the tridiagonal kernel runs (other bits than the transform passes), at
    nx = 4096 the powers of its 64-row pieces could fall below TRI_PW_SAFE and the transform passes run: the same bits."""
    assert capi.lib().dotsocp_tsolve_tri_safe(3, nx, 505) == int(safe)
    rhs = np.asfortranarray(np.random.default_rng(nx).standard_normal((3, nx, 505)))
    a = D.poisson_on_slabs(rhs, DSC)
    monkeypatch.setenv("DOTSOCP_TSOLVE", "dct")
    b = D.poisson_on_slabs(rhs, DSC)
    assert np.array_equal(a, b) == (not safe)


@gpu
def test_poisson_phi_only_before_begin():
    rho0, rho1 = D.get_example_2d("example1", 16, 16)
    var, model = D.initialize(rho0, rho1, 8)
    D.InitialScaling(var, model, True)
    ctx = D.InPALMContext(var, dict(tau=1.9, sigma=1.0, tol=0.0, maxit=1), model)
    try:
        assert capi.lib().dotsocp_poisson_phi(ctx._ctx) == -4          # DOTSOCP_ESTATE
    finally:
        ctx.close()
