"""The algebra behind the division-free tridiagonal kernels of dot-socp_amd/csrc/tri.hip (round 4; the sweeps themselves:
tri_sweep.h), restated in numpy and held against dense solves: closed-form pivots piv_t = r N_{t+1} / N_t, the two running
sums H_t = g_t + rho H_{t-1}, G_t = sum rho^s g_s from which both sweeps of a column come (tri_ends / tri_last / tri_spike /
TriFwd / TriBwd: _piece() with its flags into_rhs = !LEFT and keep_power = KEEP), for blocks that start / end on a global
Neumann row or couple to a neighbour slab.  A CPU test of the device code's mathematics -- the kernels themselves are
checked against scipy's DCT and the single slab in the GPU suite."""
import numpy as np
import pytest


def _block(ap, n, first, last):
    A = np.zeros((n, n))
    for t in range(n):
        A[t, t] = ap + 2 - (1 if first and t == 0 else 0) - (1 if last and t == n - 1 else 0)
        if t > 0:
            A[t, t - 1] = -1
        if t < n - 1:
            A[t, t + 1] = -1
    return A


def _coef(ap):                      # tri_coef
    s = np.sqrt(ap * (1 + 0.25 * ap))
    rm1 = 0.5 * ap + s
    r = 1 + rm1
    rho = 1 / r
    return dict(rho=rho, rho2=rho * rho, r=r, n0d=(rm1 * rho) * (1 + rho))


def _ends(c, bnd, n, rn1):          # tri_ends
    pe = c["rho"] if bnd else c["rho2"]
    s = 1.0 if bnd else -1.0
    N0 = (1 + c["rho"]) if bnd else c["n0d"]
    N1 = N0 if n == 1 else 1 + s * (rn1 * rn1) * pe
    return N0, N1, c["n0d"] + c["rho2"] * N1, s, pe


def _last(c, D, N1, Nn, bnd):       # tri_last
    return D / (c["r"] * Nn - N1) if bnd else c["rho"] * D / Nn


PW_SAFE = 2.0 ** -500               # TRI_PW_SAFE


def _piece(c, g, xl, xr, first, last, into_rhs=False, keep_power=None):
    """k_tri_local (Gf, Gl), tri_spike (vf, vl, wf, wl) and k_tri_final_reg (x) for one block.  The interface values enter
    as xl N_0 rho^t (k_tsolve_single) or, into_rhs, on the first / last right-hand-side entry (k_tri_final, k_tri_final_reg).
    keep_power: the backward sweep resumes rho^t from the last row whose power was still >= PW_SAFE (N_t = 1 behind it);
    False: the walk back up from rho^(n-1) itself, which is lost once that has left the normal range.  Default: what the
    kernels do -- k_tri_final / k_tri_final_reg (into_rhs) keep the power, k_tsolve_single / k_tsolve_pipe do not and are
    kept off the grids where it matters by tsolve_tri_safe()."""
    if keep_power is None:
        keep_power = into_rhs
    n = len(g)
    rn1 = c["rho"] ** (n - 1)
    f0, f1, fn, sf, pef = _ends(c, first, n, rn1)
    b0, b1, bn, sb, peb = _ends(c, last, n, rn1)
    gg = np.array(g, dtype=float)
    if into_rhs:
        gg[0] += xl
        gg[-1] += xr
    H = G = 0.0
    pw = 1.0
    ts, pws = 0, 1.0
    Dv = np.zeros(n)
    for t in range(n):
        H = gg[t] + c["rho"] * H
        G += pw * gg[t]
        Dv[t] = H + (sf * pef * pw) * G
        if pw >= PW_SAFE:
            ts, pws = t, pw
        if t + 1 < n:
            pw *= c["rho"]
    if into_rhs:
        Gf, Gl = _piece(c, g, 0.0, 0.0, first, last)[:2]        # k_tri_local sees the slab's own right-hand side
        cl = 0.0
        xn = _last(c, Dv[-1], f1, fn, last)
    else:
        Gl = _last(c, Dv[-1], f1, fn, last)
        Gf = _last(c, G + (sb * peb * rn1) * H, b1, bn, first)
        cl = xl * f0
        xn = _last(c, (Dv[-1] + cl * pw) + xr * f1, f1, fn, last)
    if keep_power:
        pw = pws
    else:
        ts = n - 1
    x = np.zeros(n)
    x[-1] = xn
    Nt1 = f1
    for t in range(n - 2, -1, -1):
        if t < ts:
            pw *= c["r"]
        Nt = f0 if t == 0 else (1.0 if t > ts else 1 + sf * (pw * pw) * pef)
        xn = c["rho"] * ((Dv[t] + (0.0 if t > ts else cl * pw)) + Nt * xn) / Nt1
        x[t] = xn
        Nt1 = Nt
    if last:
        den = c["r"] * fn - f1
        vl, wl = rn1 * f0 / den, f1 / den
    else:
        vl, wl = rn1 * c["rho"] * f0 / fn, c["rho"] * f1 / fn
    if first:
        den = c["r"] * bn - b1
        wf, vf = rn1 * b0 / den, b1 / den
    else:
        wf, vf = rn1 * c["rho"] * b0 / bn, c["rho"] * b1 / bn
    return Gf, Gl, x, (vf, vl, wf, wl)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_closed_form_sweeps_against_dense_solves(seed):
    rng = np.random.default_rng(seed)
    worst = 0.0
    for _ in range(1500):
        n = int(rng.integers(1, 70))
        ap = float(10 ** rng.uniform(-4, 4))        # a' = (CY + CX) / (nt - 1)^2: 6e-4 .. 5e5 on the grids of BASELINE.json
        first, last = bool(rng.integers(2)), bool(rng.integers(2))
        if n == 1 and first and last:
            continue
        A = _block(ap, n, first, last)
        g = rng.standard_normal(n)
        c = _coef(ap)
        xl, xr = rng.standard_normal(2)
        Gf, Gl, x, (vf, vl, wf, wl) = _piece(c, g, xl, xr, first, last)
        sol = np.linalg.solve(A, g)
        g2 = g.copy()
        g2[0] += xl
        g2[-1] += xr
        sol2 = np.linalg.solve(A, g2)
        Ai = np.linalg.inv(A)
        e = max(max(abs(Gf - sol[0]), abs(Gl - sol[-1])) / np.max(np.abs(sol)),
                np.max(np.abs(x - sol2)) / np.max(np.abs(sol2)),
                max(abs(vf - Ai[0, 0]), abs(vl - Ai[-1, 0]), abs(wf - Ai[0, -1]), abs(wl - Ai[-1, -1])) / np.max(np.abs(Ai)))
        worst = max(worst, e)
    assert worst <= 2e-11, worst           # observed 2e-12: the conditioning of the smallest modes (a' ~ 1e-4, n ~ 70)


def test_partitioned_solve_equals_the_whole_column():
    """NSUB pieces coupled through the reduced system (k_tri_reduced's sweep, also inside k_tsolve_single) give the solution
    of the whole Neumann column."""
    rng = np.random.default_rng(7)
    for _ in range(200):
        P = int(rng.integers(2, 9))
        sizes = [int(rng.integers(1, 40)) for _ in range(P)]
        if sizes[0] == 1 and P == 1:
            continue
        nt = sum(sizes)
        ap = float(10 ** rng.uniform(-3.5, 3))
        c = _coef(ap)
        g = rng.standard_normal(nt)
        whole = np.linalg.solve(_block(ap, nt, True, True), g)
        off = np.cumsum([0] + sizes)
        loc = []
        for p in range(P):
            gp = g[off[p]:off[p + 1]]
            Gf, Gl, _, spike = _piece(c, gp, 0.0, 0.0, p == 0, p == P - 1)
            vf, vl, wf, wl = spike
            if p == 0:
                vf = vl = 0.0
            if p == P - 1:
                wf = wl = 0.0
            loc.append((Gf, Gl, vf, vl, wf, wl))
        A_, B_, al, ga = [0.0] * P, [0.0] * P, [0.0] * P, [0.0] * P
        for p, (Gf, Gl, vf, vl, wf, wl) in enumerate(loc):
            if p == 0:
                A_[0], B_[0], al[0], ga[0] = Gf, wf, Gl, wl
            else:
                den = 1.0 - vf * ga[p - 1]
                A_[p] = (Gf + vf * al[p - 1]) / den
                B_[p] = wf / den
                al[p] = Gl + vl * (al[p - 1] + ga[p - 1] * A_[p])
                ga[p] = wl + vl * ga[p - 1] * B_[p]
        Fnext = 0.0
        x = np.zeros(nt)
        for p in range(P - 1, -1, -1):
            Fp = A_[p] + B_[p] * Fnext
            Lprev = al[p - 1] + ga[p - 1] * Fp if p > 0 else 0.0
            gp = g[off[p]:off[p + 1]]
            x[off[p]:off[p + 1]] = _piece(c, gp, Lprev, Fnext, p == 0, p == P - 1)[2]
            Fnext = Fp
        assert np.max(np.abs(x - whole)) <= 1e-10 * np.max(np.abs(whole))


# ---- the regime where rho^(n-1) leaves the normal range (slabs of more than 64 nodes and large a') ----
LD = np.longdouble


def _thomas_ld(ap, g, first=True, last=True):
    """(a' I + tridiag(-1, [2 - first, 2, ..., 2 - last], -1)) x = g by elimination in long double (diagonally dominant)"""
    n = len(g)
    d = np.full(n, LD(ap) + 2, dtype=LD)
    if first:
        d[0] -= 1
    if last:
        d[-1] -= 1
    b = np.array(g, dtype=LD)
    for t in range(1, n):
        w = LD(1) / d[t - 1]
        d[t] -= w
        b[t] += w * b[t - 1]
    x = np.zeros(n, dtype=LD)
    x[-1] = b[-1] / d[-1]
    for t in range(n - 2, -1, -1):
        x[t] = (b[t] + x[t + 1]) / d[t]
    return x


def _partitioned(ap, g, sizes, into_rhs=True, **kw):
    """k_tri_local -> k_tri_reduced -> k_tri_final over slabs of `sizes` nodes (the interface values on the right-hand
    side); into_rhs=False: the pieces of k_tsolve_single (the left interface value as xl N_0 rho^t)"""
    c = _coef(ap)
    P = len(sizes)
    off = np.cumsum([0] + list(sizes))
    A_, B_, al, ga = [0.0] * P, [0.0] * P, [0.0] * P, [0.0] * P
    for p in range(P):
        Gf, Gl, _, (vf, vl, wf, wl) = _piece(c, g[off[p]:off[p + 1]], 0.0, 0.0, p == 0, p == P - 1, **kw)
        if p == 0:
            A_[0], B_[0], al[0], ga[0] = Gf, (0.0 if P == 1 else wf), Gl, (0.0 if P == 1 else wl)
        else:
            if p == P - 1:
                wf = wl = 0.0
            den = 1.0 - vf * ga[p - 1]
            A_[p] = (Gf + vf * al[p - 1]) / den
            B_[p] = wf / den
            al[p] = Gl + vl * (al[p - 1] + ga[p - 1] * A_[p])
            ga[p] = wl + vl * ga[p - 1] * B_[p]
    Fnext = 0.0
    x = np.zeros(len(g))
    for p in range(P - 1, -1, -1):
        Fp = A_[p] + B_[p] * Fnext
        Lprev = al[p - 1] + ga[p - 1] * Fp if p > 0 else 0.0
        x[off[p]:off[p + 1]] = _piece(c, g[off[p]:off[p + 1]], Lprev, Fnext, p == 0, p == P - 1, into_rhs=into_rhs, **kw)[2]
        Fnext = Fp
    return x


def _power_underflows(ap, n):
    return (n - 1) * np.log2(_coef(ap)["r"]) > 1000.0          # rho^(n-1) < 2^-1000: denormal or zero


def _err(x, ref):
    return float(np.max(np.abs(x.astype(LD) - ref)) / np.max(np.abs(ref)))


def _bound(ap):
    return 1e-12 * max(1.0, 1e-2 / ap)


def _draw(rng, underflow):
    """slab sizes and a': n up to 256 nodes per slab, a' in 1e-4 .. 1e5; underflow: the longest slab has rho^(n-1) < 2^-1000"""
    P = int(rng.integers(2, 5))
    if underflow:
        nmax = int(rng.integers(65, 257))
        lo = 2.0 ** (1050.0 / (nmax - 1))                     # r >= lo; a' = r - 2 + 1 / r
        ap = float(10 ** rng.uniform(np.log10(lo - 2 + 1 / lo), 5))
    else:
        nmax = int(rng.integers(2, 257))
        ap = float(10 ** rng.uniform(-4, 5))
    sizes = [nmax] + [int(rng.integers(2, nmax + 1)) for _ in range(P - 1)]
    rng.shuffle(sizes)
    return ap, [int(v) for v in sizes]


@pytest.mark.parametrize("seed", [0, 1])
def test_partitioned_solve_where_the_powers_underflow(seed):
    """Slabs of up to 256 nodes, a' up to 1e5, four draws in ten with rho^(n-1) denormal or zero on the longest slab, against
    an elimination in long double.  Bound: 1e-12 max(1, 1e-2 / a') of the column's max-abs -- the rounding of the sweeps
    (<= 3e-14 where a' >= 1e-2) times the 1 / a' growth of the column's condition below that.  The walk back up from
    rho^(n-1) itself (keep_power=False, the kernels before the fix) is wrong by 1e-6 there."""
    rng = np.random.default_rng(100 + seed)
    worst_ratio, worst_old, n_under = 0.0, 0.0, 0
    for i in range(120):
        under = i % 5 < 2
        ap, sizes = _draw(rng, under)
        g = rng.standard_normal(sum(sizes))
        ref = _thomas_ld(ap, g)
        e = _err(_partitioned(ap, g, sizes), ref)
        assert e <= _bound(ap), (ap, sizes, e)
        worst_ratio = max(worst_ratio, e / _bound(ap))
        if under:
            assert _power_underflows(ap, max(sizes))
            n_under += 1
            worst_old = max(worst_old, _err(_partitioned(ap, g, sizes, keep_power=False), ref))
        else:
            # the powers that stay normal: the fix changes no bit
            if not _power_underflows(ap, max(sizes)) and _coef(ap)["rho"] ** (max(sizes) - 1) >= PW_SAFE:
                assert np.array_equal(_partitioned(ap, g, sizes), _partitioned(ap, g, sizes, keep_power=False))
    print(f"worst error / bound {worst_ratio:.2e}; walk from rho^(n-1): worst {worst_old:.2e} over {n_under} draws")
    assert n_under >= 40
    assert worst_old > 1e-9


@pytest.mark.parametrize("n,ap", [(256, 64.0), (256, 16.0), (200, 40.0), (170, 130.0), (128, 1000.0), (131, 246.0)])
def test_final_sweep_on_the_long_slabs_of_the_issue(n, ap):
    """The (n, a') pairs at which the walk from rho^(n-1) was measured wrong (1e-7 .. 1e-10), on two and four slabs."""
    rng = np.random.default_rng(n)
    for P in (2, 4):
        g = rng.standard_normal(n * P)
        ref = _thomas_ld(ap, g)
        e = _err(_partitioned(ap, g, [n] * P), ref)
        assert e <= _bound(ap), (P, e)


# ---- the single slab: k_tsolve_single / k_tsolve_pipe keep the walk from rho^(n-1); tsolve_tri_safe() keeps them off ----
def _pieces(nt, nsub):
    base, rem = divmod(nt, nsub)
    return [base + (1 if p < rem else 0) for p in range(nsub)]


def _nsub(nt):                      # tsolve_nsub
    return 1 if nt <= 8 else (2 if nt <= 32 else (4 if nt <= 136 else 8))


def _ap_max(ny, nx, nt):
    return 4.0 * ((ny - 1) ** 2 + (nx - 1) ** 2) / (nt - 1) ** 2


def test_single_slab_guard_matches_the_model():
    """dotsocp_tsolve_tri_safe (pure host arithmetic) against the model of k_tsolve_single's pieces, the left interface as
    xl N_0 rho^t and the power walked back up from rho^(n-1): on every grid the guard lets through, the model holds the
    bound at the grid's largest a' (where the powers are smallest); on the 1-D grids it turns away, the powers do fall
    below PW_SAFE, and once rho^(n-1) is zero (100 001 space points at nt = 505) the model is wrong by 4e-9 of the column
    at the largest a' -- what the guard is for."""
    from dotsocp_amd import capi
    safe = capi.lib().dotsocp_tsolve_tri_safe
    rng = np.random.default_rng(11)
    for ny, nx, nt in [(1024, 1024, 128), (1025, 1025, 129), (2049, 2049, 257), (128, 1, 32), (4096, 4096, 129)]:
        assert safe(ny, nx, nt) == 1                         # the grids of BASELINE.json and their neighbours
    assert safe(64, 64, 513) == 0                            # tsolve_tri_supported
    for ny, nt, want in [(3900, 505, 1), (4096, 505, 0), (70001, 505, 0), (100001, 505, 0), (2048, 505, 1), (300000, 400, 0), (5000, 136, 1), (20000, 136, 0),
                         (3000000, 136, 0), (1000, 40, 1)]:
        assert safe(ny, 1, nt) == want, (ny, nt)
        ap = _ap_max(ny, 1, nt)
        sizes = _pieces(nt, _nsub(nt))
        assert (_coef(ap)["rho"] ** (max(sizes) - 1) >= PW_SAFE) == bool(want)
        g = rng.standard_normal(nt)
        e = _err(_partitioned(ap, g, sizes, into_rhs=False), _thomas_ld(ap, g))
        if want:
            assert e <= _bound(ap), (ny, nt, e)
        elif _power_underflows(ap, max(sizes)):
            print(f"1-D {ny} x {nt}: the walk from rho^(n-1) = {_coef(ap)['rho'] ** (max(sizes) - 1):.3g}: error {e:.2e}")
            assert e > 1e-9 or _coef(ap)["rho"] ** (max(sizes) - 1) > 0, (ny, nt, e)
