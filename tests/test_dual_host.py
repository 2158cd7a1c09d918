"""The numpy twin of the dual lower bound alone (dot-socp_amd/dual.py: hopf_lax, dual_bound); no device.

The separable transform against the brute-force minimum over all node pairs, the pair inequality that makes the bound a
bound, a closed form, the tie / signed-zero / non-finite rules of include/dotsocp.h, and the certificate itself: on three
problems solved with the oracle both bounds stay below the exact discrete transport cost between the node histograms
(scipy's HiGHS on the transport LP) and within 5 % of it."""
import numpy as np
import pytest

from dotsocp_amd import dual as DU


def _sqdist(ny, nx):
    """|x - y|^2 between all pairs of the ny x nx nodes of the unit square, nodes flat with y fastest"""
    y, x = np.meshgrid(np.arange(ny) / (ny - 1), np.arange(nx) / (nx - 1), indexing="ij")
    y, x = y.ravel(order="F"), x.ravel(order="F")
    return (x[:, None] - x[None, :]) ** 2 + (y[:, None] - y[None, :]) ** 2


def asymmetric_problem():
    """The asymmetric pair of Gaussians, ny 13 x nx 17"""
    X, Y = np.meshgrid(np.linspace(0, 1, 17), np.linspace(0, 1, 13))
    g = lambda mx, my, sx, sy: np.exp(-((X - mx) ** 2 / 2 / sx ** 2 + (Y - my) ** 2 / 2 / sy ** 2))    # noqa: E731
    rho0 = g(.3, .35, .1, .12) + 0.05
    rho1 = g(.7, .6, .15, .08) + 0.5 * g(.4, .8, .07, .07) + 0.05
    return rho0 / rho0.mean(), rho1 / rho1.mean()


def exact_w2(rho0, rho1):
    """W2^2 between the node histograms rho0 / sum(rho0) and rho1 / sum(rho1): the transport LP, solved by HiGHS"""
    from scipy.optimize import linprog
    from scipy.sparse import csr_matrix, eye, kron, vstack
    ny, nx = rho0.shape
    n = ny * nx
    a, b = rho0.ravel(order="F") / rho0.sum(), rho1.ravel(order="F") / rho1.sum()
    ones = csr_matrix(np.ones((1, n)))
    A = vstack([kron(eye(n), ones), kron(ones, eye(n))]).tocsr()[:-1]      # the last row is implied
    r = linprog(_sqdist(ny, nx).ravel(), A_eq=A, b_eq=np.concatenate([a, b])[:-1], bounds=(0, None), method="highs")
    assert r.status == 0, r.message
    return float(r.fun)


def test_separable_passes_equal_the_brute_force_minimum():
    rng = np.random.default_rng(1)
    ny, nx = 13, 17
    f = rng.uniform(-0.3, 0.3, (ny, nx))
    half = 0.5 * _sqdist(ny, nx)                              # [input node, output node]
    ff = f.ravel(order="F")
    for sign in (+1, -1):
        val, win, bad = DU.hopf_lax(f, sign)
        cand = ff[:, None] + half if sign > 0 else ff[:, None] - half
        brute = cand.min(axis=0) if sign > 0 else cand.max(axis=0)
        err = np.max(np.abs(val.ravel(order="F") - brute))
        print("sign", sign, "separable against brute force:", err)
        assert err <= 1e-15 and bad == 0
        assert win.dtype == np.int32 and val.shape == win.shape == (ny, nx)
        # the winners agree wherever the brute-force optimum is unique (to the rounding of the two formulations)
        order = np.sort(cand if sign > 0 else -cand, axis=0)
        unique = order[1] - order[0] > 1e-12
        assert unique.sum() > 0.9 * unique.size
        bwin = cand.argmin(axis=0) if sign > 0 else cand.argmax(axis=0)
        assert np.array_equal(win.ravel(order="F")[unique], bwin[unique])


def test_pair_inequality():
    """H(y) - f(x) <= |x - y|^2 / 2 and f(y) - B(x) <= |x - y|^2 / 2 for every pair: what makes the bound a bound"""
    rng = np.random.default_rng(2)
    for shape in ((13, 17), (29,)):
        f = rng.standard_normal(shape)
        ny, nx = shape if len(shape) == 2 else (shape[0], 1)
        if len(shape) == 2:
            half = 0.5 * _sqdist(ny, nx)
        else:
            t = np.arange(ny) / (ny - 1)
            half = 0.5 * (t[:, None] - t[None, :]) ** 2
        ff = f.ravel(order="F")
        H = DU.hopf_lax(f, +1)[0].ravel(order="F")
        B = DU.hopf_lax(f, -1)[0].ravel(order="F")
        worst_f = np.max(H[None, :] - ff[:, None] - half)
        worst_b = np.max(ff[None, :] - B[:, None] - half.T)
        print(shape, "worst excess forward", worst_f, "backward", worst_b)
        assert worst_f <= 1e-15 and worst_b <= 1e-15


def test_closed_form_of_a_linear_potential():
    """f(x) = v . x with v a multiple of h per axis: H(y) = v . y - |v|^2 / 2, attained at y - v, wherever y - v is a node"""
    ny, nx = 21, 17
    hy, hx = 1.0 / (ny - 1), 1.0 / (nx - 1)
    ky, kx = 3, -2
    vy, vx = ky * hy, kx * hx
    y, x = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    f = vy * (y * hy) + vx * (x * hx)
    H, win, _ = DU.hopf_lax(f, +1)
    inner = (y - ky >= 0) & (y - ky < ny) & (x - kx >= 0) & (x - kx < nx)
    want = vy * (y * hy) + vx * (x * hx) - 0.5 * (vy * vy + vx * vx)
    err = np.max(np.abs(H - want)[inner])
    print("closed form:", err)
    assert inner.sum() == (ny - 3) * (nx - 2) and err <= 4e-16
    assert np.array_equal(win[inner], ((y - ky) + ny * (x - kx))[inner])
    # one axis alone
    n = 33
    h = 1.0 / (n - 1)
    t = np.arange(n)
    H1, w1, _ = DU.hopf_lax(5 * h * (t * h), +1)
    assert np.max(np.abs(H1 - (5 * h * (t * h) - 0.5 * (5 * h) ** 2))[5:]) <= 4e-16 and np.array_equal(w1[5:], t[5:] - 5)


def test_ties_zeros_and_non_finite_entries():
    w = (0.5 * 0.5) * 0.5
    val, win, bad = DU.hopf_lax(w * np.array([0.0, 1.0, 0.0]), +1)
    assert win.tolist() == [0, 0, 2] and val.tolist() == [0.0, w, 0.0] and bad == 0        # three equal candidates: index 0
    val, win, _ = DU.hopf_lax(-w * np.array([0.0, 1.0, 0.0]), -1)
    assert win.tolist() == [0, 0, 2] and val.tolist() == [-0.0, -w, -0.0]
    # the value is the candidate at the winning index: -0.0 + 0.0 w = +0.0 ... unless the winner is the -0.0 itself
    w4 = (0.5 * (1.0 / 3.0)) * (1.0 / 3.0)                  # four nodes
    val, win, _ = DU.hopf_lax(np.array([w4, -0.0, 0.0, w4]), +1)
    assert win.tolist() == [0, 1, 2, 2]                     # 0: w4 ties with -0.0 + w4;  3: 0.0 + w4 ties with w4
    assert val.tolist() == [w4, 0.0, 0.0, w4]
    assert np.signbit(val).tolist() == [False] * 4          # forward, the winning -0.0 + 0.0 * w is a +0.0 ...
    val, win, _ = DU.hopf_lax(np.array([-w4, -0.0, 0.0, -w4]), -1)
    assert win.tolist() == [0, 1, 2, 2] and val.tolist() == [-w4, 0.0, 0.0, -w4]
    assert np.signbit(val).tolist() == [True, True, False, True]        # ... backward, -0.0 - 0.0 * w keeps its sign
    val, win, _ = DU.hopf_lax(np.array([0.0, -0.0]), +1)
    assert win.tolist() == [0, 1] and np.signbit(val).tolist() == [False, False]
    val, win, _ = DU.hopf_lax(np.array([-0.0, 0.0]), -1)
    assert win.tolist() == [0, 1] and np.signbit(val).tolist() == [True, False]
    # non-finite entries are replaced and counted; a line with no finite entry gives index 0
    f = np.array([np.nan, 1.0, np.inf, -np.inf, 0.5])
    val, win, bad = DU.hopf_lax(f, +1)
    assert bad == 3 and np.all(np.isfinite(val)) and set(win.tolist()) <= {1, 4}
    val, win, bad = DU.hopf_lax(f, -1)
    assert bad == 3 and np.all(np.isfinite(val)) and set(win.tolist()) <= {1, 4}
    for sign, none in ((+1, np.inf), (-1, -np.inf)):
        val, win, bad = DU.hopf_lax(np.full(5, np.nan), sign)
        assert bad == 5 and win.tolist() == [0] * 5 and np.all(val == none)
    g = np.ones((4, 3))
    g[2, :] = np.nan                                        # a row without a finite entry: its x pass gives index 0
    val, win, bad = DU.hopf_lax(g, +1)
    assert bad == 3 and np.all(np.isfinite(val)) and np.all(win % 4 != 2)
    val, win, bad = DU.hopf_lax(np.full((4, 3), np.inf), +1)
    assert bad == 12 and np.all(win == 0) and np.all(val == np.inf)


def _oracle_example1(n, nt):
    from oracle.examples import get_example_2d
    return get_example_2d("example1", n, n), nt


CERTIFICATE = {
    "example1_9x9x9": lambda: _oracle_example1(9, 9),
    "example1_17x17x9": lambda: _oracle_example1(17, 9),
    "asymmetric_13x17x9": lambda: (asymmetric_problem(), 9),
}


@pytest.mark.parametrize("case", sorted(CERTIFICATE))
def test_the_bound_certifies_the_exact_discrete_cost(case):
    from oracle import driver as OD
    (rho0, rho1), nt = CERTIFICATE[case]()
    ny, nx = rho0.shape
    var, model, _, _ = OD.solve_single_level(rho0, rho1, nt, dict(tol=1e-4))
    phi = var.phi.reshape((ny, nx, nt), order="F")
    d = DU.dual_bound(phi[:, :, 0], phi[:, :, -1], rho0, rho1)
    rho, Ex, Ey = OD.recover_RhoE(var, model)
    with np.errstate(invalid="ignore", divide="ignore"):
        cost = float(np.mean(np.where(rho > 1e-8, (Ex * Ex + Ey * Ey) / rho, 0.0)))
    exact = exact_w2(rho0, rho1)
    print(case, "cost %.6g  bound %.6g (fwd %.6g, bwd %.6g, raw %.6g)  exact %.6g" %
          (cost, d["bound"], d["bound_fwd"], d["bound_bwd"], d["dual_raw"], exact))
    print(str(d))
    assert d["bound_fwd"] <= exact + 1e-12 and d["bound_bwd"] <= exact + 1e-12
    assert d["bound"] >= 0.95 * exact                      # a cap that keeps a vacuous bound from passing, not a measurement
    assert d["bound"] == max(d["bound_fwd"], d["bound_bwd"]) and d["nonfinite"] == 0
    # (no order between `bound` and `cost` is asserted: at 9 x 9 x 9 the certified bound is the larger of the two)


def test_dual_bound_refuses_bad_masses_and_shapes():
    f = np.zeros((3, 4))
    with pytest.raises(ValueError):
        DU.dual_bound(f, f, np.zeros((3, 4)), np.ones((3, 4)))
    with pytest.raises(ValueError):
        DU.dual_bound(f, f, np.ones((3, 4)), np.full((3, 4), np.inf))
    with pytest.raises(ValueError):
        DU.dual_bound(f, f[:, :3], np.ones((3, 4)), np.ones((3, 4)))
    with pytest.raises(ValueError):
        DU.hopf_lax(np.zeros((3, 1)), +1)
    with pytest.raises(ValueError):
        DU.hopf_lax(f, 0)
