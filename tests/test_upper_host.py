"""The numpy twin of the upper bound alone (dot-socp_amd/upper.py: soft_transform, sinkhorn_round, upper_bound, plan_dense);
no device.

The separable soft transform against the dense log-sum-exp over all node pairs, its hard limit against dual.hopf_lax, the
feasibility of the rounded plan rebuilt as an n x n matrix -- for any potentials, not only converged ones --, and the
certificate itself: on three problems solved with the oracle, and on a cold 1-D problem with zero-mass nodes, the exact
discrete transport cost (scipy's HiGHS on the transport LP) lies between the dual bound and the upper bound, and the upper
bound within 5 % of it."""
import functools

import numpy as np
import pytest

from dotsocp_amd import dual as DU
from dotsocp_amd import upper as U


def _flat(a):
    return np.ravel(a, order="F")


def _exact_w2(rho0, rho1):
    """W2^2 between the node histograms rho0 / sum(rho0) and rho1 / sum(rho1): the transport LP, solved by HiGHS (the lines
    of test_dual_host.exact_w2, for layers and lines)"""
    from scipy.optimize import linprog
    from scipy.sparse import csr_matrix, eye, kron, vstack
    n = rho0.size
    a, b = _flat(rho0) / rho0.sum(), _flat(rho1) / rho1.sum()
    ones = csr_matrix(np.ones((1, n)))
    A = vstack([kron(eye(n), ones), kron(ones, eye(n))]).tocsr()[:-1]      # the last row is implied
    r = linprog(2.0 * U.pair_cost(rho0.shape).ravel(), A_eq=A, b_eq=np.concatenate([a, b])[:-1], bounds=(0, None), method="highs")
    assert r.status == 0, r.message
    return float(r.fun)


def _eps(shape, eps_h2=0.25):
    return float(U._eps(shape, eps_h2, np.float64))


def _densities(rng, shape, zeros=3):
    out = []
    for _ in range(2):
        r = rng.uniform(0.5, 1.5, shape)
        r.flat[rng.choice(r.size, zeros, replace=False)] = 0.0
        out.append(r)
    return out


@pytest.mark.parametrize("shape", [(7, 5), (13, 17), (33,)], ids=str)
def test_separable_passes_equal_the_dense_log_sum_exp(shape):
    from scipy.special import logsumexp
    rng = np.random.default_rng(sum(shape))
    eps = _eps(shape)
    f = rng.uniform(-0.3, 0.3, shape)
    rho = _densities(rng, shape)[0]
    with np.errstate(divide="ignore"):
        f = f - eps * np.log(rho / rho.sum())                 # zero-mass entries: +Inf
    f.flat[1], f.flat[f.size // 2], f.flat[-2] = np.nan, np.inf, -np.inf
    dropped = ~np.isfinite(f)
    assert dropped.sum() == 6
    val, mean = U.soft_transform(f, eps)
    c = U.pair_cost(shape)                                      # [input node, output node]
    ff = np.where(_flat(dropped), np.inf, _flat(f))
    dense = -eps * logsumexp(-(ff[:, None] + c) / eps, axis=0)
    wgt = np.exp(-(ff[:, None] + c - dense[None, :]) / eps)
    dmean = (wgt * c).sum(axis=0) / wgt.sum(axis=0)
    err, merr = np.max(np.abs(_flat(val) - dense)), np.max(np.abs(_flat(mean) - dmean))
    print(shape, "separable against dense: value", err, "of", np.max(np.abs(dense)), " mean", merr, "of", np.max(dmean))
    assert val.shape == mean.shape == shape and np.all(np.isfinite(val))
    assert err <= 1e-12 * np.max(np.abs(dense))
    assert merr <= 1e-12 * max(np.max(dmean), np.max(np.abs(dense)))
    # nothing finite at all: +Inf and a zero mean
    val, mean = U.soft_transform(np.full(shape, np.nan), eps)
    assert np.all(val == np.inf) and np.all(mean == 0.0)
    if len(shape) == 2:                                         # a row without a finite entry drops out, the rest stands
        g = rng.uniform(-0.3, 0.3, shape)
        g[2, :] = np.inf
        val, mean = U.soft_transform(g, eps)
        gg = _flat(g)
        dense = -eps * logsumexp(-(gg[:, None] + c) / eps, axis=0)
        assert np.max(np.abs(_flat(val) - dense)) <= 1e-12 * np.max(np.abs(dense))


@pytest.mark.parametrize("shape", [(7, 5), (13, 17), (33,)], ids=str)
def test_the_hard_limit_is_the_hopf_lax_transform(shape):
    rng = np.random.default_rng(3 + sum(shape))
    f = rng.uniform(-0.3, 0.3, shape)
    f.flat[4] = np.nan
    val, mean = U.soft_transform(f, _eps(shape, 1e-9))
    H, win, bad = DU.hopf_lax(f, +1)
    err = np.max(np.abs(val - H))
    print(shape, "eps = 1e-9 h^2 against hopf_lax:", err)
    assert bad == 1 and err <= 1e-8
    # ... and the mean is the winner's cost (where the winner is unique, which the random potential makes it)
    wcost = U.pair_cost(shape)[_flat(win), np.arange(f.size)]
    assert np.max(np.abs(_flat(mean) - wcost)) <= 1e-8


def _check_plan(u, rho0, rho1, what):
    """the n x n plan rebuilt from the result has the marginals a and b, and costs what `upper` says"""
    P = U.plan_dense(u["f"], u["g"], u["er"], u["ec"], rho0, rho1, u["eps"])
    a, b = _flat(rho0) / rho0.sum(), _flat(rho1) / rho1.sum()
    rows, cols = np.max(np.abs(P.sum(axis=1) - a)), np.max(np.abs(P.sum(axis=0) - b))
    cost = 2.0 * float((P * U.pair_cost(rho0.shape)).sum())
    print("%-28s rows %.2e  columns %.2e  plan cost %.12g  upper %.12g  (kept %.6g, fill %.3e)"
          % (what, rows, cols, cost, u["upper"], u["kept"], u["fill"]))
    assert np.all(P >= 0.0)
    assert rows <= 1e-13 and cols <= 1e-13
    assert abs(cost - u["upper"]) <= 1e-12 * abs(cost)
    assert 0.0 <= u["kept"] <= 1.0 + 1e-12 and u["fill"] >= 0.0
    assert np.all(u["er"] >= 0.0) and np.all(u["ec"] >= 0.0)


@pytest.mark.parametrize("shape", [(9, 9), (13, 17), (33,)], ids=str)
def test_the_rounded_plan_is_feasible_whatever_the_potentials(shape):
    rng = np.random.default_rng(11 + sum(shape))
    rho0, rho1 = _densities(rng, shape)
    # random f and g: nothing of a Sinkhorn iterate in them
    u = U.sinkhorn_round(rho0, rho1, rng.uniform(-0.05, 0.05, shape), max_sweeps=0, g_start=rng.uniform(-0.05, 0.05, shape))
    _check_plan(u, rho0, rho1, "%s random f, g" % (shape,))
    assert u["sweeps"] == 0 and np.isnan(u["defect_first"]) and u["defects"].size == 0
    # a cold start without a sweep, and with a few
    cold = U.sinkhorn_round(rho0, rho1, None, max_sweeps=0)
    _check_plan(cold, rho0, rho1, "%s cold, 0 sweeps" % (shape,))
    some = U.sinkhorn_round(rho0, rho1, None, max_sweeps=5)
    _check_plan(some, rho0, rho1, "%s cold, 5 sweeps" % (shape,))
    assert some["sweeps"] == 5 and some["defect_last"] < some["defect_first"] and some["upper"] < cold["upper"]
    assert some["zero0"] == 3 and some["zero1"] == 3 and some["nonfinite"] == 0 and some["n_nodes"] == rho0.size
    assert np.all(some["er"][rho0 == 0] == 0.0) and np.all(some["ec"][rho1 == 0] == 0.0)
    # the stop rule: behind the first sweep whose defect is small enough
    early = U.sinkhorn_round(rho0, rho1, None, max_sweeps=5, defect_tol=float(some["defects"][1]))
    assert early["sweeps"] == 2 and early["defect_last"] == some["defects"][1] and np.all(np.isnan(early["defects"][2:]))
    # non-finite entries of the start are counted and count as zero
    start = np.zeros(shape)
    start.flat[[0, 5]] = np.nan, -np.inf
    bad = U.sinkhorn_round(rho0, rho1, start, max_sweeps=5)
    assert bad["nonfinite"] == 2 and bad["upper"] == some["upper"]
    assert str(some).startswith("upper: W2^2 of the node histograms <= ")


def _asymmetric_problem():
    X, Y = np.meshgrid(np.linspace(0, 1, 17), np.linspace(0, 1, 13))
    g = lambda mx, my, sx, sy: np.exp(-((X - mx) ** 2 / 2 / sx ** 2 + (Y - my) ** 2 / 2 / sy ** 2))    # noqa: E731
    rho0 = g(.3, .35, .1, .12) + 0.05
    rho1 = g(.7, .6, .15, .08) + 0.5 * g(.4, .8, .07, .07) + 0.05
    return rho0 / rho0.mean(), rho1 / rho1.mean()


def _example1(n):
    from oracle.examples import get_example_2d
    return get_example_2d("example1", n, n)


# the three cases of test_dual_host.CERTIFICATE
CERTIFICATE = {
    "example1_9x9x9": lambda: (_example1(9), 9),
    "example1_17x17x9": lambda: (_example1(17), 9),
    "asymmetric_13x17x9": lambda: (_asymmetric_problem(), 9),
}


@functools.lru_cache(maxsize=None)
def _solved(case):
    """(rho0, rho1, phi0, phi1 of the oracle's solve at tol 1e-4, the exact cost)"""
    from oracle import driver as OD
    (rho0, rho1), nt = CERTIFICATE[case]()
    ny, nx = rho0.shape
    var = OD.solve_single_level(rho0, rho1, nt, dict(tol=1e-4))[0]
    phi = var.phi.reshape((ny, nx, nt), order="F")
    return rho0, rho1, phi[:, :, 0].copy(), phi[:, :, -1].copy(), _exact_w2(rho0, rho1)


@pytest.mark.parametrize("case", sorted(CERTIFICATE))
def test_the_bracket_encloses_the_exact_discrete_cost(case):
    rho0, rho1, phi0, phi1, exact = _solved(case)
    d = DU.dual_bound(phi0, phi1, rho0, rho1)
    u = U.upper_bound(phi0, rho0, rho1, eps_h2=0.25, max_sweeps=200)
    print(case, "bound %.9g <= exact %.9g <= upper %.9g  (upper / exact %.5f)" % (d["bound"], exact, u["upper"], u["upper"] / exact))
    print(str(u))
    assert d["bound"] <= exact + 1e-12
    assert exact <= u["upper"] + 1e-12
    assert u["upper"] <= 1.05 * exact                          # a cap that keeps a vacuous bound from passing, not a measurement
    assert u["sweeps"] == 200 and u["nonfinite"] == 0
    _check_plan(u, rho0, rho1, case + " warm")
    # the warm start is what makes it tight: the same sweeps from zeros end further away
    cold = U.upper_bound(None, rho0, rho1, eps_h2=0.25, max_sweeps=50, start=0)
    warm = U.upper_bound(phi0, rho0, rho1, eps_h2=0.25, max_sweeps=50)
    print("   50 sweeps: cold %.5f, warm %.5f of exact" % (cold["upper"] / exact, warm["upper"] / exact))
    assert exact <= warm["upper"] + 1e-12 and exact <= cold["upper"] + 1e-12
    # start = 2 with f_start = -phi0 is start = 1
    same = U.upper_bound(None, rho0, rho1, eps_h2=0.25, max_sweeps=50, start=2, f_start=-phi0)
    assert same["upper"] == warm["upper"] and np.array_equal(same["f"], warm["f"])


def test_cold_1d_box_to_gaussian_with_empty_nodes():
    n = 33
    x = np.linspace(0.0, 1.0, n)
    rho0 = ((x >= 0.125) & (x <= 0.5)).astype(np.float64)
    rho1 = np.exp(-0.5 * ((x - 0.65) / 0.08) ** 2)
    rho1[rho1 < 1e-3] = 0.0
    assert (rho0 == 0).sum() > 4 and (rho1 == 0).sum() > 4 and rho1[0] == 0.0 and rho1[-1] == 0.0
    exact = _exact_w2(rho0, rho1)
    u = U.upper_bound(None, rho0, rho1, eps_h2=0.25, max_sweeps=200, start=0)
    print("1-D cold: exact %.9g  upper %.9g  (%.5f)" % (exact, u["upper"], u["upper"] / exact))
    print(str(u))
    assert exact <= u["upper"] + 1e-12 and u["upper"] <= 1.05 * exact
    assert u["zero0"] == (rho0 == 0).sum() and u["zero1"] == (rho1 == 0).sum()
    _check_plan(u, rho0, rho1, "1-D cold")


def test_long_double_runs_the_same_code():
    rng = np.random.default_rng(8)
    rho0, rho1 = _densities(rng, (7, 5), zeros=1)
    u = U.sinkhorn_round(rho0, rho1, None, max_sweeps=3)
    v = U.sinkhorn_round(rho0, rho1, None, max_sweeps=3, dtype=np.longdouble)
    assert v["f"].dtype == np.longdouble and v["sweeps"] == 3
    assert abs(float(v["upper"]) - u["upper"]) <= 1e-12 * u["upper"]
    assert np.max(np.abs(v["f"].astype(np.float64) - u["f"])) <= 1e-13


def test_refusals():
    ok = np.ones((3, 4))
    f = np.zeros((3, 4))
    for kw in (dict(eps_h2=0.0), dict(eps_h2=-1.0), dict(eps_h2=np.inf), dict(eps_h2=np.nan), dict(max_sweeps=-1),
               dict(start=3), dict(start=-1), dict(start=2), dict(start=2, f_start=np.zeros((3, 3)))):
        with pytest.raises(ValueError):
            U.upper_bound(f, ok, ok, **kw)
    with pytest.raises(ValueError):
        U.upper_bound(None, ok, ok, start=1)                    # no potential to start from
    for r0, r1 in ((np.zeros((3, 4)), ok), (ok, np.full((3, 4), np.inf)), (ok, -ok), (ok, np.ones((3, 5))), (np.ones((3, 1)), np.ones((3, 1)))):
        with pytest.raises(ValueError):
            U.upper_bound(None, r0, r1, start=0)
    bad = ok.copy()
    bad[1, 1] = -1e-3
    with pytest.raises(ValueError):
        U.sinkhorn_round(bad, ok)
    bad[1, 1] = np.nan
    with pytest.raises(ValueError):
        U.sinkhorn_round(ok, bad)
    with pytest.raises(ValueError):
        U.soft_transform(np.zeros((3, 1)), 1.0)
    with pytest.raises(ValueError):
        U.soft_transform(f, 0.0)
