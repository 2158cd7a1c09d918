"""The multilevel transfer on generic states: the cases, the oracle's expected fine state and the rounding bounds that
tests/test_transfer_conditions.py (CPU) and tests/test_gpu_transfer.py (device) share.

TEST INFRASTRUCTURE (see oracle/__init__.py).  A transfer case is a finished coarse level (a free-running loop from the
generic start of oracle/generic_state.py) and the fine problem it is jumped to.  `expected()` applies the reference's own
sequence -- recoverOrgVar, jump_nextLevel, InitialScaling with the coarse level's last KKT row -- to ANY finished coarse
state given as arrays: to the oracle's own (CPU test) or to the one a device run downloaded (GPU test), so that the
reference and the kernels start from the same bits.

The bounds.  u = 2^-53.  Every chain below is the same real-number expression on both sides; |device - oracle| is at most
the sum of the two sides' rounding errors, each a number of roundings times u times the magnitude the rounding acts on
(first order in u; halvings and negations are exact, a factor that is the same double on both sides still counts once per
side).  Roundings per side:
  phi    sc_in * phi_c (1), at most three additions -- y, x, t (3), the factor 1/dScale (1), its product (1): 6.
         c_phi = 12, against max|phi_f|: every intermediate is a mean of scaled coarse values, and those are fine values.
  beta   sigma * beta_c (1), the factor cScale*E (1), its product (1), at most two additions -- y, x; nearest in t -- (2),
         the factor 1/cScale/E (2), its product (1): 8.  c_beta = 16, against max|beta_f|.
  q      the oracle: phiR (4), 1/h from h = 1/(n-1) (2), one product per term (1), the sum (1), the factor D/dScale (1),
         its product (1): 10.  The device: phiR (4), 1/dScale and its product (2), the coefficient D*(1/h) (3), one product
         per term (1), the sum (1): 11.  c_q = 21 -- but a difference of two phi values is held to the size of its TERMS,
         not of the result: per entry against (D/dScale) (1/h_dir) 2 max|phiR|, h_dir the mesh width of the entry's
         direction.  (Stated against max|q| the constant is c_q kappa_q with kappa_q = that magnitude / max|q|, the
         condition of the difference; both are printed.)
  alpha  betaR (5), at most four terms per adjoint sum (3), the edge factor's product (1), the factor 1/cScale/D (2), its
         product (1): 12.  c_alpha = 24, per entry against (1/cScale/D) S max|betaR| with S = 2 for the cell entries (two
         terms) and 4 * 0.7071... for the edge entries (four terms times the edge factor).
  Weighted problems divide q and alpha by the weight, entry by entry: one more rounding per side (c + 2), and the bound of
  an entry is the unweighted magnitude above DIVIDED BY THAT ENTRY'S WEIGHT.  A bound against max|q| alone would leave the
  barrier entries, 1e6 times smaller than the rest, unchecked to six digits: a kernel that skipped or misplaced the
  division there would pass.
  The scale factors of the fine level come from the package on the device's side and from the oracle on the other; they
  are asserted equal to 1e-15 relative, and what they do differ by (host numbers, no device output) is added to every
  constant in units of u.
"""
import numpy as np

from . import driver as OD
from . import generic_state as G
from . import mexops
from . import multilevel as OML
from .model import initialize

U = 2.0 ** -53
EDGE = 0.707106781186548            # oracle/mex_kernels.c: EDGE_FACTOR
C_PHI, C_BETA, C_Q, C_ALPHA, C_WEIGHT = 12, 16, 21, 24, 2

# name -> the coarse case of oracle/generic_state.CASES (or a spec of its own) ; the fine grid is 2 (n - 1) + 1 of it
TRANSFERS = {
    "66x10x6": dict(coarse="inPALM-66x10x6"),                      # -> 131 x 19 x 11, both levels pitched (80, 144)
    "1d-150x7": dict(coarse="inPALM-1d-150x7"),                    # -> 299 x 13
    "weighted-66x10x6": dict(coarse="inPALM-weighted-66x10x6"),    # -> 131 x 19 x 11, 1e6 barrier weights
    "40x12x13": dict(coarse="inPALM-40x12x13"),                    # -> 79 x 23 x 25, the time-slab grid
    "128x32x5": dict(coarse="inPALM-128x32x5"),                    # -> 255 x 63 x 9, cone columns Nz + 48 apart
    # the smallest grid: densities as tests/test_gpu_canary.py builds them for ny * nx <= 6
    "3x2x2": dict(coarse=None, spec=dict(method="inPALM", shape=(3, 2, 2), K=7)),
}
WARM_K = 7                          # iterations of the fine loop after the transfer: checks at 1, 4, 7
# The oracle's own sensitivity: a one-ulp perturbation of the coarse state that is jumped moves the fields after WARM_K fine
# iterations by at most this share of their max-abs (asserted in tests/test_transfer_conditions.py).  Measured: 1.4e-13
# (alpha, 40 x 12 x 13 -> 79 x 23 x 25), the figure of 66 x 10 x 6 -> 131 x 19 x 11 is in DESIGN.md; rounded up to one digit.
# The device is held to 100 times it, the rule of tests/test_gpu_generic_state.py.
WARM_SENSITIVITY = 2e-13
WARM_CASES = ("66x10x6", "40x12x13")
# KKT column 5 (index 4), sigma ||F*B*beta + D_w alpha||: the jump sets alpha = -F*B*beta ./ w, so the column starts at zero,
# and the oracle's own history keeps it at 1e-16 .. 2e-15 through the first seven iterations.  Rounding noise has no relative
# error to speak of; it is held below NOISE on both sides, as tests/test_gpu_generic_state.py holds the cancelling column of
# ALG2 and acc-ADMM.
WARM_CANCELLING = (4,)
NOISE = 1e-13


def _tiny(ny, nx):
    rho0 = np.ones((ny, nx))
    rho1 = np.ones((ny, nx))
    rho1.flat[0] = 1.5
    rho1 /= rho1.mean()
    return rho0, rho1


def spec(name):
    t = TRANSFERS[name]
    return G.CASES[t["coarse"]] if t["coarse"] else t["spec"]


def coarse_problem(name):
    t = TRANSFERS[name]
    if t["coarse"]:
        return G.problem(t["coarse"])
    ny, nx, nt = t["spec"]["shape"]
    return _tiny(ny, nx) + (nt, None)


def fine_shape(name):
    return tuple(2 * (n - 1) + 1 for n in spec(name)["shape"])


def fine_problem(name):
    """(rho0, rho1, nt, weight) of the fine level: the same example on the finer grid."""
    from .examples import (ensure_barrier_validity, gene_barrier_of_circle_pillar, get_example_1d, get_example_2d,
                           get_weight_by_barrier)
    s, shape = spec(name), fine_shape(name)
    if len(shape) == 2:
        rho0, rho1 = get_example_1d("gaussian", shape[0])
        return rho0, rho1, shape[1], None
    ny, nx, nt = shape
    if TRANSFERS[name]["coarse"] is None:
        return _tiny(ny, nx) + (nt, None)
    rho0, rho1 = get_example_2d("example1", ny, nx)
    weight = None
    if s.get("weighted"):
        barrier = gene_barrier_of_circle_pillar()
        weight = get_weight_by_barrier(nx, ny, nt, barrier)
        rho0, rho1, _ = ensure_barrier_validity(rho0, rho1, barrier)
    return rho0, rho1, nt, weight


def holes(shape, dims):
    """cone_holes of oracle/generic_state.py without its size check (on 3 x 2 x 2 a third of the slots are holes)."""
    probe = np.full(shape, np.nan, order="F")
    if len(dims) == 2:
        mexops.mexBFd1d(probe, np.zeros(dims[1] * (dims[0] - 1) + (dims[1] - 1) * dims[0]), dims[1], dims[0])
    else:
        ny, nx, nt = dims
        mexops.mexBFd(probe, np.zeros(ny * nx * (nt - 1) + ny * (nx - 1) * nt + (ny - 1) * nx * nt), nt, nx, ny)
    return np.isnan(probe)


def coarse_start(name, var):
    s = spec(name)
    if TRANSFERS[name]["coarse"]:
        return G.oracle_run(TRANSFERS[name]["coarse"])["start"]
    amp = dict(G.AMPLITUDES, **(s.get("amplitudes") or {}))
    rng = np.random.default_rng(G.DEFAULT_SEED)
    start = {f: np.asfortranarray(amp[f] * rng.standard_normal(np.shape(getattr(var, f)))) for f in ("phi", "q", "alpha", "z", "beta")}
    hole = holes(start["beta"].shape, s["shape"])
    start["z"][hole] = 0.0
    start["beta"][hole] = 0.0
    return start


_coarse = {}


def coarse_run(name):
    """The oracle's finished coarse level of a case (once per process, read-only): dict var, hist, sigma, start."""
    if name in _coarse:
        return _coarse[name]
    t = TRANSFERS[name]
    if t["coarse"]:
        run = G.oracle_run(t["coarse"])
    else:
        s = t["spec"]
        rho0, rho1, nt, weight = coarse_problem(name)
        var, model, o = OD.make_level(rho0, rho1, nt, dict(tol=0.0, maxit=s["K"]), s["method"], weight)
        start = coarse_start(name, var)
        G.set_state(var, start)
        st = OD.make_state(var, o, model, s["method"], weighted=False)
        st.run()
        hist, sigma = st.finish()
        run = dict(var=var, start=start, hist=hist, sigma=sigma, weight=None, opts=o)
    _coarse[name] = run
    return run


def finished(var):
    """What expected() takes from a finished level: the five arrays (alpha, beta already times sigma) and its scalars."""
    return ({f: np.array(getattr(var, f), order="F") for f in G.FIELDS},
            {k: float(getattr(var, k)) for k in ("cScale", "dScale", "D", "E", "E2")})


def expected(name, fields, scalars, last_kkt):
    """recoverOrgVar -> jump_nextLevel -> InitialScaling on copies of a finished coarse state.  Returns (var, model, raw):
    the fine level as the fine loop starts from it, and raw = dict(phi, beta, recovered): phiR and betaR before
    InitialScaling (the magnitudes the bounds of q and alpha are stated against) and the recovered coarse arrays."""
    s = spec(name)
    rho0, rho1, nt, _ = coarse_problem(name)
    var, model = initialize(rho0, rho1, nt)
    for f in G.FIELDS:
        setattr(var, f, np.array(fields[f], order="F"))
    for k, v in scalars.items():
        setattr(var, k, v)
    OD.recoverOrgVar(var)
    recovered = {f: getattr(var, f).copy(order="F") for f in G.FIELDS}
    rho0f, rho1f, ntf, wf = fine_problem(name)
    var, modelR = OML.jump_nextLevel(var, model, rho0f, rho1f, ntf, wf)
    raw = dict(phi=var.phi.copy(), beta=var.beta.copy(order="F"), recovered=recovered)
    OD.InitialScaling(var, modelR, True, np.asarray(last_kkt), dim=len(s["shape"]) - 1, weighted=wf is not None)
    return var, modelR, raw


def bounds(name, var, raw, weight=None, scale_slack=0.0):
    """Per field the bound on |device - oracle| (a number, or an array with one bound per entry) and the constant c that,
    times u max|field|, gives its largest entry -- see the module docstring.  var, raw: of expected()."""
    shape = fine_shape(name)
    nt = shape[-1]
    sp = shape[:-1]
    ncell = int(np.prod(sp)) * (nt - 1)
    cw = C_WEIGHT if weight is not None else 0
    b = {"phi": (C_PHI + scale_slack) * U * np.max(np.abs(var.phi)),
         "beta": (C_BETA + scale_slack) * U * np.max(np.abs(var.beta))}
    pmax, bmax = np.max(np.abs(raw["phi"])), np.max(np.abs(raw["beta"]))
    # q = [t differences (cells) | x differences | y differences], alpha alike
    nq = var.q.size
    inv_h = np.empty(nq)
    terms = np.empty(nq)
    inv_h[:ncell], terms[:ncell] = float(nt - 1), 2.0
    if len(shape) == 2:
        inv_h[ncell:], terms[ncell:] = float(shape[0] - 1), 4.0 * EDGE
    else:
        ny, nx, _ = shape
        nbx = ny * (nx - 1) * nt
        inv_h[ncell:ncell + nbx], inv_h[ncell + nbx:] = float(nx - 1), float(ny - 1)
        terms[ncell:] = 4.0 * EDGE
    w = 1.0 if weight is None else np.asarray(weight)
    b["q"] = (C_Q + cw + scale_slack) * U * (var.D / var.dScale) * inv_h * 2.0 * pmax / w
    b["alpha"] = (C_ALPHA + cw + scale_slack) * U * (1.0 / var.cScale / var.D) * terms * bmax / w
    return b


def worst(err, bound):
    """Largest error as a share of its bound (entry by entry where the bound is an array)."""
    return float(np.max(np.abs(err) / bound))


def kappa(name, var, b, weight=None):
    """The condition numbers that turn the bounds of q and alpha into multiples of u max|field|."""
    cw = C_WEIGHT if weight is not None else 0
    return {"q": float(np.max(b["q"]) / ((C_Q + cw) * U * np.max(np.abs(var.q)))),
            "alpha": float(np.max(b["alpha"]) / ((C_ALPHA + cw) * U * np.max(np.abs(var.alpha))))}


def warm_opts(name, sigma):
    """The options of the fine loop after the jump: solver_dotsocp2d.m:245 for sigma, WARM_K iterations, no stop."""
    s = spec(name)
    o = OD.default_opts(dict(tol=0.0, maxit=WARM_K), s["method"], s.get("weighted", False))
    o["sigma"] = 10 ** (np.log10(o["sigma"] * sigma) / 2)
    return o


def warm_run(name, fields, scalars, last_kkt, sigma):
    """The oracle's fine loop, WARM_K iterations from its own transfer of the given coarse state: (var, hist, sigma)."""
    s = spec(name)
    var, modelR, _ = expected(name, fields, scalars, last_kkt)
    st = OD.make_state(var, warm_opts(name, sigma), modelR, s["method"], weighted=s.get("weighted", False))
    st.run()
    hist, sig = st.finish()
    return var, hist, sig
