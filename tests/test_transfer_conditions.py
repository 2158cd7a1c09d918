"""The inputs of tests/test_gpu_transfer.py do their job, and its bounds can fail: with the oracle alone (no device), for
every transfer case of oracle/transfer_state.py,

  * the finished coarse state that is jumped has no zero entry in phi and none in beta outside the slots mexBFd leaves
    unwritten, and the oracle's fine beta is zero exactly in the fine grid's such slots;
  * the factors that enter the transfer -- sigma, dScale and cScale * E of the coarse level; 1 / dScale, 1 / cScale / E,
    1 / cScale / D and D / dScale of the fine level -- differ from 1 by more than 1 %, and so does every pair of them from
    each other: a dropped or swapped factor then shows.  NOT in every single case, and it cannot be: a first level has
    dScale = sqrt(2) E = D identically (InitialScaling with Escale2 = sqrt(2)), cScale = max(1, .) is clamped to 1 on the
    weighted and the smallest grid, and where the KKT ratio of the coarse level hits the clamp of InitialScaling the fine
    level has D = E.  Asserted is that every factor and every pair is told apart by at least one case (the weighted and the
    3 x 2 x 2 -> 5 x 3 x 3 case have D != E on the fine level);
  * deliberately wrong transfers -- beta linear in t instead of nearest, its cell index off by one, the odd phi layers taken
    from layer tc alone, the y and the x neighbour swapped, sigma left out, the cone columns read Nz apart where they are
    stored Nz + 48 apart -- miss the bound of the GPU test by at least a factor 1e3 on at least one field.  The variants are
    small numpy functions put in the place of the reference's interpolation, or applied to its input;
  * the fine loop after the jump is not rounding-sensitive: a one-ulp perturbation of the coarse state moves the fields
    after its first 7 iterations by <= oracle/transfer_state.WARM_SENSITIVITY of their max-abs; the GPU test allows 100 x.
"""
import itertools

import numpy as np
import pytest

from oracle import generic_state as G
from oracle import multilevel as OML
from oracle import transfer_state as T

CASES = list(T.TRANSFERS)
FOUR = ("phi", "q", "alpha", "beta")
MISS = 1e3


def _coarse(name):
    run = T.coarse_run(name)
    fields, scalars = T.finished(run["var"])
    return run, fields, scalars


_right = {}


def _expected(name):
    if name not in _right:
        run, fields, scalars = _coarse(name)
        var, model, raw = T.expected(name, fields, scalars, run["hist"]["kkt"][-1])
        weight = T.fine_problem(name)[3]
        _right[name] = (var, raw, T.bounds(name, var, raw, weight), weight)
    return _right[name]


@pytest.mark.parametrize("name", CASES)
def test_the_coarse_state_is_generic(name):
    run, fields, _ = _coarse(name)
    shape = T.spec(name)["shape"]
    hole = T.holes(fields["beta"].shape, shape)
    assert np.all(fields["phi"] != 0.0)
    assert np.all(fields["beta"][~hole] != 0.0) and np.all(fields["beta"][hole] == 0.0)
    assert run["hist"]["iter"][-1] == T.spec(name)["K"]
    var, raw, bounds, weight = _expected(name)
    fhole = T.holes(var.beta.shape, T.fine_shape(name))
    assert np.all(var.beta[fhole] == 0.0) and np.all(var.beta[~fhole] != 0.0)
    assert np.all(var.z == 0.0) and np.all(var.phi != 0.0)
    k = T.kappa(name, var, bounds, weight)
    print("\n%s -> %s: kappa_q %.1f kappa_alpha %.2f" % (name, "x".join(map(str, T.fine_shape(name))), k["q"], k["alpha"]))
    # the bounds of q and alpha stay useful multiples of u max|field|
    assert k["q"] <= 500 and k["alpha"] <= 10
    if weight is not None:
        assert (weight == 1e6).sum() > 0


def _factors(name):
    run, _, c = _coarse(name)
    f = _expected(name)[0]
    return {"sigma_c": run["sigma"], "dScale_c": c["dScale"], "cScale_c*E_c": c["cScale"] * c["E"],
            "1/dScale_f": 1.0 / f.dScale, "1/cScale_f/E_f": 1.0 / f.cScale / f.E, "1/cScale_f/D_f": 1.0 / f.cScale / f.D,
            "D_f/dScale_f": f.D / f.dScale}


def test_every_factor_is_told_apart_somewhere():
    fac = {name: _factors(name) for name in CASES}
    names = list(next(iter(fac.values())))
    for name, f in fac.items():
        print("\n%s: %s" % (name, "  ".join("%s %.4f" % kv for kv in f.items())))
    apart = lambda a, b: abs(a - b) > 1e-2 * max(abs(a), abs(b))        # noqa: E731
    for k in names:
        assert any(apart(f[k], 1.0) for f in fac.values()), k
        # sigma, the only factor a transfer can drop without a trace in the scalars, differs from 1 in EVERY case
        assert k != "sigma_c" or all(apart(f[k], 1.0) for f in fac.values())
    for a, b in itertools.combinations(names, 2):
        assert any(apart(f[a], f[b]) for f in fac.values()), (a, b)
    # D and E of the fine level themselves
    assert sum(apart(_expected(n)[0].D, _expected(n)[0].E) for n in CASES) >= 2


# --------------------------------------------------------------------------------------------------
# wrong transfers
# --------------------------------------------------------------------------------------------------
_stagger, _phi, _mean2 = OML._interpolate_tStagger, OML.interpolate_phi, OML._movmean2


def _beta_linear_in_t(f):
    """cell-centred linear interpolation along t (weights 3/4, 1/4; clamped at the ends) instead of nearest"""
    r = _stagger(f)
    n = r.shape[-1]
    k = np.arange(n)
    other = np.clip(np.where(k % 2 == 0, k - 1, k + 1), 0, n - 1)
    return 0.75 * r + 0.25 * r[..., other]


def _beta_cell_off_by_one(f):
    r = _stagger(f)
    n = r.shape[-1]
    return r[..., np.minimum(np.arange(n) + 1, n - 1)]


def _phi_odd_layers_from_tc(phi, dims):
    ntR = 2 * (dims[-1] - 1) + 1
    r = _phi(phi, dims).reshape((-1, ntR), order="F").copy(order="F")
    r[:, 1::2] = r[:, 0:-1:2]
    return r.reshape(-1, order="F")


def _neighbours_swapped(f, d):
    """the mean of neighbouring pairs along d taken with the neighbour along the OTHER space axis"""
    if f.ndim != 3 or d == 2:
        return _mean2(f, d)
    o = 1 - d
    n = f.shape[o]
    nb = np.take(f, np.minimum(np.arange(n) + 1, n - 1), axis=o)
    cut = [slice(None)] * 3
    cut[d] = slice(0, f.shape[d] - 1)
    return ((f + nb) / 2.0)[tuple(cut)]


def _columns_nz_apart(beta):
    """the ten columns stored Nz + 48 apart (zeros in the gaps) and read Nz apart"""
    nz, k = beta.shape
    flat = np.zeros((nz + 48) * k)
    for j in range(k):
        flat[j * (nz + 48):j * (nz + 48) + nz] = beta[:, j]
    return np.asfortranarray(flat[:nz * k].reshape((nz, k), order="F"))


VARIANTS = {
    "beta-linear-in-t": dict(patch=("_interpolate_tStagger", _beta_linear_in_t), cells=2),
    "beta-cell-off-by-one": dict(patch=("_interpolate_tStagger", _beta_cell_off_by_one), cells=2),
    "phi-odd-layers-from-tc": dict(patch=("interpolate_phi", _phi_odd_layers_from_tc)),
    "xy-neighbours-swapped": dict(patch=("_movmean2", _neighbours_swapped), only_2d=True),
    "sigma-missing": dict(beta=lambda b, run: b / run["sigma"]),
    "columns-Nz-apart": dict(beta=lambda b, run: _columns_nz_apart(b), only=("128x32x5",)),
}


def _applies(name, variant):
    """the swap needs two space axes; the misread column stride a grid whose columns are NOT Nz apart on the device; another
    rule along t two coarse cells (3 x 2 x 2 has one: it feeds both fine cells under either rule)"""
    v, shape = VARIANTS[variant], T.spec(name)["shape"]
    return (not (v.get("only_2d") and len(shape) == 2) and ("only" not in v or name in v["only"])
            and shape[-1] - 1 >= v.get("cells", 1))


def test_the_padded_case_is_the_only_padded_one():
    for name in CASES:
        shape = T.spec(name)["shape"]
        assert (len(shape) == 3 and shape[0] * shape[1] >= 4096) == (name in VARIANTS["columns-Nz-apart"]["only"])


@pytest.mark.parametrize("name,variant", [(n, v) for v in VARIANTS for n in CASES if _applies(n, v)])
def test_a_wrong_transfer_misses_the_bound(name, variant, monkeypatch):
    v = VARIANTS[variant]
    shape = T.spec(name)["shape"]
    run, fields, scalars = _coarse(name)
    var, raw, bounds, weight = _expected(name)
    if "patch" in v:
        monkeypatch.setattr(OML, *v["patch"])
    if "beta" in v:
        fields = dict(fields, beta=v["beta"](fields["beta"], run))
    wrong, _, _ = T.expected(name, fields, scalars, run["hist"]["kkt"][-1])
    miss = {f: T.worst(getattr(wrong, f) - getattr(var, f), bounds[f]) for f in FOUR}
    print("\n%s [%s]: error / bound  %s" % (name, variant, "  ".join("%s %.1e" % kv for kv in miss.items())))
    assert max(miss.values()) >= MISS, miss
    if variant == "xy-neighbours-swapped":
        assert shape[0] != shape[1]                   # on a square, symmetric state the swap could cancel
        assert miss["phi"] >= MISS and miss["beta"] >= MISS


def test_the_unpatched_sequence_is_the_reference():
    """expected() run twice gives the same bits: the variants above differ because of what they change, nothing else."""
    name = "66x10x6"
    run, fields, scalars = _coarse(name)
    again, _, _ = T.expected(name, fields, scalars, run["hist"]["kkt"][-1])
    for f in G.FIELDS:
        np.testing.assert_array_equal(getattr(again, f), getattr(_expected(name)[0], f))


# --------------------------------------------------------------------------------------------------
# the warm start's sensitivity
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.WARM_CASES)
def test_the_warm_start_is_not_rounding_sensitive(name):
    run, fields, scalars = _coarse(name)
    last = run["hist"]["kkt"][-1]
    var, hist, sigma = T.warm_run(name, fields, scalars, last, run["sigma"])
    twin_fields = G.perturbed(fields)
    assert any(np.any(twin_fields[f] != fields[f]) for f in G.FIELDS)
    twin, thist, tsigma = T.warm_run(name, twin_fields, scalars, last, run["sigma"])
    np.testing.assert_array_equal(hist["iter"], [1, 4, 7])
    np.testing.assert_array_equal(thist["iter"], hist["iter"])
    moved = {f: np.max(np.abs(getattr(twin, f) - getattr(var, f))) / np.max(np.abs(getattr(var, f))) for f in G.FIELDS}
    generic = [c for c in range(7) if c not in T.WARM_CANCELLING]
    kmoved = np.max((np.abs(thist["kkt"] - hist["kkt"]) / hist["kkt"])[:, generic])
    print("\n%s: one-ulp perturbation of the coarse state moves the fine fields after %d iterations by %s, the KKT history by "
          "%.1e, sigma by %.1e" % (name, T.WARM_K, " ".join("%s %.1e" % kv for kv in moved.items()), kmoved,
                                  abs(tsigma - sigma) / sigma))
    assert hist["kkt"][:, generic].min() >= 1e-3      # these columns are generic: the relative comparison means something
    for c in T.WARM_CANCELLING:                       # ... and this one is rounding noise (oracle/transfer_state.py)
        assert np.all(hist["kkt"][:, c] <= T.NOISE) and np.all(thist["kkt"][:, c] <= T.NOISE)
    assert max(moved.values()) <= T.WARM_SENSITIVITY, moved
    assert kmoved <= 1e-12
    # the loop did move the transferred state
    start = _expected(name)[0]
    assert np.max(np.abs(var.q - start.q)) > 1e-2 * np.max(np.abs(start.q))
