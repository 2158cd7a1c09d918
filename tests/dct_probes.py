"""Probes and long-double references for the one-axis DCT passes (dotsocp_dct_axis), entry by entry.

White noise makes every output entry O(1), so a bar of 1e-13 sqrt(size) lets an error of 1e4 ulp through in any single
entry.  The probes here have outputs whose every entry is known in closed form and small:

  (A)  impulses: line l of a batch is a unit impulse at position p_l.  Forward the answer is column p_l of the orthonormal
       DCT-II matrix, c_k cos(pi k (2 p_l + 1) / 2n), inverse (an impulse at bin k) it is row k; the entries have size
       u = sqrt(2 / n).  The positions: the ends and the middle of the line, both sides of every internal boundary of the
       family that serves the length (boundaries()), and 16 seeded random ones.
  (A') the same batches with every second line scaled by 2^-30 (exact): all FFT families pack two real lines into one
       complex line, and the error of the small line, measured on the scale of its unit partner, shows their cross-talk.
  (B)  dynamic range: forward x = fl(v_1 + 2^-20 v_k), k in {2, n/2, n-3} (v_k: the k-th basis vector) -- what a Poisson
       right-hand side looks like -- checked at the bins {0, 1, 2, k-1, k, k+1, n/2, n-1} and at seeded random ones
       against the long-double dot product of the ROUNDED x with the basis vector; inverse the spectrum e_1 + 2^-20 e_k,
       every entry against the exact sum.

References: np.longdouble throughout, PI = 4 arctan(1), the argument reduced exactly in integers, m = (2j+1) k mod 4n.

Figures: E = max entry error / (eps * scale), eps = 2^-52, scale = u * amplitude for (A) (the amplitude of the line; of
its unit partner in (A')) and for the inverse (B), ||x||_2 for the forward (B).  E is computed for the device, for scipy
and -- up to n = 65537 -- for the numpy model of the family (tools/*_proto.py: dct2 / dct3 on the same pairs of lines; the
power-of-two transforms inside the LDS have none) on
the very same arrays; the device must stay within 4 x the larger of the two CPU figures (the kernels run radix-4/8/16
register butterflies with contraction, in another order than the radix-2 models; scipy and the models differ by about 2
among themselves).  For (B) the bound is not below 4 eps ||x||_inf, x the signal in the time domain.  The dense family
has its own bound in (A) and (A'): an impulse makes every product a table entry times one, so each entry must be within
1 ulp of the long-double value (plus 2^-59 u, the accuracy of a long-double cosine: _ulp_excess).

No device code here: measure() takes the transform as a callable.  `python -m dct_probes OUT.npz CASE...` (from tests/)
runs the cases on the device in a process of its own -- the switches of the dispatcher are read once per process -- and
writes the figures."""
import functools
import math
import os
import sys

import numpy as np
import scipy.fft as sfft

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

LD = np.longdouble
PI = 4 * np.arctan(LD(1))
EPS = 2.0 ** -52
SMALL = 2.0 ** -30          # (A'): every second line
TINY = 2.0 ** -20           # (B): the second component
MODEL_MAX_N = 65537
MARGIN = 4.0

FAMILIES = ("fft1", "fft2", "pfa", "rader", "bluestein1", "bluestein2", "dense")
PFA_FACTORS = {1025: (25, 41), 513: (27, 19), 129: (3, 43), 65: (5, 13), 33: (3, 11), 17: (1, 17), 9: (9, 1), 5: (5, 1),
               3: (3, 1)}


# ---------------------------------------------------------------------------------------------- cases
# (family, (ny, nx, nt), axis[, positions]): the transform runs along `axis`, the other two extents give the lines.  Which
# kernel instance each shape takes is written down in tests/test_gpu_dct_probes.py.  The number of lines is odd -- the
# last line has no partner -- except where the instance asks otherwise: EVEN says why.
CASES = {
    "fft1": [((8, 9, 1), 0), ((64, 9, 1), 0), ((64, 65, 1), 0), ((1024, 9, 1), 0), ((1024, 1, 1), 0),
             ((128, 9, 1), 0), ((512, 9, 1), 0), ((2048, 9, 1), 0),
             ((9, 8, 1), 1), ((10, 8, 1), 1), ((9, 64, 1), 1), ((10, 64, 1), 1), ((32, 64, 1), 1), ((9, 1024, 1), 1),
             ((10, 1024, 1), 1), ((16, 1024, 1), 1), ((10, 2048, 1), 1),
             ((3, 3, 8), 2), ((2, 5, 64), 2), ((3, 3, 1024), 2), ((2, 8, 1024), 2)],
    "fft1-pipe": [((128, 32768, 1), 0), ((512, 8192, 1), 0), ((2048, 2048, 1), 0),
                  ((512, 128, 64), 1), ((512, 512, 16), 1), ((2048, 2048, 1), 1),
                  # 256 and 1024: the lengths of the parity-gate grid and of the benchmark grid
                  ((256, 16384, 1), 0), ((1024, 4096, 1), 0), ((512, 256, 32), 1), ((512, 1024, 8), 1)],
    "fft2": [((4096, 9, 1), 0), ((8192, 9, 1), 0), ((33, 16384, 1), 1), ((3, 3, 16384), 2), ((65536, 5, 1), 0, 14),
             ((1 << 19, 5, 1), 0, 8), ((1 << 20, 5, 1), 0, 8)],
    "pfa": [c for n in (1025, 513, 129, 17, 3) for c in (((n, 9, 1), 0), ((9, n, 1), 1), ((10, n, 1), 1), ((3, 3, n), 2))] +
           [((2, 5, 129), 2)],
    "rader": [((257, 9, 1), 0), ((9, 257, 1), 1), ((3, 3, 257), 2)],
    "bluestein1": [c for n in (500, 1000, 1023) for c in (((n, 9, 1), 0), ((9, n, 1), 1), ((3, 3, n), 2))],
    "bluestein2": [((4101, 9, 1), 0), ((9, 4101, 1), 1), ((3, 3, 4101), 2), ((65537, 5, 1), 0, 14), ((524287, 5, 1), 0, 5)],
    "dense": [((47, 31, 1), 0), ((31, 47, 1), 1), ((47, 515, 1), 0), ((515, 47, 1), 1)] +
             [c for n in (48, 96, 1026) for c in (((n, 63, 1), 0), ((63, n, 1), 1), ((n, 130, 1), 0), ((130, n, 1), 1))] +
             [((99, 130, 1), 0), ((130, 99, 1), 1), ((5, 26, 96), 2)],
}
EVEN = "a 16-byte access carries both lines of a pair (the `vec` instances), whole tiles (the pipelined ones), or the " \
       "130 lines of the ragged MFMA tiles"
# the switches of the dispatcher are read once per process: (environment, family that must serve the lengths, cases)
SWITCHED = {
    "dct_long_min_256": (dict(DOTSOCP_DCT_LONG_MIN="256"), "fft2",
                         [((256, 9, 1), 0), ((9, 256, 1), 1), ((512, 9, 1), 0), ((10, 512, 1), 1), ((2048, 9, 1), 0),
                          ((3, 3, 2048), 2)]),
    "cdft_long_min_129": (dict(DOTSOCP_CDFT_LONG_MIN="129"), "bluestein2",
                          [((130, 9, 1), 0), ((1000, 9, 1), 0), ((9, 1000, 1), 1), ((1536, 9, 1), 0), ((1537, 9, 1), 0),
                           ((3, 3, 1537), 2), ((2049, 9, 1), 0)]),
    "cdft_min_48": (dict(DOTSOCP_CDFT_MIN="48"), "bluestein1",
                    [((48, 9, 1), 0), ((9, 48, 1), 1), ((100, 9, 1), 0), ((3, 3, 100), 2)]),
    "pfa_cdft_off": (dict(DOTSOCP_PFA="0", DOTSOCP_CDFT="0"), "dense",
                     [((1025, 63, 1), 0), ((1025, 130, 1), 0), ((130, 1025, 1), 1), ((257, 63, 1), 0), ((257, 130, 1), 0),
                      ((130, 257, 1), 1)]),
}
SWITCHED.update({"dct_pipe_off_%d" % i: (dict(DOTSOCP_DCT_PIPE="0"), "fft1", [c])
                 for i, c in enumerate(CASES["fft1-pipe"])})
SWITCHES = ("DOTSOCP_DCT_LONG_MIN", "DOTSOCP_CDFT_LONG_MIN", "DOTSOCP_CDFT_MIN", "DOTSOCP_DCT_PIPE", "DOTSOCP_PFA",
            "DOTSOCP_CDFT")


def cases_of(group):
    fam = group.split("-")[0]
    return [(fam,) + c for c in CASES[group]]


def all_cases():
    """every case of the GPU tests, the switched ones included"""
    out = [c for g in CASES for c in cases_of(g)]
    for env, fam, cs in SWITCHED.values():
        out += [(fam,) + c for c in cs]
    return out


# ---------------------------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=1)
def _cos_table(n):
    t = np.cos(PI * np.arange(4 * n).astype(LD) / LD(2 * n))
    t.setflags(write=False)
    return t


def _cosm(n, m):
    """cos(pi m / 2n) in long double for an integer array 0 <= m < 4n (many entries: looked up in the table of all 4n)"""
    m = np.asarray(m, dtype=np.int64)
    if m.size > 2 * n:
        return _cos_table(n)[m]
    return np.cos(PI * m.astype(LD) / LD(2 * n))


def _ck(n, k):
    k = np.asarray(k)
    return np.where(k == 0, np.sqrt(LD(1) / n), np.sqrt(LD(2) / n))


def basis_rows(n, ks):
    """[len(ks), n]: the orthonormal DCT-II basis vectors v_k[j] = c_k cos(pi k (2j+1) / 2n)"""
    ks = np.asarray(ks, dtype=np.int64)
    j = np.arange(n, dtype=np.int64)
    m = ((2 * j[None, :] + 1) * ks[:, None]) % (4 * n)
    return _ck(n, ks)[:, None] * _cosm(n, m)


def matrix_columns(n, ps):
    """[len(ps), n]: row i is column ps[i] of the DCT-II matrix, the transform of a unit impulse at ps[i]"""
    ps = np.asarray(ps, dtype=np.int64)
    k = np.arange(n, dtype=np.int64)
    m = ((2 * ps[:, None] + 1) * k[None, :]) % (4 * n)
    return _ck(n, k)[None, :] * _cosm(n, m)


# ---------------------------------------------------------------------------------------------- positions
def split2(N):
    """N = a * b, a >= b powers of two (tools/dct_long_proto.split, tools/cdft_long_proto.split)"""
    lg = N.bit_length() - 1
    return 1 << (lg - lg // 2), 1 << (lg // 2)


def conv_length(n):
    return 1 << (2 * n - 2).bit_length()


def boundaries(family, n):
    """both sides of every internal boundary of the family's index arithmetic at length n, the most telling ones first"""
    if family == "fft2":                               # n = n1 n2, j = j1 n2 + j2, k = k1 + n1 k2
        n1, n2 = split2(n)
        out = [n2 - 1, n2, n2 + 1, n - n2 - 1, n - n2, n1 - 1, n1, n1 + 1]
    elif family == "bluestein2":                       # M = m1 m2; the partner of column j2 is column (n - j2) mod m2
        m1, m2 = split2(conv_length(n))
        r = n % m2
        out = [m2 - 1, m2, m2 + 1, n - m2 - 1, n - m2, r, (r + 1) // 2, (r + 1) // 2 + 1]
    elif family == "pfa":                              # Good-Thomas maps: j = 0 mod N1, j = 0 mod N2
        N1, N2 = PFA_FACTORS[n]
        out = [N1, N2, n - N1, n - N2, N1 - 1, N2 + 1]
    elif family == "bluestein1":                       # chirp exponent j^2 mod 2n: its first wrap
        s = math.isqrt(2 * n)
        out = [s, s + 1, n - 1]
    elif family == "rader":                            # g = 3: g^0, g^1, g^-1 = 86, g^255 = 86, the spare slot of index 0
        out = [1, 3, 86, n - 1, 0]
    elif family == "dense":                            # 64 outputs per MFMA tile of each parity, j chunks of 8
        out = [7, 8, 63, 64, 65, 127, 128, 129]
    else:
        out = []
    return [p for i, p in enumerate(out) if 0 <= p < n and p not in out[:i]]          # in this order: the first ones survive a cut


def generic_positions(n):
    return sorted({p for p in (0, 1, 2, 3, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1) if 0 <= p < n})


def positions(family, n, npos=None, seed=0):
    """the impulse positions of a probe: boundaries first, then the ends and the middle, then 16 seeded random ones (all
    positions up to n = 32); cut to `npos`; an odd number of them"""
    rng = np.random.default_rng(7919 * n + seed)
    P = []
    for p in boundaries(family, n) + generic_positions(n) + (list(range(n)) if n <= 32 else rng.integers(0, n, 16).tolist()):
        if p not in P:
            P.append(int(p))
    if npos is not None:
        P = P[:npos]
    if len(P) % 2 == 0:
        rest = [p for p in range(n) if p not in P]
        P.append(rest[len(rest) // 3] if rest else P[0])
    return P


def batches(m, L):
    """index arrays of length L that cover 0 .. m-1: chunks of L, a short one filled up cyclically; m < L: cycled"""
    if m <= L:
        return [np.arange(L) % m]
    return [np.arange(s, s + L) % m for s in range(0, m, L)]


# ---------------------------------------------------------------------------------------------- probes
class Probe:
    """U: [m, n] float64 lines; ref: [m, n] long double, or (bins, values) lists per line for the forward (B);
    scale[m]: what eps multiplies in E; floor[m]: absolute floor of the bound (0: none)"""

    def __init__(self, kind, inverse, U, ref, scale, floor, bins=None):
        self.kind, self.inverse, self.U, self.ref, self.scale, self.floor, self.bins = kind, inverse, U, ref, scale, floor, bins


@functools.lru_cache(maxsize=2)
def _impulse_probe(family, n, npos, inverse):
    P = positions(family, n, npos)
    U = np.zeros((len(P), n))
    U[np.arange(len(P)), P] = 1.0
    ref = basis_rows(n, P) if inverse else matrix_columns(n, P)
    u = math.sqrt(2.0 / n)
    U.setflags(write=False)
    ref.setflags(write=False)
    return Probe("A", inverse, U, ref, np.full(len(P), u), np.zeros(len(P)))


def b_modes(n):
    ks = [k for k in (2, n // 2, n - 3) if 2 <= k < n]
    ks = sorted(set(ks)) or [n - 1]
    if len(ks) % 2 == 0:
        ks.append(n - 1 if n - 1 not in ks else 1)
    return ks


@functools.lru_cache(maxsize=2)
def _range_probe(family, n, inverse):
    ks = b_modes(n)
    V = basis_rows(n, [1] + ks)
    xt = V[0][None, :] + LD(TINY) * V[1:]                      # the signal in the time domain
    u = math.sqrt(2.0 / n)
    if inverse:
        U = np.zeros((len(ks), n))
        U[:, 1] = 1.0
        for i, k in enumerate(ks):
            U[i, k] += TINY
        floor = MARGIN * EPS * np.max(np.abs(xt), axis=1).astype(np.float64)
        return Probe("B", 1, U, xt, np.full(len(ks), u), floor)
    U = xt.astype(np.float64)
    rng = np.random.default_rng(104729 * n + 1)
    nrand = 16 if n < (1 << 17) else 4
    bins, vals = [], []
    Ul = U.astype(LD)
    for i, k in enumerate(ks):
        b = sorted({q for q in (0, 1, 2, k - 1, k, k + 1, n // 2, n - 1) if 0 <= q < n} | set(rng.integers(0, n, nrand).tolist()))
        B = basis_rows(n, b)
        bins.append(np.array(b))
        vals.append((B * Ul[i][None, :]).sum(axis=1))
    scale = np.sqrt((U * U).sum(axis=1))
    floor = MARGIN * EPS * np.max(np.abs(U), axis=1)
    return Probe("B", 0, U, vals, scale, floor, bins)


def probes(family, n, npos, inverse):
    a = _impulse_probe(family, n, npos, inverse)
    return [a, Probe("A'", a.inverse, a.U, a.ref, a.scale, a.floor), _range_probe(family, n, inverse)]


def line_factors(kind, L):
    """(A'): every second line of a batch times 2^-30"""
    s = np.ones(L)
    if kind == "A'":
        s[1::2] = SMALL
    return s


# ---------------------------------------------------------------------------------------------- layout
def lines_to_array(X, shape, axis):
    """[L, n] lines -> Fortran array of `shape` with the lines along `axis`, line l at the l-th position of the other
    two axes in memory order (the order in which the kernels pair lines)"""
    n = shape[axis]
    other = [s for i, s in enumerate(shape) if i != axis]
    T = np.asarray(X).reshape(other + [n], order="F")
    return np.asfortranarray(np.moveaxis(T, 2, axis))


def array_to_lines(a, axis):
    n = a.shape[axis]
    return np.moveaxis(a, axis, 2).reshape((a.size // n, n), order="F")


# ---------------------------------------------------------------------------------------------- CPU baselines
def scipy_lines(X, inverse):
    return sfft.dct(X, type=3 if inverse else 2, axis=1, norm="ortho")


@functools.lru_cache(maxsize=2)
def model_for(family, n):
    if n > MODEL_MAX_N:
        return None
    if family == "pfa":
        from pfa_proto import Pfa
        return Pfa(*PFA_FACTORS[n])
    if family in ("rader", "bluestein1"):
        from cdft_proto import Cdft
        return Cdft(n)
    if family == "fft2":
        from dct_long_proto import DctLong
        return DctLong(n)
    if family == "bluestein2":
        from cdft_long_proto import CdftLong
        return CdftLong(n)
    if family == "dense":
        from dct_dense_proto import DctDense
        return DctDense(n)
    return None


def model_lines(model, X, inverse):
    """the family's numpy model on the pairs (2r, 2r+1) of the batch; a last line without partner is paired with zeros"""
    if hasattr(model, "lines"):                  # the dense product has no pairs
        return model.lines(X, bool(inverse))
    out = np.empty_like(X)
    f = model.dct3 if inverse else model.dct2
    for r in range(0, X.shape[0], 2):
        xb = X[r + 1] if r + 1 < X.shape[0] else np.zeros(X.shape[1])
        a, b = f(X[r].copy(), xb.copy())
        out[r] = a
        if r + 1 < X.shape[0]:
            out[r + 1] = b
    return out


# ---------------------------------------------------------------------------------------------- figures
def _errors(pr, idx, s, got):
    """per line of the batch: max entry error (long double reference), as float64"""
    if pr.bins is None:
        ref = pr.ref[idx] * s[:, None].astype(LD)
        return np.max(np.abs(got.astype(LD) - ref), axis=1).astype(np.float64)
    return np.array([float(np.max(np.abs(got[r, pr.bins[i]].astype(LD) - pr.ref[i]))) for r, i in enumerate(idx)])


def _ulp_excess(pr, idx, s, got):
    """dense family, (A) / (A'): max over entries of |got - ref| / (ulp(ref) + 2^-59 u), the line's own amplitude.  The
    second term is the accuracy of the long-double cosines themselves, in the table of the plan and in the reference
    alike: the argument PI m / 2n <= 2 pi carries three roundings (PI, the product, the quotient), 3 * 2^-64 * 2 pi =
    1e-18 in absolute terms each side.  It is all there is to an entry that is zero in exact arithmetic, cos(pi / 2),
    more than the ulp of an entry below u / 100 -- the even / odd split reads the mirror image C[k][n-1-j], whose
    argument is another one -- and 1 / 128 ulp of an entry of size u."""
    ref = pr.ref[idx] * s[:, None].astype(LD)
    ulp = np.spacing(np.abs(ref.astype(np.float64))) + (2.0 ** -59 * pr.scale[idx] * s)[:, None]
    return float(np.max(np.abs(got.astype(LD) - ref) / ulp))


def case_shape(case):
    family, shape, axis = case[:3]
    return family, tuple(shape), axis, (case[3] if len(case) > 3 else None)


def case_id(case):
    family, shape, axis, npos = case_shape(case)
    return "%s-%s-axis%d" % (family, "x".join(str(s) for s in shape), axis)


def measure(case, transform=None, models=True):
    """One row per (direction, probe): E of scipy, of the family's model and -- with `transform(a, axis, inverse)` -- of the
    device, the bound and where the device's worst entry is.  E of (A'): every line on the scale of the unit lines."""
    family, shape, axis, npos = case_shape(case)
    n = shape[axis]
    L = int(np.prod(shape)) // n
    model = model_for(family, n) if models else None
    rows = []
    for inverse in (0, 1):
        for pr in probes(family, n, npos, inverse):
            E = {"scipy": 0.0, "model": 0.0, "device": 0.0}
            floorE, ulps, worst = 0.0, 0.0, None
            for idx in batches(pr.U.shape[0], L):
                s = line_factors(pr.kind, L)
                X = pr.U[idx] * s[:, None]
                scale = EPS * pr.scale[idx]                   # (A'): the small lines on the scale of their unit partners
                floorE = max(floorE, float(np.max(pr.floor[idx] / scale)))
                runs = [("scipy", scipy_lines(X, inverse))]
                if model is not None:
                    runs.append(("model", model_lines(model, X, inverse)))
                if transform is not None:
                    got = array_to_lines(transform(lines_to_array(X, shape, axis), axis, bool(inverse)), axis)
                    runs.append(("device", got))
                    if family == "dense" and pr.kind != "B":
                        ulps = max(ulps, _ulp_excess(pr, idx, s, got))
                for name, got in runs:
                    e = _errors(pr, idx, s, got) / scale
                    if name == "device" and float(e.max()) >= E["device"]:
                        worst = int(idx[int(np.argmax(e))])
                    E[name] = max(E[name], float(e.max()))
            bound = max(MARGIN * max(E["scipy"], E["model"]), floorE)
            rows.append(dict(case=case_id(case), family=family, n=n, axis=axis, inverse=inverse, kind=pr.kind,
                             E_scipy=E["scipy"], E_model=E["model"], E_device=E["device"], bound=bound, ulps=ulps,
                             worst_line=-1 if worst is None else worst))
    return rows


def passes(row):
    if row["family"] == "dense" and row["kind"] != "B":
        return row["ulps"] <= 1.0
    return row["E_device"] <= row["bound"]


def format_row(r):
    tail = "ulps %.2f (bound 1)" % r["ulps"] if r["family"] == "dense" and r["kind"] != "B" else \
        "E_device / bound %.3f" % (r["E_device"] / r["bound"] if r["bound"] > 0 else float("inf"))
    return "%-34s %s %-2s  E_device %9.3g  E_scipy %8.3g  E_model %8.3g  bound %8.3g  %s%s" % (
        r["case"], "inv" if r["inverse"] else "fwd", r["kind"], r["E_device"], r["E_scipy"], r["E_model"], r["bound"], tail,
        "" if passes(r) else "   <-- FAILS (line of probe %d)" % r["worst_line"])


KEYS = ("case", "family", "n", "axis", "inverse", "kind", "E_scipy", "E_model", "E_device", "bound", "ulps", "worst_line")


def save_rows(path, rows, **extra):
    np.savez(path, **{k: np.array([r[k] for r in rows]) for k in KEYS}, **extra)


def load_rows(path):
    with np.load(path) as z:
        cols = {k: z[k].tolist() for k in KEYS}
        extra = {k: z[k].tolist() for k in z.files if k not in KEYS}
    return [dict(zip(KEYS, vals)) for vals in zip(*(cols[k] for k in KEYS))], extra


def parse_case(spec):
    """family:n0xn1xn2:axis[:npos]"""
    f = spec.split(":")
    return (f[0], tuple(int(s) for s in f[1].split("x")), int(f[2])) + ((int(f[3]),) if len(f) > 3 else ())


def spec_of(case):
    family, shape, axis, npos = case_shape(case)
    return "%s:%s:%d" % (family, "x".join(str(s) for s in shape), axis) + ("" if npos is None else ":%d" % npos)


def family_on_device(D, n, axis):
    """the name used here for what the dispatcher of the library picks for a line of length n along `axis`"""
    alg = D.dct_algorithm(n)
    if alg == "fft":
        return "fft%d" % D.dct_levels(n, axis)
    if alg == "bluestein":
        return "bluestein%d" % D.cdft_levels(n)
    return alg


def kernel_on_device(D, shape, axis):
    """which kernel generation the library's launcher takes for this pass on the current device (capi.DCT_PASS_KERNELS:
    the launchers switch on the function that answers)"""
    from dotsocp_amd import capi
    return capi.dct_pass_kernel(shape, axis)


def main(argv):
    sys.path.insert(0, ROOT)
    import dotsocp_amd as D
    cases = [parse_case(s) for s in argv[2:]]
    rows, fams, kernels = [], [], []
    for case in cases:
        family, shape, axis, npos = case_shape(case)
        fams.append(family_on_device(D, shape[axis], axis))
        kernels.append(kernel_on_device(D, shape, axis))
        rows += measure(case, D.dct_axis)
    for r in rows:
        print(format_row(r))
    save_rows(argv[1], rows, families=np.array(fams), kernels=np.array(kernels))


if __name__ == "__main__":
    main(sys.argv)
