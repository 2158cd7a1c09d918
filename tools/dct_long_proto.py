"""numpy prototype of the two-level DCT of csrc/dct_long.hip for power-of-two lines that do not fit the LDS: Makhoul's
reordering, the length-n complex DFT as n2 column transforms of length n1, the twiddle exp(-2 pi i j2 k1 / n) and n1 row
transforms of length n2 (n = n1 n2, input index j = j1 n2 + j2, output index k = k1 + n1 k2), the scratch array between
the two passes, the factored tables, and the pairing of rows (DCT-II post-processing) resp. of input elements (DCT-III
pre-processing) -- checked against scipy.  Development aid; the kernels follow it step by step."""
import numpy as np
import scipy.fft as sf

LONG_MAX_LOG2 = 20


def split(n):
    """n = n1 * n2 with n1 >= n2 powers of two: the column pass takes the longer transform, the row pass -- which stages
    a row AND its mirror -- the shorter one"""
    lg = n.bit_length() - 1
    assert n == 1 << lg and 8 <= lg <= LONG_MAX_LOG2, n
    l2 = lg // 2
    return 1 << (lg - l2), 1 << l2


def makhoul(n):
    k = np.arange(n)
    return np.where(k % 2 == 0, k // 2, n - 1 - k // 2)


def unit(num, den):
    """exp(-2 pi i num / den) for integer arrays num: the index is reduced exactly in integers, the table entry comes from
    long double"""
    num = np.asarray(num, dtype=np.int64) % den
    a = -2.0 * np.pi * num.astype(np.longdouble) / np.longdouble(den)
    return (np.cos(a) + 1j * np.sin(a)).astype(np.complex128)


class DctLong:
    def __init__(self, n):
        self.n = n
        self.n1, self.n2 = n1, n2 = split(n)
        # the n-point twiddle exp(-2 pi i m / n), m = j2 * k1 < n, as hi[m // n2] * lo[m % n2]
        self.hi = unit(np.arange(n1), n1)
        self.lo = unit(np.arange(n2), n)
        # ww[k] = sc * exp(-i pi k / 2n), ww[0] /= sqrt(2), factored for k = k1 + n1 k2 (forward) and j = j1 n2 + j2 (inverse)
        sc = 2.0 / np.sqrt(2.0 * n)
        self.fa = sc * unit(np.arange(n1), 4 * n)          # k1
        self.fb = unit(np.arange(n2), 4 * n2)              # k2
        self.ia = sc * unit(np.arange(n1), 4 * n1)         # j1
        self.ib = unit(np.arange(n2), 4 * n)               # j2

    # ---- the two passes of the DFT; `scratch` is the [n1][n2] array in global memory between them ----
    def columns(self, v):
        n1, n2 = self.n1, self.n2
        a = v.reshape(n1, n2)                              # a[j1, j2]
        c = np.fft.fft(a, axis=0)                          # c[k1, j2]
        m = np.arange(n1)[:, None] * np.arange(n2)[None, :]
        return c * (self.hi[m // n2] * self.lo[m % n2])

    def rows(self, scratch):
        return np.fft.fft(scratch, axis=1)                 # X[k1, k2] = X[k1 + n1 k2]

    def dct2(self, xa, xb):
        n, n1, n2 = self.n, self.n1, self.n2
        v = np.zeros(n, complex)
        v[makhoul(n)] = xa + 1j * xb
        X = self.rows(self.columns(v))
        k1 = np.arange(n1)[:, None]
        k2 = np.arange(n2)[None, :]
        # partner n - k of k = k1 + n1 k2: row n1 - k1, column n2 - 1 - k2; row 0 is its own partner with column -k2
        pr = (n1 - k1) % n1 + 0 * k2
        pc = np.where(k1 == 0, (n2 - k2) % n2, n2 - 1 - k2)
        Vm = X[pr, pc]
        w = self.fa[k1] * self.fb[k2]
        w[0, 0] /= np.sqrt(2.0)
        Va = 0.5 * (X + np.conj(Vm))
        Vb = (X - np.conj(Vm)) / 2j
        out = np.empty(n, complex)
        out[(k1 + n1 * k2).ravel()] = ((w * Va).real + 1j * (w * Vb).real).ravel()
        return out.real, out.imag

    def dct3(self, Xa, Xb):
        n, n1, n2 = self.n, self.n1, self.n2
        j = np.arange(n)
        e = (self.ia[j // n2] * self.ib[j % n2])           # sc * exp(-i pi j / 2n) = ww[j] (j > 0)
        wm = -e.imag - 1j * e.real                         # ww[n - j]
        pj = (n - j) % n

        def g(Xr):
            out = 0.5 * (e * Xr + np.conj(wm) * Xr[pj])
            out[0] = e[0].real / np.sqrt(2.0) * Xr[0]
            return out
        y = self.rows(self.columns(g(Xa) + 1j * g(Xb)))
        k = (np.arange(n1)[:, None] + n1 * np.arange(n2)[None, :]).ravel()
        v = np.empty(n, complex)
        v[k] = y.ravel()
        v = v[makhoul(n)]
        return v.real, v.imag


def levels(n, axis, long_min=None):
    """dotsocp_dct_levels: 0 no transform, 1 inside the LDS (or one of the other families), 2 two-level, -1 unsupported"""
    if axis not in (0, 1, 2):
        return -1
    if n <= 1:
        return 0
    if n & (n - 1):
        return 1
    first = 4096 if axis == 0 else 16384
    if long_min is not None:                              # the switch lowers the start, never below 256
        first = min(first, max(256, 1 << (max(long_min, 1) - 1).bit_length()))
    if n < first:
        return 1
    return 2 if n <= 1 << LONG_MAX_LOG2 else -1


if __name__ == "__main__":
    rng = np.random.default_rng(1)
    for n in (256, 512, 4096, 8192, 65536, 1 << 20):
        P = DctLong(n)
        xa, xb = rng.standard_normal(n), rng.standard_normal(n)
        fa, fb = P.dct2(xa, xb)
        e1 = max(abs(fa - sf.dct(xa, norm="ortho")).max(), abs(fb - sf.dct(xb, norm="ortho")).max())
        ia, ib = P.dct3(xa, xb)
        e2 = max(abs(ia - sf.idct(xa, norm="ortho")).max(), abs(ib - sf.idct(xb, norm="ortho")).max())
        print(n, "%d x %d" % (P.n1, P.n2), "fwd %.2e inv %.2e" % (e1, e2))
