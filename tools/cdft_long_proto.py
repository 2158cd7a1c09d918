"""numpy prototype of the two-level Bluestein DCT of csrc/cdft_long.hip for the lengths that are not powers of two and do
not fit the LDS convolution of csrc/cdft.hip: Bluestein's cyclic convolution of length M = 2^ceil(log2(2n-1)) done as a
two-level FFT, M = m1 m2 (split as csrc/dct_long.hip splits), j = j1 m2 + j2, k = k1 + m1 k2, in three passes over a
scratch array [k1][j2]:
  column pass       m1-point FFT over j1 of a[j] = v[j] w_j (zero for j >= n), times exp(-2 pi i j2 k1 / M);
  row pass          in place: m2-point FFT over j2, times the kernel spectrum S[k1 + m1 k2] / M, unnormalised inverse
                    m2-point FFT over k2, times exp(+2 pi i k1 j2 / M);
  column pass back  inverse m1-point FFT over k1 = c[j1 m2 + j2]; j < n times w_j; DCT-II post-processing on (k, n - k),
                    whose partner lies in column (n - j2) mod m2, resp. Makhoul's un-reordering for the DCT-III.
The tables are built the way the kernels build them: chirp exponent reduced in integers, the M-point twiddle factored
as hi[m >> lg m2] lo[m mod m2], the spectrum from a long-double FFT.  Checked against scipy.  Development aid; the
kernels follow it step by step."""
import numpy as np
import scipy.fft as sf

MIN_N = 129
MAX_N = (1 << 19) - 1
DEFAULT_MIN = 4101
PFA = (3, 5, 9, 17, 33, 65, 129, 513, 1025)


def conv_length(n):
    return 1 << (2 * n - 2).bit_length()          # 2^ceil(log2(2n - 1))


def split(M):
    """M = m1 * m2 with m1 >= m2 powers of two, as tools/dct_long_proto.py"""
    lg = M.bit_length() - 1
    assert M == 1 << lg and 8 <= lg <= 20, M
    l2 = lg // 2
    return 1 << (lg - l2), 1 << l2


def makhoul(n):
    k = np.arange(n)
    return np.where(k % 2 == 0, k // 2, n - 1 - k // 2)


def unit(num, den):
    """exp(-2 pi i num / den), the index reduced exactly in integers, the entry rounded once from long double"""
    num = np.asarray(num, dtype=np.int64) % den
    a = -2.0 * np.pi * num.astype(np.longdouble) / np.longdouble(den)
    return (np.cos(a) + 1j * np.sin(a)).astype(np.complex128)


def chirp_ld(n):
    """w_j = exp(-i pi j^2 / n) = exp(-2 pi i (j^2 mod 2n) / 2n) in long double"""
    j = np.arange(n, dtype=np.int64)
    a = -2.0 * np.pi * ((j * j) % (2 * n)).astype(np.longdouble) / np.longdouble(2 * n)
    return np.cos(a) + 1j * np.sin(a)


def fft_ld(a):
    """radix-2 FFT in long double, twiddles from cos / sin of exactly reduced indices (fft_ld of cdft.hip)"""
    a = np.asarray(a, dtype=np.clongdouble).copy()
    M = a.size
    lg = M.bit_length() - 1
    idx = np.arange(M)
    rev = np.zeros(M, dtype=np.int64)
    for b in range(lg):
        rev |= ((idx >> b) & 1) << (lg - 1 - b)
    a = a[rev]
    t = -2.0 * np.pi * np.arange(M // 2).astype(np.longdouble) / np.longdouble(M)
    W = np.cos(t) + 1j * np.sin(t)
    ln = 2
    while ln <= M:
        a = a.reshape(M // ln, ln)
        w = W[:: M // ln]
        t = w * a[:, ln // 2:]
        a = np.concatenate((a[:, :ln // 2] + t, a[:, :ln // 2] - t), axis=1).reshape(M)
        ln *= 2
    return a


class CdftLong:
    def __init__(self, n):
        assert MIN_N <= n <= MAX_N and n & (n - 1), n
        self.n = n
        self.M = M = conv_length(n)
        self.m1, self.m2 = m1, m2 = split(M)
        w = chirp_ld(n)
        self.chirp = w.astype(np.complex128)
        b = np.zeros(M, dtype=np.clongdouble)
        b[:n] = np.conj(w)
        b[M - n + 1:] = np.conj(w[:0:-1])
        self.spec = (fft_ld(b) / np.longdouble(M)).astype(np.complex128)      # S[k] / M
        self.hi = unit(np.arange(m1), m1)
        self.lo = unit(np.arange(m2), M)
        k = np.arange(n)
        self.ww = 2.0 / np.sqrt(2.0 * n) * np.exp(-1j * np.pi * k / (2.0 * n))
        self.ww[0] /= np.sqrt(2.0)

    def twiddle(self, m):
        m2 = self.m2
        return self.hi[m // m2] * self.lo[m % m2]

    # ---- the three passes; `scratch` is the [m1][m2] array in global memory between them ----
    def columns(self, v):
        n, M, m1, m2 = self.n, self.M, self.m1, self.m2
        a = np.zeros(M, complex)
        a[:n] = v * self.chirp
        c = np.fft.fft(a.reshape(m1, m2), axis=0)                        # [k1, j2]
        return c * self.twiddle(np.arange(m1)[:, None] * np.arange(m2)[None, :])

    def rows(self, scratch):
        m1, m2 = self.m1, self.m2
        A = np.fft.fft(scratch, axis=1)                                  # [k1, k2] = A[k1 + m1 k2]
        Z = A * self.spec.reshape(m2, m1).T
        # unnormalised inverse through the forward butterflies on the conjugate; the scratch array keeps the conjugate of
        # y[k1, j2] exp(+2 pi i k1 j2 / M), which is what the forward butterflies of the last pass need
        yc = np.fft.fft(np.conj(Z), axis=1)
        return yc * self.twiddle(np.arange(m1)[:, None] * np.arange(m2)[None, :])

    def columns_back(self, scratch):
        """X[j] for j < n, kept as the [m1][m2] array of the LDS tiles (entries with j >= n are not used)"""
        c = np.conj(np.fft.fft(scratch, axis=0))                         # [j1, j2] = c[j1 m2 + j2]
        X = np.zeros(self.M, complex)
        X[:self.n] = c.ravel()[:self.n] * self.chirp
        return X.reshape(self.m1, self.m2)

    def mirror_columns(self):
        """(primary, mirror) columns of the tiles of the forward last pass, in the order the kernel walks them: q = 1 ..
        m2 / 2; a column that is its own mirror leaves its mirror slot to the other such column"""
        n, m2 = self.n, self.m2
        r = n % m2
        o, h = r & 1, (r + 1) >> 1
        out = []
        for q in range(1, m2 // 2 + 1):
            prim = (h - o + q) % m2
            mirr = h if (not o and q == m2 // 2) else (h - q) % m2
            out.append((prim, mirr))
        return out

    def dft(self, v):
        return self.columns_back(self.rows(self.columns(v)))

    def dct2(self, xa, xb):
        n, m2 = self.n, self.m2
        v = np.zeros(n, complex)
        v[makhoul(n)] = xa + 1j * xb
        X = self.dft(v)
        out = np.empty(n, complex)
        seen = np.zeros(n, bool)
        for prim, mirr in self.mirror_columns():
            for col in {prim, mirr}:
                pcol = (n - col) % m2
                assert pcol in (prim, mirr)                               # the partner column is in the tile
                j = np.arange(col, n, m2)
                m = np.where(j == 0, 0, n - j)
                assert np.all(m % m2 == np.where(j == 0, 0, pcol))
                V, Vm = X[j // m2, col], np.where(j == 0, X[0, 0], X[m // m2, pcol])
                Va = 0.5 * (V + np.conj(Vm))
                Vb = (V - np.conj(Vm)) / 2j
                out[j] = (self.ww[j] * Va).real + 1j * (self.ww[j] * Vb).real
                assert not seen[j].any()
                seen[j] = True
        assert seen.all()
        return out.real, out.imag

    def dct3(self, Xa, Xb):
        n, ww = self.n, self.ww

        def g(Xr):
            out = np.empty(n, complex)
            out[0] = ww[0] * Xr[0]
            out[1:] = 0.5 * (ww[1:] * Xr[1:] + np.conj(ww[:0:-1]) * Xr[:0:-1])
            return out
        y = self.dft(g(Xa) + 1j * g(Xb)).ravel()[:n][makhoul(n)]
        return y.real, y.imag


def levels(n, long_min=None, cdft_on=True, cdft_min=500):
    """dotsocp_cdft_levels: 0 no convolution transform, 1 Rader / Bluestein in the LDS, 2 two-level"""
    first = DEFAULT_MIN if long_min is None else max(MIN_N, long_min)
    if n <= 1 or n & (n - 1) == 0 or n in PFA or not cdft_on:
        return 0
    if first <= n <= MAX_N:
        return 2
    if n == 257 or max(48, cdft_min) <= n <= 1024:
        return 1
    return 0


if __name__ == "__main__":
    rng = np.random.default_rng(1)
    for n in (129, 130, 300, 1026, 1030, 1536, 2049, 4097, 4101, 16385, 65537, 524287):
        P = CdftLong(n)
        xa, xb = rng.standard_normal(n), rng.standard_normal(n)
        fa, fb = P.dct2(xa, xb)
        e1 = max(abs(fa - sf.dct(xa, norm="ortho")).max(), abs(fb - sf.dct(xb, norm="ortho")).max())
        ia, ib = P.dct3(xa, xb)
        e2 = max(abs(ia - sf.idct(xa, norm="ortho")).max(), abs(ib - sf.idct(xb, norm="ortho")).max())
        print(n, "M", P.M, "%d x %d" % (P.m1, P.m2), "fwd %.2e inv %.2e" % (e1, e2))
