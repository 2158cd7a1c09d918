"""numpy prototype of the convolution-based DCT of csrc/cdft.hip (Rader for 257, Bluestein for the other lengths up to
1024): position tables, multipliers, the spectrum of the convolution kernel, the conjugation trick for the inverse FFT,
Makhoul pre / post-processing -- checked against scipy.  Development aid; the kernel follows it step by step."""
import numpy as np
import scipy.fft as sf


def makhoul(n):
    k = np.arange(n)
    return np.where(k % 2 == 0, k // 2, n - 1 - k // 2)


def chirp(n):
    """w_j = exp(-i pi j^2 / n) with the exponent reduced exactly: (j * j) mod 2n in integers (a j * j / n in doubles is
    1e-12 off at n = 1023)"""
    j = np.arange(n, dtype=np.int64)
    return np.exp(-1j * np.pi * ((j * j) % (2 * n)).astype(np.float64) / n)


class Cdft:
    """Length-n complex DFT as a cyclic convolution of power-of-two length M.  pos_in[p] / pos_out[k]: where DFT input p
    goes / DFT output k is found in the M-point row (-1: Rader's spare slot for v_0 / X_0); mul: input and output
    multiplier (Bluestein's chirp; Rader: none); spec: FFT of the convolution kernel / M."""

    def __init__(self, n):
        self.n = n
        self.rader = n == 257
        if self.rader:
            self.g, self.M = 3, 256
            self.pw = np.array([pow(self.g, q, 257) for q in range(256)])            # g^q
            self.ipw = np.array([pow(self.g, (256 - q) % 256, 257) for q in range(256)])    # g^-q
            dlog = np.zeros(257, dtype=int)
            dlog[self.pw] = np.arange(256)
            self.pos_in = np.concatenate(([-1], dlog[1:]))                     # a_q = v_{g^q}
            self.pos_out = np.concatenate(([-1], (256 - dlog[1:]) % 256))      # X_{g^-q} sits at q
            self.mul = None
            b = np.exp(-2j * np.pi * self.ipw / 257.0)
        else:
            self.M = 1 << int(np.ceil(np.log2(2 * n - 1)))
            self.pos_in = self.pos_out = np.arange(n)
            self.mul = chirp(n)
            b = np.zeros(self.M, complex)
            b[:n] = np.conj(self.mul)
            b[self.M - n + 1:] = np.conj(self.mul[:0:-1])
        self.spec = np.fft.fft(b) / self.M
        k = np.arange(n)
        self.ww = 2.0 / np.sqrt(2.0 * n) * np.exp(-1j * np.pi * k / (2.0 * n))
        self.ww[0] /= np.sqrt(2.0)

    def dft(self, u):
        n, M = self.n, self.M
        row = np.zeros(M, complex)
        spare = 0.0
        v = u if self.mul is None else u * self.mul
        if self.rader:
            spare = v[0]
            row[self.pos_in[1:]] = v[1:]
        else:
            row[self.pos_in] = v
        A = np.fft.fft(row)
        Z = A * self.spec
        if self.rader:
            x0 = spare + A[0]
            Z[0] += spare                 # adds v_0 to every output of the convolution
        c = np.conj(np.fft.fft(np.conj(Z)))        # inverse FFT through the forward butterflies (1/M is in spec)
        if self.rader:
            X = np.empty(n, complex)
            X[0] = x0
            X[1:] = c[self.pos_out[1:]]
            return X
        return c[self.pos_out] * self.mul

    def dct2(self, xa, xb):
        n = self.n
        v = np.zeros(n, complex)
        v[makhoul(n)] = xa + 1j * xb
        V = self.dft(v)
        k = np.arange(n)
        Vm = V[(n - k) % n]
        Va = 0.5 * (V + np.conj(Vm))
        Vb = (V - np.conj(Vm)) / 2j
        return (self.ww * Va).real, (self.ww * Vb).real

    def dct3(self, Xa, Xb):
        n, ww = self.n, self.ww

        def g(Xr):
            out = np.empty(n, complex)
            out[0] = ww[0] * Xr[0]
            out[1:] = 0.5 * (ww[1:] * Xr[1:] + np.conj(ww[:0:-1]) * Xr[:0:-1])
            return out
        y = self.dft(g(Xa) + 1j * g(Xb))[makhoul(n)]
        return y.real, y.imag


if __name__ == "__main__":
    rng = np.random.default_rng(1)
    for n in (257, 49, 97, 100, 193, 300, 385, 769, 1000, 1023):
        P = Cdft(n)
        xa, xb = rng.standard_normal(n), rng.standard_normal(n)
        fa, fb = P.dct2(xa, xb)
        e1 = max(abs(fa - sf.dct(xa, norm="ortho")).max(), abs(fb - sf.dct(xb, norm="ortho")).max())
        ia, ib = P.dct3(xa, xb)
        e2 = max(abs(ia - sf.idct(xa, norm="ortho")).max(), abs(ib - sf.idct(xb, norm="ortho")).max())
        print(n, "rader" if P.rader else "bluestein", "M", P.M, "fwd %.2e inv %.2e" % (e1, e2))
