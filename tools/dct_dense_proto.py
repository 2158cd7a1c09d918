"""numpy prototype of the dense family of csrc/dct_dense.hip: the product with the n x n orthonormal DCT-II matrix, its
entries rounded once from long double with the argument reduced in integers (dense_plan_create), the sum over the
contraction index accumulated term by term in float64 in index order, as k_dct_dense accumulates it -- checked against
scipy.  (k_dct_mfma_split sums the even and the odd half separately, four terms per instruction: fewer roundings.)
Development aid."""
import numpy as np
import scipy.fft as sf


class DctDense:
    def __init__(self, n):
        self.n = n
        LD = np.longdouble
        pi = 4 * np.arctan(LD(1))
        k = np.arange(n, dtype=np.int64)[:, None]
        j = np.arange(n, dtype=np.int64)[None, :]
        m = ((2 * j + 1) * k) % (4 * n)
        sc = np.where(k == 0, np.sqrt(LD(1) / n), np.sqrt(LD(2) / n))
        self.C = (sc * np.cos(pi * m.astype(LD) / LD(2 * n))).astype(np.float64)       # C[k, j]

    @staticmethod
    def _accumulate(M, X):
        """out[l, i] = sum_c M[c, i] X[l, c], c = 0, 1, ... one product and one addition at a time"""
        acc = np.zeros((X.shape[0], M.shape[1]))
        for c in range(M.shape[0]):
            acc = acc + X[:, c, None] * M[c][None, :]
        return acc

    def lines(self, X, inverse):
        """DCT-II (DCT-III) of the rows of X: no pairs in this family"""
        return self._accumulate(self.C if inverse else np.ascontiguousarray(self.C.T), np.asarray(X, dtype=np.float64))

    def dct2(self, xa, xb):
        out = self.lines(np.stack([xa, xb]), False)
        return out[0], out[1]

    def dct3(self, Xa, Xb):
        out = self.lines(np.stack([Xa, Xb]), True)
        return out[0], out[1]


if __name__ == "__main__":
    rng = np.random.default_rng(1)
    for n in (47, 48, 96, 99, 257, 1025, 1026):
        P = DctDense(n)
        xa, xb = rng.standard_normal(n), rng.standard_normal(n)
        fa, fb = P.dct2(xa, xb)
        e1 = max(abs(fa - sf.dct(xa, norm="ortho")).max(), abs(fb - sf.dct(xb, norm="ortho")).max())
        ia, ib = P.dct3(xa, xb)
        e2 = max(abs(ia - sf.idct(xa, norm="ortho")).max(), abs(ib - sf.idct(xb, norm="ortho")).max())
        print(n, "fwd %.2e inv %.2e" % (e1, e2))
