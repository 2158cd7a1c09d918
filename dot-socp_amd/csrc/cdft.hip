// DCT-II / DCT-III for the lengths that are neither powers of two (dct_pow2.hip) nor prime-factor lengths (pfa.hip): the
// length-n complex DFT behind Makhoul's DCT (mirt_dctn.m:100-141, mirt_idctn.m:98-128 are FFT-based for ANY length) as a
// cyclic convolution of power-of-two length M, entirely in LDS (tools/cdft_proto.py is the numpy model):
//   gather through a position table (x input multiplier) -> zero-fill to M -> forward FFT (decimation in frequency,
//   bit-reversed out) -> multiply by the precomputed spectrum of the kernel (stored bit-reversed, 1/M folded in), conjugate
//   -> the same forward butterflies as decimation in time (bit-reversed in, natural out) = conjugate of the inverse FFT
//   -> scatter through a position table (x output multiplier) -> Makhoul post-processing on the pair (k, n-k).
// Two real lines travel as real and imaginary part of one complex line.  DCT-III: the same DFT on the pre-processed
// spectrum G[k] = (ww[k] X[k] + conj(ww[n-k]) X[n-k]) / 2, un-reordered on the way out.
//   Rader, n = 257 (g = 3 is a primitive root, M = 256, no padding): X_0 = sum v, X_{g^-q} = v_0 + (a (*) b)_q with
//     a_q = v_{g^q}, b_q = exp(-2 pi i g^-q / 257).  v_0 waits in the spare slot M of its row; adding it to the spectrum's
//     entry 0 adds it to every output of the convolution.
//   Bluestein, 48 <= n <= 1024: chirp w_j = exp(-i pi j^2 / n) (exponent reduced exactly, (j * j) % (2 * n)),
//     X_k = w_k sum_j (v_j w_j) conj(w_{k-j}), M = 2^ceil(log2(2n-1)) <= 2048.
// Lengths above 1024 do not fit a convolution in the LDS: cdft_long.hip runs the same algebra as a two-level FFT through a
// scratch array (by default from 4101; DOTSOCP_CDFT_LONG_MIN), the lengths in between keep the dense product.
#include "cdft.h"
#include "device_utils.h"
#include "fft_lds.h"
#include "kernels.h"

#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace dotsocp {

struct CdftPlan {
    int n, lg;             // line length; the convolution has M = 2^lg points
    bool rader;
    unsigned short *pos;   // [4][n] LDS offsets inside a row: gather by element (forward), gather by k (inverse),
                           //        scatter by k (forward), scatter by element (inverse); Rader's v_0 / X_0: slot M
    double2 *mul;          // [n] Bluestein chirp w_j (input and output multiplier); Rader: nullptr
    double2 *spec;         // [M] spectrum of the convolution kernel / M, bit-reversed order
    double2 *tw;           // [M/2] exp(-2 pi i k / M)
    double2 *ww;           // [n]  2 exp(-i pi k / 2n) / sqrt(2n), ww[0] /= sqrt(2)   (mirt_dctn.m:69-70)
};

struct CdftDev {
    int n, lg;
    const unsigned short *pos;
    const double2 *mul, *spec, *tw, *ww;
};

// convolution output q of a row (stored conjugated), times the output multiplier
template <bool RADER>
__device__ __forceinline__ double2 cdft_out(const double2 *r, unsigned pos, int k, const double2 *__restrict__ mul) {
    double2 c = r[pos];
    c.y = -c.y;
    return RADER ? c : cmul(c, mul[k]);
}

// One workgroup of T threads: 2^lp complex rows = 2^(lp+1) consecutive lines.  AXIS0: lines contiguous in memory (line L
// at L * map.outerStride), a wave sweeps the elements of a line; otherwise the lines of the tile are consecutive in
// memory (map.base) and a wave sweeps the lines of one element.
template <int T, bool AXIS0, bool INV, bool RADER>
__global__ void __launch_bounds__(T) k_cdft(const double *src, double *dst, LineMap map, int lp, CdftDev c) {
    extern __shared__ double2 lds[];
    const int n = c.n, lg = c.lg, M = 1 << lg;
    const int rowStride = row_stride(M);
    const int P = 1 << lp;
    const int tid = threadIdx.x;
    const i64 L0 = (AXIS0 ? (i64)blockIdx.x : xcd_tile(blockIdx.x, gridDim.x)) << (lp + 1);
    const i64 es = AXIS0 ? 1 : map.es;
    // strided: this thread's pair of lines is fixed
    const int rs = tid & (P - 1);
    i64 sA = 0, sB = 0;
    bool sOkA = false, sOkB = false;
    if (!AXIS0) {
        const i64 La = L0 + 2 * rs;
        sOkA = La < map.nLines;
        sOkB = La + 1 < map.nLines;
        sA = sOkA ? map.base(La) : 0;
        sB = sOkB ? map.base(La + 1) : 0;
    }
    const int total = AXIS0 ? P * n : n;              // items of the load / store loops
    const int first = AXIS0 ? tid : (tid >> lp);
    const int step = AXIS0 ? T : (T >> lp);
    // ---- gather ----
    for (int b = first; b < total; b += step) {
        int rr, e;
        i64 bA, bB;
        bool okA, okB;
        if (AXIS0) {
            rr = (int)((unsigned)b / (unsigned)n);
            e = b - rr * n;
            const i64 La = L0 + 2 * rr;
            okA = La < map.nLines;
            okB = La + 1 < map.nLines;
            bA = La * map.outerStride;
            bB = bA + map.outerStride;
        } else {
            rr = rs; e = b; bA = sA; bB = sB; okA = sOkA; okB = sOkB;
        }
        double2 *r = lds + rr * rowStride;
        double2 v;
        if (!INV) {
            v = make_double2(okA ? src[bA + e * es] : 0.0, okB ? src[bB + e * es] : 0.0);
            if (!RADER) v = cmul(v, c.mul[makhoul(e, n)]);
            r[c.pos[e]] = v;
        } else {
            const int m = e ? n - e : 0;
            const double2 xk = make_double2(okA ? src[bA + e * es] : 0.0, okB ? src[bB + e * es] : 0.0);
            const double2 xm = make_double2(okA ? src[bA + m * es] : 0.0, okB ? src[bB + m * es] : 0.0);
            const double2 wk = c.ww[e], wm = c.ww[m];
            if (e == 0) {
                v = make_double2(wk.x * xk.x, wk.x * xk.y);
            } else {
                v = idct_half(wk, xk, wm, xm);
            }
            if (!RADER) v = cmul(v, c.mul[e]);
            r[c.pos[n + e]] = v;
        }
    }
    if (!RADER) {
        const int nz = M - n;                         // zero-fill n .. M-1 of every row
        for (int b = tid; b < P * nz; b += T) {
            const int rr = (int)((unsigned)b / (unsigned)nz);
            lds[rr * rowStride + padi(n + (b - rr * nz))] = make_double2(0.0, 0.0);
        }
    }
    __syncthreads();
    fft_rows<false>(lds, lp, lg, rowStride, BlockTeam<T>{tid}, c.tw);
    // ---- spectrum of the kernel, conjugate ----
    for (int b = tid; b < (P << lg); b += T) {
        double2 *r = lds + (b >> lg) * rowStride;
        const int i = b & (M - 1);
        const double2 z = r[padi(i)];
        double2 y = cmul(z, c.spec[i]);
        if (RADER && i == 0) {
            const double2 u0 = r[M];
            r[M] = make_double2(u0.x + z.x, -(u0.y + z.y));      // X_0 = v_0 + sum of the others (kept conjugated)
            y.x += u0.x;
            y.y += u0.y;
        }
        r[padi(i)] = make_double2(y.x, -y.y);
    }
    __syncthreads();
    fft_rows<true>(lds, lp, lg, rowStride, BlockTeam<T>{tid}, c.tw);
    // ---- scatter ----
    for (int b = first; b < total; b += step) {
        int rr, e;
        i64 bA, bB;
        bool okA, okB;
        if (AXIS0) {
            rr = (int)((unsigned)b / (unsigned)n);
            e = b - rr * n;
            const i64 La = L0 + 2 * rr;
            okA = La < map.nLines;
            okB = La + 1 < map.nLines;
            bA = La * map.outerStride;
            bB = bA + map.outerStride;
        } else {
            rr = rs; e = b; bA = sA; bB = sB; okA = sOkA; okB = sOkB;
        }
        const double2 *r = lds + rr * rowStride;
        double2 o;
        if (!INV) {
            const int m = e ? n - e : 0;
            const double2 vk = cdft_out<RADER>(r, c.pos[2 * n + e], e, c.mul);
            const double2 vm = cdft_out<RADER>(r, c.pos[2 * n + m], m, c.mul);
            const double2 w = c.ww[e];
            o = dct_split(vk, vm).at_k(w);
        } else {
            o = cdft_out<RADER>(r, c.pos[3 * n + e], makhoul(e, n), c.mul);
        }
        if (okA) dst[bA + e * es] = o.x;
        if (okB) dst[bB + e * es] = o.y;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
typedef std::complex<long double> cld;

// in-place radix-2 FFT of length M = 2^lg in long double (twiddles from cosl / sinl, no recurrences)
void cdft_fft_ld(std::vector<cld> &a, int lg) {
    const long double PI = 3.141592653589793238462643383279502884L;
    const int M = 1 << lg;
    std::vector<cld> W((size_t)M / 2 + 1);
    for (int k = 0; k < M / 2; ++k) {
        const long double t = -2.0L * PI * (long double)k / (long double)M;
        W[k] = cld(cosl(t), sinl(t));
    }
    for (int i = 0; i < M; ++i) {
        int j = 0;
        for (int b = 0; b < lg; ++b) j |= ((i >> b) & 1) << (lg - 1 - b);
        if (j > i) std::swap(a[i], a[j]);
    }
    for (int len = 2; len <= M; len <<= 1)
        for (int s = 0; s < M; s += len)
            for (int k = 0; k < len / 2; ++k) {
                const cld t = W[(size_t)k * (M / len)] * a[s + k + len / 2];
                a[s + k + len / 2] = a[s + k] - t;
                a[s + k] = a[s + k] + t;
            }
}

template <class V>
static bool cdft_upload(V **out, const std::vector<V> &h) {
    return hipMalloc(out, sizeof(V) * h.size()) == hipSuccess &&
           hipMemcpy(*out, h.data(), sizeof(V) * h.size(), hipMemcpyHostToDevice) == hipSuccess;
}

CdftPlan *cdft_plan_create(i64 n64) {
    if (n64 < 48 || n64 > CDFT_MAX_N || (n64 & (n64 - 1)) == 0) return nullptr;
    const int n = (int)n64;
    const bool rader = n == 257;
    const int lg = ceil_log2(rader ? 256 : 2 * n - 1);
    const int M = 1 << lg;
    const long double PI = 3.141592653589793238462643383279502884L;
    CdftPlan *p = new CdftPlan();
    p->n = n; p->lg = lg; p->rader = rader;
    p->pos = nullptr; p->mul = p->spec = p->tw = p->ww = nullptr;
    std::vector<int> posIn(n), posOut(n);       // row position of DFT input p / of DFT output k (-1: the spare slot M)
    std::vector<cld> b((size_t)M, cld(0.0L, 0.0L));
    std::vector<double2> mul;
    if (rader) {
        const int g = 3;
        std::vector<int> pw(256), dlog(257, 0);
        int v = 1;
        for (int q = 0; q < 256; ++q) { pw[q] = v; dlog[v] = q; v = (v * g) % 257; }
        posIn[0] = posOut[0] = -1;
        for (int k = 1; k < 257; ++k) {
            posIn[k] = dlog[k];                        // a_q = v_{g^q}
            posOut[k] = (256 - dlog[k]) % 256;         // X_{g^-q} sits at q
        }
        for (int q = 0; q < 256; ++q) {
            const long double t = -2.0L * PI * (long double)pw[(256 - q) % 256] / 257.0L;      // g^-q
            b[q] = cld(cosl(t), sinl(t));
        }
    } else {
        mul.resize(n);
        for (i64 j = 0; j < n; ++j) {
            const long double t = -PI * (long double)((j * j) % (2 * n)) / (long double)n;    // exact reduction of j^2 / n
            const cld w(cosl(t), sinl(t));
            mul[j] = make_double2((double)w.real(), (double)w.imag());
            b[j] = std::conj(w);
            if (j) b[M - j] = std::conj(w);
            posIn[j] = posOut[j] = (int)j;
        }
    }
    cdft_fft_ld(b, lg);
    std::vector<double2> spec(M), tw(M / 2), ww(n);
    for (int i = 0; i < M; ++i) {
        int j = 0;
        for (int bb = 0; bb < lg; ++bb) j |= ((i >> bb) & 1) << (lg - 1 - bb);
        spec[i] = make_double2((double)(b[j].real() / (long double)M), (double)(b[j].imag() / (long double)M));
    }
    for (int k = 0; k < M / 2; ++k) {
        const long double a = -2.0L * PI * (long double)k / (long double)M;
        tw[k] = make_double2((double)cosl(a), (double)sinl(a));
    }
    for (int k = 0; k < n; ++k) {
        long double a = -PI * (long double)k / (2.0L * (long double)n);
        long double sc = 2.0L / sqrtl(2.0L * (long double)n);
        if (k == 0) sc /= sqrtl(2.0L);
        ww[k] = make_double2((double)(sc * cosl(a)), (double)(sc * sinl(a)));
    }
    std::vector<unsigned short> pos((size_t)4 * n);
    auto off = [&](int q) { return (unsigned short)(q < 0 ? M : padi(q)); };
    auto mk = [&](int k) { return (k & 1) ? (n - 1 - (k >> 1)) : (k >> 1); };
    for (int e = 0; e < n; ++e) {
        pos[e] = off(posIn[mk(e)]);
        pos[(size_t)n + e] = off(posIn[e]);
        pos[(size_t)2 * n + e] = off(posOut[e]);
        pos[(size_t)3 * n + e] = off(posOut[mk(e)]);
    }
    if (!cdft_upload(&p->pos, pos) || !cdft_upload(&p->spec, spec) || !cdft_upload(&p->tw, tw) ||
        !cdft_upload(&p->ww, ww) || (!rader && !cdft_upload(&p->mul, mul))) {
        cdft_plan_destroy(p);
        return nullptr;
    }
    return p;
}

void cdft_plan_destroy(CdftPlan *p) {
    if (!p) return;
    if (p->pos) (void)hipFree(p->pos);
    if (p->mul) (void)hipFree(p->mul);
    if (p->spec) (void)hipFree(p->spec);
    if (p->tw) (void)hipFree(p->tw);
    if (p->ww) (void)hipFree(p->ww);
    delete p;
}

int cdft_launch(const CdftPlan *p, const double *src, double *dst, const LineMap &map, bool axis0, int inverse,
                hipStream_t st) {
    if (map.nLines <= 0) return 0;
    static unsigned long long done = 0;
    if (DeviceOnce once_(done); once_) {
        const int lim = 4 * row_stride(2048) * (int)sizeof(double2);      // the largest tile: four rows of 2048 points
#define CDFT_RAISE4(T, R)                                                                              \
    allow_big_lds(k_cdft<T, true, false, R>, lim); allow_big_lds(k_cdft<T, true, true, R>, lim);       \
    allow_big_lds(k_cdft<T, false, false, R>, lim); allow_big_lds(k_cdft<T, false, true, R>, lim)
        CDFT_RAISE4(256, true);
        CDFT_RAISE4(256, false);
        CDFT_RAISE4(512, false);
#undef CDFT_RAISE4
    }
    const int lg = p->lg, M = 1 << lg;
    // rows per workgroup of 256 threads: 4096 complex points (70 KB of LDS, two workgroups per CU), at most 16 rows.  The
    // strided axes at M = 2048 take FOUR rows with 512 threads instead: 139 KB, one workgroup per CU, eight consecutive
    // lines = 64 contiguous bytes (half a 128-byte line) per element and access
    int lp = 12 - lg;
    int T = 256;
    if (!axis0 && lg == 11) { lp = 2; T = 512; }
    if (lp > 4) lp = 4;
    const i64 havePairs = (map.nLines + 1) / 2;
    while (lp > 0 && ((i64)1 << lp) > havePairs) --lp;
    const size_t lds = ((size_t)row_stride(M) << lp) * sizeof(double2);
    const i64 blocks = (map.nLines + ((i64)2 << lp) - 1) / ((i64)2 << lp);
    if (blocks >= (1ll << 31)) { set_error("too many DCT tiles"); return DOTSOCP_EINVAL; }
    const CdftDev c{p->n, lg, p->pos, p->mul, p->spec, p->tw, p->ww};
#define CDFT_GO(T_, A, I, R) \
    DS_KLAUNCH((k_cdft<T_, A, I, R>), dim3((unsigned)blocks), dim3(T_), lds, st, src, dst, map, lp, c)
#define CDFT_GO_AI(T_, R)                                                        \
    do {                                                                         \
        if (axis0) { if (inverse) CDFT_GO(T_, true, true, R); else CDFT_GO(T_, true, false, R); }   \
        else { if (inverse) CDFT_GO(T_, false, true, R); else CDFT_GO(T_, false, false, R); }        \
    } while (0)
    if (p->rader) CDFT_GO_AI(256, true);
    else if (T == 512) CDFT_GO_AI(512, false);
    else CDFT_GO_AI(256, false);
#undef CDFT_GO_AI
#undef CDFT_GO
    DS_HIP(hipGetLastError());
    return 0;
}

}  // namespace dotsocp
