// Bluestein's DCT for the lengths whose convolution does not fit the LDS (cdft.hip keeps whole convolutions there): the
// length-n complex DFT behind Makhoul's DCT as a cyclic convolution of length M = 2^ceil(log2(2n-1)), 256 <= M <= 2^20,
// and that convolution as a two-level FFT through a complex scratch array in global memory, M = m1 m2 (m1 >= m2, both at
// most 1024, split as dct_long.hip splits), j = j1 m2 + j2, k = k1 + m1 k2 (tools/cdft_long_proto.py is the numpy model):
//   column pass   k_clong_cols   a[j] = v[j] w_j (zero for j >= n), chirp w_j = exp(-i pi j^2 / n) with the exponent
//                                reduced exactly, (j * j) % (2 * n); m2 transforms of length m1 over j1, times
//                                exp(-2 pi i j2 k1 / M), into scratch[k1][j2] (the pairs of a tile interleaved);
//   row pass      k_clong_rows   in place on the scratch array: m2-point FFT over j2 (bit-reversed out), times the
//                                spectrum of the kernel S[k1 + m1 k2] / M (stored in that order), conjugate, the same
//                                butterflies as decimation in time = conjugate of the unnormalised inverse FFT over k2,
//                                times exp(-2 pi i k1 j2 / M): the scratch array now holds the CONJUGATE of what the
//                                inverse m1-point FFT wants, so that one is a forward FFT too;
//   column pass back  k_clong_back   m2 forward transforms of length m1 over k1, conjugate = c[j1 m2 + j2]; j < n, times
//                                w_j = X[j]; DCT-II post-processing on the pair (k, n - k) resp. Makhoul's un-reordering.
// Two real lines travel as the real and imaginary part of one complex line, as everywhere else.  The DCT-II
// post-processing needs X[k] and X[n - k], and n - k lies in column (n - j2) mod m2: a workgroup of the last pass stages
// columns and their mirrors together, as the row pass of dct_long.hip stages mirror rows.  The DCT-III pre-processing
// G[k] = (ww[k] X[k] + conj(ww[n-k]) X[n-k]) / 2 reads both INPUT elements in the first pass.  All tables come from the
// host in long double; the M-point twiddle is hi[m >> lg m2] lo[m mod m2] as in dct_long.hip.
//
// Tiles, LDS budget, scratch array and batching: long_scratch.h, shared with dct_long.hip.  Every line is addressed
// through LineMap on its own, so odd line counts, pitched rows and pairs that straddle a row need no special case.
#include "cdft.h"
#include "fft_lds.h"
#include "kernels.h"
#include "long_scratch.h"

#include <cmath>
#include <complex>
#include <cstdlib>
#include <vector>

namespace dotsocp {

// first length that takes the two-level convolution by default: lengths up to 4100 are pinned to the dense product
// (tests/test_cdft_algorithm.py); DESIGN.md section 3 has the measured crossover
#define CDFT_LONG_DEFAULT_MIN 4101
// Bound of the scratch array of one (plan, stream) pair, as in dct_long.hip: 16 M bytes per pair of lines, a pass over
// more lines runs in batches of whole tiles.
#define CLONG_SCRATCH_BYTES ((size_t)64 << 20)

i64 cdft_long_min() {
    static const i64 v = [] {
        const char *e = getenv("DOTSOCP_CDFT_LONG_MIN");
        const i64 m = e ? atoll(e) : (i64)CDFT_LONG_DEFAULT_MIN;
        return m < CDFT_LONG_MIN_N ? (i64)CDFT_LONG_MIN_N : m;
    }();
    return v;
}

struct CdftLongPlan {
    int n, lg, lg1, lg2;
    double2 *tab = nullptr;                // one allocation: the tables below
    const double2 *tw1, *tw2;              // [m1/2], [m2/2]  FFT twiddles of the two levels
    const double2 *hi, *lo;                // exp(-2 pi i m / M) = hi[m / m2] * lo[m % m2], m = j2 k1 < M
    const double2 *chirp;                  // [n] w_j
    const double2 *ww;                     // [n] 2 exp(-i pi k / 2n) / sqrt(2n), ww[0] /= sqrt(2)   (mirt_dctn.m:69-70)
    const double2 *spec;                   // [m1][m2] S[k1 + m1 bitrev(i)] / M at [k1][i]: the order the row pass meets
    LongScratch scratch;
};

CdftLongPlan *cdft_long_plan_create(i64 n64) {
    if (n64 < CDFT_LONG_MIN_N || n64 > CDFT_LONG_MAX_N || (n64 & (n64 - 1)) == 0) return nullptr;
    const int n = (int)n64;
    CdftLongPlan *p = new CdftLongPlan();
    p->n = n;
    p->lg = ceil_log2(2 * n64 - 1);
    p->lg2 = p->lg / 2;
    p->lg1 = p->lg - p->lg2;
    const i64 M = (i64)1 << p->lg, m1 = (i64)1 << p->lg1, m2 = (i64)1 << p->lg2;
    const long double PI = 3.141592653589793238462643383279502884L;
    typedef std::complex<long double> cld;
    std::vector<double2> t;
    t.reserve((size_t)(m1 / 2 + m2 / 2 + m1 + m2 + 2 * n64 + M));
    size_t off[7];
    off[0] = t.size(); for (i64 k = 0; k < m1 / 2; ++k) t.push_back(unit_root(k, m1));
    off[1] = t.size(); for (i64 k = 0; k < m2 / 2; ++k) t.push_back(unit_root(k, m2));
    off[2] = t.size(); for (i64 k = 0; k < m1; ++k) t.push_back(unit_root(k, m1));
    off[3] = t.size(); for (i64 k = 0; k < m2; ++k) t.push_back(unit_root(k, M));
    std::vector<cld> b((size_t)M, cld(0.0L, 0.0L));
    off[4] = t.size();
    for (i64 j = 0; j < n; ++j) {
        const long double a = -PI * (long double)((j * j) % (2 * n)) / (long double)n;    // exact reduction of j^2 / n
        const cld w(cosl(a), sinl(a));
        t.push_back(make_double2((double)w.real(), (double)w.imag()));
        b[j] = std::conj(w);
        if (j) b[M - j] = std::conj(w);
    }
    off[5] = t.size();
    for (i64 k = 0; k < n; ++k) {
        const long double a = -PI * (long double)k / (2.0L * (long double)n);
        long double sc = 2.0L / sqrtl(2.0L * (long double)n);
        if (k == 0) sc /= sqrtl(2.0L);
        t.push_back(make_double2((double)(sc * cosl(a)), (double)(sc * sinl(a))));
    }
    cdft_fft_ld(b, p->lg);
    off[6] = t.size();
    for (i64 k1 = 0; k1 < m1; ++k1)
        for (i64 i = 0; i < m2; ++i) {
            i64 k2 = 0;
            for (int bb = 0; bb < p->lg2; ++bb) k2 |= ((i >> bb) & 1) << (p->lg2 - 1 - bb);
            const cld s = b[(size_t)(k1 + m1 * k2)] / (long double)M;
            t.push_back(make_double2((double)s.real(), (double)s.imag()));
        }
    if (hipMalloc(&p->tab, sizeof(double2) * t.size()) != hipSuccess) {
        (void)hipGetLastError();
        delete p;
        return nullptr;
    }
    if (hipMemcpy(p->tab, t.data(), sizeof(double2) * t.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(p->tab);
        delete p;
        return nullptr;
    }
    p->tw1 = p->tab + off[0]; p->tw2 = p->tab + off[1];
    p->hi = p->tab + off[2];  p->lo = p->tab + off[3];
    p->chirp = p->tab + off[4]; p->ww = p->tab + off[5]; p->spec = p->tab + off[6];
    return p;
}

void cdft_long_plan_destroy(CdftLongPlan *p) {
    if (!p) return;
    p->scratch.release();
    if (p->tab) (void)hipFree(p->tab);
    delete p;
}

struct CLongArgs {
    LineMap map;
    int n, lg, lg1, lg2;
    int lP;            // log2(pairs of lines per tile)
    int lT;            // log2(columns per tile) in the column passes, log2(rows per tile) in the row pass
    i64 tile0;         // first tile of pairs of this batch
    const double2 *tw, *hi, *lo, *chirp, *ww, *spec;
};

// source element of position j of the Makhoul-ordered line of any length (v[j] = x[2j], v[n-1-j] = x[2j+1]); also where
// output position j of the inverse goes
__device__ __forceinline__ int clong_makhoul_src(int j, int n) { return j < ((n + 1) >> 1) ? 2 * j : 2 * (n - 1 - j) + 1; }

// ---------------------------------------------------------------------------------------------
// Column pass.  Workgroup = (tile of pairs) x (2^lT consecutive columns j2): row s = (c << lP) | p of the LDS holds
// column j2 = col0 + c of pair p, all m1 elements (those with j >= n are zero).  A thread keeps its row s for the whole
// kernel (LONG_THREADS is a multiple of the rows), so its line addresses are formed once.
// ---------------------------------------------------------------------------------------------
template <bool INVERSE>
__global__ void __launch_bounds__(LONG_THREADS) k_clong_cols(const double *__restrict__ src, double2 *__restrict__ scratch,
                                                              CLongArgs a) {
    extern __shared__ double2 lds[];
    const int n = a.n, m1 = 1 << a.lg1, m2 = 1 << a.lg2;
    const int rowStride = row_stride(m1);
    const int lNR = a.lT + a.lP, NR = 1 << lNR;
    const int tid = threadIdx.x;
    const unsigned nColTiles = (unsigned)(m2 >> a.lT);
    const int col0 = (int)(blockIdx.x % nColTiles) << a.lT;
    const i64 pt = blockIdx.x / nColTiles;                  // tile of pairs inside this batch
    const int s = tid & (NR - 1);
    const int p = s & ((1 << a.lP) - 1), j2 = col0 + (s >> a.lP);
    const i64 La = 2 * (((a.tile0 + pt) << a.lP) + p);
    const bool oka = La < a.map.nLines, okb = La + 1 < a.map.nLines;
    const double *sa = src + (oka ? a.map.base(La) : 0), *sb = src + (okb ? a.map.base(La + 1) : 0);
    const i64 es = a.map.es;
    double2 *row = lds + s * rowStride;
    const int jstep = LONG_THREADS >> lNR;
    for (int j0 = tid >> lNR; j0 < m1; j0 += jstep * LONG_BATCH) {
        double2 xk[LONG_BATCH], xm[LONG_BATCH];
#pragma unroll
        for (int u = 0; u < LONG_BATCH; ++u) {
            const int j1 = j0 + u * jstep;
            const int j = j1 * m2 + j2;                     // below 2^20 for every j1 < m1
            xk[u] = make_double2(0.0, 0.0);
            xm[u] = xk[u];
            if (j1 < m1 && j < n) {
                const i64 e = INVERSE ? j : clong_makhoul_src(j, n);
                if (oka) xk[u].x = sa[e * es];
                if (okb) xk[u].y = sb[e * es];
                if (INVERSE && j) {
                    const i64 em = n - j;
                    if (oka) xm[u].x = sa[em * es];
                    if (okb) xm[u].y = sb[em * es];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < LONG_BATCH; ++u) {
            const int j1 = j0 + u * jstep;
            if (j1 >= m1) break;
            const int j = j1 * m2 + j2;
            double2 v = make_double2(0.0, 0.0);
            if (j < n) {
                if (!INVERSE) {
                    v = xk[u];
                } else {
                    // G[j] = (ww[j] X[j] + conj(ww[n-j]) X[n-j]) / 2, G[0] = ww[0] X[0]   (the gather of k_cdft)
                    const double2 wk = a.ww[j];
                    if (j == 0) {
                        v = make_double2(wk.x * xk[u].x, wk.x * xk[u].y);
                    } else {
                        v = idct_half(wk, xk[u], a.ww[n - j], xm[u]);
                    }
                }
                v = cmul(v, a.chirp[j]);
            }
            row[padi(j1)] = v;
        }
    }
    __syncthreads();
    fft_rows<false>(lds, lNR, a.lg1, rowStride, BlockTeam<LONG_THREADS>{tid}, a.tw);
    // times exp(-2 pi i j2 k1 / M), to scratch[k1][j2] of this tile (pairs interleaved: the lanes of a row group are adjacent)
    double2 *out = scratch + (((pt << a.lg) + j2) << a.lP) + p;
    for (int k1 = tid >> lNR; k1 < m1; k1 += jstep) {
        const double2 v = row[padi(bitrev(k1, a.lg1))];
        const int m = j2 * k1;
        const double2 w = cmul(a.hi[m >> a.lg2], a.lo[m & (m2 - 1)]);
        out[((i64)k1 << a.lg2) << a.lP] = cmul(v, w);
    }
}

// ---------------------------------------------------------------------------------------------
// Row pass, in place.  Workgroup = (tile of pairs) x (2^lT consecutive rows k1), LDS row s = (slot << lP) | p: one
// contiguous piece of the scratch array in, the same piece out.  The forward and the inverse transform of the convolution
// meet here.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LONG_THREADS) k_clong_rows(double2 *__restrict__ scratch, CLongArgs a) {
    extern __shared__ double2 lds[];
    const int m1 = 1 << a.lg1, m2 = 1 << a.lg2;
    const int rowStride = row_stride(m2);
    const int lNR = a.lT + a.lP, NR = 1 << lNR;
    const int P = 1 << a.lP;
    const int tid = threadIdx.x;
    const unsigned nRowTiles = (unsigned)(m1 >> a.lT);
    const int row0 = (int)(blockIdx.x % nRowTiles) << a.lT;
    const i64 pt = blockIdx.x / nRowTiles;
    double2 *io = scratch + (((pt << a.lg) + ((i64)row0 << a.lg2)) << a.lP);
    const int total = m2 << lNR;
    // ---- load: (slot, j2, p) with p fastest ----
    for (int b0 = tid; b0 < total; b0 += LONG_THREADS * LONG_BATCH) {
        double2 v[LONG_BATCH];
#pragma unroll
        for (int u = 0; u < LONG_BATCH; ++u) {
            const int b = b0 + u * LONG_THREADS;
            v[u] = make_double2(0.0, 0.0);
            if (b < total) v[u] = io[b];
        }
#pragma unroll
        for (int u = 0; u < LONG_BATCH; ++u) {
            const int b = b0 + u * LONG_THREADS;
            if (b >= total) break;
            const int slot = b >> (a.lP + a.lg2), j2 = (b >> a.lP) & (m2 - 1), p = b & (P - 1);
            lds[((slot << a.lP) | p) * rowStride + padi(j2)] = v[u];
        }
    }
    __syncthreads();
    fft_rows<false>(lds, lNR, a.lg2, rowStride, BlockTeam<LONG_THREADS>{tid}, a.tw);
    // ---- spectrum of the kernel (1 / M folded in), conjugate ----
    for (int b = tid; b < (NR << a.lg2); b += LONG_THREADS) {
        const int r = b >> a.lg2, i = b & (m2 - 1);
        const int k1 = row0 + (r >> a.lP);
        double2 *q = lds + r * rowStride + padi(i);
        const double2 y = cmul(*q, a.spec[((i64)k1 << a.lg2) + i]);
        *q = make_double2(y.x, -y.y);
    }
    __syncthreads();
    fft_rows<true>(lds, lNR, a.lg2, rowStride, BlockTeam<LONG_THREADS>{tid}, a.tw);
    // ---- store: conj(y[k1][j2]) exp(-2 pi i k1 j2 / M) = conj(y[k1][j2] exp(+2 pi i k1 j2 / M)) ----
    for (int b = tid; b < total; b += LONG_THREADS) {
        const int slot = b >> (a.lP + a.lg2), j2 = (b >> a.lP) & (m2 - 1), p = b & (P - 1);
        const double2 v = lds[((slot << a.lP) | p) * rowStride + padi(j2)];
        const int m = j2 * (row0 + slot);
        const double2 w = cmul(a.hi[m >> a.lg2], a.lo[m & (m2 - 1)]);
        io[b] = cmul(v, w);
    }
}

// ---------------------------------------------------------------------------------------------
// Column pass back.  Workgroup = (tile of pairs) x (2^lT columns), LDS row s = (slot << lP) | p.  Inverse: the columns
// j2 = (g << lT) + slot.  Forward: element k = j1 m2 + j2 pairs with n - k in column (r - j2) mod m2, r = n mod m2; with
// o = r & 1, h = (r + 1) >> 1 and R = 2^(lT-1), slot i < R holds column h - o + q, q = g R + 1 + i, and slot R + i its
// mirror h - q (q = 1 .. m2 / 2 covers every column once).  For even r the columns h and h + m2 / 2 are their own
// mirrors: the latter (q = m2 / 2, last group) leaves its mirror slot to the former.
// ---------------------------------------------------------------------------------------------
template <bool INVERSE>
__global__ void __launch_bounds__(LONG_THREADS) k_clong_back(const double2 *__restrict__ scratch, double *__restrict__ dst,
                                                              CLongArgs a) {
    extern __shared__ double2 lds[];
    const int n = a.n, m1 = 1 << a.lg1, m2 = 1 << a.lg2;
    const int rowStride = row_stride(m1);
    const int lNR = a.lT + a.lP, NR = 1 << lNR;
    const int P = 1 << a.lP;
    const int tid = threadIdx.x;
    const unsigned nColTiles = (unsigned)(m2 >> a.lT);
    const int g = (int)(blockIdx.x % nColTiles);
    const i64 pt = blockIdx.x / nColTiles;
    const int s = tid & (NR - 1);
    const int p = s & (P - 1), slot = s >> a.lP;
    const int R = INVERSE ? 1 : 1 << (a.lT - 1);
    const int r = n & (m2 - 1), o = r & 1, h = (r + 1) >> 1;
    const int q = g * R + 1 + (slot & (R - 1));
    const bool selfm = !INVERSE && !o && q == (m2 >> 1);          // this slot's column is its own mirror
    int col;
    if (INVERSE) col = (g << a.lT) + slot;
    else if (slot < R) col = (h - o + q) & (m2 - 1);
    else col = selfm ? h : (h - q) & (m2 - 1);
    double2 *row = lds + s * rowStride;
    const int kstep = LONG_THREADS >> lNR;
    // ---- load: the thread's column, all k1 ----
    {
        const double2 *in = scratch + (((pt << a.lg) + col) << a.lP) + p;
        for (int k0 = tid >> lNR; k0 < m1; k0 += kstep * LONG_BATCH) {
            double2 v[LONG_BATCH];
#pragma unroll
            for (int u = 0; u < LONG_BATCH; ++u) {
                const int k1 = k0 + u * kstep;
                v[u] = make_double2(0.0, 0.0);
                if (k1 < m1) v[u] = in[((i64)k1 << a.lg2) << a.lP];
            }
#pragma unroll
            for (int u = 0; u < LONG_BATCH; ++u) {
                const int k1 = k0 + u * kstep;
                if (k1 >= m1) break;
                row[padi(k1)] = v[u];
            }
        }
    }
    __syncthreads();
    fft_rows<false>(lds, lNR, a.lg1, rowStride, BlockTeam<LONG_THREADS>{tid}, a.tw);
    // ---- store: X[j] = conj(row[j1]) w_j for j = j1 m2 + col < n ----
    const i64 La = 2 * (((a.tile0 + pt) << a.lP) + p);
    const bool oka = La < a.map.nLines, okb = La + 1 < a.map.nLines;
    double *da = dst + (oka ? a.map.base(La) : 0), *db = dst + (okb ? a.map.base(La + 1) : 0);
    const i64 es = a.map.es;
    const int pslot = selfm ? slot : (slot ^ R);
    const double2 *prow = lds + ((pslot << a.lP) | p) * rowStride;
    for (int j1 = tid >> lNR; j1 < m1; j1 += kstep) {
        const int j = j1 * m2 + col;
        if (j >= n) break;
        const double2 c = row[padi(bitrev(j1, a.lg1))];
        const double2 vk = cmul(make_double2(c.x, -c.y), a.chirp[j]);
        if (INVERSE) {
            const i64 e = clong_makhoul_src(j, n);
            if (oka) da[e * es] = vk.x;
            if (okb) db[e * es] = vk.y;
        } else {
            double2 vm = vk;
            if (j) {
                const int m = n - j;                               // column (r - col) mod m2: the partner slot's
                const double2 cm = prow[padi(bitrev(m >> a.lg2, a.lg1))];
                vm = cmul(make_double2(cm.x, -cm.y), a.chirp[m]);
            }
            const double2 w = a.ww[j];
            // (Xa[k], Xb[k]) = real(ww[k] * V_{a,b}[k])   (the scatter of k_cdft)
            const double2 o = dct_split(vk, vm).at_k(w);
            if (oka) da[j * es] = o.x;
            if (okb) db[j * es] = o.y;
        }
    }
}

int cdft_long_launch(CdftLongPlan *p, const double *src, double *dst, const LineMap &map, bool axis0, int inverse,
                     hipStream_t st) {
    if (map.nLines <= 0) return 0;
    const int m1 = 1 << p->lg1, m2 = 1 << p->lg2;
    const int lrc = long_log2_rows(m1), lrr = long_log2_rows(m2);
    const i64 pairs = (map.nLines + 1) / 2;
    // pairs per tile: strided axes take as many as all three passes can stage (the last pass of the forward transform
    // needs two columns per pair), contiguous lines one
    int lP = 0;
    if (!axis0) {
        const int lb = inverse ? lrc : lrc - 1;
        lP = lb < lrr ? lb : lrr;
        while (lP > 0 && ((i64)1 << lP) > pairs) --lP;
    }
    int lC = lrc - lP, lT = lrr - lP;
    if (lC > p->lg2) lC = p->lg2;
    if (lT > p->lg1) lT = p->lg1;
    const i64 nTiles = (pairs + ((i64)1 << lP) - 1) >> lP;
    const size_t tileBytes = (sizeof(double2) << p->lg) << lP;
    i64 perBatch = (i64)(CLONG_SCRATCH_BYTES / tileBytes);
    if (perBatch < 1) perBatch = 1;
    if (perBatch > nTiles) perBatch = nTiles;
    double2 *scratch = nullptr;
    DS_CHECK(p->scratch.get(st, (size_t)perBatch * tileBytes, &scratch));
    static unsigned long long done = 0;
    if (DeviceOnce once_(done); once_) {
        allow_big_lds(k_clong_cols<false>); allow_big_lds(k_clong_cols<true>);
        allow_big_lds(k_clong_rows);
        allow_big_lds(k_clong_back<false>); allow_big_lds(k_clong_back<true>);
    }
    const size_t ldsC = ((size_t)row_stride(m1) << (lC + lP)) * sizeof(double2);
    const size_t ldsR = ((size_t)row_stride(m2) << (lT + lP)) * sizeof(double2);
    CLongArgs ac{map, p->n, p->lg, p->lg1, p->lg2, lP, lC, 0, p->tw1, p->hi, p->lo, p->chirp, p->ww, p->spec};
    CLongArgs ar{map, p->n, p->lg, p->lg1, p->lg2, lP, lT, 0, p->tw2, p->hi, p->lo, p->chirp, p->ww, p->spec};
    for (i64 t0 = 0; t0 < nTiles; t0 += perBatch) {
        const i64 nb = nTiles - t0 < perBatch ? nTiles - t0 : perBatch;
        ac.tile0 = ar.tile0 = t0;
        const dim3 gc((unsigned)(nb * (m2 >> lC))), gr((unsigned)(nb * (m1 >> lT)));
        if (inverse) DS_KLAUNCH(k_clong_cols<true>, gc, dim3(LONG_THREADS), ldsC, st, src, scratch, ac);
        else DS_KLAUNCH(k_clong_cols<false>, gc, dim3(LONG_THREADS), ldsC, st, src, scratch, ac);
        DS_KLAUNCH(k_clong_rows, gr, dim3(LONG_THREADS), ldsR, st, scratch, ar);
        if (inverse) DS_KLAUNCH(k_clong_back<true>, gc, dim3(LONG_THREADS), ldsC, st, (const double2 *)scratch, dst, ac);
        else DS_KLAUNCH(k_clong_back<false>, gc, dim3(LONG_THREADS), ldsC, st, (const double2 *)scratch, dst, ac);
    }
    DS_HIP(hipGetLastError());
    return 0;
}

}  // namespace dotsocp
