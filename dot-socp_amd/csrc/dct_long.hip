// Power-of-two lines that do not fit the LDS (dct_pow2.hip keeps whole lines there): the two-level ("four-step") FFT
// behind the same Makhoul reordering.  n = n1 n2 (n1 >= n2, both at most 1024), input index j = j1 n2 + j2, output
// index k = k1 + n1 k2:
//   column pass  k_long_cols   n2 transforms of length n1 over j1, times exp(-2 pi i j2 k1 / n), into a complex scratch
//                              array in global memory ([k1][j2], the pairs of a tile interleaved);
//   row pass     k_long_rows   n1 transforms of length n2 over j2, real output.
// Two real lines travel as the real and imaginary part of one complex line, as everywhere else.  The pre- and
// post-processing are fused into the passes: the DCT-II post-processing needs X[k] and X[n - k], and n - k lies in row
// n1 - k1, so a workgroup of the row pass stages rows and their mirrors together; the DCT-III pre-processing needs the
// INPUT elements j and n - j, which the column pass reads from memory both (no transform lies between).  Both levels
// run the register groups of fft_lds.h.  tools/dct_long_proto.py is the numpy model of all of it.
//
// A tile is 2^lP pairs of lines x 2^lT columns (rows) of the n1 x n2 matrix.  Contiguous lines (axis 0): one pair, as
// many consecutive columns / rows as the LDS budget holds; strided axes: as many pairs of lines consecutive in memory
// as it holds.  Every line is addressed through LineMap on its own, so odd line counts, pitched rows and pairs that
// straddle a row need no special case.
#include "cdft.h"
#include "dct_families.h"
#include "device_utils.h"
#include "fft_lds.h"
#include "kernels.h"
#include "long_scratch.h"

#include <cmath>
#include <cstdlib>
#include <vector>

namespace dotsocp {

// Bound of the scratch array of one (plan, stream) pair; a pass over more lines runs in batches of whole tiles.
#define LONG_SCRATCH_BYTES ((size_t)64 << 20)

i64 dct_long_min(int axis) {
    static const i64 forced = [] {
        const char *e = getenv("DOTSOCP_DCT_LONG_MIN");
        if (!e) return (i64)0;
        i64 v = atoll(e), p = 256;        // never below 256; rounded up to a power of two
        while (p < v && p < ((i64)1 << 40)) p <<= 1;
        return p;
    }();
    const i64 first = axis == 0 ? 4096 : 16384;      // the first lengths dct_pow2.hip cannot stage
    return forced && forced < first ? forced : first; // the switch lowers the start, it cannot keep a line in the LDS
}

int dct_levels(i64 n, int axis) {
    if (axis < 0 || axis > 2) return -1;
    if (n <= 1) return 0;
    if (n & (n - 1)) return 1;
    if (n < dct_long_min(axis)) return 1;
    return n <= DCT_LONG_MAX_N ? 2 : -1;
}

int dct_length_check(i64 n) {
    if (n > DCT_LONG_MAX_N && (n & (n - 1)) == 0) {
        set_error("power-of-two DCT length %lld is above the limit of the two-level transform (largest supported: %lld = 2^20)",
                  (long long)n, (long long)DCT_LONG_MAX_N);
        return DOTSOCP_EINVAL;
    }
    // no other family serves a length above 1025 that is not a power of two, and the dense product's n x n matrices are
    // out of reach long before
    if (n > CDFT_LONG_MAX_N && (n & (n - 1)) != 0) {
        set_error("DCT length %lld is not a power of two and above the limit of the two-level Bluestein transform "
                  "(largest supported: %lld = 2^19 - 1)", (long long)n, (long long)CDFT_LONG_MAX_N);
        return DOTSOCP_EINVAL;
    }
    return 0;
}

struct LongPlan {
    i64 n;
    int lg, lg1, lg2;
    double2 *tab = nullptr;                // one allocation: the eight tables below
    const double2 *tw1, *tw2;              // [n1/2], [n2/2]  FFT twiddles of the two levels
    const double2 *hi, *lo;                // exp(-2 pi i m / n) = hi[m / n2] * lo[m % n2], m = j2 k1 < n
    const double2 *fa, *fb;                // ww[k1 + n1 k2] = fa[k1] * fb[k2]   (k > 0; ww of dct_pow2.hip)
    const double2 *ia, *ib;                // ww[j1 n2 + j2] = ia[j1] * ib[j2]
    LongScratch scratch;                   // long_scratch.h: one array per stream
};

LongPlan *long_plan_create(i64 n) {
    if (n < 256 || n > DCT_LONG_MAX_N || (n & (n - 1))) return nullptr;
    LongPlan *p = new LongPlan();
    p->n = n;
    p->lg = ceil_log2(n);
    p->lg2 = p->lg / 2;
    p->lg1 = p->lg - p->lg2;
    const i64 n1 = (i64)1 << p->lg1, n2 = (i64)1 << p->lg2;
    std::vector<double2> t;
    t.reserve((size_t)(n1 / 2 + n2 / 2 + 3 * n1 + 3 * n2));
    const long double sc = 2.0L / sqrtl(2.0L * (long double)n);
    size_t off[8];
    off[0] = t.size(); for (i64 k = 0; k < n1 / 2; ++k) t.push_back(unit_root(k, n1));
    off[1] = t.size(); for (i64 k = 0; k < n2 / 2; ++k) t.push_back(unit_root(k, n2));
    off[2] = t.size(); for (i64 k = 0; k < n1; ++k) t.push_back(unit_root(k, n1));
    off[3] = t.size(); for (i64 k = 0; k < n2; ++k) t.push_back(unit_root(k, n));
    // sc * exp(-i pi k / 2n) in long double, rounded once
    auto half = [&](i64 num, i64 den, bool with_sc) {
        const long double PI = 3.141592653589793238462643383279502884L;
        const long double a = -2.0L * PI * (long double)(num % den) / (long double)den;
        const long double s = with_sc ? sc : 1.0L;
        return make_double2((double)(s * cosl(a)), (double)(s * sinl(a)));
    };
    off[4] = t.size(); for (i64 k = 0; k < n1; ++k) t.push_back(half(k, 4 * n, true));
    off[5] = t.size(); for (i64 k = 0; k < n2; ++k) t.push_back(half(k, 4 * n2, false));
    off[6] = t.size(); for (i64 k = 0; k < n1; ++k) t.push_back(half(k, 4 * n1, true));
    off[7] = t.size(); for (i64 k = 0; k < n2; ++k) t.push_back(half(k, 4 * n, false));
    if (hipMalloc(&p->tab, sizeof(double2) * t.size()) != hipSuccess) {
        (void)hipGetLastError();
        delete p;
        return nullptr;
    }
    (void)hipMemcpy(p->tab, t.data(), sizeof(double2) * t.size(), hipMemcpyHostToDevice);
    p->tw1 = p->tab + off[0]; p->tw2 = p->tab + off[1];
    p->hi = p->tab + off[2];  p->lo = p->tab + off[3];
    p->fa = p->tab + off[4];  p->fb = p->tab + off[5];
    p->ia = p->tab + off[6];  p->ib = p->tab + off[7];
    return p;
}

void long_plan_destroy(LongPlan *p) {
    if (!p) return;
    p->scratch.release();
    if (p->tab) (void)hipFree(p->tab);
    delete p;
}

struct LongArgs {
    LineMap map;
    int lg, lg1, lg2;
    int lP;            // log2(pairs of lines per tile)
    int lT;            // log2(columns per tile) in the column pass, log2(rows per tile) in the row pass
    i64 tile0;         // first tile of pairs of this batch
    const double2 *tw, *ta, *tb, *hi, *lo;     // the level's FFT twiddles; ia / ib resp. fa / fb; hi / lo
};

// source element of position j of the Makhoul-ordered line (v[j] = x[2j], v[n-1-j] = x[2j+1]); also where output
// position j of the inverse goes
__device__ __forceinline__ i64 makhoul_src(i64 j, i64 n) { return j < (n >> 1) ? 2 * j : 2 * (n - 1 - j) + 1; }

// ---------------------------------------------------------------------------------------------
// Column pass.  Workgroup = (tile of pairs) x (2^lT consecutive columns j2): row s = (c << lP) | p of the LDS holds
// column j2 = col0 + c of pair p, all n1 elements.  A thread keeps its row s for the whole kernel (LONG_THREADS is a
// multiple of the rows), so its line addresses are formed once.
// ---------------------------------------------------------------------------------------------
template <bool INVERSE>
__global__ void __launch_bounds__(LONG_THREADS) k_long_cols(const double *__restrict__ src, double2 *__restrict__ scratch,
                                                             LongArgs a) {
    extern __shared__ double2 lds[];
    const int n1 = 1 << a.lg1, n2 = 1 << a.lg2;
    const i64 n = (i64)1 << a.lg;
    const int rowStride = row_stride(n1);
    const int lNR = a.lT + a.lP, NR = 1 << lNR;
    const int tid = threadIdx.x;
    const unsigned nColTiles = (unsigned)(n2 >> a.lT);
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
    double2 eb = make_double2(0.0, 0.0);
    if (INVERSE) eb = a.tb[j2];
    for (int j0 = tid >> lNR; j0 < n1; j0 += jstep * LONG_BATCH) {
        double2 xk[LONG_BATCH], xm[LONG_BATCH];
#pragma unroll
        for (int u = 0; u < LONG_BATCH; ++u) {
            const int j1 = j0 + u * jstep;
            xk[u] = make_double2(0.0, 0.0);
            xm[u] = xk[u];
            if (j1 < n1) {
                const i64 j = (i64)j1 * n2 + j2;
                const i64 e = INVERSE ? j : makhoul_src(j, n);
                if (oka) xk[u].x = sa[e * es];
                if (okb) xk[u].y = sb[e * es];
                if (INVERSE) {
                    const i64 em = (n - j) & (n - 1);
                    if (oka) xm[u].x = sa[em * es];
                    if (okb) xm[u].y = sb[em * es];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < LONG_BATCH; ++u) {
            const int j1 = j0 + u * jstep;
            if (j1 >= n1) break;
            if (!INVERSE) {
                row[padi(j1)] = xk[u];
            } else {
                // G[j] = (ww[j] X[j] + conj(ww[n-j]) X[n-j]) / 2, G[0] = ww[0] X[0]   (idct_combine of dct_pow2.hip);
                // ww[j] = ia[j1] ib[j2], ww[n-j] = (-imag ww[j], -real ww[j])
                const double2 wk = cmul(a.ta[j1], eb);
                if (j1 == 0 && j2 == 0) {
                    const double w0 = wk.x * 0.70710678118654752440;
                    row[0] = make_double2(w0 * xk[u].x, w0 * xk[u].y);
                } else {
                    const double2 wm = make_double2(-wk.y, -wk.x);
                    row[padi(j1)] = idct_half(wk, xk[u], wm, xm[u]);
                }
            }
        }
    }
    __syncthreads();
    fft_rows<false>(lds, lNR, a.lg1, rowStride, BlockTeam<LONG_THREADS>{tid}, a.tw);
    // times exp(-2 pi i j2 k1 / n), to scratch[k1][j2] of this tile (pairs interleaved: the lanes of a row group are adjacent)
    double2 *out = scratch + (((pt << a.lg) + j2) << a.lP) + p;
    for (int k1 = tid >> lNR; k1 < n1; k1 += jstep) {
        const double2 v = row[padi(bitrev(k1, a.lg1))];
        const int m = j2 * k1;
        const double2 w = cmul(a.hi[m >> a.lg2], a.lo[m & (n2 - 1)]);
        out[((i64)k1 << a.lg2) << a.lP] = cmul(v, w);
    }
}

// ---------------------------------------------------------------------------------------------
// Row pass.  Workgroup = (tile of pairs) x (2^lT rows k1): LDS row s = (slot << lP) | p.  Inverse: the rows
// k1 = (g << lT) + slot.  Forward: with R = 2^(lT-1), slot r < R holds row a = g R + 1 + r and slot R + r its mirror
// n1 - a -- the row that holds X[n - k] for the k of row a and the other way round; the one row that is its own mirror
// (n1 / 2, last group) leaves its mirror slot to row 0, whose partner elements lie in row 0 itself.
// ---------------------------------------------------------------------------------------------
template <bool INVERSE>
__global__ void __launch_bounds__(LONG_THREADS) k_long_rows(const double2 *__restrict__ scratch, double *__restrict__ dst,
                                                             LongArgs a) {
    extern __shared__ double2 lds[];
    const int n1 = 1 << a.lg1, n2 = 1 << a.lg2;
    const i64 n = (i64)1 << a.lg;
    const int rowStride = row_stride(n2);
    const int lNR = a.lT + a.lP, NR = 1 << lNR;
    const int P = 1 << a.lP;
    const int tid = threadIdx.x;
    const unsigned nRowTiles = (unsigned)(n1 >> a.lT);
    const int g = (int)(blockIdx.x % nRowTiles);
    const i64 pt = blockIdx.x / nRowTiles;
    const int R = INVERSE ? 1 : 1 << (a.lT - 1);
    auto row_of = [&](int slot) {
        if (INVERSE) return (g << a.lT) + slot;
        const int ra = g * R + 1 + (slot & (R - 1));
        if (slot < R) return ra;
        return (n1 - ra == ra) ? 0 : n1 - ra;
    };
    // ---- load: (slot, j2, p) with p fastest: whole rows of the scratch array, contiguous ----
    {
        const double2 *in = scratch + ((pt << a.lg) << a.lP);
        const int total = n2 << lNR;
        for (int b0 = tid; b0 < total; b0 += LONG_THREADS * LONG_BATCH) {
            double2 v[LONG_BATCH];
#pragma unroll
            for (int u = 0; u < LONG_BATCH; ++u) {
                const int b = b0 + u * LONG_THREADS;
                v[u] = make_double2(0.0, 0.0);
                if (b < total) {
                    const int slot = b >> (a.lP + a.lg2);
                    v[u] = in[(((i64)row_of(slot) << a.lg2) << a.lP) + (b & ((n2 << a.lP) - 1))];
                }
            }
#pragma unroll
            for (int u = 0; u < LONG_BATCH; ++u) {
                const int b = b0 + u * LONG_THREADS;
                if (b >= total) break;
                const int slot = b >> (a.lP + a.lg2), j2 = (b >> a.lP) & (n2 - 1), p = b & (P - 1);
                lds[((slot << a.lP) | p) * rowStride + padi(j2)] = v[u];
            }
        }
    }
    __syncthreads();
    fft_rows<false>(lds, lNR, a.lg2, rowStride, BlockTeam<LONG_THREADS>{tid}, a.tw);
    // ---- store: (k2, slot, p) with p, then the slot fastest; a thread keeps its row ----
    const int s = tid & (NR - 1);
    const int p = s & (P - 1), slot = s >> a.lP;
    const int k1 = row_of(slot);
    const i64 La = 2 * (((a.tile0 + pt) << a.lP) + p);
    const bool oka = La < a.map.nLines, okb = La + 1 < a.map.nLines;
    double *da = dst + (oka ? a.map.base(La) : 0), *db = dst + (okb ? a.map.base(La + 1) : 0);
    const i64 es = a.map.es;
    const double2 *row = lds + s * rowStride;
    const int kstep = LONG_THREADS >> lNR;
    if (INVERSE) {
        for (int k2 = tid >> lNR; k2 < n2; k2 += kstep) {
            const double2 v = row[padi(bitrev(k2, a.lg2))];
            const i64 e = makhoul_src((i64)k1 + ((i64)k2 << a.lg1), n);
            if (oka) da[e * es] = v.x;
            if (okb) db[e * es] = v.y;
        }
    } else {
        const int ra = g * R + 1 + (slot & (R - 1));
        const int pslot = (n1 - ra == ra) ? slot : (slot ^ R);
        const double2 *prow = lds + ((pslot << a.lP) | p) * rowStride;
        const double2 wa = a.ta[k1];
        for (int k2 = tid >> lNR; k2 < n2; k2 += kstep) {
            const int pk2 = k1 == 0 ? ((n2 - k2) & (n2 - 1)) : n2 - 1 - k2;
            const double2 vk = row[padi(bitrev(k2, a.lg2))], vm = prow[padi(bitrev(pk2, a.lg2))];
            double2 w = cmul(wa, a.tb[k2]);
            if (k1 == 0 && k2 == 0) w = make_double2(w.x * 0.70710678118654752440, 0.0);
            // (Xa[k], Xb[k]) = real(ww[k] * V_{a,b}[k])   (dct_post of dct_pow2.hip)
            const double2 o = dct_split(vk, vm).at_k(w);
            const i64 e = (i64)k1 + ((i64)k2 << a.lg1);
            if (oka) da[e * es] = o.x;
            if (okb) db[e * es] = o.y;
        }
    }
}

int long_launch(LongPlan *p, const double *src, double *dst, const LineMap &map, bool axis0, int inverse, hipStream_t st) {
    if (map.nLines <= 0) return 0;
    const int n1 = 1 << p->lg1, n2 = 1 << p->lg2;
    const int lrc = long_log2_rows(n1), lrr = long_log2_rows(n2);
    const i64 pairs = (map.nLines + 1) / 2;
    // pairs per tile: strided axes take as many as both passes can stage (the row pass of the forward transform needs
    // two rows per pair), contiguous lines one
    int lP = 0;
    if (!axis0) {
        lP = (inverse ? lrr : lrr - 1) < lrc ? (inverse ? lrr : lrr - 1) : lrc;
        while (lP > 0 && ((i64)1 << lP) > pairs) --lP;
    }
    int lC = lrc - lP, lT = lrr - lP;
    if (lC > p->lg2) lC = p->lg2;
    if (lT > p->lg1) lT = p->lg1;
    const i64 nTiles = (pairs + ((i64)1 << lP) - 1) >> lP;
    const size_t tileBytes = (sizeof(double2) << p->lg) << lP;
    i64 perBatch = (i64)(LONG_SCRATCH_BYTES / tileBytes);
    if (perBatch < 1) perBatch = 1;
    if (perBatch > nTiles) perBatch = nTiles;
    double2 *scratch = nullptr;
    DS_CHECK(p->scratch.get(st, (size_t)perBatch * tileBytes, &scratch));
    static unsigned long long done = 0;
    if (DeviceOnce once_(done); once_) {
        allow_big_lds(k_long_cols<false>); allow_big_lds(k_long_cols<true>);
        allow_big_lds(k_long_rows<false>); allow_big_lds(k_long_rows<true>);
    }
    const size_t ldsC = ((size_t)row_stride(n1) << (lC + lP)) * sizeof(double2);
    const size_t ldsR = ((size_t)row_stride(n2) << (lT + lP)) * sizeof(double2);
    LongArgs ac{map, p->lg, p->lg1, p->lg2, lP, lC, 0, p->tw1, p->ia, p->ib, p->hi, p->lo};
    LongArgs ar{map, p->lg, p->lg1, p->lg2, lP, lT, 0, p->tw2, p->fa, p->fb, p->hi, p->lo};
    for (i64 t0 = 0; t0 < nTiles; t0 += perBatch) {
        const i64 nb = nTiles - t0 < perBatch ? nTiles - t0 : perBatch;
        ac.tile0 = ar.tile0 = t0;
        const dim3 gc((unsigned)(nb * (n2 >> lC))), gr((unsigned)(nb * (n1 >> lT)));
        if (inverse) {
            DS_KLAUNCH(k_long_cols<true>, gc, dim3(LONG_THREADS), ldsC, st, src, scratch, ac);
            DS_KLAUNCH(k_long_rows<true>, gr, dim3(LONG_THREADS), ldsR, st, (const double2 *)scratch, dst, ar);
        } else {
            DS_KLAUNCH(k_long_cols<false>, gc, dim3(LONG_THREADS), ldsC, st, src, scratch, ac);
            DS_KLAUNCH(k_long_rows<false>, gr, dim3(LONG_THREADS), ldsR, st, (const double2 *)scratch, dst, ar);
        }
    }
    DS_HIP(hipGetLastError());
    return 0;
}

}  // namespace dotsocp
