// The power-of-two family of the DCT dispatcher (dct.hip): Makhoul's reordering + one complex FFT per PAIR of real
// lines (line a in the real part, line b in the imaginary part), entirely in LDS: one HBM read and one HBM write per
// element and axis.  A workgroup stages TL lines; for the strided axes (x, t) the TL lines are consecutive in y so that
// global accesses stay coalesced.  Three generations of kernels, picked by the launchers at the end of the file: one
// wave per row (k_dct_axis0, k_dct_strided: short lines, unaligned lines, the fused t solve of short lines), the whole
// workgroup per tile (_wg), and persistent workgroups fed by LDS-DMA (_pipe; DOTSOCP_DCT_PIPE=0 switches them off).
#include "dct_families.h"
#include "device_utils.h"
#include "fft_lds.h"
#include "kernels.h"

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include <vector>

namespace dotsocp {

struct Pow2Plan {
    i64 n;
    int lg;         // n = 2^lg
    double2 *tw;    // [n/2]  exp(-2 pi i k / n)
    double2 *ww;    // [n]    2 exp(-i pi k / 2n) / sqrt(2n), ww[0] /= sqrt(2)   (mirt_dctn.m:69-70)
    LongPlan *lng;  // lines of this length leave the LDS along some axis: the two-level transform (dct_long.hip)
};

Pow2Plan *pow2_plan_create(i64 n) {
    Pow2Plan *p = new Pow2Plan();
    p->n = n;
    p->lg = ceil_log2(n);
    p->tw = nullptr;
    p->ww = nullptr;
    p->lng = nullptr;
    if (n > DCT_LONG_MAX_N) {                // refused when the plan is made (dct_length_check has the message)
        delete p;
        return nullptr;
    }
    const i64 firstLong = dct_long_min(0) < dct_long_min(1) ? dct_long_min(0) : dct_long_min(1);
    if (n >= firstLong && !(p->lng = long_plan_create(n))) {
        delete p;
        return nullptr;
    }
    if (n >= dct_long_min(0) && n >= dct_long_min(1)) return p;      // no axis keeps such lines in the LDS: no tables
    const long double PI = 3.141592653589793238462643383279502884L;
    std::vector<double2> tw(n / 2), ww(n);
    for (i64 k = 0; k < n / 2; ++k) {
        long double a = -2.0L * PI * (long double)k / (long double)n;
        tw[k] = make_double2((double)cosl(a), (double)sinl(a));
    }
    for (i64 k = 0; k < n; ++k) {
        long double a = -PI * (long double)k / (2.0L * (long double)n);
        long double sc = 2.0L / sqrtl(2.0L * (long double)n);
        if (k == 0) sc /= sqrtl(2.0L);
        ww[k] = make_double2((double)(sc * cosl(a)), (double)(sc * sinl(a)));
    }
    if (hipMalloc(&p->tw, sizeof(double2) * (n / 2)) != hipSuccess ||
        hipMalloc(&p->ww, sizeof(double2) * n) != hipSuccess) {
        pow2_plan_destroy(p);
        return nullptr;
    }
    (void)hipMemcpy(p->tw, tw.data(), sizeof(double2) * (n / 2), hipMemcpyHostToDevice);
    (void)hipMemcpy(p->ww, ww.data(), sizeof(double2) * n, hipMemcpyHostToDevice);
    return p;
}

void pow2_plan_destroy(Pow2Plan *p) {
    if (!p) return;
    if (p->tw) (void)hipFree(p->tw);
    if (p->ww) (void)hipFree(p->ww);
    long_plan_destroy(p->lng);
    delete p;
}

// ---------------------------------------------------------------------------------------------
// Steps: what every kernel below does to a staged tile, each written once.
// ---------------------------------------------------------------------------------------------
#define DCT_WAVES 4
#define DCT_BATCH 8   // global loads in flight per lane before the first dependent LDS write
// Twiddle tables as the kernels see them: a plain pointer, or -- for the 2048-point lines of the pipelined kernels, whose
// two tile buffers leave 32 KB of LDS for tables -- the symmetric part only:
//   exp(-2 pi i (j + n/4) / n) = -i exp(-2 pi i j / n)               -> a quarter of the FFT twiddles,
//   ww[n - k] = (-imag ww[k], -real ww[k])   (0 < k < n/2)           -> half of the DCT weights (+ the entry n/2).
// (The sizes are template constants, not members: a member is a constant for the optimiser only after the view has been
// taken apart, and which products of the butterflies it fuses with their sums turned out to depend on when that is.)
template <int Q /* n / 4 entries */>
struct TwQuarter {
    const double2 *t;
    __device__ __forceinline__ double2 operator[](int j) const {
        const double2 v = t[j & (Q - 1)];
        return (j & Q) ? make_double2(v.y, -v.x) : v;
    }
};
template <int H /* n / 2: entries 0 .. H */>
struct WwHalf {
    const double2 *t;
    __device__ __forceinline__ double2 operator[](int m) const {
        const double2 v = t[m <= H ? m : 2 * H - m];
        return (m <= H) ? v : make_double2(-v.y, -v.x);
    }
};

// Where a staged tile keeps element p of its row r, and how a loop over (row, index < 2^li) items deals them out.
// Plain rows `stride` apart, the index fastest:
struct RowsLayout {
    double2 *rows;
    int stride, lrows;      // 2^lrows rows
    static constexpr bool UNROLL = false;
    __device__ __forceinline__ double2 &operator()(int r, int p) const { return (rows + r * stride)[padi(p)]; }
    __device__ __forceinline__ void split(int b, int li, int &r, int &i) const { r = b >> li; i = b & ((1 << li) - 1); }
};
// The pair-interleaved tile an LDS-DMA piece leaves (k_dct_strided_pipe), the row fastest:
template <int LROWS>
struct TileLayout {
    double2 *tile;
    static constexpr int lrows = LROWS;
    static constexpr bool UNROLL = true;
    __device__ __forceinline__ double2 &operator()(int r, int p) const { return tile[(padi(p) << LROWS) + r]; }
    __device__ __forceinline__ void split(int b, int, int &r, int &i) const { r = b & ((1 << LROWS) - 1); i = b >> LROWS; }
};

// LDS position of input element k while staging a line: forward transforms take the Makhoul order, the inverse
// the natural one, the fused t-axis solve the bit-reversed Makhoul order (its forward FFT is decimation-in-time)
template <int MODE>
__device__ __forceinline__ int stage_pos(int k, int n, int lg) {
    return MODE == 1 ? k : (MODE == 2 ? bitrev(makhoul(k, n), lg) : makhoul(k, n));
}

// Inverse pre-processing of the team's rows in place (natural order, Xa + i Xb elementwise): idct_half on every pair
// (k, n - k), both by the same thread, and G[0] = ww[0] X[0].
template <class TEAM, class LAYOUT, class WW = const double2 *>
__device__ __forceinline__ void idct_combine(LAYOUT at, int lg, TEAM tm, WW ww) {
    const int n = 1 << lg, lh = lg - 1;
    const int total = 1 << (at.lrows + lh);
    auto pair = [&](int b) {
        int r, i;
        at.split(b, lh, r, i);
        const int k = i + 1, m = n - k;                   // k = 1 .. n/2
        double2 &ek = at(r, k), &em = at(r, m);
        const double2 xk = ek, xm = em;
        const double2 wk = ww[k], wm = ww[m];
        ek = idct_half(wk, xk, wm, xm);
        if (m != k) em = idct_half(wm, xm, wk, xk);
    };
    if constexpr (LAYOUT::UNROLL) {                       // a few items per thread, their count known when compiling
#pragma unroll
        for (int b = tm.t; b < total; b += TEAM::T) pair(b);
    } else {
        for (int b = tm.t; b < total; b += TEAM::T) pair(b);
    }
    if (tm.t < (1 << at.lrows)) {
        double2 &e0 = at(tm.t, 0);
        const double w0 = ww[0].x;
        e0 = make_double2(w0 * e0.x, w0 * e0.y);
    }
    TEAM::sync();
}

// (Xa[k], Xb[k]) from the bit-reversed FFT of va + i vb in row r (LES: of a pair-interleaved tile)
template <int LES = 0, class WW = const double2 *>
__device__ __forceinline__ double2 dct_post(const double2 *__restrict__ r, int k, int n, int lg, WW ww) {
    const double2 vk = r[padi(bitrev(k, lg)) << LES];
    const double2 vm = r[padi(bitrev((n - k) & (n - 1), lg)) << LES];
    const double2 w = ww[k];
    return dct_split(vk, vm).at_k(w);
}

// The fused t step: forward post-processing, division by the spectral kernel, inverse pre-processing.
struct SolveArgs {
    i64 ny, line0, nplane; // local line L is column (y, x) = (G % ny, G / ny), G = line0 + L, of ny*nx = nplane columns
    double kscale;
    const double *cy, *cx, *ct;
};

// lambda == 0 (the constant mode of the Neumann problem) divides by kscale alone
__device__ __forceinline__ double tsolve_lambda(double e, double ct) {
    double l = e + ct;
    if (l == 0.0) l = 1.0;
    return l;
}

// On the pair (ek, em) = (V[k], V[m]), m = n - k, of one row, in place, from the natural-order spectrum V of va + i vb:
// X = dct_split weighted, Y = X / (kscale * lambda), G = idct_half; .x of X, Y is line a, .y line b.  ea / eb: CY + CX
// of line a / b; ww, ct: the weights and CT as the kernel keeps them (global memory or LDS).  m == k: em is ek.
// The operands are read here, the spectrum first, and not by the caller: the order of the loads decides how the
// compiler orders the operands of the sums below, and with that which product it contracts into each of them.
template <class WW, class CT>
__device__ __forceinline__ void tsolve_pair(double2 &ek, double2 &em, int k, int m, WW ww, CT ct, double ea, double eb,
                                            double kscale) {
    const double2 vk = ek, vm = em;
    const double2 wk = ww[k], wm = ww[m];
    const DctSplit s = dct_split(vk, vm);
    const double ctk = ct[k], ctm = ct[m];
    const double lak = tsolve_lambda(ea, ctk), lbk = tsolve_lambda(eb, ctk);
    const double lam = tsolve_lambda(ea, ctm), lbm = tsolve_lambda(eb, ctm);
    const double2 pk = s.at_k(wk), pm = s.at_m(wm);
    const double2 xk = make_double2(pk.x / (kscale * lak), pk.y / (kscale * lbk));
    const double2 xm = make_double2(pm.x / (kscale * lam), pm.y / (kscale * lbm));
    ek = idct_half(wk, xk, wm, xm);
    if (m != k) em = idct_half(wm, xm, wk, xk);
}

// k = 0: V[0] is its own partner
__device__ __forceinline__ double2 tsolve_dc(double2 v0, double w0, double ea, double eb, double ct0, double kscale) {
    const double la = tsolve_lambda(ea, ct0), lb = tsolve_lambda(eb, ct0);
    return make_double2(w0 * ((w0 * v0.x) / (kscale * la)), w0 * ((w0 * v0.y) / (kscale * lb)));
}

// Axis 0, staging: A = elements 2j, 2j + 1 of line a, B of line b -> row r (Makhoul order forward: x[2j] -> v[j],
// x[2j+1] -> v[n-1-j]; natural order inverse)
template <bool INVERSE>
__device__ __forceinline__ void axis0_stage(double2 *r, int j, int n, double2 A, double2 B) {
    if (!INVERSE) {
        r[padi(j)] = make_double2(A.x, B.x);
        r[padi(n - 1 - j)] = make_double2(A.y, B.y);
    } else {
        r[padi(2 * j)] = make_double2(A.x, B.x);
        r[padi(2 * j + 1)] = make_double2(A.y, B.y);
    }
}

// Axis 0, read-out of the transformed row r: elements 2j, 2j + 1 of the two result lines (forward: dct_post; inverse:
// x[2j] = v[j], x[2j+1] = v[n-1-j] from the bit-reversed row)
template <bool INVERSE, class WW = const double2 *>
__device__ __forceinline__ void axis0_unstage(const double2 *r, int j, int n, int lg, WW ww, double2 &A, double2 &B) {
    if (!INVERSE) {
        const double2 p0 = dct_post(r, 2 * j, n, lg, ww), p1 = dct_post(r, 2 * j + 1, n, lg, ww);
        A = make_double2(p0.x, p1.x);
        B = make_double2(p0.y, p1.y);
    } else {
        const double2 v0 = r[padi(bitrev(j, lg))], v1 = r[padi(bitrev(n - 1 - j, lg))];
        A = make_double2(v0.x, v1.x);
        B = make_double2(v0.y, v1.y);
    }
}

// Strided axes, 16-byte accesses (one carries both lines of a pair): thread tid of T loads / stores the elements
// tid >> lp, + T >> lp, ... of ITS pair of the tile that starts at line L0, row r of the LDS.  DCT_BATCH loads are issued
// before the first LDS write so that their latencies overlap.
struct PairOfLines {
    int r;
    bool ok;        // the pair exists (its second line too: the line count is even where VEC is taken)
    i64 lb;         // element offset of its first line
    __device__ __forceinline__ PairOfLines(const LineMap &map, int lp, i64 L0, int tid) {
        r = tid & ((1 << lp) - 1);
        const i64 L = L0 + 2 * r;
        ok = L < map.nLines;
        lb = ok ? map.base(L) : 0;
    }
};

template <int MODE, int T>
__device__ __forceinline__ void strided_load_vec(const double *__restrict__ src, const LineMap &map, double2 *lds, int lg,
                                                 int lp, PairOfLines pl, int tid) {
    const int n = 1 << lg, rowStride = row_stride(n);
    const int r = pl.r;
    const bool ok = pl.ok;
    const i64 lb = pl.lb;
    const int kstep = T >> lp;
    for (int k0 = tid >> lp; k0 < n; k0 += kstep * DCT_BATCH) {
        double2 gv[DCT_BATCH];
#pragma unroll
        for (int u = 0; u < DCT_BATCH; ++u) {
            const int k = k0 + u * kstep;
            gv[u] = (ok && k < n) ? *(const double2 *)(src + lb + (i64)k * map.es) : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < DCT_BATCH; ++u) {
            const int k = k0 + u * kstep;
            if (k < n) lds[r * rowStride + padi(stage_pos<MODE>(k, n, lg))] = gv[u];
        }
    }
}

template <int MODE, int T>
__device__ __forceinline__ void strided_store_vec(double *__restrict__ dst, const LineMap &map, const double2 *lds, int lg,
                                                  int lp, PairOfLines pl, int tid, const double2 *__restrict__ ww) {
    const int n = 1 << lg, rowStride = row_stride(n);
    if (pl.ok) {
        const double2 *rr = lds + pl.r * rowStride;
        for (int k = tid >> lp; k < n; k += T >> lp) {
            double2 v;
            if (MODE == 0) v = dct_post(rr, k, n, lg, ww);
            else v = rr[padi(bitrev(makhoul(k, n), lg))];
            *(double2 *)(dst + pl.lb + (i64)k * map.es) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// In-LDS kernels, axis 0 (lines contiguous in memory): a team stages 2^lrows complex rows (pairs of consecutive lines,
// the first one pair0) with 16-byte global accesses, transforms them and writes them back.
//   k_dct_axis0     every wave works alone on its own rows -- no workgroup barrier at all
//   k_dct_axis0_wg  ALL threads of the workgroup share ALL staged rows (register groups dealt round-robin,
//                   __syncthreads() between them): twice the waves per staged row at the same LDS footprint -- the
//                   footprint, not registers, caps the resident workgroups per CU, so this doubles the waves that
//                   overlap VALU, LDS and HBM phases
// ---------------------------------------------------------------------------------------------
template <bool INVERSE, class TEAM>
__device__ __forceinline__ void dct_axis0_body(const double *__restrict__ src, double *__restrict__ dst, i64 nLines,
                                               i64 ls /* doubles between lines */, int lg, int lrows, double2 *rows,
                                               i64 pair0, TEAM tm, const double2 *__restrict__ tw,
                                               const double2 *__restrict__ ww) {
    const int n = 1 << lg, lh = lg - 1;
    const int rowStride = row_stride(n);
    const int total = 1 << (lrows + lh);                                  // (row, j) with j = k / 2
    // ---- load: two consecutive elements of both lines per thread; DCT_BATCH iterations' worth of
    // 16-byte global loads are issued before the first LDS write so that their latencies overlap ----
    for (int b0 = tm.t; b0 < total; b0 += TEAM::T * DCT_BATCH) {
        double2 A[DCT_BATCH], B[DCT_BATCH];
#pragma unroll
        for (int u = 0; u < DCT_BATCH; ++u) {
            const int b = b0 + TEAM::T * u;
            const int rr = b >> lh, j = b & ((1 << lh) - 1);
            const i64 La = 2 * (pair0 + rr);
            A[u] = make_double2(0.0, 0.0);
            B[u] = A[u];
            if (b < total && La < nLines) A[u] = *(const double2 *)(src + La * ls + 2 * j);
            if (b < total && La + 1 < nLines) B[u] = *(const double2 *)(src + (La + 1) * ls + 2 * j);
        }
#pragma unroll
        for (int u = 0; u < DCT_BATCH; ++u) {
            const int b = b0 + TEAM::T * u;
            if (b >= total) break;
            axis0_stage<INVERSE>(rows + (b >> lh) * rowStride, b & ((1 << lh) - 1), n, A[u], B[u]);
        }
    }
    TEAM::sync();
    if (INVERSE) idct_combine(RowsLayout{rows, rowStride, lrows}, lg, tm, ww);
    fft_rows<false>(rows, lrows, lg, rowStride, tm, tw);
    // ---- store ----
    for (int b = tm.t; b < total; b += TEAM::T) {
        const int rr = b >> lh, j = b & ((1 << lh) - 1);
        const i64 La = 2 * (pair0 + rr);
        double2 A, B;
        axis0_unstage<INVERSE>(rows + rr * rowStride, j, n, lg, ww, A, B);
        if (La < nLines) *(double2 *)(dst + La * ls + 2 * j) = A;
        if (La + 1 < nLines) *(double2 *)(dst + (La + 1) * ls + 2 * j) = B;
    }
}

template <bool INVERSE>
__global__ void __launch_bounds__(DCT_THREADS) k_dct_axis0(const double *__restrict__ src, double *__restrict__ dst,
                                                            i64 nLines, i64 ls, int lg, int lrw /* rows of ONE wave */,
                                                            const double2 *__restrict__ tw,
                                                            const double2 *__restrict__ ww) {
    extern __shared__ double2 lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    dct_axis0_body<INVERSE>(src, dst, nLines, ls, lg, lrw, lds + (wave << lrw) * row_stride(1 << lg),
                            ((i64)blockIdx.x * DCT_WAVES + wave) << lrw, WaveTeam{lane}, tw, ww);
}

#define DCT_WG_THREADS 512
template <bool INVERSE>
__global__ void __launch_bounds__(DCT_WG_THREADS, 4) k_dct_axis0_wg(const double *__restrict__ src,
                                                                     double *__restrict__ dst, i64 nLines, i64 ls, int lg,
                                                                     int lrows, const double2 *__restrict__ tw,
                                                                     const double2 *__restrict__ ww) {
    extern __shared__ double2 lds[];
    dct_axis0_body<INVERSE>(src, dst, nLines, ls, lg, lrows, lds, (i64)blockIdx.x << lrows,
                            BlockTeam<DCT_WG_THREADS>{(int)threadIdx.x}, tw, ww);
}

// ---------------------------------------------------------------------------------------------
// In-LDS kernels, strided axes (x, t): the workgroup stages 2^lp complex rows = 2^(lp+1) lines that are CONSECUTIVE in
// memory and loads / stores them cooperatively (VEC: strided_load_vec / strided_store_vec).
//   k_dct_strided     every wave runs the FFT of its own rows between the two barriers.  MODE 2: the fused t solve --
//                     forward DCT, division by the spectral kernel, inverse DCT in one pass
//   k_dct_strided_wg  the whole workgroup shares all rows (forward / inverse, 16-byte accesses only)
// ---------------------------------------------------------------------------------------------
template <int MODE /*0 fwd, 1 inv, 2 t-solve*/, bool VEC>
__global__ void __launch_bounds__(DCT_THREADS) k_dct_strided(const double *__restrict__ src, double *__restrict__ dst,
                                                              LineMap map, int lg, int lp, SolveArgs sa,
                                                              const double2 *__restrict__ tw,
                                                              const double2 *__restrict__ ww) {
    extern __shared__ double2 lds[];
    const int n = 1 << lg;
    const int rowStride = row_stride(n);
    const int npairs = 1 << lp;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const i64 L0 = xcd_tile(blockIdx.x, gridDim.x) << (lp + 1);
    // rows of this wave: npairs / 4 each (all rows go to the first waves when npairs < 4)
    const int lrw = (lp >= 2) ? lp - 2 : 0;
    const bool waveActive = (wave << lrw) < npairs;
    double2 *rows = lds + (wave << lrw) * rowStride;
    const WaveTeam team{lane};
    const RowsLayout at{rows, rowStride, lrw};
    // ---- cooperative load ----
    if (VEC) {
        strided_load_vec<MODE, DCT_THREADS>(src, map, lds, lg, lp, PairOfLines(map, lp, L0, tid), tid);
    } else {
        const int l = tid & (2 * npairs - 1);
        const i64 L = L0 + l;
        const bool ok = L < map.nLines;
        const i64 lb = ok ? map.base(L) : 0;
        for (int k = tid >> (lp + 1); k < n; k += DCT_THREADS >> (lp + 1)) {
            const double g = ok ? src[lb + (i64)k * map.es] : 0.0;
            ((double *)&lds[(l >> 1) * rowStride + padi(stage_pos<MODE>(k, n, lg))])[l & 1] = g;
        }
    }
    __syncthreads();
    if (waveActive) {
        if (MODE == 1) idct_combine(at, lg, team, ww);
        if (MODE != 2) {
            fft_rows<false>(rows, lrw, lg, rowStride, team, tw);
        } else {
            // forward transform with natural-order output, the fused t step in place -- the lane that owns k also owns
            // n-k --, then the inverse transform on the same rows
            fft_rows<true>(rows, lrw, lg, rowStride, team, tw);
            // CY + CX of the two lines of row rr of this wave
            // (an odd line count leaves the last pair with line a alone: it keeps ITS eigenvalue, line b's is unused)
            auto eigen = [&](int rr, double &ea, double &eb) {
                i64 La = L0 + 2 * ((wave << lrw) + rr);
                if (La >= map.nLines) La = map.nLines - 1;
                const i64 Ga = sa.line0 + La;
                const i64 Gb = (La + 1 < map.nLines && Ga + 1 < sa.nplane) ? Ga + 1 : Ga;
                ea = sa.cy[Ga % sa.ny] + sa.cx[Ga / sa.ny];
                eb = sa.cy[Gb % sa.ny] + sa.cx[Gb / sa.ny];
            };
            const int lh = lg - 1;
            const int total = 1 << (lrw + lh);
            for (int b = lane; b < total; b += 64) {
                int rr, i;
                at.split(b, lh, rr, i);
                double ea, eb;
                eigen(rr, ea, eb);
                const int k = i + 1, m = n - k;                   // k = 1 .. n/2
                tsolve_pair(at(rr, k), at(rr, m), k, m, ww, sa.ct, ea, eb, sa.kscale);
            }
            if (lane < (1 << lrw)) {
                double ea, eb;
                eigen(lane, ea, eb);
                at(lane, 0) = tsolve_dc(at(lane, 0), ww[0].x, ea, eb, sa.ct[0], sa.kscale);
            }
            wave_lds_sync();
            fft_rows<false>(rows, lrw, lg, rowStride, team, tw);
        }
    }
    __syncthreads();
    // ---- cooperative store ----
    if (VEC) {
        // (the pair's address is formed again, not kept in registers across the transform)
        strided_store_vec<MODE, DCT_THREADS>(dst, map, lds, lg, lp, PairOfLines(map, lp, L0, tid), tid, ww);
    } else {
        const int l = tid & (2 * npairs - 1);
        const i64 L = L0 + l;
        if (L < map.nLines) {
            const i64 lb = map.base(L);
            const double2 *rr = lds + (l >> 1) * rowStride;
            for (int k = tid >> (lp + 1); k < n; k += DCT_THREADS >> (lp + 1)) {
                double2 v;
                if (MODE == 0) v = dct_post(rr, k, n, lg, ww);
                else v = rr[padi(bitrev(makhoul(k, n), lg))];
                dst[lb + (i64)k * map.es] = (l & 1) ? v.y : v.x;
            }
        }
    }
}

template <int MODE /*0 fwd, 1 inv*/, int T>
__global__ void __launch_bounds__(T, 4) k_dct_strided_wg(const double *__restrict__ src,
                                                                       double *__restrict__ dst, LineMap map, int lg,
                                                                       int lp, const double2 *__restrict__ tw,
                                                                       const double2 *__restrict__ ww) {
    extern __shared__ double2 lds[];
    const int rowStride = row_stride(1 << lg);
    const int tid = threadIdx.x;
    const BlockTeam<T> team{tid};
    const i64 L0 = xcd_tile(blockIdx.x, gridDim.x) << (lp + 1);
    const PairOfLines pl(map, lp, L0, tid);
    strided_load_vec<MODE, T>(src, map, lds, lg, lp, pl, tid);
    __syncthreads();
    if (MODE == 1) idct_combine(RowsLayout{lds, rowStride, lp}, lg, team, ww);
    fft_rows<false>(lds, lp, lg, rowStride, team, tw);
    strided_store_vec<MODE, T>(dst, map, lds, lg, lp, pl, tid, ww);
}

}  // namespace dotsocp

#include "dct_pow2_pipe.h"

namespace dotsocp {

#define DCT_LDS_BUDGET (72 * 1024)

// log2 of the complex rows (pairs of lines) a workgroup stages: as many as fit the LDS budget
// with `nbuf` buffers, a power of two, at most 32 and no more than the problem has; for the
// strided axes the lines are consecutive in memory, so more rows = wider coalesced segments.
static int tile_log2_rows(int n, i64 nLines, int nbuf) {
    const size_t rowBytes = (size_t)row_stride(n) * sizeof(double2) * nbuf;
    i64 rows = (i64)(DCT_LDS_BUDGET / rowBytes);
    if (rows < 1) rows = 1;
    if (rows > 32) rows = 32;
    const i64 havePairs = (nLines + 1) / 2;
    int lp = floor_log2(rows);
    while (lp > 0 && ((i64)1 << lp) > havePairs) --lp;
    return lp;
}

int device_cus_of(int dev) {
    static int cus[64] = {0};
    if (dev < 0 || dev >= 64) return 256;
    if (cus[dev] == 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        cus[dev] = v;
    }
    return cus[dev];
}

int device_cus() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    return device_cus_of(dev);
}

static bool dct_pipe_enabled() {
    static const bool on = !(getenv("DOTSOCP_DCT_PIPE") && atoi(getenv("DOTSOCP_DCT_PIPE")) == 0);
    return on;
}

// f(std::integral_constant<int, V>()) for the V in [Lo, Hi] that equals v, or -- v < 0 -- for every V of the range.
// A runtime line length or mode becomes a kernel's template argument; launching one instance and unlocking the large
// LDS for all of them walk the same range.
template <int Lo, class F, int... I>
static void for_const_impl(int v, F &f, std::integer_sequence<int, I...>) {
    ((v < 0 || v == Lo + I ? (void)f(std::integral_constant<int, Lo + I>()) : (void)0), ...);
}
template <int Lo, int Hi, class F>
static void for_const(int v, F f) {
    for_const_impl<Lo>(v, f, std::make_integer_sequence<int, Hi - Lo + 1>());
}
#define ALL_CONST (-1)

// ---------------------------------------------------------------------------------------------
// Choice: which kernel a pass takes.  choose_strided / choose_axis0 are pure host arithmetic on the shape of the pass, the
// alignment of its arrays and the CU count; the launchers below switch on their answer and on nothing else, and
// pow2_pass_kind / pow2_tsolve_pipelined (dotsocp_dct_pass_kernel, dotsocp_tsolve_kernel) give the same answer to the tests.
// ---------------------------------------------------------------------------------------------
enum { PK_WAVE, PK_WG, PK_WG1024, PK_PIPE, PK_TSOLVE_PIPE };
struct Pow2Choice {
    int kind;           // PK_*
    bool vec;           // strided axes: one 16-byte access carries both lines of a pair
    int lp;             // log2 of the staged pairs (axis 0: of the rows of ONE wave, lrw)
    size_t lds;         // bytes of the in-LDS kernels' tile (PK_WG1024: of the doubled one)
    unsigned blocks;
    int G, nTiles;      // pipelined kernels: persistent workgroups, tiles
    size_t ldsPipe;
};

// mode 0: DCT-II, 1: DCT-III, 2: the fused t solve (ny, line0, nplane: SolveArgs)
static Pow2Choice choose_strided(int mode, int n, int lg, const LineMap &map, i64 ny, i64 line0, i64 nplane, bool aligned,
                                 int ncu) {
    Pow2Choice c{};
    // t-axis solve (two transforms per row, in place): half the rows per workgroup so that twice as many
    // workgroups are resident
    c.lp = tile_log2_rows(n, map.nLines, mode == 2 ? 2 : 1);
    c.lds = ((size_t)1 << c.lp) * row_stride(n) * sizeof(double2);
    const i64 linesPerBlock = (i64)2 << c.lp;
    c.blocks = (unsigned)((map.nLines + linesPerBlock - 1) / linesPerBlock);
    // one 16-byte access carries both lines of a pair when consecutive lines are adjacent, even-aligned doubles
    c.vec = (map.nin % 2 == 0) && (map.outerStride % 2 == 0) && (map.es % 2 == 0) && aligned;
    c.kind = PK_WAVE;
    // fused t-axis solve, pipelined: eigenvalue tables in LDS, a tile = consecutive columns of one x
    // (rows of whole layers may be pitched: map.nin = ny lines per row, rows map.outerStride apart, time nodes map.es apart)
    if (dct_pipe_enabled() && c.vec && mode == 2 && lg >= TS_LG_MIN && lg <= TS_LG_MAX &&
        ((map.outerStride == 0 && map.es == map.nin) || (map.nin == ny && line0 == 0))) {
        const i64 tileLines = ((i64)2 << TS_LG_CPLX) / n;
        const i64 nxv = ny > 0 ? nplane / ny : 0;
        c.ldsPipe = tsolve_lds(lg, ny).bytes;
        c.G = ncu * (c.ldsPipe <= DCT_LDS_MAX / 2 ? 2 : 1);     // two workgroups per CU when they fit
        if (tileLines >= 2 && ny % tileLines == 0 && line0 % tileLines == 0 && map.nLines % tileLines == 0 &&
            nxv * ny == nplane && c.ldsPipe <= DCT_LDS_MAX && map.nLines / tileLines >= 2 * (i64)c.G &&
            map.nLines / tileLines < (1ll << 30)) {
            c.nTiles = (int)(map.nLines / tileLines);
            c.kind = PK_TSOLVE_PIPE;
            return c;
        }
    }
    // pipelined persistent kernel (see k_dct_axis0_pipe): whole tiles of 4096 complex values, the chip filled twice over
    if (dct_pipe_enabled() && c.vec && mode != 2 && lg >= PIPE_LG_MIN && lg <= PIPE_LG_MAX) {
        const i64 tileLines = ((i64)2 << PIPE_LG_CPLX) / n;
        c.G = ncu & ~31;
        if (map.nin % tileLines == 0 && map.nLines % tileLines == 0 && c.G >= 32 && map.nLines / tileLines >= 2 * (i64)c.G &&
            map.nLines / tileLines < (1ll << 30)) {
            c.nTiles = (int)(map.nLines / tileLines);
            c.ldsPipe = (((size_t)2 << PIPE_LG_CPLX) + pipe_tab_count(lg).tw + pipe_tab_count(lg).ww) * sizeof(double2);
            c.kind = PK_PIPE;
            return c;
        }
    }
    if (c.vec && mode != 2 && ((i64)n << c.lp) >= 2 * DCT_WG_THREADS) {
        // long lines: one workgroup of 1024 threads with the whole LDS (twice the rows) keeps 16 waves per CU
        // like two workgroups of 512 would, and widens the contiguous segment per line to 128 bytes
        const size_t lds2 = c.lds * 2;
        if (lds2 <= DCT_LDS_MAX && lds2 > DCT_LDS_MAX / 2 && map.nLines >= ((i64)4 << c.lp)) {
            c.lp += 1;
            c.lds = lds2;
            c.blocks = (unsigned)((map.nLines + ((i64)2 << c.lp) - 1) / ((i64)2 << c.lp));
            c.kind = PK_WG1024;
            return c;
        }
        c.kind = PK_WG;
    }
    return c;
}

static int launch_strided(int mode, const Pow2Plan *p, const double *src, double *dst, const LineMap &map,
                          const SolveArgs &sa, hipStream_t st) {
    const int n = (int)p->n, lg = p->lg;
    const double2 *tw = p->tw, *ww = p->ww;
    const Pow2Choice c = choose_strided(mode, n, lg, map, sa.ny, sa.line0, sa.nplane,
                                        ((uintptr_t)src | (uintptr_t)dst) % 16 == 0, device_cus());
    if (c.kind != PK_WG1024 && c.lds > DCT_LDS_MAX) {
        set_error("power-of-two DCT length %d does not fit the LDS in one pass (largest supported there: 8192)", n);
        return DOTSOCP_EINVAL;
    }
    switch (c.kind) {
        case PK_TSOLVE_PIPE: {
            static unsigned long long done_tp = 0;
            if (DeviceOnce once_(done_tp); once_)
                for_const<TS_LG_MIN, TS_LG_MAX>(ALL_CONST, [](auto k) { allow_big_lds(k_dct_tsolve_pipe<decltype(k)::value>); });
            for_const<TS_LG_MIN, TS_LG_MAX>(lg, [&](auto k) {
                DS_KLAUNCH((k_dct_tsolve_pipe<decltype(k)::value>), dim3((unsigned)c.G), dim3(TS_THREADS), c.ldsPipe, st, src, dst,
                           map, c.nTiles, sa, tw, ww);
            });
            break;
        }
        case PK_PIPE: {
            static unsigned long long done_sp = 0;
            if (DeviceOnce once_(done_sp); once_)
                for_const<PIPE_LG_MIN, PIPE_LG_MAX>(ALL_CONST, [](auto k) {
                    allow_big_lds(k_dct_strided_pipe<0, decltype(k)::value>);
                    allow_big_lds(k_dct_strided_pipe<1, decltype(k)::value>);
                });
            for_const<PIPE_LG_MIN, PIPE_LG_MAX>(lg, [&](auto k) {
                for_const<0, 1>(mode, [&](auto m) {
                    DS_KLAUNCH((k_dct_strided_pipe<decltype(m)::value, decltype(k)::value>), dim3((unsigned)c.G),
                               dim3(PIPE_THREADS), c.ldsPipe, st, src, dst, map, c.nTiles, tw, ww);
                });
            });
            break;
        }
        case PK_WG1024:
        case PK_WG: {
            static unsigned long long done_wg = 0;
            if (DeviceOnce once_(done_wg); once_)
                for_const<0, 1>(ALL_CONST, [](auto m) {
                    allow_big_lds(k_dct_strided_wg<decltype(m)::value, 512>);
                    allow_big_lds(k_dct_strided_wg<decltype(m)::value, 1024>);
                });
            for_const<0, 1>(mode, [&](auto m) {
                if (c.kind == PK_WG1024)
                    DS_KLAUNCH((k_dct_strided_wg<decltype(m)::value, 1024>), dim3(c.blocks), dim3(1024), c.lds, st, src, dst, map,
                               lg, c.lp, tw, ww);
                else
                    DS_KLAUNCH((k_dct_strided_wg<decltype(m)::value, 512>), dim3(c.blocks), dim3(DCT_WG_THREADS), c.lds, st, src,
                               dst, map, lg, c.lp, tw, ww);
            });
            break;
        }
        default: {
            static unsigned long long done = 0;
            if (DeviceOnce once_(done); once_)
                for_const<0, 2>(ALL_CONST, [](auto m) {
                    allow_big_lds(k_dct_strided<decltype(m)::value, true>);
                    allow_big_lds(k_dct_strided<decltype(m)::value, false>);
                });
            for_const<0, 2>(mode, [&](auto m) {
                if (c.vec)
                    DS_KLAUNCH((k_dct_strided<decltype(m)::value, true>), dim3(c.blocks), dim3(DCT_THREADS), c.lds, st, src, dst,
                               map, lg, c.lp, sa, tw, ww);
                else
                    DS_KLAUNCH((k_dct_strided<decltype(m)::value, false>), dim3(c.blocks), dim3(DCT_THREADS), c.lds, st, src, dst,
                               map, lg, c.lp, sa, tw, ww);
            });
        }
    }
    DS_HIP(hipGetLastError());
    return 0;
}

// lines of this length along this axis (0: y; else x / t) leave the LDS: the two-level transform (dct_long.hip)
static bool pow2_two_level(i64 n, int axis) { return n >= dct_long_min(axis == 0 ? 0 : 1); }

// line map of the fused t solve over the columns line0 .. line0 + nl - 1 (pow2_launch_tsolve)
static LineMap tsolve_map(i64 ny, i64 nplane, i64 nl, i64 pitch0) {
    LineMap map;
    map.nin = nl;
    map.outerStride = 0;
    map.nLines = nl;
    map.es = nl;
    if (pitch0 > ny) {      // whole layers with pitched rows: line L = (y, x) = (L % ny, L / ny) starts at y + pitch0 * x
        map.nin = ny;
        map.outerStride = pitch0;
        map.es = pitch0 * (nplane / ny);
    }
    return map;
}

int pow2_launch_strided(const Pow2Plan *p, const double *src, double *dst, const LineMap &map, int inverse, hipStream_t st) {
    if (pow2_two_level(p->n, 1)) return long_launch(p->lng, src, dst, map, false, inverse, st);
    return launch_strided(inverse ? 1 : 0, p, src, dst, map, SolveArgs{}, st);
}

int pow2_launch_tsolve(const Pow2Plan *p, const double *src, double *dst, i64 ny, i64 nplane, i64 line0, i64 nl,
                       double kscale, const double *cy, const double *cx, const double *ct, hipStream_t st, i64 pitch0) {
    const LineMap map = tsolve_map(ny, nplane, nl, pitch0);
    if (map.nLines <= 0) return 0;
    SolveArgs sa{ny, line0, nplane, kscale, cy, cx, ct};
    return launch_strided(2, p, src, dst, map, sa, st);
}

// axis 0: PK_WAVE, PK_WG or PK_PIPE; lp = lrw, the log2 of the rows of one wave
static Pow2Choice choose_axis0(i64 n, int lg, const LineMap &map, bool aligned, int ncu) {
    Pow2Choice c{};
    // each wave owns 2^lrw rows; a workgroup of 4 waves stages 4 * 2^lrw rows
    const int lp = tile_log2_rows((int)n, map.nLines, 1);
    const int lrw = lp >= 2 ? lp - 2 : 0;
    c.vec = aligned;
    c.lp = lrw;
    c.lds = ((size_t)DCT_WAVES << lrw) * row_stride((int)n) * sizeof(double2);
    const i64 linesPerBlock = (i64)(2 * DCT_WAVES) << lrw;
    c.blocks = (unsigned)((map.nLines + linesPerBlock - 1) / linesPerBlock);
    c.kind = PK_WAVE;
    // pipelined persistent kernel: whole tiles of 8192 doubles, enough of them to fill the chip twice
    const i64 tileLines = ((i64)2 << PIPE_LG_CPLX) / n;
    if (dct_pipe_enabled() && lg >= PIPE_LG_MIN && lg <= PIPE_LG_MAX && map.nLines % tileLines == 0 && aligned) {
        const i64 nTiles = map.nLines / tileLines;
        if (nTiles >= 2 * (i64)ncu && nTiles < (1ll << 30)) {
            c.ldsPipe = (2 * (size_t)axis0_pipe_buf(lg) + pipe_tab_count(lg).tw + pipe_tab_count(lg).ww) * sizeof(double2);
            c.G = ncu;
            c.nTiles = (int)nTiles;
            c.kind = PK_PIPE;
            return c;
        }
    }
    if (((n / 2) << lp) >= 2 * DCT_WG_THREADS) {
        // same rows per workgroup (4 << lrw complex rows), twice the threads, shared by all of them
        const int lrows = lrw + 2;
        c.blocks = (unsigned)((((map.nLines + 1) / 2) + ((i64)1 << lrows) - 1) >> lrows);
        c.kind = PK_WG;
    }
    return c;
}

int pow2_launch_axis0(const Pow2Plan *p, const double *src, double *dst, const LineMap &map, int inverse, hipStream_t st) {
    if (pow2_two_level(p->n, 0)) return long_launch(p->lng, src, dst, map, true, inverse, st);
    const i64 n = p->n;
    const int lg = p->lg;
    const double2 *tw = p->tw, *ww = p->ww;
    const Pow2Choice c = choose_axis0(n, lg, map, ((uintptr_t)src | (uintptr_t)dst) % 16 == 0, device_cus());
    if (c.lds > DCT_LDS_MAX) {
        set_error("power-of-two DCT length %lld does not fit the LDS (largest supported: 2048 along y, 8192 along x / t)",
                  (long long)n);
        return DOTSOCP_EINVAL;
    }
    static unsigned long long done = 0;
    if (DeviceOnce once_(done); once_)
        for_const<0, 1>(ALL_CONST, [](auto i) {
            allow_big_lds(k_dct_axis0<decltype(i)::value != 0>);
            allow_big_lds(k_dct_axis0_wg<decltype(i)::value != 0>);
        });
    switch (c.kind) {
        case PK_PIPE: {
            static unsigned long long done_pipe = 0;
            if (DeviceOnce once_(done_pipe); once_)
                for_const<PIPE_LG_MIN, PIPE_LG_MAX>(ALL_CONST, [](auto k) {
                    allow_big_lds(k_dct_axis0_pipe<false, decltype(k)::value>);
                    allow_big_lds(k_dct_axis0_pipe<true, decltype(k)::value>);
                });
            for_const<PIPE_LG_MIN, PIPE_LG_MAX>(lg, [&](auto k) {
                for_const<0, 1>(inverse ? 1 : 0, [&](auto i) {
                    DS_KLAUNCH((k_dct_axis0_pipe<decltype(i)::value != 0, decltype(k)::value>), dim3((unsigned)c.G),
                               dim3(PIPE_THREADS), c.ldsPipe, st, src, dst, c.nTiles, map.outerStride, tw, ww);
                });
            });
            break;
        }
        case PK_WG:
            for_const<0, 1>(inverse ? 1 : 0, [&](auto i) {
                DS_KLAUNCH(k_dct_axis0_wg<decltype(i)::value != 0>, dim3(c.blocks), dim3(DCT_WG_THREADS), c.lds, st, src, dst,
                           map.nLines, map.outerStride, lg, c.lp + 2, tw, ww);
            });
            break;
        default:
            for_const<0, 1>(inverse ? 1 : 0, [&](auto i) {
                DS_KLAUNCH(k_dct_axis0<decltype(i)::value != 0>, dim3(c.blocks), dim3(DCT_THREADS), c.lds, st, src, dst,
                           map.nLines, map.outerStride, lg, c.lp, tw, ww);
            });
    }
    DS_HIP(hipGetLastError());
    return 0;
}

static int pass_kind_of(int pk) {
    return pk == PK_WAVE ? DOTSOCP_PASS_POW2_WAVE : (pk == PK_PIPE ? DOTSOCP_PASS_POW2_PIPE : DOTSOCP_PASS_POW2_WG);
}

int pow2_pass_kind(i64 n, const LineMap &map, bool axis0, int ncu) {
    if (pow2_two_level(n, axis0 ? 0 : 1)) return DOTSOCP_PASS_POW2_LONG;
    const int lg = ceil_log2(n);
    if (axis0) return pass_kind_of(choose_axis0(n, lg, map, true, ncu).kind);
    return pass_kind_of(choose_strided(0, (int)n, lg, map, 0, 0, 0, true, ncu).kind);
}

bool pow2_tsolve_pipelined(i64 n, i64 ny, i64 nplane, i64 line0, i64 nl, i64 pitch0, int ncu) {
    const LineMap map = tsolve_map(ny, nplane, nl, pitch0);
    return map.nLines > 0 && choose_strided(2, (int)n, ceil_log2(n), map, ny, line0, nplane, true, ncu).kind == PK_TSOLVE_PIPE;
}

}  // namespace dotsocp
