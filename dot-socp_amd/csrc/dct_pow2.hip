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
    p->lg = 0;
    while (((i64)1 << p->lg) < n) ++p->lg;
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

#define DCT_WAVES 4
#define DCT_BATCH 8   // global loads in flight per lane before the first dependent LDS write
// Twiddle tables as the kernels see them: a plain pointer, or -- for the 2048-point lines of the pipelined kernels, whose
// two tile buffers leave 32 KB of LDS for tables -- the symmetric part only:
//   exp(-2 pi i (j + n/4) / n) = -i exp(-2 pi i j / n)               -> a quarter of the FFT twiddles,
//   ww[n - k] = (-imag ww[k], -real ww[k])   (0 < k < n/2)           -> half of the DCT weights (+ the entry n/2).
struct TwQuarter {
    const double2 *t;
    int q;                  // n / 4 entries
    __device__ __forceinline__ double2 operator[](int j) const {
        const double2 v = t[j & (q - 1)];
        return (j & q) ? make_double2(v.y, -v.x) : v;
    }
};
struct WwHalf {
    const double2 *t;
    int h;                  // n / 2: entries 0 .. h
    __device__ __forceinline__ double2 operator[](int m) const {
        const double2 v = t[m <= h ? m : 2 * h - m];
        return (m <= h) ? v : make_double2(-v.y, -v.x);
    }
};

// LDS position of input element k while staging a line: forward transforms take the Makhoul order, the inverse
// the natural one, the fused t-axis solve the bit-reversed Makhoul order (its forward FFT is decimation-in-time)
template <int MODE>
__device__ __forceinline__ int stage_pos(int k, int n, int lg) {
    return MODE == 1 ? k : (MODE == 2 ? bitrev(makhoul(k, n), lg) : makhoul(k, n));
}

// Inverse pre-processing on the calling wave's rows (natural order, Xa + i Xb elementwise):
//   G[k] = (ww[k] X[k] + conj(ww[n-k]) X[n-k]) / 2, so that fft(G) = real(fft(ww .* X))
//   (mirt_idctn.m:109,119-120).  k and n-k are handled by the same lane.
__device__ __forceinline__ void idct_combine_wave(double2 *rows, int lrw, int lg, int rowStride, int lane,
                                                  const double2 *__restrict__ ww) {
    const int n = 1 << lg, lh = lg - 1;
    const int total = 1 << (lrw + lh);
    for (int b = lane; b < total; b += 64) {
        double2 *r = rows + (b >> lh) * rowStride;
        const int k = (b & ((1 << lh) - 1)) + 1;          // 1 .. n/2
        const int m = n - k;
        const double2 xk = r[padi(k)], xm = r[padi(m)];
        const double2 wk = ww[k], wm = ww[m];
        const double gar = 0.5 * (wk.x * xk.x + wm.x * xm.x), gai = 0.5 * (wk.y * xk.x - wm.y * xm.x);
        const double gbr = 0.5 * (wk.x * xk.y + wm.x * xm.y), gbi = 0.5 * (wk.y * xk.y - wm.y * xm.y);
        r[padi(k)] = make_double2(gar - gbi, gai + gbr);
        if (m != k) {
            const double har = 0.5 * (wm.x * xm.x + wk.x * xk.x), hai = 0.5 * (wm.y * xm.x - wk.y * xk.x);
            const double hbr = 0.5 * (wm.x * xm.y + wk.x * xk.y), hbi = 0.5 * (wm.y * xm.y - wk.y * xk.y);
            r[padi(m)] = make_double2(har - hbi, hai + hbr);
        }
    }
    if (lane < (1 << lrw)) {
        double2 *r = rows + lane * rowStride;
        const double w0 = ww[0].x;
        r[0] = make_double2(w0 * r[0].x, w0 * r[0].y);
    }
    wave_lds_sync();
}

// (Xa[k], Xb[k]) = real(ww[k] * V_{a,b}[k]) from the bit-reversed FFT of va + i vb:
// V_a = (V[k] + conj(V[n-k])) / 2, V_b = (V[k] - conj(V[n-k])) / (2i)   (mirt_dctn.m:130)
template <int LES = 0, class WW = const double2 *>
__device__ __forceinline__ double2 dct_post(const double2 *__restrict__ r, int k, int n, int lg, WW ww) {
    const double2 vk = r[padi(bitrev(k, lg)) << LES];
    const double2 vm = r[padi(bitrev((n - k) & (n - 1), lg)) << LES];
    const double2 w = ww[k];
    const double ar = 0.5 * (vk.x + vm.x), ai = 0.5 * (vk.y - vm.y);
    const double br = 0.5 * (vk.y + vm.y), bi = -0.5 * (vk.x - vm.x);
    return make_double2(w.x * ar - w.y * ai, w.x * br - w.y * bi);
}

// ---------------------------------------------------------------------------------------------
// Axis 0 (lines contiguous in memory): every wave works alone on its own 2^lrw complex rows
// (pairs of consecutive lines) -- 16-byte global accesses, no workgroup barrier at all.
// ---------------------------------------------------------------------------------------------
template <bool INVERSE>
__global__ void __launch_bounds__(DCT_THREADS) k_dct_axis0(const double *__restrict__ src, double *__restrict__ dst,
                                                            i64 nLines, i64 ls /* doubles between lines */, int lg, int lrw,
                                                            const double2 *__restrict__ tw,
                                                            const double2 *__restrict__ ww) {
    extern __shared__ double2 lds[];
    const int n = 1 << lg, lh = lg - 1;
    const int rowStride = row_stride(n);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int rw = 1 << lrw;
    double2 *rows = lds + (wave << lrw) * rowStride;
    const i64 pair0 = ((i64)blockIdx.x * DCT_WAVES + wave) << lrw;      // first pair of lines of this wave
    const int total = 1 << (lrw + lh);                                    // (row, j) with j = k / 2
    // ---- load: two consecutive elements of both lines per lane; DCT_BATCH iterations' worth of
    // 16-byte global loads are issued before the first LDS write so that their latencies overlap ----
    for (int b0 = lane; b0 < total; b0 += 64 * DCT_BATCH) {
        double2 A[DCT_BATCH], B[DCT_BATCH];
#pragma unroll
        for (int u = 0; u < DCT_BATCH; ++u) {
            const int b = b0 + 64 * u;
            const int rr = b >> lh, j = b & ((1 << lh) - 1);
            const i64 La = 2 * (pair0 + rr);
            A[u] = make_double2(0.0, 0.0);
            B[u] = A[u];
            if (b < total && La < nLines) A[u] = *(const double2 *)(src + La * ls + 2 * j);
            if (b < total && La + 1 < nLines) B[u] = *(const double2 *)(src + (La + 1) * ls + 2 * j);
        }
#pragma unroll
        for (int u = 0; u < DCT_BATCH; ++u) {
            const int b = b0 + 64 * u;
            if (b >= total) break;
            const int rr = b >> lh, j = b & ((1 << lh) - 1);
            double2 *r = rows + rr * rowStride;
            if (!INVERSE) {
                r[padi(j)] = make_double2(A[u].x, B[u].x);               // x[2j]   -> v[j]
                r[padi(n - 1 - j)] = make_double2(A[u].y, B[u].y);       // x[2j+1] -> v[n-1-j]
            } else {
                r[padi(2 * j)] = make_double2(A[u].x, B[u].x);
                r[padi(2 * j + 1)] = make_double2(A[u].y, B[u].y);
            }
        }
    }
    wave_lds_sync();
    if (INVERSE) idct_combine_wave(rows, lrw, lg, rowStride, lane, ww);
    fft_rows_wave(rows, lrw, lg, rowStride, lane, tw);
    // ---- store ----
    for (int b = lane; b < total; b += 64) {
        const int rr = b >> lh, j = b & ((1 << lh) - 1);
        const i64 La = 2 * (pair0 + rr);
        const double2 *r = rows + rr * rowStride;
        double2 A, B;
        if (!INVERSE) {
            const double2 p0 = dct_post(r, 2 * j, n, lg, ww), p1 = dct_post(r, 2 * j + 1, n, lg, ww);
            A = make_double2(p0.x, p1.x);
            B = make_double2(p0.y, p1.y);
        } else {
            const double2 v0 = r[padi(bitrev(j, lg))], v1 = r[padi(bitrev(n - 1 - j, lg))];
            A = make_double2(v0.x, v1.x);                      // x[2j] = v[j], x[2j+1] = v[n-1-j]
            B = make_double2(v0.y, v1.y);
        }
        if (La < nLines) *(double2 *)(dst + La * ls + 2 * j) = A;
        if (La + 1 < nLines) *(double2 *)(dst + (La + 1) * ls + 2 * j) = B;
    }
    (void)rw;
}

// ---------------------------------------------------------------------------------------------
// Strided axes (x, t): the workgroup stages 2^lp complex rows = 2^(lp+1) lines that are
// CONSECUTIVE in memory, loads / stores them cooperatively (VEC: one 16-byte access carries both
// lines of a pair), and every wave runs the FFT of its own rows between the two barriers.
// TSOLVE: forward DCT, division by the spectral kernel, inverse DCT in one pass (t axis).
// ---------------------------------------------------------------------------------------------
struct SolveArgs {
    i64 ny, line0, nplane; // TSOLVE: local line L is column (y, x) = (G % ny, G / ny), G = line0 + L, of ny*nx = nplane columns
    double kscale;
    const double *cy, *cx, *ct;
};

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
    // ---- cooperative load ----
    if (VEC) {
        const int r = tid & (npairs - 1);
        const i64 L = L0 + 2 * r;
        const bool ok = L < map.nLines;
        const i64 lb = ok ? map.base(L) : 0;
        const int kstep = DCT_THREADS >> lp;
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
        if (MODE == 1) idct_combine_wave(rows, lrw, lg, rowStride, lane, ww);
        if (MODE != 2) {
            fft_rows_wave(rows, lrw, lg, rowStride, lane, tw);
        } else {
            // forward transform with natural-order output, then -- in place, the lane that owns k also owns n-k --
            // X = DCT post-processing (dct_post), Y = X / (kscale * lambda), G = inverse pre-processing
            // (idct_combine_wave) in one go, then the inverse transform on the same rows
            fft_rows_wave_dit(rows, lrw, lg, rowStride, lane, tw);
            const int lh = lg - 1;
            const int total = 1 << (lrw + lh);
            for (int b = lane; b < total; b += 64) {
                const int rr = b >> lh;
                double2 *r = rows + rr * rowStride;
                // (an odd line count leaves the last pair with line a alone: it keeps ITS eigenvalue, line b's is unused)
                i64 La = L0 + 2 * ((wave << lrw) + rr);
                if (La >= map.nLines) La = map.nLines - 1;
                const i64 Ga = sa.line0 + La;
                const i64 Gb = (La + 1 < map.nLines && Ga + 1 < sa.nplane) ? Ga + 1 : Ga;
                const double ea = sa.cy[Ga % sa.ny] + sa.cx[Ga / sa.ny];                    // CY + CX of line a
                const double eb = sa.cy[Gb % sa.ny] + sa.cx[Gb / sa.ny];
                const int k = (b & ((1 << lh) - 1)) + 1;          // 1 .. n/2
                const int m = n - k;
                const double2 vk = r[padi(k)], vm = r[padi(m)];
                const double2 wk = ww[k], wm = ww[m];
                const double ar = 0.5 * (vk.x + vm.x), ai = 0.5 * (vk.y - vm.y);
                const double br = 0.5 * (vk.y + vm.y), bi = -0.5 * (vk.x - vm.x);
                const double ctk = sa.ct[k], ctm = sa.ct[m];
                double lak = ea + ctk, lbk = eb + ctk, lam = ea + ctm, lbm = eb + ctm;
                if (lak == 0.0) lak = 1.0;
                if (lbk == 0.0) lbk = 1.0;
                if (lam == 0.0) lam = 1.0;
                if (lbm == 0.0) lbm = 1.0;
                // Y[k], Y[n-k]: .x = line a, .y = line b
                const double2 xk = make_double2((wk.x * ar - wk.y * ai) / (sa.kscale * lak),
                                                (wk.x * br - wk.y * bi) / (sa.kscale * lbk));
                const double2 xm = make_double2((wm.x * ar + wm.y * ai) / (sa.kscale * lam),
                                                (wm.x * br + wm.y * bi) / (sa.kscale * lbm));
                const double gar = 0.5 * (wk.x * xk.x + wm.x * xm.x), gai = 0.5 * (wk.y * xk.x - wm.y * xm.x);
                const double gbr = 0.5 * (wk.x * xk.y + wm.x * xm.y), gbi = 0.5 * (wk.y * xk.y - wm.y * xm.y);
                r[padi(k)] = make_double2(gar - gbi, gai + gbr);
                if (m != k) {
                    const double har = 0.5 * (wm.x * xm.x + wk.x * xk.x), hai = 0.5 * (wm.y * xm.x - wk.y * xk.x);
                    const double hbr = 0.5 * (wm.x * xm.y + wk.x * xk.y), hbi = 0.5 * (wm.y * xm.y - wk.y * xk.y);
                    r[padi(m)] = make_double2(har - hbi, hai + hbr);
                }
            }
            if (lane < (1 << lrw)) {                               // k = 0: V[0] is its own partner
                double2 *r = rows + lane * rowStride;
                i64 La = L0 + 2 * ((wave << lrw) + lane);
                if (La >= map.nLines) La = map.nLines - 1;
                const i64 Ga = sa.line0 + La;
                const i64 Gb = (La + 1 < map.nLines && Ga + 1 < sa.nplane) ? Ga + 1 : Ga;
                double la = (sa.cy[Ga % sa.ny] + sa.cx[Ga / sa.ny]) + sa.ct[0];
                double lb2 = (sa.cy[Gb % sa.ny] + sa.cx[Gb / sa.ny]) + sa.ct[0];
                if (la == 0.0) la = 1.0;
                if (lb2 == 0.0) lb2 = 1.0;
                const double w0 = ww[0].x;
                const double2 v0 = r[0];
                r[0] = make_double2(w0 * ((w0 * v0.x) / (sa.kscale * la)), w0 * ((w0 * v0.y) / (sa.kscale * lb2)));
            }
            wave_lds_sync();
            fft_rows_wave(rows, lrw, lg, rowStride, lane, tw);
        }
    }
    __syncthreads();
    // ---- cooperative store ----
    const double2 *out = lds;
    if (VEC) {
        const int r = tid & (npairs - 1);
        const i64 L = L0 + 2 * r;
        if (L < map.nLines) {
            const i64 lb = map.base(L);
            const double2 *rr = out + r * rowStride;
            for (int k = tid >> lp; k < n; k += DCT_THREADS >> lp) {
                double2 v;
                if (MODE == 0) v = dct_post(rr, k, n, lg, ww);
                else v = rr[padi(bitrev(makhoul(k, n), lg))];
                *(double2 *)(dst + lb + (i64)k * map.es) = v;
            }
        }
    } else {
        const int l = tid & (2 * npairs - 1);
        const i64 L = L0 + l;
        if (L < map.nLines) {
            const i64 lb = map.base(L);
            const double2 *rr = out + (l >> 1) * rowStride;
            for (int k = tid >> (lp + 1); k < n; k += DCT_THREADS >> (lp + 1)) {
                double2 v;
                if (MODE == 0) v = dct_post(rr, k, n, lg, ww);
                else v = rr[padi(bitrev(makhoul(k, n), lg))];
                dst[lb + (i64)k * map.es] = (l & 1) ? v.y : v.x;
            }
        }
    }
}


// ---------------------------------------------------------------------------------------------
// Workgroup-wide flavour: ALL threads of the workgroup share ALL staged rows (butterfly groups are
// dealt round-robin to the T threads, __syncthreads() between register groups).  Twice the waves per
// staged row of the per-wave flavour above at the same LDS footprint -- the footprint, not registers,
// caps the resident workgroups per CU, so this doubles the waves that overlap VALU, LDS and HBM phases.
// ---------------------------------------------------------------------------------------------
template <bool RAWB = false, class WW = const double2 *>
__device__ __forceinline__ void idct_combine_wg(double2 *rows, int lrows, int lg, int rowStride, int t, int T, WW ww) {
    const int n = 1 << lg, lh = lg - 1;
    const int total = 1 << (lrows + lh);
    for (int b = t; b < total; b += T) {
        double2 *r = rows + (b >> lh) * rowStride;
        const int k = (b & ((1 << lh) - 1)) + 1;          // 1 .. n/2
        const int m = n - k;
        const double2 xk = r[padi(k)], xm = r[padi(m)];
        const double2 wk = ww[k], wm = ww[m];
        const double gar = 0.5 * (wk.x * xk.x + wm.x * xm.x), gai = 0.5 * (wk.y * xk.x - wm.y * xm.x);
        const double gbr = 0.5 * (wk.x * xk.y + wm.x * xm.y), gbi = 0.5 * (wk.y * xk.y - wm.y * xm.y);
        r[padi(k)] = make_double2(gar - gbi, gai + gbr);
        if (m != k) {
            const double har = 0.5 * (wm.x * xm.x + wk.x * xk.x), hai = 0.5 * (wm.y * xm.x - wk.y * xk.x);
            const double hbr = 0.5 * (wm.x * xm.y + wk.x * xk.y), hbi = 0.5 * (wm.y * xm.y - wk.y * xk.y);
            r[padi(m)] = make_double2(har - hbi, hai + hbr);
        }
    }
    if (t < (1 << lrows)) {
        double2 *r = rows + t * rowStride;
        const double w0 = ww[0].x;
        r[0] = make_double2(w0 * r[0].x, w0 * r[0].y);
    }
    if (RAWB) lds_barrier(); else __syncthreads();
}

#define DCT_WG_THREADS 512
// Axis 0, workgroup-wide: the workgroup stages 2^lrows complex rows (pairs of consecutive lines).
template <bool INVERSE>
__global__ void __launch_bounds__(DCT_WG_THREADS, 4) k_dct_axis0_wg(const double *__restrict__ src,
                                                                     double *__restrict__ dst, i64 nLines, i64 ls, int lg,
                                                                     int lrows, const double2 *__restrict__ tw,
                                                                     const double2 *__restrict__ ww) {
    extern __shared__ double2 lds[];
    const int n = 1 << lg, lh = lg - 1;
    const int rowStride = row_stride(n);
    const int tid = threadIdx.x;
    const i64 pair0 = (i64)blockIdx.x << lrows;
    const int total = 1 << (lrows + lh);
    for (int b0 = tid; b0 < total; b0 += DCT_WG_THREADS * DCT_BATCH) {
        double2 A[DCT_BATCH], B[DCT_BATCH];
#pragma unroll
        for (int u = 0; u < DCT_BATCH; ++u) {
            const int b = b0 + DCT_WG_THREADS * u;
            const int rr = b >> lh, j = b & ((1 << lh) - 1);
            const i64 La = 2 * (pair0 + rr);
            A[u] = make_double2(0.0, 0.0);
            B[u] = A[u];
            if (b < total && La < nLines) A[u] = *(const double2 *)(src + La * ls + 2 * j);
            if (b < total && La + 1 < nLines) B[u] = *(const double2 *)(src + (La + 1) * ls + 2 * j);
        }
#pragma unroll
        for (int u = 0; u < DCT_BATCH; ++u) {
            const int b = b0 + DCT_WG_THREADS * u;
            if (b >= total) break;
            const int rr = b >> lh, j = b & ((1 << lh) - 1);
            double2 *r = lds + rr * rowStride;
            if (!INVERSE) {
                r[padi(j)] = make_double2(A[u].x, B[u].x);
                r[padi(n - 1 - j)] = make_double2(A[u].y, B[u].y);
            } else {
                r[padi(2 * j)] = make_double2(A[u].x, B[u].x);
                r[padi(2 * j + 1)] = make_double2(A[u].y, B[u].y);
            }
        }
    }
    __syncthreads();
    if (INVERSE) idct_combine_wg(lds, lrows, lg, rowStride, tid, DCT_WG_THREADS, ww);
    fft_rows_wg(lds, lrows, lg, rowStride, tid, DCT_WG_THREADS, tw);
    for (int b = tid; b < total; b += DCT_WG_THREADS) {
        const int rr = b >> lh, j = b & ((1 << lh) - 1);
        const i64 La = 2 * (pair0 + rr);
        const double2 *r = lds + rr * rowStride;
        double2 A, B;
        if (!INVERSE) {
            const double2 p0 = dct_post(r, 2 * j, n, lg, ww), p1 = dct_post(r, 2 * j + 1, n, lg, ww);
            A = make_double2(p0.x, p1.x);
            B = make_double2(p0.y, p1.y);
        } else {
            const double2 v0 = r[padi(bitrev(j, lg))], v1 = r[padi(bitrev(n - 1 - j, lg))];
            A = make_double2(v0.x, v1.x);
            B = make_double2(v0.y, v1.y);
        }
        if (La < nLines) *(double2 *)(dst + La * ls + 2 * j) = A;
        if (La + 1 < nLines) *(double2 *)(dst + (La + 1) * ls + 2 * j) = B;
    }
}

// ---------------------------------------------------------------------------------------------
// Pipelined flavour (axis 0, n = 128 .. 2048).  What limits the kernels above is not a unit but the bytes in flight:
// while a workgroup computes, its tile sits in LDS and nothing of it travels, and the LDS holds two tiles only (the
// same kernels with the transform skipped run at the copy rate; the transform's time adds in full).  Here ONE
// persistent workgroup of 512 threads per CU (two waves per SIMD, 256 registers each) walks tiles of 8192 doubles
// (whole lines, contiguous in memory) through two LDS buffers, and the lines of a tile arrive by LDS-DMA
// (global_load_lds_dwordx4: no registers, so the loads of tile k+1 and k+2 are in flight during the transform and the
// stores of tile k).  Per tile:
//   raw lines -> paired rows in Makhoul / natural order, in place (all reads, barrier, all writes) | [inverse
//   pre-processing] | FFT | post-processing + stores | wait for the DMA of tile k+1 (counted: only the stores just
//   issued are younger and stay in flight) | barrier | DMA of tile k+2 into the buffer just drained.
// The twiddle tables live in LDS too: an ordinary global load in the loop would make the compiler wait for
// everything in flight.  LDS: 2 x 4 x (n + 1) x 16 B + 1.5 n x 16 B = 152 KB at n = 1024.
// ---------------------------------------------------------------------------------------------
#define PIPE_THREADS 512
#define PIPE_IT ((1 << (PIPE_LG_CPLX - 1)) / PIPE_THREADS)   // (row, j) items per thread
#define PIPE_LG_CPLX 12   // complex elements per tile: 4096 = 8192 doubles = 64 KB of lines
#define PIPE_NS 8         // global store instructions per wave and tile
#define PIPE_ND 8         // LDS-DMA instructions per wave and tile (64 pieces of 1 KB over 8 waves)

// A double from a wave-uniform global address through the scalar cache: no vector-memory operation, so nothing the
// counted waits of the pipelined kernels would have to account for (the compiler takes a vector load for such a read
// when it cannot prove that the kernel's stores leave the table alone, and then waits for everything in flight).
__device__ __forceinline__ double sload_f64(const double *p) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)p);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((uintptr_t)p >> 32));
    const double *sp = (const double *)(((uintptr_t)hi << 32) | (uintptr_t)lo);
    double v;
    asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(sp) : "memory");
    return v;
}

// the register groups of fft_rows_wg for a length known at compile time (same plan, same arithmetic)
// the same register groups on a pair-interleaved tile (dif_group<., LES>): item b = (row b % rows, group b / rows), so the
// lanes of a wave sweep the rows of one element first -- consecutive LDS addresses
template <int LG, int LROWS, int T, int ST = 0, int SL = LG, class TW = const double2 *>
__device__ __forceinline__ void fft_tile_pipe(double2 *tile, int t, TW tw) {
    constexpr int NST = (LG + 3) >> 2;
    constexpr int BASEB = LG / NST, EXTRA = LG % NST;
    if constexpr (ST < NST) {
        constexpr int LR = BASEB + (ST < EXTRA ? 1 : 0);
        constexpr int LPR = LG - LR;
        constexpr int TOTAL = 1 << (LROWS + LPR);
#pragma unroll
        for (int b = t; b < TOTAL; b += T)
            dif_group<LR, LROWS>(tile + (b & ((1 << LROWS) - 1)), SL, b >> LROWS, LG, tw);
        lds_barrier();
        fft_tile_pipe<LG, LROWS, T, ST + 1, SL - LR>(tile, t, tw);
    }
}

template <int LG, int LROWS, int T, int ST = ((LG + 3) >> 2) - 1, int SL = 0>
__device__ __forceinline__ void fft_tile_pipe_dit(double2 *tile, int t, const double2 *__restrict__ tw) {
    constexpr int NST = (LG + 3) >> 2;
    constexpr int BASEB = LG / NST, EXTRA = LG % NST;
    if constexpr (ST >= 0) {
        constexpr int LR = BASEB + (ST < EXTRA ? 1 : 0);
        constexpr int SL2 = SL + LR;
        constexpr int LPR = LG - LR;
        constexpr int TOTAL = 1 << (LROWS + LPR);
#pragma unroll
        for (int b = t; b < TOTAL; b += T)
            dit_group<LR, LROWS>(tile + (b & ((1 << LROWS) - 1)), SL2, b >> LROWS, LG, tw);
        lds_barrier();
        fft_tile_pipe_dit<LG, LROWS, T, ST - 1, SL2>(tile, t, tw);
    }
}

// inverse pre-processing (idct_combine_wg) on a pair-interleaved tile
template <int LG, int LROWS, int T, class WW = const double2 *>
__device__ __forceinline__ void idct_combine_tile(double2 *tile, int t, WW ww) {
    constexpr int n = 1 << LG, lh = LG - 1;
    constexpr int TOTAL = 1 << (LROWS + lh);
#pragma unroll
    for (int b = t; b < TOTAL; b += T) {
        double2 *r = tile + (b & ((1 << LROWS) - 1));
        const int k = (b >> LROWS) + 1;                     // 1 .. n/2
        const int m = n - k;
        const int ik = padi(k) << LROWS, im = padi(m) << LROWS;
        const double2 xk = r[ik], xm = r[im];
        const double2 wk = ww[k], wm = ww[m];
        const double gar = 0.5 * (wk.x * xk.x + wm.x * xm.x), gai = 0.5 * (wk.y * xk.x - wm.y * xm.x);
        const double gbr = 0.5 * (wk.x * xk.y + wm.x * xm.y), gbi = 0.5 * (wk.y * xk.y - wm.y * xm.y);
        r[ik] = make_double2(gar - gbi, gai + gbr);
        if (m != k) {
            const double har = 0.5 * (wm.x * xm.x + wk.x * xk.x), hai = 0.5 * (wm.y * xm.x - wk.y * xk.x);
            const double hbr = 0.5 * (wm.x * xm.y + wk.x * xk.y), hbi = 0.5 * (wm.y * xm.y - wk.y * xk.y);
            r[im] = make_double2(har - hbi, hai + hbr);
        }
    }
    if (t < (1 << LROWS)) {
        const double w0 = ww[0].x;
        tile[t] = make_double2(w0 * tile[t].x, w0 * tile[t].y);
    }
    lds_barrier();
}

template <int LG, int LROWS, int T, int RS, int ST = 0, int SL = LG, class TW = const double2 *>
__device__ __forceinline__ void fft_rows_pipe(double2 *rows, int t, TW tw) {
    constexpr int NST = (LG + 3) >> 2;
    constexpr int BASEB = LG / NST, EXTRA = LG % NST;
    if constexpr (ST < NST) {
        constexpr int LR = BASEB + (ST < EXTRA ? 1 : 0);
        constexpr int LPR = LG - LR;
        constexpr int TOTAL = 1 << (LROWS + LPR);
#pragma unroll
        for (int b = t; b < TOTAL; b += T) dif_group<LR>(rows + (b >> LPR) * RS, SL, b & ((1 << LPR) - 1), LG, tw);
        lds_barrier();
        fft_rows_pipe<LG, LROWS, T, RS, ST + 1, SL - LR>(rows, t, tw);
    }
}

template <bool INVERSE, int LG>
__global__ void __launch_bounds__(PIPE_THREADS) k_dct_axis0_pipe(const double *__restrict__ src, double *__restrict__ dst,
                                                                  int nTiles, i64 ls /* doubles between lines */,
                                                                  const double2 *__restrict__ tw,
                                                                  const double2 *__restrict__ ww) {
    extern __shared__ double2 lds[];
    constexpr int n = 1 << LG, lh = LG - 1;
    constexpr int LPT = (2 << PIPE_LG_CPLX) / n;      // lines per tile
    constexpr int PPL = n / 128;                      // 1-KB DMA pieces per line
    constexpr int RS = n + 1;                         // odd row stride: rows start on different banks
    constexpr int lrows = PIPE_LG_CPLX - LG;          // 2^lrows rows (pairs of lines) per tile
    constexpr int BUF = RS << lrows;                  // complex elements per buffer
    // 2048-point lines: only the symmetric part of the tables fits beside the two buffers (TwQuarter, WwHalf)
    constexpr bool BIG = LG > 10;
    constexpr int NTW = BIG ? (n >> 2) : (n >> 1), NWW = BIG ? (n >> 1) + 1 : n;
    double2 *twS = lds + 2 * BUF, *wwS = twS + NTW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < NTW; i += PIPE_THREADS) twS[i] = tw[i];
    for (int i = tid; i < NWW; i += PIPE_THREADS) wwS[i] = ww[i];
    typename std::conditional<BIG, TwQuarter, const double2 *>::type twA;
    typename std::conditional<BIG, WwHalf, const double2 *>::type wwA;
    if constexpr (BIG) { twA = TwQuarter{twS, n >> 2}; wwA = WwHalf{wwS, n >> 1}; } else { twA = twS; wwA = wwS; }
    const unsigned ldsBase = (unsigned)(uintptr_t)lds;
    // the lines of a tile land back to back in LDS (n doubles apart) whatever their distance in memory
    auto dma = [&](int tile, int b) {
        const char *g = (const char *)(src + (i64)tile * LPT * ls) + lane * 16;
        const unsigned l0 = ldsBase + (unsigned)b * (unsigned)(BUF * 16) + (unsigned)(wave * PIPE_ND) * 1024u;
#pragma unroll
        for (int i = 0; i < PIPE_ND; ++i) {
            const int piece = wave * PIPE_ND + i;
            glds16(g + (i64)(piece / PPL) * (ls * 8) + (piece % PPL) * 1024, l0 + (unsigned)i * 1024u);
        }
    };
    int tile = blockIdx.x;
    const int stride = gridDim.x;
    if (tile < nTiles) dma(tile, 0);
    if (tile + stride < nTiles) dma(tile + stride, 1);
    // the first tile has landed when only the second one's DMA is outstanding (vector-memory operations of a wave
    // complete in issue order)
    if (tile + stride < nTiles) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(PIPE_ND) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
    // items of the staging / store loops: (row, j < n / 2) = (b >> lh, b & (n / 2 - 1)) for b = tid + u * threads, four per thread
    auto item_row = [&](int u) { return (tid + u * PIPE_THREADS) >> lh; };
    auto item_j = [&](int u) { return (tid + u * PIPE_THREADS) & ((1 << lh) - 1); };
    for (int it = 0; tile < nTiles; tile += stride, ++it) {
        const int b = it & 1;
        double2 *buf = lds + b * BUF;
        // raw lines (n doubles apart, unpadded) -> rows of pairs: all reads, barrier, all writes (same buffer)
        {
            const double *raw = (const double *)buf;
            double2 A[PIPE_IT], B[PIPE_IT];
#pragma unroll
            for (int u = 0; u < PIPE_IT; ++u) {
                const int rr = item_row(u), j0 = item_j(u);
                A[u] = *(const double2 *)(raw + (2 * rr) * n + 2 * j0);
                B[u] = *(const double2 *)(raw + (2 * rr + 1) * n + 2 * j0);
            }
            lds_barrier();
#pragma unroll
            for (int u = 0; u < PIPE_IT; ++u) {
                double2 *r = buf + item_row(u) * RS;
                const int j0 = item_j(u);
                if (!INVERSE) {
                    r[padi(j0)] = make_double2(A[u].x, B[u].x);
                    r[padi(n - 1 - j0)] = make_double2(A[u].y, B[u].y);
                } else {
                    r[padi(2 * j0)] = make_double2(A[u].x, B[u].x);
                    r[padi(2 * j0 + 1)] = make_double2(A[u].y, B[u].y);
                }
            }
        }
        lds_barrier();
        if (INVERSE) idct_combine_wg<true>(buf, lrows, LG, RS, tid, PIPE_THREADS, wwA);
        fft_rows_pipe<LG, lrows, PIPE_THREADS, RS>(buf, tid, twA);
        double *out = dst + (i64)tile * LPT * ls;
#pragma unroll
        for (int u = 0; u < PIPE_IT; ++u) {
            const int rr = item_row(u), j0 = item_j(u);
            const double2 *r = buf + rr * RS;
            double2 Av, Bv;
            if (!INVERSE) {
                const double2 p0 = dct_post(r, 2 * j0, n, LG, wwA), p1 = dct_post(r, 2 * j0 + 1, n, LG, wwA);
                Av = make_double2(p0.x, p1.x);
                Bv = make_double2(p0.y, p1.y);
            } else {
                const double2 v0 = r[padi(bitrev(j0, LG))], v1 = r[padi(bitrev(n - 1 - j0, LG))];
                Av = make_double2(v0.x, v1.x);
                Bv = make_double2(v0.y, v1.y);
            }
            *(double2 *)(out + (2 * rr) * ls + 2 * j0) = Av;
            *(double2 *)(out + (2 * rr + 1) * ls + 2 * j0) = Bv;
        }
        // the next tile has landed when only this tile's stores are outstanding; one barrier then says both "every wave's
        // pieces of the next tile are in LDS" and "this buffer is drained"
        if (tile + stride < nTiles) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(PIPE_NS) : "memory");
        lds_barrier();
        if (tile + 2 * stride < nTiles) dma(tile + 2 * stride, b);
    }
}

// Strided axes, pipelined (forward / inverse): a tile = 2^lrows pairs of lines that are consecutive in memory x all n
// elements = 4096 complex values, every (pair, k) one 16-byte access.  The tile lives in LDS pair-interleaved and in the
// order the transform wants: slot (padi(p) << lrows) + r holds position p of pair r, i.e. line element k = 2 p resp.
// 2 (n - 1 - p) + 1 (Makhoul order, forward) or k = p (inverse).  An LDS-DMA piece fills 64 consecutive slots = 64 / NP
// positions of all NP pairs: each lane fetches its own (pair, k) element, a piece still reads 64 / NP whole segments of
// NP x 16 bytes, and the tile is ready for the first butterfly group when it has landed -- no staging pass.  At
// n = 1024 a tile is 64 bytes wide: the workgroups are ordered such that the two tiles sharing every 128-byte line run
// at the same time on the same XCD (one fetch into its L2).
template <int MODE /*0 fwd, 1 inv*/, int LG>
__global__ void __launch_bounds__(PIPE_THREADS) k_dct_strided_pipe(const double *__restrict__ src, double *__restrict__ dst,
                                                                    LineMap map, int nTiles, const double2 *__restrict__ tw,
                                                                    const double2 *__restrict__ ww) {
    extern __shared__ double2 lds[];
    constexpr int n = 1 << LG;
    constexpr int lrows = PIPE_LG_CPLX - LG;          // log2(pairs per tile)
    constexpr int NP = 1 << lrows;
    constexpr int BUF = 1 << PIPE_LG_CPLX;            // complex elements per buffer (no padding: the swizzle permutes)
    constexpr bool BIG = LG > 10;                     // 2048-point lines: symmetric part of the tables only (see k_dct_axis0_pipe)
    constexpr int NTW = BIG ? (n >> 2) : (n >> 1), NWW = BIG ? (n >> 1) + 1 : n;
    double2 *twS = lds + 2 * BUF, *wwS = twS + NTW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < NTW; i += PIPE_THREADS) twS[i] = tw[i];
    for (int i = tid; i < NWW; i += PIPE_THREADS) wwS[i] = ww[i];
    typename std::conditional<BIG, TwQuarter, const double2 *>::type twA;
    typename std::conditional<BIG, WwHalf, const double2 *>::type wwA;
    if constexpr (BIG) { twA = TwQuarter{twS, n >> 2}; wwA = WwHalf{wwS, n >> 1}; } else { twA = twS; wwA = wwS; }
    const unsigned ldsBase = (unsigned)(uintptr_t)lds;
    // element offset of a tile's first line (the 2 NP lines of a tile are consecutive in memory: nin % (2 NP) == 0)
    auto tile_base = [&](int tile) { return map.base((i64)tile << (lrows + 1)); };
    auto dma = [&](int tile, int b) {
        const double *g0 = src + tile_base(tile) + 2 * (lane & (NP - 1));
        const unsigned l0 = ldsBase + (unsigned)b * (unsigned)(BUF * 16);
#pragma unroll
        for (int i = 0; i < PIPE_ND; ++i) {
            const int c = wave * PIPE_ND + i;                         // piece: slots 64 c .. 64 c + 63
            const int p = padi(((c << 6) + lane) >> lrows);          // position held by this lane's slot
            const int k = (MODE == 1) ? p : ((p < (n >> 1)) ? 2 * p : 2 * (n - 1 - p) + 1);
            glds16(g0 + (i64)k * map.es, l0 + (unsigned)c * 1024u);
        }
    };
    // tile order: workgroup w runs on XCD w % 8; the tiles 2p and 2p + 1 (n = 2048, tiles 32 bytes wide: 4p .. 4p + 3) that
    // share every 128-byte line go to workgroups of one XCD at the same time
    const int w = blockIdx.x, stride = gridDim.x;     // gridDim.x is a multiple of 32
    int tile = BIG ? (((((w >> 5) << 3) + (w & 7)) << 2) | ((w >> 3) & 3))
                   : (((((w >> 4) << 3) + (w & 7)) << 1) | ((w >> 3) & 1));
    if (tile < nTiles) dma(tile, 0);
    if (tile + stride < nTiles) dma(tile + stride, 1);
    // the first tile has landed when only the second one's DMA is outstanding (vector-memory operations of a wave
    // complete in issue order)
    if (tile + stride < nTiles) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(PIPE_ND) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
    for (int it = 0; tile < nTiles; tile += stride, ++it) {
        const int b = it & 1;
        double2 *buf = lds + b * BUF;
        if (MODE == 1) idct_combine_tile<LG, lrows, PIPE_THREADS>(buf, tid, wwA);
        fft_tile_pipe<LG, lrows, PIPE_THREADS>(buf, tid, twA);
        {
            // item u of this thread: pair r0, k = k0 + u * (threads / NP)
            const int r0 = tid & (NP - 1), k0 = tid >> lrows;
            const double2 *rr = buf + r0;
            double *o = dst + tile_base(tile) + 2 * r0 + (i64)k0 * map.es;
            const i64 ostep = (i64)(PIPE_THREADS >> lrows) * map.es;
#pragma unroll
            for (int u = 0; u < 2 * PIPE_IT; ++u) {
                const int k = k0 + u * (PIPE_THREADS >> lrows);
                double2 v;
                if (MODE == 0) v = dct_post<lrows>(rr, k, n, LG, wwA);
                else v = rr[padi(bitrev(makhoul(k, n), LG)) << lrows];
                *(double2 *)o = v;
                o += ostep;
            }
        }
        // the next tile has landed when only this tile's stores are outstanding; one barrier then says both "every wave's
        // pieces of the next tile are in LDS" and "this buffer is drained"
        if (tile + stride < nTiles) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(PIPE_NS) : "memory");
        lds_barrier();
        if (tile + 2 * stride < nTiles) dma(tile + 2 * stride, b);
    }
}

// Fused t-axis solve (k_dct_strided<2>: forward DCT, division by the spectral kernel, inverse DCT), pipelined.  A tile =
// 2^lrows pairs of consecutive columns (y, y + 1) x all n time nodes, pair-interleaved in LDS like the strided kernel's;
// the eigenvalue tables CY, CT sit in LDS beside the twiddles (no ordinary global load inside the loop; CX of the tile's
// one x is a scalar load, which the vector memory counter does not see).  This pass is bound by its own chain of LDS /
// VALU phases (two transforms, seven barriers per tile), not by HBM: tiles of 2048 values and workgroups of 256 threads, so that TWO workgroups fit a CU
// and fill each other's gaps (tiles of 1024 values with 256 threads, three workgroups per CU: 2.71 instead of 2.48 ms for the
// whole solve at 1024 x 1024 x 128; with 128 threads: 2.48 -- measured, not kept).  Needs ny % (lines per tile) == 0: a tile has one x.
#define TS_THREADS 256
#define TS_LG_CPLX 11
#define TS_IT ((1 << (TS_LG_CPLX - 1)) / TS_THREADS)
template <int LG>
__global__ void __launch_bounds__(TS_THREADS) k_dct_tsolve_pipe(const double *__restrict__ src, double *__restrict__ dst,
                                                                 LineMap map, int nTiles, SolveArgs sa,
                                                                 const double2 *__restrict__ tw,
                                                                 const double2 *__restrict__ ww) {
    extern __shared__ double2 lds[];
    constexpr int n = 1 << LG;
    constexpr int lrows = TS_LG_CPLX - LG;
    constexpr int NP = 1 << lrows;
    constexpr int BUF = 1 << TS_LG_CPLX;              // pair-interleaved tile (see k_dct_strided_pipe), no padding
    constexpr int TS_ND = (1 << (TS_LG_CPLX - 6)) / (TS_THREADS / 64);     // DMA pieces per wave and tile
    static_assert(TS_ND == PIPE_ND && (1 << TS_LG_CPLX) / TS_THREADS == PIPE_NS, "wait counts are shared with the other pipes");
    double2 *twS = lds + 2 * BUF, *wwS = twS + (n >> 1);
    double *ctS = (double *)(wwS + n), *cyS = ctS + n;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < (n >> 1); i += TS_THREADS) twS[i] = tw[i];
    for (int i = tid; i < n; i += TS_THREADS) wwS[i] = ww[i];
    for (int i = tid; i < n; i += TS_THREADS) ctS[i] = sa.ct[i];
    for (int i = tid; i < (int)sa.ny; i += TS_THREADS) cyS[i] = sa.cy[i];
    const unsigned ldsBase = (unsigned)(uintptr_t)lds;
    // slot (padi(p) << lrows) + r holds position p of pair r; the forward transform is decimation-in-time, so position p
    // is element makhoul^-1(bitrev(p)) of the line
    auto dma = [&](int tile, int b) {
        const double *g0 = src + map.base((i64)tile << (lrows + 1)) + 2 * (lane & (NP - 1));   // pitched rows: a tile lies in one row
        const unsigned l0 = ldsBase + (unsigned)b * (unsigned)(BUF * 16);
#pragma unroll
        for (int i = 0; i < TS_ND; ++i) {
            const int c = wave * TS_ND + i;
            const int q = bitrev(padi(((c << 6) + lane) >> lrows), LG);
            const int k = (q < (n >> 1)) ? 2 * q : 2 * (n - 1 - q) + 1;
            glds16(g0 + (i64)k * map.es, l0 + (unsigned)c * 1024u);
        }
    };
    int tile = blockIdx.x;
    const int stride = gridDim.x;
    if (tile < nTiles) dma(tile, 0);
    if (tile + stride < nTiles) dma(tile + stride, 1);
    // the first tile has landed when only the second one's DMA is outstanding (vector-memory operations of a wave
    // complete in issue order)
    if (tile + stride < nTiles) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(PIPE_ND) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
    for (int it = 0; tile < nTiles; tile += stride, ++it) {
        const int b = it & 1;
        double2 *buf = lds + b * BUF;
        fft_tile_pipe_dit<LG, lrows, TS_THREADS>(buf, tid, twS);
        // spectrum in natural order: DCT post-processing, division, inverse pre-processing on the pair (k, n - k)
        {
            const i64 G0 = sa.line0 + ((i64)tile << (lrows + 1));     // first column of the tile: (y0, x0)
            const int y0 = (int)(G0 % sa.ny), x0 = (int)(G0 / sa.ny);
            const double ex = sload_f64(sa.cx + x0);
#pragma unroll
            for (int u = 0; u < TS_IT; ++u) {
                const int bb = tid + u * TS_THREADS;
                const int rr = bb & (NP - 1);
                double2 *r = buf + rr;
                const double ea = cyS[y0 + 2 * rr] + ex, eb = cyS[y0 + 2 * rr + 1] + ex;
                const int k = (bb >> lrows) + 1;                   // 1 .. n/2
                const int m = n - k;
                const int ik = padi(k) << lrows, im = padi(m) << lrows;
                const double2 vk = r[ik], vm = r[im];
                const double2 wk = wwS[k], wm = wwS[m];
                const double ar = 0.5 * (vk.x + vm.x), ai = 0.5 * (vk.y - vm.y);
                const double br = 0.5 * (vk.y + vm.y), bi = -0.5 * (vk.x - vm.x);
                const double ctk = ctS[k], ctm = ctS[m];
                double lak = ea + ctk, lbk = eb + ctk, lam = ea + ctm, lbm = eb + ctm;
                if (lak == 0.0) lak = 1.0;
                if (lbk == 0.0) lbk = 1.0;
                if (lam == 0.0) lam = 1.0;
                if (lbm == 0.0) lbm = 1.0;
                const double2 xk = make_double2((wk.x * ar - wk.y * ai) / (sa.kscale * lak),
                                                (wk.x * br - wk.y * bi) / (sa.kscale * lbk));
                const double2 xm = make_double2((wm.x * ar + wm.y * ai) / (sa.kscale * lam),
                                                (wm.x * br + wm.y * bi) / (sa.kscale * lbm));
                const double gar = 0.5 * (wk.x * xk.x + wm.x * xm.x), gai = 0.5 * (wk.y * xk.x - wm.y * xm.x);
                const double gbr = 0.5 * (wk.x * xk.y + wm.x * xm.y), gbi = 0.5 * (wk.y * xk.y - wm.y * xm.y);
                r[ik] = make_double2(gar - gbi, gai + gbr);
                if (m != k) {
                    const double har = 0.5 * (wm.x * xm.x + wk.x * xk.x), hai = 0.5 * (wm.y * xm.x - wk.y * xk.x);
                    const double hbr = 0.5 * (wm.x * xm.y + wk.x * xk.y), hbi = 0.5 * (wm.y * xm.y - wk.y * xk.y);
                    r[im] = make_double2(har - hbi, hai + hbr);
                }
            }
            if (tid < NP) {                                        // k = 0: V[0] is its own partner
                const int rr = tid;
                double2 *r = buf + rr;
                double la = (cyS[y0 + 2 * rr] + ex) + ctS[0];
                double lb2 = (cyS[y0 + 2 * rr + 1] + ex) + ctS[0];
                if (la == 0.0) la = 1.0;
                if (lb2 == 0.0) lb2 = 1.0;
                const double w0 = wwS[0].x;
                const double2 v0 = r[0];
                r[0] = make_double2(w0 * ((w0 * v0.x) / (sa.kscale * la)), w0 * ((w0 * v0.y) / (sa.kscale * lb2)));
            }
        }
        lds_barrier();
        fft_tile_pipe<LG, lrows, TS_THREADS>(buf, tid, twS);
        {
            const int r0 = tid & (NP - 1), k0 = tid >> lrows;
            const double2 *rr = buf + r0;
            double *o = dst + map.base((i64)tile << (lrows + 1)) + 2 * r0 + (i64)k0 * map.es;
            const i64 ostep = (i64)(TS_THREADS >> lrows) * map.es;
#pragma unroll
            for (int u = 0; u < 2 * TS_IT; ++u) {
                const int k = k0 + u * (TS_THREADS >> lrows);
                *(double2 *)o = rr[padi(bitrev(makhoul(k, n), LG)) << lrows];
                o += ostep;
            }
        }
        // the next tile has landed when only this tile's stores are outstanding; one barrier then says both "every wave's
        // pieces of the next tile are in LDS" and "this buffer is drained"
        if (tile + stride < nTiles) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(PIPE_NS) : "memory");
        lds_barrier();
        if (tile + 2 * stride < nTiles) dma(tile + 2 * stride, b);
    }
}

// Strided axes, workgroup-wide (forward / inverse only; 16-byte accesses: both lines of a pair per access).
template <int MODE /*0 fwd, 1 inv*/, int T>
__global__ void __launch_bounds__(T, 4) k_dct_strided_wg(const double *__restrict__ src,
                                                                       double *__restrict__ dst, LineMap map, int lg,
                                                                       int lp, const double2 *__restrict__ tw,
                                                                       const double2 *__restrict__ ww) {
    extern __shared__ double2 lds[];
    const int n = 1 << lg;
    const int rowStride = row_stride(n);
    const int npairs = 1 << lp;
    const int tid = threadIdx.x;
    const i64 L0 = xcd_tile(blockIdx.x, gridDim.x) << (lp + 1);
    const int r = tid & (npairs - 1);
    const i64 L = L0 + 2 * r;
    const bool ok = L < map.nLines;
    const i64 lb = ok ? map.base(L) : 0;
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
            if (k < n) lds[r * rowStride + padi(MODE == 1 ? k : makhoul(k, n))] = gv[u];
        }
    }
    __syncthreads();
    if (MODE == 1) idct_combine_wg(lds, lp, lg, rowStride, tid, T, ww);
    fft_rows_wg(lds, lp, lg, rowStride, tid, T, tw);
    if (ok) {
        const double2 *rr = lds + r * rowStride;
        for (int k = tid >> lp; k < n; k += kstep) {
            double2 v;
            if (MODE == 0) v = dct_post(rr, k, n, lg, ww);
            else v = rr[padi(bitrev(makhoul(k, n), lg))];
            *(double2 *)(dst + lb + (i64)k * map.es) = v;
        }
    }
}

#define DCT_LDS_BUDGET (72 * 1024)

static int floor_log2(i64 v) {
    int l = 0;
    while (((i64)2 << l) <= v) ++l;
    return l;
}

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
// log2 of the line lengths the pipelined kernels are instantiated for
#define TS_LG_MIN 5
#define TS_LG_MAX 10
#define PIPE_LG_MIN 7
#define PIPE_LG_MAX 11

// ---------------------------------------------------------------------------------------------
// Which kernel a pass takes.  choose_strided / choose_axis0 are pure host arithmetic on the shape of the pass, the
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
        c.ldsPipe = (((size_t)2 << TS_LG_CPLX) + (size_t)(n >> 1) + (size_t)n) * sizeof(double2) +
                    ((size_t)n + (size_t)ny) * sizeof(double);
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
            // tables: n / 2 twiddles + n weights (2048-point lines: n / 4 + n / 2 + 1, TwQuarter / WwHalf)
            const size_t ntab = lg > 10 ? (size_t)(n >> 2) + (size_t)(n >> 1) + 1 : (size_t)(n >> 1) + (size_t)n;
            c.ldsPipe = (((size_t)2 << PIPE_LG_CPLX) + ntab) * sizeof(double2);
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

static int lg_of(i64 n) {
    int lg = 0;
    while (((i64)1 << lg) < n) ++lg;
    return lg;
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
            const size_t rs = (size_t)n + 1;
            const size_t ntab = lg > 10 ? (size_t)(n >> 2) + (size_t)(n >> 1) + 1 : (size_t)(n >> 1) + (size_t)n;
            c.ldsPipe = (2 * (rs << (PIPE_LG_CPLX - lg)) + ntab) * sizeof(double2);
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
    const int lg = lg_of(n);
    if (axis0) return pass_kind_of(choose_axis0(n, lg, map, true, ncu).kind);
    return pass_kind_of(choose_strided(0, (int)n, lg, map, 0, 0, 0, true, ncu).kind);
}

bool pow2_tsolve_pipelined(i64 n, i64 ny, i64 nplane, i64 line0, i64 nl, i64 pitch0, int ncu) {
    const LineMap map = tsolve_map(ny, nplane, nl, pitch0);
    return map.nLines > 0 && choose_strided(2, (int)n, lg_of(n), map, ny, line0, nplane, true, ncu).kind == PK_TSOLVE_PIPE;
}

}  // namespace dotsocp
