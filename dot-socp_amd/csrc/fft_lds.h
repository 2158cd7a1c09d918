// LDS FFT building blocks shared by the power-of-two DCT kernels (dct_pow2.hip) and the convolution-based DFT
// (cdft.hip): line addressing, the bank-spreading row layout, radix-2 register groups (decimation in frequency
// and in time), the two drivers over them (fft_rows: sizes known at run time, fft_tile: at compile time), the arithmetic
// on a pair (k, n - k) of a DCT's spectrum, and the integer logarithms of the host side.
#pragma once
#include "device_utils.h"

#include <mutex>

namespace dotsocp {

// Line addressing shared by all axes: line L, element k lives at
//   (L % nin) + (L / nin) * outerStride + k * nin
// axis 0: nin = 1, outerStride = n;  axis 1: nin = n0, outerStride = n0*n1;  axis 2: nin = n0*n1.
// With pitched rows (pitch >= n0) the element stride is no longer the line count per group:
// axis 0: nin = 1, outerStride = pitch, es = 1;  axis 1: nin = n0, outerStride = pitch*n1, es = pitch;
// axis 2: nin = n0, outerStride = pitch, es = pitch*n1.  (The power-of-two kernels run unpitched: es == nin there.)
struct LineMap {
    i64 nin, outerStride, nLines, es;
    __device__ __forceinline__ i64 base(i64 L) const { return (L % nin) + (L / nin) * outerStride; }
    __device__ __forceinline__ i64 addr(i64 L, i64 k) const { return base(L) + k * es; }
};

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

__device__ __forceinline__ int bitrev(int k, int lg) { return (int)(__brev((unsigned)k) >> (32 - lg)); }

// Position of element p inside its LDS row: the low four bits (which sixteenth of the 64 banks a 16-byte element
// falls on) are XOR-ed with the next two groups of four bits, so that the stride-16 / stride-64 / ... accesses of the
// grouped FFT stages AND the bit-reversed reads of the post-processing (consecutive k -> multiples of n / 16 apart)
// spread over all banks; a permutation inside aligned blocks of 16, so rows need no padding.  (Additive padding
// p + p / 16 left the bit-reversed reads four deep on the same banks and cost n / 16 elements per row.)
__device__ __host__ __forceinline__ int padi(int p) { return p ^ ((p >> 4) & 15) ^ ((p >> 8) & 15); }
__device__ __host__ __forceinline__ int row_stride(int n) { return n + (n >> 4) + 1; }

// LDS hand-off between the lanes of ONE wavefront: DS operations of a wave execute in order, so
// draining the wave's outstanding LDS operations is all the synchronisation that is needed.
__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// d * exp(-2 pi i t / 16), t in [0, 8): the constant part of the twiddles inside a register group
__device__ __forceinline__ double2 mul_w16(double2 d, int t) {
    const double h = 0.70710678118654752440;   // cos(pi/4)
    const double c1 = 0.92387953251128675613;  // cos(pi/8)
    const double s1 = 0.38268343236508977173;  // sin(pi/8)
    switch (t) {
        case 0: return d;
        case 1: return make_double2(d.x * c1 + d.y * s1, d.y * c1 - d.x * s1);
        case 2: return make_double2(h * (d.x + d.y), h * (d.y - d.x));
        case 3: return make_double2(d.x * s1 + d.y * c1, d.y * s1 - d.x * c1);
        case 4: return make_double2(d.y, -d.x);
        case 5: return make_double2(d.y * c1 - d.x * s1, -(d.x * c1 + d.y * s1));
        case 6: return make_double2(h * (d.y - d.x), -h * (d.x + d.y));
        default: return make_double2(d.y * s1 - d.x * c1, -(d.x * s1 + d.y * c1));
    }
}

// One group of LR radix-2 stages done in registers: the lane owns the R = 2^LR elements base + m * (S/R) of one
// sub-transform of span S = 2^sl and performs the butterflies of LR spans on them.
//   DIT = false, decimation in frequency: spans S, S/2, ..., S/2^(LR-1), the twiddle applied after the subtraction (same
//                data flow as LR passes of the textbook in-place radix-2 DIF, so the output order is plain bit reversal)
//   DIT = true,  decimation in time: the same element set, spans S/2^(LR-1), ..., S/2, S in INCREASING order with the
//                twiddle applied before the add / subtract -- bit-reversed input, natural-order output.  Used where the
//                spectrum is needed in place in natural order (fused t-axis solve).
// LES > 0: the rows of a tile are interleaved element by element (element p of row r at (padi(p) << LES) + r, `row`
// = tile + r) -- the image an LDS-DMA piece leaves when each lane fetches one (pair, k) element; LES = 0: plain rows
template <bool DIT, int LR, int LES = 0, class TW = const double2 *>
__device__ __forceinline__ void fft_group(double2 *__restrict__ row, int sl, int bidx, int lg, TW tw) {
    constexpr int R = 1 << LR;
    const int strideLog = sl - LR;
    const int j = bidx & ((1 << strideLog) - 1);
    const int base = ((bidx >> strideLog) << sl) + j;
    double2 x[R];
#pragma unroll
    for (int m = 0; m < R; ++m) x[m] = row[padi(base + (m << strideLog)) << LES];
    const int tj = j << (lg - sl);   // j * N / S
#pragma unroll
    for (int i = 0; i < LR; ++i) {
        const int u = DIT ? LR - 1 - i : i;
        const int hm = R >> (u + 1);
        const double2 bu = tw[tj << u];
#pragma unroll
        for (int m = 0; m < R; ++m) {
            if ((m / hm) & 1) continue;
            const int mm = m % hm;
            if constexpr (!DIT) {
                const double2 a = x[m], b = x[m + hm];
                x[m] = make_double2(a.x + b.x, a.y + b.y);
                double2 d = make_double2(a.x - b.x, a.y - b.y);
                d = mul_w16(d, (mm << u) * (16 / R));
                x[m + hm] = cmul(d, bu);
            } else {
                const double2 a = x[m];
                const double2 t = cmul(mul_w16(x[m + hm], (mm << u) * (16 / R)), bu);
                x[m] = make_double2(a.x + t.x, a.y + t.y);
                x[m + hm] = make_double2(a.x - t.x, a.y - t.y);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < R; ++m) row[padi(base + (m << strideLog)) << LES] = x[m];
}

// Makhoul reordering v[j] = x[2j], v[n-1-j] = x[2j+1] (mirt_dctn.m:71) -- also the output
// reordering of the inverse (mirt_idctn.m:71-73,120).
__device__ __forceinline__ int makhoul(int k, int n) { return (k & 1) ? (n - 1 - (k >> 1)) : (k >> 1); }

// ---------------------------------------------------------------------------------------------
// Drivers over the register groups.  A TEAM is the set of threads that shares the rows: its member t is the calling
// thread's index in it, T the thread count, sync() the hand-off after every register group.
//   WaveTeam      one wavefront: DS operations of a wave execute in order, draining them is all the hand-off needed
//   BlockTeam<T>  the workgroup, __syncthreads()
//   PipeTeam<T>   the workgroup, lds_barrier(): waits for LDS traffic only, so that the global loads and stores of the
//                 pipelined kernels stay in flight across it
// ---------------------------------------------------------------------------------------------
enum { SYNC_WAVE, SYNC_BLOCK, SYNC_LDS };
template <int NT, int SYNC>
struct Team {
    int t;
    static constexpr int T = NT;
    static __device__ __forceinline__ void sync() {
        if constexpr (SYNC == SYNC_WAVE) wave_lds_sync();
        else if constexpr (SYNC == SYNC_BLOCK) __syncthreads();
        else lds_barrier();
    }
};
using WaveTeam = Team<64, SYNC_WAVE>;
template <int T> using BlockTeam = Team<T, SYNC_BLOCK>;
template <int T> using PipeTeam = Team<T, SYNC_LDS>;

// FFT of the 2^lrows complex rows (length n = 2^lg, rowStride apart) that the team shares, in LDS: ceil(lg/4) register
// groups dealt round-robin to the team's threads, a hand-off after each.  DIT = false: natural order in, bit-reversed
// order out; DIT = true: the same groups in reverse order, bit-reversed order in, natural order out.
template <bool DIT, class TEAM, class TW = const double2 *>
__device__ __forceinline__ void fft_rows(double2 *rows, int lrows, int lg, int rowStride, TEAM tm, TW tw) {
    const int nst = (lg + 3) >> 2;
    const int baseBits = lg / nst, extra = lg % nst;
    int sl = DIT ? 0 : lg;
    for (int st = DIT ? nst - 1 : 0; DIT ? st >= 0 : st < nst; st += DIT ? -1 : 1) {
        const int lr = baseBits + (st < extra ? 1 : 0);
        if (DIT) sl += lr;
        const int lpr = lg - lr;                        // log2(groups per row)
        const int total = 1 << (lrows + lpr);
        for (int b = tm.t; b < total; b += TEAM::T) {
            double2 *r = rows + (b >> lpr) * rowStride;
            const int bidx = b & ((1 << lpr) - 1);
            switch (lr) {
                case 4: fft_group<DIT, 4>(r, sl, bidx, lg, tw); break;
                case 3: fft_group<DIT, 3>(r, sl, bidx, lg, tw); break;
                case 2: fft_group<DIT, 2>(r, sl, bidx, lg, tw); break;
                default: fft_group<DIT, 1>(r, sl, bidx, lg, tw); break;
            }
        }
        if (!DIT) sl -= lr;
        TEAM::sync();
    }
}

// The same register groups for a length and a tile known at compile time (same plan, same arithmetic), lds_barrier()
// after each.  RS > 0: 2^LROWS plain rows, RS apart.  RS = 0: a pair-interleaved tile (LES = LROWS above): item b =
// (row b % rows, group b / rows), so the lanes of a wave sweep the rows of one element first -- consecutive addresses.
template <bool DIT, int LG, int LROWS, int T, int RS = 0, int I = 0, int SL = (DIT ? 0 : LG), class TW = const double2 *>
__device__ __forceinline__ void fft_tile(double2 *tile, int t, TW tw) {
    constexpr int NST = (LG + 3) >> 2;
    constexpr int BASEB = LG / NST, EXTRA = LG % NST;
    if constexpr (I < NST) {
        constexpr int ST = DIT ? NST - 1 - I : I;
        constexpr int LR = BASEB + (ST < EXTRA ? 1 : 0);
        constexpr int S = DIT ? SL + LR : SL;           // log2 of the span this group works on
        constexpr int LPR = LG - LR;
        constexpr int TOTAL = 1 << (LROWS + LPR);
#pragma unroll
        for (int b = t; b < TOTAL; b += T) {
            if constexpr (RS == 0) fft_group<DIT, LR, LROWS>(tile + (b & ((1 << LROWS) - 1)), S, b >> LROWS, LG, tw);
            else fft_group<DIT, LR>(tile + (b >> LPR) * RS, S, b & ((1 << LPR) - 1), LG, tw);
        }
        lds_barrier();
        fft_tile<DIT, LG, LROWS, T, RS, I + 1, (DIT ? S : S - LR)>(tile, t, tw);
    }
}

// ---------------------------------------------------------------------------------------------
// The arithmetic on a pair (k, n - k) of the spectrum of two real lines (a in the real, b in the imaginary part), shared
// by every DCT built on a complex FFT here.  These files contract a * b + c, so every expression below is the one its
// callers used to spell out, term for term: a regrouped sum rounds differently.
// (pfa.hip keeps its own pfa_pre / pfa_post: it compiles with contraction off and folds the signs so that the two halves
// of a pair share their products -- gk = (gar - gbi, gai + gbr), gm = (gar + gbi, gbr - gai) -- which is a different
// expression tree from the two idct_half calls below and rounds differently once contracted.)
// ---------------------------------------------------------------------------------------------
// Inverse pre-processing: G[k] = (ww[k] X[k] + conj(ww[n-k]) X[n-k]) / 2, so that fft(G) = real(fft(ww .* X))
// (mirt_idctn.m:109,119-120), for X = Xa + i Xb.  G[n-k] is the same call with the roles of k and n - k swapped.
__device__ __forceinline__ double2 idct_half(double2 wk, double2 xk, double2 wm, double2 xm) {
    const double gar = 0.5 * (wk.x * xk.x + wm.x * xm.x), gai = 0.5 * (wk.y * xk.x - wm.y * xm.x);
    const double gbr = 0.5 * (wk.x * xk.y + wm.x * xm.y), gbi = 0.5 * (wk.y * xk.y - wm.y * xm.y);
    return make_double2(gar - gbi, gai + gbr);
}

// Forward post-processing: the spectra of the two lines from V = fft(va + i vb),
// V_a = (V[k] + conj(V[n-k])) / 2 = ar + i ai, V_b = (V[k] - conj(V[n-k])) / (2i) = br + i bi, and
// (Xa[k], Xb[k]) = real(ww[k] V_{a,b}[k]), (Xa[n-k], Xb[n-k]) = real(ww[n-k] conj(V_{a,b}[k]))   (mirt_dctn.m:130)
struct DctSplit {
    double ar, ai, br, bi;
    __device__ __forceinline__ double2 at_k(double2 w) const { return make_double2(w.x * ar - w.y * ai, w.x * br - w.y * bi); }
    __device__ __forceinline__ double2 at_m(double2 w) const { return make_double2(w.x * ar + w.y * ai, w.x * br + w.y * bi); }
};
__device__ __forceinline__ DctSplit dct_split(double2 vk, double2 vm) {
    return DctSplit{0.5 * (vk.x + vm.x), 0.5 * (vk.y - vm.y), 0.5 * (vk.y + vm.y), -0.5 * (vk.x - vm.x)};
}

// ---- host side ----
constexpr int floor_log2(i64 v) {
    int l = 0;
    while (((i64)2 << l) <= v) ++l;
    return l;
}
constexpr int ceil_log2(i64 v) {
    int l = 0;
    while (((i64)1 << l) < v) ++l;
    return l;
}

// the dynamic-LDS limit of the kernels built on these rows
#define DCT_LDS_MAX (160 * 1024)

template <class K>
static void allow_big_lds(K kernel, int bytes = DCT_LDS_MAX) {
    (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// Function attributes belong to the (function, device) pair: a process that drives several GPUs (dotsocp_create_multi)
// has to raise the dynamic-LDS limit once on EVERY device it launches on.  true = not done yet on the current device.
inline std::mutex attr_mutex;
struct DeviceOnce {
    // `if (DeviceOnce once(mask); once) { raise the attributes }`: the lock is held while they are raised and the device's
    // bit is set only afterwards, so a second host thread can neither skip the block early nor launch in between
    std::unique_lock<std::mutex> lock;
    unsigned long long *mask;
    unsigned long long bit = 0;
    bool first = true;
    explicit DeviceOnce(unsigned long long &m) : lock(attr_mutex), mask(&m) {
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) {
            bit = 1ull << dev;
            first = !(m & bit);
        }
    }
    ~DeviceOnce() { if (first && bit) *mask |= bit; }
    explicit operator bool() const { return first; }
};

}  // namespace dotsocp
