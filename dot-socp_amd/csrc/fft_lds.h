// LDS FFT building blocks shared by the power-of-two DCT kernels (dct_pow2.hip) and the convolution-based DFT
// (cdft.hip): line addressing, the bank-spreading row layout, radix-2 register groups (decimation in frequency
// and in time) and the per-wave / per-workgroup drivers over them.
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

// One group of LR radix-2 decimation-in-frequency stages done in registers: the lane owns the
// R = 2^LR elements base + m * (S/R) of one sub-transform of span S = 2^sl and performs the
// butterflies of spans S, S/2, ..., S/2^(LR-1) on them (same data flow as LR passes of the
// textbook in-place radix-2 DIF, so the output order is plain bit reversal).
// LES > 0: the rows of a tile are interleaved element by element (element p of row r at (padi(p) << LES) + r, `row`
// = tile + r) -- the image an LDS-DMA piece leaves when each lane fetches one (pair, k) element; LES = 0: plain rows
template <int LR, int LES = 0, class TW = const double2 *>
__device__ __forceinline__ void dif_group(double2 *__restrict__ row, int sl, int bidx, int lg, TW tw) {
    constexpr int R = 1 << LR;
    const int strideLog = sl - LR;
    const int j = bidx & ((1 << strideLog) - 1);
    const int base = ((bidx >> strideLog) << sl) + j;
    double2 x[R];
#pragma unroll
    for (int m = 0; m < R; ++m) x[m] = row[padi(base + (m << strideLog)) << LES];
    const int tj = j << (lg - sl);   // j * N / S
#pragma unroll
    for (int u = 0; u < LR; ++u) {
        const int hm = R >> (u + 1);
        const double2 bu = tw[tj << u];
#pragma unroll
        for (int m = 0; m < R; ++m) {
            if ((m / hm) & 1) continue;
            const int mm = m % hm;
            const double2 a = x[m], b = x[m + hm];
            x[m] = make_double2(a.x + b.x, a.y + b.y);
            double2 d = make_double2(a.x - b.x, a.y - b.y);
            d = mul_w16(d, (mm << u) * (16 / R));
            x[m + hm] = cmul(d, bu);
        }
    }
#pragma unroll
    for (int m = 0; m < R; ++m) row[padi(base + (m << strideLog)) << LES] = x[m];
}

// FFT of the `nrows` = 2^lrw complex rows (length n = 2^lg) owned by the CALLING WAVE, in LDS:
// natural order in, bit-reversed order out; ceil(lg/4) register groups with a wave-level LDS
// hand-off after each (no workgroup barrier).
__device__ __forceinline__ void fft_rows_wave(double2 *rows, int lrw, int lg, int rowStride, int lane,
                                              const double2 *__restrict__ tw) {
    const int nst = (lg + 3) >> 2;
    const int baseBits = lg / nst, extra = lg % nst;
    int sl = lg;
    for (int st = 0; st < nst; ++st) {
        const int lr = baseBits + (st < extra ? 1 : 0);
        const int lpr = lg - lr;                        // log2(butterflies per row)
        const int total = 1 << (lrw + lpr);
        for (int b = lane; b < total; b += 64) {
            double2 *r = rows + (b >> lpr) * rowStride;
            const int bidx = b & ((1 << lpr) - 1);
            switch (lr) {
                case 4: dif_group<4>(r, sl, bidx, lg, tw); break;
                case 3: dif_group<3>(r, sl, bidx, lg, tw); break;
                case 2: dif_group<2>(r, sl, bidx, lg, tw); break;
                default: dif_group<1>(r, sl, bidx, lg, tw); break;
            }
        }
        sl -= lr;
        wave_lds_sync();
    }
}

// Decimation-in-time twin of dif_group: same element set (base + m * S/R), the butterflies of spans S/2^(LR-1),
// ..., S/2, S in INCREASING order with the twiddle applied before the add / subtract -- bit-reversed input,
// natural-order output.  Used where the spectrum is needed in place in natural order (fused t-axis solve).
template <int LR, int LES = 0, class TW = const double2 *>
__device__ __forceinline__ void dit_group(double2 *__restrict__ row, int sl, int bidx, int lg, TW tw) {
    constexpr int R = 1 << LR;
    const int strideLog = sl - LR;
    const int j = bidx & ((1 << strideLog) - 1);
    const int base = ((bidx >> strideLog) << sl) + j;
    double2 x[R];
#pragma unroll
    for (int m = 0; m < R; ++m) x[m] = row[padi(base + (m << strideLog)) << LES];
    const int tj = j << (lg - sl);   // j * N / S
#pragma unroll
    for (int u = LR - 1; u >= 0; --u) {
        const int hm = R >> (u + 1);
        const double2 bu = tw[tj << u];
#pragma unroll
        for (int m = 0; m < R; ++m) {
            if ((m / hm) & 1) continue;
            const int mm = m % hm;
            const double2 a = x[m];
            const double2 t = cmul(mul_w16(x[m + hm], (mm << u) * (16 / R)), bu);
            x[m] = make_double2(a.x + t.x, a.y + t.y);
            x[m + hm] = make_double2(a.x - t.x, a.y - t.y);
        }
    }
#pragma unroll
    for (int m = 0; m < R; ++m) row[padi(base + (m << strideLog)) << LES] = x[m];
}

// FFT of the calling wave's rows, bit-reversed order in, natural order out (the register groups of
// fft_rows_wave in reverse order).
__device__ __forceinline__ void fft_rows_wave_dit(double2 *rows, int lrw, int lg, int rowStride, int lane,
                                                  const double2 *__restrict__ tw) {
    const int nst = (lg + 3) >> 2;
    const int baseBits = lg / nst, extra = lg % nst;
    int sl = 0;
    for (int st = nst - 1; st >= 0; --st) {
        const int lr = baseBits + (st < extra ? 1 : 0);
        sl += lr;
        const int lpr = lg - lr;
        const int total = 1 << (lrw + lpr);
        for (int b = lane; b < total; b += 64) {
            double2 *r = rows + (b >> lpr) * rowStride;
            const int bidx = b & ((1 << lpr) - 1);
            switch (lr) {
                case 4: dit_group<4>(r, sl, bidx, lg, tw); break;
                case 3: dit_group<3>(r, sl, bidx, lg, tw); break;
                case 2: dit_group<2>(r, sl, bidx, lg, tw); break;
                default: dit_group<1>(r, sl, bidx, lg, tw); break;
            }
        }
        wave_lds_sync();
    }
}

// Makhoul reordering v[j] = x[2j], v[n-1-j] = x[2j+1] (mirt_dctn.m:71) -- also the output
// reordering of the inverse (mirt_idctn.m:71-73,120).
__device__ __forceinline__ int makhoul(int k, int n) { return (k & 1) ? (n - 1 - (k >> 1)) : (k >> 1); }

template <bool RAWB = false>
__device__ __forceinline__ void fft_rows_wg(double2 *rows, int lrows, int lg, int rowStride, int t, int T,
                                            const double2 *__restrict__ tw) {
    const int nst = (lg + 3) >> 2;
    const int baseBits = lg / nst, extra = lg % nst;
    int sl = lg;
    for (int st = 0; st < nst; ++st) {
        const int lr = baseBits + (st < extra ? 1 : 0);
        const int lpr = lg - lr;
        const int total = 1 << (lrows + lpr);
        for (int b = t; b < total; b += T) {
            double2 *r = rows + (b >> lpr) * rowStride;
            const int bidx = b & ((1 << lpr) - 1);
            switch (lr) {
                case 4: dif_group<4>(r, sl, bidx, lg, tw); break;
                case 3: dif_group<3>(r, sl, bidx, lg, tw); break;
                case 2: dif_group<2>(r, sl, bidx, lg, tw); break;
                default: dif_group<1>(r, sl, bidx, lg, tw); break;
            }
        }
        sl -= lr;
        if (RAWB) lds_barrier(); else __syncthreads();
    }
}

// Decimation-in-time twin of fft_rows_wg: bit-reversed order in, natural order out.
template <bool RAWB = false>
__device__ __forceinline__ void fft_rows_wg_dit(double2 *rows, int lrows, int lg, int rowStride, int t, int T,
                                                const double2 *__restrict__ tw) {
    const int nst = (lg + 3) >> 2;
    const int baseBits = lg / nst, extra = lg % nst;
    int sl = 0;
    for (int st = nst - 1; st >= 0; --st) {
        const int lr = baseBits + (st < extra ? 1 : 0);
        sl += lr;
        const int lpr = lg - lr;
        const int total = 1 << (lrows + lpr);
        for (int b = t; b < total; b += T) {
            double2 *r = rows + (b >> lpr) * rowStride;
            const int bidx = b & ((1 << lpr) - 1);
            switch (lr) {
                case 4: dit_group<4>(r, sl, bidx, lg, tw); break;
                case 3: dit_group<3>(r, sl, bidx, lg, tw); break;
                case 2: dit_group<2>(r, sl, bidx, lg, tw); break;
                default: dit_group<1>(r, sl, bidx, lg, tw); break;
            }
        }
        if (RAWB) lds_barrier(); else __syncthreads();
    }
}

// ---- host side: the dynamic-LDS limit of the kernels built on these rows ----
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
