// The dense family of the DCT dispatcher (dct.hip): the lengths that have no fast transform -- below the Bluestein
// crossover, above 1024, or with DOTSOCP_PFA=0 / DOTSOCP_CDFT=0 -- as the product with the n x n DCT matrix (exact,
// O(n^2) per line): on the fp64 matrix cores from 48 points and 64 lines on, a plain LDS-tiled product below.
#include "dct_families.h"
#include "device_utils.h"
#include "fft_lds.h"
#include "kernels.h"

#include <cmath>
#include <vector>

namespace dotsocp {

#define DENSE_SPLIT_MIN 48    // shortest length that gets the even / odd matrices of k_dct_mfma_split

struct DensePlan {
    i64 n;
    double *Cfwd;   // Cfwd[j*n + k] = C[k][j]   (forward,  out_k = sum_j C[k][j] in_j)
    double *Cinv;   // Cinv[j*n + k] = C[j][k]   (inverse)
    // even / odd split of the matrix (k_dct_mfma_split, n >= DENSE_SPLIT_MIN), [contraction index][output index]:
    double *Ef, *Of;   // Ef[j*ne + k'] = C[2k'][j] (j < njE), Of[j*no + k'] = C[2k'+1][j] (j < h)
    double *Ei, *Oi;   // Ei[k'*njE + j] = C[2k'][j],          Oi[k'*h + j]  = C[2k'+1][j]
    int ne, no, h, njE;
};

DensePlan *dense_plan_create(i64 n) {
    DensePlan *p = new DensePlan();
    p->n = n;
    p->Cfwd = p->Cinv = nullptr;
    p->Ef = p->Of = p->Ei = p->Oi = nullptr;
    p->ne = p->no = p->h = p->njE = 0;
    const long double PI = 3.141592653589793238462643383279502884L;
    std::vector<double> cf((size_t)n * n), ci((size_t)n * n);
    for (i64 k = 0; k < n; ++k) {
        long double sc = sqrtl(2.0L / (long double)n);
        if (k == 0) sc /= sqrtl(2.0L);
        for (i64 j = 0; j < n; ++j) {
            // reduce the argument exactly: cos(pi * m / (2n)) with m = (2j+1) k mod 4n
            i64 m = ((2 * j + 1) * k) % (4 * n);
            double v = (double)(sc * cosl(PI * (long double)m / (2.0L * (long double)n)));
            cf[(size_t)j * n + k] = v;   // C[k][j] stored with k contiguous
            ci[(size_t)k * n + j] = v;   // C[k][j] stored with j contiguous: inverse out_j = sum_k C[k][j] X_k
        }
    }
    if (hipMalloc(&p->Cfwd, sizeof(double) * n * n) != hipSuccess ||
        hipMalloc(&p->Cinv, sizeof(double) * n * n) != hipSuccess) {
        dense_plan_destroy(p);
        return nullptr;
    }
    (void)hipMemcpy(p->Cfwd, cf.data(), sizeof(double) * n * n, hipMemcpyHostToDevice);
    (void)hipMemcpy(p->Cinv, ci.data(), sizeof(double) * n * n, hipMemcpyHostToDevice);
    if (n >= DENSE_SPLIT_MIN) {
        const int h = (int)(n / 2), ne = (int)((n + 1) / 2), no = (int)(n / 2), njE = h + (int)(n & 1);
        p->ne = ne; p->no = no; p->h = h; p->njE = njE;
        auto Cm = [&](i64 k, i64 j) { return cf[(size_t)j * n + k]; };
        std::vector<double> ef((size_t)njE * ne), of((size_t)h * no), ei((size_t)ne * njE), oi((size_t)no * h);
        for (int j = 0; j < njE; ++j)
            for (int k = 0; k < ne; ++k) ef[(size_t)j * ne + k] = ei[(size_t)k * njE + j] = Cm(2 * k, j);
        for (int j = 0; j < h; ++j)
            for (int k = 0; k < no; ++k) of[(size_t)j * no + k] = oi[(size_t)k * h + j] = Cm(2 * k + 1, j);
        double **dst4[4] = {&p->Ef, &p->Of, &p->Ei, &p->Oi};
        std::vector<double> *src4[4] = {&ef, &of, &ei, &oi};
        for (int i = 0; i < 4; ++i) {
            if (hipMalloc(dst4[i], sizeof(double) * src4[i]->size()) != hipSuccess) {
                dense_plan_destroy(p);
                return nullptr;
            }
            (void)hipMemcpy(*dst4[i], src4[i]->data(), sizeof(double) * src4[i]->size(), hipMemcpyHostToDevice);
        }
    }
    return p;
}

void dense_plan_destroy(DensePlan *p) {
    if (!p) return;
    double *tables[6] = {p->Cfwd, p->Cinv, p->Ef, p->Of, p->Ei, p->Oi};
    for (double *t : tables)
        if (t) (void)hipFree(t);
    delete p;
}

// Short lengths or few lines: out_k = sum_j M[j*n + k] in_j.  A workgroup stages TL lines in
// LDS and produces the outputs k in [blockIdx.y * KC, +KC) of each of them.
//   axis 0 (lines contiguous):  thread <-> k, accumulating all TL lines per load of M (M is read once
//                               per TL lines);  KC = 256
//   strided axes (LINE_FAST):   thread <-> (line, k) with the line index fastest so that global
//                               accesses stay coalesced;  KC = 256 / TL
#define DENSE_TL 8
template <bool LINE_FAST>
__global__ void __launch_bounds__(DCT_THREADS) k_dct_dense(const double *__restrict__ src, double *__restrict__ dst,
                                                            LineMap map, int n, int TL,
                                                            const double *__restrict__ M) {
    extern __shared__ double2 buf[];
    double *tile = (double *)buf;   // [TL][n]
    const i64 L0 = (i64)blockIdx.x * TL;
    const int total = TL * n;
    for (int e = threadIdx.x; e < total; e += DCT_THREADS) {
        int l, k;
        if (LINE_FAST) { l = e % TL; k = e / TL; } else { k = e % n; l = e / n; }
        const i64 L = L0 + l;
        tile[l * n + k] = (L < map.nLines) ? src[map.addr(L, k)] : 0.0;
    }
    __syncthreads();
    if (LINE_FAST) {
        const int KC = DCT_THREADS / TL;
        const int l = threadIdx.x % TL, k = blockIdx.y * KC + threadIdx.x / TL;
        const i64 L = L0 + l;
        if (k >= n || L >= map.nLines) return;
        const double *in = tile + l * n;
        double acc = 0.0;
#pragma unroll 4
        for (int j = 0; j < n; ++j) acc += M[(i64)j * n + k] * in[j];
        dst[map.addr(L, k)] = acc;
    } else {
        const int k = blockIdx.y * DCT_THREADS + threadIdx.x;
        if (k >= n) return;
        double acc[DENSE_TL];
#pragma unroll
        for (int l = 0; l < DENSE_TL; ++l) acc[l] = 0.0;
#pragma unroll 2
        for (int j = 0; j < n; ++j) {
            const double m = M[(i64)j * n + k];
#pragma unroll
            for (int l = 0; l < DENSE_TL; ++l)
                if (l < TL) acc[l] += m * tile[l * n + j];
        }
#pragma unroll
        for (int l = 0; l < DENSE_TL; ++l)
            if (l < TL && L0 + l < map.nLines) dst[map.addr(L0 + l, k)] = acc[l];
    }
}


// ---------------------------------------------------------------------------------------------
// Dense lengths on the fp64 matrix cores.  Along a non-power-of-two axis the transform is the product of the
// n x n DCT matrix with the lines, out_l[k] = sum_j M[k][j] in_l[j]: v_mfma_f64_16x16x4_f64 tiles, a workgroup
// computes 64 outputs k of 128 lines, its four waves 64 k x 32 lines each (4 x 2 accumulator tiles), the j
// range streamed through LDS in double-buffered chunks of 8 (16: fewer barriers but half the resident workgroups,
// 27.0 vs 24.3 ms per 1025^2 x 129 Poisson solve) (next chunk's global loads in flight in registers
// during the MFMAs, one barrier per chunk).  M is staged as [j][k] (k contiguous, as stored); the lines as
// [j][line] on the strided axes (lines consecutive in memory) and as [line][j] on axis 0 (j contiguous in memory),
// so that global loads, LDS fragment reads (row strides 16 mod 32 doubles / 18 doubles: conflict-free) and the
// stores of the 16 x 16 result tiles (16 consecutive addresses per row) are all coalesced.
//   strided axes: D[k][line] = M . X      a = M fragment, b = line fragment
//   axis 0      : D[line][k] = X' . M'    a = line fragment, b = M fragment
// Operand / result lane maps of the f64 MFMA: a: A[lane & 15][lane >> 4], b: B[lane >> 4][lane & 15],
// d[r]: D[(lane >> 4) + 4 r][lane & 15]   (cdna_hip_programming.md, fragment layout).
// ---------------------------------------------------------------------------------------------
typedef double mf_double4 __attribute__((ext_vector_type(4)));
#define MF_KT 64
#define MF_LT 128
#define MF_MS (MF_KT + 16)
#define MF_XS (MF_LT + 16)      // strided axes: [j][line]


// Even / odd split of the dense transform: C[k][n-1-j] = (-1)^k C[k][j], so with h = floor(n/2)
//   forward:  X[2k']   = sum_{j<h} C[2k'][j]   (x[j] + x[n-1-j])  (+ C[2k'][h] x[h] for odd n)
//             X[2k'+1] = sum_{j<h} C[2k'+1][j] (x[j] - x[n-1-j])
//   inverse:  E[j] = sum_k' C[2k'][j] X[2k'], O[j] = sum_k' C[2k'+1][j] X[2k'+1],  x[j] = E + O, x[n-1-j] = E - O
// -- half the multiply-adds of the full product.  The tiling is the one described above; the forward kernel forms the sums /
// differences while staging the lines (parity = blockIdx.z), the inverse kernel keeps two accumulator sets
// (E, O) per tile of j <= h and writes both mirror images.  Matrices (DensePlan): Ef, Of stored [j][k'] (k'
// contiguous), Ei, Oi stored [k'][j] (j contiguous) -- always [contraction index][output index].
struct SplitArgs {
    const double *Me, *Mo;
    int ne, no, h, njE;       // even / odd k counts, floor(n/2), h + (n odd ? 1 : 0)
    int xcd;                  // XCD-aware tile order
};

template <bool AXIS0, int MF_KC, bool INV>
__global__ void __launch_bounds__(256) k_dct_mfma_split(const double *__restrict__ src, double *__restrict__ dst,
                                                         LineMap map, int n, SplitArgs sp) {
    constexpr int MF_XZ = MF_KC + 2;
    constexpr int XSZ = (MF_KC * MF_XS > MF_LT * MF_XZ) ? MF_KC * MF_XS : MF_LT * MF_XZ;
    constexpr int NPH = INV ? 2 : 1;
    __shared__ double Ms[2][MF_KC * MF_MS];
    __shared__ double Xs[2][XSZ];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // the output tiles that share a line tile run back to back on ONE XCD (xcd_tile), so that the lines come
    // from that XCD's L2 for all but the first of them
    const i64 P = sp.xcd ? xcd_tile(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y)
                         : (i64)blockIdx.x + (i64)gridDim.x * blockIdx.y;
    const int o0 = (int)(P % gridDim.x) * MF_KT;       // first output index of the tile (k' forward, j inverse)
    const i64 L0 = (P / gridDim.x) * MF_LT;
    const int li = lane & 15, lh = lane >> 4;
    mf_double4 acc[NPH][4][2];
#pragma unroll
    for (int ph = 0; ph < NPH; ++ph)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[ph][a][b] = (mf_double4){0.0, 0.0, 0.0, 0.0};
    constexpr int MU = MF_KC / 4, XU = MF_KC / 2, ZSTEP = 256 / MF_KC;
    double mreg[MU], xreg[XU];
    const int m_oo = tid & 63, m_cc = tid >> 6;
    const int x_ll = AXIS0 ? (tid / MF_KC) : (tid & 127);
    const int x_cc = AXIS0 ? (tid % MF_KC) : (tid >> 7);
    i64 xbase = 0;
    bool x_ok = false;
    if (!AXIS0) {
        x_ok = (L0 + x_ll) < map.nLines;
        xbase = x_ok ? map.base(L0 + x_ll) : 0;
    }
    auto at = [&](i64 L, i64 lbase, int j) { return AXIS0 ? src[L * map.outerStride + j] : src[lbase + (i64)j * map.es]; };
#pragma unroll
    for (int ph = 0; ph < NPH; ++ph) {
        const int par = INV ? ph : (int)blockIdx.z;               // 0: even part, 1: odd part
        const double *__restrict__ M = par ? sp.Mo : sp.Me;
        const int ld = INV ? (par ? sp.h : sp.njE) : (par ? sp.no : sp.ne);         // output indices the matrix holds
        const int ncontr = INV ? (par ? sp.no : sp.ne) : (par ? sp.h : sp.njE);
        const bool m_ok = (o0 + m_oo) < ld;
        // the contraction element c of a line: forward x[c] +- x[n-1-c] (the middle one alone), inverse x[2c + par]
        auto elem = [&](i64 L, i64 lbase, int c) {
            if (INV) return at(L, lbase, 2 * c + par);
            if (c >= sp.h) return at(L, lbase, c);                // c == h: middle element of an odd length (even part)
            const double u = at(L, lbase, c), v = at(L, lbase, n - 1 - c);
            return par ? u - v : u + v;
        };
        auto fetch = [&](int c0) {
#pragma unroll
            for (int u = 0; u < MU; ++u) {
                const int c = c0 + m_cc + 4 * u;
                mreg[u] = (m_ok && c < ncontr) ? M[(i64)c * ld + o0 + m_oo] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < XU; ++u) {
                if (AXIS0) {
                    const i64 L = L0 + x_ll + ZSTEP * u;
                    const int c = c0 + x_cc;
                    xreg[u] = (L < map.nLines && c < ncontr) ? elem(L, 0, c) : 0.0;
                } else {
                    const int c = c0 + x_cc + 2 * u;
                    xreg[u] = (x_ok && c < ncontr) ? elem(0, xbase, c) : 0.0;
                }
            }
        };
        auto stash = [&](int buf) {
#pragma unroll
            for (int u = 0; u < MU; ++u) Ms[buf][(m_cc + 4 * u) * MF_MS + m_oo] = mreg[u];
#pragma unroll
            for (int u = 0; u < XU; ++u) {
                if (AXIS0) Xs[buf][(x_ll + ZSTEP * u) * MF_XZ + x_cc] = xreg[u];
                else Xs[buf][(x_cc + 2 * u) * MF_XS + x_ll] = xreg[u];
            }
        };
        const int nch = (ncontr + MF_KC - 1) / MF_KC;
        fetch(0);
        stash(0);
        __syncthreads();
        for (int c = 0; c < nch; ++c) {
            const int buf = c & 1;
            if (c + 1 < nch) fetch((c + 1) * MF_KC);
#pragma unroll
            for (int kk = 0; kk < MF_KC; kk += 4) {
                double mf[4], xf[2];
#pragma unroll
                for (int a = 0; a < 4; ++a) mf[a] = Ms[buf][(kk + lh) * MF_MS + a * 16 + li];
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    xf[b] = AXIS0 ? Xs[buf][(wave * 32 + b * 16 + li) * MF_XZ + kk + lh]
                                  : Xs[buf][(kk + lh) * MF_XS + wave * 32 + b * 16 + li];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        acc[ph][a][b] = AXIS0 ? __builtin_amdgcn_mfma_f64_16x16x4f64(xf[b], mf[a], acc[ph][a][b], 0, 0, 0)
                                              : __builtin_amdgcn_mfma_f64_16x16x4f64(mf[a], xf[b], acc[ph][a][b], 0, 0, 0);
            }
            if (c + 1 < nch) stash(buf ^ 1);
            __syncthreads();
        }
    }
    // ---- store ----
    const int nout = INV ? sp.njE : (blockIdx.z ? sp.no : sp.ne);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = o0 + a * 16 + (AXIS0 ? li : lh + 4 * r);
                const i64 L = L0 + wave * 32 + b * 16 + (AXIS0 ? lh + 4 * r : li);
                if (o >= nout || L >= map.nLines) continue;
                const i64 lbase = AXIS0 ? L * map.outerStride : map.base(L);
                const i64 es = map.es;
                if (!INV) {
                    dst[lbase + (i64)(2 * o + (int)blockIdx.z) * es] = acc[0][a][b][r];
                } else {
                    const double E = acc[0][a][b][r], O = acc[NPH - 1][a][b][r];
                    dst[lbase + (i64)o * es] = E + O;
                    if (o < sp.h) dst[lbase + (i64)(n - 1 - o) * es] = E - O;
                }
            }
}

int dense_launch(const DensePlan *p, const double *src, double *dst, const LineMap &map, bool axis0, int inverse,
                 hipStream_t st) {
    const i64 n = p->n;
    if (src == dst) {
        set_error("dense DCT path needs distinct src/dst");
        return DOTSOCP_EINVAL;
    }
    if (n >= DENSE_SPLIT_MIN && map.nLines >= 64) {
        SplitArgs sp{inverse ? p->Ei : p->Ef, inverse ? p->Oi : p->Of, p->ne, p->no, p->h, p->njE, 1};
        const unsigned lt = (unsigned)((map.nLines + MF_LT - 1) / MF_LT);
        if (inverse) {
            dim3 grid((unsigned)((p->njE + MF_KT - 1) / MF_KT), lt, 1);
            if (axis0) DS_KLAUNCH((k_dct_mfma_split<true, 8, true>), grid, dim3(256), 0, st, src, dst, map, (int)n, sp);
            else DS_KLAUNCH((k_dct_mfma_split<false, 8, true>), grid, dim3(256), 0, st, src, dst, map, (int)n, sp);
        } else {
            dim3 grid((unsigned)((p->ne + MF_KT - 1) / MF_KT), lt, 2);
            if (axis0) DS_KLAUNCH((k_dct_mfma_split<true, 8, false>), grid, dim3(256), 0, st, src, dst, map, (int)n, sp);
            else DS_KLAUNCH((k_dct_mfma_split<false, 8, false>), grid, dim3(256), 0, st, src, dst, map, (int)n, sp);
        }
        DS_HIP(hipGetLastError());
        return 0;
    }
    int TL = DENSE_TL;
    while (TL > 1 && (size_t)TL * n * sizeof(double) > 65536) TL >>= 1;
    while (TL > 1 && map.nLines < (i64)TL * 64) TL >>= 1;      // few lines: favour more workgroups
    const size_t lds = (size_t)TL * n * sizeof(double);
    const unsigned bx = (unsigned)((map.nLines + TL - 1) / TL);
    const double *M = inverse ? p->Cinv : p->Cfwd;
    if (!axis0) {
        const int KC = DCT_THREADS / TL;
        DS_KLAUNCH((k_dct_dense<true>), dim3(bx, (unsigned)((n + KC - 1) / KC)), dim3(DCT_THREADS), lds, st, src,
                           dst, map, (int)n, TL, M);
    } else {
        DS_KLAUNCH((k_dct_dense<false>), dim3(bx, (unsigned)((n + DCT_THREADS - 1) / DCT_THREADS)),
                           dim3(DCT_THREADS), lds, st, src, dst, map, (int)n, TL, M);
    }
    DS_HIP(hipGetLastError());
    return 0;
}

}  // namespace dotsocp
