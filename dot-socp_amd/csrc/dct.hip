// Batched orthonormal DCT-II / DCT-III along one axis of an [n0][n1][n2] fp64 array (n0
// fastest) -- the transforms behind the Neumann-Poisson solve phi = idctn(dctn(rhs) ./ kernel)
// (socp/dot2d/utils/oper_poisson3dim.m:4; mirt_dctn.m:64-141, mirt_idctn.m:59-128).
//
// This file is the dispatcher.  dct_choose_algorithm() picks one of four transform families for a length when its
// plan is made, the plan stores that choice (`alg`) beside the chosen family's own plan, and every launcher below
// switches on it:
//   powers of two                         Makhoul's reordering + FFT in LDS            dct_pow2.hip
//     ... from 4096 (y) / 16384 (x, t) up to 2^20: two-level FFT through a scratch array   dct_long.hip
//   the 2^k+1 grids of the multilevel driver   prime-factor transform                  pfa.hip
//   257 and the other lengths up to 1024  Rader / Bluestein convolution                cdft.hip
//     ... from 4101 (DOTSOCP_CDFT_LONG_MIN) up to 2^19 - 1: Bluestein with a two-level convolution   cdft_long.hip
//   the rest (up to 4100)                 product with the dense DCT matrix            dct_dense.hip
// What is not a transform stays here too: the copy of a length-1 axis and the spectral division.
#include "cdft.h"
#include "dct_families.h"
#include "fft_lds.h"
#include "kernels.h"
#include "pfa.h"

#include <cstdlib>
#include <cstring>

namespace dotsocp {

// smallest length that takes Bluestein by default: the measured crossover against the dense product on both axis kinds
// (profiles/cdft_pass_times.csv); DOTSOCP_CDFT_MIN overrides, never below 48
#define CDFT_DEFAULT_MIN 500

int dct_choose_algorithm(i64 n) {
    static const bool pfa_on = !(getenv("DOTSOCP_PFA") && atoi(getenv("DOTSOCP_PFA")) == 0);
    static const bool cdft_on = !(getenv("DOTSOCP_CDFT") && atoi(getenv("DOTSOCP_CDFT")) == 0);
    static const i64 nb = [] {
        const char *e = getenv("DOTSOCP_CDFT_MIN");
        const i64 v = e ? atoll(e) : CDFT_DEFAULT_MIN;
        return v < 48 ? (i64)48 : v;
    }();
    if (n <= 1) return DCT_ALG_NONE;
    if ((n & (n - 1)) == 0) return DCT_ALG_FFT;
    if (pfa_supported(n)) return pfa_on ? DCT_ALG_PFA : DCT_ALG_DENSE;
    // the two-level convolution first: its switch may claim lengths the LDS convolution or the dense product would serve
    if (cdft_on && n >= cdft_long_min() && n <= CDFT_LONG_MAX_N) return DCT_ALG_BLUESTEIN;
    if (cdft_on && n == 257) return DCT_ALG_RADER;
    if (cdft_on && n >= nb && n <= CDFT_MAX_N) return DCT_ALG_BLUESTEIN;
    return DCT_ALG_DENSE;
}

int cdft_levels(i64 n) {
    const int alg = dct_choose_algorithm(n);
    if (alg == DCT_ALG_RADER) return 1;
    if (alg == DCT_ALG_BLUESTEIN) return n >= cdft_long_min() ? 2 : 1;
    return 0;
}

struct DctPlan {
    i64 n;
    int alg;            // dct_choose_algorithm(n): which one of the plans below exists
    Pow2Plan *pow2;
    PfaPlan *pfa;
    CdftPlan *cdft;
    CdftLongPlan *clong;   // DCT_ALG_BLUESTEIN with cdft_levels(n) == 2, instead of `cdft`
    DensePlan *dense;
};

DctPlan *dct_plan_create(i64 n) {
    DctPlan *p = new DctPlan();
    p->n = n;
    p->alg = dct_choose_algorithm(n);      // reads DOTSOCP_PFA / DOTSOCP_CDFT / DOTSOCP_CDFT_MIN / DOTSOCP_CDFT_LONG_MIN
    bool ok = true;
    switch (p->alg) {
        case DCT_ALG_FFT: ok = (p->pow2 = pow2_plan_create(n)) != nullptr; break;
        // three small tables (pfa.hip) resp. a handful of tables of length n or M = 2^k < 4n (cdft.hip) instead of the
        // n x n matrices of the dense product (16 MB and two million long-double cosines at n = 1025)
        case DCT_ALG_PFA: ok = (p->pfa = pfa_plan_create(n)) != nullptr; break;
        case DCT_ALG_RADER:
        case DCT_ALG_BLUESTEIN:
            if (cdft_levels(n) == 2) ok = (p->clong = cdft_long_plan_create(n)) != nullptr;
            else ok = (p->cdft = cdft_plan_create(n)) != nullptr;
            break;
        case DCT_ALG_DENSE: ok = (p->dense = dense_plan_create(n)) != nullptr; break;
        default: break;                    // n <= 1: nothing to transform
    }
    if (!ok) {
        dct_plan_destroy(p);
        return nullptr;
    }
    return p;
}

void dct_plan_destroy(DctPlan *p) {
    if (!p) return;
    pow2_plan_destroy(p->pow2);
    pfa_plan_destroy(p->pfa);
    cdft_plan_destroy(p->cdft);
    cdft_long_plan_destroy(p->clong);
    dense_plan_destroy(p->dense);
    delete p;
}

bool dct_plan_is_pow2(const DctPlan *p) { return p->alg == DCT_ALG_FFT; }
// (a t length that takes the two-level transform has no fused pass: forward pass, division, inverse pass)
static bool alg_has_tsolve(int alg, i64 n) { return (alg == DCT_ALG_FFT && n < dct_long_min(2)) || alg == DCT_ALG_PFA; }
bool dct_plan_has_tsolve(const DctPlan *p) { return alg_has_tsolve(p->alg, p->n); }

__global__ void __launch_bounds__(256) k_copy(const double *__restrict__ src, double *__restrict__ dst, i64 n) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) dst[i] = src[i];
}

int launch_dct_t_solve(const DctPlan *p, const double *src, double *dst, i64 ny, i64 nplane, i64 line0, i64 nl,
                       i64 nt, double kscale, const double *cy, const double *cx, const double *ct, hipStream_t st,
                       i64 pitch0) {
    if (p->n != nt || !dct_plan_has_tsolve(p)) {
        set_error("fused t-axis solve needs a power-of-two nt inside the LDS or one of the prime-factor lengths");
        return DOTSOCP_EINVAL;
    }
    const bool pitched = pitch0 > ny;
    if (pitched && (line0 != 0 || nl != nplane || nplane % ny != 0)) {
        set_error("fused t-axis solve: pitched rows need whole layers");
        return DOTSOCP_EINVAL;
    }
    if (p->alg == DCT_ALG_FFT)
        return pow2_launch_tsolve(p->pow2, src, dst, ny, nplane, line0, nl, kscale, cy, cx, ct, st, pitch0);
    if (nl <= 0) return 0;
    if (pitched) {
        // whole layers: nx rows of ny lines, rows pitch0 apart, time nodes pitch0 * nx apart
        const i64 nxv = nplane / ny;
        PfaSolveArgs a{kscale, cy, cx, ct, ny, 0, ny};
        return pfa_launch_strided(p->pfa, src, dst, ny, nxv, pitch0, pitch0 * nxv, pitch0, pitch0 * nxv, 2, &a, st);
    }
    PfaSolveArgs a{kscale, cy, cx, ct, ny, line0, 0};
    return pfa_launch_strided(p->pfa, src, dst, nl, 1, 0, nl, 0, nl, 2, &a, st);
}

// the lines of one axis of an [n0][n1][n2] array whose rows are P0 >= n0 doubles apart
static LineMap axis_map(i64 n0, i64 n1, i64 n2, int axis, i64 P0) {
    const i64 dims[3] = {n0, n1, n2};
    const i64 n = dims[axis];
    LineMap map;
    if (P0 == n0) {
        if (axis == 0) { map.nin = 1; map.outerStride = n; map.es = 1; }
        else if (axis == 1) { map.nin = n0; map.outerStride = n0 * n1; map.es = n0; }
        else { map.nin = n0 * n1; map.outerStride = 0; map.es = n0 * n1; }
    } else {
        // (power-of-two lengths: the axis-0 kernels take the line distance as an argument, the strided ones honour map.es)
        if (axis == 0) { map.nin = 1; map.outerStride = P0; map.es = 1; }
        else if (axis == 1) { map.nin = n0; map.outerStride = P0 * n1; map.es = P0; }
        else { map.nin = n0; map.outerStride = P0; map.es = P0 * n1; }
    }
    map.nLines = n0 * n1 * n2 / n;
    return map;
}

int launch_dct_axis(const DctPlan *p, const double *src, double *dst, i64 n0, i64 n1, i64 n2, int axis, int inverse,
                    hipStream_t st, i64 pitch0) {
    const i64 P0 = pitch0 > n0 ? pitch0 : n0;           // row pitch of both arrays
    const i64 dims[3] = {n0, n1, n2};
    const i64 n = dims[axis];
    const i64 total = n0 * n1 * n2;
    if (total <= 0) return 0;
    if (n != p->n) {
        set_error("dct plan length mismatch (%lld vs %lld)", (long long)n, (long long)p->n);
        return DOTSOCP_EINVAL;
    }
    if (n == 1) {
        const i64 all = P0 * n1 * n2;                     // pad entries travel with the rows
        if (src != dst)
            DS_KLAUNCH(k_copy, dim3(launch_blocks(all, 256, 1 << 14)), dim3(256), 0, st, src, dst, all);
        DS_HIP(hipGetLastError());
        return 0;
    }
    const LineMap map = axis_map(n0, n1, n2, axis, P0);
    switch (p->alg) {
        case DCT_ALG_FFT:
            if (axis == 0) return pow2_launch_axis0(p->pow2, src, dst, map, inverse, st);
            return pow2_launch_strided(p->pow2, src, dst, map, inverse, st);
        case DCT_ALG_PFA:
            if (axis == 0) return pfa_launch_axis0(p->pfa, src, dst, map.nLines, P0, P0, inverse, st);
            if (axis == 1) return pfa_launch_strided(p->pfa, src, dst, n0, n2, P0 * n1, P0, P0 * n1, P0, inverse ? 1 : 0, nullptr, st);
            return pfa_launch_strided(p->pfa, src, dst, n0, n1, P0, P0 * n1, P0, P0 * n1, inverse ? 1 : 0, nullptr, st);
        case DCT_ALG_RADER:
        case DCT_ALG_BLUESTEIN:
            if (p->clong) return cdft_long_launch(p->clong, src, dst, map, axis == 0, inverse, st);
            return cdft_launch(p->cdft, src, dst, map, axis == 0, inverse, st);
        case DCT_ALG_DENSE: return dense_launch(p->dense, src, dst, map, axis == 0, inverse, st);
        default: set_error("dct plan of length %lld has no transform", (long long)p->n); return DOTSOCP_EINVAL;
    }
}

// data ./= kscale * ((CY[ky] + CX[kx]) + CT[kt]) with the zero eigenvalue replaced by 1
// (initialize_FFTkernel.m:6-15, solver_socp_inPALM.m:96).
__global__ void __launch_bounds__(256) k_spectral_divide(double *__restrict__ data, i64 ny, i64 py, i64 nxl, i64 nt, i64 x0,
                                                          double kscale, const double *__restrict__ cy,
                                                          const double *__restrict__ cx,
                                                          const double *__restrict__ ct) {
    const i64 y = (i64)blockIdx.x * 64 + threadIdx.x;
    const i64 x = (i64)blockIdx.y * 4 + threadIdx.y;
    const i64 t = blockIdx.z;
    if (y >= ny || x >= nxl) return;
    double lam = (cy[y] + cx[x0 + x]) + ct[t];
    if (lam == 0.0) lam = 1.0;
    const i64 i = y + py * (x + nxl * t);
    data[i] = data[i] / (kscale * lam);
}

__global__ void __launch_bounds__(256) k_spectral_divide_pencil(double *__restrict__ data, i64 ny, i64 line0, i64 nl,
                                                                 i64 nt, double kscale, const double *__restrict__ cy,
                                                                 const double *__restrict__ cx,
                                                                 const double *__restrict__ ct) {
    const i64 L = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 t = blockIdx.y;
    if (L >= nl) return;
    const i64 G = line0 + L;
    double lam = (cy[G % ny] + cx[G / ny]) + ct[t];
    if (lam == 0.0) lam = 1.0;
    data[L + nl * t] = data[L + nl * t] / (kscale * lam);
}

int launch_spectral_divide_pencil(double *data, i64 ny, i64 line0, i64 nl, i64 nt, double kscale, const double *cy,
                                  const double *cx, const double *ct, hipStream_t st) {
    if (nl * nt <= 0) return 0;
    dim3 grid((unsigned)((nl + 255) / 256), (unsigned)nt);
    DS_KLAUNCH(k_spectral_divide_pencil, grid, dim3(256), 0, st, data, ny, line0, nl, nt, kscale, cy, cx, ct);
    DS_HIP(hipGetLastError());
    return 0;
}

int launch_spectral_divide(double *data, i64 ny, i64 nt, i64 x0, i64 nxl, double kscale, const double *cy,
                           const double *cx, const double *ct, hipStream_t st, i64 pitch0) {
    if (ny * nxl * nt <= 0) return 0;
    dim3 grid((unsigned)((ny + 63) / 64), (unsigned)((nxl + 3) / 4), (unsigned)nt);
    DS_KLAUNCH(k_spectral_divide, grid, dim3(64, 4), 0, st, data, ny, pitch0 > ny ? pitch0 : ny, nxl, nt, x0, kscale, cy, cx, ct);
    DS_HIP(hipGetLastError());
    return 0;
}

bool tsolve_tri_allowed() {
    const char *e = getenv("DOTSOCP_TSOLVE");          // read per call: the tests switch it inside one process
    return !(e && strcmp(e, "dct") == 0);
}

// The alternatives of the single slab's t step, from the transform family of nt and the shape (pure host arithmetic):
// launch_poisson_t_single switches on it, poisson_t_kind (dotsocp_tsolve_kernel) refines the same answer by kernel.
enum { TS_TRI, TS_FUSED, TS_THREE };
static int choose_t_single(int alg, i64 ny, i64 nx, i64 nt, i64 plane, bool allow_tri, int ncu) {
    if (allow_tri && tsolve_tri_preferred(nt, alg == DCT_ALG_FFT, plane, ncu) && tsolve_tri_safe(ny, nx, nt)) return TS_TRI;
    return alg_has_tsolve(alg, nt) ? TS_FUSED : TS_THREE;
}

int launch_poisson_t_single(const DctPlan *pt, const Grid &g, double kscale, const double *cy, const double *cx,
                            const double *ct, double *p, double *p2, i64 pitch0, hipStream_t st, bool allow_tri) {
    const i64 ny = g.ny, nx = g.nx, nt = g.nt;
    switch (choose_t_single(pt->alg, ny, nx, nt, g.plane, allow_tri, device_cus())) {
        case TS_TRI:
            // no transform along t: the (ky, kx) modes are tridiagonal systems in t (tri.hip: k_tsolve_single / _pipe)
            return launch_tsolve_tri(g, nt, kscale, cy, cx, p, st);
        case TS_FUSED:
            return launch_dct_t_solve(pt, p, p, ny, ny * nx, 0, ny * nx, nt, kscale, cy, cx, ct, st, pitch0);
        default:
            DS_CHECK(launch_dct_axis(pt, p, p2, ny, nx, nt, 2, 0, st, pitch0));
            DS_CHECK(launch_spectral_divide(p2, ny, nt, 0, nx, kscale, cy, cx, ct, st, pitch0));
            return launch_dct_axis(pt, p2, p, ny, nx, nt, 2, 1, st, pitch0);
    }
}

int dct_pass_kind(i64 n0, i64 n1, i64 n2, int axis, i64 pitch0, int ncu) {
    const i64 dims[3] = {n0, n1, n2};
    const i64 n = dims[axis];
    if (n <= 1) return DOTSOCP_PASS_NONE;
    if (dct_choose_algorithm(n) != DCT_ALG_FFT) return DOTSOCP_PASS_OTHER;
    return pow2_pass_kind(n, axis_map(n0, n1, n2, axis, pitch0 > n0 ? pitch0 : n0), axis == 0, ncu);
}

int poisson_t_kind(i64 ny, i64 nx, i64 nt, i64 pitch0, bool allow_tri, int ncu) {
    const i64 py = pitch0 > ny ? pitch0 : ny;
    const int alg = dct_choose_algorithm(nt);
    switch (choose_t_single(alg, ny, nx, nt, py * nx, allow_tri, ncu)) {
        case TS_TRI: return tsolve_tri_pipelined(nt, py * nx, ncu) ? DOTSOCP_TSOLVE_TRI_PIPE : DOTSOCP_TSOLVE_TRI;
        case TS_FUSED:
            if (alg != DCT_ALG_FFT) return DOTSOCP_TSOLVE_FUSED_PFA;
            return pow2_tsolve_pipelined(nt, ny, ny * nx, 0, ny * nx, pitch0, ncu) ? DOTSOCP_TSOLVE_FUSED_PIPE
                                                                                   : DOTSOCP_TSOLVE_FUSED;
        default: return DOTSOCP_TSOLVE_PASSES;
    }
}

}  // namespace dotsocp
