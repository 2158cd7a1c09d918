// The weight pyramid of the weighted multilevel driver on the device (weights.h, include/dotsocp.h: dotsocp_weights_*).
//   * k_weight_restrict: socp/wdot2d/utils/downSample_q.m:4-21 and downSample_barrier.m:4-21 -- the Kronecker product of
//     three 1-D restrictions (P ./ sum(P, 1))' of gene_prolongMat1dim_linear / _nearest, applied as the stencil it is:
//         linear   nodes 2m+1 -> m+1   (1/4, 1/2, 1/4), at both ends (2/3, 1/3)
//         nearest  edges 2m   -> m     (1/2, 1/2)
//     q0: linear in y and x, nearest in t;  bx: nearest in x, linear in y and t;  by: nearest in y, linear in x and t.
//     The barrier variant restricts log(w) and stores exp of the result.
//   * k_weight_space: examples/wdot2d/get_weight_by_barrier.m:20-33 -- two 2-D arrays repeated over t, ones on the time edges.
//   * k_weight_log10_sum / _final: the sum behind `adjust` of InitialScaling (solver_wdotsocp2d.m:312-316), in a fixed order.
// Index order as everywhere: y fastest, then x, then t.  A pyramid level is stored in the reference layout (unpitched).
#include <algorithm>

#include "device_utils.h"
#include "weights.h"

namespace dotsocp {

namespace {

// two neighbouring doubles of a row; rows of 2^k + 1 doubles start on odd multiples of 8 bytes
struct __attribute__((aligned(8))) Pair {
    double a, b;
};

__device__ __forceinline__ i64 clampi(i64 v, i64 lo, i64 hi) { return v < lo ? lo : (v > hi ? hi : v); }

// coarse node i of a linear axis from the fine nodes 2i - 1, 2i, 2i + 1.  All three are always loaded (from clamped
// addresses, DESIGN.md section 3 "loads must leave together"); at an end the one outside the axis is not used.
__device__ __forceinline__ double lin3(double prev, double own, double next, bool first, bool last) {
    const double nb = first ? next : prev;
    const double e = (2.0 / 3.0) * own + (1.0 / 3.0) * nb;
    const double m = 0.25 * prev + 0.5 * own + 0.25 * next;
    return (first || last) ? e : m;
}

constexpr int WR_XC = 8;                  // coarse x per workgroup
constexpr int WR_ROWS = 2 * WR_XC + 1;    // fine x rows they are made of (linear: 2 j0 - 1 .. 2 (j0 + XC - 1) + 1)

}  // namespace

// One component.  Fine (n0, n1, n2) -> coarse (m0, m1, m2); YL / XL / TL: the axis is linear (else nearest).
// y is on the lanes: a lane holds the fine entries 2i, 2i + 1 of its coarse i (one 16-byte load) and gets 2i - 1 from the
// lane below, so a wave reads whole cache lines; on a linear y axis lane 0 only serves its neighbour (63 coarse y per wave).
// A workgroup makes WR_XC coarse x of one coarse t: every fine x row it needs is loaded at its two or three fine t,
// restricted along y and t by one wave and left in LDS -- a fine row shared by two coarse x is loaded, and its logarithm
// taken, once -- and the x restriction then reads the LDS rows.
template <bool LOG, bool YL, bool XL, bool TL>
__global__ void __launch_bounds__(256) k_weight_restrict(const double *__restrict__ f, double *__restrict__ c, i64 n0, i64 n1,
                                                          i64 n2, i64 m0, i64 m1, i64 m2) {
    __shared__ double rows[WR_ROWS][64];
    constexpr int YW = YL ? 63 : 64;
    constexpr int NT = TL ? 3 : 2;
    constexpr int NR = XL ? WR_ROWS : 2 * WR_XC;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const i64 i = (i64)blockIdx.x * YW + lane - (YL ? 1 : 0);
    const i64 j0 = (i64)blockIdx.y * WR_XC;
    const i64 k = blockIdx.z;
    const i64 ys = clampi(2 * i, 0, n0 - 2);       // the pair (ys, ys + 1) is always inside the row
    const bool ytop = 2 * i > n0 - 2;              // last node of a linear axis: the pair is (2i - 1, 2i)
    const i64 xb = 2 * j0 - (XL ? 1 : 0), tb = 2 * k - (TL ? 1 : 0);
    for (int r = wv; r < NR; r += 4) {
        const i64 x = clampi(xb + r, 0, n1 - 1);
        Pair p[NT];
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
            const i64 t = clampi(tb + tt, 0, n2 - 1);
            p[tt] = *reinterpret_cast<const Pair *>(f + (n0 * (x + n1 * t) + ys));
        }
        double v[NT];
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
            double a = p[tt].a, b = p[tt].b;
            if (LOG) { a = log(a); b = log(b); }
            if (YL) {
                const double prev = __shfl_up(b, 1, 64);
                v[tt] = lin3(prev, ytop ? b : a, b, i == 0, ytop);
            } else {
                v[tt] = 0.5 * a + 0.5 * b;
            }
        }
        rows[r][lane] = TL ? lin3(v[0], v[1], v[NT - 1], k == 0, k == m2 - 1) : 0.5 * v[0] + 0.5 * v[1];
    }
    __syncthreads();
    if (i < 0 || i >= m0 || (YL && lane == 0)) return;
    for (int jj = wv; jj < WR_XC; jj += 4) {
        const i64 j = j0 + jj;
        if (j >= m1) break;
        double v;
        if (XL) v = lin3(rows[2 * jj][lane], rows[2 * jj + 1][lane], rows[2 * jj + 2][lane], j == 0, j == m1 - 1);
        else v = 0.5 * rows[2 * jj][lane] + 0.5 * rows[2 * jj + 1][lane];
        if (LOG) v = exp(v);
        c[i + m0 * (j + m1 * k)] = v;
    }
}

template <bool LOG, bool YL, bool XL, bool TL>
static int restrict_component(const double *f, double *c, i64 n0, i64 n1, i64 n2, hipStream_t st) {
    const i64 m0 = YL ? (n0 + 1) / 2 : n0 / 2, m1 = XL ? (n1 + 1) / 2 : n1 / 2, m2 = TL ? (n2 + 1) / 2 : n2 / 2;
    const i64 yw = YL ? 63 : 64;
    DS_ARG(m2 <= 65535 && (m1 + WR_XC - 1) / WR_XC <= 65535, "weight pyramid: axis too long for one launch");
    dim3 grid((unsigned)((m0 + yw - 1) / yw), (unsigned)((m1 + WR_XC - 1) / WR_XC), (unsigned)m2);
    DS_KLAUNCH((k_weight_restrict<LOG, YL, XL, TL>), grid, dim3(256), 0, st, f, c, n0, n1, n2, m0, m1, m2);
    DS_HIP(hipGetLastError());
    return 0;
}

// blockIdx.y = time node t: the cell layer t of q0 (t < nt - 1) and the node layers t of bx and by
__global__ void __launch_bounds__(256) k_weight_space(double *__restrict__ w, const double *__restrict__ wX,
                                                       const double *__restrict__ wY, i64 ny, i64 nx, i64 nt) {
    const i64 t = blockIdx.y;
    const i64 plane = ny * nx, bxl = ny * (nx - 1), byl = (ny - 1) * nx;
    double *q0 = w + plane * t, *bx = w + plane * (nt - 1) + bxl * t, *by = w + plane * (nt - 1) + bxl * nt + byl * t;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < plane; e += (i64)gridDim.x * blockDim.x) {
        if (t < nt - 1) q0[e] = 1.0;
        if (e < bxl) bx[e] = wX[e];
        if (e < byl) by[e] = wY[e];
    }
}

// Fixed-order sum of log10(w + 1e-10) in two levels, like k_kkt_final: block b adds its own contiguous piece (every
// thread its strided entries, then a tree over the 256 threads), one more workgroup adds the blocks' sums.
__global__ void __launch_bounds__(256) k_weight_log10_sum(const double *__restrict__ w, i64 n, double *__restrict__ partials) {
    const i64 per = (n + gridDim.x - 1) / gridDim.x;
    const i64 e0 = (i64)blockIdx.x * per, e1 = (e0 + per < n) ? e0 + per : n;
    double v = 0.0;
    for (i64 e = e0 + threadIdx.x; e < e1; e += 256) v += log10(w[e] + 1e-10);
    __shared__ double red[256];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(256) k_weight_log10_final(double *__restrict__ partials, int nblocks) {
    double v = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) v += partials[b];
    __shared__ double red[256];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[nblocks] = red[0];
}

int launch_weight_restrict(const double *fine, double *coarse, i64 ny, i64 nx, i64 nt, bool log_mean, hipStream_t st) {
    const i64 my = (ny + 1) / 2, mx = (nx + 1) / 2, mt = (nt + 1) / 2;
    const i64 bxF = ny * nx * (nt - 1), byF = bxF + ny * (nx - 1) * nt;
    const i64 bxC = my * mx * (mt - 1), byC = bxC + my * (mx - 1) * mt;
    if (log_mean) {
        DS_CHECK((restrict_component<true, true, true, false>(fine, coarse, ny, nx, nt - 1, st)));
        DS_CHECK((restrict_component<true, true, false, true>(fine + bxF, coarse + bxC, ny, nx - 1, nt, st)));
        DS_CHECK((restrict_component<true, false, true, true>(fine + byF, coarse + byC, ny - 1, nx, nt, st)));
    } else {
        DS_CHECK((restrict_component<false, true, true, false>(fine, coarse, ny, nx, nt - 1, st)));
        DS_CHECK((restrict_component<false, true, false, true>(fine + bxF, coarse + bxC, ny, nx - 1, nt, st)));
        DS_CHECK((restrict_component<false, false, true, true>(fine + byF, coarse + byC, ny - 1, nx, nt, st)));
    }
    return 0;
}

int launch_weight_space(double *w, const double *wX, const double *wY, i64 ny, i64 nx, i64 nt, hipStream_t st) {
    DS_ARG(nt <= 65535, "weight pyramid: too many time nodes for one launch");
    dim3 grid((unsigned)launch_blocks(ny * nx, 256, 1024), (unsigned)nt);
    DS_KLAUNCH(k_weight_space, grid, dim3(256), 0, st, w, wX, wY, ny, nx, nt);
    DS_HIP(hipGetLastError());
    return 0;
}

int launch_weight_log10_sum(const double *w, i64 n, double *partials, hipStream_t st) {
    DS_KLAUNCH(k_weight_log10_sum, dim3(WEIGHT_LOG10_BLOCKS), dim3(256), 0, st, w, n, partials);
    DS_KLAUNCH(k_weight_log10_final, dim3(1), dim3(256), 0, st, partials, WEIGHT_LOG10_BLOCKS);
    DS_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
i64 weights_level_len(i64 ny, i64 nx, i64 nt, int levels, int level, i64 *lny, i64 *lnx, i64 *lnt) {
    if (levels < 1 || level < 0 || level >= levels || ny < 2 || nx < 2 || nt < 2) return -1;
    i64 len = -1;
    for (int l = levels - 1; l >= 0; --l) {
        if (l == level) {
            len = ny * nx * (nt - 1) + ny * (nx - 1) * nt + (ny - 1) * nx * nt;
            if (lny) *lny = ny;
            if (lnx) *lnx = nx;
            if (lnt) *lnt = nt;
        }
        if (l == 0) break;
        if (ny < 3 || nx < 3 || nt < 3 || !(ny & 1) || !(nx & 1) || !(nt & 1)) return -1;   // 2m + 1 -> m + 1 on every axis
        ny = (ny + 1) / 2; nx = (nx + 1) / 2; nt = (nt + 1) / 2;
    }
    return len;
}

Weights::~Weights() {
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (st || partials || !lev.empty()) (void)hipSetDevice(device);
    if (st) (void)hipStreamSynchronize(st);
    for (auto &l : lev) dfree(l.w);
    dfree(partials);
    if (st) (void)hipStreamDestroy(st);
    if (cur >= 0) (void)hipSetDevice(cur);
}

int Weights::init(int dev, i64 ny, i64 nx, i64 nt, int nlev) {
    DS_ARG(weights_level_len(ny, nx, nt, nlev, 0) >= 0,
           "weight pyramid: needs ny, nx, nt >= 2, levels >= 1 and 2^k*m+1 sizes on every axis down to the coarsest level");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available (libdotsocp has no CPU fallback)");
        return DOTSOCP_ENODEVICE;
    }
    DS_ARG(dev >= 0 && dev < ndev, "device ordinal out of range");
    device = dev;
    levels = nlev;
    DS_HIP(hipSetDevice(device));
    DS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    lev.resize(nlev);
    for (int l = 0; l < nlev; ++l) {
        Level &L = lev[l];
        L.Nq = weights_level_len(ny, nx, nt, nlev, l, &L.ny, &L.nx, &L.nt);
        DS_CHECK(dmalloc(&L.w, L.Nq));
    }
    DS_CHECK(dmalloc(&partials, WEIGHT_LOG10_BLOCKS + 1));
    return 0;
}

int Weights::check_level(int level, bool need_filled) const {
    DS_ARG(level >= 0 && level < levels, "weight pyramid: level out of range");
    if (need_filled && !lev[level].filled) {
        set_error("weight pyramid: level %d has not been filled (set / set_space, then restrict)", level);
        return DOTSOCP_ESTATE;
    }
    return 0;
}

int Weights::level_for_upload(int level, const Level **out) const {
    DS_CHECK(check_level(level, true));
    *out = &lev[level];
    return 0;
}

int Weights::finest_done() {
    DS_HIP(ds_stream_synchronize(st));
    for (auto &l : lev) l.filled = false;        // the coarser levels belong to the weight that was set before
    lev[levels - 1].filled = true;
    return 0;
}

int Weights::set(const double *weight) {
    DS_ARG(weight != nullptr, "weight is NULL");
    DS_HIP(hipSetDevice(device));
    Level &L = lev[levels - 1];
    DS_HIP(ds_memcpy_async(L.w, weight, sizeof(double) * (size_t)L.Nq, hipMemcpyHostToDevice, st));
    return finest_done();
}

int Weights::set_space(const double *weightX, const double *weightY) {
    DS_ARG(weightX != nullptr && weightY != nullptr, "weightX / weightY is NULL");
    DS_HIP(hipSetDevice(device));
    Level &L = lev[levels - 1];
    const i64 nX = L.ny * (L.nx - 1), nY = (L.ny - 1) * L.nx;
    double *d = nullptr;
    DS_CHECK(dmalloc(&d, nX + nY));
    int rc = 0;
    if (ds_memcpy_async(d, weightX, sizeof(double) * (size_t)nX, hipMemcpyHostToDevice, st) != hipSuccess ||
        ds_memcpy_async(d + nX, weightY, sizeof(double) * (size_t)nY, hipMemcpyHostToDevice, st) != hipSuccess) {
        set_error("weight pyramid: upload of weightX / weightY failed");
        rc = DOTSOCP_EHIP;
    }
    if (!rc) rc = launch_weight_space(L.w, d, d + nX, L.ny, L.nx, L.nt, st);
    if (!rc) rc = finest_done();
    else (void)ds_stream_synchronize(st);
    dfree(d);
    return rc;
}

int Weights::restrict_all(int log_mean) {
    if (!lev[levels - 1].filled) {
        set_error("weight pyramid: restrict() needs set() or set_space() first");
        return DOTSOCP_ESTATE;
    }
    DS_HIP(hipSetDevice(device));
    for (int l = levels - 2; l >= 0; --l) {
        const Level &F = lev[l + 1];
        DS_CHECK(launch_weight_restrict(F.w, lev[l].w, F.ny, F.nx, F.nt, log_mean != 0, st));
    }
    DS_HIP(ds_stream_synchronize(st));
    for (auto &l : lev) l.filled = true;
    return 0;
}

int Weights::log10_mean(int level, double *mean) {
    DS_ARG(mean != nullptr, "mean is NULL");
    DS_CHECK(check_level(level, true));
    DS_HIP(hipSetDevice(device));
    const Level &L = lev[level];
    DS_CHECK(launch_weight_log10_sum(L.w, L.Nq, partials, st));
    double sum = 0.0;
    DS_HIP(ds_memcpy_async(&sum, partials + WEIGHT_LOG10_BLOCKS, sizeof(double), hipMemcpyDeviceToHost, st));
    DS_HIP(ds_stream_synchronize(st));
    *mean = sum / (double)L.Nq;
    return 0;
}

int Weights::download(int level, double *host) {
    DS_ARG(host != nullptr, "host pointer is NULL");
    DS_CHECK(check_level(level, true));
    DS_HIP(hipSetDevice(device));
    const Level &L = lev[level];
    host_first_touch(host, sizeof(double) * (size_t)L.Nq);
    DS_HIP(ds_memcpy_async(host, L.w, sizeof(double) * (size_t)L.Nq, hipMemcpyDeviceToHost, st));
    DS_HIP(ds_stream_synchronize(st));
    return 0;
}

}  // namespace dotsocp
