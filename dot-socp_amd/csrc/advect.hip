// Particle transport along the solved flow: the velocity v = E / rho of the Benamou-Brenier solution at the nodes
// (the arrows of utils/show_movement_2d.m, without the plot) and its characteristics, the Monge map, by classical RK4.
// Semantics: include/dotsocp.h (dotsocp_recover_velocity, dotsocp_advect_particles, dotsocp_push_mass, dotsocp_map_report); the numpy twin dot-socp_amd/advect.py
// follows the kernels below operation by operation, and this file is built without contraction (Makefile), so the two
// agree bit for bit.
//   k_velocity_layer  one node layer of (vX, vY) from alpha: rho, Ex, Ey are the expressions of outputs_node.h, i.e. the
//                     bits dotsocp_recover_outputs writes; no grid-sized velocity array is ever made
//   k_advect          one thread per particle, one launch per time interval: all nsub RK4 steps with the position in
//                     registers; every stage gathers 4 corners x 2 layers x 2 components from the two layers of the interval
//   k_deposit         one thread per particle, once per requested frame: the particle's mass units split over the corners of
//                     its cell and added to a plane of 64-bit counts by four returnless integer atomics
//   k_frame_l1        counts -> frame (in place) and the tile sums of |frame - rho| against the node layer, in the report's order
//   k_advect<., true> the same march, adding up |step|^2 and |step| per particle (dotsocp_map_report)
//   k_map_final       displacement, path length, action and detour of every particle; sums, maxima and the detour histogram
// Index conventions as everywhere: y fastest (rows `py` apart); X = the component / coordinate along the second array
// index, Y = along the first.  1-D problems live in the Y slot (ny = nx1d, nx = 1): their kernels touch Y alone.
#include "device_utils.h"
#include "kernels.h"
#include "outputs_node.h"

namespace dotsocp {

// v = E / rho where rho > floor and the quotient is finite, else 0: the field is finite everywhere (a NaN density fails
// the comparison)
__device__ __forceinline__ double vel_quot(double E, double rho, double floor) {
    const double q = E / rho;
    return (rho > floor && isfinite(q)) ? q : 0.0;
}

// node layer `tl` (slab-local) -> vX, vY [y + py * x]
template <int DIM, bool WEIGHTED>
__global__ void __launch_bounds__(TILE_Y *TILE_X) k_velocity_layer(Grid g, OutArgs o, i64 tl, double floor,
                                                                    double *__restrict__ vX, double *__restrict__ vY) {
    const i64 y = (i64)blockIdx.x * TILE_Y + threadIdx.x;
    const i64 x = (i64)blockIdx.y * TILE_X + threadIdx.y;
    if (y >= g.ny || x >= g.nx) return;
    const i64 tg = g.t0 + tl, col = y + g.py * x, node = col + g.plane * tl;
    const bool ends = (tg == 0 || tg == g.nt - 1);
    const double rho = out_rho<WEIGHTED>(g, o, tg, tl, col, node);
    const double f = ends ? 2.0 : 1.0;
    if (DIM == 2) {
        double Ex = 0.0;
        if (x >= 1 && x <= g.nx - 2) {
            const i64 e = out_edge_x(g, y, x, tl);
            Ex = out_flux(out_a<WEIGHTED>(o, e - g.py), out_a<WEIGHTED>(o, e), f);
        }
        vX[col] = vel_quot(Ex, rho, floor);
    }
    double Ey = 0.0;
    if (y >= 1 && y <= g.ny - 2) {
        const i64 e = out_edge_y(g, y, x, tl);
        Ey = out_flux(out_a<WEIGHTED>(o, e - 1), out_a<WEIGHTED>(o, e), f);
    }
    vY[col] = vel_quot(Ey, rho, floor);
}

int launch_velocity_layer(const Grid &g, const double *alpha, const double *weight, const double *rho0, const double *rho1,
                          const double *a_prev, double sig, double cD, bool dim1, i64 tl, double floor, double *vX, double *vY,
                          hipStream_t st) {
    if (tl < 0 || tl >= g.ntl) { set_error("internal: velocity layer outside its slab"); return DOTSOCP_ESTATE; }
    OutArgs o{nullptr, alpha, weight, rho0, rho1, a_prev, sig, cD, 0.0};
    dim3 grid((unsigned)((g.ny + TILE_Y - 1) / TILE_Y), (unsigned)((g.nx + TILE_X - 1) / TILE_X), 1), block(TILE_Y, TILE_X);
    if (dim1) {
        if (weight) DS_KLAUNCH((k_velocity_layer<1, true>), grid, block, 0, st, g, o, tl, floor, vX, vY);
        else DS_KLAUNCH((k_velocity_layer<1, false>), grid, block, 0, st, g, o, tl, floor, vX, vY);
    } else {
        if (weight) DS_KLAUNCH((k_velocity_layer<2, true>), grid, block, 0, st, g, o, tl, floor, vX, vY);
        else DS_KLAUNCH((k_velocity_layer<2, false>), grid, block, 0, st, g, o, tl, floor, vX, vY);
    }
    DS_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------
// particles
// ---------------------------------------------------------------------------------------
// one particle per thread; workgroups of 64, 128, 256 and 512 ran within 5 % of each other (profiles/advect_time.txt)
#define ADV_BLOCK 256

__device__ __forceinline__ double adv_clamp(double u) { return u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u); }

// seeds outside [0, 1] are moved onto the boundary before the first step (not counted as clamped); flags start at zero
template <int DIM>
__global__ void __launch_bounds__(ADV_BLOCK) k_advect_seed(i64 n, double *__restrict__ px, double *__restrict__ py,
                                                          unsigned int *__restrict__ flag) {
    const i64 p = (i64)blockIdx.x * ADV_BLOCK + threadIdx.x;
    if (p >= n) return;
    if (DIM == 2) px[p] = adv_clamp(px[p]);
    py[p] = adv_clamp(py[p]);
    flag[p] = 0u;
}

struct AdvectArgs {
    const double *vX0, *vY0, *vX1, *vY1;    // velocity layers of node k and node k + 1 of the interval
    i64 ny, nx, py;                         // nodes along Y / along X, row pitch
    i64 n;
    int nsub, dir;
    double dt, hh, h6;                      // dir / ((nt - 1) nsub), dt / 2, dt / 6
    double *px, *py_;                       // positions, SoA
    unsigned int *flag;                     // sticky: the clamp at the end of some step moved this particle
    double *sq, *len;                       // k_advect<., true>: sum of |step|^2 and of |step| so far, per particle
};

// cell index and weight along one axis of n nodes: u in [0, 1]
__device__ __forceinline__ void adv_cell(double u, i64 n, i64 &i, double &a) {
    const double f = u * (double)(n - 1);
    i = (i64)floor(f);
    if (i > n - 2) i = n - 2;
    a = f - (double)i;
}

// one layer at (x, y): along Y (the contiguous index) first, then along X
template <int DIM>
__device__ __forceinline__ double adv_layer(const double *__restrict__ F, i64 py, i64 i, double a, i64 j, double c) {
    if (DIM == 1) return (1.0 - c) * F[j] + c * F[j + 1];
    const double *p = F + j + py * i;
    const double f0 = (1.0 - c) * p[0] + c * p[1];
    const double f1 = (1.0 - c) * p[py] + c * p[py + 1];
    return (1.0 - a) * f0 + a * f1;
}

template <int DIM>
__device__ __forceinline__ void adv_velocity(const AdvectArgs &A, double x, double y, double b, double &vx, double &vy) {
    i64 i = 0, j;
    double a = 0.0, c;
    if (DIM == 2) adv_cell(x, A.nx, i, a);
    adv_cell(y, A.ny, j, c);
    if (DIM == 2) vx = (1.0 - b) * adv_layer<2>(A.vX0, A.py, i, a, j, c) + b * adv_layer<2>(A.vX1, A.py, i, a, j, c);
    else vx = 0.0;
    vy = (1.0 - b) * adv_layer<DIM>(A.vY0, A.py, i, a, j, c) + b * adv_layer<DIM>(A.vY1, A.py, i, a, j, c);
}

// ACC (dotsocp_map_report): the march also adds up what every step actually moved the particle -- between the position
// before the step and the one after its end clamp -- as |step|^2 and |step|, in march order
template <int DIM, bool ACC>
__global__ void __launch_bounds__(ADV_BLOCK) k_advect(AdvectArgs A) {
    const i64 p = (i64)blockIdx.x * ADV_BLOCK + threadIdx.x;
    if (p >= A.n) return;
    double x = DIM == 2 ? A.px[p] : 0.0, y = A.py_[p];
    double sq = 0.0, len = 0.0;
    if (ACC) { sq = A.sq[p]; len = A.len[p]; }
    bool moved = false;
    const double den = (double)(2 * A.nsub);
    for (int s = 0; s < A.nsub; ++s) {
        // stage fractions inside the interval: forward from node k, backward from node k + 1
        const int e0 = A.dir > 0 ? 2 * s : 2 * (A.nsub - s);
        const double b0 = (double)e0 / den, b1 = (double)(e0 + A.dir) / den, b2 = (double)(e0 + 2 * A.dir) / den;
        double k1x, k1y, k2x, k2y, k3x, k3y, k4x, k4y;
        adv_velocity<DIM>(A, x, y, b0, k1x, k1y);
        adv_velocity<DIM>(A, adv_clamp(x + A.hh * k1x), adv_clamp(y + A.hh * k1y), b1, k2x, k2y);
        adv_velocity<DIM>(A, adv_clamp(x + A.hh * k2x), adv_clamp(y + A.hh * k2y), b1, k3x, k3y);
        adv_velocity<DIM>(A, adv_clamp(x + A.dt * k3x), adv_clamp(y + A.dt * k3y), b2, k4x, k4y);
        const double ux = x + A.h6 * (((k1x + 2.0 * k2x) + 2.0 * k3x) + k4x);
        const double uy = y + A.h6 * (((k1y + 2.0 * k2y) + 2.0 * k3y) + k4y);
        moved = moved || ux < 0.0 || ux > 1.0 || uy < 0.0 || uy > 1.0;
        const double xo = x, yo = y;
        x = adv_clamp(ux);
        y = adv_clamp(uy);
        if (ACC) {
            const double ex = x - xo, ey = y - yo;
            const double s2 = DIM == 2 ? ex * ex + ey * ey : ey * ey;
            sq = sq + s2;
            len = len + sqrt(s2);
        }
    }
    if (DIM == 2) A.px[p] = x;
    A.py_[p] = y;
    if (moved) A.flag[p] = 1u;
    if (ACC) { A.sq[p] = sq; A.len[p] = len; }
}

// *count += number of set flags
__global__ void __launch_bounds__(ADV_BLOCK) k_advect_count(const unsigned int *__restrict__ flag, i64 n,
                                                           unsigned long long *__restrict__ count) {
    unsigned long long c = 0;
    for (i64 p = (i64)blockIdx.x * ADV_BLOCK + threadIdx.x; p < n; p += (i64)gridDim.x * ADV_BLOCK) c += flag[p] ? 1u : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

int launch_advect_seed(bool dim1, i64 n, double *px, double *py, unsigned int *flag, hipStream_t st) {
    if (n <= 0) return 0;
    const dim3 grid((unsigned)launch_blocks(n, ADV_BLOCK, (i64)1 << 30));
    if (dim1) DS_KLAUNCH(k_advect_seed<1>, grid, dim3(ADV_BLOCK), 0, st, n, px, py, flag);
    else DS_KLAUNCH(k_advect_seed<2>, grid, dim3(ADV_BLOCK), 0, st, n, px, py, flag);
    DS_HIP(hipGetLastError());
    return 0;
}

int launch_advect(bool dim1, i64 ny, i64 nx, i64 py, const double *vX0, const double *vY0, const double *vX1,
                  const double *vY1, i64 n, int nsub, int dir, double dt, double *px, double *py_, unsigned int *flag,
                  hipStream_t st, double *sq, double *len) {
    if (n <= 0) return 0;
    AdvectArgs A{vX0, vY0, vX1, vY1, ny, nx, py, n, nsub, dir, dt, 0.5 * dt, dt / 6.0, px, py_, flag, sq, len};
    const dim3 grid((unsigned)launch_blocks(n, ADV_BLOCK, (i64)1 << 30));
    if (sq && len) {
        if (dim1) DS_KLAUNCH((k_advect<1, true>), grid, dim3(ADV_BLOCK), 0, st, A);
        else DS_KLAUNCH((k_advect<2, true>), grid, dim3(ADV_BLOCK), 0, st, A);
    } else {
        if (dim1) DS_KLAUNCH((k_advect<1, false>), grid, dim3(ADV_BLOCK), 0, st, A);
        else DS_KLAUNCH((k_advect<2, false>), grid, dim3(ADV_BLOCK), 0, st, A);
    }
    DS_HIP(hipGetLastError());
    return 0;
}

int launch_advect_count(const unsigned int *flag, i64 n, unsigned long long *count, hipStream_t st) {
    if (n <= 0) return 0;
    DS_KLAUNCH(k_advect_count, dim3((unsigned)launch_blocks(n, ADV_BLOCK, 1024)), dim3(ADV_BLOCK), 0, st, flag, n, count);
    DS_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------
// mass carried by the particles (dotsocp_push_mass): bilinear deposit in integer units, frame and its distance to rho
// ---------------------------------------------------------------------------------------
// One thread per particle: its M units are split over the corners of its cell -- the cell and the weights of adv_cell, as the
// velocity interpolation takes them -- by round-to-nearest-even of weight * M on three corners and the remainder on the
// fourth, and added with returnless 64-bit integer atomics (two's complement: a remainder of -1 wraps exactly).  Integer
// sums know no order, so neither the particle order nor the launch shape nor the slab split shows in a bit.  Particles in
// grid order (seeds_on_nodes) put the lanes of a wavefront on contiguous row segments of the plane.
template <int DIM>
__global__ void __launch_bounds__(ADV_BLOCK) k_deposit(i64 n, const double *__restrict__ px, const double *__restrict__ py_,
                                                      const i64 *__restrict__ units, i64 ny, i64 nx, i64 py,
                                                      unsigned long long *__restrict__ cnt) {
    const i64 p = (i64)blockIdx.x * ADV_BLOCK + threadIdx.x;
    if (p >= n) return;
    const i64 M = units[p];
    if (M == 0) return;
    const double Md = (double)M;
    i64 j;
    double c;
    adv_cell(py_[p], ny, j, c);
    if (j < 0) j = 0;               // positions are finite and in [0, 1]; whatever else arrives stays inside the plane
    if (DIM == 1) {
        const i64 d0 = __double2ll_rn((1.0 - c) * Md);
        atomicAdd(cnt + j, (unsigned long long)d0);
        atomicAdd(cnt + j + 1, (unsigned long long)(M - d0));
        return;
    }
    i64 i;
    double a;
    adv_cell(px[p], nx, i, a);
    if (i < 0) i = 0;
    const i64 d00 = __double2ll_rn(((1.0 - c) * (1.0 - a)) * Md);
    const i64 d10 = __double2ll_rn((c * (1.0 - a)) * Md);
    const i64 d01 = __double2ll_rn(((1.0 - c) * a) * Md);
    const i64 d11 = M - d00 - d10 - d01;
    unsigned long long *q = cnt + j + py * i;
    atomicAdd(q, (unsigned long long)d00);
    atomicAdd(q + 1, (unsigned long long)d10);
    atomicAdd(q + py, (unsigned long long)d01);
    atomicAdd(q + py + 1, (unsigned long long)d11);
}

int launch_deposit(bool dim1, i64 ny, i64 nx, i64 py, i64 n, const double *px, const double *py_, const i64 *units,
                   unsigned long long *cnt, hipStream_t st) {
    if (n <= 0) return 0;
    const dim3 grid((unsigned)launch_blocks(n, ADV_BLOCK, (i64)1 << 30));
    if (dim1) DS_KLAUNCH(k_deposit<1>, grid, dim3(ADV_BLOCK), 0, st, n, px, py_, units, ny, nx, py, cnt);
    else DS_KLAUNCH(k_deposit<2>, grid, dim3(ADV_BLOCK), 0, st, n, px, py_, units, ny, nx, py, cnt);
    DS_HIP(hipGetLastError());
    return 0;
}

// counts -> frame = (double)count * unit, in place, and the tile sums of |frame - rho| against node layer `tl` of the slab:
// rho as k_velocity_layer forms it, tiles and the order of the additions as k_report's layer sums (lanes, then wavefronts;
// launch_report_rows adds the tiles), so the sum depends on (ny, nx) alone
template <bool WEIGHTED>
__global__ void __launch_bounds__(TILE_Y *TILE_X) k_frame_l1(Grid g, OutArgs o, i64 tl, double unit, double *__restrict__ frame,
                                                              double *__restrict__ partials) {
    __shared__ double s_red[TILE_X];
    const int lane = threadIdx.x, xl = threadIdx.y;
    const i64 y = (i64)blockIdx.x * TILE_Y + lane;
    const i64 x = (i64)blockIdx.y * TILE_X + xl;
    double v = 0.0;
    if (y < g.ny && x < g.nx) {
        const i64 tg = g.t0 + tl, col = y + g.py * x, node = col + g.plane * tl;
        const double rho = out_rho<WEIGHTED>(g, o, tg, tl, col, node);
        const double f = (double)__double_as_longlong(frame[col]) * unit;
        frame[col] = f;
        v = fabs(f - rho);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) s_red[xl] = v;
    __syncthreads();
    if (lane == 0 && xl == 0) {
        double s = s_red[0];
#pragma unroll
        for (int wv = 1; wv < TILE_X; ++wv) s += s_red[wv];
        partials[blockIdx.x + (i64)gridDim.x * blockIdx.y] = s;
    }
}

int launch_frame_l1(const Grid &g, const double *alpha, const double *weight, const double *rho0, const double *rho1,
                    const double *a_prev, double sig, double cD, i64 tl, double unit, double *frame, double *partials,
                    double *sum, hipStream_t st) {
    if (tl < 0 || tl >= g.ntl) { set_error("internal: frame layer outside its slab"); return DOTSOCP_ESTATE; }
    OutArgs o{nullptr, alpha, weight, rho0, rho1, a_prev, sig, cD, 0.0};
    dim3 grid((unsigned)((g.ny + TILE_Y - 1) / TILE_Y), (unsigned)((g.nx + TILE_X - 1) / TILE_X), 1), block(TILE_Y, TILE_X);
    if (weight) DS_KLAUNCH(k_frame_l1<true>, grid, block, 0, st, g, o, tl, unit, frame, partials);
    else DS_KLAUNCH(k_frame_l1<false>, grid, block, 0, st, g, o, tl, unit, frame, partials);
    DS_HIP(hipGetLastError());
    return launch_report_rows(partials, report_tiles(g), 1, sum, st);
}

// ---------------------------------------------------------------------------------------
// judgement of the map (dotsocp_map_report): displacement, path length and action of every particle, their mass-weighted sums
// ---------------------------------------------------------------------------------------
// One thread per particle, after the last interval: the per-particle values from the end position, the seed (clamped as
// k_advect_seed clamps it) and the two sums of k_advect<., true>.  Sums: the 64 lanes of a wavefront by shuffles, the four
// wavefronts in index order through LDS, one row of MS_COUNT partial sums per workgroup; launch_report_rows adds the
// workgroups by k_report_final's tree, so the order depends on n alone.  Threads behind the last particle add +0.0 (every
// term is >= 0: no bit changes).  Histogram, counts and maxima (the bit patterns of non-negative doubles order as unsigned
// integers) go through LDS counters and are flushed with one 64-bit integer atomic per slot and workgroup.
struct MapArgs {
    i64 n;
    const double *px, *py_, *sq, *len;      // end positions and path sums (the particle block)
    const double *sx, *sy;                  // seeds as given
    const double *mass;                     // or nullptr: every mass is 1.0
    const double *edges;                    // DOTSOCP_REPORT_BINS + 1 doubles
    double steps;                           // (double)((nt - 1) nsub) = 1 / |dt|
    double *disp, *action;                  // per-particle outputs or nullptr (len is there already)
    double *partials;                       // [MS_COUNT][workgroups]
    unsigned long long *counts;             // [MC_COUNT]
};

template <int DIM>
__global__ void __launch_bounds__(ADV_BLOCK) k_map_final(MapArgs a) {
    __shared__ double s_edges[DOTSOCP_REPORT_BINS + 1];
    __shared__ unsigned int s_cnt[DOTSOCP_REPORT_BINS + 2];               // MC_HIST .. MC_STILL
    __shared__ unsigned long long s_key[3];
    __shared__ double s_red[ADV_BLOCK / 64][MS_COUNT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid < DOTSOCP_REPORT_BINS + 1) s_edges[tid] = a.edges[tid];
    if (tid < DOTSOCP_REPORT_BINS + 2) s_cnt[tid] = 0;
    if (tid < 3) s_key[tid] = 0;
    __syncthreads();
    const i64 p = (i64)blockIdx.x * ADV_BLOCK + tid;
    double v[MS_COUNT];
#pragma unroll
    for (int i = 0; i < MS_COUNT; ++i) v[i] = 0.0;
    double disp = 0.0, len = 0.0, detour = 0.0;
    bool over = false, still = false;
    if (p < a.n) {
        const double dy = a.py_[p] - adv_clamp(a.sy[p]);
        double disp2 = dy * dy;
        if (DIM == 2) {
            const double dx = a.px[p] - adv_clamp(a.sx[p]);
            disp2 = dx * dx + dy * dy;
        }
        disp = sqrt(disp2);
        len = a.len[p];
        const double action = a.sq[p] * a.steps, len2 = len * len;
        const double r = 1.0 - disp / len;
        detour = (len > 0.0 && r > 0.0) ? r : 0.0;
        if (a.disp) a.disp[p] = disp;
        if (a.action) a.action[p] = action;
        const double m = a.mass ? a.mass[p] : 1.0;
        v[MS_MASS] = m;
        v[MS_DISP2] = m * disp2;
        v[MS_LEN2] = m * len2;
        v[MS_ACTION] = m * action;
        v[MS_DISP] = m * disp;
        v[MS_LEN] = m * len;
        const int j = report_bin(s_edges, detour);
        if (j >= 0) atomicAdd(&s_cnt[MC_HIST + j], 1u);
        over = detour > s_edges[DOTSOCP_REPORT_BINS];
        still = len == 0.0;
    }
    // the two counts a rough flow sends most particles to: one LDS atomic per wavefront instead of one per lane
    const unsigned long long b_over = __ballot(over), b_still = __ballot(still);
    if (lane == 0) {
        if (b_over) atomicAdd(&s_cnt[MC_OVER], (unsigned int)__popcll(b_over));
        if (b_still) atomicAdd(&s_cnt[MC_STILL], (unsigned int)__popcll(b_still));
    }
    unsigned long long key[3] = {(unsigned long long)__double_as_longlong(disp), (unsigned long long)__double_as_longlong(len),
                                 (unsigned long long)__double_as_longlong(detour)};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        unsigned long long k = key[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_down(k, off, 64);
            k = o > k ? o : k;
        }
        if (lane == 0 && k) atomicMax(&s_key[i], k);
    }
#pragma unroll
    for (int i = 0; i < MS_COUNT; ++i) {
        double s = v[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) s_red[wv][i] = s;
    }
    __syncthreads();
    if (tid < MS_COUNT) {
        double s = s_red[0][tid];
#pragma unroll
        for (int w = 1; w < ADV_BLOCK / 64; ++w) s += s_red[w][tid];
        a.partials[(i64)tid * gridDim.x + blockIdx.x] = s;
    }
    if (tid < DOTSOCP_REPORT_BINS + 2) {
        if (s_cnt[tid]) atomicAdd(&a.counts[tid], (unsigned long long)s_cnt[tid]);
    } else if (tid < DOTSOCP_REPORT_BINS + 5) {
        const int k = tid - (DOTSOCP_REPORT_BINS + 2);
        if (s_key[k]) atomicMax(&a.counts[MC_DISP_MAX + k], s_key[k]);
    }
}

i64 map_blocks(i64 n) { return (n + ADV_BLOCK - 1) / ADV_BLOCK; }

int launch_map_final(bool dim1, i64 n, const double *px, const double *py_, const double *sq, const double *len, const double *sx,
                     const double *sy, const double *mass, const double *edges, double steps, double *disp, double *action,
                     double *partials, double *sums, unsigned long long *counts, hipStream_t st) {
    if (n <= 0) return 0;
    MapArgs a{n, px, py_, sq, len, sx, sy, mass, edges, steps, disp, action, partials, counts};
    const i64 blocks = map_blocks(n);
    if (blocks > ((i64)1 << 30)) { set_error("invalid argument: map_report() serves up to 2^38 particles"); return DOTSOCP_EINVAL; }
    if (dim1) DS_KLAUNCH(k_map_final<1>, dim3((unsigned)blocks), dim3(ADV_BLOCK), 0, st, a);
    else DS_KLAUNCH(k_map_final<2>, dim3((unsigned)blocks), dim3(ADV_BLOCK), 0, st, a);
    DS_HIP(hipGetLastError());
    return launch_report_rows(partials, blocks, MS_COUNT, sums, st);
}

}  // namespace dotsocp
