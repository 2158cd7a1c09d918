// Pictures of the density evolution (include/dotsocp.h: dotsocp_render_evolution): the frames of utils/show_evolution_2d.m
// and export_evolution_2d.m and the arrows of show_movement_2d.m, without the figure window, from the device-resident alpha.
// rho, Ex, Ey at a node are the expressions of outputs_node.h -- the bits dotsocp_recover_outputs writes -- and this file is
// built without contraction (Makefile), so the numpy twin dot-socp_amd/render.py agrees byte for byte.
//   k_rho_range   one pass over a slab's node layers in the tile shape of k_report (a 64 x 4 tile of columns marches over a
//                 chunk of layers, a(.) of the cell below stays in a register: every alpha0 entry is requested once): max and
//                 min of the finite unmasked rho as ordered integer keys, the counts of non-finite and of masked nodes.
//                 Neither extremum nor count depends on an order: 64-bit integer atomics, no floating-point atomic.
//   k_render      one frame node -> uint8 picture [ny][nx][channels], x fastest.  rho is read as everywhere else: a wavefront
//                 takes 64 consecutive y of one column (pitched rows, g.py), so the loads are whole cache lines; the picture
//                 wants x fastest, so the indices of a 64 x 64 tile go through LDS and leave transposed: consecutive threads
//                 store consecutive bytes of an image row.  A tile row is RND_PITCH = 68 bytes = 17 dwords: the 64 lanes of
//                 a wavefront write one byte each into 64 different rows, 17 dwords apart -- 17 is odd, so the 32 lanes of
//                 a half land on 32 different banks; the transposed reads run along a row, four lanes per dword.
//   k_movement    one thread per kept node (y = 0, skip_y, .., x = 0, skip_x, ..): Ex, Ey, zeroed where rho is small, dense.
#include <cmath>

#include "device_utils.h"
#include "kernels.h"
#include "outputs_node.h"

namespace dotsocp {

#define RND_GROUPS 16384            // workgroups the range pass aims at (k_report's figure)

template <bool WEIGHTED>
__global__ void __launch_bounds__(TILE_Y *TILE_X) k_rho_range(Grid g, OutArgs o, const unsigned char *__restrict__ barrier,
                                                               i64 chunk, unsigned long long *__restrict__ counts) {
    __shared__ unsigned long long s_key[2];
    __shared__ unsigned int s_cnt[2];
    const int lane = threadIdx.x, xl = threadIdx.y, tid = xl * TILE_Y + lane;
    if (tid < 2) { s_key[tid] = 0; s_cnt[tid] = 0; }
    __syncthreads();
    const i64 y = (i64)blockIdx.x * TILE_Y + lane;
    const i64 x = (i64)blockIdx.y * TILE_X + xl;
    const bool inb = (y < g.ny) && (x < g.nx);
    const i64 tbeg = (i64)blockIdx.z * chunk;
    const i64 tend = (tbeg + chunk < g.ntl) ? tbeg + chunk : g.ntl;
    // lanes outside the grid load column 0 (it always exists) and use nothing of it
    const i64 col = inb ? y + g.py * x : 0;
    const bool masked = inb && barrier != nullptr && barrier[y + g.ny * x] != 0;
    double a_below;                                 // a(.) of cell tbeg - 1 (unused on the global first layer)
    if (tbeg > 0) a_below = out_a<WEIGHTED>(o, col + g.plane * (tbeg - 1));
    else a_below = g.first ? 0.0 : o.a_prev[col];
    double rmax = -INFINITY, rmin = INFINITY;
    unsigned int n_bad = 0, n_mask = 0;
    for (i64 tl = tbeg; tl < tend; ++tl) {
        const i64 tg = g.t0 + tl;
        const bool ends = (tg == 0 || tg == g.nt - 1), cell = tl < g.ncl;
        const double a_here = out_a<WEIGHTED>(o, cell ? col + g.plane * tl : col);
        const double r_end = ends ? (tg == 0 ? o.rho0 : o.rho1)[col] : 0.0;
        const double rho = ends ? r_end : out_mean2(a_below, a_here);
        a_below = a_here;
        if (!inb) continue;
        if (masked) ++n_mask;
        else if (isfinite(rho)) {
            const double r = rho + 0.0;             // a -0.0 counts as the +0.0 it equals
            rmax = r > rmax ? r : rmax;
            rmin = r < rmin ? r : rmin;
        } else ++n_bad;
    }
    // threads -> wavefront (shuffles) -> LDS -> one 64-bit integer atomic per slot and workgroup
    unsigned long long kmax = rmax > -INFINITY ? report_key(rmax) : 0ull, kmin = rmin < INFINITY ? ~report_key(rmin) : 0ull;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long pmax = __shfl_down(kmax, off, 64), pmin = __shfl_down(kmin, off, 64);
        kmax = pmax > kmax ? pmax : kmax;
        kmin = pmin > kmin ? pmin : kmin;
        n_bad += __shfl_down(n_bad, off, 64);
        n_mask += __shfl_down(n_mask, off, 64);
    }
    if (lane == 0) {
        if (kmax) atomicMax(&s_key[0], kmax);
        if (kmin) atomicMax(&s_key[1], kmin);
        if (n_bad) atomicAdd(&s_cnt[0], n_bad);
        if (n_mask) atomicAdd(&s_cnt[1], n_mask);
    }
    __syncthreads();
    if (tid < 2) {
        if (s_key[tid]) atomicMax(&counts[RR_MAX + tid], s_key[tid]);
    } else if (tid < 4) {
        if (s_cnt[tid - 2]) atomicAdd(&counts[RR_NONFINITE + tid - 2], (unsigned long long)s_cnt[tid - 2]);
    }
}

int launch_rho_range(const Grid &g, const double *alpha, const double *weight, const double *rho0, const double *rho1,
                     const double *a_prev, double sig, double cD, const unsigned char *barrier, unsigned long long *counts,
                     hipStream_t st) {
    if (g.ntl <= 0) return 0;
    OutArgs o{nullptr, alpha, weight, rho0, rho1, a_prev, sig, cD, 0.0};
    const i64 tiles = report_tiles(g);
    i64 chunks = (RND_GROUPS + tiles - 1) / tiles;
    if (chunks > g.ntl) chunks = g.ntl;
    const i64 chunk = (g.ntl + chunks - 1) / chunks;
    chunks = (g.ntl + chunk - 1) / chunk;
    dim3 grid((unsigned)((g.ny + TILE_Y - 1) / TILE_Y), (unsigned)((g.nx + TILE_X - 1) / TILE_X), (unsigned)chunks);
    if (weight) DS_KLAUNCH(k_rho_range<true>, grid, dim3(TILE_Y, TILE_X), 0, st, g, o, barrier, chunk, counts);
    else DS_KLAUNCH(k_rho_range<false>, grid, dim3(TILE_Y, TILE_X), 0, st, g, o, barrier, chunk, counts);
    DS_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------
// frames
// ---------------------------------------------------------------------------------------
#define RND_TX 64                   // columns of a picture tile (rows: TILE_Y)
#define RND_PITCH (RND_TX + 4)      // bytes of a tile row in LDS

struct RenderArgs {
    OutArgs o;
    i64 tl;                         // node layer of the slab
    const unsigned char *barrier;   // ny x nx, y fastest, or nullptr
    const double *levels;           // nlevels ascending doubles (LEVELS)
    const unsigned char *lut;       // 256 x 3 (CHANNELS = 3)
    int nlevels, barrier_index;
    double vmax, k;                 // the scale, 255.0 / vmax
    unsigned char *image;           // [ny][nx][CHANNELS]
};

// index of a density (include/dotsocp.h); lev: the LDS table
template <int MODE>
__device__ __forceinline__ int render_index(double rho, const RenderArgs &a, const double *lev) {
    if (MODE == DOTSOCP_RENDER_LEVELS) {
        const double s = rho * a.k;
        // the number of levels <= s by a branch-free binary search over the padded table: every probe lies in 0 .. 254;
        // an s of +Inf also counts the pad, a NaN counts nothing
        int i = 0;
#pragma unroll
        for (int step = 128; step >= 1; step >>= 1) i += (lev[i + step - 1] <= s) ? step : 0;
        return i < a.nlevels ? i : a.nlevels;
    }
    const double v = (rho / a.vmax) * 256.0;
    const int i = rho > 0.0 ? (v >= 255.0 ? 255 : (int)v) : 0;
    return MODE == DOTSOCP_RENDER_INVERTED ? 255 - i : i;
}

template <bool WEIGHTED, int MODE, int CHANNELS>
__global__ void __launch_bounds__(TILE_Y *TILE_X) k_render(Grid g, RenderArgs a) {
    __shared__ unsigned char s_idx[TILE_Y * RND_PITCH];
    __shared__ double s_lev[MODE == DOTSOCP_RENDER_LEVELS ? RND_LEVELS : 1];
    __shared__ unsigned char s_lut[CHANNELS == 3 ? 768 : 4];
    const int lane = threadIdx.x, xl = threadIdx.y, tid = xl * TILE_Y + lane;
    if (MODE == DOTSOCP_RENDER_LEVELS && tid < RND_LEVELS) s_lev[tid] = tid < a.nlevels ? a.levels[tid] : INFINITY;
    if (CHANNELS == 3)
        for (int j = tid; j < 768; j += TILE_Y * TILE_X) s_lut[j] = a.lut[j];
    if (MODE == DOTSOCP_RENDER_LEVELS) __syncthreads();
    const i64 y0 = (i64)blockIdx.x * TILE_Y, x0 = (i64)blockIdx.y * RND_TX;
    const i64 y = y0 + lane;
    const int tw = (int)(g.nx - x0 < RND_TX ? g.nx - x0 : RND_TX), th = (int)(g.ny - y0 < TILE_Y ? g.ny - y0 : TILE_Y);
    const i64 tg = g.t0 + a.tl;
    if (y < g.ny) {
        for (int xs = xl; xs < tw; xs += TILE_X) {
            const i64 x = x0 + xs, col = y + g.py * x;
            const double rho = out_rho<WEIGHTED>(g, a.o, tg, a.tl, col, col + g.plane * a.tl);
            const bool masked = a.barrier != nullptr && a.barrier[y + g.ny * x] != 0;
            s_idx[lane * RND_PITCH + xs] = (unsigned char)(masked ? a.barrier_index : render_index<MODE>(rho, a, s_lev));
        }
    }
    __syncthreads();
    // the tile's share of image row y0 + yy: tw * CHANNELS consecutive bytes
    const unsigned rowb = (unsigned)tw * CHANNELS, total = (unsigned)th * rowb;
    for (unsigned j = tid; j < total; j += TILE_Y * TILE_X) {
        const unsigned yy = j / rowb, r = j - yy * rowb;
        const unsigned xx = CHANNELS == 3 ? r / 3u : r;
        const unsigned idx = s_idx[yy * RND_PITCH + xx];
        a.image[((y0 + yy) * g.nx + x0) * CHANNELS + r] = CHANNELS == 3 ? s_lut[3u * idx + (r - 3u * xx)] : (unsigned char)idx;
    }
}

template <bool WEIGHTED, int MODE>
static void render_launch(const Grid &g, const RenderArgs &a, int channels, dim3 grid, hipStream_t st) {
    if (channels == 3) DS_KLAUNCH((k_render<WEIGHTED, MODE, 3>), grid, dim3(TILE_Y, TILE_X), 0, st, g, a);
    else DS_KLAUNCH((k_render<WEIGHTED, MODE, 1>), grid, dim3(TILE_Y, TILE_X), 0, st, g, a);
}

int launch_render(const Grid &g, const double *alpha, const double *weight, const double *rho0, const double *rho1,
                  const double *a_prev, double sig, double cD, i64 tl, int mode, int channels, const unsigned char *barrier,
                  const double *levels, int nlevels, const unsigned char *lut, int barrier_index, double vmax,
                  unsigned char *image, hipStream_t st) {
    if (tl < 0 || tl >= g.ntl) { set_error("internal: frame layer outside its slab"); return DOTSOCP_ESTATE; }
    const i64 tiles_x = (g.nx + RND_TX - 1) / RND_TX;
    if (tiles_x > 65535) { set_error("invalid argument: render_evolution() serves up to %d columns", 65535 * RND_TX); return DOTSOCP_EINVAL; }
    RenderArgs a{{nullptr, alpha, weight, rho0, rho1, a_prev, sig, cD, 0.0}, tl, barrier, levels, lut, nlevels, barrier_index,
                 vmax, 255.0 / vmax, image};
    dim3 grid((unsigned)((g.ny + TILE_Y - 1) / TILE_Y), (unsigned)tiles_x, 1);
    const bool w = weight != nullptr;
    switch (mode) {
        case DOTSOCP_RENDER_LINEAR:
            if (w) render_launch<true, DOTSOCP_RENDER_LINEAR>(g, a, channels, grid, st);
            else render_launch<false, DOTSOCP_RENDER_LINEAR>(g, a, channels, grid, st);
            break;
        case DOTSOCP_RENDER_INVERTED:
            if (w) render_launch<true, DOTSOCP_RENDER_INVERTED>(g, a, channels, grid, st);
            else render_launch<false, DOTSOCP_RENDER_INVERTED>(g, a, channels, grid, st);
            break;
        case DOTSOCP_RENDER_LEVELS:
            if (w) render_launch<true, DOTSOCP_RENDER_LEVELS>(g, a, channels, grid, st);
            else render_launch<false, DOTSOCP_RENDER_LEVELS>(g, a, channels, grid, st);
            break;
        default: set_error("internal: unknown render mode"); return DOTSOCP_ESTATE;
    }
    DS_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------
// arrows
// ---------------------------------------------------------------------------------------
#define MV_BLOCK 256

struct MoveArgs {
    OutArgs o;
    i64 tl, skip_y, skip_x, my, mx;
    double thr;                     // vmax * mask_frac
    double *mvX, *mvY;              // [mx][my], y fastest; mvX nullptr: 1-D
};

template <bool WEIGHTED>
__global__ void __launch_bounds__(MV_BLOCK) k_movement(Grid g, MoveArgs a) {
    const i64 p = (i64)blockIdx.x * MV_BLOCK + threadIdx.x;
    if (p >= a.my * a.mx) return;
    const i64 jx = p / a.my, jy = p - jx * a.my;
    const i64 y = jy * a.skip_y, x = jx * a.skip_x;
    const i64 tg = g.t0 + a.tl, col = y + g.py * x;
    const double rho = out_rho<WEIGHTED>(g, a.o, tg, a.tl, col, col + g.plane * a.tl);
    const double f = (tg == 0 || tg == g.nt - 1) ? 2.0 : 1.0;
    const bool small = rho < a.thr;
    if (a.mvX) {
        double Ex = 0.0;
        if (x >= 1 && x <= g.nx - 2) {
            const i64 e = out_edge_x(g, y, x, a.tl);
            Ex = out_flux(out_a<WEIGHTED>(a.o, e - g.py), out_a<WEIGHTED>(a.o, e), f);
        }
        a.mvX[p] = small ? 0.0 : Ex;
    }
    double Ey = 0.0;
    if (y >= 1 && y <= g.ny - 2) {
        const i64 e = out_edge_y(g, y, x, a.tl);
        Ey = out_flux(out_a<WEIGHTED>(a.o, e - 1), out_a<WEIGHTED>(a.o, e), f);
    }
    a.mvY[p] = small ? 0.0 : Ey;
}

int launch_movement(const Grid &g, const double *alpha, const double *weight, const double *rho0, const double *rho1,
                    const double *a_prev, double sig, double cD, i64 tl, i64 skip_y, i64 skip_x, i64 my, i64 mx, double thr,
                    double *mvX, double *mvY, hipStream_t st) {
    if (tl < 0 || tl >= g.ntl) { set_error("internal: arrow layer outside its slab"); return DOTSOCP_ESTATE; }
    if (my * mx <= 0) return 0;
    MoveArgs a{{nullptr, alpha, weight, rho0, rho1, a_prev, sig, cD, 0.0}, tl, skip_y, skip_x, my, mx, thr, mvX, mvY};
    const dim3 grid((unsigned)launch_blocks(my * mx, MV_BLOCK, (i64)1 << 30));
    if (weight) DS_KLAUNCH(k_movement<true>, grid, dim3(MV_BLOCK), 0, st, g, a);
    else DS_KLAUNCH(k_movement<false>, grid, dim3(MV_BLOCK), 0, st, g, a);
    DS_HIP(hipGetLastError());
    return 0;
}

}  // namespace dotsocp
