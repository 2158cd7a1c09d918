// The geodesic's profile (include/dotsocp.h: dotsocp_geodesic_profile): per time node the mass, the first and second
// moments, the momentum, the kinetic energy, the entropy and the squared density of the solved flow, the layer's largest
// density and the size of its support -- from the device-resident alpha (and the weight) in ONE pass; q is not read.
//
// The march is k_report's (report.hip): a workgroup owns a 64 x 4 tile of (y, x) columns and a chunk of node layers, forms
// rho, Ex, Ey with the expressions of k_outputs (outputs_node.h: the same bits), keeps alpha0 of the cell below in a
// register, and issues every load of a step from clamped addresses in one basic block.  Nothing grid-sized is written:
//   * per layer the GEO_SUMS sums and the maximum: wavefront shuffles by 32 .. 1, then the four wavefronts in index order
//     through LDS, one row of partials per (layer, quantity, tile); launch_report_rows adds the tiles of a row.  This is
//     the report's order, step for step: the mass row carries the bits of its layer sums of rho, the kin row those of its
//     cost terms.  A layer lies in exactly one chunk of exactly one slab, so the order depends on (ny, nx) alone;
//   * the maximum over the finite rho goes the same way with fmax for + (exact in any order), the support count as an
//     integer: ballot, four wavefronts, one count per (layer, tile); k_geo_extras combines the tiles of a layer.
// No atomic of any kind.
#include <cmath>

#include "device_utils.h"
#include "kernels.h"
#include "outputs_node.h"

namespace dotsocp {

#define GEO_ROWS (DOTSOCP_GEO_SUMS + 1)     // the sums, then the maximum
#define GEO_GROUPS 16384                    // workgroups a launch aims at (launch_report)

struct GeoArgs {
    OutArgs o;                      // (o.q is not read)
    double floor;                   // DOTSOCP_REPORT_RHO_FLOOR
    int dim1;                       // 1-D problem (ny = nx1d, nx = 1): the only axis is X, the engine's Ey the public Ex
    i64 chunk;                      // node layers per blockIdx.z
    double *partials;               // [ntl][DOTSOCP_GEO_SUMS][tiles]
    double *pmax;                   // [ntl][tiles]
    unsigned long long *pcnt;       // [ntl][tiles]
};

template <bool WEIGHTED>
__global__ void __launch_bounds__(TILE_Y *TILE_X) k_geodesic(Grid g, GeoArgs a) {
    __shared__ double s_red[2][TILE_X][GEO_ROWS];
    __shared__ unsigned int s_cnt[2][TILE_X];
    const int lane = threadIdx.x, xl = threadIdx.y, tid = xl * TILE_Y + lane;
    const i64 y = (i64)blockIdx.x * TILE_Y + lane;
    const i64 x = (i64)blockIdx.y * TILE_X + xl;
    const bool inb = (y < g.ny) && (x < g.nx);
    const bool hasX = inb && x >= 1 && x <= g.nx - 2, hasY = inb && y >= 1 && y <= g.ny - 2;
    const i64 tbeg = (i64)blockIdx.z * a.chunk;
    const i64 tend = (tbeg + a.chunk < g.ntl) ? tbeg + a.chunk : g.ntl;
    const i64 tiles = (i64)gridDim.x * gridDim.y, tile = blockIdx.x + (i64)gridDim.x * blockIdx.y;
    const OutArgs &o = a.o;
    // the node's coordinates in the unit square (include/dotsocp.h): the engine's x is the public X, its y the public Y; a
    // 1-D problem lives in the engine's y
    const double X = a.dim1 ? (double)y / (double)(g.ny - 1) : (double)x / (double)(g.nx - 1);
    const double Y = a.dim1 ? 0.0 : (double)y / (double)(g.ny - 1);
    // Every lane loads on every step, from its own entry or -- outside the grid, on the x / y boundary, above the last cell
    // layer -- from `safe`, an entry that always exists (alpha0 of the slab's first cell layer); what such a load returns is
    // never used (report.hip)
    const i64 col = inb ? y + g.py * x : 0, safe = col;
    const i64 ex0 = hasX ? out_edge_x(g, y, x, 0) : safe, exs = hasX ? g.bxLayer : 0, exd = hasX ? g.py : 0;
    const i64 ey0 = hasY ? out_edge_y(g, y, x, 0) : safe, eys = hasY ? g.byLayer : 0, eyd = hasY ? 1 : 0;
    double a_below;                                 // a(.) of cell t - 1
    {
        const double ab = out_a<WEIGHTED>(o, tbeg > 0 ? col + g.plane * (tbeg - 1) : safe);
        const double ap = g.first ? 0.0 : o.a_prev[col];
        a_below = tbeg > 0 ? ab : ap;
    }
    int par = 0;
    for (i64 tl = tbeg; tl < tend; ++tl) {
        const i64 tg = g.t0 + tl;
        const bool ends = (tg == 0 || tg == g.nt - 1), cell = tl < g.ncl;
        // ---- all loads of the step ----
        const i64 node = cell ? col + g.plane * tl : safe;
        const i64 ax = ex0 + exs * tl, ay = ey0 + eys * tl;                 // alpha edges of node layer tl (always owned)
        const double a_here = out_a<WEIGHTED>(o, node);
        const double axl = out_a<WEIGHTED>(o, ax - exd), axh = out_a<WEIGHTED>(o, ax);
        const double ayl = out_a<WEIGHTED>(o, ay - eyd), ayh = out_a<WEIGHTED>(o, ay);
        const double r_end = ends ? (tg == 0 ? o.rho0 : o.rho1)[col] : 0.0;
        // ---- node: rho, Ex, Ey ----
        const double rho = ends ? r_end : out_mean2(a_below, cell ? a_here : 0.0);
        a_below = a_here;
        const double f = ends ? 2.0 : 1.0;
        const double Ex = hasX ? out_flux(axl, axh, f) : 0.0, Ey = hasY ? out_flux(ayl, ayh, f) : 0.0;
        // ---- the terms of include/dotsocp.h, zero outside the grid ----
        double v[GEO_ROWS];
#pragma unroll
        for (int i = 0; i < DOTSOCP_GEO_SUMS; ++i) v[i] = 0.0;
        v[DOTSOCP_GEO_SUMS] = -INFINITY;
        bool above = false;
        if (inb) {
            const double rX = rho * X, rY = a.dim1 ? 0.0 : rho * Y;
            v[0] = rho;
            v[1] = rX;
            v[2] = rY;
            v[3] = rX * X;
            v[4] = a.dim1 ? 0.0 : rY * Y;
            v[5] = a.dim1 ? 0.0 : rX * Y;
            v[6] = a.dim1 ? Ey : Ex;
            v[7] = a.dim1 ? 0.0 : Ey;
            above = rho > a.floor;
            if (above) v[8] = (Ex * Ex + Ey * Ey) / rho;                    // (the report's cost term)
            if (rho > 0.0) v[9] = rho * log(rho);
            v[10] = rho * rho;
            if (isfinite(rho)) v[DOTSOCP_GEO_SUMS] = rho + 0.0;             // (+ 0.0: a -0.0 counts as the +0.0 it equals)
        }
        // ---- the layer sums of this tile: lanes, then wavefronts, always in the same order ----
#pragma unroll
        for (int i = 0; i < GEO_ROWS; ++i) {
            double w = v[i];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double u = __shfl_down(w, off, 64);
                w = (i < DOTSOCP_GEO_SUMS) ? w + u : fmax(w, u);
            }
            if (lane == 0) s_red[par][xl][i] = w;
        }
        const unsigned long long votes = __ballot(above);
        if (lane == 0) s_cnt[par][xl] = (unsigned int)__popcll(votes);
        __syncthreads();            // (s_red[par] is written again two layers on, behind the barrier of the next one)
        if (tid < GEO_ROWS) {
            double w = s_red[par][0][tid];
#pragma unroll
            for (int wv = 1; wv < TILE_X; ++wv) w = (tid < DOTSOCP_GEO_SUMS) ? w + s_red[par][wv][tid] : fmax(w, s_red[par][wv][tid]);
            if (tid < DOTSOCP_GEO_SUMS) a.partials[(tl * DOTSOCP_GEO_SUMS + tid) * tiles + tile] = w;
            else a.pmax[tl * tiles + tile] = w;
        } else if (tid == GEO_ROWS) {
            unsigned long long c = 0;
#pragma unroll
            for (int wv = 0; wv < TILE_X; ++wv) c += s_cnt[par][wv];
            a.pcnt[tl * tiles + tile] = c;
        }
        par ^= 1;
    }
}

// one workgroup per layer: omax[layer] = the maximum, ocnt[layer] = the sum over the layer's tiles (exact in any order)
__global__ void __launch_bounds__(256) k_geo_extras(const double *__restrict__ pmax, const unsigned long long *__restrict__ pcnt,
                                                    i64 tiles, double *__restrict__ omax, unsigned long long *__restrict__ ocnt) {
    const double *pm = pmax + (i64)blockIdx.x * tiles;
    const unsigned long long *pc = pcnt + (i64)blockIdx.x * tiles;
    double m = -INFINITY;
    unsigned long long c = 0;
    for (i64 b = threadIdx.x; b < tiles; b += 256) {
        m = fmax(m, pm[b]);
        c += pc[b];
    }
    __shared__ double rm[256];
    __shared__ unsigned long long rc[256];
    rm[threadIdx.x] = m;
    rc[threadIdx.x] = c;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) {
            rm[threadIdx.x] = fmax(rm[threadIdx.x], rm[threadIdx.x + off]);
            rc[threadIdx.x] += rc[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        omax[blockIdx.x] = rm[0];
        ocnt[blockIdx.x] = rc[0];
    }
}

i64 geodesic_doubles(const Grid &g) { return (i64)GEO_ROWS * g.ntl * (report_tiles(g) + 1); }
i64 geodesic_counts(const Grid &g) { return g.ntl * (report_tiles(g) + 1); }

int launch_geodesic(const Grid &g, const double *alpha, const double *weight, const double *rho0, const double *rho1,
                    const double *a_prev, double sig, double cD, bool dim1, double *buf, unsigned long long *cnt, hipStream_t st) {
    if (g.ntl <= 0) return 0;
    const i64 tiles = report_tiles(g), rows = DOTSOCP_GEO_SUMS * g.ntl;
    // buf: [partials: rows x tiles | pmax: ntl x tiles | sums: rows | max: ntl], cnt: [ntl x tiles | ntl]
    double *partials = buf, *pmax = partials + rows * tiles, *sums = pmax + g.ntl * tiles, *omax = sums + rows;
    GeoArgs a{{nullptr, alpha, weight, rho0, rho1, a_prev, sig, cD, 0.0}, DOTSOCP_REPORT_RHO_FLOOR, dim1 ? 1 : 0, 0, partials, pmax, cnt};
    // the chunks of launch_report: enough workgroups to fill the device evenly, few re-read layers, gridDim.z below its limit
    i64 chunks = (GEO_GROUPS + tiles - 1) / tiles;
    if (chunks > g.ntl) chunks = g.ntl;
    a.chunk = (g.ntl + chunks - 1) / chunks;
    chunks = (g.ntl + a.chunk - 1) / a.chunk;
    dim3 grid((unsigned)((g.ny + TILE_Y - 1) / TILE_Y), (unsigned)((g.nx + TILE_X - 1) / TILE_X), (unsigned)chunks);
    if (weight) DS_KLAUNCH(k_geodesic<true>, grid, dim3(TILE_Y, TILE_X), 0, st, g, a);
    else DS_KLAUNCH(k_geodesic<false>, grid, dim3(TILE_Y, TILE_X), 0, st, g, a);
    DS_CHECK(launch_report_rows(partials, tiles, rows, sums, st));
    DS_KLAUNCH(k_geo_extras, dim3((unsigned)g.ntl), dim3(256), 0, st, (const double *)pmax, (const unsigned long long *)cnt, tiles, omax,
               cnt + g.ntl * tiles);
    DS_HIP(hipGetLastError());
    return 0;
}

}  // namespace dotsocp
