// Solution report (include/dotsocp.h: dotsocp_solution_report): what the reference's demos compute from the downloaded
// outputs -- check_massConservation.m:16-27, hist_negative_density.m:14, hist_violation_q_{1d,2d}.m:4 over the bins of
// hist_positive_value.m:28-55, and the transport cost -- from the device-resident alpha and q in ONE pass.
//
// A workgroup owns a 64 x 4 tile of (y, x) columns and marches over a chunk of time layers.  Per node layer it forms
// rho, Ex, Ey and per cell layer q0, bx, by with the expressions of k_outputs (outputs_node.h: the same bits); alpha0 of
// the cell below and the x / y averages of the upper edge layer stay in registers for the next step, so every entry of
// alpha, the weight and q is requested from memory once (the x / y neighbours of an edge come out of the cache).
// Nothing grid-sized is written:
//   * per layer: the sums of rho, min(rho, 0) and the cost terms -- wavefront shuffles, then the four wavefronts through
//     LDS, one row of three partial sums per (layer, tile); k_report_final adds the tiles of a layer in index order.  A
//     layer lies in exactly one chunk of exactly one slab, so the order depends on (ny, nx) alone: no pitch, no slab
//     count and no chunk length changes a bit, and there is no floating-point atomic anywhere;
//   * per workgroup: the two 49-bin histograms and the counts in LDS counters, min(rho) / max(fq) as order-preserving
//     integer keys; flushed once with 64-bit integer atomics (integer sums and maxima do not depend on the order).
#include <cmath>
#include <cstring>

#include "device_utils.h"
#include "kernels.h"
#include "outputs_node.h"

namespace dotsocp {

#define REP_EDGES (DOTSOCP_REPORT_BINS + 1)

// 10.^linspace(-8, -1, 50): the exponents as linspace forms them (start + j * step, the last one the end point itself)
void report_edges_host(double edges[REP_EDGES]) {
    const double start = -8.0, stop = -1.0, step = (stop - start) / DOTSOCP_REPORT_BINS;
    for (int j = 0; j < REP_EDGES; ++j) edges[j] = pow(10.0, j == DOTSOCP_REPORT_BINS ? stop : j * step + start);
}

// the inverse of report_key (device_utils.h); `none`: what a zeroed slot stands for
double report_key_decode(unsigned long long key, bool inverted, double none) {
    if (key == 0) return none;
    if (inverted) key = ~key;
    const unsigned long long b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
    double v;
    memcpy(&v, &b, sizeof v);
    return v;
}

#define REP_GROUPS 16384            // workgroups a launch aims at (256 CUs x 8 resident x 8 rounds)

struct ReportArgs {
    OutArgs o;
    const double *edges;            // REP_EDGES doubles
    double floor;                   // DOTSOCP_REPORT_RHO_FLOOR
    int dim1;                       // 1-D problem (ny = nx1d, nx = 1): fq with |bx| where the 2-D formula has the square root
    i64 chunk;                      // node layers per blockIdx.z
    double *partials;               // [ntl][3][tiles]
    unsigned long long *counts;     // [RC_COUNT]
};

template <bool WEIGHTED>
__global__ void __launch_bounds__(TILE_Y *TILE_X) k_report(Grid g, ReportArgs a) {
    __shared__ double s_edges[REP_EDGES];
    __shared__ unsigned int s_hist[2 * DOTSOCP_REPORT_BINS + 3];      // RC_RHO_HIST .. RC_NONFINITE
    __shared__ unsigned long long s_key[2];
    __shared__ double s_red[2][TILE_X][3];
    const int lane = threadIdx.x, xl = threadIdx.y, tid = xl * TILE_Y + lane;
    if (tid < REP_EDGES) s_edges[tid] = a.edges[tid];
    if (tid < 2 * DOTSOCP_REPORT_BINS + 3) s_hist[tid] = 0;
    if (tid < 2) s_key[tid] = 0;
    __syncthreads();
    const i64 y = (i64)blockIdx.x * TILE_Y + lane;
    const i64 x = (i64)blockIdx.y * TILE_X + xl;
    const bool inb = (y < g.ny) && (x < g.nx);
    const bool hasX = inb && x >= 1 && x <= g.nx - 2, hasY = inb && y >= 1 && y <= g.ny - 2;
    const i64 tbeg = (i64)blockIdx.z * a.chunk;
    const i64 tend = (tbeg + a.chunk < g.ntl) ? tbeg + a.chunk : g.ntl;
    const i64 tiles = (i64)gridDim.x * gridDim.y, tile = blockIdx.x + (i64)gridDim.x * blockIdx.y;
    const OutArgs &o = a.o;
    // Every lane loads on every step, from its own entry or -- outside the grid, on the x / y boundary, above the last cell
    // layer -- from `safe`, an entry that always exists (alpha0 / q0 of the slab's first cell layer; there is at least
    // one); what such a load returns is never used.  The ten (weighted: fifteen) loads of a step thus stand in one basic
    // block and are issued together instead of one memory round trip after the other.
    const i64 col = inb ? y + g.py * x : 0, safe = col;
    const i64 ex0 = hasX ? out_edge_x(g, y, x, 0) : safe, exs = hasX ? g.bxLayer : 0, exd = hasX ? g.py : 0;
    const i64 ey0 = hasY ? out_edge_y(g, y, x, 0) : safe, eys = hasY ? g.byLayer : 0, eyd = hasY ? 1 : 0;
    double a_below = 0.0, mx = 0.0, my = 0.0;       // a(.) of cell t - 1; x / y averages of the b edges of layer t
    {
        const bool head = tbeg < g.ncl;             // the chunk starts on a cell layer
        const i64 ex = head ? ex0 + exs * tbeg : safe, ey = head ? ey0 + eys * tbeg : safe;
        const double ab = out_a<WEIGHTED>(o, tbeg > 0 ? col + g.plane * (tbeg - 1) : safe);
        const double ap = g.first ? 0.0 : o.a_prev[col];
        const double bxl = out_b(o, ex - (head ? exd : 0)), bxh = out_b(o, ex);
        const double byl = out_b(o, ey - (head ? eyd : 0)), byh = out_b(o, ey);
        a_below = tbeg > 0 ? ab : ap;
        mx = hasX ? out_mean2(bxl, bxh) : 0.0;
        my = hasY ? out_mean2(byl, byh) : 0.0;
    }
    unsigned int n_neg = 0, n_pos = 0, n_bad = 0;
    double rmin = INFINITY, fmax = -INFINITY;
    int par = 0;
    for (i64 tl = tbeg; tl < tend; ++tl) {
        const i64 tg = g.t0 + tl;
        const bool ends = (tg == 0 || tg == g.nt - 1), cell = tl < g.ncl;
        // ---- all loads of the step ----
        const i64 node = cell ? col + g.plane * tl : safe;
        const i64 ax = ex0 + exs * tl, ay = ey0 + eys * tl;                 // alpha edges of node layer tl (always owned)
        const i64 qx = cell ? ex0 + exs * (tl + 1) : safe, qy = cell ? ey0 + eys * (tl + 1) : safe;   // b edges of layer tl + 1
        const i64 qxd = cell ? exd : 0, qyd = cell ? eyd : 0;
        const double a_here = out_a<WEIGHTED>(o, node);
        const double axl = out_a<WEIGHTED>(o, ax - exd), axh = out_a<WEIGHTED>(o, ax);
        const double ayl = out_a<WEIGHTED>(o, ay - eyd), ayh = out_a<WEIGHTED>(o, ay);
        const double q0 = out_b(o, node);
        const double bxl = out_b(o, qx - qxd), bxh = out_b(o, qx);
        const double byl = out_b(o, qy - qyd), byh = out_b(o, qy);
        const double r_end = ends ? (tg == 0 ? o.rho0 : o.rho1)[col] : 0.0;
        // ---- node: rho, Ex, Ey ----
        const double rho = ends ? r_end : out_mean2(a_below, cell ? a_here : 0.0);
        a_below = a_here;
        const double f = ends ? 2.0 : 1.0;
        const double Ex = hasX ? out_flux(axl, axh, f) : 0.0, Ey = hasY ? out_flux(ayl, ayh, f) : 0.0;
        double s_mass = 0.0, s_neg = 0.0, s_cost = 0.0;
        if (inb) {
            if (isfinite(rho)) rmin = fmin(rmin, rho + 0.0);          // (+ 0.0: a -0.0 counts as the +0.0 it equals)
            else ++n_bad;
            if (rho < 0.0) { ++n_neg; s_neg = rho; }
            s_mass = rho;
            if (rho > a.floor) s_cost = (Ex * Ex + Ey * Ey) / rho;
            const int jr = report_bin(s_edges, -rho);
            if (jr >= 0) atomicAdd(&s_hist[RC_RHO_HIST + jr], 1u);
        }
        // ---- cell: q0, bx, by, fq ----
        const double m1x = out_mean2(bxl, bxh), m1y = out_mean2(byl, byh);
        const double bx = hasX ? out_mean2(mx, m1x) : 0.0, by = hasY ? out_mean2(my, m1y) : 0.0;
        mx = m1x;
        my = m1y;
        if (inb && cell) {
            double fq;
            if (a.dim1) fq = (q0 + .5 * (by * by)) / (1.0 + fabs(q0) + fabs(by));
            else fq = (q0 + .5 * (bx * bx + by * by)) / (1.0 + fabs(q0) + sqrt(bx * bx + by * by));
            if (isfinite(fq)) fmax = fmax > fq + 0.0 ? fmax : fq + 0.0;
            else ++n_bad;
            if (fq > 0.0) ++n_pos;
            const int jq = report_bin(s_edges, fq);
            if (jq >= 0) atomicAdd(&s_hist[RC_FQ_HIST + jq], 1u);
        }
        // ---- the three layer sums of this tile: lanes, then wavefronts, always in the same order ----
        double v3[3] = {s_mass, s_neg, s_cost};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double v = v3[i];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) s_red[par][xl][i] = v;
        }
        __syncthreads();            // (s_red[par] is written again two layers on, behind the barrier of the next one)
        if (tid < 3) {
            double v = s_red[par][0][tid];
#pragma unroll
            for (int wv = 1; wv < TILE_X; ++wv) v += s_red[par][wv][tid];
            a.partials[(tl * 3 + tid) * tiles + tile] = v;
        }
        par ^= 1;
    }
    // ---- counts and extrema: threads -> LDS -> one 64-bit integer atomic per slot and workgroup ----
    if (n_neg) atomicAdd(&s_hist[RC_RHO_NEG], n_neg);
    if (n_pos) atomicAdd(&s_hist[RC_FQ_POS], n_pos);
    if (n_bad) atomicAdd(&s_hist[RC_NONFINITE], n_bad);
    if (rmin < INFINITY) atomicMax(&s_key[0], ~report_key(rmin));
    if (fmax > -INFINITY) atomicMax(&s_key[1], report_key(fmax));
    __syncthreads();
    if (tid < 2 * DOTSOCP_REPORT_BINS + 3) {
        if (s_hist[tid]) atomicAdd(&a.counts[tid], (unsigned long long)s_hist[tid]);
    } else if (tid < 2 * DOTSOCP_REPORT_BINS + 5) {
        const int k = tid - (2 * DOTSOCP_REPORT_BINS + 3);
        if (s_key[k]) atomicMax(&a.counts[RC_RHO_MIN + k], s_key[k]);
    }
}

// sums[row] = partials[row][0] + ... + partials[row][tiles - 1], always by the same tree (row = 3 * layer + quantity)
__global__ void __launch_bounds__(256) k_report_final(const double *__restrict__ partials, i64 tiles, double *__restrict__ sums) {
    const double *p = partials + (i64)blockIdx.x * tiles;
    double v = 0.0;
    for (i64 b = threadIdx.x; b < tiles; b += 256) v += p[b];
    __shared__ double red[256];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = red[0];
}

int launch_report_rows(const double *partials, i64 tiles, i64 rows, double *sums, hipStream_t st) {
    if (rows <= 0) return 0;
    DS_KLAUNCH(k_report_final, dim3((unsigned)rows), dim3(256), 0, st, partials, tiles, sums);
    DS_HIP(hipGetLastError());
    return 0;
}

i64 report_tiles(const Grid &g) { return ((g.ny + TILE_Y - 1) / TILE_Y) * ((g.nx + TILE_X - 1) / TILE_X); }

int launch_report(const Grid &g, const double *q, const double *alpha, const double *weight, const double *rho0,
                  const double *rho1, const double *a_prev, double sig, double cD, double dD, bool dim1, const double *edges,
                  double *partials, double *sums, unsigned long long *counts, hipStream_t st) {
    if (g.ntl <= 0) return 0;
    ReportArgs a{{q, alpha, weight, rho0, rho1, a_prev, sig, cD, dD}, edges, DOTSOCP_REPORT_RHO_FLOOR, dim1 ? 1 : 0, 0,
                 partials, counts};
    // enough workgroups to fill the device evenly, few re-read layers (a chunk reads one alpha0 layer and one layer of b
    // edges that its neighbour reads too: 3 % at 32 layers per chunk); at most REP_GROUPS chunks, so gridDim.z stays below
    // its limit of 65535 on every grid
    const i64 tiles = report_tiles(g);
    i64 chunks = (REP_GROUPS + tiles - 1) / tiles;
    if (chunks > g.ntl) chunks = g.ntl;
    a.chunk = (g.ntl + chunks - 1) / chunks;
    chunks = (g.ntl + a.chunk - 1) / a.chunk;
    dim3 grid((unsigned)((g.ny + TILE_Y - 1) / TILE_Y), (unsigned)((g.nx + TILE_X - 1) / TILE_X), (unsigned)chunks);
    if (weight) DS_KLAUNCH(k_report<true>, grid, dim3(TILE_Y, TILE_X), 0, st, g, a);
    else DS_KLAUNCH(k_report<false>, grid, dim3(TILE_Y, TILE_X), 0, st, g, a);
    DS_KLAUNCH(k_report_final, dim3((unsigned)(3 * g.ntl)), dim3(256), 0, st, (const double *)partials, tiles, sums);
    DS_HIP(hipGetLastError());
    return 0;
}

}  // namespace dotsocp
