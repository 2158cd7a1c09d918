// Matrix-free staggered-gradient stencils of the loop, one entry per thread: rhs = A'(w.*q - alpha) + c and the
// q-step / alpha-update (the marching q-step kernels of the fused dataflow: qstep_march.hip).
// A = D * [Dt; Dx; Dy] are forward differences
// (socp/dot2d/utils/initialize.m:35-39,67-87, scaled by D in solver_dotsocp2d.m:338);
// summation orders follow the column/row order of the reference's sparse products
//  so that results agree with the oracle to the last bit.
#include "device_utils.h"
#include "gather_tile.h"
#include "kernels.h"

#include <cstdlib>

namespace dotsocp {

static inline dim3 tile_grid(const Grid &g, i64 layers) {
    return dim3((unsigned)((g.ny + TILE_Y - 1) / TILE_Y), (unsigned)((g.nx + TILE_X - 1) / TILE_X), (unsigned)layers);
}

// ---------------------------------------------------------------------------------------
// rhs(y,x,t) = sum over the (up to) six staggered neighbours, Neumann: missing ones dropped
// (solver_socp_inPALM.m:194; weighted: solver_wsocp_inPALM.m:200)
// ---------------------------------------------------------------------------------------
template <bool WEIGHTED>
__global__ void __launch_bounds__(TILE_Y *TILE_X) k_rhs(RhsArgs a, double *__restrict__ rhs) {
    const i64 y = (i64)blockIdx.x * TILE_Y + threadIdx.x;
    const i64 x = (i64)blockIdx.y * TILE_X + threadIdx.y;
    const i64 tl = blockIdx.z;
    if (y >= a.g.ny || x >= a.g.nx) return;
    rhs[y + a.g.py * (x + a.g.nx * tl)] = rhs_value<WEIGHTED>(a, y, x, tl);
}

int launch_rhs(const Grid &g, const LoopCoef &c, const double *q, const double *alpha, const double *cvec,
               const double *weight, const double *u0_prev, double *rhs, hipStream_t st, bool c_ends) {
    if (g.Nphi <= 0) return 0;
    RhsArgs a{g, c.at, c.ax, c.ay, q, alpha, cvec, weight, u0_prev, c_ends ? 1 : 0};
    if (weight)
        DS_KLAUNCH(k_rhs<true>, tile_grid(g, g.ntl), dim3(TILE_Y, TILE_X), 0, st, a, rhs);
    else
        DS_KLAUNCH(k_rhs<false>, tile_grid(g, g.ntl), dim3(TILE_Y, TILE_X), 0, st, a, rhs);
    DS_HIP(hipGetLastError());
    return 0;
}

template <bool WEIGHTED>
__global__ void __launch_bounds__(TILE_Y *TILE_X) k_u0_tail(Grid g, const double *__restrict__ q,
                                                             const double *__restrict__ alpha,
                                                             const double *__restrict__ weight,
                                                             double *__restrict__ out) {
    const i64 y = (i64)blockIdx.x * TILE_Y + threadIdx.x;
    const i64 x = (i64)blockIdx.y * TILE_X + threadIdx.y;
    if (y >= g.ny || x >= g.nx) return;
    const i64 k = y + g.py * (x + g.nx * (g.ncl - 1));
    out[y + g.py * x] = WEIGHTED ? weight[k] * q[k] - alpha[k] : q[k] - alpha[k];
}

int launch_u0_tail(const Grid &g, const double *q, const double *alpha, const double *weight, double *out,
                   hipStream_t st) {
    if (g.ncl <= 0) return 0;
    if (weight)
        DS_KLAUNCH(k_u0_tail<true>, tile_grid(g, 1), dim3(TILE_Y, TILE_X), 0, st, g, q, alpha, weight, out);
    else
        DS_KLAUNCH(k_u0_tail<false>, tile_grid(g, 1), dim3(TILE_Y, TILE_X), 0, st, g, q, alpha, weight, out);
    DS_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------
// q-step and alpha update, one staggered entry per thread:
//   tmp = (A phi)_k ; q2 = (F* B* (z + beta))_k
//   q_k = (w_k (tmp + alpha_k) + q2) * diagQInv_k          (solver_socp_inPALM.m:204-206; w: :212)
//   alpha_k += tau (tmp - w_k q_k)                           (:211,214; w: :217)
// diagQInv = 1 ./ oper_q  (socp/dot2d/utils/oper_q.m:13-26, wdot2d/utils/oper_q.m:15-28)
// ---------------------------------------------------------------------------------------
struct WSum {
    const double *z, *b;
    i64 Nz;
    __device__ __forceinline__ double operator()(int j, i64 cell) const { return z[j * Nz + cell] + b[j * Nz + cell]; }
};

// inPALM / ALG2: alpha += tau (A phi - w q)
template <bool WEIGHTED>
__device__ __forceinline__ void q_update(const LoopCoef &c, double tmp, double q2, double diag_c, double dinv, i64 k,
                                         const double *__restrict__ weight, double *__restrict__ q, double *alpha) {
    const double a = alpha[k];
    double qn, r;
    if (WEIGHTED) {
        const double w = weight[k];
        const double di = 1.0 / (diag_c + w * w);
        qn = (w * (tmp + a) + q2) * di;
        r = tmp - w * qn;
    } else {
        qn = (tmp + a + q2) * dinv;
        r = tmp - qn;
    }
    q[k] = qn;
    alpha[k] = a + c.tau * r;
}

template <bool WEIGHTED, int SEG>
__global__ void __launch_bounds__(TILE_Y *TILE_X) k_qstep(Grid g, LoopCoef c, const double *__restrict__ phi,
                                                           const double *__restrict__ z,
                                                           const double *__restrict__ beta,
                                                           const double *__restrict__ weight,
                                                           const double *__restrict__ tail_bx,
                                                           const double *__restrict__ tail_by,
                                                           double *__restrict__ q, double *__restrict__ alpha) {
    const i64 y = (i64)blockIdx.x * TILE_Y + threadIdx.x;
    const i64 x = (i64)blockIdx.y * TILE_X + threadIdx.y;
    const i64 tl = blockIdx.z;
    WSum W{z, beta, g.Nc};
    const i64 node = y + g.py * (x + g.nx * tl);
    if (SEG == 0) {
        if (y >= g.ny || x >= g.nx) return;
        const double tmp = fwd_diff(c.at, phi[node], phi[node + g.plane]);
        const double q2 = c.s * (W(9, node) - W(0, node));
        q_update<WEIGHTED>(c, tmp, q2, c.c1, c.dinv1, node, weight, q, alpha);
    } else {
        const bool tbnd = (g.t0 + tl == 0) || (g.t0 + tl == g.nt - 1);
        const double dc = tbnd ? c.c2 : c.c1;
        const double di = tbnd ? c.dinv2 : c.dinv1;
        if (SEG == 1) {
            if (y >= g.ny || x >= g.nx - 1) return;
            const double tmp = fwd_diff(c.ax, phi[node], phi[node + g.py]);
            const double q2 = c.sf * gather_bx(g, W, y, x, tl, tail_bx);
            q_update<WEIGHTED>(c, tmp, q2, dc, di, bx_index(g, y, x, tl), weight, q, alpha);
        } else {
            if (y >= g.ny - 1 || x >= g.nx) return;
            const double tmp = fwd_diff(c.ay, phi[node], phi[node + 1]);
            const double q2 = c.sf * gather_by(g, W, y, x, tl, tail_by);
            q_update<WEIGHTED>(c, tmp, q2, dc, di, by_index(g, y, x, tl), weight, q, alpha);
        }
    }
}

template <bool WEIGHTED>
static int launch_qstep_t(const Grid &g, const LoopCoef &c, const double *phi, const double *z, const double *beta,
                          const double *weight, const double *tail_bx, const double *tail_by, double *q,
                          double *alpha, hipStream_t st) {
    dim3 blk(TILE_Y, TILE_X);
    if (g.Nz > 0)
        DS_KLAUNCH((k_qstep<WEIGHTED, 0>), tile_grid(g, g.ncl), blk, 0, st, g, c, phi, z, beta, weight, tail_bx,
                           tail_by, q, alpha);
    if (g.bxLayer > 0)
        DS_KLAUNCH((k_qstep<WEIGHTED, 1>), tile_grid(g, g.ntl), blk, 0, st, g, c, phi, z, beta, weight, tail_bx,
                           tail_by, q, alpha);
    if (g.byLayer > 0)
        DS_KLAUNCH((k_qstep<WEIGHTED, 2>), tile_grid(g, g.ntl), blk, 0, st, g, c, phi, z, beta, weight, tail_bx,
                           tail_by, q, alpha);
    DS_HIP(hipGetLastError());
    return 0;
}

int launch_qstep(const Grid &g, const LoopCoef &c, const double *phi, const double *z, const double *beta,
                 const double *weight, const double *tail_bx, const double *tail_by, double *q, double *alpha,
                 hipStream_t st) {
    return weight ? launch_qstep_t<true>(g, c, phi, z, beta, weight, tail_bx, tail_by, q, alpha, st)
                  : launch_qstep_t<false>(g, c, phi, z, beta, weight, tail_bx, tail_by, q, alpha, st);
}

// q-step on the adjoint sums produced by the fused cone kernel (fused.hip): q2 already holds
// sf * sum for tile-interior edges and the own tile's raw partial for tile-boundary edges.
// One launch for all three kinds of entries: the thread of node (y, x, tl) owns the q0 entry of
// the cell that starts there and the bx / by edges that leave it; phi(node) is loaded once
template <bool WEIGHTED>
__global__ void __launch_bounds__(TILE_Y *TILE_X) k_qstep_fused(Grid g, LoopCoef c, FusedGeom fg,
                                                                 const double *__restrict__ phi,
                                                                 const double *__restrict__ q2v,
                                                                 const double *__restrict__ sx,
                                                                 const double *__restrict__ sy,
                                                                 const double *__restrict__ weight,
                                                                 const double *__restrict__ tail_bx,
                                                                 const double *__restrict__ tail_by,
                                                                 double *__restrict__ q, double *alpha) {
    const i64 y = (i64)blockIdx.x * TILE_Y + threadIdx.x;
    const i64 x = (i64)blockIdx.y * TILE_X + threadIdx.y;
    const i64 tl = blockIdx.z;
    const i64 node = y + g.py * (x + g.nx * tl);
    if (y >= g.ny || x >= g.nx) return;
    const double p0 = phi[node];
    if (tl < g.ncl) {
        const double tmp = fwd_diff(c.at, p0, phi[node + g.plane]);
        q_update<WEIGHTED>(c, tmp, q2v[node], c.c1, c.dinv1, node, weight, q, alpha);
    }
    const bool tbnd = (g.t0 + tl == 0) || (g.t0 + tl == g.nt - 1);
    const double dc = tbnd ? c.c2 : c.c1;
    const double di = tbnd ? c.dinv2 : c.dinv1;
    if (x < g.nx - 1) {
        const i64 e = bx_index(g, y, x, tl);
        const double tmp = fwd_diff(c.ax, p0, phi[node + g.py]);
        double q2 = q2v[e];
        if (sx_split(fg, x)) q2 = c.sf * (q2 + sx[sx_index(g, fg, y, x, tl)]);
        if (tl == 0 && !g.first) q2 += tail_bx[y + g.py * x];          // left slab's part, already times sf
        q_update<WEIGHTED>(c, tmp, q2, dc, di, e, weight, q, alpha);
    }
    if (y < g.ny - 1) {
        const i64 e = by_index(g, y, x, tl);
        const double tmp = fwd_diff(c.ay, p0, phi[node + 1]);
        double q2 = q2v[e];
        if (sy_split(y)) q2 = c.sf * (q2 + sy[sy_index(g, fg, y, x, tl)]);
        if (tl == 0 && !g.first) q2 += tail_by[y + g.pyb * x];
        q_update<WEIGHTED>(c, tmp, q2, dc, di, e, weight, q, alpha);
    }
}

int launch_qstep_fused(const Grid &g, const LoopCoef &c, const FusedGeom &fg, const double *phi, const double *q2,
                       const double *sx, const double *sy, const double *weight, const double *tail_bx,
                       const double *tail_by, double *q_out, double *alpha, hipStream_t st) {
    dim3 blk(TILE_Y, TILE_X);
    if (weight)
        DS_KLAUNCH(k_qstep_fused<true>, tile_grid(g, g.ntl), blk, 0, st, g, c, fg, phi, q2, sx, sy, weight, tail_bx, tail_by,
                   q_out, alpha);
    else
        DS_KLAUNCH(k_qstep_fused<false>, tile_grid(g, g.ntl), blk, 0, st, g, c, fg, phi, q2, sx, sy, weight, tail_bx, tail_by,
                   q_out, alpha);
    DS_HIP(hipGetLastError());
    return 0;
}

// After a sigma update (alpha, c <- / factor, solver_socp_inPALM.m:312-314) the right-hand side A'(w.*q - alpha) + c the
// q-step left behind becomes  A'(w.*q) - (A' alpha - c) / factor = (rhs + r) - r / factor  with the r = A' alpha - c the
// KKT variant of the q-step stored; c is divided on the way (alpha stays pending: APend).
// c is divided in [0, c_lo) and [c_hi, n) only: everything (c_lo = n), or the end layers a slab holds when the rest of c is
// known to be zero (Slab::c_ends).
__global__ void __launch_bounds__(256) k_rhs_sigma_fix(double *__restrict__ rhs, const double *__restrict__ r,
                                                        double *__restrict__ cvec, i64 n, double factor, i64 c_lo, i64 c_hi) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
        const double rv = r[i];
        rhs[i] = (rhs[i] + rv) - rv / factor;
        if (i < c_lo || i >= c_hi) cvec[i] = cvec[i] / factor;
    }
}

// the index range of c that holds no global end layer: [c_lo, c_hi)
static inline void c_interior(const Grid &g, i64 &c_lo, i64 &c_hi) {
    c_lo = g.first ? g.plane : 0;
    c_hi = g.last ? g.Nphi - g.plane : g.Nphi;
    if (c_hi < c_lo) c_hi = c_lo;
}

int launch_rhs_sigma_fix(const Grid &g, double *rhs, const double *r, double *cvec, double factor, hipStream_t st,
                         bool c_ends) {
    const i64 n = g.Nphi;
    if (n <= 0) return 0;
    i64 c_lo = n, c_hi = n;
    if (c_ends) c_interior(g, c_lo, c_hi);
    DS_KLAUNCH(k_rhs_sigma_fix, dim3(launch_blocks(n, 256, 1 << 22)), dim3(256), 0, st, rhs, r, cvec, n, factor, c_lo, c_hi);
    DS_HIP(hipGetLastError());
    return 0;
}

// *flag |= 1 if any double of c[lo, hi) is not the all-zero bit pattern (a -0.0 counts as non-zero)
__global__ void __launch_bounds__(256) k_any_nonzero_bits(const double *__restrict__ c, i64 lo, i64 hi, int *flag) {
    bool any = false;
    for (i64 i = lo + (i64)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (i64)gridDim.x * blockDim.x)
        any = any || (__double_as_longlong(c[i]) != 0);
    if (any) atomicOr(flag, 1);
}

int launch_c_interior_test(const Grid &g, const double *cvec, int *flag, hipStream_t st) {
    i64 lo, hi;
    c_interior(g, lo, hi);
    if (hi <= lo) return 0;
    DS_KLAUNCH(k_any_nonzero_bits, dim3(launch_blocks(hi - lo, 256, 1 << 14)), dim3(256), 0, st, cvec, lo, hi, flag);
    DS_HIP(hipGetLastError());
    return 0;
}

// time-slab mode: rhs(:, :, first layer) += (D/ht) * u0 of the left neighbour's last cell
__global__ void __launch_bounds__(TILE_Y *TILE_X) k_rhs_fixup(Grid g, double at, const double *__restrict__ u0_prev,
                                                               double *__restrict__ rhs) {
    const i64 y = (i64)blockIdx.x * TILE_Y + threadIdx.x;
    const i64 x = (i64)blockIdx.y * TILE_X + threadIdx.y;
    if (y >= g.ny || x >= g.nx) return;
    const i64 i = y + g.py * x;
    rhs[i] = rhs[i] + at * u0_prev[i];
}

int launch_rhs_fixup(const Grid &g, const LoopCoef &c, const double *u0_prev, double *rhs, hipStream_t st) {
    DS_KLAUNCH(k_rhs_fixup, tile_grid(g, 1), dim3(TILE_Y, TILE_X), 0, st, g, c.at, u0_prev, rhs);
    DS_HIP(hipGetLastError());
    return 0;
}

// tmp_q = A phi in q layout (solver_socp_PALM.m:137): forward differences times D/h, like the q-step
__global__ void __launch_bounds__(TILE_Y *TILE_X) k_grad(Grid g, LoopCoef c, const double *__restrict__ phi,
                                                          double *__restrict__ out) {
    const i64 y = (i64)blockIdx.x * TILE_Y + threadIdx.x;
    const i64 x = (i64)blockIdx.y * TILE_X + threadIdx.y;
    const i64 tl = blockIdx.z;
    if (y >= g.ny || x >= g.nx) return;
    const i64 node = y + g.py * (x + g.nx * tl);
    const double p0 = phi[node];
    // (the edge indices written out: through bx_index / by_index the compiler orders the address sums differently)
    if (tl < g.ncl) out[node] = fwd_diff(c.at, p0, phi[node + g.plane]);
    if (x < g.nx - 1) out[g.offBx + g.bxLayer * tl + y + g.py * x] = fwd_diff(c.ax, p0, phi[node + g.py]);
    if (y < g.ny - 1) out[g.offBy + g.byLayer * tl + y + g.pyb * x] = fwd_diff(c.ay, p0, phi[node + 1]);
}

int launch_grad(const Grid &g, const LoopCoef &c, const double *phi, double *out, hipStream_t st) {
    DS_KLAUNCH(k_grad, tile_grid(g, g.ntl), dim3(TILE_Y, TILE_X), 0, st, g, c, phi, out);
    DS_HIP(hipGetLastError());
    return 0;
}

// Time-slab mode: the fused cone kernel leaves, in the halo layer (index ncl) of q2 and of the side
// buffers, the adjoint sums that the LAST owned cell contributes to the first edge layer of the
// right neighbour.  This kernel completes them (tile-boundary edges) into two contiguous planes.
__global__ void __launch_bounds__(TILE_Y *TILE_X) k_tail_finalize(Grid g, LoopCoef c, FusedGeom fg,
                                                                   const double *__restrict__ q2v,
                                                                   const double *__restrict__ sx,
                                                                   const double *__restrict__ sy,
                                                                   double *__restrict__ tail_bx,
                                                                   double *__restrict__ tail_by) {
    const i64 y = (i64)blockIdx.x * TILE_Y + threadIdx.x;
    const i64 x = (i64)blockIdx.y * TILE_X + threadIdx.y;
    const i64 tl = g.ncl;
    // (indices written out, as in k_grad)
    if (y < g.ny && x < g.nx - 1) {
        double v = q2v[g.offBx + g.bxLayer * tl + y + g.py * x];
        if (sx_split(fg, x)) v = c.sf * (v + sx[(tl * fg.nxblk + (x / fg.XB + 1)) * g.ny + y]);
        tail_bx[y + g.py * x] = v;
    }
    if (y < g.ny - 1 && x < g.nx) {
        double v = q2v[g.offBy + g.byLayer * tl + y + g.pyb * x];
        if (sy_split(y)) v = c.sf * (v + sy[(tl * g.nx + x) * fg.nyblk + (y / 64 + 1)]);
        tail_by[y + g.pyb * x] = v;
    }
}

int launch_tail_finalize(const Grid &g, const LoopCoef &c, const FusedGeom &fg, const double *q2, const double *sx,
                         const double *sy, double *tail_bx, double *tail_by, hipStream_t st) {
    DS_KLAUNCH(k_tail_finalize, tile_grid(g, 1), dim3(TILE_Y, TILE_X), 0, st, g, c, fg, q2, sx, sy, tail_bx,
                       tail_by);
    DS_HIP(hipGetLastError());
    return 0;
}

// Time-slab mode, KKT block: what the right neighbour needs from this slab's LAST cell layer --
// alpha0, w.*alpha0 and the raw partial adjoint sums of beta (cone columns 4,5 / 8,9).
__global__ void __launch_bounds__(TILE_Y *TILE_X) k_kkt_tail(Grid g, const double *__restrict__ alpha,
                                                              const double *__restrict__ beta,
                                                              const double *__restrict__ weight,
                                                              double *__restrict__ a0, double *__restrict__ a0w,
                                                              double *__restrict__ bt_bx, double *__restrict__ bt_by) {
    const i64 y = (i64)blockIdx.x * TILE_Y + threadIdx.x;
    const i64 x = (i64)blockIdx.y * TILE_X + threadIdx.y;
    const i64 tl = g.ncl - 1;
    if (y < g.ny && x < g.nx) {
        const i64 cidx = y + g.py * (x + g.nx * tl);
        const double a = alpha[cidx];
        a0[y + g.py * x] = a;
        a0w[y + g.py * x] = weight ? weight[cidx] * a : a;
    }
    if (y < g.ny && x < g.nx - 1) {
        double acc = beta[3 * g.Nc + y + g.py * ((x + 1) + g.nx * tl)];
        acc += beta[4 * g.Nc + y + g.py * (x + g.nx * tl)];
        bt_bx[y + g.py * x] = acc;
    }
    if (y < g.ny - 1 && x < g.nx) {
        double acc = beta[7 * g.Nc + (y + 1) + g.py * (x + g.nx * tl)];
        acc += beta[8 * g.Nc + y + g.py * (x + g.nx * tl)];
        bt_by[y + g.pyb * x] = acc;
    }
}

int launch_kkt_tail(const Grid &g, const double *alpha, const double *beta, const double *weight, double *a0,
                    double *a0w, double *bt_bx, double *bt_by, hipStream_t st) {
    DS_KLAUNCH(k_kkt_tail, tile_grid(g, 1), dim3(TILE_Y, TILE_X), 0, st, g, alpha, beta, weight, a0, a0w, bt_bx,
                       bt_by);
    DS_HIP(hipGetLastError());
    return 0;
}

// One-process-per-slab transposes of the Poisson solve: the slab rows [t][col] <-> the send / receive staging
// area in which the columns of every peer's pencil are contiguous, [peer][t][col - cut(peer)], in ONE launch
// (cut[j] .. cut[j+1] are the columns of pencil j; the area of peer j starts at cut[j] * ntl).
template <bool PACK>
__global__ void __launch_bounds__(256) k_pencil_pack(PencilCuts pc, i64 plane, i64 ntl, double *__restrict__ slab,
                                                      double *__restrict__ stage) {
    const i64 col = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 t = blockIdx.y;
    if (col >= plane) return;
    int j = (int)((col * pc.world) / plane);                 // first guess, then walk to the owning pencil
    while (j > 0 && col < pc.cut[j]) --j;
    while (j < pc.world - 1 && col >= pc.cut[j + 1]) ++j;
    const i64 c0 = pc.cut[j], w = pc.cut[j + 1] - c0;
    const i64 si = c0 * ntl + t * w + (col - c0);
    if (PACK) stage[si] = slab[t * plane + col];
    else slab[t * plane + col] = stage[si];
}

int launch_pencil_pack(bool pack, const PencilCuts &pc, i64 plane, i64 ntl, double *slab, double *stage, hipStream_t st) {
    if (plane * ntl <= 0) return 0;
    dim3 grid((unsigned)((plane + 255) / 256), (unsigned)ntl);
    if (pack) DS_KLAUNCH(k_pencil_pack<true>, grid, dim3(256), 0, st, pc, plane, ntl, slab, stage);
    else DS_KLAUNCH(k_pencil_pack<false>, grid, dim3(256), 0, st, pc, plane, ntl, slab, stage);
    DS_HIP(hipGetLastError());
    return 0;
}

// x = x * mul / div  (left to right, like `alpha * dScale2 / cScale2^2`, solver_socp_inPALM.m:170-178,312-314)
__global__ void __launch_bounds__(256) k_scale(double *__restrict__ x, i64 n, double mul, double div, int use_mul) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
        double v = x[i];
        if (use_mul) v = v * mul;
        x[i] = v / div;
    }
}

int launch_scale(double *x, i64 n, double mul, double div, hipStream_t st) {
    if (n <= 0) return 0;
    DS_KLAUNCH(k_scale, dim3(launch_blocks(n, 256, 1 << 22)), dim3(256), 0, st, x, n, mul, div,
                       (int)(mul != 1.0));
    DS_HIP(hipGetLastError());
    return 0;
}

}  // namespace dotsocp
