// The per-node / per-cell expressions of the driver outputs (recover_RhoE.m:14-25, recover_q.m:12-22 after recoverOrgVar),
// shared by k_outputs (transfer.hip), which stores them, k_report (report.hip), which only judges them, and the velocity and
// frame kernels of advect.hip: all must produce the same bits, so every factor and every average is stated once, here.
//   a(k) = [w(k) *] (cD * (sig * alpha(k)))   sigma of finish(), cScale * D of recoverOrgVar, weight of wdot2d/utils/recover_RhoE.m:11
//   b(k) = dD * q(k)
#pragma once
#include "common.h"

namespace dotsocp {

// Time slabs: the density at a slab's first node averages over the left neighbour's last cell, whose a(.) arrives
// ready-made in `a_prev` (k_out_tail).
struct OutArgs {
    const double *q, *alpha, *weight, *rho0, *rho1, *a_prev;
    double sig, cD, dD;
};

__device__ __forceinline__ double out_a(const OutArgs &a, i64 k) {
    const double v = a.cD * (a.sig * a.alpha[k]);
    return a.weight ? a.weight[k] * v : v;
}

// ... with the weight's presence known at compile time: no branch between the loads of a layer
template <bool WEIGHTED>
__device__ __forceinline__ double out_a(const OutArgs &a, i64 k) {
    const double v = a.cD * (a.sig * a.alpha[k]);
    return WEIGHTED ? a.weight[k] * v : v;
}

__device__ __forceinline__ double out_b(const OutArgs &a, i64 k) { return a.dD * a.q[k]; }

// rho between two cells, the x / y average of two edge values of q, and the t average of two such averages
__device__ __forceinline__ double out_mean2(double lo, double hi) { return (lo + hi) / 2; }

// rho at node `node` = col + g.plane * tl of the slab (global layer tg): the given ends, else the mean of the cell below
// (on the slab's first layer: a_prev) and the cell here
template <bool WEIGHTED>
__device__ __forceinline__ double out_rho(const Grid &g, const OutArgs &o, i64 tg, i64 tl, i64 col, i64 node) {
    if (tg == 0) return o.rho0[col];
    if (tg == g.nt - 1) return o.rho1[col];
    return out_mean2(tl == 0 ? o.a_prev[col] : out_a<WEIGHTED>(o, node - g.plane), out_a<WEIGHTED>(o, node));
}

// Ex / Ey at a node from the two edges around it; f = 2 on the first and last time layer, else 1
__device__ __forceinline__ double out_flux(double lo, double hi, double f) { return (lo * f + hi * f) / 2; }

// bx edge (y, x+1/2, t) -- its left neighbour is g.py before it; by edge (y+1/2, x, t) -- the one below is 1 before it
__device__ __forceinline__ i64 out_edge_x(const Grid &g, i64 y, i64 x, i64 t) { return g.offBx + g.bxLayer * t + y + g.py * x; }
__device__ __forceinline__ i64 out_edge_y(const Grid &g, i64 y, i64 x, i64 t) { return g.offBy + g.byLayer * t + y + g.pyb * x; }

}  // namespace dotsocp
