// One step of the q-step's march through the time layers on a 64 x QTX tile of nodes: the step k_qstep_rhs takes and
// k_qcone takes again with a cone cell one step behind it (qstep_march.hip).  Both kernels call these functions, so "the
// same loads, the same arithmetic, the same order" holds by construction.  A step is written in phases -- all loads of the
// layer (from clamped, always valid addresses; the few that exist on tile / slab borders only sit under their condition but
// are loads and nothing else), then the arithmetic, then the caller's stores -- so that the loads leave together and are
// waited for once.  (With a load, its use and a store inside one `if` per entry the step was five dependent memory round
// trips long.)
#pragma once
#include "device_utils.h"

namespace dotsocp {

// A scaling of alpha that is still pending in memory (sigma update, solver_socp_inPALM.m:312: alpha = alpha / factor) is
// applied on load with k_scale's arithmetic; the q-step writes the scaled values into the ping-pong partner.
struct APend {
    int on;
    double mul, div;
};

// One staggered entry of the q-step on operands that are in registers: tmp = (A phi)_k, q2 = (F*B*(z + beta))_k, a = alpha_k,
// w = weight_k.  Returns alpha_k as used (after the pending scaling); qn = q^+, an = alpha^+, u = w q^+ - alpha^+.
// MULT 0: alpha + tau (A phi - w q) (inPALM); 1: (alpha + A phi) - w q (acc-ADMM); 2: alpha stays (PALM's first q-step)
template <bool WEIGHTED, int MULT = 0>
__device__ __forceinline__ double q_calc(const LoopCoef &c, double tmp, double q2, double diag_c, double dinv, double w,
                                         double a, const APend &ap, double &qn, double &an, double &u) {
    if (ap.on) a = a * ap.mul / ap.div;
    if (WEIGHTED) {
        const double di = 1.0 / (diag_c + w * w);
        qn = (w * (tmp + a) + q2) * di;
        if (MULT == 2) {
            an = a;
        } else if (MULT == 1) {
            const double t = a + tmp;                 // alpha + tmp_q - w.*q (solver_wsocp_accADMM.m:243)
            an = t - w * qn;
        } else {
            const double r = tmp - w * qn;
            an = a + c.tau * r;
        }
        u = w * qn - an;
    } else {
        qn = (tmp + a + q2) * dinv;
        if (MULT == 2) {
            an = a;
        } else if (MULT == 1) {
            const double t = a + tmp;                 // alpha + tmp_q - q (solver_socp_accADMM.m:237)
            an = t - qn;
        } else {
            const double r = tmp - qn;
            an = a + c.tau * r;
        }
        u = qn - an;
    }
    return a;
}

// F*B*(BF q + d) of one q entry, with mexBFd's / mexBFdConj's arithmetic: a q0 entry sits in columns 1 and 10 of its cell
// (d cancels), a staggered edge in one column of each of the four cells around it -- two on the first and the last layer
__device__ __forceinline__ double fbbf_cell(const LoopCoef &c, double q0) {
    return c.s * ((c.dF + c.s * q0) - (c.dF - c.s * q0));
}
__device__ __forceinline__ double fbbf_edge(const LoopCoef &c, double e, bool tbnd) {
    const double v = c.sf * e;
    double acc = v + v;
    if (!tbnd) {
        acc += v;
        acc += v;
    }
    return c.sf * acc;
}

// What a thread of the tile is: the thread of node (y, x) owns, on every layer, the q0 entry of the cell that starts there
// and the bx / by edges that leave it; the first column / row of the tile also recomputes the neighbour tile's edge.
template <int QTX>
struct QTile {
    int lane, xl;
    i64 y, x, yc, xc;               // yc / xc: (0, 0) for a thread outside the grid (its addresses stay valid)
    bool inb, hasBx, hasBy;
    bool rightCol, topRow;          // fetch the phi halo strip right of / above the tile
    bool leftTile, belowTile;       // the bx edge on the left / the by edge below belongs to the tile there
    bool sxOwn, syOwn;              // own edge on a tile border of the cone kernel: its sum is completed from sx / sy
};

template <int QTX>
__device__ __forceinline__ QTile<QTX> q_tile(const Grid &g, const FusedGeom &fg, const BlockId &blk) {
    QTile<QTX> t;
    t.lane = threadIdx.x;
    t.xl = threadIdx.y;
    t.y = (i64)blk.x * TILE_Y + t.lane;
    t.x = (i64)blk.y * QTX + t.xl;
    t.inb = (t.y < g.ny) && (t.x < g.nx);
    t.hasBx = t.inb && (t.x < g.nx - 1);
    t.hasBy = t.inb && (t.y < g.ny - 1);
    t.rightCol = t.hasBx && (t.xl == QTX - 1);
    t.topRow = t.hasBy && (t.lane == TILE_Y - 1);
    t.leftTile = t.inb && (t.xl == 0) && (t.x >= 1);
    t.belowTile = t.inb && (t.lane == 0) && (t.y >= 1);
    t.sxOwn = t.hasBx && sx_split(fg, t.x);
    t.syOwn = t.hasBy && sy_split(t.y);
    t.yc = t.inb ? t.y : 0;
    t.xc = t.inb ? t.x : 0;
    return t;
}

// phi of the layer the march stands on lives in LDS with a one-entry halo in x and y, ph[par][QTX + 2][TILE_Y + 2]: every
// phi entry is fetched ONCE per tile and layer (own column as the "t + 1" value of the step before, the four halo strips by
// the border lanes) and the x / y neighbours are read from there -- read from global they cost a second fetch of the whole
// layer, a step later
struct PhiHalo {
    double hx, hl, hy, hb;          // right, left, above, below
};

template <int QTX>
__device__ __forceinline__ PhiHalo load_phi_halo(const Grid &g, const QTile<QTX> &t, const double *__restrict__ phi, i64 node) {
    PhiHalo h{0.0, 0.0, 0.0, 0.0};
    if (t.rightCol) h.hx = phi[node + g.py];
    if (t.leftTile) h.hl = phi[node - g.py];
    if (t.topRow) h.hy = phi[node + 1];
    if (t.belowTile) h.hb = phi[node - 1];
    return h;
}

template <int QTX>
__device__ __forceinline__ void store_phi_layer(double (&ph)[QTX + 2][TILE_Y + 2], const QTile<QTX> &t, double p,
                                                const PhiHalo h) {     // by value: the strips stay in registers
    ph[t.xl + 1][t.lane + 1] = p;
    if (t.xl == QTX - 1) ph[QTX + 1][t.lane + 1] = h.hx;
    if (t.xl == 0) ph[0][t.lane + 1] = h.hl;
    if (t.lane == TILE_Y - 1) ph[t.xl + 1][TILE_Y + 1] = h.hy;
    if (t.lane == 0) ph[t.xl + 1][0] = h.hb;
}

// the arrays a step reads (weight: WEIGHTED only; tail_bx / tail_by: `tails` only; qk: `pcorr` only)
struct QSrc {
    const double *phi, *q2v, *sx, *sy, *weight, *tail_bx, *tail_by, *cvec, *alpha_in, *qk;
    int c_ends;                     // c is zero off the two global end layers: no load elsewhere
};

// everything a thread loads for node layer tl
struct QLayerIn {
    i64 node, eX, eY;               // node; own bx / by entry (the node where there is none)
    bool tbnd, hasCell;
    double dc, di;                  // diagonal of the edges of this layer and its inverse
    double pTl;                     // phi of the next layer (this one again at the end) with its halo strips
    PhiHalo h;
    double pXl, pYl;                // phi at x + 1, y + 1
    double al0, alX, alY, g0, gX, gY, k0v, kXv, kYv, cv, w0, wX, wY, sxv, syv, tXv, tYv;
    bool sxL, syB;                  // the neighbour's edge lies on a tile border of the cone kernel
    double pLl, alL, gL, wL, sxLv, tLv, kLv;   // the left tile's edge (leftTile)
    double pBl, alB, gB, wB, syBv, tBv, kBv;   // the lower tile's edge (belowTile)
};

// tails: slab mode, tl == 0 on a slab that is not the first -- the left neighbour's share of the first edge layer is added;
// pcorr: the gather was given as p2 = F*B*((1 + tau) z + beta) and qk = q^k is loaded to correct it (PALM's first q-step)
template <bool WEIGHTED, int QTX>
__device__ __forceinline__ QLayerIn q_layer_load(const Grid &g, const LoopCoef &c, const FusedGeom &fg, const QTile<QTX> &t,
                                                 const QSrc &a, const double (&ph)[QTX + 2][TILE_Y + 2], i64 tl, bool tails,
                                                 bool pcorr) {
    QLayerIn in;
    const i64 y = t.y, x = t.x;
    in.node = t.yc + g.py * (t.xc + g.nx * tl);
    in.tbnd = (g.t0 + tl == 0) || (g.t0 + tl == g.nt - 1);
    in.dc = in.tbnd ? c.c2 : c.c1;
    in.di = in.tbnd ? c.dinv2 : c.dinv1;
    in.hasCell = t.inb && (tl < g.ncl);
    const i64 node = in.node;
    const i64 eX = t.hasBx ? bx_index(g, t.yc, t.xc, tl) : node;
    const i64 eY = t.hasBy ? by_index(g, t.yc, t.xc, tl) : node;
    in.eX = eX;
    in.eY = eY;
    const i64 k0 = in.hasCell ? node : 0;                       // q0 entries exist for tl < ncl only
    const i64 nodeT = in.hasCell ? node + g.plane : node;       // the layer of the next step
    in.pTl = a.phi[nodeT];
    in.h = load_phi_halo(g, t, a.phi, nodeT);
    in.pXl = ph[t.xl + 2][t.lane + 1];
    in.pYl = ph[t.xl + 1][t.lane + 2];
    in.al0 = a.alpha_in[k0]; in.alX = a.alpha_in[eX]; in.alY = a.alpha_in[eY];
    in.g0 = a.q2v[k0];
    in.gX = a.q2v[eX]; in.gY = a.q2v[eY];
    in.k0v = 0.0; in.kXv = 0.0; in.kYv = 0.0;
    if (pcorr) { in.k0v = a.qk[k0]; in.kXv = a.qk[eX]; in.kYv = a.qk[eY]; }
    // c of an interior layer is known to be zero: no load (the condition is uniform over the workgroup; cv keeps all
    // its uses, so the results are those of loading the zero)
    in.cv = 0.0;
    if (!a.c_ends || in.tbnd) in.cv = a.cvec[node];
    in.w0 = 1.0; in.wX = 1.0; in.wY = 1.0;
    if (WEIGHTED) { in.w0 = a.weight[k0]; in.wX = a.weight[eX]; in.wY = a.weight[eY]; }
    in.sxv = a.sx[t.sxOwn ? sx_index(g, fg, y, x, tl) : 0];
    in.syv = a.sy[t.syOwn ? sy_index(g, fg, y, x, tl) : 0];
    in.tXv = 0.0; in.tYv = 0.0;
    if (tails) {
        if (t.hasBx) in.tXv = a.tail_bx[y + g.py * x];
        if (t.hasBy) in.tYv = a.tail_by[y + g.pyb * x];
    }
    // neighbour tiles' edges (first column / first row of the tile)
    in.sxL = false; in.syB = false;
    in.pLl = 0.0; in.alL = 0.0; in.gL = 0.0; in.wL = 1.0; in.sxLv = 0.0; in.tLv = 0.0; in.kLv = 0.0;
    if (t.leftTile) {
        const i64 eL = bx_index(g, y, x - 1, tl);
        in.sxL = sx_split(fg, x - 1);
        in.pLl = ph[0][t.lane + 1];
        in.alL = a.alpha_in[eL];
        in.gL = a.q2v[eL];
        if (pcorr) in.kLv = a.qk[eL];
        if (WEIGHTED) in.wL = a.weight[eL];
        if (in.sxL) in.sxLv = a.sx[sx_index(g, fg, y, x - 1, tl)];
        if (tails) in.tLv = a.tail_bx[y + g.py * (x - 1)];
    }
    in.pBl = 0.0; in.alB = 0.0; in.gB = 0.0; in.wB = 1.0; in.syBv = 0.0; in.tBv = 0.0; in.kBv = 0.0;
    if (t.belowTile) {
        const i64 eB = by_index(g, y - 1, x, tl);
        in.syB = sy_split(y - 1);
        in.pBl = ph[t.xl + 1][0];
        in.alB = a.alpha_in[eB];
        in.gB = a.q2v[eB];
        if (pcorr) in.kBv = a.qk[eB];
        if (WEIGHTED) in.wB = a.weight[eB];
        if (in.syB) in.syBv = a.sy[sy_index(g, fg, y - 1, x, tl)];
        if (tails) in.tBv = a.tail_by[(y - 1) + g.pyb * x];
    }
    return in;
}

// the q-step of the layer's entries: tmp = A phi, q^+, alpha^+, u = w q^+ - alpha^+ and alpha as loaded (ain) of the three
// own entries (zeros where the thread has none), q^+, alpha^+ and u of the two neighbour tiles' edges
struct QLayerOut {
    double pT;                                     // phi of the next layer where the cell exists, else 0
    double tmp0, q0n, a0n, ain0, u0;
    double tmpX, qXn, aXn, ainX, ubx;
    double tmpY, qYn, aYn, ainY, uby;
    double qL, aL, ubx_l, qB, aB, uby_b;
};

template <bool WEIGHTED, int MULT, int QTX>
__device__ __forceinline__ QLayerOut q_layer_calc(const LoopCoef &c, const QTile<QTX> &t, const QLayerIn &in, const APend &ap,
                                                  double p0, bool tails, bool pcorr) {
    QLayerOut o{};
    // the adjoint sums of an edge on a tile border are completed from the neighbour tile's partial (k_qstep_fused)
    double g0 = in.g0, gX = in.gX, gY = in.gY;
    if (t.sxOwn) gX = c.sf * (gX + in.sxv);
    if (t.syOwn) gY = c.sf * (gY + in.syv);
    if (tails) { gX += in.tXv; gY += in.tYv; }
    if (pcorr) {
        g0 = g0 - c.tau * fbbf_cell(c, in.k0v);
        gX = gX - c.tau * fbbf_edge(c, in.kXv, in.tbnd);
        gY = gY - c.tau * fbbf_edge(c, in.kYv, in.tbnd);
    }
    if (in.hasCell) {
        o.pT = in.pTl;
        o.tmp0 = fwd_diff(c.at, p0, o.pT);
        o.ain0 = q_calc<WEIGHTED, MULT>(c, o.tmp0, g0, c.c1, c.dinv1, in.w0, in.al0, ap, o.q0n, o.a0n, o.u0);
    }
    if (t.hasBx) {
        o.tmpX = fwd_diff(c.ax, p0, in.pXl);
        o.ainX = q_calc<WEIGHTED, MULT>(c, o.tmpX, gX, in.dc, in.di, in.wX, in.alX, ap, o.qXn, o.aXn, o.ubx);
    }
    if (t.hasBy) {
        o.tmpY = fwd_diff(c.ay, p0, in.pYl);
        o.ainY = q_calc<WEIGHTED, MULT>(c, o.tmpY, gY, in.dc, in.di, in.wY, in.alY, ap, o.qYn, o.aYn, o.uby);
    }
    if (t.leftTile) {
        double q2 = in.gL;
        if (in.sxL) q2 = c.sf * (q2 + in.sxLv);
        if (tails) q2 += in.tLv;
        if (pcorr) q2 = q2 - c.tau * fbbf_edge(c, in.kLv, in.tbnd);
        q_calc<WEIGHTED, MULT>(c, fwd_diff(c.ax, in.pLl, p0), q2, in.dc, in.di, in.wL, in.alL, ap, o.qL, o.aL, o.ubx_l);
    }
    if (t.belowTile) {
        double q2 = in.gB;
        if (in.syB) q2 = c.sf * (q2 + in.syBv);
        if (tails) q2 += in.tBv;
        if (pcorr) q2 = q2 - c.tau * fbbf_edge(c, in.kBv, in.tbnd);
        q_calc<WEIGHTED, MULT>(c, fwd_diff(c.ay, in.pBl, p0), q2, in.dc, in.di, in.wB, in.alB, ap, o.qB, o.aB, o.uby_b);
    }
    return o;
}

// A value of the bx edge at x - 1 / the by edge at y - 1, after the step's barrier: handed over by the thread that owns the
// edge (through its LDS slot in `slots`, resp. a lane shuffle) or, on the tile's first column / row, the recomputed entry of
// the neighbour tile; `none` where there is no such edge (x == 0: never used).  (The slots as an array, not as a callable
// that reads them: k_qcone is two registers larger with the closure.)
template <int QTX, class T, int NX, int NY>
__device__ __forceinline__ T from_left(const QTile<QTX> &t, const T (&slots)[NX][NY], T recomputed, T none) {
    if (t.x < 1) return none;
    return (t.xl > 0) ? slots[t.xl - 1][t.lane] : recomputed;
}
template <int QTX>
__device__ __forceinline__ double from_below(const QTile<QTX> &t, double shuffled, double recomputed) {
    return t.belowTile ? recomputed : shuffled;
}

// (A' v)(y, x, tl) of a staggered field from the six entries around the node -- v0m / v0: cells tl - 1 / tl, vxm / vx: bx edges
// at x - 1 / x, vym / vy: by edges at y - 1 / y -- in the order of rhs_value(), missing neighbours dropped (Neumann)
template <int QTX>
__device__ __forceinline__ double adjoint_sum(const Grid &g, const LoopCoef &c, const QTile<QTX> &t, i64 tl, double v0m,
                                              double v0, double vxm, double vx, double vym, double vy) {
    double r = 0.0;
    if (tl >= 1) r += c.at * v0m;
    if (tl < g.ncl) r += (-c.at) * v0;
    if (t.x >= 1) r += c.ax * vxm;
    if (t.x <= g.nx - 2) r += (-c.ax) * vx;
    if (t.y >= 1) r += c.ay * vym;
    if (t.y <= g.ny - 2) r += (-c.ay) * vy;
    return r;
}

}  // namespace dotsocp
