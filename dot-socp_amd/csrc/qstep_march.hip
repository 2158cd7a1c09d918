// The q-step as one march through the time layers: q^{k+1}, alpha^{k+1} and the next right-hand side in one pass
// (k_qstep_rhs), and the same march with the next iteration's gamma-reading cone pass one step behind it (k_qcone).  Both
// kernels take their step from qstep_tile.h.
#include "device_utils.h"
#include "gather_tile.h"
#include "kernels.h"
#include "qstep_tile.h"

#include <cstdlib>

namespace dotsocp {

// ---------------------------------------------------------------------------------------
// q-step + alpha update + the NEXT iteration's right-hand side in one pass (fused dataflow):
//   q^{k+1}, alpha^{k+1} as in k_qstep_fused, then rhs = A'(w.*q^{k+1} - alpha^{k+1}) + c (solver_socp_inPALM.m:194
//   of iteration k+1) while u = w.*q - alpha is still in registers: saves re-reading q and alpha (6 of the 8
//   arrays k_rhs streams).  A workgroup owns a 64 (y) x 4 (x) tile of nodes and marches through a chunk of
//   time layers; the thread of node (y, x, tl) owns the q0 entry of the cell that starts there and the bx /
//   by edges that leave it.  u of the t-1 cell is carried in a register, u of the x-1 edge comes through LDS,
//   u of the y-1 edge through a lane shuffle; on a tile / chunk boundary the neighbour's entry is recomputed
//   (reads only -- alpha is ping-ponged, so no other workgroup's writes are observed).  The sum order is the
//   one of rhs_value().  Time-slab mode: the term of the left neighbour's last cell is added by k_rhs_fixup
//   after the u0 exchange.
// ---------------------------------------------------------------------------------------

struct QRhsArgs {
    const double *phi, *q2v, *sx, *sy, *weight, *tail_bx, *tail_by, *cvec, *alpha_in;
    double *q_out, *alpha_out, *rhs;
    double *u0_tail;   // time slabs, VAR 0 - 2 (optional): raw u0 = w.*q0^+ - alpha0^+ of the last owned cell layer, for the right slab's rhs
    i64 TC, z0, zstride;   // layers per chunk; this launch runs the chunks z0 + blockIdx.z * zstride
    // VAR 2 (acc-ADMM, Halpern step folded in): q_out receives the raw q^+ (the cone pass needs it), the
    // extrapolated q goes to q_state in place and the extrapolated alpha to alpha_out
    double *q_state;
    const double *q_anchor, *alpha_anchor;
    double c1, c2, om_rho, rho;
    APend ap;          // pending scaling of alpha_in (VAR 0)
    int xcd;           // XCD-aware tile order
    // VAR 3 with the gather given as p2 = F*B*((1 + tau) z + beta) (k_cone_fused modes 5 / 6): qk = q^k, and the gather the
    // q-step uses is p2 - tau F*B*(BF q^k + d)
    const double *qk;
    // KKT variant (VAR 0, single slab): per-workgroup partial sums, r = A' alpha^+ - c per node, DOT complementarity scalars
    double *partials, *resid;
    double kappa, dsD;
    int c_ends;        // c is zero off the two global end layers (Slab::c_ends): the steps on other layers take cv = 0
};

// VAR 0: inPALM / ALG2; 1: acc-ADMM multiplier arithmetic, raw outputs; 2: acc-ADMM with the Halpern step of q and
// alpha folded in (solver_socp_accADMM.m:373-379); 3: PALM's first q-step (q only, solver_socp_PALM.m:196-200).
// The rhs is formed from the raw u = w.*q^+ - alpha^+ in all cases (VAR 3: alpha^+ = alpha)
//
// KKT = true (VAR 0, one slab): the iteration ends with a KKT check (solver_socp_inPALM.m:220-267).  Everything of that
// block that depends on phi^{k+1}, q^{k+1}, alpha^{k+1}, A phi and c only is accumulated here, where those values are in
// registers anyway: ||q||^2, ||alpha||^2, ||A phi||^2, ||A phi - w q||^2, <w q, alpha>, <c, phi>, ||phi||^2,
// ||A' alpha - c||^2 (a second accumulation next to the rhs, alpha of the x-1 / y-1 / t-1 entries travelling beside u) and
// the momentum terms of compute_kkt_dot_complement.m:10-18 for all edges whose two density nodes lie in this tile (the
// edges on the tile's right / upper border are left to k_kkt_bnd).  r = A' alpha - c is also stored per node: after a
// sigma update the right-hand side of the next phi-step is rhs + r - r / factor (launch_rhs_sigma_fix) instead of a new pass.
enum { Q_Q2 = 0, Q_ALPHA2, Q_APHI2, Q_PRIM1, Q_QALPHA, Q_CPHI, Q_PHI2, Q_DUAL1, Q_MRHOB, Q_M2, Q_RHOB2, Q_COUNT };

template <bool WEIGHTED, int VAR, bool KKT = false, int QTX = TILE_X>
__global__ void __launch_bounds__(TILE_Y *QTX, (QTX > TILE_X && !WEIGHTED ? 4 : 1)) k_qstep_rhs(Grid g, LoopCoef c, FusedGeom fg, QRhsArgs a) {
    __shared__ double xch[2][QTX][TILE_Y];
    __shared__ double ph[2][QTX + 2][TILE_Y + 2];                           // phi of the layer the march stands on (qstep_tile.h)
    __shared__ double xcha[KKT ? 2 : 1][KKT ? QTX : 1][KKT ? TILE_Y : 1];   // alpha^+ of the bx edge
    __shared__ double xchr[KKT ? 2 : 1][KKT ? QTX : 1][KKT ? TILE_Y : 1];   // density at the node
    double S[Q_COUNT];     // KKT only (dead code otherwise)
    if (KKT) {
#pragma unroll
        for (int i = 0; i < Q_COUNT; ++i) S[i] = 0.0;
    }
    auto wgt = [&](i64 k) { return WEIGHTED ? a.weight[k] : 1.0; };
    // sums every staggered entry contributes to (edge_sums of k_kkt)
    auto entry = [&](double tmp, double qn, double an, double w) {
        const double wq = w * qn;
        S[Q_Q2] += qn * qn;
        S[Q_ALPHA2] += an * an;
        S[Q_APHI2] += tmp * tmp;
        const double r1 = tmp - wq;
        S[Q_PRIM1] += r1 * r1;
        S[Q_QALPHA] += wq * an;
    };
    double a0prev = 0.0, rhoTprev = 0.0;
    // XCD-aware tile order (device_utils.h): tiles that are neighbours in y or x run on the same XCD back to back, so
    // what they share -- the cache lines of the by rows (length ny - 1: never line-aligned), the phi row above, the
    // neighbour tile's edge that is recomputed here -- is served by that XCD's L2 instead of a second HBM fetch
    const BlockId blk = block_id(a.xcd != 0);
    const QTile<QTX> t = q_tile<QTX>(g, fg, blk);
    const int lane = t.lane, xl = t.xl;
    const i64 y = t.y, x = t.x;
    const bool inb = t.inb;
    const i64 t0 = ((i64)blk.z * a.zstride + a.z0) * a.TC;
    const i64 t1 = (t0 + a.TC < g.ntl) ? t0 + a.TC : g.ntl;
    auto put = [&](i64 k, double qn, double an, double ain) {
        a.q_out[k] = qn;
        if (VAR == 3) return;                         // PALM's first q-step: alpha is not touched
        if (VAR == 2) {
            double v = a.om_rho * a.q_state[k];
            v = v + a.rho * qn;
            a.q_state[k] = a.c1 * a.q_anchor[k] + a.c2 * v;
            v = a.om_rho * ain;
            v = v + a.rho * an;
            a.alpha_out[k] = a.c1 * a.alpha_anchor[k] + a.c2 * v;
        } else {
            a.alpha_out[k] = an;
        }
    };
    constexpr int MULT = (VAR == 3 ? 2 : (VAR != 0 ? 1 : 0));
    const QSrc src{a.phi, a.q2v, a.sx, a.sy, a.weight, a.tail_bx, a.tail_by, a.cvec, a.alpha_in, a.qk, a.c_ends};
    const bool pcorr = (VAR == 3) && (a.qk != nullptr);
    double u0prev = 0.0;
    double p0 = 0.0;
    if (inb) {
        const i64 node0 = y + g.py * (x + g.nx * t0);
        p0 = a.phi[node0];
        store_phi_layer<QTX>(ph[0], t, p0, load_phi_halo(g, t, a.phi, node0));      // the chunk's first layer
        if (t0 > 0) {       // cell in front of the chunk (owned by the previous chunk): recompute, do not store
            const i64 k = node0 - g.plane;
            const double tmp = fwd_diff(c.at, a.phi[k], p0);
            double qn, an;
            double g0f = a.q2v[k];
            if (pcorr) g0f = g0f - c.tau * fbbf_cell(c, a.qk[k]);
            q_calc<WEIGHTED, MULT>(c, tmp, g0f, c.c1, c.dinv1, wgt(k), a.alpha_in[k], a.ap, qn, an, u0prev);
            if (KKT) {
                a0prev = an;
                rhoTprev = a.kappa * (wgt(k) * an);
            }
        }
    }
    int par = 0;
    __syncthreads();                                              // ph[0] is complete
    for (i64 tl = t0; tl < t1; ++tl) {
        const bool tails = (tl == 0) && !g.first;                // slab mode: the left neighbour's share of the first layer
        // KKT variant on a slab that is not the first: the sums of its first node / edge layer need the left neighbour's
        // last cell (alpha0 for A' alpha, the density for the momentum terms) -- they are left to a one-layer launch of
        // k_kkt after the exchange; the q0 entries of that layer need no neighbour and stay here
        const bool lay0 = KKT && tails;
        const QLayerIn in = q_layer_load<WEIGHTED, QTX>(g, c, fg, t, src, ph[par], tl, tails, pcorr);
        const QLayerOut o = q_layer_calc<WEIGHTED, MULT, QTX>(c, t, in, a.ap, p0, tails, pcorr);
        double mbx = 0.0, mby = 0.0;     // KKT: momentum kappa (w alpha^+) of the own edges
        double rhoT = 0.0;               // KKT: density of the cell that starts at this node
        if (KKT) {
            if (in.hasCell) {
                entry(o.tmp0, o.q0n, o.a0n, in.w0);
                rhoT = a.kappa * (in.w0 * o.a0n);
            }
            if (t.hasBx && !lay0) {
                entry(o.tmpX, o.qXn, o.aXn, in.wX);
                mbx = a.kappa * (in.wX * o.aXn);
                S[Q_M2] += mbx * mbx;
            }
            if (t.hasBy && !lay0) {
                entry(o.tmpY, o.qYn, o.aYn, in.wY);
                mby = a.kappa * (in.wY * o.aYn);
                S[Q_M2] += mby * mby;
            }
        }
        // ---------------- stores ----------------
        if (in.hasCell) {
            put(in.node, o.q0n, o.a0n, o.ain0);
            if (VAR != 3 && a.u0_tail && tl == g.ncl - 1 && !g.last) a.u0_tail[y + g.py * x] = o.u0;
        }
        if (t.hasBx) put(in.eX, o.qXn, o.aXn, o.ainX);
        if (t.hasBy) put(in.eY, o.qYn, o.aYn, o.ainY);
        // density at the node: mean of the two cells that meet there in time, zero outside (movmean's padding)
        const double rhoN = (rhoTprev + rhoT) / 2.0;
        xch[par][xl][lane] = o.ubx;
        store_phi_layer<QTX>(ph[par ^ 1], t, in.pTl, in.h);
        if (KKT) {
            xcha[par][xl][lane] = o.aXn;
            xchr[par][xl][lane] = rhoN;
        }
        __syncthreads();
        const double uby_s = __shfl_up(o.uby, 1, 64);
        const double aby_s = KKT ? __shfl_up(o.aYn, 1, 64) : 0.0;
        const double rhoU = KKT ? __shfl_down(rhoN, 1, 64) : 0.0;
        if (inb) {
            const double ubx_m = from_left(t, xch[par], o.ubx_l, 0.0);
            const double uby_m = from_below(t, uby_s, o.uby_b);
            a.rhs[in.node] = adjoint_sum(g, c, t, tl, u0prev, o.u0, ubx_m, o.ubx, uby_m, o.uby) + in.cv;
            if (KKT && !lay0) {
                const double abx_m = from_left(t, xcha[par], o.aL, 0.0);
                const double aby_m = from_below(t, aby_s, o.aB);
                // A' alpha^+ in the order of k_kkt's node part
                double ra = adjoint_sum(g, c, t, tl, a0prev, o.a0n, abx_m, o.aXn, aby_m, o.aYn);
                ra = ra - in.cv;
                a.resid[in.node] = ra;
                S[Q_DUAL1] += ra * ra;
                S[Q_CPHI] += in.cv * p0;
                S[Q_PHI2] += p0 * p0;
                // compute_kkt_dot_complement.m:10-18: momentum against mean density times b, edges inside the tile
                if (x < g.nx - 1 && xl < QTX - 1) {
                    const double rm = (rhoN + xchr[par][xl + 1][lane]) / 2.0;
                    const double rb = a.dsD * (rm * o.qXn);
                    const double d = mbx - rb;
                    S[Q_MRHOB] += d * d;
                    S[Q_RHOB2] += rb * rb;
                }
                if (y < g.ny - 1 && lane < TILE_Y - 1) {
                    const double rm = (rhoN + rhoU) / 2.0;
                    const double rb = a.dsD * (rm * o.qYn);
                    const double d = mby - rb;
                    S[Q_MRHOB] += d * d;
                    S[Q_RHOB2] += rb * rb;
                }
            }
        }
        u0prev = o.u0;
        if (KKT) {
            a0prev = o.a0n;
            rhoTprev = rhoT;
        }
        p0 = o.pT;
        par ^= 1;
    }
    if (KKT) {
        // workgroup reduction as in k_kkt: wavefront shuffles, LDS across the four wavefronts, one partial row per workgroup
        __shared__ double red[QTX][Q_COUNT];
        static const int slot[Q_COUNT] = {S_Q2, S_ALPHA2, S_APHI2, S_PRIM1, S_QALPHA, S_CPHI, S_PHI2, S_DUAL1, S_MRHOB, S_M2, S_RHOB2};
#pragma unroll
        for (int i = 0; i < Q_COUNT; ++i) {
            double v = S[i];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) red[xl][i] = v;
        }
        __syncthreads();
        if (xl == 0 && lane < S_COUNT) {
            double v = 0.0;
#pragma unroll
            for (int i = 0; i < Q_COUNT; ++i)
                if (slot[i] == lane) {
                    v = red[0][i];
#pragma unroll
                    for (int wv = 1; wv < QTX; ++wv) v += red[wv][i];
                }
            // one row per tile and CHUNK (a slab's q-step runs as several launches over disjoint sets of chunks)
            const i64 b = blk.x + (i64)gridDim.x * (blk.y + (i64)gridDim.y * ((i64)blk.z * a.zstride + a.z0));
            a.partials[b * S_COUNT + lane] = v;
        }
    }
}

static int launch_qstep_rhs_var(int var, const Grid &g, const LoopCoef &c, const FusedGeom &fg, QRhsArgs a, hipStream_t st,
                                i64 z0 = 0, i64 zcount = -1, i64 zstride = 1);

int launch_qstep_rhs(const Grid &g, const LoopCoef &c, const FusedGeom &fg, const double *phi, const double *q2,
                     const double *sx, const double *sy, const double *weight, const double *tail_bx,
                     const double *tail_by, const double *cvec, double *q_out, const double *alpha_in, double *alpha_out,
                     double *rhs, hipStream_t st, i64 z0, i64 zcount, i64 zstride, const QStepExtra *ex) {
    QRhsArgs a{};
    a.phi = phi; a.q2v = q2; a.sx = sx; a.sy = sy; a.weight = weight; a.tail_bx = tail_bx; a.tail_by = tail_by;
    a.cvec = cvec; a.alpha_in = alpha_in; a.q_out = q_out; a.alpha_out = alpha_out; a.rhs = rhs;
    a.ap = APend{0, 1.0, 1.0};
    if (ex) {
        a.ap = APend{ex->aops.n, ex->aops.mul, ex->aops.div};
        a.partials = ex->partials;
        a.resid = ex->resid;
        a.u0_tail = ex->u0_tail;
        a.kappa = ex->kappa;
        a.dsD = ex->dsD;
        a.c_ends = ex->c_ends;
    }
    return launch_qstep_rhs_var(0, g, c, fg, a, st, z0, zcount, zstride);
}

// blocks of the q-step launch: one row of partial sums each in the KKT variant
i64 qstep_rhs_blocks(const Grid &g, const FusedGeom &fg) { return fg.nyblk * fg.nxblk * qstep_rhs_chunks(g, fg); }

// var 1 / 2: the acc-ADMM flavours (see k_qstep_rhs); `acc` carries the Halpern weights and the extra arrays of var 2
int launch_qstep_rhs_acc(int var, const Grid &g, const LoopCoef &c, const FusedGeom &fg, const double *phi,
                         const double *q2, const double *sx, const double *sy, const double *weight, const double *cvec,
                         double *q_raw, const double *alpha_in, double *alpha_out, double *rhs, double *q_state,
                         const double *q_anchor, const double *alpha_anchor, const AccCoef &k, hipStream_t st,
                         const double *tail_bx, const double *tail_by, double *u0_tail) {
    QRhsArgs a{};
    a.phi = phi; a.q2v = q2; a.sx = sx; a.sy = sy; a.weight = weight; a.cvec = cvec;
    a.tail_bx = tail_bx; a.tail_by = tail_by; a.u0_tail = u0_tail;
    a.alpha_in = alpha_in; a.q_out = q_raw; a.alpha_out = alpha_out; a.rhs = rhs;
    a.q_state = q_state; a.q_anchor = q_anchor; a.alpha_anchor = alpha_anchor;
    a.c1 = k.c1; a.c2 = k.c2; a.om_rho = k.om_rho; a.rho = k.rho;
    return launch_qstep_rhs_var(var, g, c, fg, a, st);
}

i64 qstep_rhs_chunks(const Grid &g, const FusedGeom &fg, i64 *TCout) {
    // short chunks of time layers (measured at 1024x1024x128: 3.45 ms with 8-layer chunks, 4.2 ms with one chunk per
    // tile -- the march is latency-bound per workgroup); each extra chunk recomputes one cell
    const i64 tiles = fg.nyblk * fg.nxblk;
    const i64 target = 32768;
    i64 chunks = (target + tiles - 1) / tiles;
    i64 TC = (g.ntl + chunks - 1) / chunks;
    if (TC < 8) TC = 8;
    // a slab of a time-slab decomposition: at least four chunks, so that the two in the middle -- which need neither
    // neighbour -- can run while the phi head and the adjoint tails travel (Solver::step)
    if (!(g.first && g.last) && cone_split_enabled() && g.ntl >= 12) {
        // ... the LAST chunk -- the only one that waits for the phi head of the right neighbour -- about a quarter of the
        // slab, the chunks in front of it up to eight layers each (16 layers: 6 + 6 + 4)
        const i64 tail = (g.ntl / 4 < 4) ? 4 : g.ntl / 4;
        const i64 body = g.ntl - tail, nb = (body + 7) / 8;
        TC = (body + nb - 1) / nb;
    }
    if (TC > g.ntl) TC = g.ntl;
    if (TC < 1) TC = 1;
    if (TCout) *TCout = TC;
    return (g.ntl + TC - 1) / TC;
}

static int launch_qstep_rhs_var(int var, const Grid &g, const LoopCoef &c, const FusedGeom &fg, QRhsArgs a, hipStream_t st,
                                i64 z0, i64 zcount, i64 zstride) {
    i64 TC = 1;
    const i64 chunks = qstep_rhs_chunks(g, fg, &TC);
    if (zcount < 0) zcount = chunks - z0;
    if (z0 < 0 || zcount <= 0 || zstride < 1 || z0 + (zcount - 1) * zstride >= chunks) return 0;
    a.TC = TC;
    a.z0 = z0;
    a.zstride = zstride;
    a.xcd = 1;
    dim3 grid((unsigned)fg.nyblk, (unsigned)fg.nxblk, (unsigned)zcount);
    dim3 blk(TILE_Y, TILE_X);
    // the plain inPALM instance may run on tiles twice as wide (the recomputed x - 1 edge and the phi halo columns cost
    // half as much); the KKT variant keeps the tile of k_kkt_bnd, which finishes the edges on ITS tile borders
    // (1024 x 1024 x 128: 18.35 -> 17.6 GB per launch by the PMC counters, same time; small grids keep the narrow tile:
    // they need the workgroup count more than the bytes)
    const char *qe = getenv("DOTSOCP_QTX");                   // read per launch: the tests switch it inside one process
    const int qtx_env = qe ? atoi(qe) : 0;
    const int qtx = qtx_env ? qtx_env : ((fg.nyblk * fg.nxblk * zcount >= 8192 && !a.weight) ? 2 * TILE_X : TILE_X);
    if (var == 0 && !a.partials && qtx == 2 * TILE_X) {
        dim3 grid2((unsigned)fg.nyblk, (unsigned)((g.nx + 2 * TILE_X - 1) / (2 * TILE_X)), (unsigned)zcount);
        dim3 blk2(TILE_Y, 2 * TILE_X);
        if (a.weight) DS_KLAUNCH((k_qstep_rhs<true, 0, false, 2 * TILE_X>), grid2, blk2, 0, st, g, c, fg, a);
        else DS_KLAUNCH((k_qstep_rhs<false, 0, false, 2 * TILE_X>), grid2, blk2, 0, st, g, c, fg, a);
        DS_HIP(hipGetLastError());
        return 0;
    }
#define QRHS_LAUNCH(W, V) DS_KLAUNCH((k_qstep_rhs<W, V>), grid, blk, 0, st, g, c, fg, a)
    if (var == 0 && a.partials) {          // iteration with a KKT check
        if (a.weight) DS_KLAUNCH((k_qstep_rhs<true, 0, true>), grid, blk, 0, st, g, c, fg, a);
        else DS_KLAUNCH((k_qstep_rhs<false, 0, true>), grid, blk, 0, st, g, c, fg, a);
    } else if (a.weight) {
        if (var == 0) QRHS_LAUNCH(true, 0); else if (var == 1) QRHS_LAUNCH(true, 1); else QRHS_LAUNCH(true, 2);
    } else {
        if (var == 0) QRHS_LAUNCH(false, 0); else if (var == 1) QRHS_LAUNCH(false, 1);
        else if (var == 2) QRHS_LAUNCH(false, 2); else QRHS_LAUNCH(false, 3);
    }
#undef QRHS_LAUNCH
    DS_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------
// The q-step of iteration k with the gamma-reading cone pass of iteration k + 1 behind it (single slab, inPALM / ALG2,
// unweighted; scheduled by Solver::step, solver.h: "The early cone pass").  That pass needs q^{k+1} and gamma^k only, and
// the thread of node (y, x, tl) of k_qstep_rhs computes exactly the entries cone cell (y, x, tl) reads: q0 of the cell that
// starts there, its bx / by edges and -- on the tile's first column / row -- the neighbour tile's edge.  So the march takes,
// at step tl, the q-step of node layer tl (the march step of qstep_tile.h, as k_qstep_rhs<false, 0> calls it) and then cone
// cell tl - 1 (k_cone_fused<1, 4, NT, true, GOUT>: the same helpers in the same order), whose EdgeQuad of layer tl - 1 and
// q0 were kept in registers; the x - 1 edge comes through the LDS slot that carries the edge's u, the y - 1 edge by a lane
// shuffle.  q^{k+1} makes no round trip through memory: the steady form (GOUT: gamma out) does not store it at all, the
// exit form (beta out) stores it for the readers behind it.  The gather writes its sums into buffers other than the ones
// the q-step part reads.  A chunk of node layers [t0, t1) stores the q-step of these layers and the cone cells / edge
// layers [t0 - 1, t1 - 1) (the last chunk: also the final edge layer); it starts two layers early without storing, which
// gives it u0 of cell t0 - 1, the quad of layer t0 - 1 and the gather's carried entries of cell t0 - 2 -- reads of
// ping-ponged or read-only arrays only.
// ---------------------------------------------------------------------------------------
template <bool NT, bool GOUT>
__global__ void __launch_bounds__(TILE_Y *TILE_X, 3) k_qcone(Grid g, LoopCoef c, FusedGeom fg, QConeArgs a) {
    constexpr int XB = TILE_X;
    __shared__ double2 xch[2][XB][TILE_Y];         // (u, q^{k+1}) of the bx edge
    __shared__ double ph[2][XB + 2][TILE_Y + 2];   // phi of the layer the march stands on (qstep_tile.h)
    __shared__ double2 gch[2][XB][64];             // the gather's hand-off (gather_tile.h)
    const APend ap{a.ap_on, a.ap_mul, a.ap_div};
    const BlockId blk = block_id(true);
    const QTile<XB> t = q_tile<XB>(g, fg, blk);
    const int lane = t.lane, xl = t.xl;
    const i64 y = t.y, x = t.x;
    const bool inb = t.inb;
    const i64 t0 = (i64)blk.z * a.TC;
    const i64 t1 = (t0 + a.TC < g.ntl) ? t0 + a.TC : g.ntl;
    const i64 tstart = (t0 >= 2) ? t0 - 2 : 0;
    const i64 tstop = (t1 == g.ntl) ? t1 + 1 : t1;      // one virtual step on the last chunk emits the final edge layer
    const i64 nxblk = gridDim.y, nyblk = gridDim.x;
    // the q-step part is k_qstep_rhs<false, 0>: no weight, no adjoint tails (one slab), no qk
    const QSrc src{a.phi, a.q2v, a.sx, a.sy, nullptr, nullptr, nullptr, a.cvec, a.alpha_in, nullptr, a.c_ends};
    double p0 = 0.0;
    if (inb) {
        const i64 node0 = y + g.py * (x + g.nx * tstart);
        p0 = a.phi[node0];
        store_phi_layer<XB>(ph[0], t, p0, load_phi_halo(g, t, a.phi, node0));
    }
    double u0prev = 0.0;                   // u of the q0 entry of cell tl - 1 (a chunk's unstored first step: unused)
    double q0c = 0.0;                      // q0^{k+1} of cell tl - 1
    EdgeQuad eprev{0.0, 0.0, 0.0, 0.0};    // the cell's edges of layer tl - 1, times sf
    GatherCarry gc;
    int par = 0;
    __syncthreads();                                              // ph[0] is complete
    for (i64 tl = tstart; tl < tstop; ++tl) {
        const bool own = tl >= t0;                                // false on the two steps in front of the chunk
        const bool hasC = (tl > tstart) && (tl - 1 < g.ncl);      // cone cell tl - 1 exists and its first quad is in eprev
        // ---------------- loads of the cone cell ----------------
        const i64 ci = t.yc + g.py * (t.xc + g.nx * (hasC ? tl - 1 : 0));
        double b[10];
        if (hasC) {
#pragma unroll
            for (int j = 0; j < 10; ++j) b[j] = ld_stream<NT>(a.gamma_in + j * g.Nc + ci);
        }
        EdgeQuad ecur{0.0, 0.0, 0.0, 0.0};
        double q0n = 0.0;
        if (tl < g.ntl) {
            // ======== the q-step of node layer tl ========
            const QLayerIn in = q_layer_load<false, XB>(g, c, fg, t, src, ph[par], tl, false, false);
            const QLayerOut o = q_layer_calc<false, 0, XB>(c, t, in, ap, p0, false, false);
            q0n = o.q0n;
            // ---------------- stores ----------------
            if (own) {
                if (in.hasCell) {
                    a.alpha_out[in.node] = o.a0n;
                    if (!GOUT) a.q_out[in.node] = o.q0n;
                }
                if (t.hasBx) {
                    a.alpha_out[in.eX] = o.aXn;
                    if (!GOUT) a.q_out[in.eX] = o.qXn;
                }
                if (t.hasBy) {
                    a.alpha_out[in.eY] = o.aYn;
                    if (!GOUT) a.q_out[in.eY] = o.qYn;
                }
            }
            xch[par][xl][lane] = make_double2(o.ubx, o.qXn);
            store_phi_layer<XB>(ph[par ^ 1], t, in.pTl, in.h);
            __syncthreads();
            const double uby_s = __shfl_up(o.uby, 1, 64);
            const double qY_s = __shfl_up(o.qYn, 1, 64);
            if (inb) {
                const double2 r = from_left(t, xch[par], make_double2(o.ubx_l, o.qL),
                                            make_double2(0.0, 0.0));
                const double uby_m = from_below(t, uby_s, o.uby_b), qY_m = from_below(t, qY_s, o.qB);
                if (own) a.rhs[in.node] = adjoint_sum(g, c, t, tl, u0prev, o.u0, r.x, o.ubx, uby_m, o.uby) + in.cv;
                // the four edges around cell column (y, x) at layer tl, as load_edges() returns them
                ecur.xm = (x >= 1) ? c.sf * r.y : 0.0;
                ecur.xp = (x <= g.nx - 2) ? c.sf * o.qXn : 0.0;
                ecur.ym = (y >= 1) ? c.sf * qY_m : 0.0;
                ecur.yp = (y <= g.ny - 2) ? c.sf * o.qYn : 0.0;
            }
            u0prev = o.u0;
            p0 = o.pT;
            par ^= 1;
        }
        if (tl > tstart) {
            // ======== cone cell tl - 1: k_cone_fused<1, 4, NT, true, GOUT>, then edge layer tl - 1 of the gather ========
            double w[10];
            if (hasC) {
                double v[10];
                build_z2(v, q0c, eprev, ecur, c.s, c.dF);
#pragma unroll
                for (int j = 0; j < 10; ++j) b[j] = mult_finish(b[j], v[j], c.tau);
                if (!GOUT && own && inb) {
#pragma unroll
                    for (int j = 0; j < 10; ++j) st_stream<NT>(a.beta_out + j * g.Nc + ci, b[j]);
                }
#pragma unroll
                for (int j = 0; j < 10; ++j) v[j] = v[j] - b[j];
                proj_row<10>(v);
                if (GOUT && own && inb) {
#pragma unroll
                    for (int j = 0; j < 10; ++j) st_stream<NT>(a.beta_out + j * g.Nc + ci, mult_carry(b[j], v[j], c.tau));
                }
#pragma unroll
                for (int j = 0; j < 10; ++j) w[j] = v[j] + b[j];
                if (own && inb) a.q2_out[ci] = c.s * (w[9] - w[0]);
            } else {
#pragma unroll
                for (int j = 0; j < 10; ++j) w[j] = 0.0;
            }
            gather_emit<XB>(g, c.sf, gch, gc, w, tl - 1, own && inb, x, y, xl, lane, nxblk, nyblk, blk.y, blk.x, a.q2_out,
                            a.sx_out, a.sy_out);
        }
        eprev = ecur;
        q0c = q0n;
    }
}

i64 qcone_chunk_len(const Grid &g) {
    i64 TC = g.ntl;                                       // one chunk per tile (measured)
    if (const char *e = getenv("DOTSOCP_QCONE_TC")) {     // read per launch: the tests switch it inside one process
        const i64 n = atoll(e);
        if (n >= 1) TC = n;
    }
    return TC < g.ntl ? TC : g.ntl;
}

int launch_qcone(const Grid &g, const LoopCoef &c, const FusedGeom &fg, QConeArgs a, bool gout, hipStream_t st) {
    if (fg.XB != TILE_X || !(g.first && g.last) || g.ncl < 1) { set_error("internal: k_qcone on a grid it does not serve"); return DOTSOCP_ESTATE; }
    a.TC = qcone_chunk_len(g);
    const i64 chunks = (g.ntl + a.TC - 1) / a.TC;
    dim3 grid((unsigned)fg.nyblk, (unsigned)fg.nxblk, (unsigned)chunks);
    dim3 blk(TILE_Y, TILE_X);
    const bool nt = stream_nt_enabled();
    if (gout) {
        if (nt) DS_KLAUNCH((k_qcone<true, true>), grid, blk, 0, st, g, c, fg, a);
        else DS_KLAUNCH((k_qcone<false, true>), grid, blk, 0, st, g, c, fg, a);
    } else {
        if (nt) DS_KLAUNCH((k_qcone<true, false>), grid, blk, 0, st, g, c, fg, a);
        else DS_KLAUNCH((k_qcone<false, false>), grid, blk, 0, st, g, c, fg, a);
    }
    DS_HIP(hipGetLastError());
    return 0;
}

// PALM's first q-step (solver_socp_PALM.m:196-200): q_out = (A phi + alpha + q2) .* diagQInv, alpha untouched,
// plus the rhs of the phi-step that follows it (:204), A'(q_out - alpha) + c
int launch_qstep_palm_first(const Grid &g, const LoopCoef &c, const FusedGeom &fg, const double *phi, const double *q2,
                            const double *sx, const double *sy, const double *cvec, double *q_out, const double *alpha,
                            double *rhs, hipStream_t st, const double *tail_bx, const double *tail_by, const double *qk) {
    QRhsArgs a{};
    a.phi = phi; a.q2v = q2; a.sx = sx; a.sy = sy; a.cvec = cvec; a.tail_bx = tail_bx; a.tail_by = tail_by;
    a.alpha_in = alpha; a.q_out = q_out; a.rhs = rhs; a.qk = qk;
    return launch_qstep_rhs_var(3, g, c, fg, a, st);
}

}  // namespace dotsocp
