// Host-side launchers of the gfx950 kernels (definitions in *.hip).
#pragma once
#include "common.h"
#include "defer.h"
#include "particle_block.h"

namespace dotsocp {

// Scalars of one inPALM iteration (solver_socp_inPALM.m:53-59,96-97,194-215).
struct LoopCoef {
    double s;      // scaleBF = E / D
    double sf;     // edge_factor(s)
    double dF;     // scaleD = E / dScale
    double at, ax, ay;   // D/ht, D/hx, D/hy  (entries of D * grad, initialize.m:67-87)
    double tau;
    double c1, c2;       // (1+) 2 s^2, (1+) s^2  -- diagonal of I + s^2 F*B*BF (oper_q.m:14-23); without the 1 when weighted
    double dinv1, dinv2; // 1/c1, 1/c2 (unweighted diagQInv)
};

// Number of partial-sum slots produced by the KKT kernels.
enum {
    S_Q2 = 0, S_Z2, S_APHI2, S_ALPHA2, S_BETA2, S_FBBETA2, S_PRIM1, S_PRIM2, S_DUAL1, S_DUAL2,
    S_COMPLEM, S_DOTCOMP, S_RHO2, S_RHOFQ2, S_MRHOB, S_M2, S_RHOB2, S_QALPHA, S_CPHI, S_PHI2,
    S_COUNT
};

struct KktCoef {
    double sigma;
    double kappa;      // sigma * cScale * D      (compute_kkt_dot_complement.m:2)
    double dsD;        // dScale / D
    double dsE;        // dScale / E
};

// A scaling x <- x * mul / div (then x * mul2 / div2) that is still pending in memory: whoever loads x next applies it with
// k_scale's arithmetic (device_utils.h: apply_scale_ops) instead of a pass of its own.  Plain data: travels inside kernel
// arguments (FusedArgs, QStepExtra).
struct ScaleOps {
    int n;                  // number of pending operations (0, 1 or 2: a sigma update followed by a rescale)
    double mul, div;
    double mul2, div2;      // second pending operation, applied after the first
    bool empty() const { return n == 0; }
    void clear() { n = 0; }
    bool push(double m, double d) {      // false: both slots are taken (flush first)
        if (n >= 2) return false;
        if (n == 0) { mul = m; div = d; } else { mul2 = m; div2 = d; }
        n += 1;
        return true;
    }
};

// ---------------- cone.hip ----------------
int launch_proj_soc(double *out, const double *in, i64 M, i64 K, hipStream_t st);
int launch_bfd(const Grid &g, double *z, const double *q, double s, double dF, hipStream_t st);
// tail_bx / tail_by (time slabs, not the first): raw partial sums w4(x+1) + w5(x) resp. w8(y+1) + w9(y) of the left
// neighbour's last cell layer (launch_kkt_tail's bt_bx / bt_by)
int launch_bfd_conj(const Grid &g, double *q, const double *w, double s, hipStream_t st, const double *tail_bx = nullptr,
                    const double *tail_by = nullptr);
// z = Pi_Q(B F q + d - beta), B F q + d regenerated from q on the fly (solver_socp_inPALM.m:199)
int launch_cone_proj(const Grid &g, const LoopCoef &c, const double *q, const double *beta, double *z,
                     hipStream_t st);
// beta += tau * (z - (B F q + d))    (solver_socp_inPALM.m:212-215)
int launch_beta_update(const Grid &g, const LoopCoef &c, const double *q, const double *z, double *beta,
                       hipStream_t st);
// partial adjoint sums of the LAST owned cell layer for the right neighbour (time-slab mode)
int launch_gather_tail(const Grid &g, const double *z, const double *beta, double *tail_bx, double *tail_by,
                       hipStream_t st);

// ---------------- fused.hip ----------------
// Tile geometry of the fused cone kernel; the q-step needs it to find the edges whose adjoint
// sum is split between q2 (own tile's part) and the side buffers sx / sy (neighbour tile's part).
struct FusedGeom {
    int XB;               // tile width in x (columns per workgroup); tile height in y is 64
    i64 nyblk, nxblk;     // tiles in y / x
    i64 TC, chunks;       // time cells per chunk, number of chunks
    i64 sx_len, sy_len;   // side buffer lengths (doubles)
};
struct FusedArgs {
    const double *q_old;    // q^{k-1} (modes 1, 2)
    const double *q;        // q^k
    const double *beta_in;
    double *beta_out;       // modes 1, 2 (mode 1: must differ from beta_in when chunks > 1)
    double *z_out;          // mode 2
    double *q2;             // modes 0, 1: adjoint sums, q layout
    double *sx, *sy;        // modes 0, 1: tile-boundary partial sums
    const double *q3;       // mode 5: q~^k, the argument of the new projection (q then is q^k of the multiplier step)
    double *p2, *sxp, *syp; // modes 5, 6: second gather, F*B*((1 + tau) z + beta), layout of q2 / sx / sy
    i64 TC;
    // pending scaling of beta_in (sigma update / rescale block, solver_socp_inPALM.m:176,313), applied on
    // load exactly like k_scale would have: b = b * mul / div
    ScaleOps bops;
    int xcd;                // permute the tile order so that y-neighbouring tiles share an XCD (device_utils.h)
    int z0;                 // first chunk of this launch (launch_cone_fused can launch a range of chunks)
    // chunks launched ONE PER LAUNCH in ascending order on one stream (time slabs): the last cell's "t + 1" cone entries
    // w3, w4, w7, w8 travel to the next chunk through four layer planes instead of that chunk recomputing the cell
    const double *carry_in; // read by a chunk that is not the first (nullptr: recompute the cell in front)
    double *carry_out;      // written by a chunk that is not the last (may be the buffer carry_in points to)
};
// rows that are not a multiple of 16 doubles (128 bytes): neighbouring tiles share cache lines (2^k+1 grids)
bool tile_xcd_remap(const Grid &g);
int fused_geometry(const Grid &g, FusedGeom &fg);
// mode 0: projection + gather; 1: deferred beta update + projection + gather; 2: materialise beta and z;
// 3: z only, from (q_old, beta_in); 4: deferred beta update + gather of (z^k + beta^k) (PALM's first q-step)
// [z0, z0 + zcount) = the chunks to launch (zcount < 0: all from z0 on); chunks are independent of each other
// flavour (mode 1 only): CONE_GIN -- beta_in holds gamma^{k-1} = beta^{k-1} + tau z^k, q_old is not read;
// CONE_GOUT -- beta_out receives gamma^k = beta^k + tau z^{k+1} instead of beta^k
enum { CONE_GIN = 1, CONE_GOUT = 2 };
int launch_cone_fused(int mode, const Grid &g, const LoopCoef &c, const FusedGeom &fg, FusedArgs a,
                      hipStream_t st, i64 z0 = 0, i64 zcount = -1, int flavour = 0);
// time-slab mode: split every slab's cone pass into >= 2 chunks so that the chunks in front of the last one --
// which alone reads the q halo -- can start before the halo has arrived
bool cone_split_enabled();

// ---------------- acc.hip (acc-ADMM loop) ----------------
struct KktWork;
struct AccArgs {
    const double *q;                 // q^+ of this iteration (modes 0, 1)
    const double *z_in, *beta_in;    // current state
    const double *z0, *beta0;        // Halpern anchors (mode 1)
    double *z0_out, *beta0_out;      // mode 3: the anchors, written
    double bdiv;                     // mode 3: factor of the sigma update
    // mode 0 on an iteration that ends with a KKT check (one slab; launch_acc_cone_kkt): the cell part of the KKT sums and the
    // F*B*beta^+ terms of all edges are taken while z^+, beta^+ are in registers (k_kkt_cells<., true>'s sums and gather)
    KktCoef kk;
    const double *alpha_p, *weight;  // alpha^+ of the q-step, the weight field (or nullptr)
    double *partials;
    int nostore;                     // ... and z^+, beta^+ are not written (the pass after the block recomputes them)
    double *z_out, *beta_out;        // mode 0: z^+, beta^+; mode 1: new state (buffers other than the inputs)
    double *q2, *sx, *sy;            // modes 1, 2: adjoint sums for the next q-step
    i64 TC;
    double c1, c2, om_rho, rho;      // Halpern weights: 1/(k+2), (k+1)/(k+2), 1 - rho, rho
};
struct AccCoef {
    double c1, c2, om_rho, rho;      // as above (Halpern) or c1 = theta/(2(k+theta)), c2 = k/(k+theta)
    double om_c1, c1c2;              // 1 - c1, c1 + c2 (theta != 2)
};
// mode 0: multiplier + z-step, raw outputs; 1: + Halpern step + gather; 2: gather of (z + beta) only;
// 3: mode 1 after a sigma update (beta, beta^+ divided by a.bdiv, anchors = x^+ stored)
int launch_acc_cone(int mode, const Grid &g, const LoopCoef &c, const FusedGeom &fg, AccArgs a, hipStream_t st);
// mode 0 + KKT sums: region 1 of the partial sums (cells, edges inside the tiles) and regions 2, 3 (edges on tile borders:
// F*B*beta^+ only); a.q2 / sx / sy are scratch
int launch_acc_cone_kkt(const Grid &g, const LoopCoef &c, const FusedGeom &fg, AccArgs a, const KktWork &w, hipStream_t st);
// Halpern step right after a sigma update: x, x^+ divided by div, anchor = x^+ stored, x extrapolated with k = 0
int launch_acc_restart(double *x, const double *xp, double *anchor, i64 n, const AccCoef &k, double div, hipStream_t st);
// element-wise extrapolation of one state array (modes: see acc.hip)
int launch_acc_interp(double *x, const double *xp, double *aux, i64 n, const AccCoef &k, int mode, int write_aux,
                      hipStream_t st);

// ---------------- transfer.hip (driver steps on the device) ----------------
// gf: the fine slab; phic / betac hold the coarse layers tc0, tc0 + 1, ... (a single coarse slab: its own arrays, tc0 = 0;
// Nzc = doubles per cone column in betac, < 0: gc.Nz); gc is read for ny, nx only
int launch_prolong_phi(const Grid &gf, const Grid &gc, const double *phic, double *phif, double sc_in, double sc_out,
                       hipStream_t st, i64 tc0 = 0);
int launch_prolong_beta(const Grid &gf, const Grid &gc, const double *betac, double *betaf, double *neg, double sc_in0,
                        double sc_in1, double sc_out, hipStream_t st, i64 tc0 = 0, i64 Nzc = -1);
int launch_scale_div(double *x, const double *w, i64 n, double sc, hipStream_t st);
// time slabs: q = F*B*w on the slab's first edge layer in one slab's summation order; p3 .. p8: the left neighbour's last
// cell layer of the cone columns 3, 4, 7, 8
int launch_conj_first_layer(const Grid &g, double *q, const double *w, double s, const double *p3, const double *p4,
                            const double *p7, const double *p8, hipStream_t st);
int launch_fill(double *x, i64 n, double v, hipStream_t st);
// slab-aware: `out` holds the slab's own layers (ntl node layers resp. ncl cell layers); a_prev: launch_out_tail of the
// left neighbour (nullptr on the first slab)
int launch_outputs(const Grid &g, const double *q, const double *alpha, const double *weight, const double *rho0,
                   const double *rho1, const double *a_prev, double sig, double cD, double dD, int which, double *out,
                   hipStream_t st);
int launch_out_tail(const Grid &g, const double *alpha, const double *weight, double sig, double cD, double *out,
                    hipStream_t st);

// ---------------- advect.hip: node velocity v = E / rho layer by layer, particles along it (RK4) ----------------
// node layer `tl` of the slab -> vX, vY (rows g.py apart; 1-D: vY alone): E / rho of the values launch_outputs writes where
// rho > floor and the quotient is finite, else 0.  rho0 / rho1 / a_prev as for launch_outputs.
int launch_velocity_layer(const Grid &g, const double *alpha, const double *weight, const double *rho0, const double *rho1,
                          const double *a_prev, double sig, double cD, bool dim1, i64 tl, double floor, double *vX, double *vY,
                          hipStream_t st);
// particles: positions SoA (px along the second array index, py along the first; 1-D: py alone), one sticky flag each
int launch_advect_seed(bool dim1, i64 n, double *px, double *py, unsigned int *flag, hipStream_t st);     // clamp to [0, 1], flags <- 0
// the nsub RK4 steps of one time interval between the velocity layers (vX0, vY0) of node k and (vX1, vY1) of node k + 1;
// dt = dir / ((nt - 1) nsub).  sq, len (n doubles each, or both nullptr): the accumulating march of dotsocp_map_report --
// sq[p] += |step|^2, len[p] += |step| of every step, between the position before it and the one after its end clamp
int launch_advect(bool dim1, i64 ny, i64 nx, i64 py, const double *vX0, const double *vY0, const double *vX1,
                  const double *vY1, i64 n, int nsub, int dir, double dt, double *px, double *py_, unsigned int *flag,
                  hipStream_t st, double *sq = nullptr, double *len = nullptr);
int launch_advect_count(const unsigned int *flag, i64 n, unsigned long long *count, hipStream_t st);       // *count += set flags
// dotsocp_push_mass: cnt (ny x nx 64-bit counts, rows py apart, zeroed by the caller) += the bilinear split of every
// particle's units[p] over the corners of its cell, by integer atomics (include/dotsocp.h states the rounding)
int launch_deposit(bool dim1, i64 ny, i64 nx, i64 py, i64 n, const double *px, const double *py_, const i64 *units,
                   unsigned long long *cnt, hipStream_t st);
// frame: the counts of launch_deposit, converted in place to (double)count * unit; *sum <- the sum over the nodes of
// |frame - rho(:, :, tl)|, rho as launch_outputs writes it, added in the report's order (report_tiles(g) doubles at
// `partials`).  rho0 / rho1 / a_prev as for launch_outputs.
int launch_frame_l1(const Grid &g, const double *alpha, const double *weight, const double *rho0, const double *rho1,
                    const double *a_prev, double sig, double cD, i64 tl, double unit, double *frame, double *partials,
                    double *sum, hipStream_t st);
// dotsocp_map_report, after the last interval: rows of the partial sums (mass and the mass-weighted disp^2, len^2, action,
// disp, len) and slots of the 64-bit counters (zeroed before the launch): detour histogram, detour > last edge, len == 0,
// and the maxima of disp, len, detour as the bit patterns of these non-negative doubles
// (MS_* rows, MC_* slots: particle_block.h)
i64 map_blocks(i64 n);              // workgroups of the launch: partials holds MS_COUNT * map_blocks(n) doubles
// px, py_, sq, len: the particle block after the march; sx, sy: the seeds as given (clamped here); mass: n doubles or nullptr
// (all 1.0); edges: DOTSOCP_REPORT_BINS + 1 doubles; steps = (nt - 1) nsub; disp, action: n doubles each or nullptr;
// sums[MS_COUNT] <- the totals, added by the fixed tree of launch_report_rows over the workgroups
int launch_map_final(bool dim1, i64 n, const double *px, const double *py_, const double *sq, const double *len, const double *sx,
                     const double *sy, const double *mass, const double *edges, double steps, double *disp, double *action,
                     double *partials, double *sums, unsigned long long *counts, hipStream_t st);

// ---------------- report.hip: the solution report (mass, negativity, f(q) histograms) in one pass over alpha and q ----------------
// Slots of the 64-bit counters one report accumulates (device array, zeroed before the launch): the two histograms, three
// counts, and min(rho) / max(fq) over the finite values as order-preserving integer keys (report_key_decode; 0: no value)
enum { RC_RHO_HIST = 0, RC_FQ_HIST = DOTSOCP_REPORT_BINS, RC_RHO_NEG = 2 * DOTSOCP_REPORT_BINS, RC_FQ_POS, RC_NONFINITE,
       RC_RHO_MIN, RC_FQ_MAX, RC_COUNT };
void report_edges_host(double edges[DOTSOCP_REPORT_BINS + 1]);
double report_key_decode(unsigned long long key, bool inverted, double none);
// workgroups per layer (depends on ny, nx only) and doubles of the partial-sum buffer of a slab: [ntl][3][tiles]
i64 report_tiles(const Grid &g);
// sums[r] = partials[r * tiles] + ... + partials[r * tiles + tiles - 1], r < rows, by the fixed tree of the report's layer sums
int launch_report_rows(const double *partials, i64 tiles, i64 rows, double *sums, hipStream_t st);
// image.hip: dotsocp_imresize / dotsocp_image_density behind their argument checks (host pointers, the null stream of `device`)
int image_resize(void *out, const void *in, int dtype, i64 h_in, i64 w_in, i64 planes, i64 h_out, i64 w_out, int device);
int image_density(const dotsocp_image_opts *o, const dotsocp_image *imgs, int nimg, double *rho, int device);
// one slab: `partials` [ntl][3][tiles] <- per-workgroup layer sums of rho, min(rho, 0) and the cost terms; `sums` [ntl][3]
// <- their totals, added in tile order; counts[RC_COUNT] += this slab's share.  rho0 / rho1 / a_prev as for launch_outputs;
// edges: DOTSOCP_REPORT_BINS + 1 doubles on the device.
int launch_report(const Grid &g, const double *q, const double *alpha, const double *weight, const double *rho0,
                  const double *rho1, const double *a_prev, double sig, double cD, double dD, bool dim1, const double *edges,
                  double *partials, double *sums, unsigned long long *counts, hipStream_t st);

// ---------------- geodesic.hip: the geodesic's profile (layer sums of moments, momentum, energy, entropy) in one pass over alpha ----------------
// doubles / 64-bit counts of a slab's buffers: [partials ntl x DOTSOCP_GEO_SUMS x tiles | maxima ntl x tiles | sums ntl x
// DOTSOCP_GEO_SUMS | max ntl] and [counts ntl x tiles | count ntl]; every slot is written by every launch
i64 geodesic_doubles(const Grid &g);
i64 geodesic_counts(const Grid &g);
// one slab: sums (layer tl, quantity i at sums[tl * DOTSOCP_GEO_SUMS + i]) <- the layer sums added in the report's order, max[tl]
// <- the largest finite rho (-Inf: none), count[tl] <- nodes with rho > DOTSOCP_REPORT_RHO_FLOOR; they stand at
// buf + (DOTSOCP_GEO_SUMS + 1) * ntl * tiles (sums, then max) and cnt + ntl * tiles.  rho0 / rho1 / a_prev as for launch_outputs.
int launch_geodesic(const Grid &g, const double *alpha, const double *weight, const double *rho0, const double *rho1,
                    const double *a_prev, double sig, double cD, bool dim1, double *buf, unsigned long long *cnt, hipStream_t st);

// ---------------- hopflax.hip: Hopf-Lax transform of a node layer, sums of the dual bound (dotsocp_dual_bound) ----------------
#define HL_MAX_LEN (1 << 20)        // nodes of a line (the limit of the DCT)
#define HL_YOUT 1024                // outputs of a workgroup of the y pass: one line, 256 threads with 4 outputs each
#define HL_CHUNK_MAX 1024           // inputs the y pass stages at a time (DOTSOCP_HL_CHUNK lowers it)
#define HL_XOUT 32                  // outputs of a workgroup of the x pass: 64 lines, 4 wavefronts with 8 outputs each
#define HL_XCHUNK_MAX 32            // inputs the x pass stages at a time (DOTSOCP_HL_CHUNK lowers it)
// One pass of the transform over `lines` lines of n nodes: out[j] = min_i in[i] + (double)((i - j)^2) w (forward) resp.
// max_i in[i] - ... (backward), w = (0.5 h) h, h = 1 / (n - 1); arg[j] = the smallest winning i.  Non-finite inputs count as
// +Inf / -Inf.  pass_y: the nodes of a line are contiguous, lines `pitch` apart; pass_x: lines are contiguous (1 apart), the
// nodes of a line `pitch` apart.  in != out; arg has the layout of out.
int launch_hl_pass_y(bool forward, const double *in, double *out, int *arg, i64 n, i64 lines, i64 pitch, hipStream_t st);
int launch_hl_pass_x(bool forward, const double *in, double *out, int *arg, i64 n, i64 lines, i64 pitch, hipStream_t st);
int hl_chunk(int deflt);            // min(deflt, DOTSOCP_HL_CHUNK), at least 1 (read at every call: a test switch)
int launch_hl_layer(const double *in, double *out, i64 n, double mul, hipStream_t st);      // out = mul * in
// rows of the partial sums and slots of the 64-bit counters (zeroed before the launch; extrema as the keys of the report)
enum { HS_M0 = 0, HS_M1, HS_P0R0, HS_P1R1, HS_HR1, HS_BR0, HS_G1, HS_G0, HS_MAP, HS_COUNT };
enum { HC_G1_MAX = 0, HC_G1_MIN, HC_G0_MAX, HC_G0_MIN, HC_NONFINITE, HC_COUNT };
struct HlReduceArgs {
    i64 ny, nx, py;                 // layers ny x nx, rows py apart
    const double *phi0, *phi1, *H, *B, *rho0, *rho1;
    const int *ixf, *iyf, *ixb, *iyb;       // winners of the passes (ix*: nullptr for a 1-D line)
    int *arg_fwd, *arg_bwd;         // flat winner of every node, iy + ny * ix[iy, x]
    double hx, hy;                  // 1 / (nx - 1), 1 / (ny - 1)
    double *partials;               // [HS_COUNT][hl_blocks(ny * nx)]
    unsigned long long *counts;     // [HC_COUNT]
};
i64 hl_blocks(i64 nodes);
int launch_hl_reduce(const HlReduceArgs &a, double *sums /* HS_COUNT */, hipStream_t st);

// ---------------- softlax.hip: soft Hopf-Lax transform and the node kernels of the upper bound (dotsocp_plan_bound) ----------------
// One soft pass over `lines` lines of n nodes (include/dotsocp.h, "Soft pass"): out[j] = m - eps log(s), mean[j] = q / s.  The
// layouts, tiles and chunks are those of launch_hl_pass_y / _x (HL_YOUT, HL_XOUT, DOTSOCP_HL_CHUNK); pm: the prior mean in
// the layout of `in`, or nullptr (zeros; the x pass has none).  in, out and mean are distinct arrays.
int launch_sl_pass_y(const double *in, const double *pm, double *out, double *mean, i64 n, i64 lines, i64 pitch, double eps,
                     hipStream_t st);
int launch_sl_pass_x(const double *in, double *out, double *mean, i64 n, i64 lines, i64 pitch, double eps, hipStream_t st);
// All node kernels: one thread per node of an unpitched layer of n = ny * nx nodes in memory order, workgroups of 256
// (hl_blocks(n) of them); sums by the tree of launch_hl_reduce (partials: [rows][hl_blocks(n)]).
enum { SM_M0 = 0, SM_M1, SM_COUNT };                            // k_sl_mass: rows of the sums
enum { SC_ZERO0 = 0, SC_ZERO1, SC_BAD, SC_NONFINITE, SC_COUNT };   // 64-bit counters (zeroed before the first launch)
enum { SS_KEPT = 0, SS_COST, SS_R0, SS_R1X, SS_R1Y, SS_R2, SS_C0, SS_C1X, SS_C1Y, SS_C2, SS_COUNT };     // k_sl_final
// sums[SM_COUNT] <- the masses; counts: entries == 0 of rho0 / rho1, entries of either that are negative or not finite
int launch_sl_mass(const double *rho0, const double *rho1, i64 n, double *partials, double *sums, unsigned long long *counts,
                   hipStream_t st);
// a = rho0 / m0, b = rho1 / m1, la = -(eps log a), lb likewise; f = 0.0 (mode 0), -src (1) or src (2), non-finite entries
// counted (SC_NONFINITE) and replaced by 0.0; in = la - f
struct SlInitArgs {
    const double *rho0, *rho1, *src;
    double *a, *b, *la, *lb, *f, *in;
    i64 n;
    double m0, m1, eps;
    int mode;
    unsigned long long *counts;
};
int launch_sl_init(const SlInitArgs &a, hipStream_t st);
// x = v < x ? v : x (v != nullptr); in = l - x
int launch_sl_minsub(const double *l, double *x, const double *v, double *in, i64 n, hipStream_t st);
// *sum <- sum_i (a_i > 0 ? a_i |exp((f_i - v_i) ieps) - 1| : 0); f = v; in = la - f
int launch_sl_defect(const double *a, const double *la, double *f, const double *v, double *in, i64 n, double ieps,
                     double *partials, double *sum, hipStream_t st);
// the masses of the kept plan, what is missing and the ten sums (include/dotsocp.h, "Rounding"): f = f', fh = f^, g = g', gt = g~
struct SlFinalArgs {
    const double *a, *b, *f, *fh, *g, *gt, *E;
    double *er, *ec;
    i64 ny, nx;
    double hx, hy, ieps;            // hx = 0 for a 1-D line
    double *partials;               // [SS_COUNT][hl_blocks(ny * nx)]
};
int launch_sl_final(const SlFinalArgs &a, double *sums /* SS_COUNT */, hipStream_t st);
// The moment flavour of the soft pass (include/dotsocp.h, "Moment pass"; dotsocp_plan_map): out and mean as above, bit for
// bit, and da[j] = qa / s, the mean signed displacement along the pass's axis (candidate minus output).  The y pass of a
// layer carries the x pass's da through as pb: db[j] = qb / s (pb == nullptr, a line: db is not written).
int launch_sl_mom_y(const double *in, const double *pm, const double *pb, double *out, double *mean, double *da, double *db,
                    i64 n, i64 lines, i64 pitch, double eps, hipStream_t st);
int launch_sl_mom_x(const double *in, double *out, double *mean, double *da, i64 n, i64 lines, i64 pitch, double eps,
                    hipStream_t st);
// the map of the plan per source node (include/dotsocp.h, "Map"): rows of the sums; disp_max: one 64-bit key, zeroed before
enum { SP_ROWS = 0, SP_MAP, SP_SPREAD, SP_COST, SP_DISP, SP_COUNT };
struct SlMapArgs {
    const double *a, *f, *fh, *er;          // a, f', f^ and er of k_sl_final
    const double *kc, *kdx, *kdy;           // the kept rows' mean cost and displacement: the moment transform (kdx: nullptr for a line)
    double *Dx, *Dy, *C, *row, *spread;
    i64 ny, nx;
    double hx, hy, ieps;                    // hx = 0 for a 1-D line
    double kappa, mx, my, m2;               // C0 / fill;  C1x / C0, C1y / C0, C2 / C0  (0 where the divisor is 0)
    double *partials;                       // [SP_COUNT][hl_blocks(ny * nx)]
    unsigned long long *disp_max;
};
int launch_sl_map(const SlMapArgs &a, double *sums /* SP_COUNT */, hipStream_t st);
// X, Y <- clamp(node + tau * D) of every node of an unpitched layer; flag[i] = 1 where the clamp changed a node with units > 0
int launch_sl_frame_pos(const double *Dx, const double *Dy, const i64 *units, i64 ny, i64 nx, double hx, double hy, double tau,
                        double *X, double *Y, unsigned int *flag, hipStream_t st);
// the 64-bit counts of launch_deposit -> (double)count * unit, in place
int launch_sl_frame(double *frame, i64 n, double unit, hipStream_t st);
// dotsocp_plan_map behind the C ABI (solver_upper.hip)
int plan_map(const double *rho0, const double *rho1, i64 ny, i64 nx, const double *f_start, const dotsocp_upper_opts *o,
             dotsocp_upper *res, double *f, double *g, double *E, double *er, double *ec, double *defects,
             dotsocp_plan_map_t *map_res, double *Dx, double *Dy, double *C, double *row, double *spread, const double *taus,
             i64 nf, double *frames, int device);
// dotsocp_plan_bound behind the C ABI (solver_upper.hip)
int plan_bound(const double *rho0, const double *rho1, i64 ny, i64 nx, const double *f_start, const dotsocp_upper_opts *o,
               dotsocp_upper *res, double *f, double *g, double *E, double *er, double *ec, double *defects, int device);

// ---------------- render.hip: pictures of the density evolution (dotsocp_render_evolution) ----------------
// Slots of the 64-bit counters of the range pass (zeroed before the launch): max / min of the finite unmasked rho as the
// keys of the report (max: report_key_decode(k, false, .), min: (k, true, .); 0: no value), then two plain counts
enum { RR_MAX = 0, RR_MIN, RR_NONFINITE, RR_MASKED, RR_COUNT };
#define RND_LEVELS 255              // slots of k_render's level table in LDS: nlevels <= 254, the rest +Inf
// one slab: counts[RR_COUNT] += this slab's share.  rho0 / rho1 / a_prev as for launch_outputs; barrier: ny x nx bytes on
// the device, y fastest, non-zero = masked, or nullptr
int launch_rho_range(const Grid &g, const double *alpha, const double *weight, const double *rho0, const double *rho1,
                     const double *a_prev, double sig, double cD, const unsigned char *barrier, unsigned long long *counts,
                     hipStream_t st);
// node layer `tl` of the slab -> image [ny][nx][channels] (device, x fastest): the index of include/dotsocp.h for `mode`
// (DOTSOCP_RENDER_*), through the 256 x 3 table `lut` when channels = 3; levels: nlevels ascending doubles on the device
// (LEVELS mode)
int launch_render(const Grid &g, const double *alpha, const double *weight, const double *rho0, const double *rho1,
                  const double *a_prev, double sig, double cD, i64 tl, int mode, int channels, const unsigned char *barrier,
                  const double *levels, int nlevels, const unsigned char *lut, int barrier_index, double vmax,
                  unsigned char *image, hipStream_t st);
// node layer `tl` -> mvX, mvY [mx][my] (device, y fastest; mvX nullptr: 1-D): Ex, Ey at the nodes (jy * skip_y, jx * skip_x),
// +0.0 where rho < thr
int launch_movement(const Grid &g, const double *alpha, const double *weight, const double *rho0, const double *rho1,
                    const double *a_prev, double sig, double cD, i64 tl, i64 skip_y, i64 skip_x, i64 my, i64 mx, double thr,
                    double *mvX, double *mvY, hipStream_t st);

// ---------------- qstep_march.hip: the q-step as one march through the time layers (march step: qstep_tile.h) ----------------
// q-step + alpha update (alpha_in -> alpha_out, distinct buffers) + rhs of the next iteration's phi-step
// ex (optional): a scaling of alpha_in that is still pending in memory (applied on load), and -- partials != nullptr, one
// slab only -- the KKT variant: the sums of the KKT block that need only phi, q^+, alpha^+, A phi and c are accumulated in
// the same pass (one row of S_COUNT partial sums per workgroup at `partials`), r = A' alpha^+ - c goes to `resid`
struct QStepExtra {
    ScaleOps aops;           // pending scaling of alpha_in (one slot is ever used)
    double *partials, *resid;
    double kappa, dsD;       // KktCoef
    double *u0_tail;         // time slabs: w.*q0^+ - alpha0^+ of the last owned cell layer goes here too (the right slab's rhs)
    int c_ends;              // c is zero off the two global end layers: they alone are loaded
};
int launch_qstep_rhs(const Grid &g, const LoopCoef &c, const FusedGeom &fg, const double *phi, const double *q2,
                     const double *sx, const double *sy, const double *weight, const double *tail_bx,
                     const double *tail_by, const double *cvec, double *q_out, const double *alpha_in, double *alpha_out,
                     double *rhs, hipStream_t st, i64 z0 = 0, i64 zcount = -1, i64 zstride = 1,
                     const QStepExtra *ex = nullptr);
i64 qstep_rhs_blocks(const Grid &g, const FusedGeom &fg);
// The q-step (plain inPALM instance of launch_qstep_rhs: one slab, no weight) and, one march step behind it, the
// gamma-reading cone pass of the NEXT iteration on the q it has just formed (k_qcone).  gout: that pass
// writes gamma (the steady form: q is not stored, q_out is not touched) or beta (the exit form: q goes to q_out).
// q2v / sx / sy are the sums the q-step reads, q2_out / sx_out / sy_out (other buffers) receive the new ones.
struct QConeArgs {
    const double *phi, *q2v, *sx, *sy, *cvec, *alpha_in, *gamma_in;
    double *alpha_out, *rhs, *q_out, *beta_out, *q2_out, *sx_out, *sy_out;
    i64 TC;                    // node layers per chunk (set by the launcher)
    int ap_on;                 // pending scaling of alpha_in, applied on load (QStepExtra::aops)
    double ap_mul, ap_div;
    int c_ends;                // c is zero off the two global end layers
};
int launch_qcone(const Grid &g, const LoopCoef &c, const FusedGeom &fg, QConeArgs a, bool gout, hipStream_t st);
// node layers per chunk of that launch: one chunk per tile, or DOTSOCP_QCONE_TC=n (results do not depend on it)
i64 qcone_chunk_len(const Grid &g);
// chunks of time layers of that launch (z0 + i * zstride, i < zcount, selects chunks; chunks are independent of each other: only
// chunk 0 reads the adjoint tails of the left neighbour slab and only the last one the phi halo of the right one -- and
// writes the u0 tail)
i64 qstep_rhs_chunks(const Grid &g, const FusedGeom &fg, i64 *TC = nullptr);
// acc-ADMM: q-step + multiplier + next rhs (var 1: raw q^+, alpha^+; var 2: raw q^+ plus the Halpern step of q in
// place in q_state and of alpha into alpha_out, buffers other than alpha_in)
int launch_qstep_rhs_acc(int var, const Grid &g, const LoopCoef &c, const FusedGeom &fg, const double *phi,
                         const double *q2, const double *sx, const double *sy, const double *weight, const double *cvec,
                         double *q_raw, const double *alpha_in, double *alpha_out, double *rhs, double *q_state,
                         const double *q_anchor, const double *alpha_anchor, const AccCoef &k, hipStream_t st,
                         const double *tail_bx = nullptr, const double *tail_by = nullptr, double *u0_tail = nullptr);
// PALM (solver_socp_PALM.m:196-200): first q-step without the alpha update
int launch_qstep_palm_first(const Grid &g, const LoopCoef &c, const FusedGeom &fg, const double *phi, const double *q2,
                            const double *sx, const double *sy, const double *cvec, double *q_out, const double *alpha,
                            double *rhs, hipStream_t st, const double *tail_bx = nullptr, const double *tail_by = nullptr,
                            const double *qk = nullptr);   // qk: q2 / sx / sy hold k_cone_fused's second gather (modes 5, 6)

// ---------------- stencil.hip: one-entry-per-thread stencils, halo helpers, scalings ----------------
// q-step + alpha update reading the precomputed adjoint sums q2 (+ side buffers) of the fused kernel;
// writes q^{k+1} into q_out (q^k stays intact for the deferred beta update).
int launch_qstep_fused(const Grid &g, const LoopCoef &c, const FusedGeom &fg, const double *phi,
                       const double *q2, const double *sx, const double *sy, const double *weight,
                       const double *tail_bx, const double *tail_by, double *q_out, double *alpha,
                       hipStream_t st);
// rhs <- (rhs + r) - r / factor, c <- c / factor  (sigma update without a new pass over q and alpha)
// (c_ends: c is zero off the two global end layers, which alone are divided)
int launch_rhs_sigma_fix(const Grid &g, double *rhs, const double *r, double *cvec, double factor, hipStream_t st,
                         bool c_ends = false);
// *flag (device, cleared by the caller) |= 1 unless every layer of the slab's c except global layer 0 and nt - 1 is
// all-zero bits
int launch_c_interior_test(const Grid &g, const double *cvec, int *flag, hipStream_t st);
int launch_rhs_fixup(const Grid &g, const LoopCoef &c, const double *u0_prev, double *rhs, hipStream_t st);
// tmp_q = A phi in q layout (solver_socp_PALM.m:137)
int launch_grad(const Grid &g, const LoopCoef &c, const double *phi, double *out, hipStream_t st);
// time-slab mode: complete the adjoint sums of the last owned cell for the right neighbour (values times sf)
int launch_tail_finalize(const Grid &g, const LoopCoef &c, const FusedGeom &fg, const double *q2, const double *sx,
                         const double *sy, double *tail_bx, double *tail_by, hipStream_t st);
// time-slab mode, KKT block: alpha0, w.*alpha0 and raw adjoint partial sums of beta of the last owned cell layer
int launch_kkt_tail(const Grid &g, const double *alpha, const double *beta, const double *weight, double *a0,
                    double *a0w, double *bt_bx, double *bt_by, hipStream_t st);
// rhs = A'(w.*q - alpha) + c   (solver_socp_inPALM.m:194, solver_wsocp_inPALM.m:200)
int launch_rhs(const Grid &g, const LoopCoef &c, const double *q, const double *alpha, const double *cvec,
               const double *weight, const double *u0_prev, double *rhs, hipStream_t st, bool c_ends = false);
// q-step + alpha update (solver_socp_inPALM.m:204-206,211,214; solver_wsocp_inPALM.m:210-217)
int launch_qstep(const Grid &g, const LoopCoef &c, const double *phi, const double *z, const double *beta,
                 const double *weight, const double *tail_bx, const double *tail_by, double *q,
                 double *alpha, hipStream_t st);
// u0 = w.*q0 - alpha0 of the last owned cell layer (halo for the right neighbour's rhs)
int launch_u0_tail(const Grid &g, const double *q, const double *alpha, const double *weight, double *out,
                   hipStream_t st);
int launch_scale(double *x, i64 n, double mul, double div, hipStream_t st);   // x = x * mul / div
// slab rows <-> per-peer contiguous staging of the slab <-> pencil transposes (one process per slab)
#define DS_MAX_WORLD 64
struct PencilCuts {
    int world;
    i64 cut[DS_MAX_WORLD + 1];
};
int launch_pencil_pack(bool pack, const PencilCuts &pc, i64 plane, i64 ntl, double *slab, double *stage, hipStream_t st);

// ---------------- tri.hip: time-slab Poisson solve by partitioned tridiagonal systems (no transposes) ----------------
#define TRI_EXTRA 256     // room for the whole (0, 0) line of a slab in a message: slabs of at most 256 time nodes
int launch_tri_local(const Grid &g, i64 nt, double kscale, const double *cy, const double *cx, const PencilCuts &pc,
                     const double *r, double *send, hipStream_t st);
int launch_tri_reduced(const Grid &g, i64 nt, double kscale, const double *cy, const double *cx, const PencilCuts &pc,
                       int rank, i64 l0, i64 nl, const i64 *slab_n, const double *recv, double *back, double *zero_work,
                       hipStream_t st, const double *own_recv = nullptr, double *own_back = nullptr);
int launch_tri_final(const Grid &g, i64 nt, double kscale, const double *cy, const double *cx, const PencilCuts &pc,
                     const double *back, double *x, hipStream_t st);
// the SINGLE slab's t-axis solve by the same elimination, in place on x = [g.plane][nt] (no transform along t; any nt <= 512)
bool tsolve_tri_supported(i64 nt);
bool tsolve_tri_preferred(i64 nt, bool pow2, i64 plane, int ncu);   // faster than the transform pass(es) along t?
bool tsolve_tri_safe(i64 ny, i64 nx, i64 nt);                 // no power rho^t of a piece leaves the safe range (else: transform passes)
int launch_tsolve_tri(const Grid &g, i64 nt, double kscale, const double *cy, const double *cx, double *x, hipStream_t st);
bool tsolve_tri_pipelined(i64 nt, i64 plane, int ncu);        // launch_tsolve_tri: k_tsolve_pipe (else k_tsolve_single)
int device_cus();              // compute units of the current device, cached per device (dct_pow2.hip); 256 if the query fails
int device_cus_of(int dev);    // ... of device `dev`
// up to DS_MAX_WORLD messages copied by ONE launch on the receiving slab's stream: message m = count[m] doubles from
// src[m] (this or a peer device) to dst[m] -- the exchanges between the slabs of one process (one launch per receiver
// instead of one event-ordered copy per message)
struct GatherMsgs {
    const double *src[DS_MAX_WORLD];
    double *dst[DS_MAX_WORLD];
    i64 count[DS_MAX_WORLD];
    int n;
};
int launch_gather_msgs(const GatherMsgs &m, hipStream_t st);

// ---------------- kkt.hip ----------------
#define KKT_SLICES 64
struct KktWork {
    double *partials;   // [maxBlocks][S_COUNT]
    i64 maxBlocks;
    double *sums;       // [S_COUNT] device, followed by [KKT_SLICES][S_COUNT] intermediate sums (launch_kkt_final)
};
// Halo layers from the LEFT neighbour slab's last cell (all nullptr on the first slab):
// alpha0, w.*alpha0, and the partial adjoint sums of beta (columns 4,5 / 8,9).
struct KktHalo {
    const double *a0_prev, *a0w_prev, *btail_bx, *btail_by;
};
i64 kkt_partials_needed(const Grid &g);
// parts: bit mask of 1 node, 2 cell (+ q0 entries; needs a stored z), 4 bx edges, 8 by edges
// layer0: only the slab's first node / edge layer (the folded path on time slabs leaves it to this launch; parts 1|4|8),
// partial sums in their own regions; resid (part 1): A' alpha - c per visited node
int launch_kkt(const Grid &g, const LoopCoef &c, const KktCoef &k, const double *phi, const double *q,
               const double *alpha, const double *z, const double *beta, const double *cvec,
               const double *weight, const KktHalo &halo, const KktWork &w, int parts, hipStream_t st,
               bool layer0 = false, double *resid = nullptr);
// the node / q0-entry / edge sums that need no multiplier (parts 1, 16, 4, 8 of k_kkt without the F*B*beta terms): regions
// 0, 4, 5, 6 of the partial sums -- what is left when the cone pass has taken the cell sums (launch_acc_cone_kkt)
int launch_kkt_nodual(const Grid &g, const LoopCoef &c, const KktCoef &k, const double *phi, const double *q,
                      const double *alpha, const double *cvec, const double *weight, const KktWork &w, hipStream_t st);
// tile-border edges: F*B*beta terms from the raw partial sums in q2 / sx / sy (regions 2, 3)
int launch_kkt_bnd_dual(const Grid &g, const LoopCoef &c, const KktCoef &k, const FusedGeom &fg, const double *q,
                        const double *alpha, const double *weight, const double *q2, const double *sx, const double *sy,
                        const KktWork &w, hipStream_t st);
// fused path: pending multiplier step (beta_in -> beta_out, distinct buffers) + the cell part of the sums
// edges (one slab, after a q-step in its KKT variant): also the F*B*beta' sums of every edge and the momentum terms of
// the edges on tile borders (a.q2 / a.sx / a.sy are scratch; q_new = q^{k+1})
int launch_kkt_cells_update(const Grid &g, const LoopCoef &c, const KktCoef &k, const FusedGeom &fg, FusedArgs a,
                            const double *phi, const double *alpha, const double *weight, const KktWork &w,
                            hipStream_t st, bool edges = false, const double *q_new = nullptr);
// the rescale block's five norms of an iterate whose multiplier step is pending (a.q_old, a.q, a.beta_in [+ pending ops]):
// S_PHI2, S_Q2, S_ALPHA2, S_Z2, S_BETA2 as partial sums (clear w.partials first, launch_kkt_final afterwards)
int launch_norms(const Grid &g, const LoopCoef &c, const KktCoef &k, const FusedGeom &fg, FusedArgs a, const double *phi,
                 const double *alpha, const double *weight, const KktWork &w, hipStream_t st);
// partial sums of the q-step's KKT variant: region 0 of w.partials
double *kkt_qstep_partials(const Grid &g, const KktWork &w);
int launch_kkt_final(const Grid &g, const KktWork &w, hipStream_t st);

// ---------------- dct.hip: plan, choice of the transform family, dispatch, spectral division ----------------
// (the families: dct_pow2.hip / dct_long.hip, pfa.hip, cdft.hip / cdft_long.hip, dct_dense.hip -- dct_families.h, pfa.h, cdft.h)
// Which transform a DCT plan of length n uses (dotsocp_dct_algorithm of include/dotsocp.h).
enum { DCT_ALG_NONE = 0, DCT_ALG_FFT = 1, DCT_ALG_PFA = 2, DCT_ALG_RADER = 3, DCT_ALG_BLUESTEIN = 4, DCT_ALG_DENSE = 5 };
// Pure host arithmetic (no HIP call); honours DOTSOCP_PFA, DOTSOCP_CDFT, DOTSOCP_CDFT_MIN and
// DOTSOCP_CDFT_LONG_MIN, each read once per process.
int dct_choose_algorithm(i64 n);
struct DctPlan;   // the choice for one axis length and the chosen family's tables
// 0 no transform (n <= 1), 1 one pass with the line in LDS (or one of the other families), 2 the two-level transform of
// dct_long.hip, negative: unsupported (a power of two above 2^20).  (Lengths that are no powers of two: 1 whatever the family.)  dct_length_check: 0, or DOTSOCP_EINVAL with the limit
// in the error text -- asked before plans and contexts are made, so that nothing fails at a launch.
int dct_levels(i64 n, int axis);
int dct_length_check(i64 n);
// 0 no convolution transform (power of two, prime-factor length, dense product), 1 Rader / Bluestein inside the LDS
// (cdft.hip), 2 Bluestein with the two-level convolution of cdft_long.hip (DOTSOCP_CDFT_LONG_MIN)
int cdft_levels(i64 n);
DctPlan *dct_plan_create(i64 n);
void dct_plan_destroy(DctPlan *p);
// Orthonormal DCT-II (inverse=0) / DCT-III (inverse=1) along one axis of an [n0][n1][n2] array
// (n0 fastest), src -> dst.  axis = 0, 1 or 2.  src == dst is allowed for every length but those of the dense product.
// pitch0 > n0: the rows of both arrays are pitch0 doubles apart ([pitch0][n1][n2] with n0 valid entries per row);
// power-of-two n0 is never pitched.
int launch_dct_axis(const DctPlan *p, const double *src, double *dst, i64 n0, i64 n1, i64 n2, int axis,
                    int inverse, hipStream_t st, i64 pitch0 = 0);
// Power-of-two and prime-factor nt (dct_plan_has_tsolve): DCT-II along t, spectral division, DCT-III along t in ONE pass over a
// pencil [nl][nt]: the columns line0 .. line0+nl-1 of the ny*nx = nplane (y, x) columns (y fastest),
// all nt time nodes; src -> dst (may alias).
bool dct_plan_is_pow2(const DctPlan *p);
bool dct_plan_has_tsolve(const DctPlan *p);   // fused forward / divide / inverse pass along t available
int launch_dct_t_solve(const DctPlan *p, const double *src, double *dst, i64 ny, i64 nplane, i64 line0, i64 nl,
                       i64 nt, double kscale, const double *cy, const double *cx, const double *ct, hipStream_t st,
                       i64 pitch0 = 0);   // pitch0 > ny: whole layers (line0 = 0, nl = nplane) with pitched rows
// same pencil, an nt without the fused pass: spectral division only (between two DCT passes)
int launch_spectral_divide_pencil(double *data, i64 ny, i64 line0, i64 nl, i64 nt, double kscale, const double *cy,
                                  const double *cx, const double *ct, hipStream_t st);
// data[i] /= kscale * lambda(i)  with lambda the DCT eigenvalues of initialize_FFTkernel.m:6-15
// for global dims (ny, nx, nt); the local block covers x in [x0, x0+nxl) (pencil mode) and all y, t.
int launch_spectral_divide(double *data, i64 ny, i64 nt, i64 x0, i64 nxl, double kscale, const double *cy,
                           const double *cx, const double *ct, hipStream_t st, i64 pitch0 = 0);
// DOTSOCP_TSOLVE=dct switches the tridiagonal t solves (tri.hip) off
bool tsolve_tri_allowed();
// The single slab's t step of the Poisson solve, in place on p = [pitch0 or ny][nx][nt] (p2: scratch of the same size),
// by the fastest of: the tridiagonal solve (allow_tri and tsolve_tri_preferred), the fused t pass (dct_plan_has_tsolve),
// forward transform + spectral division + inverse transform.
int launch_poisson_t_single(const DctPlan *pt, const Grid &g, double kscale, const double *cy, const double *cx,
                            const double *ct, double *p, double *p2, i64 pitch0, hipStream_t st, bool allow_tri);
// Which kernel launch_dct_axis resp. launch_poisson_t_single take on a device of ncu CUs (DOTSOCP_PASS_* / DOTSOCP_TSOLVE_*
// of include/dotsocp.h).  Pure host arithmetic on the same choice functions the launchers switch on; the arrays are taken to
// be 16-byte aligned, as every allocation of the library is.
int dct_pass_kind(i64 n0, i64 n1, i64 n2, int axis, i64 pitch0, int ncu);
int poisson_t_kind(i64 ny, i64 nx, i64 nt, i64 pitch0, bool allow_tri, int ncu);
// row pitch of a context's device arrays for rows of ny doubles (solver_slabs.hip: Solver::row_pitch)
i64 default_row_pitch(i64 ny);

}  // namespace dotsocp
