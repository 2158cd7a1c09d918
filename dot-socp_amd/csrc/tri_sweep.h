// The closed-form, division-free elimination of one t-axis tridiagonal system, written once: every kernel of tri.hip
// -- the time-slab kernels k_tri_local / k_tri_reduced / k_tri_final / k_tri_final_reg and the single slab's
// k_tsolve_single / k_tsolve_pipe -- calls these functions and keeps no arithmetic of its own, as the CPU model of
// tests/test_tri_closed_form.py has one _piece() for all of them.  The helpers take and return scalars (small structs of
// doubles); the register arrays of a kernel stay in the kernel or are passed to an inlined function that indexes them with
// constants only -- k_tsolve_pipe counts its vector-memory operations, so a helper that spills would break it.
//
// The pivots of a block depend on the mode and the row only, and have a closed form.  With x = 1 + a'/2 = cosh(theta),
// r = e^theta = x + sqrt(x^2 - 1), rho = 1 / r, the elimination from a block's first row gives
//     piv_t = r N_{t+1} / N_t ,   N_t = 1 - rho^(2t+2)  (row 0 couples to a neighbour slab: delta_0 = a' + 2)
//                                 N_t = 1 + rho^(2t+1)  (row 0 is the global first / last row: delta_0 = a' + 1)
// (both satisfy N_{t+1} = (1 - rho^2) + rho^2 N_t -- a recurrence of positive terms, no cancellation), and a global
// boundary row at the END of the sweep has piv = r N_n / N_{n-1} - 1.  In the scaled variable D_t = d_t N_t the sweep
// d_t = g_t + d_{t-1} / piv_{t-1} becomes  D_t = g_t N_t + rho D_{t-1}:  no division per row (the kernels of round 2
// spent 2 n dependent IEEE divisions per mode here and were bound by them: 43 + 57 us on a slab of 16 layers that
// streams in 27 + 54, 530 + 630 us on 64 layers).  The last unknown is rho D_{n-1} / N_n (boundary end:
// D_{n-1} / (r N_n - N_{n-1})).  The sweep from the other end is the same recurrence on the reversed column; as a
// weighted sum, sum_t rho^t N'_{n-1-t} g_t, it runs in the same ascending pass over the column.
#pragma once
#include "device_utils.h"

namespace dotsocp {

struct TriCoef {
    double rho, rho2, r, r2, n0d;      // n0d = 1 - rho^2, formed without cancellation
};
__device__ __forceinline__ TriCoef tri_coef(double ap) {
    TriCoef c;
    const double s = sqrt(ap * (1.0 + 0.25 * ap));     // sqrt(x^2 - 1)
    const double rm1 = 0.5 * ap + s;                    // r - 1
    c.r = 1.0 + rm1;
    c.rho = 1.0 / c.r;
    c.rho2 = c.rho * c.rho;
    c.r2 = c.r * c.r;
    c.n0d = (rm1 * c.rho) * (1.0 + c.rho);              // (1 - rho) (1 + rho)
    return c;
}
__device__ __forceinline__ double tri_n0(const TriCoef &c, bool bnd) { return bnd ? 1.0 + c.rho : c.n0d; }
// s pe of N_j = 1 + s pe rho^(2j) for a sweep that starts on a boundary row (bnd) or not
__device__ __forceinline__ double tri_spe(const TriCoef &c, bool bnd) { return bnd ? c.rho : -c.rho2; }
// x / n for n in (0, 2]: reciprocal seed, two Newton steps, one residual correction (the result of the IEEE sequence to
// the last bit or one off it, at about half its instructions)
__device__ __forceinline__ double tri_div(double x, double n) {
    double r = __builtin_amdgcn_rcp(n);
    double e = __builtin_fma(-n, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-n, r, 1.0);
    r = __builtin_fma(r, e, r);
    const double q = x * r;
    return __builtin_fma(__builtin_fma(-n, q, x), r, q);
}
// N_0, N_{n-1}, N_n of the sweep over n rows that starts on a boundary row (bnd: N_j = 1 + rho^(2j+1)) or not
// (N_j = 1 - rho^(2j+2)); rn1 = rho^(n-1).
struct TriEnds {
    double N0, N1, Nn;
};
__device__ __forceinline__ TriEnds tri_ends(const TriCoef &c, bool bnd, int n, double rn1) {
    TriEnds e;
    e.N0 = tri_n0(c, bnd);
    e.N1 = (n == 1) ? e.N0 : 1.0 + (bnd ? 1.0 : -1.0) * ((rn1 * rn1) * (bnd ? c.rho : c.rho2));
    e.Nn = c.n0d + c.rho2 * e.N1;
    return e;
}
__device__ __forceinline__ double tri_powi(double x, int k) {
    double r = 1.0;
    while (k > 0) {
        if (k & 1) r *= x;
        x *= x;
        k >>= 1;
    }
    return r;
}
// the last unknown of a sweep over n rows from its D_{n-1}; bnd: the sweep ENDS on a global boundary row
__device__ __forceinline__ double tri_last(const TriCoef &c, double D, const TriEnds &e, bool bnd) {
    return bnd ? tri_div(D, c.r * e.Nn - e.N1) : tri_div(c.rho * D, e.Nn);
}

// ---- forward step ----
// Both sweeps of a column come out of two running sums, H_t = g_t + rho H_{t-1} and G_t = sum_{s <= t} rho^s g_s:
//     D_t = sum_{s <= t} rho^(t-s) N_s g_s = H_t + s_f pe_f rho^t G_t            (front sweep, kept per row when ROWS)
//     F   = sum_t rho^t N'_{n-1-t} g_t     = G_{n-1} + s_b pe_b rho^(n-1) H_{n-1}  (back sweep, as a weighted sum)
// -- neither sum needs a power walked back up from a value that may have underflowed.  step(gt, t, more) takes row t
// (more: another row follows, so pw ends as rho^(n-1)); the loop around it and where D goes belong to the kernel.
// KEEP: remember the last row whose power was still >= TRI_PW_SAFE, and that power, for the backward step below.
#define TRI_PW_SAFE 0x1p-500
template <bool KEEP, bool ROWS = true>
struct TriFwd {
    double H = 0.0, G = 0.0, pw = 1.0, D = 0.0;
    int ts = 0;
    double pws = 1.0;
    __device__ __forceinline__ double front(double spe) const { return H + (spe * pw) * G; }     // D of the last row taken
    __device__ __forceinline__ double back(double speb) const { return G + (speb * pw) * H; }    // F (after the last row)
    __device__ __forceinline__ void step(const TriCoef &c, double spe, double gt, int t, bool more) {
        H = gt + c.rho * H;
        G += pw * gt;
        if (ROWS) D = front(spe);
        if (KEEP && pw >= TRI_PW_SAFE) { ts = t; pws = pw; }
        if (more) pw *= c.rho;
    }
};

// ---- backward step ----
// x_t = rho (D_t [+ cl rho^t] + N_t x_{t+1}) / N_{t+1}, one fast division per row, N_t = 1 + s pe rho^(2t) from rho^t walked
// up row by row (pw *= r).  Two compile-time choices:
//   LEFT  the left interface value enters here as cl rho^t, cl = xl N_0 (D_t is linear in the right-hand side; the tsolve
//         kernels, whose forward sweep runs before the interface values exist), or it was added to g_0 before the forward
//         sweep (the slab kernels).
//   KEEP  where the walk starts.  rho^(n-1) leaves the normal range once (n - 1) log10(r) > 308 -- slabs of more than 64
//         nodes with a' = (CY + CX) / (nt-1)^2 in the hundreds, e.g. 2048 x 2048 x 256 on two GPUs.  From a zero the walk
//         stays zero and every N_t, t >= 1, came out as 1 (errors of 1e-7 of a high mode); from a denormal it carries that
//         value's few bits.  With KEEP the walk resumes from the last row t* = ts whose power was still >= TRI_PW_SAFE
//         (TriFwd<true>): behind t* N_t IS 1 in double (rho^(2t) < 2^-1000).  Where rho^(n-1) >= TRI_PW_SAFE, t* = n - 1
//         and the arithmetic is that of KEEP = false, which walks up from rho^(n-1) whatever it is.
// Instances: k_tri_final, k_tri_final_reg<NTL>: <LEFT = false, KEEP = true>; k_tsolve_single<R, NSUB>,
// k_tsolve_pipe<R, NSUB>: <true, false>.  The tsolve kernels keep KEEP = false for their register budget (k_tsolve_pipe
// sits at 166 VGPRs; ts and pws would live across both barriers) -- with LEFT a lost power costs them the whole cl term
// as well -- and are kept off the grids where it matters by the host: their pieces have n = ceil(nt / NSUB) <= 64 rows,
// rho^(n-1) < 2^-1022 needs r > 2^(1022 / (n-1)): 7.6e4 on 64 rows (nt >= 505), 2e9 on 34 (nt = 136 or 272), and
// r ~ a' <= 4 ((ny-1)^2 + (nx-1)^2) / (nt-1)^2: no 2-D grid that fits a device, but a 1-D grid from 70 000 space points
// at nt = 505 .. 511.  tsolve_tri_safe(), asked by launch_poisson_t_single, sends every grid whose largest a' could take
// rho^(n-1) below TRI_PW_SAFE to the transform passes along t, which exist for every length.
template <bool LEFT, bool KEEP>
struct TriBwd {
    double xn, Nt1, pw, cl;
    int ts;
    // the last row: fw after the forward sweep over the piece; xl, xr: the neighbours' interface values (LEFT only)
    template <bool FK, bool FR>
    __device__ __forceinline__ TriBwd(const TriCoef &c, const TriEnds &f, const TriFwd<FK, FR> &fw, bool last, double xl, double xr) {
        cl = LEFT ? xl * f.N0 : 0.0;                               // D_t gains cl rho^t; D_{n-1} also xr N_{n-1}
        xn = tri_last(c, LEFT ? (fw.D + cl * fw.pw) + xr * f.N1 : fw.D, f, last);
        Nt1 = f.N1;
        pw = KEEP ? fw.pws : fw.pw;                                // (pws = rho^(n-1) unless that fell below TRI_PW_SAFE)
        ts = fw.ts;
    }
    // row t < n - 1, rows in descending order; Dt: the forward sweep's D_t.  Returns x_t.
    __device__ __forceinline__ double step(const TriCoef &c, const TriEnds &f, double spe, double Dt, int t) {
        if (!KEEP || t < ts) pw *= c.r;                            // rho^t
        const double Nt = (t == 0) ? f.N0 : ((KEEP && t > ts) ? 1.0 : 1.0 + spe * (pw * pw));
        xn = tri_div(c.rho * ((LEFT ? Dt + cl * pw : Dt) + Nt * xn), Nt1);
        Nt1 = Nt;
        return xn;
    }
};

// ---- spike values ----
// first / last entries of A_p^-1 e_first (vf, vl) and A_p^-1 e_last (wf, wl) of a block of n rows:
// prod_{s < n-1} 1 / piv_s = rho^(n-1) N_0 / N_{n-1}, 1 / piv_{n-1} = rho N_{n-1} / N_n (boundary end: N_{n-1} / (r N_n - N_{n-1}));
// f, b: the ends of the sweeps from the front and from the back, rn1 = rho^(n-1).  The first block has no left neighbour
// (vf = vl = 0), the last no right one.
struct TriSpike {
    double vf, vl, wf, wl;
};
__device__ __forceinline__ TriSpike tri_spike_ends(const TriCoef &c, const TriEnds &f, const TriEnds &b, double rn1, bool first, bool last) {
    TriSpike k;
    if (last) {
        const double den = c.r * f.Nn - f.N1;
        k.vl = tri_div(rn1 * f.N0, den);
        k.wl = tri_div(f.N1, den);
    } else {
        k.vl = tri_div((rn1 * c.rho) * f.N0, f.Nn);
        k.wl = tri_div(c.rho * f.N1, f.Nn);
    }
    if (first) {
        const double den = c.r * b.Nn - b.N1;
        k.wf = tri_div(rn1 * b.N0, den);
        k.vf = tri_div(b.N1, den);
    } else {
        k.wf = tri_div((rn1 * c.rho) * b.N0, b.Nn);
        k.vf = tri_div(c.rho * b.N1, b.Nn);
    }
    if (first) k.vf = k.vl = 0.0;
    if (last) k.wf = k.wl = 0.0;
    return k;
}
__device__ __forceinline__ TriSpike tri_spike(const TriCoef &c, int n, bool first, bool last) {
    const double rn1 = tri_powi(c.rho, n - 1);
    return tri_spike_ends(c, tri_ends(c, first, n, rn1), tri_ends(c, last, n, rn1), rn1, first, last);
}

// ---- reduced block-bidiagonal sweep over the P pieces of a column ----
// unknowns F_p (first value of piece p), L_p (last value):  F_p = Gf + vf L_{p-1} + wf F_{p+1},  L_p = Gl + vl L_{p-1} + wl F_{p+1}
// forward: L_{p-1} = al_prev + ga_prev F_p  ->  F_p = A + B F_{p+1},  L_p = al + ga F_{p+1}   (head: p == 0, no L_{-1})
// back substitution from Fnext = F_{p+1} (0 behind the last piece): piece p needs L_{p-1} and F_{p+1}.
// Storage of (A, B, al, ga) per piece stays with the caller: registers in k_tri_reduced, LDS in the tsolve kernels.
// (the spike values as four scalars and the outputs by reference, straight into the caller's storage: with a TriSpike
// argument or a struct returned, the same arithmetic cost k_tri_reduced<16> 20 VGPRs and kept k_tri_reduced<DS_MAX_WORLD>
// from unrolling)
__device__ __forceinline__ void tri_red_fwd(bool head, double Gf, double Gl, double vf, double vl, double wf, double wl, double al_prev,
                                            double ga_prev, double &A, double &B, double &al, double &ga) {
    if (head) {
        A = Gf; B = wf; al = Gl; ga = wl;
    } else {
        const double den = 1.0 - vf * ga_prev;
        A = (Gf + vf * al_prev) / den;
        B = wf / den;
        al = Gl + vl * (al_prev + ga_prev * A);
        ga = wl + vl * ga_prev * B;
    }
}
// returns F_p; Lprev = L_{p-1} (0 for the head)
__device__ __forceinline__ double tri_red_back(bool head, double A, double B, double al_prev, double ga_prev, double Fnext, double &Lprev) {
    const double F = A + B * Fnext;
    Lprev = head ? 0.0 : al_prev + ga_prev * F;
    return F;
}

// ---- the singular (0, 0) mode ----
// T x = g - mean(g) by recurrence from x_0 = 0, in place on the column col[0 .. nt) whose sum the caller formed while
// gathering it.  Returns the shift the caller adds to every entry: zero mean, plus beta * mean(g) (the k = 0 coefficient
// divided by D^2 * 1).  One thread.
__device__ __forceinline__ double tri_singular(double *col, i64 nt, double sum, double beta) {
    const double gbar = sum / (double)nt;
    double xm = 0.0, xc = 0.0, acc = 0.0;          // x_{t-1}, x_t
    for (i64 t = 0; t < nt; ++t) {
        const double gt = col[t] - gbar;
        col[t] = xc;
        acc += xc;
        const double xn = (t == 0) ? xc - gt : 2.0 * xc - xm - gt;
        xm = xc;
        xc = xn;
    }
    return beta * gbar - acc / (double)nt;
}

// ---- one tile of the single slab's solve: 64 modes x nt rows in the registers of NSUB wavefronts ----
// Wavefront w holds the rows [t_w, t_w + n) of its lane's mode in X[R] (already scaled by 1 / (D^2 (nt-1)^2), zeros behind
// n); the NSUB pieces of a column are coupled exactly like time slabs.  tsolve_front: forward sweep (D_t left in X), first /
// last entry of A_p^-1 g_p and the piece's spike values into LDS.  The caller's barrier follows (k_tsolve_pipe issues the
// next tile's DMA behind it).  tsolve_back: wave 0 solves the reduced systems of the 64 modes in place in LDS, one thread
// the singular mode, then the backward sweep leaves the solution in X (the singular mode's in zcol).  Neither half issues a
// vector-memory instruction.
// LDS of a workgroup, declared by the kernel (an array nobody touches -- ex at NSUB = 1 -- is not allocated):
//     ex[NSUB][6][64]   per piece: Gf, Gl, vf, vl, wf, wl -> xl, xr, A, B, al, ga (in place)
//     zcol[NSUB * R]    the singular mode's column (the workgroup that holds mode 0 only)
struct TsMid {                         // what the front half leaves for the back half
    TriCoef c;
    TriEnds f;
    TriFwd<false> fw;
};
template <bool RAWB>
__device__ __forceinline__ void ts_barrier() {
    if (RAWB) lds_barrier(); else __syncthreads();
}

// ap: a' of the lane's mode (anything positive for mode 0, which takes its own path); tile0: this tile holds mode 0
template <int R, int NSUB>
__device__ __forceinline__ TsMid tsolve_front(double (&ex)[NSUB][6][64], double (&zcol)[NSUB * R], double (&X)[R], double ap, int w, int lane, int t0, int n, bool tile0) {
    const bool first = (w == 0), last = (w == NSUB - 1);
    TsMid k;
    k.c = tri_coef(ap);
    if (tile0 && lane == 0) {
#pragma unroll
        for (int t = 0; t < R; ++t)
            if (t < n) zcol[t0 + t] = X[t];
    }
    const double spe = tri_spe(k.c, first);
#pragma unroll
    for (int t = 0; t < R; ++t) {
        if (t < n) {
            k.fw.step(k.c, spe, X[t], t, t + 1 < n);
            X[t] = k.fw.D;
        }
    }
    k.f = tri_ends(k.c, first, n, k.fw.pw);
    if (NSUB > 1) {
        const TriEnds b = tri_ends(k.c, last, n, k.fw.pw);
        const TriSpike sp = tri_spike_ends(k.c, k.f, b, k.fw.pw, first, last);
        ex[w][0][lane] = tri_last(k.c, k.fw.back(tri_spe(k.c, last)), b, first);
        ex[w][1][lane] = tri_last(k.c, k.fw.D, k.f, last);
        ex[w][2][lane] = sp.vf;
        ex[w][3][lane] = sp.vl;
        ex[w][4][lane] = sp.wf;
        ex[w][5][lane] = sp.wl;
    }
    return k;
}

template <int R, int NSUB, bool RAWB>
__device__ __forceinline__ void tsolve_back(double (&ex)[NSUB][6][64], double (&zcol)[NSUB * R], double (&X)[R], const TsMid &k, int w,
                                            int lane, int n, bool tile0, i64 nt, double beta) {
    const bool first = (w == 0), last = (w == NSUB - 1);
    double xl = 0.0, xr = 0.0;
    if (NSUB > 1) {
        if (w == 0) {                                  // the reduced systems of the workgroup's 64 modes
#pragma unroll 1
            for (int p = 0; p < NSUB; ++p) {
                const int pp = p ? p - 1 : 0;          // (the head has no piece before it and reads nothing of it)
                double A, B, al, ga;
                tri_red_fwd(p == 0, ex[p][0][lane], ex[p][1][lane], ex[p][2][lane], ex[p][3][lane], ex[p][4][lane], ex[p][5][lane], ex[pp][4][lane],
                            ex[pp][5][lane], A, B, al, ga);
                ex[p][2][lane] = A; ex[p][3][lane] = B; ex[p][4][lane] = al; ex[p][5][lane] = ga;
            }
            double Fnext = 0.0;
#pragma unroll 1
            for (int p = NSUB - 1; p >= 0; --p) {
                const int pp = p ? p - 1 : 0;
                double Lprev;
                const double Fp = tri_red_back(p == 0, ex[p][2][lane], ex[p][3][lane], ex[pp][4][lane], ex[pp][5][lane], Fnext, Lprev);
                ex[p][0][lane] = Lprev;              // the piece's left / right interface values
                ex[p][1][lane] = Fnext;
                Fnext = Fp;
            }
        }
        ts_barrier<RAWB>();
        xl = ex[w][0][lane];
        xr = ex[w][1][lane];
    }
    if (tile0) {
        if (threadIdx.x == 0) {
            double sum = 0.0;
            for (i64 t = 0; t < nt; ++t) sum += zcol[t];
            const double shift = tri_singular(zcol, nt, sum, beta);
            for (i64 t = 0; t < nt; ++t) zcol[t] += shift;
        }
        ts_barrier<RAWB>();
    }
    const double spe = tri_spe(k.c, first);
    TriBwd<true, false> bw(k.c, k.f, k.fw, last, xl, xr);
#pragma unroll
    for (int t = R - 1; t >= 0; --t) {
        if (t == n - 1) X[t] = bw.xn;
        else if (t < n - 1) X[t] = bw.step(k.c, k.f, spe, X[t], t);
    }
}

}  // namespace dotsocp
