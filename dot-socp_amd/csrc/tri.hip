// The t axis of the Poisson solve as tridiagonal systems: across time slabs WITHOUT the slab <-> pencil transposes
// (option B), and -- the same elimination inside one workgroup -- on the single slab (k_tsolve_*).
//
// After the y and x transforms every (ky, kx) mode is an independent system along t,
//     D^2 ((CY[ky] + CX[kx]) I + T) phi = r ,   T = (nt-1)^2 tridiag(-1, [1, 2, ..., 2, 1], -1)
// -- the Neumann matrix whose eigen-decomposition is the t-axis DCT with the eigenvalues CT of
// initialize_FFTkernel.m:6-15, so its solution IS idct_t(dct_t(r) ./ kernel) (to rounding; zero mode below).
// With the time axis cut into slabs the system is solved by partitioning (Wang / SPIKE):
//   k_tri_local   every slab, per mode: first / last entry of A_p^{-1} g_p (two eliminations from the two ends;
//                 A_p = the slab's diagonal block, g = r / (D^2 (nt-1)^2))                 -> 2 numbers per mode
//   exchange A    the 2 numbers of every mode go to the rank that owns the mode (pencil ranges of the columns)
//   k_tri_reduced owner, per mode: the 2P interface values from the block-bidiagonal reduced system
//   exchange B    every slab gets the neighbours' interface values of its modes back
//   k_tri_final   every slab, per mode: A_p x = g_p + e_first x_left + e_last x_right (Thomas)
// Volume per rank and solve: 4 numbers per mode instead of 2 ntl (two transposes): 8x less at 8 slabs of 16.
// The (0, 0) mode is singular (kernel == 0 -> 1, initialize_FFTkernel.m:15): its single line of nt values
// travels whole to the owner of column 0, which solves T x = g - mean(g) by recurrence, removes the mean and adds
// (nt-1)^2 mean(g) -- the k = 0 coefficient divided by D^2 * 1.
// The arithmetic of all of it -- forward step, backward step, spike values, reduced sweep, singular mode, and the tile solve
// of the two k_tsolve_* kernels -- is in tri_sweep.h; the kernels here are loops, loads, stores and message layout.
#include "device_utils.h"
#include "kernels.h"
#include "tri_sweep.h"

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <mutex>

namespace dotsocp {

struct TriGeom {
    i64 ny, plane, ntl;       // local slab: ntl time nodes; ny = row pitch (a pad entry of a row is a mode of its own, all zeros)
    int first, last;          // slab holds global t = 0 / t = nt-1
    double beta;              // (nt-1)^2
    double kscale;            // D^2
    const double *cy, *cx;
    PencilCuts pc;            // owner ranges of the modes (columns)
};

__device__ __forceinline__ double tri_aprime(const TriGeom &g, i64 m) { return (g.cy[m % g.ny] + g.cx[m / g.ny]) / g.beta; }

__device__ __forceinline__ int tri_owner(const PencilCuts &pc, i64 m, i64 plane) {
    int j = (int)((m * pc.world) / plane);
    while (j > 0 && m < pc.cut[j]) --j;
    while (j < pc.world - 1 && m >= pc.cut[j + 1]) ++j;
    return j;
}

// message to owner j starts at 2 cut[j] + TRI_EXTRA j and holds [first values | last values | TRI_EXTRA extras]
__device__ __forceinline__ i64 tri_msg_off(const PencilCuts &pc, int j) { return 2 * pc.cut[j] + (i64)TRI_EXTRA * j; }

// One ascending pass over the column of a mode: both eliminations at once, nothing kept (any slab length)
__global__ void __launch_bounds__(256) k_tri_local(TriGeom g, const double *__restrict__ r, double *__restrict__ send) {
    const i64 m = (i64)blockIdx.x * 256 + threadIdx.x;
    if (m >= g.plane) return;
    const double sc = 1.0 / (g.kscale * g.beta);
    const int n = (int)g.ntl;
    const int j = tri_owner(g.pc, m, g.plane);
    const i64 off = tri_msg_off(g.pc, j), w = g.pc.cut[j + 1] - g.pc.cut[j];
    if (m == 0) {                                 // the singular mode travels whole
        for (int t = 0; t < n; ++t) send[off + 2 * w + t] = r[g.plane * t] * sc;
        send[off] = 0.0;
        send[off + w] = 0.0;
        return;
    }
    const TriCoef c = tri_coef(tri_aprime(g, m));
    const bool first = g.first != 0, last = g.last != 0;
    TriFwd<false, false> fw;
    constexpr int U = 8;
    for (int t0 = 0; t0 < n; t0 += U) {
        double gv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) gv[u] = (t0 + u < n) ? r[m + g.plane * (t0 + u)] * sc : 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (t0 + u < n) fw.step(c, 0.0, gv[u], t0 + u, t0 + u + 1 < n);        // (no D per row: s pe not needed yet)
        }
    }
    const TriEnds f = tri_ends(c, first, n, fw.pw), b = tri_ends(c, last, n, fw.pw);
    send[off + (m - g.pc.cut[j])] = tri_last(c, fw.back(tri_spe(c, last)), b, first);          // first entry of A^-1 g
    send[off + w + (m - g.pc.cut[j])] = tri_last(c, fw.front(tri_spe(c, first)), f, last);     // last entry
}

struct TriReduced {
    int P, rank;              // slabs, this owner
    i64 l0, nl;               // owned modes [l0, l0 + nl)
    i64 nt;
    i64 slab_n[DS_MAX_WORLD]; // time nodes of every slab
    // one slab per process: the message of slab `own` (this rank's) does not travel -- it is read where k_tri_local wrote it
    // (own_recv, inside tri_send) and its answer is written where k_tri_final reads it (own_back, inside tri_brecv)
    int own;                  // -1: every message lies in recv / back
    const double *own_recv;
    double *own_back;
};

// PMAX: compile-time bound on the number of slabs -- the four sweep arrays are then fully unrolled and live in registers
// (a run-time bound of DS_MAX_WORLD puts 2 KB per thread into scratch: the generic instance, used above 16 slabs only)
template <int PMAX>
__global__ void __launch_bounds__(128) k_tri_reduced(TriGeom g, TriReduced q, const double *__restrict__ recv,
                                                      double *__restrict__ back, double *__restrict__ zero_work) {
    const i64 i = (i64)blockIdx.x * 128 + threadIdx.x;
    if (i >= q.nl) return;
    const i64 m = q.l0 + i;
    const i64 stride = 2 * q.nl + TRI_EXTRA;      // one message per slab
    auto msg_in = [&](int p) { return (p == q.own) ? q.own_recv : recv + p * stride; };
    auto msg_out = [&](int p) { return (p == q.own) ? q.own_back : back + p * stride; };
    if (m == 0) {
        double sum = 0.0;
        i64 tg = 0;
        for (int p = 0; p < q.P; ++p)
            for (i64 t = 0; t < q.slab_n[p]; ++t, ++tg) {
                const double v = msg_in(p)[2 * q.nl + t];
                zero_work[tg] = v;
                sum += v;
            }
        const double shift = tri_singular(zero_work, q.nt, sum, g.beta);
        tg = 0;
        for (int p = 0; p < q.P; ++p)
            for (i64 t = 0; t < q.slab_n[p]; ++t, ++tg) msg_out(p)[2 * q.nl + t] = zero_work[tg] + shift;
        for (int p = 0; p < q.P; ++p) { msg_out(p)[i] = 0.0; msg_out(p)[q.nl + i] = 0.0; }
        return;
    }
    const TriCoef c = tri_coef(tri_aprime(g, m));
    double A[PMAX], B[PMAX], al[PMAX], ga[PMAX];
#pragma unroll
    for (int p = 0; p < PMAX; ++p) {
        if (p >= q.P) break;
        const TriSpike k = tri_spike(c, (int)q.slab_n[p], p == 0, p == q.P - 1);
        const double *mi = msg_in(p);
        const double Gf = mi[i], Gl = mi[q.nl + i];
        const int pp = p ? p - 1 : 0;              // (the head has no slab before it and reads nothing of it)
        tri_red_fwd(p == 0, Gf, Gl, k.vf, k.vl, k.wf, k.wl, al[pp], ga[pp], A[p], B[p], al[p], ga[p]);
    }
    // back substitution; slab p needs L_{p-1} and F_{p+1}
    double Fnext = 0.0;                            // F_{p+1}
#pragma unroll
    for (int p = PMAX - 1; p >= 0; --p) {
        if (p >= q.P) continue;
        double Lprev;
        const int pp = p ? p - 1 : 0;
        const double F = tri_red_back(p == 0, A[p], B[p], al[pp], ga[pp], Fnext, Lprev);
        double *mo = msg_out(p);
        mo[i] = Lprev;
        mo[q.nl + i] = Fnext;
        Fnext = F;
    }
}

// A_p x = g + e_first x_left + e_last x_right: forward step per row (xl / xr added to the first / last right-hand-side
// entry), backward step per row with the power resumed from the last safe row (tri_sweep.h).
// Generic slab length: D_t is parked in x between the sweeps (two reads and two writes of the slab).
__global__ void __launch_bounds__(256) k_tri_final(TriGeom g, const double *__restrict__ back, double *__restrict__ x) {
    const i64 m = (i64)blockIdx.x * 256 + threadIdx.x;
    if (m >= g.plane) return;
    const int n = (int)g.ntl;
    const int j = tri_owner(g.pc, m, g.plane);
    const i64 off = tri_msg_off(g.pc, j), w = g.pc.cut[j + 1] - g.pc.cut[j];
    if (m == 0) {
        for (int t = 0; t < n; ++t) x[g.plane * t] = back[off + 2 * w + t];
        return;
    }
    const TriCoef c = tri_coef(tri_aprime(g, m));
    const bool first = g.first != 0, last = g.last != 0;
    const double sc = 1.0 / (g.kscale * g.beta);
    const double xl = back[off + (m - g.pc.cut[j])], xr = back[off + w + (m - g.pc.cut[j])];
    const double spe = tri_spe(c, first);                           // s pe of the front sequence
    TriFwd<true> fw;
    for (int t = 0; t < n; ++t) {
        double gt = x[m + g.plane * t] * sc;
        if (t == 0) gt += xl;
        if (t == n - 1) gt += xr;
        fw.step(c, spe, gt, t, t + 1 < n);
        x[m + g.plane * t] = fw.D;
    }
    const TriEnds f = tri_ends(c, first, n, fw.pw);
    TriBwd<false, true> bw(c, f, fw, last, 0.0, 0.0);
    x[m + g.plane * (n - 1)] = bw.xn;
    for (int t = n - 2; t >= 0; --t) x[m + g.plane * t] = bw.step(c, f, spe, x[m + g.plane * t], t);
}

// Register-resident flavour for short slabs (ntl <= NTL): the column of a mode is read ONCE into registers, both sweeps
// run there, and the result is written once -- one read and one write of the slab.
template <int NTL>
__global__ void __launch_bounds__(256) k_tri_final_reg(TriGeom g, const double *__restrict__ back, double *__restrict__ x) {
    const i64 m = (i64)blockIdx.x * 256 + threadIdx.x;
    if (m >= g.plane) return;
    const int n = (int)g.ntl;
    const int j = tri_owner(g.pc, m, g.plane);
    const i64 off = tri_msg_off(g.pc, j), w = g.pc.cut[j + 1] - g.pc.cut[j];
    if (m == 0) {
        for (int t = 0; t < n; ++t) x[g.plane * t] = back[off + 2 * w + t];
        return;
    }
    const TriCoef c = tri_coef(tri_aprime(g, m));
    const bool first = g.first != 0, last = g.last != 0;
    const double sc = 1.0 / (g.kscale * g.beta);
    const double xl = back[off + (m - g.pc.cut[j])], xr = back[off + w + (m - g.pc.cut[j])];
    double X[NTL];
#pragma unroll
    for (int t = 0; t < NTL; ++t) X[t] = (t < n) ? x[m + g.plane * t] : 0.0;
    const double spe = tri_spe(c, first);
    TriFwd<true> fw;
#pragma unroll
    for (int t = 0; t < NTL; ++t) {
        if (t < n) {
            double gt = X[t] * sc;
            if (t == 0) gt += xl;
            if (t == n - 1) gt += xr;
            fw.step(c, spe, gt, t, t + 1 < n);
            X[t] = fw.D;
        }
    }
    const TriEnds f = tri_ends(c, first, n, fw.pw);
    TriBwd<false, true> bw(c, f, fw, last, 0.0, 0.0);
#pragma unroll
    for (int t = NTL - 1; t >= 0; --t) {
        if (t == n - 1) X[t] = bw.xn;
        else if (t < n - 1) X[t] = bw.step(c, f, spe, X[t], t);
    }
#pragma unroll
    for (int t = 0; t < NTL; ++t)
        if (t < n) x[m + g.plane * t] = X[t];
}

static int tri_reg_width(i64 ntl) {
    return ntl <= 16 ? 16 : (ntl <= 32 ? 32 : (ntl <= 64 ? 64 : 0));
}

static TriGeom make_geom(const Grid &g, i64 nt, double kscale, const double *cy, const double *cx, const PencilCuts &pc) {
    TriGeom t{};
    t.ny = g.py; t.plane = g.plane; t.ntl = g.ntl;
    t.first = g.first ? 1 : 0; t.last = g.last ? 1 : 0;
    t.beta = (double)(nt - 1) * (double)(nt - 1);
    t.kscale = kscale;
    t.cy = cy; t.cx = cx;
    t.pc = pc;
    return t;
}

int launch_tri_local(const Grid &g, i64 nt, double kscale, const double *cy, const double *cx, const PencilCuts &pc,
                     const double *r, double *send, hipStream_t st) {
    const TriGeom t = make_geom(g, nt, kscale, cy, cx, pc);
    const dim3 grid((unsigned)((g.plane + 255) / 256));
    DS_KLAUNCH(k_tri_local, grid, dim3(256), 0, st, t, r, send);
    DS_HIP(hipGetLastError());
    return 0;
}

int launch_tri_reduced(const Grid &g, i64 nt, double kscale, const double *cy, const double *cx, const PencilCuts &pc,
                       int rank, i64 l0, i64 nl, const i64 *slab_n, const double *recv, double *back, double *zero_work,
                       hipStream_t st, const double *own_recv, double *own_back) {
    if (nl <= 0) return 0;
    const TriGeom t = make_geom(g, nt, kscale, cy, cx, pc);
    TriReduced q{};
    q.P = pc.world; q.rank = rank; q.l0 = l0; q.nl = nl; q.nt = nt;
    q.own = (own_recv && own_back) ? rank : -1;
    q.own_recv = own_recv; q.own_back = own_back;
    for (int p = 0; p < pc.world; ++p) q.slab_n[p] = slab_n[p];
    const dim3 grid((unsigned)((nl + 127) / 128));
    if (pc.world <= 4) DS_KLAUNCH(k_tri_reduced<4>, grid, dim3(128), 0, st, t, q, recv, back, zero_work);
    else if (pc.world <= 8) DS_KLAUNCH(k_tri_reduced<8>, grid, dim3(128), 0, st, t, q, recv, back, zero_work);
    else if (pc.world <= 16) DS_KLAUNCH(k_tri_reduced<16>, grid, dim3(128), 0, st, t, q, recv, back, zero_work);
    else DS_KLAUNCH(k_tri_reduced<DS_MAX_WORLD>, grid, dim3(128), 0, st, t, q, recv, back, zero_work);
    DS_HIP(hipGetLastError());
    return 0;
}

int launch_tri_final(const Grid &g, i64 nt, double kscale, const double *cy, const double *cx, const PencilCuts &pc,
                     const double *back, double *x, hipStream_t st) {
    const TriGeom t = make_geom(g, nt, kscale, cy, cx, pc);
    const dim3 grid((unsigned)((g.plane + 255) / 256));
    const int rw = tri_reg_width(g.ntl);
    if (rw == 16) DS_KLAUNCH(k_tri_final_reg<16>, grid, dim3(256), 0, st, t, back, x);
    else if (rw == 32) DS_KLAUNCH(k_tri_final_reg<32>, grid, dim3(256), 0, st, t, back, x);
    else if (rw == 64) DS_KLAUNCH(k_tri_final_reg<64>, grid, dim3(256), 0, st, t, back, x);
    else DS_KLAUNCH(k_tri_final, grid, dim3(256), 0, st, t, back, x);
    DS_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The single slab's t-axis solve by the same elimination (round 4): phi^ = idct_t(dct_t(r^) ./ kernel) IS the solution of
// D^2 ((CY + CX) I + T) phi^ = r^ per (ky, kx) mode, so the t axis needs no transform at all -- for ANY nt.  A workgroup of
// NSUB wavefronts owns 64 consecutive modes (one coalesced 512-byte segment per time layer); wavefront w holds the rows
// [t_w, t_{w+1}) of those modes in registers (R = 32 at nt = 128 / 129: ~110 registers, four waves per SIMD) and the NSUB
// pieces of a column are coupled exactly like time slabs (tsolve_front / tsolve_back of tri_sweep.h: the tile solve both
// kernels below share; each kernel is only the way a tile arrives and leaves).  One read and one write of
// the array, ~20 flops per entry: bound by HBM where the fused transform pass (two FFTs, seven barriers per tile) is
// bound by its own LDS / VALU chain.  Measured: 0.62 ms at 1024 x 1024 x 128 against 0.56 ms for the pipelined transform pass
// (which therefore stays for the power-of-two lengths), 0.66 ms at 1025 x 1025 x 129 against 0.86 ms for the prime-factor pass,
// and no dense t-axis product at all for the other lengths: the default whenever nt is no power of two (Solver::poisson_all).
struct TsPiece {
    int t0, n;                // rows [t0, t0 + n) of piece w: as evenly as possible (dotsocp_slab_range_impl's rule)
};
template <int NSUB>
__device__ __forceinline__ TsPiece ts_piece(i64 nt, int w) {
    const int base = (int)(nt / NSUB), rem = (int)(nt % NSUB);
    auto t_begin = [&](int p) { return p * base + (p < rem ? p : rem); };
    const int t0 = t_begin(w);
    return TsPiece{t0, t_begin(w + 1) - t0};
}

// One tile per workgroup: global loads, the tile solve, stores.
template <int R, int NSUB>
__global__ void __launch_bounds__(64 * NSUB) k_tsolve_single(TriGeom g, i64 nt, double *__restrict__ x) {
    __shared__ double ex[NSUB][6][64];
    __shared__ double zcol[NSUB * R];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const i64 m = (i64)blockIdx.x * 64 + lane;
    const bool ok = m < g.plane;
    const i64 mc = ok ? m : 0;
    const TsPiece pc = ts_piece<NSUB>(nt, w);
    const int t0 = pc.t0, n = pc.n;
    const double sc = 1.0 / (g.kscale * g.beta);
    double X[R];
#pragma unroll
    for (int t = 0; t < R; ++t) X[t] = (t < n) ? x[mc + g.plane * (t0 + t)] * sc : 0.0;
    const bool zero = (m == 0), tile0 = (blockIdx.x == 0);
    const TsMid k = tsolve_front<R, NSUB>(ex, zcol, X, zero ? 1.0 : tri_aprime(g, mc), w, lane, t0, n, tile0);
    __syncthreads();
    tsolve_back<R, NSUB, false>(ex, zcol, X, k, w, lane, n, tile0, nt, g.beta);
    if (ok) {
#pragma unroll
        for (int t = 0; t < R; ++t)
            if (t < n) x[m + g.plane * (t0 + t)] = zero ? zcol[t0 + t] : X[t];
    }
}

// The same solve as a PERSISTENT kernel fed by LDS-DMA (the recipe of dct_pow2.hip's pipelined passes): a workgroup walks tiles of
// 64 modes; the rows of the NEXT tile travel into an LDS image [row][mode] by global_load_lds_dwordx4 (no registers) while
// the current tile is eliminated in registers and stored, so loads are in flight all the time -- the one-tile-per-workgroup
// kernel above alternates between loading and computing (0.62 ms at nt = 128 where the traffic takes 0.4).  One LDS image:
// the DMA of tile i + 1 is issued behind the barrier that follows the front half of tile i (every wave has copied its
// rows to registers by then); it has landed when only the stores issued after it are outstanding (vector-memory operations
// of a wave complete in issue order) -- counted waits and raw barriers, a fence would drain the counter.  The counts hold
// because a wave issues exactly n stores per tile behind the DMA and no other vector-memory instruction: the tile solve
// must not spill.
template <int R, int NSUB>
__global__ void __launch_bounds__(64 * NSUB) k_tsolve_pipe(TriGeom g, i64 nt, int nTiles, double *__restrict__ x) {
    extern __shared__ double img[];                    // [nt rounded up to even][64]
    __shared__ double ex[NSUB][6][64];
    __shared__ double zcol[NSUB * R];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const TsPiece pc = ts_piece<NSUB>(nt, w);
    const int t0 = pc.t0, n = pc.n;
    const double sc = 1.0 / (g.kscale * g.beta);
    const unsigned ldsBase = (unsigned)(uintptr_t)img;
    const int npairs = (int)((nt + 1) / 2);            // one DMA instruction moves two rows (2 x 512 bytes)
    // every wave issues the pairs w, w + NSUB, ...; lane l fetches modes 2 (l & 31), +1 of row 2 pair + (l >> 5)
    auto dma = [&](int tile) {
        const i64 m0 = (i64)tile * 64;
        i64 mm = m0 + 2 * (lane & 31);
        if (mm + 1 >= g.plane) mm = g.plane - 2;       // (plane is even; clamped lanes fetch something valid, never used)
        for (int pr = w; pr < npairs; pr += NSUB) {
            int row = 2 * pr + (lane >> 5);
            if (row >= nt) row = (int)nt - 1;
            glds16(x + mm + g.plane * row, ldsBase + (unsigned)pr * 1024u);
        }
    };
    int tile = blockIdx.x;
    const int stride = gridDim.x;
    if (tile < nTiles) dma(tile);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the waits inside the loop count on the stores of a previous tile)
    for (; tile < nTiles; tile += stride) {
        // the tile has landed when nothing but this wave's stores of the previous tile (issued behind its DMA) is outstanding
        if (n == R) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(R) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"i"(R > 1 ? R - 1 : 0) : "memory");
        lds_barrier();
        const i64 m = (i64)tile * 64 + lane;
        const bool ok = m < g.plane;
        const i64 mc = ok ? m : 0;
        double X[R];
#pragma unroll
        for (int t = 0; t < R; ++t) X[t] = (t < n) ? img[(t0 + t) * 64 + lane] * sc : 0.0;
        const bool zero = (m == 0);
        const TsMid k = tsolve_front<R, NSUB>(ex, zcol, X, zero ? 1.0 : tri_aprime(g, mc), w, lane, t0, n, tile == 0);
        lds_barrier();                                 // every wave has its rows in registers: the image is free
        if (tile + stride < nTiles) dma(tile + stride);
        tsolve_back<R, NSUB, true>(ex, zcol, X, k, w, lane, n, tile == 0, nt, g.beta);
        // exactly n stores per wave and tile (the wait at the top counts them; the count is per wave instruction, not per
        // lane: lanes beyond the plane store nothing)
#pragma unroll
        for (int t = 0; t < R; ++t)
            if (t < n) {
                if (ok) x[m + g.plane * (t0 + t)] = zero ? zcol[t0 + t] : X[t];
            }
    }
}

bool tsolve_tri_supported(i64 nt) { return nt >= 2 && nt <= 512; }

// wavefronts (= pieces of a column) of the kernel launch_tsolve_tri picks for nt: the table of TSOLVE() below; k_tsolve_pipe: 4
static int tsolve_nsub(i64 nt) { return nt <= 8 ? 1 : (nt <= 32 ? 2 : (nt <= 136 ? 4 : 8)); }

// Do the powers rho^t of every mode stay >= TRI_PW_SAFE over a piece (n = ceil(nt / NSUB) rows)?  The backward sweeps of
// k_tsolve_single / k_tsolve_pipe walk rho^t back up from rho^(n-1) and are wrong once that has left the normal range
// (TriBwd<., KEEP = false>, tri_sweep.h).  Largest a': CY, CX <= 4 (n-1)^2.  Pure host arithmetic (dotsocp_tsolve_tri_safe).
bool tsolve_tri_safe(i64 ny, i64 nx, i64 nt) {
    if (!tsolve_tri_supported(nt)) return false;
    const int nsub = tsolve_nsub(nt);
    const double n = (double)((nt + nsub - 1) / nsub);
    const double ap = 4.0 * ((double)(ny - 1) * (double)(ny - 1) + (double)(nx - 1) * (double)(nx - 1)) /
                      ((double)(nt - 1) * (double)(nt - 1));
    const double r = 1.0 + 0.5 * ap + sqrt(ap * (1.0 + 0.25 * ap));     // tri_coef
    return (n - 1.0) * log2(r) <= 500.0;
}

static bool tsolve_pipe_on() {
    const char *pe = getenv("DOTSOCP_TS_PIPE");        // read per call: the tests switch it inside one process
    return !(pe && atoi(pe) == 0);
}
// the persistent LDS-DMA flavour: grids with enough tiles to keep two workgroups per CU busy for many rounds; its image
// fits twice into a CU's LDS up to nt = 136
static bool tsolve_pipe_fits(i64 nt, i64 plane, int ncu) {
    return nt > 64 && nt <= 136 && (plane + 63) / 64 >= 16 * (i64)ncu && (plane % 2) == 0;
}
bool tsolve_tri_pipelined(i64 nt, i64 plane, int ncu) { return tsolve_pipe_on() && tsolve_pipe_fits(nt, plane, ncu); }
// Is the tridiagonal solve the faster t-axis solve of a single slab?  Every length without a power-of-two transform pass
// (prime-factor lengths 0.66 vs 0.86 ms at 1025 x 1025 x 129, and no dense product along t for the rest); powers of two
// where the pipelined flavour applies (0.51 vs 0.56 ms at 1024 x 1024 x 128; the one-tile-per-workgroup kernel: 0.62).
bool tsolve_tri_preferred(i64 nt, bool pow2, i64 plane, int ncu) {
    if (!tsolve_tri_supported(nt)) return false;
    return !pow2 || tsolve_tri_pipelined(nt, plane, ncu);
}

// in place on x: [plane][nt] with plane = py * nx doubles per layer (pad entries of a row are modes of their own: zeros)
int launch_tsolve_tri(const Grid &g, i64 nt, double kscale, const double *cy, const double *cx, double *x, hipStream_t st) {
    PencilCuts pc{};
    pc.world = 1;
    pc.cut[0] = 0;
    pc.cut[1] = g.plane;
    const TriGeom t = make_geom(g, nt, kscale, cy, cx, pc);
    const dim3 grid((unsigned)((g.plane + 63) / 64));
    const int nTiles = (int)((g.plane + 63) / 64);
    const size_t img = (size_t)((nt + 1) / 2) * 2 * 64 * sizeof(double);
    // persistent LDS-DMA flavour (DOTSOCP_TS_PIPE=0: the one-tile-per-workgroup kernel)
    const int G = 2 * device_cus();
    if (tsolve_tri_pipelined(nt, g.plane, device_cus())) {
        static std::mutex mu;
        static unsigned long long done = 0;
        int dev = 0;
        (void)hipGetDevice(&dev);
        {
            std::lock_guard<std::mutex> lock(mu);
            if (dev >= 0 && dev < 64 && !(done & (1ull << dev))) {
                (void)hipFuncSetAttribute((const void *)(k_tsolve_pipe<32, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024);
                (void)hipFuncSetAttribute((const void *)(k_tsolve_pipe<34, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024);
                done |= 1ull << dev;
            }
        }
        if (nt <= 128) DS_KLAUNCH((k_tsolve_pipe<32, 4>), dim3((unsigned)G), dim3(256), img, st, t, nt, nTiles, x);
        else DS_KLAUNCH((k_tsolve_pipe<34, 4>), dim3((unsigned)G), dim3(256), img, st, t, nt, nTiles, x);
        DS_HIP(hipGetLastError());
        return 0;
    }
#define TSOLVE(RR, NS) DS_KLAUNCH((k_tsolve_single<RR, NS>), grid, dim3(64 * NS), 0, st, t, nt, x)
    if (nt <= 8) TSOLVE(8, 1);
    else if (nt <= 16) TSOLVE(8, 2);
    else if (nt <= 32) TSOLVE(16, 2);
    else if (nt <= 64) TSOLVE(16, 4);
    else if (nt <= 128) TSOLVE(32, 4);
    else if (nt <= 136) TSOLVE(34, 4);
    else if (nt <= 256) TSOLVE(32, 8);
    else if (nt <= 272) TSOLVE(34, 8);
    else if (nt <= 512) TSOLVE(64, 8);
    else { set_error("tridiagonal t-solve: nt > 512"); return DOTSOCP_EINVAL; }
#undef TSOLVE
    DS_HIP(hipGetLastError());
    return 0;
}

__global__ void __launch_bounds__(256) k_gather_msgs(GatherMsgs a) {
    const int m = blockIdx.y;
    const double *__restrict__ s = a.src[m];
    double *__restrict__ d = a.dst[m];
    const i64 c = a.count[m];
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < c; i += (i64)gridDim.x * 256) d[i] = s[i];
}

int launch_gather_msgs(const GatherMsgs &m, hipStream_t st) {
    if (m.n <= 0) return 0;
    i64 cmax = 0;
    for (int i = 0; i < m.n; ++i) cmax = m.count[i] > cmax ? m.count[i] : cmax;
    if (cmax <= 0) return 0;
    const unsigned bx = (unsigned)launch_blocks(cmax, 256, 256);
    DS_KLAUNCH(k_gather_msgs, dim3(bx, (unsigned)m.n), dim3(256), 0, st, m);
    DS_HIP(hipGetLastError());
    return 0;
}

}  // namespace dotsocp
