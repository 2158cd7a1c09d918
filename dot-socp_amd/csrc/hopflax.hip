// Hopf-Lax transform of a node layer and the sums of the dual bound (include/dotsocp.h: dotsocp_dual_bound; host side:
// solver_dual.hip; numpy twin: dot-socp_amd/dual.py).
//
// One axis, n nodes, w = (0.5 h) h:  forward out[j] = min_i in[i] + (double)((i - j)^2) w,  backward out[i] = max_j in[j] -
// (double)((i - j)^2) w, the smallest winning index on ties, the value that of the winning candidate.  Plain min-plus passes:
// n candidates per output, each one add, one compare and the selects of value and index.  A thread keeps several outputs
// (value, index) in registers and scans ALL inputs of its line in ascending order with a strict compare, so the tie rule
// needs no combination step: chunks only bound what is staged in LDS at a time --
//   * the inputs of the chunk (non-finite entries replaced by +Inf / -Inf as they are staged), and
//   * the window of the distance table d^2 w that the chunk and the workgroup's outputs span, formed on the spot: the square
//     exactly in 64-bit integers, one conversion, one product.
// k_hl_pass_y: lines along the contiguous axis (the y pass; a 1-D problem's line).  A workgroup owns up to HL_YOUT
//   consecutive outputs of ONE line, thread u the outputs u, u + 256, ..: the 64 lanes read 64 consecutive table entries (no
//   bank conflict), the input is one broadcast read per candidate row.  Slices of 256 outputs behind the line's end are
//   skipped per wavefront.
// k_hl_pass_x: lines along the strided axis (the x pass).  A lane is a line (64 consecutive y: coalesced loads and stores),
//   a thread owns HL_XR consecutive outputs of it; the table entry is the same for all lanes (broadcast).
// k_hl_reduce: one thread per node in memory order (y fastest, no pitch): the nine sums by the tree of dotsocp_map_report
//   ("Sums": wavefront halving tree, ((w0 + w1) + w2) + w3, launch_report_rows over the workgroups), the extrema of the two
//   gaps as order-preserving integer keys and the count of non-finite potentials by integer atomics; it also writes the flat
//   winner of every node, iy + ny * ix[iy, x'].
#include <cmath>
#include <cstdlib>

#include "device_utils.h"
#include "kernels.h"

namespace dotsocp {

#define HL_BLOCK 256
#define HL_R (HL_YOUT / HL_BLOCK)       // outputs a thread of the y pass owns
#define HL_XWAVES (HL_BLOCK / 64)
#define HL_XR (HL_XOUT / HL_XWAVES)     // outputs a thread of the x pass owns

struct HlArgs {
    const double *in;
    double *out;
    int *arg;
    i64 n, lines;       // nodes of a line, lines
    i64 pitch;          // y pass: doubles between two lines; x pass: doubles between two nodes of a line (lines are 1 apart)
    double w;           // (0.5 h) h
    int chunk;          // inputs staged at a time
};

template <bool FWD> __device__ __forceinline__ double hl_clean(double v) {
    return isfinite(v) ? v : (FWD ? INFINITY : -INFINITY);
}

// candidates of the staged inputs [0, cnt) for NR outputs whose table rows start at t[-256 r]
template <bool FWD, int NR>
__device__ __forceinline__ void hl_scan_y(const double *s_in, const double *t, int cnt, int i0, double (&best)[HL_R], int (&bi)[HL_R]) {
    for (int ii = 0; ii < cnt; ++ii) {
        const double v = s_in[ii];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const double d = t[ii - HL_BLOCK * r];
            const double c = FWD ? v + d : v - d;
            const bool take = FWD ? c < best[r] : c > best[r];
            best[r] = take ? c : best[r];
            bi[r] = take ? i0 + ii : bi[r];
        }
    }
}

template <bool FWD>
__global__ void __launch_bounds__(HL_BLOCK) k_hl_pass_y(HlArgs a) {
    __shared__ double s_in[HL_CHUNK_MAX];
    __shared__ double s_tab[HL_CHUNK_MAX + HL_YOUT];
    const int tid = threadIdx.x;
    const i64 tiles = (a.n + HL_YOUT - 1) / HL_YOUT;
    const i64 line = (i64)blockIdx.x / tiles, j0 = ((i64)blockIdx.x % tiles) * HL_YOUT;
    const double *in = a.in + line * a.pitch;
    // slices of 256 outputs in which this wavefront has one (the same for its 64 lanes)
    int nr = 0;
#pragma unroll
    for (int r = 0; r < HL_R; ++r)
        if (j0 + (tid & ~63) + HL_BLOCK * r < a.n) nr = r + 1;
    nr = __builtin_amdgcn_readfirstlane(nr);
    double best[HL_R];
    int bi[HL_R];
#pragma unroll
    for (int r = 0; r < HL_R; ++r) { best[r] = FWD ? INFINITY : -INFINITY; bi[r] = 0; }
    // output o = tid + 256 r of the workgroup and input ii of the chunk are d = (i0 + ii) - (j0 + o) apart: slot ii + (HL_YOUT - 1) - o
    const double *t = s_tab + (HL_YOUT - 1) - tid;
    for (i64 i0 = 0; i0 < a.n; i0 += a.chunk) {
        const int cnt = (int)(a.n - i0 < a.chunk ? a.n - i0 : a.chunk);
        __syncthreads();            // the chunk before is used up
        for (int k = tid; k < cnt; k += HL_BLOCK) s_in[k] = hl_clean<FWD>(in[i0 + k]);
        for (int k = tid; k < cnt + HL_YOUT - 1; k += HL_BLOCK) {
            const i64 d = i0 - j0 + (k - (HL_YOUT - 1));
            s_tab[k] = (double)(d * d) * a.w;
        }
        __syncthreads();
        switch (nr) {
            case 1: hl_scan_y<FWD, 1>(s_in, t, cnt, (int)i0, best, bi); break;
            case 2: hl_scan_y<FWD, 2>(s_in, t, cnt, (int)i0, best, bi); break;
            case 3: hl_scan_y<FWD, 3>(s_in, t, cnt, (int)i0, best, bi); break;
            case 4: hl_scan_y<FWD, 4>(s_in, t, cnt, (int)i0, best, bi); break;
            default: break;
        }
    }
    static_assert(HL_R == 4, "the switch above lists the slice counts 1 .. HL_R");
#pragma unroll
    for (int r = 0; r < HL_R; ++r) {
        const i64 j = j0 + tid + HL_BLOCK * r;
        if (j < a.n) {
            a.out[line * a.pitch + j] = best[r];
            a.arg[line * a.pitch + j] = bi[r];
        }
    }
}

template <bool FWD>
__global__ void __launch_bounds__(HL_BLOCK) k_hl_pass_x(HlArgs a) {
    __shared__ double s_in[HL_XCHUNK_MAX][64];
    __shared__ double s_tab[HL_XCHUNK_MAX + HL_XOUT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const i64 ltiles = (a.lines + 63) / 64;
    const i64 y = ((i64)blockIdx.x % ltiles) * 64 + lane, j0 = ((i64)blockIdx.x / ltiles) * HL_XOUT;
    const bool live = y < a.lines;
    const bool work = j0 + wv * HL_XR < a.n;      // this wavefront has an output (the same for its 64 lanes)
    double best[HL_XR];
    int bi[HL_XR];
#pragma unroll
    for (int r = 0; r < HL_XR; ++r) { best[r] = FWD ? INFINITY : -INFINITY; bi[r] = 0; }
    // output o = HL_XR wv + r and input ii of the chunk are d = (i0 + ii) - (j0 + o) apart: slot ii + (HL_XOUT - 1) - o
    const double *t = s_tab + (HL_XOUT - 1) - wv * HL_XR;
    for (i64 i0 = 0; i0 < a.n; i0 += a.chunk) {
        const int cnt = (int)(a.n - i0 < a.chunk ? a.n - i0 : a.chunk);
        __syncthreads();            // the chunk before is used up
        for (int k = wv; k < cnt; k += HL_XWAVES) s_in[k][lane] = live ? hl_clean<FWD>(a.in[y + a.pitch * (i0 + k)]) : 0.0;
        for (int k = tid; k < cnt + HL_XOUT - 1; k += HL_BLOCK) {
            const i64 d = i0 - j0 + (k - (HL_XOUT - 1));
            s_tab[k] = (double)(d * d) * a.w;
        }
        __syncthreads();
        if (!work) continue;
        for (int ii = 0; ii < cnt; ++ii) {
            const double v = s_in[ii][lane];
#pragma unroll
            for (int r = 0; r < HL_XR; ++r) {
                const double d = t[ii - r];
                const double c = FWD ? v + d : v - d;
                const bool take = FWD ? c < best[r] : c > best[r];
                best[r] = take ? c : best[r];
                bi[r] = take ? (int)i0 + ii : bi[r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < HL_XR; ++r) {
        const i64 j = j0 + wv * HL_XR + r;
        if (live && j < a.n) {
            a.out[y + a.pitch * j] = best[r];
            a.arg[y + a.pitch * j] = bi[r];
        }
    }
}

int hl_chunk(int deflt) {
    int c = deflt;
    if (const char *e = getenv("DOTSOCP_HL_CHUNK")) c = atoi(e);
    return c < 1 ? 1 : (c > deflt ? deflt : c);
}

static int hl_launch_check(i64 n, i64 lines, i64 blocks) {
    if (n < 2 || n > HL_MAX_LEN || lines < 1 || blocks > 0x7fffffffLL) {
        set_error("invalid argument: dual_bound() transforms lines of 2 .. 2^20 nodes (%lld lines of %lld)", lines, n);
        return DOTSOCP_EINVAL;
    }
    return 0;
}

int launch_hl_pass_y(bool forward, const double *in, double *out, int *arg, i64 n, i64 lines, i64 pitch, hipStream_t st) {
    const i64 blocks = ((n + HL_YOUT - 1) / HL_YOUT) * lines;
    DS_CHECK(hl_launch_check(n, lines, blocks));
    const double h = 1.0 / (double)(n - 1);
    HlArgs a{in, out, arg, n, lines, pitch, (0.5 * h) * h, hl_chunk(HL_CHUNK_MAX)};
    if (forward) DS_KLAUNCH(k_hl_pass_y<true>, dim3((unsigned)blocks), dim3(HL_BLOCK), 0, st, a);
    else DS_KLAUNCH(k_hl_pass_y<false>, dim3((unsigned)blocks), dim3(HL_BLOCK), 0, st, a);
    DS_HIP(hipGetLastError());
    return 0;
}

int launch_hl_pass_x(bool forward, const double *in, double *out, int *arg, i64 n, i64 lines, i64 pitch, hipStream_t st) {
    const i64 blocks = ((n + HL_XOUT - 1) / HL_XOUT) * ((lines + 63) / 64);
    DS_CHECK(hl_launch_check(n, lines, blocks));
    const double h = 1.0 / (double)(n - 1);
    HlArgs a{in, out, arg, n, lines, pitch, (0.5 * h) * h, hl_chunk(HL_XCHUNK_MAX)};
    if (forward) DS_KLAUNCH(k_hl_pass_x<true>, dim3((unsigned)blocks), dim3(HL_BLOCK), 0, st, a);
    else DS_KLAUNCH(k_hl_pass_x<false>, dim3((unsigned)blocks), dim3(HL_BLOCK), 0, st, a);
    DS_HIP(hipGetLastError());
    return 0;
}

// out = mul * in (recoverOrgVar's phi = dScale * phi on one layer, pad entries included)
__global__ void __launch_bounds__(HL_BLOCK) k_hl_layer(const double *__restrict__ in, double *__restrict__ out, i64 n, double mul) {
    const i64 i = (i64)blockIdx.x * HL_BLOCK + threadIdx.x;
    if (i < n) out[i] = mul * in[i];
}

int launch_hl_layer(const double *in, double *out, i64 n, double mul, hipStream_t st) {
    if (n <= 0) return 0;
    DS_KLAUNCH(k_hl_layer, dim3((unsigned)((n + HL_BLOCK - 1) / HL_BLOCK)), dim3(HL_BLOCK), 0, st, in, out, n, mul);
    DS_HIP(hipGetLastError());
    return 0;
}

__global__ void __launch_bounds__(HL_BLOCK) k_hl_reduce(HlReduceArgs a) {
    __shared__ unsigned long long s_key[4];
    __shared__ unsigned int s_bad;
    __shared__ double s_red[HL_BLOCK / 64][HS_COUNT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid < 4) s_key[tid] = 0;
    if (tid == 4) s_bad = 0;
    __syncthreads();
    const i64 node = (i64)blockIdx.x * HL_BLOCK + tid;
    double v[HS_COUNT];
#pragma unroll
    for (int i = 0; i < HS_COUNT; ++i) v[i] = 0.0;
    if (node < a.ny * a.nx) {
        const i64 x = node / a.ny, y = node - x * a.ny, at = y + a.py * x;
        const double p0 = a.phi0[at], p1 = a.phi1[at], H = a.H[at], B = a.B[at], r0 = a.rho0[at], r1 = a.rho1[at];
        // the winners: (iy, ix[iy, x]) of the two passes (1-D: iy alone)
        const int fy = a.iyf[at], by = a.iyb[at];
        const int fx = a.ixf ? a.ixf[fy + a.py * x] : 0, bx = a.ixb ? a.ixb[by + a.py * x] : 0;
        a.arg_fwd[at] = (int)(fy + a.ny * fx);
        a.arg_bwd[at] = (int)(by + a.ny * bx);
        const double ex = (double)(x - bx) * a.hx, ey = (double)(y - by) * a.hy;
        const double d2 = a.ixb ? ex * ex + ey * ey : ey * ey;
        const double g1 = p1 - H, g0 = p0 - B;
        v[HS_M0] = r0;
        v[HS_M1] = r1;
        v[HS_P0R0] = p0 * r0;
        v[HS_P1R1] = p1 * r1;
        v[HS_HR1] = H * r1;
        v[HS_BR0] = B * r0;
        v[HS_G1] = fabs(g1) * r1;
        v[HS_G0] = fabs(g0) * r0;
        v[HS_MAP] = r0 * d2;
        if (isfinite(g1)) { atomicMax(&s_key[HC_G1_MAX], report_key(g1 + 0.0)); atomicMax(&s_key[HC_G1_MIN], ~report_key(g1 + 0.0)); }
        if (isfinite(g0)) { atomicMax(&s_key[HC_G0_MAX], report_key(g0 + 0.0)); atomicMax(&s_key[HC_G0_MIN], ~report_key(g0 + 0.0)); }
        const unsigned int bad = (isfinite(p0) ? 0u : 1u) + (isfinite(p1) ? 0u : 1u);
        if (bad) atomicAdd(&s_bad, bad);
    }
#pragma unroll
    for (int i = 0; i < HS_COUNT; ++i) {
        double s = v[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) s_red[wv][i] = s;
    }
    __syncthreads();
    if (tid < HS_COUNT) {
        double s = s_red[0][tid];
#pragma unroll
        for (int w = 1; w < HL_BLOCK / 64; ++w) s += s_red[w][tid];
        a.partials[(i64)tid * gridDim.x + blockIdx.x] = s;
    }
    if (tid >= 64 && tid < 68) {
        if (s_key[tid - 64]) atomicMax(&a.counts[tid - 64], s_key[tid - 64]);
    } else if (tid == 68 && s_bad) {
        atomicAdd(&a.counts[HC_NONFINITE], (unsigned long long)s_bad);
    }
}

i64 hl_blocks(i64 nodes) { return (nodes + HL_BLOCK - 1) / HL_BLOCK; }

int launch_hl_reduce(const HlReduceArgs &a, double *sums, hipStream_t st) {
    const i64 blocks = hl_blocks(a.ny * a.nx);
    if (blocks < 1 || blocks > 0x7fffffffLL) { set_error("invalid argument: dual_bound() serves layers of up to 2^39 nodes"); return DOTSOCP_EINVAL; }
    DS_KLAUNCH(k_hl_reduce, dim3((unsigned)blocks), dim3(HL_BLOCK), 0, st, a);
    DS_HIP(hipGetLastError());
    return launch_report_rows(a.partials, blocks, HS_COUNT, sums, st);
}

}  // namespace dotsocp
