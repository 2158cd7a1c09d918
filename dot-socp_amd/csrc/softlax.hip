// Soft Hopf-Lax transform of a node layer and the node kernels of the upper bound (include/dotsocp.h: dotsocp_plan_bound,
// dotsocp_upper_bound; host side: solver_upper.hip; numpy twin: dot-socp_amd/upper.py), and of the transport map of its plan
// (dotsocp_plan_map, dotsocp_upper_map): the moment flavour of the two passes, k_sl_map, the frame kernels.
//
// One axis, n nodes, w = (0.5 h) h: for output j over the candidates c_i = in[i] + (double)((i - j)^2) w
//   m = min_i c_i,   s = sum_i exp((m - c_i) ieps),   q = sum_i exp((m - c_i) ieps) ((double)((i - j)^2) w + pm[i]),
//   out[j] = m - eps log(s),   mean[j] = q / s
// -- the min-plus pass of hopflax.hip with a log-sum-exp in the place of the min.  The kernels keep that file's layout: a
// thread owns several outputs in registers and scans ALL inputs of its line in ascending order, chunks only bound what is
// staged in LDS at a time (the inputs, their prior means, the window of the distance table), so s and q are added in one
// fixed order whatever the tiles and chunks are.  The line is scanned twice: for m, then for the sums.
// A term is skipped only where the argument of exp lies below -746 in every lane of the wavefront (y pass: per slice of
// outputs; x pass: for all outputs of the thread): exp is then exactly +0.0 and s + 0.0, q + 0.0 * t leave the accumulators
// as they are.  At eps = h^2 / 4 that is all but about 40 candidates around an output, so few exponentials are left: what
// the pass costs is the two scans.
// k_sl_pass_y: lines along the contiguous axis, a workgroup owns up to HL_YOUT consecutive outputs of ONE line, thread u the
//   outputs u, u + 256, ...   k_sl_pass_x: lines along the strided axis, a lane is a line, a thread owns SL_XR consecutive outputs.
// Node kernels: one thread per node in memory order; sums by the tree of k_hl_reduce (wavefront halving tree,
//   ((w0 + w1) + w2) + w3, launch_report_rows over the workgroups), counts by integer atomics.  No floating-point atomic.
#include <cmath>

#include "device_utils.h"
#include "kernels.h"

namespace dotsocp {

#define SL_BLOCK 256
#define SL_R (HL_YOUT / SL_BLOCK)       // outputs a thread of the y pass owns
#define SL_XWAVES (SL_BLOCK / 64)
#define SL_XR (HL_XOUT / SL_XWAVES)     // outputs a thread of the x pass owns
#define SL_EXP_ZERO (-746.0)            // exp(x) is +0.0 for every x below

struct SlArgs {
    const double *in, *pm;
    double *out, *mean;
    i64 n, lines;
    i64 pitch;          // y pass: doubles between two lines; x pass: doubles between two nodes of a line (lines are 1 apart)
    double w, eps, ieps;
    int chunk;          // inputs staged at a time
    static constexpr bool MOM = false;
};
// the moment flavour (dotsocp_plan_map): beside s and q the signed displacement along the pass's own axis, candidate minus
// output, qa = sum e * ((double)(i - j) * h), and a prior displacement of the other axis carried through, qb = sum e * pb[i]
// (the y pass of a layer; the x pass and a line have none).  da = qa / s, db = qb / s, 0 on a dead line.  The plain kernels
// are the instantiation without: same statements, same order -- out and mean carry the same bits in both.
struct SlMomArgs : SlArgs {
    const double *pb;   // y pass: the x pass's mean displacement, in the layout of `in`, or nullptr
    double *da, *db;    // db: y pass with pb only
    double h;
    static constexpr bool MOM = true;
};

__device__ __forceinline__ double sl_clean(double v) { return isfinite(v) ? v : INFINITY; }

__device__ __forceinline__ bool sl_wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }

template <int NR>
__device__ __forceinline__ void sl_min_y(const double *s_in, const double *t, int cnt, double (&m)[SL_R]) {
    for (int ii = 0; ii < cnt; ++ii) {
        const double v = s_in[ii];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const double c = v + t[ii - SL_BLOCK * r];
            m[r] = c < m[r] ? c : m[r];
        }
    }
}

// MOM: dj = i0 - (j0 + tid), so that candidate ii of the chunk and the output of slice r are dj + ii - 256 r nodes apart
template <int NR, bool MOM>
__device__ __forceinline__ void sl_sum_y(const double *s_in, const double *s_pm, const double *t, int cnt, double ieps,
                                         const double (&m)[SL_R], double (&s)[SL_R], double (&q)[SL_R], i64 dj, double h,
                                         double (&qa)[MOM ? SL_R : 1], double (&qb)[MOM ? SL_R : 1]) {
    for (int ii = 0; ii < cnt; ++ii) {
        const double v = s_in[ii], p = s_pm[ii];
        const double pb = MOM ? s_pm[HL_CHUNK_MAX + ii] : 0.0;
        // the slices are 256 outputs apart: each has its own window of candidates that count, so each votes for itself
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const double d = t[ii - SL_BLOCK * r];
            const double x = (m[r] - (v + d)) * ieps;
            if (!sl_wave_any(x >= SL_EXP_ZERO)) continue;
            const double e = exp(x);
            s[r] = s[r] + e;
            q[r] = q[r] + e * (d + p);
            if constexpr (MOM) {
                qa[r] = qa[r] + e * ((double)(dj + ii - SL_BLOCK * r) * h);
                qb[r] = qb[r] + e * pb;
            }
        }
    }
}

template <class Args>
__global__ void __launch_bounds__(SL_BLOCK) k_sl_pass_y(Args a) {
    constexpr bool MOM = Args::MOM;
    __shared__ double s_in[HL_CHUNK_MAX];
    __shared__ double s_pm[(MOM ? 2 : 1) * HL_CHUNK_MAX];     // MOM: the prior displacement behind the prior mean
    __shared__ double s_tab[HL_CHUNK_MAX + HL_YOUT];
    const int tid = threadIdx.x;
    const i64 tiles = (a.n + HL_YOUT - 1) / HL_YOUT;
    const i64 line = (i64)blockIdx.x / tiles, j0 = ((i64)blockIdx.x % tiles) * HL_YOUT;
    const double *in = a.in + line * a.pitch;
    const double *pm = a.pm ? a.pm + line * a.pitch : nullptr;
    // slices of 256 outputs in which this wavefront has one (the same for its 64 lanes)
    int nr = 0;
#pragma unroll
    for (int r = 0; r < SL_R; ++r)
        if (j0 + (tid & ~63) + SL_BLOCK * r < a.n) nr = r + 1;
    nr = __builtin_amdgcn_readfirstlane(nr);
    double m[SL_R], s[SL_R], q[SL_R], qa[MOM ? SL_R : 1], qb[MOM ? SL_R : 1];
#pragma unroll
    for (int r = 0; r < SL_R; ++r) { m[r] = INFINITY; s[r] = 0.0; q[r] = 0.0; }
    if constexpr (MOM) {
#pragma unroll
        for (int r = 0; r < SL_R; ++r) { qa[r] = 0.0; qb[r] = 0.0; }
    }
    const double *pb = nullptr;
    double h = 0.0;
    if constexpr (MOM) { pb = a.pb ? a.pb + line * a.pitch : nullptr; h = a.h; }
    // output o = tid + 256 r of the workgroup and input ii of the chunk are d = (i0 + ii) - (j0 + o) apart: slot ii + (HL_YOUT - 1) - o
    const double *t = s_tab + (HL_YOUT - 1) - tid;
    for (int phase = 0; phase < 2; ++phase) {
        for (i64 i0 = 0; i0 < a.n; i0 += a.chunk) {
            const int cnt = (int)(a.n - i0 < a.chunk ? a.n - i0 : a.chunk);
            __syncthreads();            // the chunk before is used up
            for (int k = tid; k < cnt; k += SL_BLOCK) {
                s_in[k] = sl_clean(in[i0 + k]);
                if (phase) s_pm[k] = pm ? pm[i0 + k] : 0.0;
                if constexpr (MOM) { if (phase) s_pm[HL_CHUNK_MAX + k] = pb ? pb[i0 + k] : 0.0; }
            }
            for (int k = tid; k < cnt + HL_YOUT - 1; k += SL_BLOCK) {
                const i64 d = i0 - j0 + (k - (HL_YOUT - 1));
                s_tab[k] = (double)(d * d) * a.w;
            }
            __syncthreads();
            if (phase == 0) {
                switch (nr) {
                    case 1: sl_min_y<1>(s_in, t, cnt, m); break;
                    case 2: sl_min_y<2>(s_in, t, cnt, m); break;
                    case 3: sl_min_y<3>(s_in, t, cnt, m); break;
                    case 4: sl_min_y<4>(s_in, t, cnt, m); break;
                    default: break;
                }
            } else {
                const i64 dj = i0 - (j0 + tid);
                switch (nr) {
                    case 1: sl_sum_y<1, MOM>(s_in, s_pm, t, cnt, a.ieps, m, s, q, dj, h, qa, qb); break;
                    case 2: sl_sum_y<2, MOM>(s_in, s_pm, t, cnt, a.ieps, m, s, q, dj, h, qa, qb); break;
                    case 3: sl_sum_y<3, MOM>(s_in, s_pm, t, cnt, a.ieps, m, s, q, dj, h, qa, qb); break;
                    case 4: sl_sum_y<4, MOM>(s_in, s_pm, t, cnt, a.ieps, m, s, q, dj, h, qa, qb); break;
                    default: break;
                }
            }
        }
    }
    static_assert(SL_R == 4, "the switches above list the slice counts 1 .. SL_R");
#pragma unroll
    for (int r = 0; r < SL_R; ++r) {
        const i64 j = j0 + tid + SL_BLOCK * r;
        if (j < a.n) {
            const bool dead = !(m[r] < INFINITY);
            a.out[line * a.pitch + j] = dead ? INFINITY : m[r] - a.eps * log(s[r]);
            a.mean[line * a.pitch + j] = dead ? 0.0 : q[r] / s[r];
            if constexpr (MOM) {
                a.da[line * a.pitch + j] = dead ? 0.0 : qa[r] / s[r];
                if (a.db) a.db[line * a.pitch + j] = dead ? 0.0 : qb[r] / s[r];
            }
        }
    }
}

template <class Args>
__global__ void __launch_bounds__(SL_BLOCK) k_sl_pass_x(Args a) {
    constexpr bool MOM = Args::MOM;
    __shared__ double s_in[HL_XCHUNK_MAX][64];
    __shared__ double s_tab[HL_XCHUNK_MAX + HL_XOUT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const i64 ltiles = (a.lines + 63) / 64;
    const i64 y = ((i64)blockIdx.x % ltiles) * 64 + lane, j0 = ((i64)blockIdx.x / ltiles) * HL_XOUT;
    const bool live = y < a.lines;
    const bool work = j0 + wv * SL_XR < a.n;      // this wavefront has an output (the same for its 64 lanes)
    double m[SL_XR], s[SL_XR], q[SL_XR], qa[MOM ? SL_XR : 1];
#pragma unroll
    for (int r = 0; r < SL_XR; ++r) { m[r] = INFINITY; s[r] = 0.0; q[r] = 0.0; }
    double h = 0.0;
    if constexpr (MOM) {
#pragma unroll
        for (int r = 0; r < SL_XR; ++r) qa[r] = 0.0;
        h = a.h;
    }
    // output o = SL_XR wv + r and input ii of the chunk are d = (i0 + ii) - (j0 + o) apart: slot ii + (HL_XOUT - 1) - o
    const double *t = s_tab + (HL_XOUT - 1) - wv * SL_XR;
    for (int phase = 0; phase < 2; ++phase) {
        for (i64 i0 = 0; i0 < a.n; i0 += a.chunk) {
            const int cnt = (int)(a.n - i0 < a.chunk ? a.n - i0 : a.chunk);
            __syncthreads();            // the chunk before is used up
            for (int k = wv; k < cnt; k += SL_XWAVES) s_in[k][lane] = live ? sl_clean(a.in[y + a.pitch * (i0 + k)]) : INFINITY;
            for (int k = tid; k < cnt + HL_XOUT - 1; k += SL_BLOCK) {
                const i64 d = i0 - j0 + (k - (HL_XOUT - 1));
                s_tab[k] = (double)(d * d) * a.w;
            }
            __syncthreads();
            if (!work) continue;
            if (phase == 0) {
                for (int ii = 0; ii < cnt; ++ii) {
                    const double v = s_in[ii][lane];
#pragma unroll
                    for (int r = 0; r < SL_XR; ++r) {
                        const double c = v + t[ii - r];
                        m[r] = c < m[r] ? c : m[r];
                    }
                }
            } else {
                for (int ii = 0; ii < cnt; ++ii) {
                    const double v = s_in[ii][lane];
                    double d[SL_XR], x[SL_XR];
                    bool some = false;
#pragma unroll
                    for (int r = 0; r < SL_XR; ++r) {
                        d[r] = t[ii - r];
                        x[r] = (m[r] - (v + d[r])) * a.ieps;
                        some = some || x[r] >= SL_EXP_ZERO;
                    }
                    if (!sl_wave_any(some)) continue;
#pragma unroll
                    for (int r = 0; r < SL_XR; ++r) {
                        const double e = exp(x[r]);
                        s[r] = s[r] + e;
                        q[r] = q[r] + e * d[r];
                        if constexpr (MOM) qa[r] = qa[r] + e * ((double)(i0 + ii - (j0 + wv * SL_XR + r)) * h);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < SL_XR; ++r) {
        const i64 j = j0 + wv * SL_XR + r;
        if (live && j < a.n) {
            const bool dead = !(m[r] < INFINITY);
            a.out[y + a.pitch * j] = dead ? INFINITY : m[r] - a.eps * log(s[r]);
            a.mean[y + a.pitch * j] = dead ? 0.0 : q[r] / s[r];
            if constexpr (MOM) a.da[y + a.pitch * j] = dead ? 0.0 : qa[r] / s[r];
        }
    }
}

static int sl_launch_check(i64 n, i64 lines, i64 blocks, double eps) {
    if (n < 2 || n > HL_MAX_LEN || lines < 1 || blocks > 0x7fffffffLL || !(eps > 0.0) || !std::isfinite(eps)) {
        set_error("invalid argument: the soft transform takes lines of 2 .. 2^20 nodes and a positive finite eps (%lld lines of %lld)", lines, n);
        return DOTSOCP_EINVAL;
    }
    return 0;
}

int launch_sl_pass_y(const double *in, const double *pm, double *out, double *mean, i64 n, i64 lines, i64 pitch, double eps,
                     hipStream_t st) {
    const i64 blocks = ((n + HL_YOUT - 1) / HL_YOUT) * lines;
    DS_CHECK(sl_launch_check(n, lines, blocks, eps));
    const double h = 1.0 / (double)(n - 1);
    SlArgs a{in, pm, out, mean, n, lines, pitch, (0.5 * h) * h, eps, 1.0 / eps, hl_chunk(HL_CHUNK_MAX)};
    DS_KLAUNCH(k_sl_pass_y<SlArgs>, dim3((unsigned)blocks), dim3(SL_BLOCK), 0, st, a);
    DS_HIP(hipGetLastError());
    return 0;
}

int launch_sl_mom_y(const double *in, const double *pm, const double *pb, double *out, double *mean, double *da, double *db,
                    i64 n, i64 lines, i64 pitch, double eps, hipStream_t st) {
    const i64 blocks = ((n + HL_YOUT - 1) / HL_YOUT) * lines;
    DS_CHECK(sl_launch_check(n, lines, blocks, eps));
    const double h = 1.0 / (double)(n - 1);
    SlMomArgs a{{in, pm, out, mean, n, lines, pitch, (0.5 * h) * h, eps, 1.0 / eps, hl_chunk(HL_CHUNK_MAX)}, pb, da, pb ? db : nullptr, h};
    DS_KLAUNCH(k_sl_pass_y<SlMomArgs>, dim3((unsigned)blocks), dim3(SL_BLOCK), 0, st, a);
    DS_HIP(hipGetLastError());
    return 0;
}

int launch_sl_pass_x(const double *in, double *out, double *mean, i64 n, i64 lines, i64 pitch, double eps, hipStream_t st) {
    const i64 blocks = ((n + HL_XOUT - 1) / HL_XOUT) * ((lines + 63) / 64);
    DS_CHECK(sl_launch_check(n, lines, blocks, eps));
    const double h = 1.0 / (double)(n - 1);
    SlArgs a{in, nullptr, out, mean, n, lines, pitch, (0.5 * h) * h, eps, 1.0 / eps, hl_chunk(HL_XCHUNK_MAX)};
    DS_KLAUNCH(k_sl_pass_x<SlArgs>, dim3((unsigned)blocks), dim3(SL_BLOCK), 0, st, a);
    DS_HIP(hipGetLastError());
    return 0;
}

int launch_sl_mom_x(const double *in, double *out, double *mean, double *da, i64 n, i64 lines, i64 pitch, double eps,
                    hipStream_t st) {
    const i64 blocks = ((n + HL_XOUT - 1) / HL_XOUT) * ((lines + 63) / 64);
    DS_CHECK(sl_launch_check(n, lines, blocks, eps));
    const double h = 1.0 / (double)(n - 1);
    SlMomArgs a{{in, nullptr, out, mean, n, lines, pitch, (0.5 * h) * h, eps, 1.0 / eps, hl_chunk(HL_XCHUNK_MAX)}, nullptr, da, nullptr, h};
    DS_KLAUNCH(k_sl_pass_x<SlMomArgs>, dim3((unsigned)blocks), dim3(SL_BLOCK), 0, st, a);
    DS_HIP(hipGetLastError());
    return 0;
}

// ---------------- node kernels ----------------

// the workgroup's sums of v[0 .. NS) -> partials[row][block]: the tree of k_hl_reduce
template <int NS>
__device__ __forceinline__ void sl_block_sums(const double (&v)[NS], double (*s_red)[NS], double *partials) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double s = v[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) s_red[wv][i] = s;
    }
    __syncthreads();
    if (tid < NS) {
        double s = s_red[0][tid];
#pragma unroll
        for (int w = 1; w < SL_BLOCK / 64; ++w) s += s_red[w][tid];
        partials[(i64)tid * gridDim.x + blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(SL_BLOCK) k_sl_mass(const double *__restrict__ rho0, const double *__restrict__ rho1, i64 n,
                                                      double *__restrict__ partials, unsigned long long *counts) {
    __shared__ double s_red[SL_BLOCK / 64][SM_COUNT];
    __shared__ unsigned int s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const i64 i = (i64)blockIdx.x * SL_BLOCK + threadIdx.x;
    double v[SM_COUNT] = {0.0, 0.0};
    if (i < n) {
        const double r0 = rho0[i], r1 = rho1[i];
        v[SM_M0] = r0;
        v[SM_M1] = r1;
        if (r0 == 0.0) atomicAdd(&s_cnt[SC_ZERO0], 1u);
        if (r1 == 0.0) atomicAdd(&s_cnt[SC_ZERO1], 1u);
        const unsigned int bad = (isfinite(r0) && r0 >= 0.0 ? 0u : 1u) + (isfinite(r1) && r1 >= 0.0 ? 0u : 1u);
        if (bad) atomicAdd(&s_cnt[SC_BAD], bad);
    }
    sl_block_sums<SM_COUNT>(v, s_red, partials);        // (its barrier also orders the counters)
    if (threadIdx.x >= 64 && threadIdx.x < 67 && s_cnt[threadIdx.x - 64])
        atomicAdd(&counts[threadIdx.x - 64], (unsigned long long)s_cnt[threadIdx.x - 64]);
}

int launch_sl_mass(const double *rho0, const double *rho1, i64 n, double *partials, double *sums, unsigned long long *counts,
                   hipStream_t st) {
    const i64 blocks = hl_blocks(n);
    if (blocks < 1 || blocks > 0x7fffffffLL) { set_error("invalid argument: the upper bound serves layers of up to 2^39 nodes"); return DOTSOCP_EINVAL; }
    DS_KLAUNCH(k_sl_mass, dim3((unsigned)blocks), dim3(SL_BLOCK), 0, st, rho0, rho1, n, partials, counts);
    DS_HIP(hipGetLastError());
    return launch_report_rows(partials, blocks, SM_COUNT, sums, st);
}

__global__ void __launch_bounds__(SL_BLOCK) k_sl_init(SlInitArgs a) {
    __shared__ unsigned int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const i64 i = (i64)blockIdx.x * SL_BLOCK + threadIdx.x;
    if (i < a.n) {
        const double pa = a.rho0[i] / a.m0, pb = a.rho1[i] / a.m1;
        const double la = -(a.eps * log(pa)), lb = -(a.eps * log(pb));
        double f = a.mode == 0 ? 0.0 : (a.mode == 1 ? -a.src[i] : a.src[i]);
        if (!isfinite(f)) { f = 0.0; atomicAdd(&s_bad, 1u); }
        a.a[i] = pa;
        a.b[i] = pb;
        a.la[i] = la;
        a.lb[i] = lb;
        a.f[i] = f;
        a.in[i] = la - f;
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_bad) atomicAdd(&a.counts[SC_NONFINITE], (unsigned long long)s_bad);
}

int launch_sl_init(const SlInitArgs &a, hipStream_t st) {
    DS_KLAUNCH(k_sl_init, dim3((unsigned)hl_blocks(a.n)), dim3(SL_BLOCK), 0, st, a);
    DS_HIP(hipGetLastError());
    return 0;
}

__global__ void __launch_bounds__(SL_BLOCK) k_sl_minsub(const double *__restrict__ l, double *__restrict__ x,
                                                        const double *__restrict__ v, double *__restrict__ in, i64 n) {
    const i64 i = (i64)blockIdx.x * SL_BLOCK + threadIdx.x;
    if (i >= n) return;
    double xv = x[i];
    if (v) {
        const double vv = v[i];
        xv = vv < xv ? vv : xv;
        x[i] = xv;
    }
    in[i] = l[i] - xv;
}

int launch_sl_minsub(const double *l, double *x, const double *v, double *in, i64 n, hipStream_t st) {
    DS_KLAUNCH(k_sl_minsub, dim3((unsigned)hl_blocks(n)), dim3(SL_BLOCK), 0, st, l, x, v, in, n);
    DS_HIP(hipGetLastError());
    return 0;
}

__global__ void __launch_bounds__(SL_BLOCK) k_sl_defect(const double *__restrict__ a, const double *__restrict__ la,
                                                        double *__restrict__ f, const double *__restrict__ v,
                                                        double *__restrict__ in, i64 n, double ieps, double *__restrict__ partials) {
    __shared__ double s_red[SL_BLOCK / 64][1];
    const i64 i = (i64)blockIdx.x * SL_BLOCK + threadIdx.x;
    double t[1] = {0.0};
    if (i < n) {
        const double pa = a[i], fo = f[i], fn = v[i];
        if (pa > 0.0) t[0] = pa * fabs(exp((fo - fn) * ieps) - 1.0);
        f[i] = fn;
        in[i] = la[i] - fn;
    }
    sl_block_sums<1>(t, s_red, partials);
}

int launch_sl_defect(const double *a, const double *la, double *f, const double *v, double *in, i64 n, double ieps,
                     double *partials, double *sum, hipStream_t st) {
    const i64 blocks = hl_blocks(n);
    DS_KLAUNCH(k_sl_defect, dim3((unsigned)blocks), dim3(SL_BLOCK), 0, st, a, la, f, v, in, n, ieps, partials);
    DS_HIP(hipGetLastError());
    return launch_report_rows(partials, blocks, 1, sum, st);
}

__global__ void __launch_bounds__(SL_BLOCK) k_sl_final(SlFinalArgs a) {
    __shared__ double s_red[SL_BLOCK / 64][SS_COUNT];
    const i64 i = (i64)blockIdx.x * SL_BLOCK + threadIdx.x;
    double v[SS_COUNT];
#pragma unroll
    for (int k = 0; k < SS_COUNT; ++k) v[k] = 0.0;
    if (i < a.ny * a.nx) {
        const i64 x = i / a.ny, y = i - x * a.ny;
        const double pa = a.a[i], pb = a.b[i];
        const double r = pa > 0.0 ? pa * exp((a.f[i] - a.fh[i]) * a.ieps) : 0.0;
        const double k = pb > 0.0 ? pb * exp((a.g[i] - a.gt[i]) * a.ieps) : 0.0;
        const double er = fmax(pa - r, 0.0), ec = fmax(pb - k, 0.0);
        const double px = (double)x * a.hx, py = (double)y * a.hy, p2 = px * px + py * py;
        a.er[i] = er;
        a.ec[i] = ec;
        v[SS_KEPT] = k;
        v[SS_COST] = k * a.E[i];
        v[SS_R0] = er;
        v[SS_R1X] = er * px;
        v[SS_R1Y] = er * py;
        v[SS_R2] = er * p2;
        v[SS_C0] = ec;
        v[SS_C1X] = ec * px;
        v[SS_C1Y] = ec * py;
        v[SS_C2] = ec * p2;
    }
    sl_block_sums<SS_COUNT>(v, s_red, a.partials);
}

int launch_sl_final(const SlFinalArgs &a, double *sums, hipStream_t st) {
    const i64 blocks = hl_blocks(a.ny * a.nx);
    DS_KLAUNCH(k_sl_final, dim3((unsigned)blocks), dim3(SL_BLOCK), 0, st, a);
    DS_HIP(hipGetLastError());
    return launch_report_rows(a.partials, blocks, SS_COUNT, sums, st);
}

// ---------------- the map of the plan (dotsocp_plan_map) ----------------

__global__ void __launch_bounds__(SL_BLOCK) k_sl_map(SlMapArgs a) {
    __shared__ double s_red[SL_BLOCK / 64][SP_COUNT];
    __shared__ unsigned long long s_key;
    if (threadIdx.x == 0) s_key = 0;
    __syncthreads();
    const i64 i = (i64)blockIdx.x * SL_BLOCK + threadIdx.x;
    double v[SP_COUNT];
#pragma unroll
    for (int k = 0; k < SP_COUNT; ++k) v[k] = 0.0;
    double disp = 0.0;
    if (i < a.ny * a.nx) {
        const i64 x = i / a.ny, y = i - x * a.ny;
        const double pa = a.a[i];
        const double wk = pa > 0.0 ? pa * exp((a.f[i] - a.fh[i]) * a.ieps) : 0.0;      // r_i of k_sl_final
        const double wf = a.er[i] * a.kappa;
        const double row = wk + wf;
        double Dx = 0.0, Dy = 0.0, C = 0.0, spread = 0.0, d2 = 0.0;
        if (row != 0.0) {
            const double px = (double)x * a.hx, py = (double)y * a.hy, p2 = px * px + py * py;
            const double fdx = a.mx - px, fdy = a.my - py;
            const double fc = 0.5 * ((a.m2 - 2.0 * (px * a.mx + py * a.my)) + p2);
            const double kdx = a.kdx ? a.kdx[i] : 0.0;
            Dx = (wk * kdx + wf * fdx) / row;
            Dy = (wk * a.kdy[i] + wf * fdy) / row;
            C = (wk * a.kc[i] + wf * fc) / row;
            d2 = Dx * Dx + Dy * Dy;
            spread = 2.0 * C - d2;
            disp = sqrt(d2);
        }
        a.Dx[i] = Dx;
        a.Dy[i] = Dy;
        a.C[i] = C;
        a.row[i] = row;
        a.spread[i] = spread;
        v[SP_ROWS] = row;
        v[SP_MAP] = row * d2;
        v[SP_SPREAD] = row * spread;
        v[SP_COST] = row * C;
        v[SP_DISP] = row * disp;
    }
    // the largest displacement: the bit patterns of non-negative doubles order as unsigned integers (k_map_final)
    unsigned long long key = (unsigned long long)__double_as_longlong(disp);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_down(key, off, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0 && key) atomicMax(&s_key, key);
    sl_block_sums<SP_COUNT>(v, s_red, a.partials);      // (its barrier also orders s_key)
    if (threadIdx.x == 64 && s_key) atomicMax(a.disp_max, s_key);
}

int launch_sl_map(const SlMapArgs &a, double *sums, hipStream_t st) {
    const i64 blocks = hl_blocks(a.ny * a.nx);
    DS_KLAUNCH(k_sl_map, dim3((unsigned)blocks), dim3(SL_BLOCK), 0, st, a);
    DS_HIP(hipGetLastError());
    return launch_report_rows(a.partials, blocks, SP_COUNT, sums, st);
}

__device__ __forceinline__ double sl_clamp(double u) { return u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u); }     // adv_clamp of advect.hip

// the particle of node i at time tau: clamp(p + tau * D); flag[i] = 1 where a clamp moved a node that carries units (never cleared)
__global__ void __launch_bounds__(SL_BLOCK) k_sl_frame_pos(const double *__restrict__ Dx, const double *__restrict__ Dy,
                                                           const i64 *__restrict__ units, i64 ny, i64 nx, double hx, double hy,
                                                           double tau, double *__restrict__ X, double *__restrict__ Y,
                                                           unsigned int *__restrict__ flag) {
    const i64 i = (i64)blockIdx.x * SL_BLOCK + threadIdx.x;
    if (i >= ny * nx) return;
    const i64 x = i / ny, y = i - x * ny;
    const double ux = (double)x * hx + tau * Dx[i], uy = (double)y * hy + tau * Dy[i];
    const double cx = sl_clamp(ux), cy = sl_clamp(uy);
    X[i] = cx;
    Y[i] = cy;
    if ((cx != ux || cy != uy) && units[i] > 0) flag[i] = 1u;
}

int launch_sl_frame_pos(const double *Dx, const double *Dy, const i64 *units, i64 ny, i64 nx, double hx, double hy, double tau,
                        double *X, double *Y, unsigned int *flag, hipStream_t st) {
    DS_KLAUNCH(k_sl_frame_pos, dim3((unsigned)hl_blocks(ny * nx)), dim3(SL_BLOCK), 0, st, Dx, Dy, units, ny, nx, hx, hy, tau, X, Y, flag);
    DS_HIP(hipGetLastError());
    return 0;
}

// the counts of launch_deposit -> frame = (double)count * unit, in place
__global__ void __launch_bounds__(SL_BLOCK) k_sl_frame(double *__restrict__ frame, i64 n, double unit) {
    const i64 i = (i64)blockIdx.x * SL_BLOCK + threadIdx.x;
    if (i < n) frame[i] = (double)__double_as_longlong(frame[i]) * unit;
}

int launch_sl_frame(double *frame, i64 n, double unit, hipStream_t st) {
    DS_KLAUNCH(k_sl_frame, dim3((unsigned)hl_blocks(n)), dim3(SL_BLOCK), 0, st, frame, n, unit);
    DS_HIP(hipGetLastError());
    return 0;
}

}  // namespace dotsocp
