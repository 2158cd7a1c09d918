// The pipelined kernels of the power-of-two DCT family: a section of dct_pow2.hip, included there once after the steps
// and the in-LDS kernels it builds on (dct_post, idct_combine, the axis-0 staging, the fused t step), so that it is
// compiled in the same translation unit with the same flags.  Not a stand-alone header.
//
// What limits the in-LDS kernels is not a unit but the bytes in flight: while a workgroup computes, its tile sits in LDS
// and nothing of it travels, and the LDS holds two tiles only (the same kernels with the transform skipped run at the
// copy rate; the transform's time adds in full).  Here persistent workgroups walk their tiles through two LDS buffers,
// and a tile arrives by LDS-DMA (global_load_lds_dwordx4: no registers, so the loads of tile k+1 and k+2 are in flight
// during the transform and the stores of tile k).  The twiddle tables live in LDS too: an ordinary global load in the
// loop would make the compiler wait for everything in flight.  DOTSOCP_DCT_PIPE=0 switches these kernels off.
#pragma once

namespace dotsocp {

#define PIPE_THREADS 512
#define PIPE_IT ((1 << (PIPE_LG_CPLX - 1)) / PIPE_THREADS)   // (row, j) items per thread
#define PIPE_LG_CPLX 12   // complex elements per tile: 4096 = 8192 doubles = 64 KB of lines
#define PIPE_NS 8         // global store instructions per wave and tile
#define PIPE_ND 8         // LDS-DMA instructions per wave and tile (64 pieces of 1 KB over 8 waves)
// log2 of the line lengths the pipelined kernels are instantiated for
#define TS_LG_MIN 5
#define TS_LG_MAX 10
#define PIPE_LG_MIN 7
#define PIPE_LG_MAX 11

// A double from a wave-uniform global address through the scalar cache: no vector-memory operation, so nothing the
// counted waits of the pipelined kernels would have to account for (the compiler takes a vector load for such a read
// when it cannot prove that the kernel's stores leave the table alone, and then waits for everything in flight).
__device__ __forceinline__ double sload_f64(const double *p) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)p);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((uintptr_t)p >> 32));
    const double *sp = (const double *)(((uintptr_t)hi << 32) | (uintptr_t)lo);
    double v;
    asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(sp) : "memory");
    return v;
}

// ---------------------------------------------------------------------------------------------
// The skeleton the three kernels share: tables into LDS, two tiles requested, then per tile the kernel's own body and
// pipe_advance.  Each kernel brings its own dma(tile, buffer) and its own body.
// ---------------------------------------------------------------------------------------------
// Entries of the twiddle tables a pipelined kernel keeps in LDS for lines of 2^lg points: n / 2 FFT twiddles and n DCT
// weights -- for the 2048-point lines, whose two tile buffers leave 32 KB, the symmetric part only (TwQuarter, WwHalf).
// The kernels lay their LDS out with it and choose_* size the launch with it.
struct PipeTabCount { int tw, ww; };
__host__ __device__ constexpr PipeTabCount pipe_tab_count(int lg) {
    return lg > 10 ? PipeTabCount{(1 << lg) >> 2, ((1 << lg) >> 1) + 1} : PipeTabCount{(1 << lg) >> 1, 1 << lg};
}

template <int LG>
struct PipeTables {
    static constexpr bool BIG = LG > 10;
    typename std::conditional<BIG, TwQuarter<(1 << LG) / 4>, const double2 *>::type tw;
    typename std::conditional<BIG, WwHalf<(1 << LG) / 2>, const double2 *>::type ww;
};

// copies the tables to `tab` (pipe_tab_count(LG) entries, twiddles first) and returns the views the steps index
template <int LG, int T>
__device__ __forceinline__ PipeTables<LG> pipe_stage_tables(double2 *tab, const double2 *__restrict__ tw,
                                                            const double2 *__restrict__ ww, int tid) {
    constexpr PipeTabCount C = pipe_tab_count(LG);
    double2 *twS = tab, *wwS = tab + C.tw;
    for (int i = tid; i < C.tw; i += T) twS[i] = tw[i];
    for (int i = tid; i < C.ww; i += T) wwS[i] = ww[i];
    return PipeTables<LG>{{twS}, {wwS}};
}

// Requests the workgroup's first two tiles and waits for the first: it has landed when only the second one's DMA is
// outstanding (vector-memory operations of a wave complete in issue order).
template <class DMA>
__device__ __forceinline__ void pipe_prologue(int tile, int stride, int nTiles, DMA &dma) {
    if (tile < nTiles) dma(tile, 0);
    if (tile + stride < nTiles) dma(tile + stride, 1);
    if (tile + stride < nTiles) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(PIPE_ND) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
}

// End of a tile's body, right after its PIPE_NS stores per wave were issued from buffer b.  The next tile's DMA is older
// than these stores, so it has landed when only they are outstanding: the counted wait leaves them in flight.  One
// barrier then says both "every wave's pieces of the next tile are in LDS" and "buffer b is drained", and the DMA of
// tile + 2 strides may overwrite it.
template <class DMA>
__device__ __forceinline__ void pipe_advance(int tile, int stride, int nTiles, int b, DMA &dma) {
    if (tile + stride < nTiles) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(PIPE_NS) : "memory");
    lds_barrier();
    if (tile + 2 * stride < nTiles) dma(tile + 2 * stride, b);
}

// ---------------------------------------------------------------------------------------------
// Axis 0, n = 128 .. 2048.  ONE persistent workgroup of 512 threads per CU (two waves per SIMD, 256 registers each) walks
// tiles of 8192 doubles (whole lines, contiguous in memory).  Per tile:
//   raw lines -> paired rows in Makhoul / natural order, in place (all reads, barrier, all writes) | [inverse
//   pre-processing] | FFT | post-processing + stores | pipe_advance.
// LDS: 2 x 4 x (n + 1) x 16 B + 1.5 n x 16 B = 152 KB at n = 1024.
// ---------------------------------------------------------------------------------------------
__host__ __device__ constexpr int axis0_pipe_buf(int lg) { return ((1 << lg) + 1) << (PIPE_LG_CPLX - lg); }

template <bool INVERSE, int LG>
__global__ void __launch_bounds__(PIPE_THREADS) k_dct_axis0_pipe(const double *__restrict__ src, double *__restrict__ dst,
                                                                  int nTiles, i64 ls /* doubles between lines */,
                                                                  const double2 *__restrict__ tw,
                                                                  const double2 *__restrict__ ww) {
    extern __shared__ double2 lds[];
    constexpr int n = 1 << LG, lh = LG - 1;
    constexpr int LPT = (2 << PIPE_LG_CPLX) / n;      // lines per tile
    constexpr int PPL = n / 128;                      // 1-KB DMA pieces per line
    constexpr int RS = n + 1;                         // odd row stride: rows start on different banks
    constexpr int lrows = PIPE_LG_CPLX - LG;          // 2^lrows rows (pairs of lines) per tile
    constexpr int BUF = axis0_pipe_buf(LG);           // complex elements per buffer
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const PipeTables<LG> tab = pipe_stage_tables<LG, PIPE_THREADS>(lds + 2 * BUF, tw, ww, tid);
    const unsigned ldsBase = (unsigned)(uintptr_t)lds;
    // the lines of a tile land back to back in LDS (n doubles apart) whatever their distance in memory
    auto dma = [&](int tile, int b) {
        const char *g = (const char *)(src + (i64)tile * LPT * ls) + lane * 16;
        const unsigned l0 = ldsBase + (unsigned)b * (unsigned)(BUF * 16) + (unsigned)(wave * PIPE_ND) * 1024u;
#pragma unroll
        for (int i = 0; i < PIPE_ND; ++i) {
            const int piece = wave * PIPE_ND + i;
            glds16(g + (i64)(piece / PPL) * (ls * 8) + (piece % PPL) * 1024, l0 + (unsigned)i * 1024u);
        }
    };
    int tile = blockIdx.x;
    const int stride = gridDim.x;
    pipe_prologue(tile, stride, nTiles, dma);
    // items of the staging / store loops: (row, j < n / 2) = (b >> lh, b & (n / 2 - 1)) for b = tid + u * threads, four per thread
    auto item_row = [&](int u) { return (tid + u * PIPE_THREADS) >> lh; };
    auto item_j = [&](int u) { return (tid + u * PIPE_THREADS) & ((1 << lh) - 1); };
    for (int it = 0; tile < nTiles; tile += stride, ++it) {
        const int b = it & 1;
        double2 *buf = lds + b * BUF;
        // raw lines (n doubles apart, unpadded) -> rows of pairs: all reads, barrier, all writes (same buffer)
        {
            const double *raw = (const double *)buf;
            double2 A[PIPE_IT], B[PIPE_IT];
#pragma unroll
            for (int u = 0; u < PIPE_IT; ++u) {
                const int rr = item_row(u), j0 = item_j(u);
                A[u] = *(const double2 *)(raw + (2 * rr) * n + 2 * j0);
                B[u] = *(const double2 *)(raw + (2 * rr + 1) * n + 2 * j0);
            }
            lds_barrier();
#pragma unroll
            for (int u = 0; u < PIPE_IT; ++u) axis0_stage<INVERSE>(buf + item_row(u) * RS, item_j(u), n, A[u], B[u]);
        }
        lds_barrier();
        const PipeTeam<PIPE_THREADS> team{tid};
        if (INVERSE) idct_combine(RowsLayout{buf, RS, lrows}, LG, team, tab.ww);
        fft_tile<false, LG, lrows, PIPE_THREADS, RS>(buf, tid, tab.tw);
        double *out = dst + (i64)tile * LPT * ls;
#pragma unroll
        for (int u = 0; u < PIPE_IT; ++u) {
            const int rr = item_row(u), j0 = item_j(u);
            double2 Av, Bv;
            axis0_unstage<INVERSE>(buf + rr * RS, j0, n, LG, tab.ww, Av, Bv);
            *(double2 *)(out + (2 * rr) * ls + 2 * j0) = Av;
            *(double2 *)(out + (2 * rr + 1) * ls + 2 * j0) = Bv;
        }
        pipe_advance(tile, stride, nTiles, b, dma);
    }
}

// Strided axes, pipelined (forward / inverse): a tile = 2^lrows pairs of lines that are consecutive in memory x all n
// elements = 4096 complex values, every (pair, k) one 16-byte access.  The tile lives in LDS pair-interleaved and in the
// order the transform wants: slot (padi(p) << lrows) + r holds position p of pair r, i.e. line element k = 2 p resp.
// 2 (n - 1 - p) + 1 (Makhoul order, forward) or k = p (inverse).  An LDS-DMA piece fills 64 consecutive slots = 64 / NP
// positions of all NP pairs: each lane fetches its own (pair, k) element, a piece still reads 64 / NP whole segments of
// NP x 16 bytes, and the tile is ready for the first butterfly group when it has landed -- no staging pass.  At
// n = 1024 a tile is 64 bytes wide: the workgroups are ordered such that the two tiles sharing every 128-byte line run
// at the same time on the same XCD (one fetch into its L2).
template <int MODE /*0 fwd, 1 inv*/, int LG>
__global__ void __launch_bounds__(PIPE_THREADS) k_dct_strided_pipe(const double *__restrict__ src, double *__restrict__ dst,
                                                                    LineMap map, int nTiles, const double2 *__restrict__ tw,
                                                                    const double2 *__restrict__ ww) {
    extern __shared__ double2 lds[];
    constexpr int n = 1 << LG;
    constexpr int lrows = PIPE_LG_CPLX - LG;          // log2(pairs per tile)
    constexpr int NP = 1 << lrows;
    constexpr int BUF = 1 << PIPE_LG_CPLX;            // complex elements per buffer (no padding: the swizzle permutes)
    constexpr bool BIG = PipeTables<LG>::BIG;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const PipeTables<LG> tab = pipe_stage_tables<LG, PIPE_THREADS>(lds + 2 * BUF, tw, ww, tid);
    const unsigned ldsBase = (unsigned)(uintptr_t)lds;
    // element offset of a tile's first line (the 2 NP lines of a tile are consecutive in memory: nin % (2 NP) == 0)
    auto tile_base = [&](int tile) { return map.base((i64)tile << (lrows + 1)); };
    auto dma = [&](int tile, int b) {
        const double *g0 = src + tile_base(tile) + 2 * (lane & (NP - 1));
        const unsigned l0 = ldsBase + (unsigned)b * (unsigned)(BUF * 16);
#pragma unroll
        for (int i = 0; i < PIPE_ND; ++i) {
            const int c = wave * PIPE_ND + i;                         // piece: slots 64 c .. 64 c + 63
            const int p = padi(((c << 6) + lane) >> lrows);          // position held by this lane's slot
            const int k = (MODE == 1) ? p : ((p < (n >> 1)) ? 2 * p : 2 * (n - 1 - p) + 1);
            glds16(g0 + (i64)k * map.es, l0 + (unsigned)c * 1024u);
        }
    };
    // tile order: workgroup w runs on XCD w % 8; the tiles 2p and 2p + 1 (n = 2048, tiles 32 bytes wide: 4p .. 4p + 3) that
    // share every 128-byte line go to workgroups of one XCD at the same time
    const int w = blockIdx.x, stride = gridDim.x;     // gridDim.x is a multiple of 32
    int tile = BIG ? (((((w >> 5) << 3) + (w & 7)) << 2) | ((w >> 3) & 3))
                   : (((((w >> 4) << 3) + (w & 7)) << 1) | ((w >> 3) & 1));
    pipe_prologue(tile, stride, nTiles, dma);
    for (int it = 0; tile < nTiles; tile += stride, ++it) {
        const int b = it & 1;
        double2 *buf = lds + b * BUF;
        if (MODE == 1) idct_combine(TileLayout<lrows>{buf}, LG, PipeTeam<PIPE_THREADS>{tid}, tab.ww);
        fft_tile<false, LG, lrows, PIPE_THREADS>(buf, tid, tab.tw);
        {
            // item u of this thread: pair r0, k = k0 + u * (threads / NP)
            const int r0 = tid & (NP - 1), k0 = tid >> lrows;
            const double2 *rr = buf + r0;
            double *o = dst + tile_base(tile) + 2 * r0 + (i64)k0 * map.es;
            const i64 ostep = (i64)(PIPE_THREADS >> lrows) * map.es;
#pragma unroll
            for (int u = 0; u < 2 * PIPE_IT; ++u) {
                const int k = k0 + u * (PIPE_THREADS >> lrows);
                double2 v;
                if (MODE == 0) v = dct_post<lrows>(rr, k, n, LG, tab.ww);
                else v = rr[padi(bitrev(makhoul(k, n), LG)) << lrows];
                *(double2 *)o = v;
                o += ostep;
            }
        }
        pipe_advance(tile, stride, nTiles, b, dma);
    }
}

// Fused t-axis solve (k_dct_strided<2>: forward DCT, division by the spectral kernel, inverse DCT), pipelined.  A tile =
// 2^lrows pairs of consecutive columns (y, y + 1) x all n time nodes, pair-interleaved in LDS like the strided kernel's;
// the eigenvalue tables CY, CT sit in LDS beside the twiddles (no ordinary global load inside the loop; CX of the tile's
// one x is a scalar load, which the vector memory counter does not see).  This pass is bound by its own chain of LDS /
// VALU phases (two transforms, seven barriers per tile), not by HBM: tiles of 2048 values and workgroups of 256 threads, so that TWO workgroups fit a CU
// and fill each other's gaps (tiles of 1024 values with 256 threads, three workgroups per CU: 2.71 instead of 2.48 ms for the
// whole solve at 1024 x 1024 x 128; with 128 threads: 2.48 -- measured, not kept).  Needs ny % (lines per tile) == 0: a tile has one x.
#define TS_THREADS 256
#define TS_LG_CPLX 11
#define TS_IT ((1 << (TS_LG_CPLX - 1)) / TS_THREADS)

// The t solve's LDS: two tile buffers, the tables of pipe_stage_tables, then CT [n] and CY [ny] as doubles.  The kernel
// takes its pointers from it and choose_strided the size of the launch.
struct TsolveLds {
    size_t tab;         // in double2 from the start of the LDS
    size_t ct, cy;      // in doubles
    size_t bytes;
};
__host__ __device__ constexpr TsolveLds tsolve_lds(int lg, i64 ny) {
    const size_t n = (size_t)1 << lg;
    const size_t tab = (size_t)2 << TS_LG_CPLX;
    const size_t ct = 2 * (tab + (size_t)pipe_tab_count(lg).tw + (size_t)pipe_tab_count(lg).ww);
    return TsolveLds{tab, ct, ct + n, (ct + n + (size_t)ny) * sizeof(double)};
}

template <int LG>
__global__ void __launch_bounds__(TS_THREADS) k_dct_tsolve_pipe(const double *__restrict__ src, double *__restrict__ dst,
                                                                 LineMap map, int nTiles, SolveArgs sa,
                                                                 const double2 *__restrict__ tw,
                                                                 const double2 *__restrict__ ww) {
    extern __shared__ double2 lds[];
    constexpr int n = 1 << LG;
    constexpr int lrows = TS_LG_CPLX - LG;
    constexpr int NP = 1 << lrows;
    constexpr int BUF = 1 << TS_LG_CPLX;              // pair-interleaved tile (see k_dct_strided_pipe), no padding
    constexpr int TS_ND = (1 << (TS_LG_CPLX - 6)) / (TS_THREADS / 64);     // DMA pieces per wave and tile
    static_assert(TS_ND == PIPE_ND && (1 << TS_LG_CPLX) / TS_THREADS == PIPE_NS, "wait counts are shared with the other pipes");
    static_assert(!PipeTables<LG>::BIG, "the t solve keeps whole tables");
    constexpr TsolveLds L = tsolve_lds(LG, 0);
    double *ctS = (double *)lds + L.ct, *cyS = (double *)lds + L.cy;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const PipeTables<LG> tab = pipe_stage_tables<LG, TS_THREADS>(lds + L.tab, tw, ww, tid);
    for (int i = tid; i < n; i += TS_THREADS) ctS[i] = sa.ct[i];
    for (int i = tid; i < (int)sa.ny; i += TS_THREADS) cyS[i] = sa.cy[i];
    const unsigned ldsBase = (unsigned)(uintptr_t)lds;
    // slot (padi(p) << lrows) + r holds position p of pair r; the forward transform is decimation-in-time, so position p
    // is element makhoul^-1(bitrev(p)) of the line
    auto dma = [&](int tile, int b) {
        const double *g0 = src + map.base((i64)tile << (lrows + 1)) + 2 * (lane & (NP - 1));   // pitched rows: a tile lies in one row
        const unsigned l0 = ldsBase + (unsigned)b * (unsigned)(BUF * 16);
#pragma unroll
        for (int i = 0; i < TS_ND; ++i) {
            const int c = wave * TS_ND + i;
            const int q = bitrev(padi(((c << 6) + lane) >> lrows), LG);
            const int k = (q < (n >> 1)) ? 2 * q : 2 * (n - 1 - q) + 1;
            glds16(g0 + (i64)k * map.es, l0 + (unsigned)c * 1024u);
        }
    };
    int tile = blockIdx.x;
    const int stride = gridDim.x;
    pipe_prologue(tile, stride, nTiles, dma);
    for (int it = 0; tile < nTiles; tile += stride, ++it) {
        const int b = it & 1;
        double2 *buf = lds + b * BUF;
        const TileLayout<lrows> at{buf};
        fft_tile<true, LG, lrows, TS_THREADS>(buf, tid, tab.tw);
        // spectrum in natural order: the fused t step on the pairs (k, n - k), in place
        {
            const i64 G0 = sa.line0 + ((i64)tile << (lrows + 1));     // first column of the tile: (y0, x0)
            const int y0 = (int)(G0 % sa.ny), x0 = (int)(G0 / sa.ny);
            const double ex = sload_f64(sa.cx + x0);
#pragma unroll
            for (int u = 0; u < TS_IT; ++u) {
                int rr, i;
                at.split(tid + u * TS_THREADS, LG - 1, rr, i);
                const double ea = cyS[y0 + 2 * rr] + ex, eb = cyS[y0 + 2 * rr + 1] + ex;
                const int k = i + 1, m = n - k;                    // k = 1 .. n/2
                tsolve_pair(at(rr, k), at(rr, m), k, m, tab.ww, ctS, ea, eb, sa.kscale);
            }
            if (tid < NP) {                                        // k = 0: V[0] is its own partner
                const double ea = cyS[y0 + 2 * tid] + ex, eb = cyS[y0 + 2 * tid + 1] + ex;
                at(tid, 0) = tsolve_dc(at(tid, 0), tab.ww[0].x, ea, eb, ctS[0], sa.kscale);
            }
        }
        lds_barrier();
        fft_tile<false, LG, lrows, TS_THREADS>(buf, tid, tab.tw);
        {
            const int r0 = tid & (NP - 1), k0 = tid >> lrows;
            const double2 *rr = buf + r0;
            double *o = dst + map.base((i64)tile << (lrows + 1)) + 2 * r0 + (i64)k0 * map.es;
            const i64 ostep = (i64)(TS_THREADS >> lrows) * map.es;
#pragma unroll
            for (int u = 0; u < 2 * TS_IT; ++u) {
                const int k = k0 + u * (TS_THREADS >> lrows);
                *(double2 *)o = rr[padi(bitrev(makhoul(k, n), LG)) << lrows];
                o += ostep;
            }
        }
        pipe_advance(tile, stride, nTiles, b, dma);
    }
}

}  // namespace dotsocp
