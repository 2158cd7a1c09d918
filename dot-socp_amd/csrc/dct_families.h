// The transform families that live beside pfa.hip and cdft.hip: powers of two inside the LDS (dct_pow2.hip), powers of
// two beyond it (dct_long.hip, reached through the launchers of dct_pow2.hip) and the dense product (dct_dense.hip).  dct.hip picks one family per plan (dct_choose_algorithm) and dispatches on that choice.
#pragma once
#include "common.h"

namespace dotsocp {

struct LineMap;      // fft_lds.h
struct Pow2Plan;
struct DensePlan;
struct LongPlan;

#define DCT_THREADS 256

Pow2Plan *pow2_plan_create(i64 n);      // n = 2^k >= 2; nullptr on allocation failure
void pow2_plan_destroy(Pow2Plan *p);
// DCT-II (inverse = 0) / DCT-III of the lines of `map`; src == dst is allowed.
// axis 0: line L starts at L * map.outerStride, elements contiguous; strided: the x and t axes
int pow2_launch_axis0(const Pow2Plan *p, const double *src, double *dst, const LineMap &map, int inverse, hipStream_t st);
int pow2_launch_strided(const Pow2Plan *p, const double *src, double *dst, const LineMap &map, int inverse, hipStream_t st);
// DCT-II along t, division by kscale * lambda, DCT-III along t in one pass (arguments: launch_dct_t_solve of kernels.h)
int pow2_launch_tsolve(const Pow2Plan *p, const double *src, double *dst, i64 ny, i64 nplane, i64 line0, i64 nl,
                       double kscale, const double *cy, const double *cx, const double *ct, hipStream_t st, i64 pitch0);

// Which kernel those launchers take, from the shape alone (pure host arithmetic; ncu: the CU count of the device; the
// arrays are taken to be 16-byte aligned, as every allocation of the library is).  The launchers switch on the same
// choice functions (choose_axis0 / choose_strided), so the answer is what runs.
// pow2_pass_kind: DOTSOCP_PASS_POW2_* for a DCT-II / DCT-III pass over the lines of `map`
int pow2_pass_kind(i64 n, const LineMap &map, bool axis0, int ncu);
// does pow2_launch_tsolve with these arguments run k_dct_tsolve_pipe (else: k_dct_strided<2, .>)?
bool pow2_tsolve_pipelined(i64 n, i64 ny, i64 nplane, i64 line0, i64 nl, i64 pitch0, int ncu);

// Two-level transform for power-of-two lines that do not fit the LDS (dct_long.hip): 256 <= n <= DCT_LONG_MAX_N.
#define DCT_LONG_MAX_N ((i64)1 << 20)
i64 dct_long_min(int axis);             // smallest power of two that takes it along `axis` (DOTSOCP_DCT_LONG_MIN)
LongPlan *long_plan_create(i64 n);      // nullptr on allocation failure or an unsupported length
void long_plan_destroy(LongPlan *p);    // frees the scratch arrays of its streams too
// DCT-II / DCT-III of the lines of `map` (any axis, every LineMap field honoured); src == dst is allowed.  The plan's
// scratch array of stream `st` is allocated on the current device at the first launch.
int long_launch(LongPlan *p, const double *src, double *dst, const LineMap &map, bool axis0, int inverse, hipStream_t st);

DensePlan *dense_plan_create(i64 n);    // any n >= 2; nullptr on allocation failure
void dense_plan_destroy(DensePlan *p);
// axis0: line L starts at L * map.outerStride, elements contiguous.  Needs src != dst.
int dense_launch(const DensePlan *p, const double *src, double *dst, const LineMap &map, bool axis0, int inverse,
                 hipStream_t st);

}  // namespace dotsocp
