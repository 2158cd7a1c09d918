// Convolution-based DCT for the lengths that are neither powers of two nor prime-factor lengths (cdft.hip):
// Rader for 257, Bluestein for the other lengths up to 1024.
#pragma once
#include "common.h"

namespace dotsocp {

struct CdftPlan;
struct LineMap;

// Which transform a DCT plan of length n uses (dotsocp_dct_algorithm of include/dotsocp.h).
enum { DCT_ALG_NONE = 0, DCT_ALG_FFT = 1, DCT_ALG_PFA = 2, DCT_ALG_RADER = 3, DCT_ALG_BLUESTEIN = 4, DCT_ALG_DENSE = 5 };

// Pure host arithmetic (no HIP call); honours DOTSOCP_PFA, DOTSOCP_CDFT and DOTSOCP_CDFT_MIN, each read once per process.
int dct_choose_algorithm(i64 n);

CdftPlan *cdft_plan_create(i64 n);      // n = 257: Rader; any other 48 <= n <= 1024: Bluestein; nullptr otherwise
void cdft_plan_destroy(CdftPlan *p);

// DCT-II (inverse = 0) / DCT-III of the lines of `map` (fft_lds.h); axis0: line L starts at L * map.outerStride, elements
// contiguous.  src == dst is allowed.
int cdft_launch(const CdftPlan *p, const double *src, double *dst, const LineMap &map, bool axis0, int inverse,
                hipStream_t st);

}  // namespace dotsocp
