// Convolution-based DCT for the lengths that are neither powers of two nor prime-factor lengths (cdft.hip):
// Rader for 257, Bluestein for the other lengths up to 1024.
#pragma once
#include "common.h"

namespace dotsocp {

struct CdftPlan;
struct LineMap;

#define CDFT_MAX_N 1024

CdftPlan *cdft_plan_create(i64 n);      // n = 257: Rader; any other 48 <= n <= 1024: Bluestein; nullptr otherwise
void cdft_plan_destroy(CdftPlan *p);

// DCT-II (inverse = 0) / DCT-III of the lines of `map` (fft_lds.h); axis0: line L starts at L * map.outerStride, elements
// contiguous.  src == dst is allowed.
int cdft_launch(const CdftPlan *p, const double *src, double *dst, const LineMap &map, bool axis0, int inverse,
                hipStream_t st);

}  // namespace dotsocp
