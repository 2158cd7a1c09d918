// Convolution-based DCT for the lengths that are neither powers of two nor prime-factor lengths (cdft.hip):
// Rader for 257, Bluestein for the other lengths up to 1024 inside the LDS; Bluestein with a two-level convolution through
// a scratch array in global memory (cdft_long.hip) for the lengths beyond, up to 2^19 - 1.
#pragma once
#include "common.h"

#include <complex>
#include <vector>

namespace dotsocp {

struct CdftPlan;
struct CdftLongPlan;
struct LineMap;

#define CDFT_MAX_N 1024

CdftPlan *cdft_plan_create(i64 n);      // n = 257: Rader; any other 48 <= n <= 1024: Bluestein; nullptr otherwise
void cdft_plan_destroy(CdftPlan *p);

// DCT-II (inverse = 0) / DCT-III of the lines of `map` (fft_lds.h); axis0: line L starts at L * map.outerStride, elements
// contiguous.  src == dst is allowed.
int cdft_launch(const CdftPlan *p, const double *src, double *dst, const LineMap &map, bool axis0, int inverse,
                hipStream_t st);

// in-place radix-2 FFT of length 2^lg in long double (the spectrum of the convolution kernel of both plans)
void cdft_fft_ld(std::vector<std::complex<long double>> &a, int lg);

// Two-level Bluestein (cdft_long.hip): the convolution of length M = 2^ceil(log2(2n-1)), 256 <= M <= 2^20, as a two-level
// FFT in three passes over a scratch array.  Lengths: not a power of two, CDFT_LONG_MIN_N <= n <= CDFT_LONG_MAX_N.
#define CDFT_LONG_MIN_N 129
#define CDFT_LONG_MAX_N (((i64)1 << 19) - 1)
// smallest length (neither a power of two nor a prime-factor length) that takes it: DOTSOCP_CDFT_LONG_MIN, never below
// CDFT_LONG_MIN_N; default: the first length the test suite does not pin to the dense product
i64 cdft_long_min();
CdftLongPlan *cdft_long_plan_create(i64 n);     // nullptr on allocation failure or an unsupported length
void cdft_long_plan_destroy(CdftLongPlan *p);   // frees the scratch arrays of its streams too
// DCT-II / DCT-III of the lines of `map` (any axis, every LineMap field honoured); src == dst is allowed.  The plan's
// scratch array of stream `st` is allocated on the current device at the first launch.
int cdft_long_launch(CdftLongPlan *p, const double *src, double *dst, const LineMap &map, bool axis0, int inverse,
                     hipStream_t st);

}  // namespace dotsocp
