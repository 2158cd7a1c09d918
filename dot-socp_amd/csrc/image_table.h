// The tap table of one imresize pass (include/dotsocp.h: dotsocp_imresize_table): MATLAB's `contributions` for the
// antialiased bicubic kernel, written as an explicit sequence of separately rounded operations so that the numpy twin
// (images.imresize_table) repeats it bit for bit.  Plain host arithmetic without HIP: image.hip includes it, and
// tests/san/image_table_check.cpp builds it with g++ under AddressSanitizer + UBSan.
#pragma once
#include <cmath>

#ifdef __clang__
#pragma clang fp contract(off)      // one ulp in a weight can move a uint8 result
#endif

namespace dotsocp {

typedef long long img_i64;

constexpr img_i64 IMG_MAX_LEN = 65536;      // longest axis the resize serves (the tap count of a length stays in an int)

// cubic convolution kernel, a = -0.5 (Keys)
inline double imresize_cubic(double x) {
    const double ax = std::fabs(x), ax2 = ax * ax, ax3 = ax2 * ax;
    if (ax <= 1.0) return ((1.5 * ax3) - (2.5 * ax2)) + 1.0;
    if (ax <= 2.0) return (((-0.5 * ax3) + (2.5 * ax2)) - (4.0 * ax)) + 2.0;
    return 0.0;
}

inline bool imresize_lengths_ok(img_i64 n_in, img_i64 n_out) {
    return n_in >= 1 && n_out >= 1 && n_in <= IMG_MAX_LEN && n_out <= IMG_MAX_LEN;
}

// P = ceil(kernel width) + 2: the columns of the table before the all-zero ones are dropped
inline int imresize_max_taps(img_i64 n_in, img_i64 n_out) {
    const double s = (double)n_out / (double)n_in;
    const double width = s < 1.0 ? 4.0 / s : 4.0;
    return (int)std::ceil(width) + 2;
}

// weights, indices: room for n_out * imresize_max_taps() entries; filled as [n_out][*taps], indices 0-based in [0, n_in).
inline void imresize_table(img_i64 n_in, img_i64 n_out, double *weights, int *indices, int *taps) {
    const double s = (double)n_out / (double)n_in;
    const bool shrink = s < 1.0;
    const double width = shrink ? 4.0 / s : 4.0;
    const double half = width / 2.0;
    const int P = (int)std::ceil(width) + 2;
    const double shift = 0.5 * (1.0 - 1.0 / s);
    const img_i64 period = 2 * n_in;
    unsigned char *used = new unsigned char[P]();
    for (img_i64 r = 0; r < n_out; ++r) {
        const double u = (double)(r + 1) / s + shift;
        const double left = std::floor(u - half);
        double *w = weights + r * P;
        int *ix = indices + r * P;
        // the row sum by Neumaier's compensated summation, k ascending: its error stays near one rounding whatever P is, so a
        // normalised row sums to 1 within 2 ulp (a plain running sum of 69 taps, 530 -> 32, already misses that)
        double sum = 0.0, comp = 0.0;
        for (int k = 0; k < P; ++k) {
            const double pos = left + (double)k;            // 1-based position, may lie outside [1, n_in]
            const double arg = u - pos;
            w[k] = shrink ? s * imresize_cubic(s * arg) : imresize_cubic(arg);
            const double t = sum + w[k];
            comp = comp + (std::fabs(sum) >= std::fabs(w[k]) ? (sum - t) + w[k] : (w[k] - t) + sum);
            sum = t;
            img_i64 m = ((img_i64)pos - 1) % period;        // mirror through [1..n_in, n_in..1]: a true modulo
            if (m < 0) m += period;
            ix[k] = (int)(m < n_in ? m : period - 1 - m);
        }
        sum = sum + comp;
        for (int k = 0; k < P; ++k) {
            w[k] = w[k] / sum;
            if (w[k] != 0.0) used[k] = 1;
        }
    }
    int T = 0;
    for (int k = 0; k < P; ++k) T += used[k];
    for (img_i64 r = 0; r < n_out; ++r) {                   // compact in place: the destination never overtakes the source
        int t = 0;
        for (int k = 0; k < P; ++k)
            if (used[k]) {
                weights[r * T + t] = weights[r * P + k];
                indices[r * T + t] = indices[r * P + k];
                ++t;
            }
    }
    delete[] used;
    *taps = T;
}

}  // namespace dotsocp
