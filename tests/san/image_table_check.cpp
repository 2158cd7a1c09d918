// The tap tables of imresize (dot-socp_amd/csrc/image_table.h) for a list of lengths, built into buffers of exactly the
// documented size (n_out * imresize_max_taps entries) and run under ASan + UBSan: the mirror arithmetic is where such code
// overflows or indexes at -1.  Every index lies in [0, n_in), every row sums to 1 within 2 ulp, no row is empty, and the
// table holds no more columns than documented.  The row sum is taken in long double, so that the check
// adds no rounding of its own to a row of a thousand taps.
#include <cmath>
#include <cstdio>
#include <vector>

#include "image_table.h"

using namespace dotsocp;

static int failed = 0, checked = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        ++checked;                                        \
        if (!(cond)) {                                    \
            ++failed;                                     \
            printf("FAILED %s: ", #cond);                 \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
        }                                                 \
    } while (0)

static void check_table(long long n_in, long long n_out) {
    const int P = imresize_max_taps(n_in, n_out);
    std::vector<double> w((size_t)n_out * P);
    std::vector<int> idx((size_t)n_out * P);
    int taps = -1;
    imresize_table(n_in, n_out, w.data(), idx.data(), &taps);
    CHECK(taps >= 1 && taps <= P, "%lld -> %lld: %d taps, room for %d", n_in, n_out, taps, P);
    if (taps < 1 || taps > P) return;
    const double ulp = std::ldexp(1.0, -52);
    for (long long r = 0; r < n_out; ++r) {
        long double sum = 0.0L;
        int nonzero = 0;
        for (int k = 0; k < taps; ++k) {
            const int i = idx[(size_t)r * taps + k];
            const double v = w[(size_t)r * taps + k];
            CHECK(i >= 0 && i < n_in, "%lld -> %lld: row %lld tap %d has index %d", n_in, n_out, r, k, i);
            CHECK(std::isfinite(v), "%lld -> %lld: row %lld tap %d has weight %g", n_in, n_out, r, k, v);
            sum = sum + v;
            nonzero += v != 0.0;
        }
        CHECK(nonzero > 0, "%lld -> %lld: row %lld is empty", n_in, n_out, r);
        CHECK(std::fabs((double)(sum - 1.0L)) <= 2.0 * ulp, "%lld -> %lld: row %lld sums to 1 %+g", n_in, n_out, r, (double)(sum - 1.0L));
    }
}

int main() {
    const long long lens[][2] = {{5, 9}, {9, 5}, {1, 3}, {3, 1}, {1, 1}, {2, 1}, {1, 2}, {37, 9}, {29, 16}, {512, 128}, {512, 1024},
                                 {256, 257}, {257, 256}, {540, 256}, {530, 32}, {7, 7}, {2, 64}, {64, 2}, {1000, 3}, {3, 1000},
                                 {65536, 1}, {1, 4096}, {65536, 65535}, {4097, 2049}, {2049, 4097}};
    for (const auto &l : lens) check_table(l[0], l[1]);
    CHECK(!imresize_lengths_ok(0, 4) && !imresize_lengths_ok(4, 0) && !imresize_lengths_ok(65537, 4) && !imresize_lengths_ok(4, -1),
          "lengths outside 1 .. 65536 must be refused");
    printf("%d checked, %d failed\n", checked, failed);
    return failed ? 1 : 0;
}
