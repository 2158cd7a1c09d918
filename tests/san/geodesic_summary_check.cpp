// Stand-alone driver of dot-socp_amd/csrc/geodesic_summary.h for tests/test_geodesic_host.py (built with g++ under
// AddressSanitizer + UBSan): reads cases from a binary file -- per case two int64 (nt, n_layer_nodes), then nt * 11 doubles
// (the layer sums, quantity q of layer t at [t + nt * q]) and nt doubles (rho_max) -- and prints one line per case: the
// fields of dotsocp_geodesic, integers in decimal, doubles as the 16 hex digits of their bit patterns.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "geodesic_summary.h"

static unsigned long long bits(double v) {
    unsigned long long b;
    memcpy(&b, &v, sizeof b);
    return b;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    long long head[2];
    int cases = 0;
    while (fread(head, sizeof head, 1, f) == 1) {
        const long long nt = head[0], N = head[1];
        if (nt < 2 || nt > 100000 || N < 1) { fprintf(stderr, "bad case header\n"); return 2; }
        std::vector<double> sums((size_t)(nt * DOTSOCP_GEO_SUMS)), rmax((size_t)nt), mean((size_t)(nt * DOTSOCP_GEO_SUMS));
        if (fread(sums.data(), sizeof(double), sums.size(), f) != sums.size() || fread(rmax.data(), sizeof(double), rmax.size(), f) != rmax.size()) {
            fprintf(stderr, "short case\n");
            return 2;
        }
        dotsocp_geodesic r;
        dotsocp::geodesic_summarize(nt, N, sums.data(), rmax.data(), &r, (cases & 1) ? mean.data() : nullptr);
        const double d[8] = {r.cost, r.energy_min, r.energy_max, r.speed_spread, r.com_defect, r.momentum_defect, r.entropy_defect,
                             r.peak_excess};
        printf("%lld %lld", (long long)r.nt, (long long)r.n_nodes);
        for (double v : d) printf(" %016llx", bits(v));
        printf(" %lld", (long long)r.nonfinite);
        if (cases & 1) printf(" %016llx", bits(mean[(size_t)(nt * DOTSOCP_GEO_SUMS - 1)]));      // the last mean: sq of the last layer
        printf("\n");
        ++cases;
    }
    fclose(f);
    printf("%d cases\n", cases);
    return 0;
}
