// The two buffer layouts of the particle march (dot-socp_amd/csrc/particle_block.h) against the formulas they replaced:
// regions in the documented order, disjoint, without gaps, each on an 8-byte boundary, the flags wide enough for n 32-bit
// words, and the totals.  Every region is painted into a byte buffer of the total size (run under ASan + UBSan).
#include <cstdio>
#include <vector>

#include "particle_block.h"

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

struct Region { const char *name; long long off, doubles; };

// the regions follow each other from 0 to `total` in the given order; painting them touches every byte exactly once
static void check_regions(const char *what, long long n, const std::vector<Region> &r, long long total) {
    std::vector<unsigned char> paint((size_t)total * sizeof(double), 0);
    long long at = 0;
    for (const Region &g : r) {
        CHECK(g.off == at, "%s n=%lld: %s starts at %lld, the regions before it end at %lld", what, n, g.name, g.off, at);
        CHECK((g.off * (long long)sizeof(double)) % 8 == 0, "%s n=%lld: %s is not on an 8-byte boundary", what, n, g.name);
        CHECK(g.off >= 0 && g.doubles >= 0 && g.off + g.doubles <= total, "%s n=%lld: %s leaves the buffer", what, n, g.name);
        if (g.off < 0 || g.doubles < 0 || g.off + g.doubles > total) return;
        for (long long b = g.off * 8; b < (g.off + g.doubles) * 8; ++b) ++paint[(size_t)b];
        at = g.off + g.doubles;
    }
    CHECK(at == total, "%s n=%lld: the regions end at %lld, total is %lld", what, n, at, total);
    long long bad = 0;
    for (unsigned char c : paint) bad += c != 1;
    CHECK(bad == 0, "%s n=%lld: %lld bytes are in no region or in two", what, n, bad);
}

int main() {
    const long long ns[] = {1, 2, 255, 256, 257};
    // wg: ADV_BLOCK of csrc/advect.hip, restated (map_blocks(n) lives in a HIP file): a change there is not seen here
    const long long bins = DOTSOCP_REPORT_BINS, wg = 256;
    CHECK(MC_OVER == bins && MC_COUNT == bins + 5 && MS_COUNT == 6, "the enums of the map report");
    for (long long n : ns)
        for (int push = 0; push < 2; ++push)
            for (int map = 0; map < 2; ++map) {
                const ParticleBlock L(n, push, map);
                const long long nflag = (n + 1) / 2, nunit = push ? n : 0, npath = map ? 2 * n : 0;
                check_regions("ParticleBlock", n,
                              {{"px", L.px, n}, {"py", L.py, n}, {"units", L.units, nunit}, {"sq", L.sq, npath / 2},
                               {"len", L.len, npath / 2}, {"flags", L.flags, nflag}, {"count", L.count, 1}}, L.total);
                CHECK((L.count - L.flags) * 8 >= n * 4 && (L.count - L.flags) * 8 < n * 4 + 8, "n=%lld: flags hold n 32-bit words", n);
                CHECK(L.total == 2 * n + nunit + npath + nflag + 1, "n=%lld push=%d map=%d: total %lld", n, push, map, L.total);
                // the offsets the march used to form by hand
                CHECK(L.py == n && L.units == 2 * n && L.sq == 2 * n + nunit && L.flags == 2 * n + nunit + npath &&
                          L.count == 2 * n + nunit + npath + nflag, "n=%lld push=%d map=%d: offsets", n, push, map);
                if (map) CHECK(L.len == 3 * n + nunit, "n=%lld push=%d: len at %lld", n, push, L.len);
                for (int mass = 0; mass < 2; ++mass)
                    for (int disp = 0; disp < 2; ++disp)
                        for (int action = 0; action < 2; ++action) {
                            const long long blocks = (n + wg - 1) / wg;
                            const MapFinalBlock M(n, mass, disp, action, blocks);
                            const long long m_mass = 2 * n, m_disp = m_mass + (mass ? n : 0), m_act = m_disp + (disp ? n : 0),
                                            m_edges = m_act + (action ? n : 0), m_sums = m_edges + bins + 1, m_counts = m_sums + MS_COUNT,
                                            m_part = m_counts + MC_COUNT;
                            check_regions("MapFinalBlock", n,
                                          {{"seeds", M.seeds, 2 * n}, {"mass", M.mass, mass ? n : 0}, {"disp", M.disp, disp ? n : 0},
                                           {"action", M.action, action ? n : 0}, {"edges", M.edges, bins + 1}, {"sums", M.sums, MS_COUNT},
                                           {"counts", M.counts, MC_COUNT}, {"partials", M.partials, MS_COUNT * blocks}}, M.total);
                            CHECK(M.mass == m_mass && M.disp == m_disp && M.action == m_act && M.edges == m_edges && M.sums == m_sums &&
                                      M.counts == m_counts && M.partials == m_part,
                                  "n=%lld mass=%d disp=%d action=%d: offsets", n, mass, disp, action);
                            CHECK(M.total == m_part + MS_COUNT * blocks, "n=%lld mass=%d disp=%d action=%d: total %lld", n, mass, disp,
                                  action, M.total);
                        }
            }
    printf("%d checks, %d failed\n", checked, failed);
    return failed ? 1 : 0;
}
