// Layouts of the two device buffers a particle march works on (solver_particles.hip), in doubles from the buffer's start.
// Plain host arithmetic, no HIP: tests/test_particle_block_host.py compiles this header on its own.
#pragma once
#include "dotsocp.h"

namespace dotsocp {

// rows of the partial sums and slots of the 64-bit counters of k_map_final (kernels.h: launch_map_final)
enum { MS_MASS = 0, MS_DISP2, MS_LEN2, MS_ACTION, MS_DISP, MS_LEN, MS_COUNT };
enum { MC_HIST = 0, MC_OVER = DOTSOCP_REPORT_BINS, MC_STILL, MC_DISP_MAX, MC_LEN_MAX, MC_DETOUR_MAX, MC_COUNT };

// The block that travels from slab to slab:
//   [px (n) | py (n) | units (n x 64 bit, push) | sq (n, map) | len (n, map) | flags (n x 32 bit) | count (64 bit)]
// A region the march does not carry is empty: its offset is that of the next one.
struct ParticleBlock {
    long long px, py, units, sq, len, flags, count, total;
    ParticleBlock(long long n, bool push, bool map)
        : px(0), py(n), units(2 * n), sq(units + (push ? n : 0)), len(sq + (map ? n : 0)), flags(len + (map ? n : 0)),
          count(flags + (n + 1) / 2), total(count + 1) {}
};

// The buffer of k_map_final, on the slab that runs the last interval:
//   [seeds (x: n, y: n) | mass (n, if given) | disp (n, if asked for) | action (n, if asked for) | edges (bins + 1) |
//    sums (MS_COUNT) | counts (MC_COUNT x 64 bit) | partials (MS_COUNT x workgroups)]
struct MapFinalBlock {
    long long seeds, mass, disp, action, edges, sums, counts, partials, total;
    MapFinalBlock(long long n, bool with_mass, bool with_disp, bool with_action, long long workgroups)
        : seeds(0), mass(2 * n), disp(mass + (with_mass ? n : 0)), action(disp + (with_disp ? n : 0)),
          edges(action + (with_action ? n : 0)), sums(edges + DOTSOCP_REPORT_BINS + 1), counts(sums + MS_COUNT),
          partials(counts + MC_COUNT), total(partials + MS_COUNT * workgroups) {}
};

}  // namespace dotsocp
