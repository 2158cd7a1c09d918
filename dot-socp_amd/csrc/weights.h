// Device-resident weight pyramid of the weighted multilevel driver (include/dotsocp.h: dotsocp_weights_*): model.weight
// of every level of one solve, filled once at the finest level (from a host array or from two 2-D arrays), restricted level
// by level on the device (socp/wdot2d/utils/downSample_q.m / downSample_barrier.m) and handed to each level's context by a
// device-to-device copy (Solver::upload_weight_from).  Kernels and host code: weights.hip.
#pragma once
#include <vector>

#include "solver.h"

namespace dotsocp {

// Nq of level `level` of a pyramid whose finest level (levels - 1) is ny x nx x nt; optionally that level's grid.
// -1: bad level, a grid too small, or one that cannot be halved down to level 0 (pure host arithmetic).
i64 weights_level_len(i64 ny, i64 nx, i64 nt, int levels, int level, i64 *lny = nullptr, i64 *lnx = nullptr,
                      i64 *lnt = nullptr);

struct Weights {
    int device = 0;
    int levels = 0;
    hipStream_t st = nullptr;
    struct Level {
        i64 ny = 0, nx = 0, nt = 0, Nq = 0;
        double *w = nullptr;        // Nq doubles, reference layout [q0; bx; by] (unpitched)
        bool filled = false;
    };
    std::vector<Level> lev;         // lev[levels - 1] is the finest
    double *partials = nullptr;     // partial sums of log10_mean [LOG10_BLOCKS + 1]
    ~Weights();
    int init(int device, i64 ny, i64 nx, i64 nt, int levels);
    int set(const double *weight);
    int set_space(const double *weightX, const double *weightY);
    int restrict_all(int log_mean);
    int log10_mean(int level, double *mean);
    int download(int level, double *host);
    // the level as a source of Solver::upload_weight_from: EINVAL for a bad level, ESTATE for one not filled yet
    int level_for_upload(int level, const Level **out) const;

  private:
    int check_level(int level, bool need_filled) const;
    int finest_done();
};

// one restriction step: fine level (ny, nx, nt) -> coarse level ((ny + 1) / 2, ...), both in the reference layout
int launch_weight_restrict(const double *fine, double *coarse, i64 ny, i64 nx, i64 nt, bool log_mean, hipStream_t st);
// w = [ones(ny nx (nt - 1)); weightX repeated over the nt nodes; weightY repeated over the nt nodes]
int launch_weight_space(double *w, const double *wX, const double *wY, i64 ny, i64 nx, i64 nt, hipStream_t st);
// sums[0] = sum of log10(w + 1e-10) in a fixed order; `partials`: WEIGHT_LOG10_BLOCKS + 1 doubles (the sum lands in the last)
constexpr int WEIGHT_LOG10_BLOCKS = 1024;
int launch_weight_log10_sum(const double *w, i64 n, double *partials, hipStream_t st);

}  // namespace dotsocp
