// The dual lower bound on W2^2 (include/dotsocp.h: dotsocp_dual_bound; kernels: hopflax.hip).  All of it runs on the first
// slab's device, which owns phi(t = 0); phi(t = 1) is the last node layer of the last slab and travels there as one layer.
// Nothing of the context is written: the call has its own scratch, released before it returns.
#include <climits>
#include <cmath>
#include <cstring>

#include "solver.h"

namespace dotsocp {

int Solver::dual_bound(const double *rho0, const double *rho1, dotsocp_dual *res, double *H, double *B, int *arg_fwd, int *arg_bwd) {
    DS_ARG(rho0 != nullptr && rho1 != nullptr && res != nullptr, "dual_bound() needs rho0, rho1 and res (one of them is NULL)");
    DS_ARG(!remote(), "dual_bound() serves the slabs of one process; contexts with an RCCL communicator are not served");
    DS_ARG(!prob.weighted, "dual_bound(): the cost of a weighted context is not the Euclidean one, its bound is not provided");
    if (!finished) { set_error("dual_bound() needs finish()"); return DOTSOCP_ESTATE; }
    const bool dim1 = prob.dim == 1;
    DS_ARG(ny >= 2 && (dim1 || nx >= 2), "dual_bound() needs two nodes along every axis");
    DS_ARG(ny <= HL_MAX_LEN && nx <= HL_MAX_LEN && ny * nx <= INT_MAX, "dual_bound() serves axes of up to 2^20 nodes and layers of up to 2^31 - 1");
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    Slab &s0 = slabs.front(), &sl = slabs.back();
    const i64 plane = s0.g.plane, py = s0.g.py, blocks = hl_blocks(ny * nx);
    const i64 iplane = (plane + 1) / 2;                 // doubles that hold a plane of ints
    // host side of the copies: lives until the scratch below has waited for every stream
    double sums[HS_COUNT] = {0};
    unsigned long long counts[HC_COUNT] = {0};
    DeviceScratch scratch(*this);
    DS_CHECK(use(s0));
    // [phi0 | phi1 | T | H | B | rho0 | rho1 | ixf iyf ixb iyb arg_fwd arg_bwd (ints) | partials | sums | counters]
    double *buf = nullptr;
    // not poisoned as a whole (DOTSOCP_POISON=1): the six planes of ints are indices.  The passes write ix / iy / arg at
    // every y < ny of every column before k_hl_reduce reads them there, and nothing reads their pad entries; the counters
    // are set to zero below.  The regions of doubles are poisoned by name.
    DS_CHECK(scratch.alloc(&buf, 7 * plane + 6 * iplane + HS_COUNT * blocks + HS_COUNT + HC_COUNT, false));
    double *P0 = buf, *P1 = P0 + plane, *T = P1 + plane, *Hd = T + plane, *Bd = Hd + plane, *R0 = Bd + plane, *R1 = R0 + plane;
    int *ints[6];
    for (int k = 0; k < 6; ++k) ints[k] = (int *)(R1 + plane + iplane * k);
    double *partials = R1 + plane + 6 * iplane, *dsums = partials + HS_COUNT * blocks;
    unsigned long long *dcounts = (unsigned long long *)(dsums + HS_COUNT);
    DS_CHECK(poison_region(buf, sizeof(double) * (size_t)(7 * plane)));
    DS_CHECK(poison_region(partials, sizeof(double) * (size_t)(HS_COUNT * blocks + HS_COUNT)));
    hipStream_t st = s0.st;
    // (the pad entries of pitched rows stay as they come: the passes, the reduction and the row copies touch y < ny only)
    DS_HIP(ds_memset_async(dcounts, 0, sizeof(unsigned long long) * HC_COUNT, st));
    DS_CHECK(copy_rows(R0, const_cast<double *>(rho0), ny, py, nx, true, st));
    DS_CHECK(copy_rows(R1, const_cast<double *>(rho1), ny, py, nx, true, st));
    // phi in original units (recoverOrgVar, solver_dotsocp2d.m:368-386)
    DS_CHECK(launch_hl_layer(s0.phi, P0, plane, dScale, st));
    const double *last = sl.phi + plane * (sl.g.ntl - 1);
    if (&sl != &s0) {
        DS_CHECK(xcopy(sl, last, s0, T, plane));
        DS_CHECK(use(s0));
        last = T;
    }
    DS_CHECK(launch_hl_layer(last, P1, plane, dScale, st));
    for (int dir = 0; dir < 2; ++dir) {
        const bool fwd = dir == 0;
        const double *src = fwd ? P0 : P1;
        double *dst = fwd ? Hd : Bd;
        int *ix = ints[2 * dir], *iy = ints[2 * dir + 1];
        if (!dim1) {
            prof_begin(PH_HL_PASS_X);
            DS_CHECK(launch_hl_pass_x(fwd, src, T, ix, nx, ny, py, st));
            prof_end(PH_HL_PASS_X);
            src = T;
        }
        prof_begin(PH_HL_PASS_Y);
        DS_CHECK(launch_hl_pass_y(fwd, src, dst, iy, ny, nx, py, st));
        prof_end(PH_HL_PASS_Y);
    }
    HlReduceArgs ra{ny, nx, py, P0, P1, Hd, Bd, R0, R1, dim1 ? nullptr : ints[0], ints[1], dim1 ? nullptr : ints[2], ints[3],
                    ints[4], ints[5], dim1 ? 0.0 : 1.0 / (double)(nx - 1), 1.0 / (double)(ny - 1), partials, dcounts};
    prof_begin(PH_HL_REDUCE);
    DS_CHECK(launch_hl_reduce(ra, dsums, st));
    prof_end(PH_HL_REDUCE);
    DS_HIP(ds_memcpy_async(sums, dsums, sizeof sums, hipMemcpyDeviceToHost, st));
    DS_HIP(ds_memcpy_async(counts, dcounts, sizeof counts, hipMemcpyDeviceToHost, st));
    DS_CHECK(sync_all());
    DS_CHECK(prof_flush());
    const double m0 = sums[HS_M0], m1 = sums[HS_M1];
    DS_ARG(std::isfinite(m0) && m0 > 0.0 && std::isfinite(m1) && m1 > 0.0,
           "dual_bound(): the sum of rho0 or of rho1 is not a positive finite number");
    // the arrays the caller asked for, now that nothing can be refused any more
    DS_CHECK(use(s0));
    if (H) DS_CHECK(copy_rows(Hd, H, ny, py, nx, false, st));
    if (B) DS_CHECK(copy_rows(Bd, B, ny, py, nx, false, st));
    int *want[2] = {arg_fwd, arg_bwd};
    for (int k = 0; k < 2; ++k)
        if (want[k])
            DS_HIP(ds_memcpy2d_async(want[k], sizeof(int) * (size_t)ny, ints[4 + k], sizeof(int) * (size_t)py, sizeof(int) * (size_t)ny,
                                     (size_t)nx, hipMemcpyDeviceToHost, st));
    DS_CHECK(sync_all());
    DS_CHECK(canary_after());                   // the kernels wrote inside their buffers
    memset(res, 0, sizeof *res);
    const double a0 = sums[HS_P0R0] / m0, a1 = sums[HS_P1R1] / m1;
    res->n_nodes = ny * nx;
    res->nonfinite = (i64)counts[HC_NONFINITE];
    res->mass0 = m0;
    res->mass1 = m1;
    res->dual_raw = 2.0 * (a1 - a0);
    res->bound_fwd = 2.0 * (sums[HS_HR1] / m1 - a0);
    res->bound_bwd = 2.0 * (a1 - sums[HS_BR0] / m0);
    res->bound = res->bound_bwd > res->bound_fwd ? res->bound_bwd : res->bound_fwd;
    res->gap1_max = report_key_decode(counts[HC_G1_MAX], false, -INFINITY);
    res->gap1_min = report_key_decode(counts[HC_G1_MIN], true, INFINITY);
    res->gap1_mean = sums[HS_G1] / m1;
    res->gap0_max = report_key_decode(counts[HC_G0_MAX], false, -INFINITY);
    res->gap0_min = report_key_decode(counts[HC_G0_MIN], true, INFINITY);
    res->gap0_mean = sums[HS_G0] / m0;
    res->map_cost_bwd = sums[HS_MAP] / m0;
    return 0;
}

}  // namespace dotsocp
