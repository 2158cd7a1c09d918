// Driver steps on the device around the loop and the fields between host and device, on in-process time slabs too:
//   * the outputs recover_RhoE / recover_q (kernels: transfer.hip) and the solution report
//     (report.hip) and the pictures of the evolution (render.hip), with the staging of the density's ends that they share
//     with the velocity (solver_particles.hip);
//   * the multilevel transfer jump_nextLevel (+ recoverOrgVar of the coarse level, InitialScaling of the fine one; row 2);
//   * upload, upload_layers, download, the zero test of c at begin().
#include <algorithm>
#include <cmath>
#include <cstring>

#include "geodesic_summary.h"
#include "solver.h"

namespace dotsocp {

// Time slabs: a(.) of every slab's last cell, for the density at the right neighbour's first node (k_out_tail -> a0_prev)
int Solver::stage_left_tail() {
    if (!multi()) return 0;
    const double cD = cScale * D;                          // recoverOrgVar (solver_dotsocp2d.m:368-386)
    FOR_SLABS(s)
        if (!s.g.last) DS_CHECK(launch_out_tail(s.g, s.alpha, s.weight, sigma, cD, s.send_plane, s.st));
    return shift(+1, [](Slab &s) { return s.send_plane; }, [](Slab &s) { return s.a0_prev; }, slabs[0].g.plane);
}

// rho0 / rho1 -> the first / second layer of w1 (w1 holds at least two layers: nt >= 2 per slab)
int Solver::stage_rho_ends(Slab &s, const double *rho0, const double *rho1) {
    const Grid &g = slabs[0].g;
    if (s.g.first) DS_CHECK(copy_rows(s.w1, const_cast<double *>(rho0), ny, g.py, nx, true, s.st));
    if (s.g.last) DS_CHECK(copy_rows(s.w1 + g.plane, const_cast<double *>(rho1), ny, g.py, nx, true, s.st));
    return 0;
}

int Solver::canary_after() {
    if (!canary_enabled()) return 0;
    std::string what;
    const int bad = canary_check(&what);
    cur_dev = -1;
    if (bad) set_error("canary: %d device buffer(s) written out of bounds: %s", bad, what.c_str());
    return bad ? DOTSOCP_EHIP : 0;
}

// solver_dotsocp2d.m:262-281 on the device; call after finish().  Any output pointer may be NULL.  Time slabs: every
// slab produces its own layers (the density at its first node needs the left neighbour's last cell: one ny x nx layer
// to the right); in-process slabs fill the global host arrays, an RCCL rank its own slab of them.
int Solver::recover_outputs(const double *rho0, const double *rho1, double *rho, double *Ex, double *Ey, double *q0,
                            double *bx, double *by) {
    if (!finished) { set_error("recover_outputs() needs finish()"); return DOTSOCP_ESTATE; }
    DS_CHECK(need_beta_form("recover_outputs"));
    DS_CHECK(need_q("recover_outputs"));
    DS_ARG(rho == nullptr || (rho0 != nullptr && rho1 != nullptr), "rho needs rho0 and rho1");
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    const i64 plane = slabs[0].g.plane;                    // device layers (pitched rows, common.h)
    const i64 hplane = ny * nx;                            // host layers (reference layout)
    const i64 py = slabs[0].g.py;
    const double cD = cScale * D, dD = dScale / D;         // recoverOrgVar (solver_dotsocp2d.m:368-386)
    if (rho) DS_CHECK(stage_left_tail());
    double *outs[6] = {rho, Ex, Ey, q0, bx, by};
    for (int which = 0; which < 6; ++which) {
        if (!outs[which]) continue;
        {   // the host array of this output (this process's layers of it): make its pages exist before the copies
            i64 layers = 0;
            for (auto &s : slabs) layers += (which >= 3) ? s.g.ncl : s.g.ntl;
            host_first_touch(outs[which], sizeof(double) * (size_t)(hplane * layers));
        }
        FOR_SLABS(s) {
            const Grid &g = s.g;
            if (which == 0) DS_CHECK(stage_rho_ends(s, rho0, rho1));
            const i64 layers = (which >= 3) ? g.ncl : g.ntl;
            DS_CHECK(launch_outputs(g, s.q, s.alpha, s.weight, s.w1, s.w1 + plane, s.a0_prev, sigma, cD, dD, which, s.w0, s.st));
            double *h = outs[which] + (remote() ? 0 : hplane * g.t0);
            if (layers > 0) DS_CHECK(copy_rows(s.w0, h, ny, py, nx * layers, false, s.st));
        }
        DS_CHECK(sync_all());                               // w0 is reused by the next output
    }
    DS_CHECK(canary_after());                   // the kernels wrote inside their buffers
    return 0;
}

// The judgement the reference's demos pass on the downloaded outputs (check_massConservation, hist_negative_density,
// hist_violation_q_*, the transport cost), from the device-resident alpha and q: one launch_report per slab, staged like
// recover_outputs (rho0 / rho1 in w1, the left neighbour's last cell through k_out_tail / shift); what comes back is
// 3 sums per layer and RC_COUNT integers per slab, combined here -- layers in layer order, counters by integer addition.
int Solver::solution_report(const double *rho0, const double *rho1, dotsocp_report *rep, double *layer_mass, double *layer_neg) {
    DS_ARG(rho0 != nullptr && rho1 != nullptr && rep != nullptr, "solution_report() needs rho0, rho1 and rep (one of them is NULL)");
    DS_ARG(!remote(), "solution_report() serves the slabs of one process; contexts with an RCCL communicator are not reported");
    if (!finished) { set_error("solution_report() needs finish()"); return DOTSOCP_ESTATE; }
    DS_CHECK(need_beta_form("solution_report"));
    DS_CHECK(need_q("solution_report"));
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    const i64 plane = slabs[0].g.plane;
    const double cD = cScale * D, dD = dScale / D;         // recoverOrgVar (solver_dotsocp2d.m:368-386)
    DS_CHECK(stage_left_tail());
    // host side of the copies: lives until the sync_all() below
    double edges[DOTSOCP_REPORT_BINS + 1];
    report_edges_host(edges);
    std::vector<double> sums((size_t)(3 * nt));
    std::vector<unsigned long long> counts((size_t)RC_COUNT * slabs.size());
    size_t k = 0;
    FOR_SLABS(s) {
        const Grid &g = s.g;
        if (!s.rep_counts) {
            DS_CHECK(s.alloc(&s.rep_edges, DOTSOCP_REPORT_BINS + 1));
            DS_CHECK(s.alloc(&s.rep_part, 3 * g.ntl * report_tiles(g)));
            DS_CHECK(s.alloc(&s.rep_sums, 3 * g.ntl));
            DS_CHECK(s.alloc(&s.rep_counts, RC_COUNT));
        }
        DS_CHECK(stage_rho_ends(s, rho0, rho1));
        DS_HIP(ds_memcpy_async(s.rep_edges, edges, sizeof edges, hipMemcpyHostToDevice, s.st));
        DS_HIP(ds_memset_async(s.rep_counts, 0, sizeof(unsigned long long) * RC_COUNT, s.st));
        DS_CHECK(launch_report(g, s.q, s.alpha, s.weight, s.w1, s.w1 + plane, s.a0_prev, sigma, cD, dD, prob.dim == 1, s.rep_edges,
                               s.rep_part, s.rep_sums, s.rep_counts, s.st));
        DS_HIP(ds_memcpy_async(sums.data() + 3 * g.t0, s.rep_sums, sizeof(double) * 3 * g.ntl, hipMemcpyDeviceToHost, s.st));
        DS_HIP(ds_memcpy_async(counts.data() + RC_COUNT * k++, s.rep_counts, sizeof(unsigned long long) * RC_COUNT,
                               hipMemcpyDeviceToHost, s.st));
    }
    DS_CHECK(sync_all());
    DS_CHECK(canary_after());                   // the report's kernels wrote inside their buffers
    memset(rep, 0, sizeof *rep);
    const i64 hplane = ny * nx;
    rep->n_nodes = hplane * nt;
    rep->n_cells = hplane * (nt - 1);
    // max that keeps a NaN once it has met one (a layer with a NaN in it must not pass for a conserved one)
    auto worst = [](double m, double d) { return (d > m || d != d) ? d : m; };
    double cost = 0.0;
    for (i64 t = 0; t < nt; ++t) {
        const double mass = sums[3 * t] / (double)hplane, neg = sums[3 * t + 1] / (double)hplane;
        if (layer_mass) layer_mass[t] = mass;
        if (layer_neg) layer_neg[t] = neg;
        rep->mass_err = worst(rep->mass_err, fabs(mass - 1.0));
        rep->neg_err = worst(rep->neg_err, fabs(neg));
        cost += sums[3 * t + 2];
    }
    rep->cost = cost / (double)rep->n_nodes;
    unsigned long long kmin = 0, kmax = 0;
    for (size_t j = 0; j < slabs.size(); ++j) {
        const unsigned long long *c = counts.data() + RC_COUNT * j;
        for (int b = 0; b < DOTSOCP_REPORT_BINS; ++b) {
            rep->rho_hist[b] += (i64)c[RC_RHO_HIST + b];
            rep->fq_hist[b] += (i64)c[RC_FQ_HIST + b];
        }
        rep->rho_neg += (i64)c[RC_RHO_NEG];
        rep->fq_pos += (i64)c[RC_FQ_POS];
        rep->nonfinite += (i64)c[RC_NONFINITE];
        kmin = std::max(kmin, c[RC_RHO_MIN]);
        kmax = std::max(kmax, c[RC_FQ_MAX]);
    }
    rep->rho_min = report_key_decode(kmin, true, INFINITY);
    rep->fq_max = report_key_decode(kmax, false, -INFINITY);
    return 0;
}

// What separates a geodesic from a curve that joins rho0 to rho1, per time node (include/dotsocp.h:
// dotsocp_geodesic_profile): one launch_geodesic per slab over the device-resident alpha, staged like solution_report;
// DOTSOCP_GEO_SUMS sums, one maximum and one count per layer come back, are put in layer order and summarised on the host
// (geodesic_summary.h).  Every output is written behind the last step that can fail.
int Solver::geodesic_profile(const double *rho0, const double *rho1, dotsocp_geodesic *res, double *sums, double *rho_max, i64 *n_support) {
    DS_ARG(rho0 != nullptr && rho1 != nullptr && res != nullptr, "geodesic_profile() needs rho0, rho1 and res (one of them is NULL)");
    DS_ARG(!remote(), "geodesic_profile() serves the slabs of one process; contexts with an RCCL communicator are not profiled");
    if (!finished) { set_error("geodesic_profile() needs finish()"); return DOTSOCP_ESTATE; }
    DS_CHECK(need_beta_form("geodesic_profile"));
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    const i64 plane = slabs[0].g.plane;
    const double cD = cScale * D;                          // recoverOrgVar (solver_dotsocp2d.m:368-386)
    DS_CHECK(stage_left_tail());
    // host side of the copies: lives until the sync_all() below; per layer [sums | max] and the count
    const int R = DOTSOCP_GEO_SUMS;
    std::vector<double> rows((size_t)((R + 1) * nt));
    std::vector<unsigned long long> counts((size_t)nt);
    double *h_max = rows.data() + R * nt;
    FOR_SLABS(s) {
        const Grid &g = s.g;
        if (!s.geo_buf) {
            DS_CHECK(s.alloc(&s.geo_buf, geodesic_doubles(g)));
            DS_CHECK(s.alloc(&s.geo_cnt, geodesic_counts(g)));
        }
        DS_CHECK(stage_rho_ends(s, rho0, rho1));
        DS_CHECK(launch_geodesic(g, s.alpha, s.weight, s.w1, s.w1 + plane, s.a0_prev, sigma, cD, prob.dim == 1, s.geo_buf, s.geo_cnt, s.st));
        const i64 tiles = report_tiles(g);
        const double *d_sums = s.geo_buf + (R + 1) * g.ntl * tiles;
        DS_HIP(ds_memcpy_async(rows.data() + R * g.t0, d_sums, sizeof(double) * R * g.ntl, hipMemcpyDeviceToHost, s.st));
        DS_HIP(ds_memcpy_async(h_max + g.t0, d_sums + R * g.ntl, sizeof(double) * g.ntl, hipMemcpyDeviceToHost, s.st));
        DS_HIP(ds_memcpy_async(counts.data() + g.t0, s.geo_cnt + g.ntl * tiles, sizeof(unsigned long long) * g.ntl, hipMemcpyDeviceToHost,
                               s.st));
    }
    DS_CHECK(sync_all());
    DS_CHECK(canary_after());                   // the kernels wrote inside their buffers
    std::vector<double> by_quantity((size_t)(R * nt));     // the public layout: quantity q of layer t at [t + nt * q]
    for (i64 t = 0; t < nt; ++t)
        for (int q = 0; q < R; ++q) by_quantity[(size_t)(t + nt * q)] = rows[(size_t)(R * t + q)];
    geodesic_summarize(nt, ny * nx, by_quantity.data(), h_max, res);
    if (sums) memcpy(sums, by_quantity.data(), sizeof(double) * by_quantity.size());
    if (rho_max) memcpy(rho_max, h_max, sizeof(double) * (size_t)nt);
    if (n_support)
        for (i64 t = 0; t < nt; ++t) n_support[t] = (i64)counts[(size_t)t];
    return 0;
}

// The looking half of the reference's demos (show_evolution_2d, show_movement_2d, export_evolution_2d) from the
// device-resident alpha, staged like solution_report.  Two rounds: launch_rho_range per slab, combined here (the scale must
// be known, and judged, before a byte is written); then one launch_render (and launch_movement) per requested frame on the
// slab that owns its node, into that slab's scratch, and from there to the frame's place in the caller's arrays.
int Solver::render_evolution(const double *rho0, const double *rho1, const dotsocp_render_opts *o, const i64 *frame_nodes,
                             const double *levels, const unsigned char *lut, const unsigned char *barrier, unsigned char *image,
                             double *mvX, double *mvY, dotsocp_render_info *info) {
    DS_ARG(rho0 != nullptr && rho1 != nullptr && o != nullptr && frame_nodes != nullptr && image != nullptr,
           "render_evolution() needs rho0, rho1, opts, frame_nodes and image (one of them is NULL)");
    DS_ARG(!remote(), "render_evolution() serves the slabs of one process; contexts with an RCCL communicator are not rendered");
    DS_ARG(o->nf >= 1, "render_evolution() needs nf >= 1 frame nodes");
    for (i64 f = 0; f < o->nf; ++f)
        DS_ARG(frame_nodes[f] >= 0 && frame_nodes[f] < nt, "render_evolution(): a frame node lies outside [0, nt)");
    DS_ARG(o->mode == DOTSOCP_RENDER_LINEAR || o->mode == DOTSOCP_RENDER_INVERTED || o->mode == DOTSOCP_RENDER_LEVELS,
           "render_evolution(): unknown mode");
    const bool lev = o->mode == DOTSOCP_RENDER_LEVELS;
    if (lev) {
        DS_ARG(o->nlevels >= 1 && o->nlevels <= 254, "render_evolution() takes 1 to 254 levels");
        DS_ARG(levels != nullptr, "render_evolution() needs the levels in LEVELS mode");
        for (int j = 0; j < o->nlevels; ++j)
            DS_ARG(levels[j] == levels[j] && (j == 0 || levels[j] > levels[j - 1]), "render_evolution(): the levels must be strictly ascending");
    }
    DS_ARG(o->channels == 1 || o->channels == 3, "render_evolution() writes 1 or 3 channels");
    DS_ARG(o->channels == 1 || lut != nullptr, "render_evolution() needs a 256 x 3 table for 3 channels");
    DS_ARG(o->barrier_index >= 0 && o->barrier_index <= 255, "render_evolution(): barrier_index outside 0 .. 255");
    DS_ARG(o->skip_y >= 0 && o->skip_x >= 0, "render_evolution(): a skip is negative");
    DS_ARG((o->skip_y == 0) == (o->skip_x == 0), "render_evolution(): arrows need both skips >= 1 (exactly one is zero)");
    const bool arrows = o->skip_y >= 1;
    const bool dim1 = prob.dim == 1;
    DS_ARG(!arrows || (mvY != nullptr && (dim1 || mvX != nullptr)), "render_evolution(): arrows are asked for without their arrays");
    if (!finished) { set_error("render_evolution() needs finish()"); return DOTSOCP_ESTATE; }
    DS_CHECK(need_beta_form("render_evolution"));
    DS_CHECK(need_q("render_evolution"));
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    const i64 plane = slabs[0].g.plane, hplane = ny * nx;
    const double cD = cScale * D;                          // recoverOrgVar (solver_dotsocp2d.m:368-386)
    const int ch = o->channels;
    const i64 my = arrows ? (ny + o->skip_y - 1) / o->skip_y : 0, mx = arrows ? (nx + o->skip_x - 1) / o->skip_x : 0;
    const size_t img_bytes = (size_t)hplane * ch, mv_bytes = sizeof(double) * (size_t)(my * mx);
    auto owner = [&](i64 node) -> size_t {
        for (size_t k = 0; k < slabs.size(); ++k)
            if (node >= slabs[k].g.t0 && node < slabs[k].g.t0 + slabs[k].g.ntl) return k;
        return 0;
    };
    // host side of the copies: lives until the scratch below has waited for every stream
    std::vector<unsigned long long> counts((size_t)RR_COUNT * slabs.size());
    DeviceScratch scratch(*this);
    // per slab, one buffer: [counters | levels | barrier | lut | pictures of its frames | arrows of its frames], in doubles
    auto dbl = [](size_t bytes) { return (i64)((bytes + 7) / 8); };
    const i64 off_lev = RR_COUNT, off_bar = off_lev + RND_LEVELS, off_lut = off_bar + dbl((size_t)hplane);
    const i64 off_img = off_lut + dbl(768);
    std::vector<i64> mine(slabs.size(), 0);      // frames of the request per owning slab
    for (i64 f = 0; f < o->nf; ++f) ++mine[owner(frame_nodes[f])];
    DS_CHECK(stage_left_tail());
    size_t k = 0;
    FOR_SLABS(s) {
        double *buf = nullptr;
        const i64 nimg = mine[k] * dbl(img_bytes);
        // (DOTSOCP_POISON=1: the counters in front are integers, set to zero below; everything behind them is poisoned --
        // levels and arrows are doubles, mask, table and pictures are bytes that are read as values, never as indices)
        DS_CHECK(scratch.alloc(&buf, off_img + nimg + mine[k] * (dim1 ? 1 : 2) * my * mx, false));
        DS_CHECK(poison_region(buf + off_lev, sizeof(double) * (size_t)(off_img - off_lev + nimg + mine[k] * (dim1 ? 1 : 2) * my * mx)));
        DS_CHECK(stage_rho_ends(s, rho0, rho1));
        DS_HIP(ds_memset_async(buf, 0, sizeof(unsigned long long) * RR_COUNT, s.st));
        if (lev) DS_HIP(ds_memcpy_async(buf + off_lev, levels, sizeof(double) * (size_t)o->nlevels, hipMemcpyHostToDevice, s.st));
        if (barrier) DS_HIP(ds_memcpy_async(buf + off_bar, barrier, (size_t)hplane, hipMemcpyHostToDevice, s.st));
        if (ch == 3) DS_HIP(ds_memcpy_async(buf + off_lut, lut, 768, hipMemcpyHostToDevice, s.st));
        DS_CHECK(launch_rho_range(s.g, s.alpha, s.weight, s.w1, s.w1 + plane, s.a0_prev, sigma, cD,
                                  barrier ? (const unsigned char *)(buf + off_bar) : nullptr, (unsigned long long *)buf, s.st));
        DS_HIP(ds_memcpy_async(counts.data() + RR_COUNT * k++, buf, sizeof(unsigned long long) * RR_COUNT, hipMemcpyDeviceToHost, s.st));
    }
    DS_CHECK(sync_all());
    dotsocp_render_info res{};
    unsigned long long kmax = 0, kmin = 0;
    for (size_t j = 0; j < slabs.size(); ++j) {
        const unsigned long long *c = counts.data() + RR_COUNT * j;
        kmax = std::max(kmax, c[RR_MAX]);
        kmin = std::max(kmin, c[RR_MIN]);
        res.nonfinite += (i64)c[RR_NONFINITE];
        res.masked += (i64)c[RR_MASKED];
    }
    res.vmax = o->vmax > 0.0 ? o->vmax : report_key_decode(kmax, false, -INFINITY);
    res.rho_min = report_key_decode(kmin, true, INFINITY);
    res.my = my;
    res.mx = mx;
    DS_ARG(res.vmax > 0.0 && std::isfinite(res.vmax), "render_evolution(): the scale (the largest finite density, or opts.vmax) is not a positive finite number");
    const double thr = res.vmax * o->mask_frac;
    std::vector<i64> used(slabs.size(), 0);      // frames a slab has rendered so far: the slot of the next one
    for (i64 f = 0; f < o->nf; ++f) {
        const size_t j = owner(frame_nodes[f]);
        Slab &s = slabs[j];
        DS_CHECK(use(s));
        double *buf = scratch.bufs[j];
        const i64 slot = used[j]++;
        unsigned char *img = (unsigned char *)(buf + off_img + slot * dbl(img_bytes));
        DS_CHECK(launch_render(s.g, s.alpha, s.weight, s.w1, s.w1 + plane, s.a0_prev, sigma, cD, frame_nodes[f] - s.g.t0, o->mode, ch,
                               barrier ? (const unsigned char *)(buf + off_bar) : nullptr, buf + off_lev, o->nlevels,
                               (const unsigned char *)(buf + off_lut), o->barrier_index, res.vmax, img, s.st));
        DS_HIP(ds_memcpy_async(image + img_bytes * (size_t)f, img, img_bytes, hipMemcpyDeviceToHost, s.st));
        if (!arrows) continue;
        double *mv = buf + off_img + mine[j] * dbl(img_bytes) + slot * (dim1 ? 1 : 2) * my * mx;      // behind the slab's pictures
        double *dX = dim1 ? nullptr : mv, *dY = dim1 ? mv : mv + my * mx;
        DS_CHECK(launch_movement(s.g, s.alpha, s.weight, s.w1, s.w1 + plane, s.a0_prev, sigma, cD, frame_nodes[f] - s.g.t0, o->skip_y,
                                 o->skip_x, my, mx, thr, dX, dY, s.st));
        if (dX) DS_HIP(ds_memcpy_async(mvX + my * mx * f, dX, mv_bytes, hipMemcpyDeviceToHost, s.st));
        DS_HIP(ds_memcpy_async(mvY + my * mx * f, dY, mv_bytes, hipMemcpyDeviceToHost, s.st));
    }
    DS_CHECK(sync_all());
    DS_CHECK(canary_after());                   // the kernels wrote inside their buffers
    if (info) *info = res;
    return 0;
}

// jump_nextLevel.m:5-16: this = fine level (created, c / weight uploaded, begin() not yet called),
// `coarse` = the finished coarse level.  Both may be cut into in-process time slabs (any numbers of slabs, any
// placement on devices): a fine slab interpolates from the coarse layers it needs -- nodes floor(t/2) and, for odd
// t, floor(t/2) + 1; cells floor(t/2) -- which are first gathered from the coarse slabs that own them into the fine
// slab's work arrays (peer copies between devices); F*B*(-betaR) and grad(phiR) then need one layer from the
// neighbouring fine slab each, as in the loop.  One slab per process (RCCL): not available, transfer through the host.
int Solver::jump_from(Solver &coarse) {
    if (begun) { set_error("jump_next_level() must precede begin() of the fine level"); return DOTSOCP_ESTATE; }
    if (!coarse.finished) { set_error("jump_next_level() needs finish() of the coarse level"); return DOTSOCP_ESTATE; }
    DS_ARG(!remote() && !coarse.remote(), "multilevel transfer between one-slab-per-process contexts goes through the host");
    DS_ARG(prob.dim == coarse.prob.dim && prob.weighted == coarse.prob.weighted, "level kinds differ");
    DS_ARG(ny == 2 * (coarse.ny - 1) + 1 && nt == 2 * (coarse.nt - 1) + 1 &&
               (nx == 2 * (coarse.nx - 1) + 1 || (nx == 1 && coarse.nx == 1)),
           "fine grid must be 2 (n - 1) + 1 of the coarse grid in every dimension");
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    DS_CHECK(ensure_alloc());
    // everything of the coarse level has to be complete before this level's streams read it
    coarse.cur_dev = -1;
    DS_CHECK(coarse.sync_all());
    cur_dev = -1;
    cScale = prob.cScale; dScale = prob.dScale; D = prob.D; E = prob.E;
    update_coef();
    const i64 planec = coarse.slabs[0].g.plane;           // coarse layers as they are stored (pitched rows, common.h)
    // dst (on fine slab f) <- src (on coarse slab c); the coarse level is idle, so ordering on f's stream suffices
    auto pull = [&](Slab &f, double *dst, const Slab &c, const double *src, i64 count) -> int {
        if (count <= 0) return 0;
        const size_t bytes = sizeof(double) * (size_t)count;
        if (f.dev == c.dev) DS_HIP(ds_memcpy_async(dst, src, bytes, hipMemcpyDeviceToDevice, f.st));
        else DS_HIP(ds_memcpy_peer_async(dst, f.dev, src, c.dev, bytes, f.st));
        return 0;
    };
    const bool direct = !multi() && !coarse.multi() && slabs[0].dev == coarse.slabs[0].dev;
    FOR_SLABS(f) {
        const Grid &gf = f.g;
        const Grid &gc0 = coarse.slabs[0].g;                  // ny, nx of the coarse grid
        if (direct) {
            Slab &c = coarse.slabs[0];
            // phi: dScale_c * phi_c (recoverOrgVar) -> interpolate -> (1/dScale_f) * (InitialScaling)
            DS_CHECK(launch_prolong_phi(gf, c.g, c.phi, f.phi, coarse.dScale, 1.0 / dScale, f.st));
            // beta: (cScale_c E_c) * (sigma_c * beta_c) -> interpolate -> (1/cScale_f/E_f) * ; the unscaled -betaR goes to z
            DS_CHECK(launch_prolong_beta(gf, c.g, c.beta, f.beta, f.z, coarse.sigma, coarse.cScale * coarse.E,
                                         1.0 / cScale / E, f.st));
            continue;
        }
        // coarse node layers [nA, nB] -> w0 ; coarse cell layers [cA, cB] of all ten columns -> beta2 (fused buffers) or w1
        const i64 tlast = gf.t0 + gf.ntl - 1;
        const i64 nA = gf.t0 >> 1, nB = (tlast >> 1) + (tlast & 1);
        for (auto &c : coarse.slabs) {
            const i64 a = std::max<i64>(nA, c.g.t0), b = std::min<i64>(nB, c.g.t0 + c.g.ntl - 1);
            if (a <= b) DS_CHECK(pull(f, f.w0 + planec * (a - nA), c, c.phi + planec * (a - c.g.t0), planec * (b - a + 1)));
        }
        DS_CHECK(launch_prolong_phi(gf, gc0, f.w0, f.phi, coarse.dScale, 1.0 / dScale, f.st, nA));
        if (gf.ncl > 0) {
            const i64 cA = gf.t0 >> 1, cB = (gf.t0 + gf.ncl - 1) >> 1, nl = cB - cA + 1;
            double *tmp = f.beta2;
            if (!tmp) { set_error("multilevel transfer on time slabs needs the fused dataflow"); return DOTSOCP_EINVAL; }
            for (auto &c : coarse.slabs) {
                const i64 a = std::max<i64>(cA, c.g.t0), b = std::min<i64>(cB, c.g.t0 + c.g.ncl - 1);
                if (a > b) continue;
                for (int j = 0; j < 10; ++j)
                    DS_CHECK(pull(f, tmp + (i64)j * nl * planec + planec * (a - cA), c,
                                  c.beta + (i64)j * c.g.Nc + planec * (a - c.g.t0), planec * (b - a + 1)));
            }
            DS_CHECK(launch_prolong_beta(gf, gc0, tmp, f.beta, f.z, coarse.sigma, coarse.cScale * coarse.E, 1.0 / cScale / E,
                                         f.st, cA, nl * planec));
        }
    }
    // x <- sc * x ./ w over the owned entries of a q-layout array (the halo layers of a slab are exchanged at begin())
    auto scale_owned = [&](Slab &f, double *x, double sc, bool always) -> int {
        const Grid &g = f.g;
        if (!always && !f.weight) return 0;
        const double *w = f.weight;
        DS_CHECK(launch_scale_div(x, w, g.Nz, sc, f.st));
        DS_CHECK(launch_scale_div(x + g.offBx, w ? w + g.offBx : nullptr, g.bxLayer * g.ntl, sc, f.st));
        DS_CHECK(launch_scale_div(x + g.offBy, w ? w + g.offBy : nullptr, g.byLayer * g.ntl, sc, f.st));
        return 0;
    };
    // alpha = F*B*(-betaR) ./ w, times 1/cScale_f/D_f; a slab's first edge layer needs the last cell layer of its left neighbour
    if (multi()) {
        FOR_SLABS(f)
            if (!f.g.last)
                DS_CHECK(launch_kkt_tail(f.g, f.alpha, f.z, nullptr, f.send_plane, f.send_plane2, f.send_bx, f.send_by, f.st));
        DS_CHECK(shift(+1, [](Slab &s) { return s.send_bx; }, [](Slab &s) { return s.btail_bx; }, slabs[0].g.bxLayer));
        DS_CHECK(shift(+1, [](Slab &s) { return s.send_by; }, [](Slab &s) { return s.btail_by; }, slabs[0].g.byLayer));
    }
    FOR_SLABS(f) DS_CHECK(launch_bfd_conj(f.g, f.alpha, f.z, 1.0, f.st, f.btail_bx, f.btail_by));
    if (multi()) {
        // ... which adds the neighbour's pair as one term.  The transfer gives the bits of one slab on any split: the first
        // edge layer once more, from the neighbour's last cell layer of the columns 3, 4 -> w0 and 7, 8 -> w1 (both free
        // again, two layers at least), in mexBFdConj's order
        const i64 plane = slabs[0].g.plane;
        static const int cols[4] = {3, 4, 7, 8};
        for (int k = 0; k < 4; ++k)
            DS_CHECK(shift(+1, [k](Slab &s) { return s.z + (i64)cols[k] * s.g.Nc + s.g.plane * (s.g.ncl - 1); },
                           [k](Slab &s) { return (k < 2 ? s.w0 : s.w1) + s.g.plane * (k & 1); }, plane));
        FOR_SLABS(f)
            if (!f.g.first)
                DS_CHECK(launch_conj_first_layer(f.g, f.alpha, f.z, 1.0, f.w0, f.w0 + plane, f.w1, f.w1 + plane, f.st));
        DS_CHECK(sync_all());                   // the copies read the neighbours' z, which is zeroed below
    }
    FOR_SLABS(f) DS_CHECK(scale_owned(f, f.alpha, 1.0 / cScale / D, true));
    // q = (D_f/dScale_f) * grad(phiR) ./ w : the D_f / h factors are those of the loop's own stencil; the forward time
    // difference of a slab's last cell layer reads the first phi layer of its right neighbour
    if (multi())
        DS_CHECK(shift(-1, [](Slab &s) { return s.phi; }, [](Slab &s) { return s.phi + s.g.plane * s.g.ntl; }, slabs[0].g.plane));
    FOR_SLABS(f) {
        DS_CHECK(launch_grad(f.g, lc, f.phi, f.q, f.st));
        DS_CHECK(scale_owned(f, f.q, 1.0, false));
        DS_HIP(ds_memset_async(f.z, 0, sizeof(double) * 10 * f.g.Nc, f.st));       // var.z of initialize.m
    }
    DS_CHECK(sync_all());
    DS_CHECK(canary_after());                   // the gathers into w0 / beta2 and the kernels wrote inside their buffers
    return 0;
}

// --------------------------------------------------------------------------------------
// upload / download.  Host pointers hold the GLOBAL field in the reference layout; with an RCCL
// communicator attached they hold this process's slab of it (same layout restricted to the owned
// layers: q = [q0 cells | bx layers | by layers]).
// --------------------------------------------------------------------------------------
static const int k1dCols[6] = {0, 5, 6, 7, 8, 9};   // 1-D cone columns inside the 10-plane layout

i64 Solver::field_len(int field) const {
    i64 ntn = nt, ntc = nt - 1;
    if (remote()) { ntn = slabs[0].g.ntl; ntc = slabs[0].g.ncl; }
    const i64 Nz = ny * nx * ntc, Nphi = ny * nx * ntn;
    const i64 Nq = Nz + ny * (nx - 1) * ntn + (ny - 1) * nx * ntn;
    switch (field) {
        case DOTSOCP_F_PHI: case DOTSOCP_F_C: return Nphi;
        case DOTSOCP_F_Q: case DOTSOCP_F_ALPHA: case DOTSOCP_F_WEIGHT: return Nq;
        case DOTSOCP_F_Z: case DOTSOCP_F_BETA: return Nz * (prob.dim == 1 ? 6 : 10);
        default: return -1;
    }
}

// rows of `rowlen` doubles: device rows `pitch` apart, the other side contiguous (reference layout) -- host rows, or with
// ROWS_FROM_DEV rows on device `src_dev` that are read
int Solver::copy_rows(double *dev, double *host, i64 rowlen, i64 pitch, i64 nrows, int dir, hipStream_t st, int src_dev) {
    if (rowlen <= 0 || nrows <= 0) return 0;
    const bool up = dir != ROWS_DOWN;
    hipMemcpyKind kind = dir == ROWS_UP ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    if (dir == ROWS_FROM_DEV) {
        kind = hipMemcpyDeviceToDevice;
        int here = -1;
        DS_HIP(hipGetDevice(&here));
        if (src_dev >= 0 && src_dev != here) {
            // between devices only whole blocks travel: copy_field stages the layers of a pitched slab on the slab's own
            // device first, so a pitched request never arrives here
            DS_ARG(pitch == rowlen, "pitched rows cannot be copied between devices");
            DS_HIP(ds_memcpy_peer_async(dev, here, host, src_dev, sizeof(double) * rowlen * nrows, st));
            return 0;
        }
    }
    if (pitch == rowlen) {
        if (up) DS_HIP(ds_memcpy_async(dev, host, sizeof(double) * rowlen * nrows, kind, st));
        else DS_HIP(ds_memcpy_async(host, dev, sizeof(double) * rowlen * nrows, kind, st));
        return 0;
    }
    if (up) DS_HIP(ds_memcpy2d_async(dev, sizeof(double) * pitch, host, sizeof(double) * rowlen, sizeof(double) * rowlen,
                                    (size_t)nrows, kind, st));
    else DS_HIP(ds_memcpy2d_async(host, sizeof(double) * rowlen, dev, sizeof(double) * pitch, sizeof(double) * rowlen,
                                 (size_t)nrows, kind, st));
    return 0;
}

// DOTSOCP_WEIGHT_STAGE=1: every slab stages its layers of a device source as if the source lived on another device
static bool weight_stage_forced() {
    const char *e = getenv("DOTSOCP_WEIGHT_STAGE");
    return e && atoi(e) != 0;
}

// `host`: the global field in the reference layout -- on the host (dir = ROWS_DOWN / ROWS_UP), or on device `src_dev`
// (ROWS_FROM_DEV: read from there).  A slab with pitched rows on ANOTHER device than the source cannot take its rows one
// by one (copy_rows): its three contiguous layer ranges of [q0; bx; by] travel as peer copies into a staging buffer on
// the slab's device and the rows are spread from there.
static int copy_field(Solver &S, int field, double *host, int up, int src_dev = -1) {
    DeviceScratch staged(S);               // staging buffers: released once every stream of the context is idle
    const i64 ny = S.ny, nx = S.nx;
    i64 ntn = S.nt, ntc = S.nt - 1;
    if (S.remote()) { ntn = S.slabs[0].g.ntl; ntc = S.slabs[0].g.ncl; }
    // host side: the reference layout q = [q0 (ny, nx, nt-1) ; bx (ny, nx-1, nt) ; by (ny-1, nx, nt)]; device side: rows
    // py (by: pyb) doubles apart (common.h)
    const i64 hplane = ny * nx, hbx = ny * (nx - 1), hby = (ny - 1) * nx;
    const i64 NzG = hplane * ntc;
    const i64 bxG = NzG, byG = NzG + hbx * ntn;
    for (auto &s : S.slabs) {
        DS_CHECK(S.use(s));
        hipStream_t cur = s.st;
        const Grid &g = s.g;
        const i64 t0 = S.remote() ? 0 : g.t0;
        auto nodes = [&](double *dev, double *h, i64 layers) { return S.copy_rows(dev, h, ny, g.py, nx * layers, up, cur, src_dev); };
        switch (field) {
            case DOTSOCP_F_PHI: DS_CHECK(nodes(s.phi, host + hplane * t0, g.ntl)); break;
            case DOTSOCP_F_C: DS_CHECK(nodes(s.c, host + hplane * t0, g.ntl)); break;
            case DOTSOCP_F_Q: case DOTSOCP_F_ALPHA: case DOTSOCP_F_WEIGHT: {
                double *d = field == DOTSOCP_F_Q ? s.q : (field == DOTSOCP_F_ALPHA ? s.alpha : s.weight);
                double *part[3] = {host + hplane * t0, host + bxG + hbx * t0, host + byG + hby * t0};
                const i64 count[3] = {hplane * g.ncl, hbx * g.ntl, hby * g.ntl};
                int from = src_dev;
                if (up == Solver::ROWS_FROM_DEV && ((s.dev != src_dev && g.py > ny) || weight_stage_forced())) {
                    double *buf = nullptr;
                    DS_CHECK(staged.alloc(&buf, count[0] + count[1] + count[2]));
                    for (int k = 0; k < 3; ++k) {
                        if (count[k] > 0)
                            DS_HIP(ds_memcpy_peer_async(buf, s.dev, part[k], src_dev, sizeof(double) * (size_t)count[k], cur));
                        part[k] = buf;
                        buf += count[k];
                    }
                    from = s.dev;
                }
                DS_CHECK(S.copy_rows(d, part[0], ny, g.py, nx * g.ncl, up, cur, from));
                DS_CHECK(S.copy_rows(d + g.offBx, part[1], ny, g.py, (nx - 1) * g.ntl, up, cur, from));
                DS_CHECK(S.copy_rows(d + g.offBy, part[2], ny - 1, g.pyb, nx * g.ntl, up, cur, from));
                break;
            }
            case DOTSOCP_F_Z: case DOTSOCP_F_BETA: {
                double *d = field == DOTSOCP_F_Z ? s.z : s.beta;
                const int K = S.prob.dim == 1 ? 6 : 10;
                if (up && S.prob.dim == 1) DS_HIP(ds_memset_async(d, 0, sizeof(double) * 10 * g.Nc, cur));
                for (int j = 0; j < K; ++j) {
                    const int pj = S.prob.dim == 1 ? k1dCols[j] : j;
                    DS_CHECK(nodes(d + pj * g.Nc, host + j * NzG + hplane * t0, g.ncl));
                }
                break;
            }
        }
    }
    DS_CHECK(S.sync_all());
    return 0;
}

int Solver::upload(int field, const double *host) {
    DS_ARG(host != nullptr, "host pointer is NULL");
    DS_ARG(field_len(field) >= 0, "unknown field");
    DS_ARG(field != DOTSOCP_F_WEIGHT || prob.weighted, "weight uploaded to an unweighted problem");
    if (begun) { set_error("upload() after begin()"); return DOTSOCP_ESTATE; }
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    DS_CHECK(ensure_alloc());
    return copy_field(*this, field, const_cast<double *>(host), true);
}

// model.weight from a device array in the reference layout (a level of a weight pyramid): the row copies of upload(),
// device to device -- rows land py / pyb apart, the pad entries keep the ones alloc_slabs gave them, every slab takes its
// layers (peer copies where the array lives on another device; copy_field stages those of a pitched slab).  The copies
// between DIFFERENT devices have never run on hardware (one-GPU boxes); DOTSOCP_WEIGHT_STAGE=1 runs the staged form on one.
int Solver::upload_weight_from(const double *src, int src_dev, i64 src_ny, i64 src_nx, i64 src_nt) {
    DS_ARG(src != nullptr, "weight source is NULL");
    DS_ARG(prob.weighted, "weight handed to an unweighted problem");
    DS_ARG(prob.dim == 2, "the weight pyramid serves 2-D problems");
    DS_ARG(!remote(), "contexts with an RCCL communicator take their weight from the host");
    DS_ARG(src_ny == ny && src_nx == nx && src_nt == nt, "the pyramid level is not this context's grid");
    if (begun) { set_error("upload() after begin()"); return DOTSOCP_ESTATE; }
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    DS_CHECK(ensure_alloc());
    return copy_field(*this, DOTSOCP_F_WEIGHT, const_cast<double *>(src), ROWS_FROM_DEV, src_dev);
}

// model.c of initialize.m:42-50 is zero except on its first and last time layer, and every operation of the loop on c
// (x * mul / div with positive factors) keeps a +0.0 what it is.  One reduction per slab at begin(), when every upload
// of c is over (upload() after begin() is refused); a c that was never uploaded is the zeros of its allocation and passes.
int Solver::detect_c_ends() {
    FOR_SLABS(s) {
        int *flag = nullptr, h = 1;
        DS_CHECK(dmalloc(&flag, 1));
        int rc = 0;
        if (ds_memset_async(flag, 0, sizeof(int), s.st) != hipSuccess) rc = DOTSOCP_EHIP;
        if (!rc) rc = launch_c_interior_test(s.g, s.c, flag, s.st);
        if (!rc && ds_memcpy_async(&h, flag, sizeof(int), hipMemcpyDeviceToHost, s.st) != hipSuccess) rc = DOTSOCP_EHIP;
        if (!rc && ds_stream_synchronize(s.st) != hipSuccess) rc = DOTSOCP_EHIP;
        dfree(flag);
        if (rc) { if (rc == DOTSOCP_EHIP) set_error("the zero test of c failed"); return rc; }
        s.c_ends = (h == 0);
    }
    return 0;
}

// time layers [t0, t0 + n) of a node field (phi, c) from a host buffer that holds only those layers; the other layers
// keep what they have (zeros after create).  model.c of initialize.m:42-50 is zero except for its first and last layer:
// a driver uploads those two instead of a vector as long as the grid (1 GB at 1025 x 1025 x 129).
int Solver::upload_layers(int field, const double *host, i64 t0, i64 n) {
    DS_ARG(host != nullptr, "host pointer is NULL");
    DS_ARG(field == DOTSOCP_F_PHI || field == DOTSOCP_F_C, "layer uploads serve the node fields (phi, c)");
    const i64 ntn = remote() ? slabs[0].g.ntl : nt;
    DS_ARG(t0 >= 0 && n >= 0 && t0 + n <= ntn, "layer range outside the field");
    if (begun) { set_error("upload() after begin()"); return DOTSOCP_ESTATE; }
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    DS_CHECK(ensure_alloc());
    const i64 hplane = ny * nx;
    for (auto &s : slabs) {
        DS_CHECK(use(s));
        const Grid &g = s.g;
        const i64 base = remote() ? 0 : g.t0;
        const i64 lo = std::max(t0, base), hi = std::min(t0 + n, base + g.ntl);
        if (lo >= hi) continue;
        double *dev = (field == DOTSOCP_F_PHI ? s.phi : s.c) + g.plane * (lo - base);
        DS_CHECK(copy_rows(dev, const_cast<double *>(host) + hplane * (lo - t0), ny, g.py, nx * (hi - lo), true, s.st));
    }
    DS_CHECK(sync_all());
    return 0;
}

int Solver::download(int field, double *host) {
    DS_ARG(host != nullptr, "host pointer is NULL");
    DS_ARG(field_len(field) >= 0, "unknown field");
    DS_ARG(field != DOTSOCP_F_WEIGHT || prob.weighted, "no weight in an unweighted problem");
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    DS_CHECK(ensure_alloc());
    if (field == DOTSOCP_F_Z || field == DOTSOCP_F_BETA) {
        DS_CHECK(need_beta_form("download"));
        DS_CHECK(ensure_z());
        DS_CHECK(flush_beta());
    }
    if (field == DOTSOCP_F_ALPHA) DS_CHECK(flush_alpha());
    if (field == DOTSOCP_F_Q) DS_CHECK(need_q("download"));
    host_first_touch(host, sizeof(double) * (size_t)field_len(field));
    DS_CHECK(copy_field(*this, field, host, false));
    // after finish(): var.alpha = sigma * alpha, var.beta = sigma * beta  (solver_socp_inPALM.m:335-336)
    if (finished && (field == DOTSOCP_F_ALPHA || field == DOTSOCP_F_BETA)) host_scale(host, field_len(field), sigma);
    return 0;
}

}  // namespace dotsocp
