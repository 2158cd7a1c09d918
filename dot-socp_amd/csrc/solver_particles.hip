// Velocity v = E / rho and particles along it (kernels: advect.hip; semantics: include/dotsocp.h): dotsocp_recover_velocity and
// the three marches dotsocp_advect_particles, dotsocp_push_mass, dotsocp_map_report.  The velocity exists one node layer at a
// time: every slab keeps a ring of two layers, slot (global node & 1), filled by k_velocity_layer from the slab's own alpha --
// or, for the node behind a slab's last cell, by its right neighbour, which owns that node, and copied over.
#include <cmath>
#include <cstring>

#include "solver.h"

namespace dotsocp {

int Solver::velocity_stage(const double *rho0, const double *rho1) {
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    DS_CHECK(stage_left_tail());
    FOR_SLABS(s) {
        if (!s.adv_vel) DS_CHECK(s.zalloc(&s.adv_vel, 4 * slabs[0].g.plane));
        s.adv_have[0] = s.adv_have[1] = -1;
        DS_CHECK(stage_rho_ends(s, rho0, rho1));
    }
    return 0;
}

int Solver::velocity_layer(Slab &s, i64 tg, double floor) {
    const int slot = (int)(tg & 1);
    if (s.adv_have[slot] == tg) return 0;
    const Grid &g = s.g;
    const i64 plane = g.plane;
    double *dst = s.adv_vel + 2 * plane * slot;
    if (tg >= g.t0 && tg < g.t0 + g.ntl) {
        DS_CHECK(use(s));
        const bool prof = &s == &slabs[0];
        if (prof) prof_begin(PH_VELOCITY);
        DS_CHECK(launch_velocity_layer(g, s.alpha, s.weight, s.w1, s.w1 + plane, s.a0_prev, sigma, cScale * D, prob.dim == 1,
                                       tg - g.t0, floor, dst, dst + plane, s.st));
        if (prof) prof_end(PH_VELOCITY);
    } else {
        const size_t r = (size_t)(&s - slabs.data()) + 1;
        if (tg != g.t0 + g.ntl || r >= slabs.size()) { set_error("internal: velocity layer %lld is not this slab's", tg); return DOTSOCP_ESTATE; }
        DS_CHECK(velocity_layer(slabs[r], tg, floor));
        DS_CHECK(xcopy(slabs[r], slabs[r].adv_vel + 2 * plane * slot, s, dst, 2 * plane));
    }
    s.adv_have[slot] = tg;
    return 0;
}

int Solver::recover_velocity(const double *rho0, const double *rho1, double floor, double *vX, double *vY) {
    DS_ARG(rho0 != nullptr && rho1 != nullptr, "recover_velocity() needs rho0 and rho1 (one of them is NULL)");
    DS_ARG(!remote(), "recover_velocity() serves the slabs of one process; contexts with an RCCL communicator are not served");
    if (!finished) { set_error("recover_velocity() needs finish()"); return DOTSOCP_ESTATE; }
    DS_CHECK(need_beta_form("recover_velocity"));
    DS_CHECK(velocity_stage(rho0, rho1));
    const i64 hplane = ny * nx;
    FOR_SLABS(s) {
        const Grid &g = s.g;
        for (i64 tl = 0; tl < g.ntl; ++tl) {
            const i64 tg = g.t0 + tl;
            DS_CHECK(velocity_layer(s, tg, floor));
            double *d = s.adv_vel + 2 * g.plane * (tg & 1);
            if (vX) DS_CHECK(copy_rows(d, vX + hplane * tg, ny, g.py, nx, false, s.st));
            if (vY) DS_CHECK(copy_rows(d + g.plane, vY + hplane * tg, ny, g.py, nx, false, s.st));
        }
    }
    DS_CHECK(sync_all());
    DS_CHECK(prof_flush());
    return canary_after();
}

// --------------------------------------------------------------------------------------
// The march of the three particle calls.  The particles live in one block per slab (particle_block.h); the slab that owns
// cell layer k runs interval k, the block travels when the march leaves a slab.
// FRAMES: every slab also has a frame buffer [count plane / frame (plane) | tile sums (report_tiles) | l1 sums (nf)].  A frame is
// deposited by the slab that OWNS its node (whose rho layer the comparison needs): going forward the particles are handed to
// the right neighbour before the deposit at a slab's first node, one step earlier than the interval behind it would ask.
// PATH_SUMS: the march is k_advect<., true>; the slab of the last interval has the buffer of k_map_final (MapFinalBlock).
// --------------------------------------------------------------------------------------
namespace {

#define MARCH_ARG(cond, fmt) do { if (!(cond)) { set_error("invalid argument: " fmt, who); return DOTSOCP_EINVAL; } } while (0)
enum Carry { TRAJECTORIES, FRAMES, PATH_SUMS };     // what a march carries beyond the positions

struct March {
    Solver &S;
    const char *who;                    // the call: every message names it
    const Carry kind;
    const bool have_opts, dim1;
    const i64 n;
    const int nsub, dir;
    const double floor;
    double *const x, *const y;          // host, in: seeds, out: end positions
    const double *mass = nullptr;       // host: n (FRAMES), n or NULL = all 1.0 (PATH_SUMS)
    i64 *n_clamped = nullptr;
    double *traj_x = nullptr, *traj_y = nullptr;                    // TRAJECTORIES: n x nt each or NULL
    const i64 *nodes = nullptr;         // FRAMES: nf ascending frame nodes
    i64 nf = 0;
    double *frames = nullptr;           // ... host: ny x nx x nf
    double *l1 = nullptr;               // ... host: nf, or NULL
    double unit = 0.0;                  // ... 2^(e - 50) for n * max(mass) in [2^(e-1), 2^e)
    double *unit_out = nullptr;         // ... where the caller wants the unit, or NULL
    dotsocp_map_report_t *rep = nullptr;                            // PATH_SUMS: the report and
    double *disp = nullptr, *len = nullptr, *action = nullptr;      // n each or NULL

    template <class Opts>
    March(Solver &s, const char *call, Carry k, const Opts *o, double *x_, double *y_)
        : S(s), who(call), kind(k), have_opts(o != nullptr), dim1(s.prob.dim == 1), n(o ? o->n : 0), nsub(o ? o->nsub : 0),
          dir(o ? o->direction : 0), floor(o ? o->rho_floor : 0.0), x(x_), y(y_), scratch(s) {}

    // pointers and options, the seeds and masses, then the context: finished, beta in memory, a cell along every axis
    int check(const double *rho0, const double *rho1) {
        MARCH_ARG(rho0 != nullptr && rho1 != nullptr && have_opts && y != nullptr && (dim1 || x != nullptr),
                  "%s() needs rho0, rho1, opts and x (2-D: y too); one of them is NULL");
        if (kind == FRAMES) MARCH_ARG(mass != nullptr && nodes != nullptr && frames != nullptr,
                                      "%s() needs mass, frame_nodes and frames; one of them is NULL");
        if (kind == PATH_SUMS) MARCH_ARG(rep != nullptr, "%s() needs rep; it is NULL");
        MARCH_ARG(n >= 1, "%s() needs n >= 1 particles");
        MARCH_ARG(nsub >= 1, "%s() needs nsub >= 1 steps per time interval");
        MARCH_ARG(dir == 1 || dir == -1, "%s() runs in direction +1 or -1");
        if (kind == FRAMES) MARCH_ARG(nf >= 1, "%s() needs nf >= 1 frame nodes");
        MARCH_ARG(!S.remote(), "%s() serves the slabs of one process; contexts with an RCCL communicator are not served");
        for (i64 k = 0; k < nf; ++k)
            MARCH_ARG(nodes[k] >= 0 && nodes[k] < S.nt && (k == 0 || nodes[k] > nodes[k - 1]),
                      "%s(): frame_nodes must be strictly ascending node indices in [0, nt)");
        double mmax = mass ? 0.0 : 1.0;
        for (i64 p = 0; p < n; ++p) {
            MARCH_ARG(std::isfinite(y[p]) && (dim1 || std::isfinite(x[p])), "%s(): a seed is not finite");
            if (!mass) continue;
            MARCH_ARG(std::isfinite(mass[p]) && mass[p] >= 0.0, "%s(): a mass is negative or not finite");
            mmax = mass[p] > mmax ? mass[p] : mmax;
        }
        MARCH_ARG(mmax > 0.0, "%s(): all masses are zero");
        if (kind == FRAMES) {
            int e = 0;
            (void)frexp((double)n * mmax, &e);
            unit = ldexp(1.0, e - 50);
            MARCH_ARG(std::isfinite((double)n * mmax) && unit >= 2.2250738585072014e-308,
                      "%s(): n * max(mass) overflows, or its unit 2^(e-50) is not a normal double");
        }
        if (!S.finished) { set_error("%s() needs finish()", who); return DOTSOCP_ESTATE; }
        DS_CHECK(S.need_beta_form(who));
        MARCH_ARG(S.ny >= 2 && (dim1 || S.nx >= 2), "%s() needs two nodes along every axis");
        if (unit_out) *unit_out = unit;
        return 0;
    }

    const size_t nb = sizeof(double) * (size_t)n;      // bytes of one region of n doubles
    i64 plane = 0, tiles = 0;           // doubles of a device layer, report_tiles of it
    const ParticleBlock L{n, kind == FRAMES, kind == PATH_SUMS};
    MapFinalBlock M{0, false, false, false, 0};
    double *final_buf = nullptr;        // PATH_SUMS: on slab `fin`, the one that runs the last interval
    const size_t fin = dir > 0 ? S.slabs.size() - 1 : 0;
    size_t cur = dir > 0 ? 0 : S.slabs.size() - 1;      // the slab that holds the particles
    i64 fi = 0;                         // FRAMES: the next requested frame
    // host side of the copies: declared before `scratch`, so alive until its destructor has waited for every stream
    std::vector<i64> units;             // FRAMES: units per particle
    std::vector<double> l1_host;
    std::vector<size_t> owner;          // FRAMES: the slab that deposited frame f
    double edges[DOTSOCP_REPORT_BINS + 1], msums[MS_COUNT] = {0};
    unsigned long long mcounts[MC_COUNT] = {0}, count = 0;
    DeviceScratch scratch;              // LAST member: destroyed first, and its destructor synchronises

    // scratch.bufs by purpose: the block of slab k (at: a region of the current slab's); FRAMES: its frame buffer, behind the blocks
    template <class T = double> T *at(i64 off) const { return (T *)(block(cur) + off); }
    double *block(size_t k) const { return scratch.bufs[k]; }
    double *frame(size_t k) const { return scratch.bufs[S.slabs.size() + k]; }
    // Buffers with integer regions stay as they come under DOTSOCP_POISON=1; their regions of doubles [fp_off, + fp_len) and
    // [fp_off2, + fp_len2) are poisoned by name.  The block: units, flags and count are integers -- seed() sets the whole
    // block of the first slab to zero, hand_over() copies the whole block to the next.  The frame buffer: the deposit layer
    // is 64-bit integers, set to zero by frame_at() before every deposit.
    int alloc_per_slab(i64 doubles, i64 fp_off, i64 fp_len, i64 fp_off2 = 0, i64 fp_len2 = 0) {
        double *b;
        for (auto &s : S.slabs) {
            DS_CHECK(S.use(s));
            DS_CHECK(scratch.alloc(&b, doubles, false));
            if (fp_len > 0) DS_CHECK(poison_region(b + fp_off, sizeof(double) * (size_t)fp_len));
            if (fp_len2 > 0) DS_CHECK(poison_region(b + fp_off2, sizeof(double) * (size_t)fp_len2));
        }
        return 0;
    }

    // PATH_SUMS: the final buffer with the seeds as given, the masses and the bin edges, counters zeroed
    int map_stage() {
        Slab &s = S.slabs[fin];
        DS_CHECK(S.use(s));
        // (DOTSOCP_POISON=1: the counters are integers, set to zero below; the doubles around them are poisoned by name)
        DS_CHECK(scratch.alloc(&final_buf, M.total, false));
        double *b = final_buf;
        DS_CHECK(poison_region(b, sizeof(double) * (size_t)M.counts));
        DS_CHECK(poison_region(b + M.partials, sizeof(double) * (size_t)(M.total - M.partials)));
        report_edges_host(edges);
        if (!dim1) DS_HIP(ds_memcpy_async(b + M.seeds, x, nb, hipMemcpyHostToDevice, s.st));
        DS_HIP(ds_memcpy_async(b + M.seeds + n, y, nb, hipMemcpyHostToDevice, s.st));
        if (mass) DS_HIP(ds_memcpy_async(b + M.mass, mass, nb, hipMemcpyHostToDevice, s.st));
        DS_HIP(ds_memcpy_async(b + M.edges, edges, sizeof edges, hipMemcpyHostToDevice, s.st));
        DS_HIP(ds_memset_async(b + M.counts, 0, sizeof(unsigned long long) * MC_COUNT, s.st));
        return 0;
    }

    int hand_over() {
        const size_t nxt = dir > 0 ? cur + 1 : cur - 1;
        if (nxt >= S.slabs.size()) { set_error("internal: the particles left the last slab"); return DOTSOCP_ESTATE; }
        DS_CHECK(S.xcopy(S.slabs[cur], block(cur), S.slabs[nxt], block(nxt), L.total));
        cur = nxt;
        return 0;
    }

    // FRAMES: the particles stand at `node`: if it is the next requested frame, deposit, convert, compare and download it
    int frame_at(i64 node) {
        if (fi < 0 || fi >= nf || nodes[fi] != node) return 0;
        while (dir > 0 && node >= S.slabs[cur].g.t0 + S.slabs[cur].g.ntl) DS_CHECK(hand_over());
        Slab &s = S.slabs[cur];
        const Grid &g = s.g;
        if (node < g.t0 || node >= g.t0 + g.ntl) { set_error("internal: frame node %lld is not this slab's", node); return DOTSOCP_ESTATE; }
        DS_CHECK(S.use(s));
        double *F = frame(cur);
        const bool prof = cur == 0;
        DS_HIP(ds_memset_async(F, 0, sizeof(double) * (size_t)plane, s.st));
        if (prof) S.prof_begin(PH_DEPOSIT);
        DS_CHECK(launch_deposit(dim1, S.ny, S.nx, g.py, n, at(L.px), at(L.py), at<i64>(L.units), (unsigned long long *)F, s.st));
        if (prof) { S.prof_end(PH_DEPOSIT); S.prof_begin(PH_FRAME_L1); }
        DS_CHECK(launch_frame_l1(g, s.alpha, s.weight, s.w1, s.w1 + plane, s.a0_prev, S.sigma, S.cScale * S.D, node - g.t0, unit, F,
                                 F + plane, F + plane + tiles + fi, s.st));
        if (prof) S.prof_end(PH_FRAME_L1);
        DS_CHECK(S.copy_rows(F, frames + S.ny * S.nx * fi, S.ny, g.py, S.nx, false, s.st));
        owner[(size_t)fi] = cur;
        fi += dir;
        return 0;
    }

    // the particles have arrived at `node`: its column of the trajectories, its frame
    int at_node(i64 node) {
        hipStream_t st = S.slabs[cur].st;
        if (traj_x && !dim1) DS_HIP(ds_memcpy_async(traj_x + n * node, at(L.px), nb, hipMemcpyDeviceToHost, st));
        if (traj_y) DS_HIP(ds_memcpy_async(traj_y + n * node, at(L.py), nb, hipMemcpyDeviceToHost, st));
        return kind == FRAMES ? frame_at(node) : 0;
    }

    int seed() {
        Slab &s = S.slabs[cur];
        DS_CHECK(S.use(s));
        DS_HIP(ds_memset_async(block(cur), 0, sizeof(double) * (size_t)L.total, s.st));
        if (!dim1) DS_HIP(ds_memcpy_async(at(L.px), x, nb, hipMemcpyHostToDevice, s.st));
        DS_HIP(ds_memcpy_async(at(L.py), y, nb, hipMemcpyHostToDevice, s.st));
        if (kind == FRAMES) DS_HIP(ds_memcpy_async(at(L.units), units.data(), nb, hipMemcpyHostToDevice, s.st));
        DS_CHECK(launch_advect_seed(dim1, n, at(L.px), at(L.py), at<unsigned int>(L.flags), s.st));
        return at_node(dir > 0 ? 0 : S.nt - 1);
    }

    // the interval between nodes k and k + 1: run by the slab that owns cell k
    int interval(i64 k) {
        while (k < S.slabs[cur].g.t0 || k >= S.slabs[cur].g.t0 + S.slabs[cur].g.ncl) DS_CHECK(hand_over());
        Slab &s = S.slabs[cur];
        DS_CHECK(S.velocity_layer(s, k, floor));
        DS_CHECK(S.velocity_layer(s, k + 1, floor));
        DS_CHECK(S.use(s));
        const double *L0 = s.adv_vel + 2 * s.g.plane * (k & 1), *L1 = s.adv_vel + 2 * s.g.plane * ((k + 1) & 1);
        const double dt = (double)dir / (double)((S.nt - 1) * (i64)nsub);
        const bool prof = cur == 0, sums = kind == PATH_SUMS;
        if (prof) S.prof_begin(sums ? PH_ADVECT_PATH : PH_ADVECT);
        DS_CHECK(launch_advect(dim1, S.ny, S.nx, s.g.py, L0, L0 + s.g.plane, L1, L1 + s.g.plane, n, nsub, dir, dt, at(L.px), at(L.py),
                               at<unsigned int>(L.flags), s.st, sums ? at(L.sq) : nullptr, sums ? at(L.len) : nullptr));
        if (prof) S.prof_end(sums ? PH_ADVECT_PATH : PH_ADVECT);
        return at_node(dir > 0 ? k + 1 : k);
    }

    // PATH_SUMS: k_map_final on the slab that holds the particles, and the downloads of what it made
    int map_final() {
        Slab &s = S.slabs[cur];
        if (cur != fin) { set_error("internal: the particles ended on slab %zu, the seeds wait on slab %zu", cur, fin); return DOTSOCP_ESTATE; }
        double *b = final_buf;
        const bool prof = cur == 0;
        if (prof) S.prof_begin(PH_MAP_FINAL);
        DS_CHECK(launch_map_final(dim1, n, at(L.px), at(L.py), at(L.sq), at(L.len), b + M.seeds, b + M.seeds + n,
                                  mass ? b + M.mass : nullptr, b + M.edges, (double)((S.nt - 1) * (i64)nsub), disp ? b + M.disp : nullptr,
                                  action ? b + M.action : nullptr, b + M.partials, b + M.sums, (unsigned long long *)(b + M.counts),
                                  s.st));
        if (prof) S.prof_end(PH_MAP_FINAL);
        if (disp) DS_HIP(ds_memcpy_async(disp, b + M.disp, nb, hipMemcpyDeviceToHost, s.st));
        if (len) DS_HIP(ds_memcpy_async(len, at(L.len), nb, hipMemcpyDeviceToHost, s.st));
        if (action) DS_HIP(ds_memcpy_async(action, b + M.action, nb, hipMemcpyDeviceToHost, s.st));
        DS_HIP(ds_memcpy_async(msums, b + M.sums, sizeof msums, hipMemcpyDeviceToHost, s.st));
        DS_HIP(ds_memcpy_async(mcounts, b + M.counts, sizeof mcounts, hipMemcpyDeviceToHost, s.st));
        return 0;
    }

    // count the clamped particles, reduce (PATH_SUMS), download everything (l1: from every slab that deposited) and wait for it
    int finish() {
        Slab &s = S.slabs[cur];
        DS_CHECK(S.use(s));
        auto *counter = at<unsigned long long>(L.count);
        DS_CHECK(launch_advect_count(at<unsigned int>(L.flags), n, counter, s.st));
        if (kind == PATH_SUMS) DS_CHECK(map_final());
        if (!dim1) DS_HIP(ds_memcpy_async(x, at(L.px), nb, hipMemcpyDeviceToHost, s.st));
        DS_HIP(ds_memcpy_async(y, at(L.py), nb, hipMemcpyDeviceToHost, s.st));
        DS_HIP(ds_memcpy_async(&count, counter, sizeof count, hipMemcpyDeviceToHost, s.st));
        for (size_t k = 0; l1 && k < S.slabs.size(); ++k) {
            DS_CHECK(S.use(S.slabs[k]));
            bool mine = false;
            for (i64 f = 0; f < nf; ++f) mine = mine || owner[(size_t)f] == k;
            if (mine) DS_HIP(ds_memcpy_async(l1_host.data() + nf * (i64)k, frame(k) + plane + tiles, sizeof(double) * (size_t)nf,
                                             hipMemcpyDeviceToHost, S.slabs[k].st));
        }
        DS_CHECK(S.sync_all());
        DS_CHECK(S.prof_flush());
        return S.canary_after();
    }

    void fill_map_report() const {
        memset(rep, 0, sizeof *rep);
        auto dbl = [&](int slot) { double v; memcpy(&v, &mcounts[slot], sizeof v); return v; };
        rep->n = n;
        rep->n_clamped = (i64)count;
        rep->n_still = (i64)mcounts[MC_STILL];
        rep->mass = msums[MS_MASS];
        rep->cost_map = msums[MS_DISP2] / rep->mass;
        rep->cost_length = msums[MS_LEN2] / rep->mass;
        rep->cost_action = msums[MS_ACTION] / rep->mass;
        rep->disp_mean = msums[MS_DISP] / rep->mass;
        rep->len_mean = msums[MS_LEN] / rep->mass;
        rep->disp_max = dbl(MC_DISP_MAX);
        rep->len_max = dbl(MC_LEN_MAX);
        rep->detour_max = dbl(MC_DETOUR_MAX);
        for (int j = 0; j < DOTSOCP_REPORT_BINS; ++j) rep->detour_hist[j] = (i64)mcounts[MC_HIST + j];
        rep->detour_over = (i64)mcounts[MC_OVER];
    }

    int run(const double *rho0, const double *rho1) {
        DS_CHECK(check(rho0, rho1));
        if (kind == FRAMES) units.resize((size_t)n);
        for (size_t p = 0; p < units.size(); ++p) units[p] = llrint(mass[p] / unit);   // one division, one rounding
        DS_CHECK(S.velocity_stage(rho0, rho1));
        plane = S.slabs[0].g.plane;
        tiles = report_tiles(S.slabs[0].g);
        M = MapFinalBlock(n, mass != nullptr, disp != nullptr, action != nullptr, map_blocks(n));
        fi = dir > 0 ? 0 : nf - 1;
        l1_host.resize((size_t)(nf * (i64)S.slabs.size()));
        owner.resize((size_t)nf);
        DS_CHECK(alloc_per_slab(L.total, L.px, L.units, L.sq, L.flags - L.sq));
        if (kind == FRAMES) DS_CHECK(alloc_per_slab(plane + tiles + nf, plane, tiles + nf));
        if (kind == PATH_SUMS) DS_CHECK(map_stage());
        DS_CHECK(seed());
        for (i64 step = 0; step < S.nt - 1; ++step) DS_CHECK(interval(dir > 0 ? step : S.nt - 2 - step));
        DS_CHECK(finish());
        if (n_clamped) *n_clamped = (i64)count;
        if (kind == PATH_SUMS) fill_map_report();
        for (i64 f = 0; l1 && f < nf; ++f) l1[f] = l1_host[(size_t)(nf * (i64)owner[(size_t)f] + f)] / (double)(S.ny * S.nx);
        return 0;
    }
};

}  // namespace

int Solver::advect_particles(const double *rho0, const double *rho1, const dotsocp_advect_opts *o, double *x, double *y,
                             double *traj_x, double *traj_y, i64 *n_clamped) {
    March m(*this, "advect_particles", TRAJECTORIES, o, x, y);
    m.traj_x = traj_x, m.traj_y = traj_y, m.n_clamped = n_clamped;
    return m.run(rho0, rho1);
}

int Solver::push_mass(const double *rho0, const double *rho1, const dotsocp_push_opts *o, double *x, double *y,
                      const double *mass, const i64 *frame_nodes, double *frames, i64 *n_clamped, double *unit, double *l1) {
    March m(*this, "push_mass", FRAMES, o, x, y);
    m.mass = mass, m.nodes = frame_nodes, m.nf = o && frame_nodes ? o->nf : 0, m.frames = frames, m.l1 = l1;
    m.n_clamped = n_clamped, m.unit_out = unit;
    return m.run(rho0, rho1);
}

int Solver::map_report(const double *rho0, const double *rho1, const dotsocp_advect_opts *o, double *x, double *y, const double *mass,
                       dotsocp_map_report_t *rep, double *disp, double *len, double *action) {
    March m(*this, "map_report", PATH_SUMS, o, x, y);
    m.mass = mass, m.rep = rep, m.disp = disp, m.len = len, m.action = action;
    return m.run(rho0, rho1);
}

}  // namespace dotsocp
