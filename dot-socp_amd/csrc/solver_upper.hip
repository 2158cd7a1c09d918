// The upper bound on W2^2 and the map of its plan (include/dotsocp.h: dotsocp_plan_bound, dotsocp_upper_bound, dotsocp_plan_map,
// dotsocp_upper_map; kernels: softlax.hip).  One engine
// on unpitched layers serves the stateless call (host arrays, the null stream of `device`) and the context call (the first
// slab's device and stream; phi(t = 0) is copied out of the slab's pitched rows).  Nothing of a context is written: the
// call has its own scratch, released before it returns.
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "solver.h"

namespace dotsocp {
namespace {

// where the engine runs: S owns the profiling events (nullptr: the stateless call, which has none)
struct UpperRun {
    Solver *S;
    hipStream_t st;
    void begin(int phase) const { if (S) S->prof_begin(phase); }
    void end(int phase) const { if (S) S->prof_end(phase); }
};

int upper_check_opts(const dotsocp_upper_opts *o, const double *f_start, bool stateless) {
    DS_ARG(o != nullptr, "the upper bound needs its options (opts is NULL)");
    DS_ARG(std::isfinite(o->eps_h2) && o->eps_h2 > 0.0, "upper bound: eps_h2 must be positive and finite");
    DS_ARG(o->max_sweeps >= 0, "upper bound: max_sweeps must not be negative");
    DS_ARG(o->start >= 0 && o->start <= 2, "upper bound: start is 0 (zeros), 1 (the potential) or 2 (f_start)");
    DS_ARG(o->start != 2 || f_start != nullptr, "upper bound: start = 2 needs f_start");
    DS_ARG(!(stateless && o->start == 1), "upper bound: start = 1 needs a context (dotsocp_upper_bound)");
    return 0;
}

// What dotsocp_plan_map / dotsocp_upper_map ask of the engine beside the bound.  The arrays are host arrays on the engine's
// axes (a line lives along y: its displacement is Dy); each may be nullptr.  Frames: nf values of tau; `frames` takes the
// finished frames (double)count * unit, `counts` the raw 64-bit planes instead (the context call converts them on the slab
// that owns the frame's time node, where l1 is formed).
struct MapRequest {
    dotsocp_plan_map_t *res;
    double *Dx, *Dy, *C, *row, *spread;
    const double *taus;
    i64 nf;
    double *frames;
    i64 *counts;
};

int map_check_frames(const dotsocp_plan_map_t *map_res, i64 nf, const void *taus, const double *frames) {
    DS_ARG(map_res != nullptr, "the plan map needs its result struct (map_res is NULL)");
    DS_ARG(nf >= 0, "plan map: nf must not be negative");
    DS_ARG(nf == 0 || (taus != nullptr && frames != nullptr), "plan map: nf > 0 needs its times (taus / frame_nodes) and frames");
    return 0;
}

// Scratch: alloc(double **, i64, bool fp).  Layers ny x nx unpitched, y fastest (a line: ny nodes, nx = 1).  rho0, rho1 and
// the outputs are host arrays; the start: mode 0 none, 1 the negative of d_start (device, unpitched), 2 h_start (host).
template <class Scratch>
int upper_engine(Scratch &scratch, const UpperRun &run, i64 ny, i64 nx, bool dim1, const double *rho0, const double *rho1,
                 int mode, const double *d_start, const double *h_start, const dotsocp_upper_opts *o, dotsocp_upper *res,
                 double *f, double *g, double *E, double *er, double *ec, double *defects, const MapRequest *map = nullptr) {
    const i64 n = ny * nx, blocks = hl_blocks(n);
    hipStream_t st = run.st;
    const double hy = 1.0 / (double)(ny - 1), hx = dim1 ? 0.0 : 1.0 / (double)(nx - 1);
    const double eps = dim1 ? (o->eps_h2 * hy) * hy : (o->eps_h2 * hx) * hy, ieps = 1.0 / eps;
    DS_ARG(std::isfinite(eps) && eps > 0.0 && std::isfinite(ieps), "upper bound: eps_h2 hx hy is not a positive normal number");
    // [a | b | la | lb | f | g | in | v | v2 | E | mean | T | TM | er | ec | partials | sums | counters]
    enum { L_A = 0, L_B, L_LA, L_LB, L_F, L_G, L_IN, L_V, L_V2, L_E, L_MEAN, L_T, L_TM, L_ER, L_EC, L_COUNT };
    const i64 nsums = SS_COUNT + SM_COUNT + 1;
    double *buf = nullptr;
    // the counters are integers: the buffer is not poisoned as a whole (DOTSOCP_POISON=1), its doubles are, by name
    DS_CHECK(scratch.alloc(&buf, L_COUNT * n + SS_COUNT * blocks + nsums + SC_COUNT, false));
    auto layer = [&](int k) { return buf + (i64)k * n; };
    double *partials = buf + (i64)L_COUNT * n, *dsums = partials + SS_COUNT * blocks;
    double *dmass = dsums + SS_COUNT, *ddefect = dmass + SM_COUNT;
    unsigned long long *dcounts = (unsigned long long *)(dsums + nsums);
    DS_CHECK(poison_region(buf, sizeof(double) * (size_t)(L_COUNT * n + SS_COUNT * blocks + nsums)));
    DS_HIP(ds_memset_async(dcounts, 0, sizeof(unsigned long long) * SC_COUNT, st));
    // the densities wait in er / ec, a host start in v: all three are read by the first two kernels and written much later
    double *R0 = layer(L_ER), *R1 = layer(L_EC);
    DS_HIP(ds_memcpy_async(R0, rho0, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
    DS_HIP(ds_memcpy_async(R1, rho1, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
    if (mode == 2) DS_HIP(ds_memcpy_async(layer(L_V), h_start, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
    double mass[SM_COUNT] = {0};
    unsigned long long counts[SC_COUNT] = {0};
    run.begin(PH_SL_NODE);
    DS_CHECK(launch_sl_mass(R0, R1, n, partials, dmass, dcounts, st));
    run.end(PH_SL_NODE);
    DS_HIP(ds_memcpy_async(mass, dmass, sizeof mass, hipMemcpyDeviceToHost, st));
    DS_HIP(ds_memcpy_async(counts, dcounts, sizeof counts, hipMemcpyDeviceToHost, st));
    DS_HIP(ds_stream_synchronize(st));
    const double m0 = mass[SM_M0], m1 = mass[SM_M1];
    DS_ARG(counts[SC_BAD] == 0, "upper bound: an entry of rho0 or rho1 is negative or not finite");
    DS_ARG(std::isfinite(m0) && m0 > 0.0 && std::isfinite(m1) && m1 > 0.0,
           "upper bound: the sum of rho0 or of rho1 is not a positive finite number");
    // the map: the unit of the frames by the rule of dotsocp_push_mass, n the node count; its own scratch
    // [TA | KDY | KDX | Dx | Dy | C | row | spread | X | Y | counts | units | partials | sums | key, clamped | flags]
    enum { M_TA = 0, M_KDY, M_KDX, M_DX, M_DY, M_C, M_ROW, M_SPREAD, M_X, M_Y, M_CNT, M_UNITS, M_COUNT };
    double unit = 0.0, *mbuf = nullptr;
    std::vector<i64> units;
    if (map) {
        double mmax = 0.0;
        for (i64 i = 0; i < n; ++i) mmax = rho0[i] > mmax ? rho0[i] : mmax;
        int e = 0;
        (void)frexp((double)n * mmax, &e);
        unit = ldexp(1.0, e - 50);
        DS_ARG(std::isfinite((double)n * mmax) && unit >= 2.2250738585072014e-308,
               "plan map: nodes * max(rho0) overflows, or its unit 2^(e-50) is not a normal double");
        DS_CHECK(scratch.alloc(&mbuf, M_COUNT * n + SP_COUNT * blocks + SP_COUNT + 2 + (n + 1) / 2, false));
        DS_CHECK(poison_region(mbuf, sizeof(double) * (size_t)(M_CNT * n)));
        DS_CHECK(poison_region(mbuf + M_COUNT * n, sizeof(double) * (size_t)(SP_COUNT * blocks + SP_COUNT)));
    }
    auto mlayer = [&](int k) { return mbuf ? mbuf + (i64)k * n : nullptr; };
    double *mpartials = mlayer(M_COUNT), *dmsums = map ? mpartials + SP_COUNT * blocks : nullptr;
    unsigned long long *dmcounts = map ? (unsigned long long *)(dmsums + SP_COUNT) : nullptr;   // the key of disp_max, the clamped nodes
    unsigned int *dflags = map ? (unsigned int *)(dmcounts + 2) : nullptr;
    auto transform = [&](const double *in, double *out, double *mean) -> int {
        if (!dim1) {
            run.begin(PH_SL_PASS_X);
            DS_CHECK(launch_sl_pass_x(in, layer(L_T), layer(L_TM), nx, ny, ny, eps, st));
            run.end(PH_SL_PASS_X);
        }
        run.begin(PH_SL_PASS_Y);
        DS_CHECK(launch_sl_pass_y(dim1 ? in : layer(L_T), dim1 ? nullptr : layer(L_TM), out, mean, ny, nx, ny, eps, st));
        run.end(PH_SL_PASS_Y);
        return 0;
    };
    // the moment flavour: the same values, and the mean displacements in KDX / KDY
    auto transform_mom = [&](const double *in, double *out, double *mean) -> int {
        if (!dim1) {
            run.begin(PH_SL_PASS_X);
            DS_CHECK(launch_sl_mom_x(in, layer(L_T), layer(L_TM), mlayer(M_TA), nx, ny, ny, eps, st));
            run.end(PH_SL_PASS_X);
        }
        run.begin(PH_SL_PASS_Y);
        DS_CHECK(launch_sl_mom_y(dim1 ? in : layer(L_T), dim1 ? nullptr : layer(L_TM), dim1 ? nullptr : mlayer(M_TA), out, mean,
                                 mlayer(M_KDY), dim1 ? nullptr : mlayer(M_KDX), ny, nx, ny, eps, st));
        run.end(PH_SL_PASS_Y);
        return 0;
    };
    auto node = [&](int rc) -> int { run.end(PH_SL_NODE); return rc; };
    double *A = layer(L_A), *B = layer(L_B), *LA = layer(L_LA), *LB = layer(L_LB), *F = layer(L_F), *G = layer(L_G);
    double *IN = layer(L_IN), *V = layer(L_V), *V2 = layer(L_V2), *Ed = layer(L_E), *MEAN = layer(L_MEAN);
    SlInitArgs ia{R0, R1, mode == 1 ? d_start : (mode == 2 ? V : nullptr), A, B, LA, LB, F, IN, n, m0, m1, eps, mode, dcounts};
    run.begin(PH_SL_NODE);
    DS_CHECK(node(launch_sl_init(ia, st)));
    std::vector<double> defect;
    i64 sweeps = 0;
    while (sweeps < o->max_sweeps) {
        double d = 0.0;
        DS_CHECK(transform(IN, G, MEAN));                       // g = S(la - f)
        run.begin(PH_SL_NODE);
        DS_CHECK(node(launch_sl_minsub(LB, G, nullptr, IN, n, st)));
        DS_CHECK(transform(IN, V, MEAN));                       // f_new = S(lb - g)
        run.begin(PH_SL_NODE);
        DS_CHECK(node(launch_sl_defect(A, LA, F, V, IN, n, ieps, partials, ddefect, st)));
        DS_HIP(ds_memcpy_async(&d, ddefect, sizeof d, hipMemcpyDeviceToHost, st));
        DS_HIP(ds_stream_synchronize(st));
        defect.push_back(d);
        ++sweeps;
        if (d <= o->defect_tol) break;
    }
    DS_CHECK(transform(IN, G, MEAN));                           // g = S(la - f)
    run.begin(PH_SL_NODE);
    DS_CHECK(node(launch_sl_minsub(LB, G, nullptr, IN, n, st)));
    DS_CHECK(transform(IN, V, MEAN));                           // f~
    run.begin(PH_SL_NODE);
    DS_CHECK(node(launch_sl_minsub(LA, F, V, IN, n, st)));      // f' = min(f, f~)
    DS_CHECK(transform(IN, V, Ed));                             // (g~, E)
    run.begin(PH_SL_NODE);
    DS_CHECK(node(launch_sl_minsub(LB, G, V, IN, n, st)));      // g' = min(g, g~)
    DS_CHECK(map ? transform_mom(IN, V2, MEAN) : transform(IN, V2, MEAN));      // f^ (map: and the moments of its weights)
    SlFinalArgs fa{A, B, F, V2, G, V, Ed, layer(L_ER), layer(L_EC), ny, nx, hx, hy, ieps, partials};
    double sums[SS_COUNT] = {0};
    run.begin(PH_SL_NODE);
    DS_CHECK(node(launch_sl_final(fa, dsums, st)));
    DS_HIP(ds_memcpy_async(sums, dsums, sizeof sums, hipMemcpyDeviceToHost, st));
    DS_HIP(ds_memcpy_async(counts, dcounts, sizeof counts, hipMemcpyDeviceToHost, st));
    double msums[SP_COUNT] = {0};
    unsigned long long mcounts[2] = {0, 0};
    if (map) {
        DS_HIP(ds_stream_synchronize(st));      // the node kernel takes the fill's moments as scalars
        const double R0s = sums[SS_R0], C0s = sums[SS_C0], fill = R0s < C0s ? R0s : C0s;
        SlMapArgs ma{A, F, V2, layer(L_ER), MEAN, dim1 ? nullptr : mlayer(M_KDX), mlayer(M_KDY),
                     mlayer(M_DX), mlayer(M_DY), mlayer(M_C), mlayer(M_ROW), mlayer(M_SPREAD), ny, nx, hx, hy, ieps,
                     fill > 0.0 ? C0s / fill : 0.0, C0s > 0.0 ? sums[SS_C1X] / C0s : 0.0, C0s > 0.0 ? sums[SS_C1Y] / C0s : 0.0,
                     C0s > 0.0 ? sums[SS_C2] / C0s : 0.0, mpartials, dmcounts};
        DS_HIP(ds_memset_async(dmcounts, 0, sizeof(unsigned long long) * 2, st));
        run.begin(PH_SL_NODE);
        DS_CHECK(node(launch_sl_map(ma, dmsums, st)));
        if (map->nf > 0) {
            units.resize((size_t)n);
            for (i64 i = 0; i < n; ++i) units[(size_t)i] = llrint(rho0[i] / unit);     // one division, one rounding
            i64 *dunits = (i64 *)mlayer(M_UNITS);
            DS_HIP(ds_memcpy_async(dunits, units.data(), sizeof(i64) * (size_t)n, hipMemcpyHostToDevice, st));
            DS_HIP(ds_memset_async(dflags, 0, sizeof(unsigned int) * (size_t)n, st));
            for (i64 k = 0; k < map->nf; ++k) {
                DS_HIP(ds_memset_async(mlayer(M_CNT), 0, sizeof(double) * (size_t)n, st));
                DS_CHECK(launch_sl_frame_pos(mlayer(M_DX), mlayer(M_DY), dunits, ny, nx, hx, hy, map->taus[k], mlayer(M_X),
                                             mlayer(M_Y), dflags, st));
                DS_CHECK(launch_deposit(dim1, ny, nx, ny, n, mlayer(M_X), mlayer(M_Y), dunits, (unsigned long long *)mlayer(M_CNT), st));
                if (map->counts) {
                    DS_HIP(ds_memcpy_async(map->counts + n * k, mlayer(M_CNT), sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
                } else {
                    DS_CHECK(launch_sl_frame(mlayer(M_CNT), n, unit, st));
                    DS_HIP(ds_memcpy_async(map->frames + n * k, mlayer(M_CNT), sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
                }
            }
            DS_CHECK(launch_advect_count(dflags, n, dmcounts + 1, st));
        }
        DS_HIP(ds_memcpy_async(msums, dmsums, sizeof msums, hipMemcpyDeviceToHost, st));
        DS_HIP(ds_memcpy_async(mcounts, dmcounts, sizeof mcounts, hipMemcpyDeviceToHost, st));
        double *mwant[5] = {map->Dx, map->Dy, map->C, map->row, map->spread};
        const int mhave[5] = {M_DX, M_DY, M_C, M_ROW, M_SPREAD};
        for (int k = 0; k < 5; ++k)
            if (mwant[k]) DS_HIP(ds_memcpy_async(mwant[k], mlayer(mhave[k]), sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    }
    // the arrays the caller asked for: nothing can be refused any more
    double *want[5] = {f, g, E, er, ec};
    const double *have[5] = {F, G, Ed, layer(L_ER), layer(L_EC)};
    for (int k = 0; k < 5; ++k)
        if (want[k]) DS_HIP(ds_memcpy_async(want[k], have[k], sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    DS_HIP(ds_stream_synchronize(st));
    if (defects)
        for (i64 k = 0; k < o->max_sweeps; ++k) defects[k] = k < sweeps ? defect[(size_t)k] : NAN;
    memset(res, 0, sizeof *res);
    res->n_nodes = n;
    res->sweeps = sweeps;
    res->zero0 = (i64)counts[SC_ZERO0];
    res->zero1 = (i64)counts[SC_ZERO1];
    res->nonfinite = (i64)counts[SC_NONFINITE];
    res->eps = eps;
    res->mass0 = m0;
    res->mass1 = m1;
    const double R0s = sums[SS_R0], C0s = sums[SS_C0], fill = R0s < C0s ? R0s : C0s;
    res->kept = sums[SS_KEPT];
    res->cost_kept = sums[SS_COST];
    res->fill = fill;
    res->cost_fill = fill > 0.0 ? 0.5 * ((sums[SS_R2] * C0s + R0s * sums[SS_C2]) -
                                         2.0 * (sums[SS_R1X] * sums[SS_C1X] + sums[SS_R1Y] * sums[SS_C1Y])) / fill
                                : 0.0;
    res->upper = 2.0 * (res->cost_kept + res->cost_fill);
    res->defect_first = sweeps ? defect.front() : NAN;
    res->defect_last = sweeps ? defect.back() : NAN;
    if (map) {
        dotsocp_plan_map_t *m = map->res;
        memset(m, 0, sizeof *m);
        m->rows = msums[SP_ROWS];
        m->map_cost = msums[SP_MAP];
        m->spread = msums[SP_SPREAD];
        m->cost_rows = 2.0 * msums[SP_COST];
        m->disp_mean = msums[SP_DISP];
        memcpy(&m->disp_max, &mcounts[0], sizeof(double));
        m->n_clamped = (i64)mcounts[1];
        m->unit = unit;
    }
    return 0;
}

int upper_check_dims(i64 ny, i64 nx, bool dim1) {
    DS_ARG(ny >= 2 && (dim1 || nx >= 2), "the upper bound needs two nodes along every axis");
    DS_ARG(ny <= HL_MAX_LEN && nx <= HL_MAX_LEN && ny * nx <= INT_MAX, "the upper bound serves axes of up to 2^20 nodes and layers of up to 2^31 - 1");
    return 0;
}

// the stateless call's device and scratch: released, and the caller's device restored, on every path
struct PlanCall {
    int prev = -1;
    bool switched = false;
    std::vector<double *> bufs;
    ~PlanCall() {
        if (!bufs.empty()) (void)hipDeviceSynchronize();
        for (double *b : bufs) dfree(b);
        if (switched && prev >= 0) (void)hipSetDevice(prev);
    }
    int enter(int device) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
            set_error("no HIP device available (libdotsocp has no CPU fallback)");
            return DOTSOCP_ENODEVICE;
        }
        DS_ARG(device >= 0 && device < n, "device ordinal out of range");
        (void)hipGetDevice(&prev);
        DS_HIP(hipSetDevice(device));
        switched = true;
        (void)hipGetLastError();
        return 0;
    }
    int alloc(double **p, i64 n, bool fp = true) { DS_CHECK(dmalloc(p, n, fp)); bufs.push_back(*p); return 0; }
};

int canary_now() {
    if (!canary_enabled()) return 0;
    std::string what;
    const int bad = canary_check(&what);
    if (bad) set_error("canary: %d device buffer(s) written out of bounds: %s", bad, what.c_str());
    return bad ? DOTSOCP_EHIP : 0;
}

}  // namespace

int plan_bound(const double *rho0, const double *rho1, i64 ny, i64 nx, const double *f_start, const dotsocp_upper_opts *o,
               dotsocp_upper *res, double *f, double *g, double *E, double *er, double *ec, double *defects, int device) {
    DS_ARG(rho0 != nullptr && rho1 != nullptr && res != nullptr, "plan_bound() needs rho0, rho1 and res (one of them is NULL)");
    DS_CHECK(upper_check_opts(o, f_start, true));
    const bool dim1 = ny == 1;
    const i64 iy = dim1 ? nx : ny, ix = dim1 ? 1 : nx;          // a line lives along y, as in a 1-D context
    DS_CHECK(upper_check_dims(iy, ix, dim1));
    PlanCall c;
    DS_CHECK(c.enter(device));
    dotsocp_upper got;
    DS_CHECK(upper_engine(c, UpperRun{nullptr, nullptr}, iy, ix, dim1, rho0, rho1, o->start, nullptr, f_start, o, &got, f, g, E,
                          er, ec, defects));
    DS_CHECK(canary_now());                     // the kernels wrote inside their buffers
    *res = got;
    return 0;
}

int plan_map(const double *rho0, const double *rho1, i64 ny, i64 nx, const double *f_start, const dotsocp_upper_opts *o,
             dotsocp_upper *res, double *f, double *g, double *E, double *er, double *ec, double *defects,
             dotsocp_plan_map_t *map_res, double *Dx, double *Dy, double *C, double *row, double *spread, const double *taus,
             i64 nf, double *frames, int device) {
    DS_ARG(rho0 != nullptr && rho1 != nullptr && res != nullptr, "plan_map() needs rho0, rho1 and res (one of them is NULL)");
    DS_CHECK(map_check_frames(map_res, nf, taus, frames));
    for (i64 k = 0; k < nf; ++k)
        DS_ARG(std::isfinite(taus[k]) && taus[k] >= 0.0 && taus[k] <= 1.0, "plan map: every tau is finite and in [0, 1]");
    DS_CHECK(upper_check_opts(o, f_start, true));
    const bool dim1 = ny == 1;
    const i64 iy = dim1 ? nx : ny, ix = dim1 ? 1 : nx;          // a line lives along y, as in a 1-D context
    DS_CHECK(upper_check_dims(iy, ix, dim1));
    PlanCall c;
    DS_CHECK(c.enter(device));
    dotsocp_upper got;
    dotsocp_plan_map_t mgot;
    const MapRequest rq{&mgot, dim1 ? nullptr : Dx, dim1 ? Dx : Dy, C, row, spread, taus, nf, frames, nullptr};
    DS_CHECK(upper_engine(c, UpperRun{nullptr, nullptr}, iy, ix, dim1, rho0, rho1, o->start, nullptr, f_start, o, &got, f, g, E,
                          er, ec, defects, &rq));
    DS_CHECK(canary_now());                     // the kernels wrote inside their buffers
    *res = got;
    *map_res = mgot;
    return 0;
}

namespace {

// what dotsocp_upper_map adds to dotsocp_upper_bound (nullptr: the bound alone)
struct CtxMap {
    dotsocp_plan_map_t *res;
    double *Dx, *Dy, *C, *row, *spread;
    const i64 *nodes;
    i64 nf;
    double *frames, *l1;
};

#define CTX_ARG(cond, msg) do { if (!(cond)) { set_error(msg, who); return DOTSOCP_EINVAL; } } while (0)

int ctx_upper(Solver &S, const char *who, const double *rho0, const double *rho1, const double *f_start, const dotsocp_upper_opts *o,
              dotsocp_upper *res, double *f, double *g, double *E, double *er, double *ec, double *defects, const CtxMap *m) {
    CTX_ARG(rho0 != nullptr && rho1 != nullptr && res != nullptr, "%s() needs rho0, rho1 and res (one of them is NULL)");
    CTX_ARG(!S.remote(), "%s() serves the slabs of one process; contexts with an RCCL communicator are not served");
    CTX_ARG(!S.prob.weighted, "%s(): the cost of a weighted context is not the Euclidean one, its bound is not provided");
    if (!S.finished) { set_error("%s() needs finish()", who); return DOTSOCP_ESTATE; }
    DS_CHECK(upper_check_opts(o, f_start, false));
    const bool dim1 = S.prob.dim == 1;
    const i64 ny = S.ny, nx = S.nx, n = ny * nx;
    DS_CHECK(upper_check_dims(ny, nx, dim1));
    std::vector<double> taus, l1_host;
    std::vector<i64> cnt;
    if (m) {
        DS_CHECK(map_check_frames(m->res, m->nf, m->nodes, m->frames));
        for (i64 k = 0; k < m->nf; ++k) {
            DS_ARG(m->nodes[k] >= 0 && m->nodes[k] < S.nt, "plan map: a frame node lies outside [0, nt)");
            taus.push_back((double)m->nodes[k] / (double)(S.nt - 1));
        }
        if (m->nf > 0) DS_CHECK(S.need_beta_form(who));
        cnt.resize((size_t)(n * m->nf));
        l1_host.resize((size_t)m->nf);
    }
    S.cur_dev = -1;
    DS_CHECK(S.use_dev(S.device));
    Slab &s0 = S.slabs.front();
    DeviceScratch scratch(S);
    DS_CHECK(S.use(s0));
    hipStream_t st = s0.st;
    double *start = nullptr;
    if (o->start == 1) {
        // phi(t = 0) in original units (recoverOrgVar: one product per entry), out of the slab's pitched rows
        const i64 plane = s0.g.plane, py = s0.g.py;
        double *tmp = nullptr;
        DS_CHECK(scratch.alloc(&tmp, plane));
        DS_CHECK(scratch.alloc(&start, n));
        DS_CHECK(launch_hl_layer(s0.phi, tmp, plane, S.dScale, st));
        DS_HIP(ds_memcpy2d_async(start, sizeof(double) * (size_t)ny, tmp, sizeof(double) * (size_t)py, sizeof(double) * (size_t)ny,
                                 (size_t)nx, hipMemcpyDeviceToDevice, st));
    }
    dotsocp_upper got;
    dotsocp_plan_map_t mgot;
    MapRequest rq{};
    if (m) rq = MapRequest{&mgot, dim1 ? nullptr : m->Dx, dim1 ? m->Dx : m->Dy, m->C, m->row, m->spread, taus.data(), m->nf, nullptr, cnt.data()};
    DS_CHECK(upper_engine(scratch, UpperRun{&S, st}, ny, nx, dim1, rho0, rho1, o->start, start, f_start, o, &got, f, g, E, er,
                          ec, defects, m ? &rq : nullptr));
    if (m && m->nf > 0) {
        // every counts plane travels through the host to the slab that owns the frame's time node: there rho of that node is
        // formed, the plane becomes the frame and l1 is summed -- kernel and order of dotsocp_push_mass
        DS_CHECK(S.stage_left_tail());
        for (auto &s : S.slabs) DS_CHECK(S.stage_rho_ends(s, rho0, rho1));
        const i64 plane = s0.g.plane, tiles = report_tiles(s0.g);
        std::vector<double *> F(S.slabs.size(), nullptr);
        for (i64 k = 0; k < m->nf; ++k) {
            size_t own = 0;
            while (own + 1 < S.slabs.size() && m->nodes[k] >= S.slabs[own].g.t0 + S.slabs[own].g.ntl) ++own;
            Slab &s = S.slabs[own];
            const Grid &sg = s.g;
            DS_CHECK(S.use(s));
            if (!F[own]) {
                DS_CHECK(scratch.alloc(&F[own], plane + tiles + m->nf, false));     // the plane holds integers first
                DS_CHECK(poison_region(F[own] + plane, sizeof(double) * (size_t)(tiles + m->nf)));
                DS_HIP(ds_memset_async(F[own], 0, sizeof(double) * (size_t)plane, s.st));
            }
            DS_CHECK(S.copy_rows(F[own], (double *)(cnt.data() + n * k), ny, sg.py, nx, true, s.st));
            DS_CHECK(launch_frame_l1(sg, s.alpha, s.weight, s.w1, s.w1 + plane, s.a0_prev, S.sigma, S.cScale * S.D, m->nodes[k] - sg.t0,
                                     mgot.unit, F[own], F[own] + plane, F[own] + plane + tiles + k, s.st));
            DS_CHECK(S.copy_rows(F[own], m->frames + n * k, ny, sg.py, nx, false, s.st));
            DS_HIP(ds_memcpy_async(&l1_host[(size_t)k], F[own] + plane + tiles + k, sizeof(double), hipMemcpyDeviceToHost, s.st));
        }
    }
    DS_CHECK(S.sync_all());
    DS_CHECK(S.prof_flush());
    DS_CHECK(S.canary_after());                 // the kernels wrote inside their buffers
    *res = got;
    if (m) {
        *m->res = mgot;
        for (i64 k = 0; m->l1 && k < m->nf; ++k) m->l1[k] = l1_host[(size_t)k] / (double)n;
    }
    return 0;
}

}  // namespace

int Solver::upper_bound(const double *rho0, const double *rho1, const double *f_start, const dotsocp_upper_opts *o,
                        dotsocp_upper *res, double *f, double *g, double *E, double *er, double *ec, double *defects) {
    return ctx_upper(*this, "upper_bound", rho0, rho1, f_start, o, res, f, g, E, er, ec, defects, nullptr);
}

int Solver::upper_map(const double *rho0, const double *rho1, const double *f_start, const dotsocp_upper_opts *o, dotsocp_upper *res,
                      double *f, double *g, double *E, double *er, double *ec, double *defects, dotsocp_plan_map_t *map_res,
                      double *Dx, double *Dy, double *C, double *row, double *spread, const i64 *frame_nodes, i64 nf, double *frames,
                      double *l1) {
    const CtxMap m{map_res, Dx, Dy, C, row, spread, frame_nodes, nf, frames, l1};
    return ctx_upper(*this, "upper_map", rho0, rho1, f_start, o, res, f, g, E, er, ec, defects, &m);
}

}  // namespace dotsocp
