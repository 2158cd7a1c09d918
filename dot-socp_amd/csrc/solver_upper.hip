// The upper bound on W2^2 (include/dotsocp.h: dotsocp_plan_bound, dotsocp_upper_bound; kernels: softlax.hip).  One engine
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

// Scratch: alloc(double **, i64, bool fp).  Layers ny x nx unpitched, y fastest (a line: ny nodes, nx = 1).  rho0, rho1 and
// the outputs are host arrays; the start: mode 0 none, 1 the negative of d_start (device, unpitched), 2 h_start (host).
template <class Scratch>
int upper_engine(Scratch &scratch, const UpperRun &run, i64 ny, i64 nx, bool dim1, const double *rho0, const double *rho1,
                 int mode, const double *d_start, const double *h_start, const dotsocp_upper_opts *o, dotsocp_upper *res,
                 double *f, double *g, double *E, double *er, double *ec, double *defects) {
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
    DS_CHECK(transform(IN, V2, MEAN));                          // f^
    SlFinalArgs fa{A, B, F, V2, G, V, Ed, layer(L_ER), layer(L_EC), ny, nx, hx, hy, ieps, partials};
    double sums[SS_COUNT] = {0};
    run.begin(PH_SL_NODE);
    DS_CHECK(node(launch_sl_final(fa, dsums, st)));
    DS_HIP(ds_memcpy_async(sums, dsums, sizeof sums, hipMemcpyDeviceToHost, st));
    DS_HIP(ds_memcpy_async(counts, dcounts, sizeof counts, hipMemcpyDeviceToHost, st));
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

int Solver::upper_bound(const double *rho0, const double *rho1, const double *f_start, const dotsocp_upper_opts *o,
                        dotsocp_upper *res, double *f, double *g, double *E, double *er, double *ec, double *defects) {
    DS_ARG(rho0 != nullptr && rho1 != nullptr && res != nullptr, "upper_bound() needs rho0, rho1 and res (one of them is NULL)");
    DS_ARG(!remote(), "upper_bound() serves the slabs of one process; contexts with an RCCL communicator are not served");
    DS_ARG(!prob.weighted, "upper_bound(): the cost of a weighted context is not the Euclidean one, its bound is not provided");
    if (!finished) { set_error("upper_bound() needs finish()"); return DOTSOCP_ESTATE; }
    DS_CHECK(upper_check_opts(o, f_start, false));
    const bool dim1 = prob.dim == 1;
    DS_CHECK(upper_check_dims(ny, nx, dim1));
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    Slab &s0 = slabs.front();
    DeviceScratch scratch(*this);
    DS_CHECK(use(s0));
    hipStream_t st = s0.st;
    double *start = nullptr;
    if (o->start == 1) {
        // phi(t = 0) in original units (recoverOrgVar: one product per entry), out of the slab's pitched rows
        const i64 plane = s0.g.plane, py = s0.g.py;
        double *tmp = nullptr;
        DS_CHECK(scratch.alloc(&tmp, plane));
        DS_CHECK(scratch.alloc(&start, ny * nx));
        DS_CHECK(launch_hl_layer(s0.phi, tmp, plane, dScale, st));
        DS_HIP(ds_memcpy2d_async(start, sizeof(double) * (size_t)ny, tmp, sizeof(double) * (size_t)py, sizeof(double) * (size_t)ny,
                                 (size_t)nx, hipMemcpyDeviceToDevice, st));
    }
    dotsocp_upper got;
    DS_CHECK(upper_engine(scratch, UpperRun{this, st}, ny, nx, dim1, rho0, rho1, o->start, start, f_start, o, &got, f, g, E, er,
                          ec, defects));
    DS_CHECK(sync_all());
    DS_CHECK(prof_flush());
    DS_CHECK(canary_after());                   // the kernels wrote inside their buffers
    *res = got;
    return 0;
}

}  // namespace dotsocp
