// extern "C" surface of libdotsocp (include/dotsocp.h).
#include <cstring>
#include <new>

#include "comm.h"
#include "image_table.h"
#include "solver.h"
#include "weights.h"

using namespace dotsocp;

namespace dotsocp {
extern thread_local std::string g_last_error;
int dotsocp_slab_range_impl(i64 nt, int world, int rank, i64 *t0, i64 *t1);
}

struct dotsocp_ctx {
    Solver s;
};

struct dotsocp_weights {
    Weights w;
};

static int require_device() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error("no HIP device available (libdotsocp has no CPU fallback)");
        return DOTSOCP_ENODEVICE;
    }
    return 0;
}

// RAII device buffer for the host-pointer operator entry points (through the device block cache of guard.hip: a MATLAB
// loop over mexBFd / mexProjSoc gets the same buffers back call after call instead of a malloc / free pair per call)
struct DevBuf {
    double *p = nullptr;
    ~DevBuf() { dfree(p); }
    int alloc(i64 n) { return dmalloc(&p, n); }
};

extern "C" {

const char *dotsocp_last_error(void) { return g_last_error.c_str(); }
const char *dotsocp_version(void) { return "dotsocp-mi355x 0.1 (gfx950)"; }

int dotsocp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------ B2, device pointers
int dotsocp_proj_soc_dev(double *d_out, const double *d_in, dotsocp_i64 M, dotsocp_i64 K, void *stream) {
    DS_ARG(M >= 0 && K >= 2, "mexProjSoc needs an M x K matrix with K >= 2");
    DS_ARG(d_out && d_in, "NULL pointer");
    return launch_proj_soc(d_out, d_in, M, K, (hipStream_t)stream);
}

static int make_grid(Grid &g, i64 nt, i64 nx, i64 ny) {
    DS_ARG(nt >= 2 && nx >= 1 && ny >= 1, "need nt >= 2, nx >= 1, ny >= 1");
    g.set(ny, nx, nt, 0, nt);
    return 0;
}

int dotsocp_bfd_dev(double *d_z, const double *d_q, dotsocp_i64 nt, dotsocp_i64 nx, dotsocp_i64 ny, double scale,
                    double dF, void *stream) {
    Grid g;
    DS_CHECK(make_grid(g, nt, nx, ny));
    DS_ARG(d_z && d_q, "NULL pointer");
    return launch_bfd(g, d_z, d_q, scale, dF, (hipStream_t)stream);
}

int dotsocp_bfd_conj_dev(double *d_q, const double *d_z, dotsocp_i64 nt, dotsocp_i64 nx, dotsocp_i64 ny,
                         double scale, void *stream) {
    Grid g;
    DS_CHECK(make_grid(g, nt, nx, ny));
    DS_ARG(d_z && d_q, "NULL pointer");
    return launch_bfd_conj(g, d_q, d_z, scale, (hipStream_t)stream);
}

// ------------------------------------------------------------------ B2, host pointers
int dotsocp_proj_soc(double *out, const double *in, dotsocp_i64 M, dotsocp_i64 K) {
    DS_ARG(M >= 0 && K >= 2, "mexProjSoc needs an M x K matrix with K >= 2");
    if (M == 0) return 0;                      // empty matrix (mxGetPr may be NULL): nothing to do, like the reference
    DS_ARG(out && in, "NULL pointer");
    DS_CHECK(require_device());
    DevBuf a, b;
    DS_CHECK(a.alloc(M * K));
    DS_CHECK(b.alloc(M * K));
    DS_HIP(hipMemcpy(a.p, in, sizeof(double) * M * K, hipMemcpyHostToDevice));
    DS_CHECK(launch_proj_soc(b.p, a.p, M, K, nullptr));
    DS_HIP(hipDeviceSynchronize());
    DS_HIP(hipMemcpy(out, b.p, sizeof(double) * M * K, hipMemcpyDeviceToHost));
    return 0;
}

int dotsocp_bfd(double *z, const double *q, dotsocp_i64 nt, dotsocp_i64 nx, dotsocp_i64 ny, double scale,
                double dF) {
    Grid g;
    DS_CHECK(make_grid(g, nt, nx, ny));
    DS_ARG(z && q, "NULL pointer");
    DS_CHECK(require_device());
    DevBuf dz, dq;
    DS_CHECK(dz.alloc(10 * g.Nz));
    DS_CHECK(dq.alloc(g.NqAlloc));
    // in-place semantics: slots that mexBFd does not write keep the caller's values
    DS_HIP(hipMemcpy(dz.p, z, sizeof(double) * 10 * g.Nz, hipMemcpyHostToDevice));
    DS_HIP(hipMemcpy(dq.p, q, sizeof(double) * g.NqAlloc, hipMemcpyHostToDevice));
    DS_CHECK(launch_bfd(g, dz.p, dq.p, scale, dF, nullptr));
    DS_HIP(hipDeviceSynchronize());
    DS_HIP(hipMemcpy(z, dz.p, sizeof(double) * 10 * g.Nz, hipMemcpyDeviceToHost));
    return 0;
}

int dotsocp_bfd_conj(double *q, const double *z, dotsocp_i64 nt, dotsocp_i64 nx, dotsocp_i64 ny, double scale) {
    Grid g;
    DS_CHECK(make_grid(g, nt, nx, ny));
    DS_ARG(z && q, "NULL pointer");
    DS_CHECK(require_device());
    DevBuf dz, dq;
    DS_CHECK(dz.alloc(10 * g.Nz));
    DS_CHECK(dq.alloc(g.NqAlloc));
    DS_HIP(hipMemcpy(dz.p, z, sizeof(double) * 10 * g.Nz, hipMemcpyHostToDevice));
    DS_CHECK(launch_bfd_conj(g, dq.p, dz.p, scale, nullptr));
    DS_HIP(hipDeviceSynchronize());
    DS_HIP(hipMemcpy(q, dq.p, sizeof(double) * g.NqAlloc, hipMemcpyDeviceToHost));
    return 0;
}

// 1-D operators: the 1-D grid nx x nt is the 2-D grid with ny = nx1d, nx = 1 (no bx edges);
// cone columns [1 | bx(x-,t) bx(x+,t) bx(x-,t+1) bx(x+,t+1) | 6] live in planes {0, 5,6,7,8, 9}.
static const int k1dCols[6] = {0, 5, 6, 7, 8, 9};

int dotsocp_bfd1d(double *z, const double *q, dotsocp_i64 nt, dotsocp_i64 nx, double scale, double dF) {
    Grid g;
    DS_CHECK(make_grid(g, nt, 1, nx));
    DS_ARG(z && q, "NULL pointer");
    DS_CHECK(require_device());
    DevBuf dz, dq;
    DS_CHECK(dz.alloc(10 * g.Nz));
    DS_CHECK(dq.alloc(g.NqAlloc));
    for (int j = 0; j < 6; ++j)
        DS_HIP(hipMemcpy(dz.p + k1dCols[j] * g.Nz, z + j * g.Nz, sizeof(double) * g.Nz, hipMemcpyHostToDevice));
    DS_HIP(hipMemcpy(dq.p, q, sizeof(double) * g.NqAlloc, hipMemcpyHostToDevice));
    DS_CHECK(launch_bfd(g, dz.p, dq.p, scale, dF, nullptr));
    DS_HIP(hipDeviceSynchronize());
    for (int j = 0; j < 6; ++j)
        DS_HIP(hipMemcpy(z + j * g.Nz, dz.p + k1dCols[j] * g.Nz, sizeof(double) * g.Nz, hipMemcpyDeviceToHost));
    return 0;
}

int dotsocp_bfd_conj1d(double *q, const double *z, dotsocp_i64 nt, dotsocp_i64 nx, double scale) {
    Grid g;
    DS_CHECK(make_grid(g, nt, 1, nx));
    DS_ARG(z && q, "NULL pointer");
    DS_CHECK(require_device());
    DevBuf dz, dq;
    DS_CHECK(dz.alloc(10 * g.Nz));
    DS_CHECK(dq.alloc(g.NqAlloc));
    DS_HIP(hipMemset(dz.p, 0, sizeof(double) * 10 * g.Nz));
    for (int j = 0; j < 6; ++j)
        DS_HIP(hipMemcpy(dz.p + k1dCols[j] * g.Nz, z + j * g.Nz, sizeof(double) * g.Nz, hipMemcpyHostToDevice));
    DS_CHECK(launch_bfd_conj(g, dq.p, dz.p, scale, nullptr));
    DS_HIP(hipDeviceSynchronize());
    DS_HIP(hipMemcpy(q, dq.p, sizeof(double) * g.NqAlloc, hipMemcpyDeviceToHost));
    return 0;
}

static int dctn_dev(double *a, double *b, i64 ny, i64 nx, i64 nt, int inverse, DctPlan *py, DctPlan *px, DctPlan *pt) {
    // forward: y, x, t ; inverse: t, x, y (separable, any order gives the same transform).
    // result ends in `b`.
    if (!inverse) {
        DS_CHECK(launch_dct_axis(py, a, b, ny, nx, nt, 0, 0, nullptr));
        DS_CHECK(launch_dct_axis(px, b, a, ny, nx, nt, 1, 0, nullptr));
        DS_CHECK(launch_dct_axis(pt, a, b, ny, nx, nt, 2, 0, nullptr));
    } else {
        DS_CHECK(launch_dct_axis(pt, a, b, ny, nx, nt, 2, 1, nullptr));
        DS_CHECK(launch_dct_axis(px, b, a, ny, nx, nt, 1, 1, nullptr));
        DS_CHECK(launch_dct_axis(py, a, b, ny, nx, nt, 0, 1, nullptr));
    }
    return 0;
}

struct Plans {
    DctPlan *py = nullptr, *px = nullptr, *pt = nullptr;
    ~Plans() { dct_plan_destroy(py); dct_plan_destroy(px); dct_plan_destroy(pt); }
    int make(i64 ny, i64 nx, i64 nt) {
        DS_CHECK(dct_length_check(ny)); DS_CHECK(dct_length_check(nx)); DS_CHECK(dct_length_check(nt));
        py = dct_plan_create(ny); px = dct_plan_create(nx); pt = dct_plan_create(nt);
        if (!py || !px || !pt) { set_error("DCT plan allocation failed"); return DOTSOCP_EHIP; }
        return 0;
    }
};

int dotsocp_dctn(double *a, dotsocp_i64 ny, dotsocp_i64 nx, dotsocp_i64 nt, int inverse) {
    DS_ARG(a && ny >= 1 && nx >= 1 && nt >= 1, "bad array");
    DS_CHECK(dct_length_check(ny)); DS_CHECK(dct_length_check(nx)); DS_CHECK(dct_length_check(nt));
    DS_CHECK(require_device());
    const i64 n = ny * nx * nt;
    DevBuf da, db;
    Plans pl;
    DS_CHECK(da.alloc(n));
    DS_CHECK(db.alloc(n));
    DS_CHECK(pl.make(ny, nx, nt));
    DS_HIP(hipMemcpy(da.p, a, sizeof(double) * n, hipMemcpyHostToDevice));
    DS_CHECK(dctn_dev(da.p, db.p, ny, nx, nt, inverse, pl.py, pl.px, pl.pt));
    DS_HIP(hipDeviceSynchronize());
    DS_HIP(hipMemcpy(a, db.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    return 0;
}

// Test support: the one pass of dotsocp_dctn along `axis` -- its length checks, its plan for that length, its source
// and destination buffers (dctn_dev: y and t go a -> b, x goes b -> a, in both directions).
int dotsocp_dct_axis(double *a, dotsocp_i64 ny, dotsocp_i64 nx, dotsocp_i64 nt, int axis, int inverse) {
    DS_ARG(a && ny >= 1 && nx >= 1 && nt >= 1, "bad array");
    DS_ARG(axis >= 0 && axis <= 2, "axis must be 0 (y), 1 (x) or 2 (t)");
    DS_CHECK(dct_length_check(ny)); DS_CHECK(dct_length_check(nx)); DS_CHECK(dct_length_check(nt));
    DS_CHECK(require_device());
    const i64 n = ny * nx * nt;
    DevBuf da, db;
    Plans pl;
    DS_CHECK(da.alloc(n));
    DS_CHECK(db.alloc(n));
    DS_CHECK(pl.make(ny, nx, nt));
    DctPlan *plan = axis == 0 ? pl.py : axis == 1 ? pl.px : pl.pt;
    double *src = axis == 1 ? db.p : da.p, *dst = axis == 1 ? da.p : db.p;
    DS_HIP(hipMemcpy(src, a, sizeof(double) * n, hipMemcpyHostToDevice));
    DS_CHECK(launch_dct_axis(plan, src, dst, ny, nx, nt, axis, inverse ? 1 : 0, nullptr));
    DS_HIP(hipDeviceSynchronize());
    DS_HIP(hipMemcpy(a, dst, sizeof(double) * n, hipMemcpyDeviceToHost));
    return 0;
}

int dotsocp_oper_poisson(double *res, const double *rhs, dotsocp_i64 ny, dotsocp_i64 nx, dotsocp_i64 nt,
                         double kernelScale) {
    DS_ARG(res && rhs && ny >= 1 && nx >= 1 && nt >= 1, "bad array");
    DS_CHECK(dct_length_check(ny)); DS_CHECK(dct_length_check(nx)); DS_CHECK(dct_length_check(nt));
    DS_CHECK(require_device());
    const i64 n = ny * nx * nt;
    DevBuf da, db, cy, cx, ct;
    Plans pl;
    DS_CHECK(da.alloc(n));
    DS_CHECK(db.alloc(n));
    DS_CHECK(pl.make(ny, nx, nt));
    const double pi = 3.14159265358979323846;
    auto table = [&](DevBuf &d, i64 m) -> int {
        std::vector<double> t((size_t)m);
        for (i64 k = 0; k < m; ++k) t[k] = (2.0 * (double)(m - 1) * (double)(m - 1)) * (1.0 - cos(pi * (double)k / (double)m));
        DS_CHECK(d.alloc(m));
        DS_HIP(hipMemcpy(d.p, t.data(), sizeof(double) * m, hipMemcpyHostToDevice));
        return 0;
    };
    DS_CHECK(table(cy, ny));
    DS_CHECK(table(cx, nx));
    DS_CHECK(table(ct, nt));
    DS_HIP(hipMemcpy(da.p, rhs, sizeof(double) * n, hipMemcpyHostToDevice));
    // y, x forward, the t step in place (unpitched rows), x, y inverse
    Grid g;
    g.set(ny, nx, nt, 0, nt);
    DS_CHECK(launch_dct_axis(pl.py, da.p, db.p, ny, nx, nt, 0, 0, nullptr));
    DS_CHECK(launch_dct_axis(pl.px, db.p, da.p, ny, nx, nt, 1, 0, nullptr));
    DS_CHECK(launch_poisson_t_single(pl.pt, g, kernelScale, cy.p, cx.p, ct.p, da.p, db.p, 0, nullptr, tsolve_tri_allowed()));
    DS_CHECK(launch_dct_axis(pl.px, da.p, db.p, ny, nx, nt, 1, 1, nullptr));
    DS_CHECK(launch_dct_axis(pl.py, db.p, da.p, ny, nx, nt, 0, 1, nullptr));
    DS_HIP(hipDeviceSynchronize());
    DS_HIP(hipMemcpy(res, da.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------ B1
dotsocp_ctx *dotsocp_create(const dotsocp_problem *prob, int device, int nslabs) {
    dotsocp_ctx *c = new (std::nothrow) dotsocp_ctx();
    if (!c) { set_error("out of host memory"); return nullptr; }
    if (c->s.init(prob, device, nslabs) != 0) {
        delete c;
        return nullptr;
    }
    return c;
}

dotsocp_ctx *dotsocp_create_multi(const dotsocp_problem *prob, int first_device, int ngpu) {
    dotsocp_ctx *c = new (std::nothrow) dotsocp_ctx();
    if (!c) { set_error("out of host memory"); return nullptr; }
    if (c->s.init(prob, first_device, ngpu, true) != 0) {
        delete c;
        return nullptr;
    }
    return c;
}

void dotsocp_destroy(dotsocp_ctx *ctx) { delete ctx; }

int dotsocp_slab_range(dotsocp_i64 nt, int world, int rank, dotsocp_i64 *t0, dotsocp_i64 *t1) {
    DS_ARG(t0 && t1 && world >= 1 && rank >= 0 && rank < world && nt >= 2 * world, "bad slab request");
    return dotsocp_slab_range_impl(nt, world, rank, t0, t1);
}

int dotsocp_rccl_unique_id(unsigned char id[128]) {
    DS_ARG(id != nullptr, "id is NULL");
    Rccl &api = rccl_api();
    DS_CHECK(api.load());
    ncclUniqueId uid;
    static_assert(sizeof(uid) == 128, "ncclUniqueId is expected to be 128 bytes");
    DS_NCCL(api.GetUniqueId(&uid));
    memcpy(id, &uid, sizeof uid);
    return 0;
}

int dotsocp_attach_rccl(dotsocp_ctx *ctx, const unsigned char id[128], int rank, int world) {
    if (!ctx) { set_error("ctx is NULL"); return DOTSOCP_EINVAL; }
    return ctx->s.attach_rccl(id, rank, world);
}

#define CTX_OR_FAIL()                                      \
    do {                                                   \
        if (!ctx) { set_error("ctx is NULL"); return DOTSOCP_EINVAL; } \
        (void)hipGetLastError();   /* a stale error of an earlier, failed call must not be blamed on this one */ \
    } while (0)

int dotsocp_dct_algorithm(dotsocp_i64 n) { return dct_choose_algorithm(n); }
int dotsocp_dct_levels(dotsocp_i64 n, int axis) { return dct_levels(n, axis); }
int dotsocp_cdft_levels(dotsocp_i64 n) { return cdft_levels(n); }
int dotsocp_tsolve_tri_safe(dotsocp_i64 ny, dotsocp_i64 nx, dotsocp_i64 nt) { return tsolve_tri_safe(ny, nx, nt) ? 1 : 0; }

int dotsocp_dct_pass_kernel(int device, dotsocp_i64 ny, dotsocp_i64 nx, dotsocp_i64 nt, dotsocp_i64 pitch, int axis) {
    DS_ARG(ny >= 1 && nx >= 1 && nt >= 1 && axis >= 0 && axis <= 2 && device >= 0, "bad pass request");
    return dct_pass_kind(ny, nx, nt, axis, pitch, device_cus_of(device));
}
int dotsocp_tsolve_kernel(int device, dotsocp_i64 ny, dotsocp_i64 nx, dotsocp_i64 nt, dotsocp_i64 pitch) {
    DS_ARG(ny >= 1 && nx >= 1 && nt >= 2 && device >= 0, "bad t-solve request");
    return poisson_t_kind(ny, nx, nt, pitch, tsolve_tri_allowed(), device_cus_of(device));
}
dotsocp_i64 dotsocp_row_pitch(dotsocp_i64 ny) { return default_row_pitch(ny); }

int dotsocp_cone_writes_beta(dotsocp_i64 it, double last_sigma_it, dotsocp_i64 maxit, int check_step_by_step,
                             int ends_run, int rescale, double maxFeas, double relGap) {
    return cone_writes_beta(SchedState{it, maxit, last_sigma_it, check_step_by_step != 0, rescale, maxFeas, relGap, ends_run ? 1 : -1}) ? 1 : 0;
}
int dotsocp_rescale_due(dotsocp_i64 it, int rescale, double maxFeas, double relGap) {
    return rescale_due(it, rescale, maxFeas, relGap) ? 1 : 0;
}
int dotsocp_qcone_form(dotsocp_i64 it, double last_sigma_it, dotsocp_i64 maxit, int check_step_by_step, int ends_run,
                       int next_ends_run, int rescale, double maxFeas, double relGap) {
    const long long run_left = ends_run ? 1 : (next_ends_run ? 2 : -1);
    return qcone_form(SchedState{it, maxit, last_sigma_it, check_step_by_step != 0, rescale, maxFeas, relGap, run_left});
}

dotsocp_i64 dotsocp_field_len(const dotsocp_problem *p, int field) {
    if (!p || (p->dim != 1 && p->dim != 2) || p->nt < 2 || p->nx < 1 || (p->dim == 2 && p->ny < 1)) return -1;
    const i64 ny = p->dim == 1 ? p->nx : p->ny, nx = p->dim == 1 ? 1 : p->nx, nt = p->nt;
    const i64 Nphi = ny * nx * nt, Nz = ny * nx * (nt - 1);
    const i64 Nq = Nz + ny * (nx - 1) * nt + (ny - 1) * nx * nt;
    switch (field) {
        case DOTSOCP_F_PHI: case DOTSOCP_F_C: return Nphi;
        case DOTSOCP_F_Q: case DOTSOCP_F_ALPHA: case DOTSOCP_F_WEIGHT: return Nq;
        case DOTSOCP_F_Z: case DOTSOCP_F_BETA: return Nz * (p->dim == 1 ? 6 : 10);
        default: return -1;
    }
}

int dotsocp_upload(dotsocp_ctx *ctx, int field, const double *host) { CTX_OR_FAIL(); return ctx->s.upload(field, host); }
dotsocp_i64 dotsocp_release_cache(void) { return (dotsocp_i64)device_cache_release(); }

int dotsocp_upload_layers(dotsocp_ctx *ctx, int field, const double *host, dotsocp_i64 t0, dotsocp_i64 n) {
    CTX_OR_FAIL();
    return ctx->s.upload_layers(field, host, t0, n);
}
int dotsocp_download(dotsocp_ctx *ctx, int field, double *host) { CTX_OR_FAIL(); return ctx->s.download(field, host); }
int dotsocp_begin(dotsocp_ctx *ctx, const dotsocp_opts *opts) { CTX_OR_FAIL(); return ctx->s.begin(opts); }
int dotsocp_begin_method(dotsocp_ctx *ctx, const dotsocp_opts *opts, int method, const dotsocp_acc_opts *acc) {
    CTX_OR_FAIL();
    return ctx->s.begin_method(opts, method, acc);
}
int dotsocp_recover_outputs(dotsocp_ctx *ctx, const double *rho0, const double *rho1, double *rho, double *Ex,
                            double *Ey, double *q0, double *bx, double *by) {
    CTX_OR_FAIL();
    if (ctx->s.prob.dim == 1)     // 1-D problems live in the y slot of the engine (ny = nx1d, nx = 1)
        return ctx->s.recover_outputs(rho0, rho1, rho, nullptr, Ex, q0, nullptr, bx);
    return ctx->s.recover_outputs(rho0, rho1, rho, Ex, Ey, q0, bx, by);
}

int dotsocp_report_edges(double edges[DOTSOCP_REPORT_BINS + 1]) {
    if (!edges) { set_error("invalid argument: report_edges() needs an array of %d doubles", DOTSOCP_REPORT_BINS + 1); return DOTSOCP_EINVAL; }
    report_edges_host(edges);
    return 0;
}

int dotsocp_solution_report(dotsocp_ctx *ctx, const double *rho0, const double *rho1, dotsocp_report *rep, double *layer_mass,
                            double *layer_neg) {
    CTX_OR_FAIL();
    return ctx->s.solution_report(rho0, rho1, rep, layer_mass, layer_neg);
}

int dotsocp_geodesic_profile(dotsocp_ctx *ctx, const double *rho0, const double *rho1, dotsocp_geodesic *res, double *sums,
                             double *rho_max, dotsocp_i64 *n_support) {
    CTX_OR_FAIL();
    return ctx->s.geodesic_profile(rho0, rho1, res, sums, rho_max, n_support);
}

int dotsocp_recover_velocity(dotsocp_ctx *ctx, const double *rho0, const double *rho1, double rho_floor, double *vx, double *vy) {
    CTX_OR_FAIL();
    if (ctx->s.prob.dim == 1)     // 1-D problems live in the y slot of the engine (ny = nx1d, nx = 1)
        return ctx->s.recover_velocity(rho0, rho1, rho_floor, nullptr, vx);
    return ctx->s.recover_velocity(rho0, rho1, rho_floor, vx, vy);
}

int dotsocp_advect_particles(dotsocp_ctx *ctx, const double *rho0, const double *rho1, const dotsocp_advect_opts *o, double *x,
                             double *y, double *traj_x, double *traj_y, dotsocp_i64 *n_clamped) {
    CTX_OR_FAIL();
    if (ctx->s.prob.dim == 1)
        return ctx->s.advect_particles(rho0, rho1, o, nullptr, x, nullptr, traj_x, n_clamped);
    return ctx->s.advect_particles(rho0, rho1, o, x, y, traj_x, traj_y, n_clamped);
}

int dotsocp_push_mass(dotsocp_ctx *ctx, const double *rho0, const double *rho1, const dotsocp_push_opts *o, double *x, double *y,
                      const double *mass, const dotsocp_i64 *frame_nodes, double *frames, dotsocp_i64 *n_clamped, double *unit,
                      double *l1) {
    CTX_OR_FAIL();
    if (ctx->s.prob.dim == 1)
        return ctx->s.push_mass(rho0, rho1, o, nullptr, x, mass, frame_nodes, frames, n_clamped, unit, l1);
    return ctx->s.push_mass(rho0, rho1, o, x, y, mass, frame_nodes, frames, n_clamped, unit, l1);
}

int dotsocp_map_report(dotsocp_ctx *ctx, const double *rho0, const double *rho1, const dotsocp_advect_opts *o, double *x, double *y,
                       const double *mass, dotsocp_map_report_t *rep, double *disp, double *len, double *action) {
    CTX_OR_FAIL();
    if (ctx->s.prob.dim == 1)
        return ctx->s.map_report(rho0, rho1, o, nullptr, x, mass, rep, disp, len, action);
    return ctx->s.map_report(rho0, rho1, o, x, y, mass, rep, disp, len, action);
}

int dotsocp_dual_bound(dotsocp_ctx *ctx, const double *rho0, const double *rho1, dotsocp_dual *res, double *H, double *B,
                       int *arg_fwd, int *arg_bwd) {
    CTX_OR_FAIL();
    return ctx->s.dual_bound(rho0, rho1, res, H, B, arg_fwd, arg_bwd);
}

int dotsocp_plan_bound(const double *rho0, const double *rho1, dotsocp_i64 ny, dotsocp_i64 nx, const double *f_start,
                       const dotsocp_upper_opts *o, dotsocp_upper *res, double *f, double *g, double *E, double *er, double *ec,
                       double *defects, int device) {
    return plan_bound(rho0, rho1, ny, nx, f_start, o, res, f, g, E, er, ec, defects, device);
}

int dotsocp_plan_map(const double *rho0, const double *rho1, dotsocp_i64 ny, dotsocp_i64 nx, const double *f_start,
                     const dotsocp_upper_opts *o, dotsocp_upper *res, double *f, double *g, double *E, double *er, double *ec,
                     double *defects, dotsocp_plan_map_t *map_res, double *Dx, double *Dy, double *C, double *row, double *spread,
                     const double *taus, dotsocp_i64 nf, double *frames, int device) {
    return plan_map(rho0, rho1, ny, nx, f_start, o, res, f, g, E, er, ec, defects, map_res, Dx, Dy, C, row, spread, taus, nf,
                    frames, device);
}

int dotsocp_upper_bound(dotsocp_ctx *ctx, const double *rho0, const double *rho1, const double *f_start,
                        const dotsocp_upper_opts *o, dotsocp_upper *res, double *f, double *g, double *E, double *er, double *ec,
                        double *defects) {
    CTX_OR_FAIL();
    return ctx->s.upper_bound(rho0, rho1, f_start, o, res, f, g, E, er, ec, defects);
}

int dotsocp_upper_map(dotsocp_ctx *ctx, const double *rho0, const double *rho1, const double *f_start, const dotsocp_upper_opts *o,
                      dotsocp_upper *res, double *f, double *g, double *E, double *er, double *ec, double *defects,
                      dotsocp_plan_map_t *map_res, double *Dx, double *Dy, double *C, double *row, double *spread,
                      const dotsocp_i64 *frame_nodes, dotsocp_i64 nf, double *frames, double *l1) {
    CTX_OR_FAIL();
    return ctx->s.upper_map(rho0, rho1, f_start, o, res, f, g, E, er, ec, defects, map_res, Dx, Dy, C, row, spread, frame_nodes, nf,
                            frames, l1);
}

int dotsocp_render_evolution(dotsocp_ctx *ctx, const double *rho0, const double *rho1, const dotsocp_render_opts *opts,
                             const dotsocp_i64 *frame_nodes, const double *levels, const unsigned char *lut,
                             const unsigned char *barrier, unsigned char *image, double *mvx, double *mvy,
                             dotsocp_render_info *info) {
    CTX_OR_FAIL();
    if (ctx->s.prob.dim != 1 || !opts)
        return ctx->s.render_evolution(rho0, rho1, opts, frame_nodes, levels, lut, barrier, image, mvx, mvy, info);
    // 1-D problems live in the y slot of the engine: the stride along the axis and the one component go there
    dotsocp_render_opts o = *opts;
    if (o.skip_y >= 1 && o.skip_x >= 1) { o.skip_y = o.skip_x; o.skip_x = 1; }
    dotsocp_render_info got{};
    const int rc = ctx->s.render_evolution(rho0, rho1, &o, frame_nodes, levels, lut, barrier, image, nullptr, mvx, &got);
    if (rc == 0 && info) {
        *info = got;
        info->mx = got.my;
        info->my = got.my > 0 ? 1 : 0;
    }
    return rc;
}

int dotsocp_jump_next_level(dotsocp_ctx *coarse, dotsocp_ctx *fine) {
    if (!coarse || !fine) { set_error("context is NULL"); return DOTSOCP_EINVAL; }
    return fine->s.jump_from(coarse->s);
}

int dotsocp_run(dotsocp_ctx *ctx, dotsocp_i64 n_iters, dotsocp_i64 *done) { CTX_OR_FAIL(); return ctx->s.run(n_iters, done); }
int dotsocp_finish(dotsocp_ctx *ctx, dotsocp_result *res) { CTX_OR_FAIL(); return ctx->s.finish(res); }

int dotsocp_get_history(dotsocp_ctx *ctx, double *kkt, double *time, double *iter, double *pdGap) {
    CTX_OR_FAIL();
    const Solver &s = ctx->s;
    const size_t n = s.hist_iter.size();
    for (size_t i = 0; i < n; ++i) {
        if (kkt) for (int j = 0; j < 7; ++j) kkt[j * n + i] = s.hist_kkt[i * 7 + j];   // len x 7, column-major
        if (time) time[i] = s.hist_time[i];
        if (iter) iter[i] = s.hist_iter[i];
        if (pdGap) pdGap[i] = s.hist_gap[i];
    }
    return 0;
}

int dotsocp_set_profiling(dotsocp_ctx *ctx, int on) {
    CTX_OR_FAIL();
    ctx->s.profiling = on != 0;
    return 0;
}

int dotsocp_kernel_time(dotsocp_ctx *ctx, const char *name, double *avg_ms, dotsocp_i64 *launches) {
    CTX_OR_FAIL();
    DS_ARG(name != nullptr, "name is NULL");
    static const char *names[PH_COUNT] = {"rhs", "poisson", "cone_proj", "qstep", "beta", "kkt",
                                          "cone_fused_a", "cone_fused_b", "materialise", "comm",
                                          "interp", "acc_cone", "acc_gather", "qstep_first", "transpose", "cone_carry", "qcone",
                                          "velocity_layer", "advect", "deposit", "frame_l1", "advect_path", "map_final",
                                          "hl_pass_x", "hl_pass_y", "hl_reduce", "sl_pass_x", "sl_pass_y", "sl_node"};
    for (int i = 0; i < PH_COUNT; ++i)
        if (strcmp(name, names[i]) == 0) {
            const i64 n = ctx->s.phase_launches[i];
            if (avg_ms) *avg_ms = n ? ctx->s.phase_ms[i] / (double)n : 0.0;
            if (launches) *launches = n;
            return 0;
        }
    set_error("unknown kernel family '%s'", name);
    return DOTSOCP_EINVAL;
}

// test hooks of the allocator (guard.hip): what n doubles from dmalloc hold as they are handed out -- no kernel of the
// library runs on them; the bytes the device block cache holds on one device (device < 0: on all)
int dotsocp_debug_alloc_peek(dotsocp_i64 n, double *out) {
    DS_ARG(n >= 1 && out != nullptr, "debug_alloc_peek() needs n >= 1 and an array of n doubles");
    DS_CHECK(require_device());
    DevBuf d;
    DS_CHECK(d.alloc(n));
    DS_HIP(hipMemcpy(out, d.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

dotsocp_i64 dotsocp_debug_cache_held(int device) { return (dotsocp_i64)device_cache_held(device); }

int dotsocp_canary_check(void) {
    std::string rep;
    const int bad = canary_check(&rep);
    if (bad) set_error("canary: %d device buffer(s) written out of bounds: %s", bad, rep.c_str());
    return bad;
}

// ------------------------------------------------------------------ weight pyramid (weights.hip)
#define WEIGHTS_OR_FAIL()                                  \
    do {                                                   \
        if (!w) { set_error("weight pyramid is NULL"); return DOTSOCP_EINVAL; } \
        (void)hipGetLastError();                           \
    } while (0)

dotsocp_weights *dotsocp_weights_create(int device, dotsocp_i64 ny, dotsocp_i64 nx, dotsocp_i64 nt, int levels) {
    dotsocp_weights *w = new (std::nothrow) dotsocp_weights();
    if (!w) { set_error("out of host memory"); return nullptr; }
    if (w->w.init(device, ny, nx, nt, levels) != 0) {
        delete w;
        return nullptr;
    }
    return w;
}

void dotsocp_weights_destroy(dotsocp_weights *w) { delete w; }

dotsocp_i64 dotsocp_weights_len(dotsocp_i64 ny, dotsocp_i64 nx, dotsocp_i64 nt, int levels, int level) {
    return weights_level_len(ny, nx, nt, levels, level);
}

int dotsocp_weights_set(dotsocp_weights *w, const double *weight) { WEIGHTS_OR_FAIL(); return w->w.set(weight); }
int dotsocp_weights_set_space(dotsocp_weights *w, const double *weightX, const double *weightY) {
    WEIGHTS_OR_FAIL();
    return w->w.set_space(weightX, weightY);
}
int dotsocp_weights_restrict(dotsocp_weights *w, int log_mean) { WEIGHTS_OR_FAIL(); return w->w.restrict_all(log_mean); }
int dotsocp_weights_log10_mean(dotsocp_weights *w, int level, double *mean) { WEIGHTS_OR_FAIL(); return w->w.log10_mean(level, mean); }
int dotsocp_weights_download(dotsocp_weights *w, int level, double *host) { WEIGHTS_OR_FAIL(); return w->w.download(level, host); }

int dotsocp_upload_weight_from(dotsocp_ctx *ctx, dotsocp_weights *w, int level) {
    CTX_OR_FAIL();
    WEIGHTS_OR_FAIL();
    const Weights::Level *L = nullptr;
    DS_CHECK(w->w.level_for_upload(level, &L));
    return ctx->s.upload_weight_from(L->w, w->w.device, L->ny, L->nx, L->nt);
}

// ------------------------------------------------------------------ pictures (image.hip, image_table.h)
int dotsocp_imresize_taps(dotsocp_i64 n_in, dotsocp_i64 n_out) {
    DS_ARG(imresize_lengths_ok(n_in, n_out), "imresize: lengths must lie in 1 .. 65536");
    return imresize_max_taps(n_in, n_out);
}

int dotsocp_imresize_table(dotsocp_i64 n_in, dotsocp_i64 n_out, double *weights, int *indices, int *taps) {
    DS_ARG(imresize_lengths_ok(n_in, n_out), "imresize: lengths must lie in 1 .. 65536");
    DS_ARG(weights && indices && taps, "NULL pointer");
    imresize_table(n_in, n_out, weights, indices, taps);
    return 0;
}

int dotsocp_imresize(void *out, const void *in, int dtype, dotsocp_i64 h_in, dotsocp_i64 w_in, dotsocp_i64 planes,
                     dotsocp_i64 h_out, dotsocp_i64 w_out, int device) {
    return image_resize(out, in, dtype, h_in, w_in, planes, h_out, w_out, device);
}

int dotsocp_image_density(const dotsocp_image_opts *o, const dotsocp_image *imgs, int nimg, double *rho, int device) {
    return image_density(o, imgs, nimg, rho, device);
}

int dotsocp_poisson_phi(dotsocp_ctx *ctx) { CTX_OR_FAIL(); return ctx->s.poisson_phi(); }

int dotsocp_synchronize(dotsocp_ctx *ctx) {
    CTX_OR_FAIL();
    ctx->s.cur_dev = -1;
    return ctx->s.sync_all();
}

}  // extern "C"
