// Devices, streams and slabs of a Solver: error text, device selection, per-device plans and tables, slab placement
// and allocation (every device buffer of a slab is owned by the slab: Slab::alloc / zalloc, freed by free_slabs), the RCCL attach.
#include "solver.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "comm.h"

namespace dotsocp {

thread_local std::string g_last_error;

static int make_eig_table(double **dev, i64 n, i64 len = 0);

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

int Solver::use_dev(int d) {
    if (cur_dev == d) return 0;
    DS_HIP(hipSetDevice(d));
    cur_dev = d;
    return 0;
}

int Solver::use(const Slab &s) {
    DS_CHECK(use_dev(s.dev));
    if (stream_stress_enabled() && begun && !finished) {       // race detector: perturb the relative timing of the streams
        if (s.st) stream_stress(s.st);
        if (s.st_z) stream_stress(s.st_z);
    }
    return 0;
}

int Solver::sync_all() {
    for (auto &s : slabs) {
        DS_CHECK(use(s));
        if (s.st_z) DS_HIP(ds_stream_synchronize(s.st_z));
        if (s.st) DS_HIP(ds_stream_synchronize(s.st));
    }
    if (slabs.empty() && stream) {
        DS_CHECK(use_dev(device));
        DS_HIP(ds_stream_synchronize(stream));
    }
    return 0;
}


DevRes *Solver::res_for(int dev) {
    for (auto *r : devres)
        if (r->dev == dev) return r;
    if (use_dev(dev) != 0) return nullptr;
    DevRes *r = new DevRes();
    r->dev = dev;
    r->py = dct_plan_create(ny);
    r->px = dct_plan_create(nx);
    r->pt = dct_plan_create(nt);
    // (cy as long as a pitched row: the t-solves of a time-slab context treat the pad entries of a row as modes of their own)
    if (!r->py || !r->px || !r->pt || make_eig_table(&r->cy, ny, row_pitch()) != 0 || make_eig_table(&r->cx, nx) != 0 ||
        make_eig_table(&r->ct, nt) != 0) {
        set_error("DCT plan allocation failed on device %d", dev);
        dct_plan_destroy(r->py); dct_plan_destroy(r->px); dct_plan_destroy(r->pt);
        dfree(r->cy); dfree(r->cx); dfree(r->ct);
        delete r;
        return nullptr;
    }
    devres.push_back(r);
    return r;
}

void Solver::free_slabs() {
    defer.reset();                   // joins the slab threads (their queues are empty outside run())
    for (auto &s : slabs) {
        (void)use(s);
        if (s.st_z) (void)ds_stream_synchronize(s.st_z);
        if (s.st) (void)ds_stream_synchronize(s.st);
        for (auto &e : s.ev) if (e) (void)hipEventDestroy(e);
        if (s.st != stream) {        // slab 0 borrows the solver's own streams
            if (s.st_z) (void)hipStreamDestroy(s.st_z);
            if (s.st) (void)hipStreamDestroy(s.st);
        }
        if (s.h_sums) (void)hipHostFree(s.h_sums);
        for (void *p : s.owned) dfree(p);
    }
    slabs.clear();
}

Solver::~Solver() {
    cur_dev = -1;
    if (stream) (void)sync_all();   // init() got as far as the device: release what lives there
    if (stream && canary_enabled()) {
        std::string rep;
        const int bad = canary_check(&rep);
        cur_dev = -1;
        if (bad) fprintf(stderr, "libdotsocp: canary: %d device buffer(s) written out of bounds: %s\n", bad, rep.c_str());
    }
    if (nccl) (void)rccl_api().CommDestroy((ncclComm_t)nccl);
    free_slabs();
    for (auto *r : devres) {
        (void)use_dev(r->dev);
        dct_plan_destroy(r->py); dct_plan_destroy(r->px); dct_plan_destroy(r->pt);
        dfree(r->cy); dfree(r->cx); dfree(r->ct);
        delete r;
    }
    devres.clear();
    (void)use_dev(device);
    dfree(d_red);
    if (h_sums) (void)hipHostFree(h_sums);
    for (auto &p : pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto e : event_pool) (void)hipEventDestroy(e);
    if (stream_z) (void)hipStreamDestroy(stream_z);
    if (stream) (void)hipStreamDestroy(stream);
}

static int make_eig_table(double **dev, i64 n, i64 len) {
    // (2 (n-1)^2) (1 - cos(pi k / n))   -- initialize_FFTkernel.m:6-8; entries n .. len-1 (pads of a pitched row, whose data
    // are zeros) repeat the last one: any positive number keeps their systems regular
    if (len < n) len = n;
    std::vector<double> t((size_t)len);
    const double pi = 3.14159265358979323846;
    for (i64 k = 0; k < n; ++k) t[k] = (2.0 * (double)(n - 1) * (double)(n - 1)) * (1.0 - cos(pi * (double)k / (double)n));
    for (i64 k = n; k < len; ++k) t[k] = (n > 1) ? t[n - 1] : 1.0;
    DS_CHECK(dmalloc(dev, len));
    DS_HIP(hipMemcpy(*dev, t.data(), sizeof(double) * len, hipMemcpyHostToDevice));
    return 0;
}

int dotsocp_slab_range_impl(i64 nt, int world, int rank, i64 *t0, i64 *t1) {
    // nodes are dealt as evenly as possible; the last slab owns one cell layer fewer than nodes
    const i64 base = nt / world, rem = nt % world;
    const i64 a = rank * base + std::min<i64>(rank, rem);
    const i64 b = a + base + (rank < rem ? 1 : 0);
    *t0 = a;
    *t1 = b;
    return 0;
}

// pencil j of `world`: columns [l0, l1) of the ny*nx (y, x) columns, boundaries on even columns
void pencil_range(i64 plane, int world, int j, i64 *l0, i64 *l1) {
    auto cut = [&](int k) -> i64 { return (k >= world) ? plane : 2 * ((plane / 2) * k / world); };
    *l0 = cut(j);
    *l1 = cut(j + 1);
}

// The second stream of a slab carries its messages and the small kernels between them (solver.h: comm_z): highest
// priority, so that their workgroups are placed ahead of the queued workgroups of the bulk kernel on the main stream
static int make_second_stream(hipStream_t *st) {
    int least = 0, greatest = 0;
    DS_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    DS_HIP(hipStreamCreateWithPriority(st, hipStreamNonBlocking, greatest));
    return 0;
}

int Solver::init(const dotsocp_problem *p, int dev, int nslabs, bool multi_dev) {
    DS_ARG(p != nullptr, "prob is NULL");
    DS_ARG(p->dim == 1 || p->dim == 2, "prob.dim must be 1 or 2");
    DS_ARG(p->nt >= 2 && p->nx >= 1, "grid too small");
    prob = *p;
    device = dev;
    if (p->dim == 1) { ny = p->nx; nx = 1; } else { ny = p->ny; nx = p->nx; }
    nt = p->nt;
    DS_ARG(ny >= 1 && nx >= 1, "grid too small");
    DS_ARG(nslabs >= 1 && nslabs <= nt / 2, "nslabs must be in [1, nt/2]");
    DS_CHECK(dct_length_check(ny)); DS_CHECK(dct_length_check(nx)); DS_CHECK(dct_length_check(nt));
    if (const char *e = getenv("DOTSOCP_FUSED")) fused = (atoi(e) != 0);
    if (nslabs > 1 && !fused) {
        set_error("time slabs need the fused dataflow (unset DOTSOCP_FUSED=0)");
        return DOTSOCP_EINVAL;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available (libdotsocp has no CPU fallback)");
        return DOTSOCP_ENODEVICE;
    }
    DS_ARG(dev >= 0 && dev < ndev, "device ordinal out of range");
    ndev_visible = ndev;
    multi_device = multi_dev && nslabs > 1;
    cur_dev = -1;
    DS_CHECK(use_dev(dev));
    DS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    DS_CHECK(make_second_stream(&stream_z));
    overlap = nslabs > 1;                         // pays when there is communication to hide
    if (const char *e = getenv("DOTSOCP_OVERLAP")) overlap = (atoi(e) != 0);
    if (const char *e = getenv("DOTSOCP_KKT_FOLD")) kkt_fold = (atoi(e) != 0);
    if (const char *e = getenv("DOTSOCP_NORM_CACHE")) norm_cache = (atoi(e) != 0);
    tri_tsolve = tsolve_tri_allowed();
    DS_HIP(hipHostMalloc((void **)&h_sums, sizeof(double) * (S_COUNT + 1)));
    DS_CHECK(dmalloc(&d_red, S_COUNT + 1));
    if (!res_for(dev)) return DOTSOCP_EHIP;
    world = nslabs;
    rank = 0;
    // device arrays are allocated on first use (upload / begin) or by attach_rccl(), so that a process
    // that is about to become one rank of many never allocates the whole grid
    return 0;
}

int Solver::ensure_alloc() {
    if (!slabs.empty()) return 0;
    DS_CHECK(alloc_slabs(remote() ? rank : 0, remote() ? 1 : world));
    DS_CHECK(sync_all());
    return 0;
}

// Row pitch of the device arrays (common.h: Grid::py).  The single slab of a one-GPU context stores rows whose length is
// no multiple of 16 doubles -- the 2^k+1 grids of the reference's multilevel driver -- padded to the next multiple of
// 128 bytes; time-slab contexts keep the reference layout (their messages and the partitioned t-solve index the
// (y, x) columns of a layer linearly).  DOTSOCP_PITCH=0: never.
// pad between the ten columns of z and beta (common.h: Grid::Nc)
i64 Solver::column_pad() const { return (ny * nx >= 4096) ? 48 : 0; }

i64 Solver::row_pitch() const { return default_row_pitch(ny); }

i64 default_row_pitch(i64 ny) {
    static const bool on = !(getenv("DOTSOCP_PITCH") && atoi(getenv("DOTSOCP_PITCH")) == 0);
    if (!on || ny <= 16) return ny;
    if (ny % 16 == 0) {
        // Rows whose length in bytes is a multiple of 2 KB: the x lines of the Poisson solve (one 64-byte piece per row, rows a
        // power of two apart) keep hitting the same DRAM banks -- with rows 128 bytes longer the x passes of the pipelined DCT
        // kernels take 0.41 / 0.47 instead of 0.50 / 0.52 ms at 1024 x 1024 x 128 (rocprofv3, same box).  DOTSOCP_PITCH2=0: off.
        const char *e = getenv("DOTSOCP_PITCH2");
        const bool on2 = !(e && atoi(e) == 0);
        return (on2 && ny >= 512 && ny % 256 == 0) ? ny + 16 : ny;
    }
    return (ny + 15) / 16 * 16;
}

int Solver::alloc_slabs(int first, int count) {
    free_slabs();
    peer_ok = true;
    cross_device = false;
    comm_z = overlap && world > 1 && fused;      // messages on the second streams (solver.h)
    comm_depth = 0;
    comm_async = false;
    slabs.resize(count);
    const i64 plane = row_pitch() * nx;          // doubles per layer as stored (Grid::plane)
    for (int r = 0; r < count; ++r) {
        Slab &s = slabs[r];
        s.index = first + r;
        // placement: dotsocp_create_multi deals the slabs round-robin over the visible devices, starting at `device`
        s.dev = (multi_device && !remote()) ? (device + r) % ndev_visible : device;
        DS_CHECK(use(s));
        // dotsocp_create(.., nslabs): all slabs on ONE device share its pair of streams -- their kernels would only compete
        // for the same HBM (8 slabs of 1024 x 1024 x 16 on concurrent streams: 15.8 ms per iteration, one after the other
        // 8 x 1.63); dotsocp_create_multi gives every slab its own pair, whichever device it lands on
        if (r == 0 || !multi_device) {
            s.st = stream; s.st_z = stream_z;
        } else {
            DS_HIP(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));
            DS_CHECK(make_second_stream(&s.st_z));
        }
        for (auto &e : s.ev) DS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        DS_HIP(hipHostMalloc((void **)&s.h_sums, sizeof(double) * S_COUNT));
        s.res = res_for(s.dev);
        if (!s.res) return DOTSOCP_EHIP;
        i64 t0, t1;
        dotsocp_slab_range_impl(nt, world, s.index, &t0, &t1);
        s.g.set(ny, nx, nt, t0, t1 - t0, row_pitch(), column_pad());
        const Grid &g = s.g;
        DS_CHECK(s.zalloc(&s.phi, g.NphiAlloc));
        DS_CHECK(s.zalloc(&s.q, g.NqAlloc));
        DS_CHECK(s.zalloc(&s.alpha, g.NqAlloc));
        DS_CHECK(s.zalloc(&s.z, 10 * g.Nc));
        DS_CHECK(s.zalloc(&s.beta, 10 * g.Nc));
        DS_CHECK(s.zalloc(&s.c, g.Nphi));
        // pitched rows: the pad entries are never written by the tile kernels, so they are zeroed once here -- the few
        // kernels that stream over whole arrays (scalings, sums of squares) then leave them zero / add nothing
        if (g.py > g.ny) {
            DS_CHECK(s.zalloc(&s.w0, g.Nphi));
            DS_CHECK(s.zalloc(&s.w1, g.Nphi));
        } else {
            DS_CHECK(s.alloc(&s.w0, g.Nphi));
            DS_CHECK(s.alloc(&s.w1, g.Nphi));
        }
        if (prob.weighted) {
            DS_CHECK(s.alloc(&s.weight, g.NqAlloc));
            DS_CHECK(launch_fill(s.weight, g.NqAlloc, 1.0, s.st));      // pad entries of a weight are ones (x ./ w stays finite)
        }
        if (fused) {
            fused_geometry(g, s.fg);
            DS_CHECK(s.zalloc(&s.q_old, g.NqAlloc));
            DS_CHECK(s.zalloc(&s.q2, g.NqAlloc));
            if (g.py > g.ny || g.Nc > g.Nz) DS_CHECK(s.zalloc(&s.beta2, 10 * g.Nc));
            else DS_CHECK(s.alloc(&s.beta2, 10 * g.Nc));
            DS_CHECK(s.zalloc(&s.sx, s.fg.sx_len));
            DS_CHECK(s.zalloc(&s.sy, s.fg.sy_len));
            DS_CHECK(s.zalloc(&s.alpha2, g.NqAlloc));
        }
        s.kw.maxBlocks = kkt_partials_needed(g);
        DS_CHECK(s.zalloc(&s.kw.partials, s.kw.maxBlocks * S_COUNT));
        DS_CHECK(s.alloc(&s.kw.sums, S_COUNT * (1 + KKT_SLICES)));
        pencil_range(plane, world, s.index, &s.l0, &s.nl);
        s.nl -= s.l0;
        if (multi()) {
            DS_CHECK(s.alloc(&s.pencil, s.nl * nt));
            DS_CHECK(s.alloc(&s.pencil2, s.nl * nt));
            DS_CHECK(s.alloc(&s.stage, g.Nphi));
            if (fused) DS_CHECK(s.zalloc(&s.carry, 4 * g.plane));
            if (!g.first) {
                DS_CHECK(s.zalloc(&s.u0_prev, plane));
                DS_CHECK(s.zalloc(&s.a0_prev, plane));
                DS_CHECK(s.zalloc(&s.a0w_prev, plane));
                DS_CHECK(s.zalloc(&s.tail_bx, g.bxLayer));
                DS_CHECK(s.zalloc(&s.btail_bx, g.bxLayer));
                DS_CHECK(s.zalloc(&s.tail_by, g.byLayer));
                DS_CHECK(s.zalloc(&s.btail_by, g.byLayer));
            }
            if (!g.last) {
                DS_CHECK(s.zalloc(&s.send_plane, plane));
                DS_CHECK(s.zalloc(&s.send_plane2, plane));
                DS_CHECK(s.zalloc(&s.send_bx, g.bxLayer));
                DS_CHECK(s.zalloc(&s.send_by, g.byLayer));
            }
        }
    }
    // neighbours on different devices copy layers into each other's memory
    for (auto &a : slabs)
        for (auto &b : slabs) {
            if (a.dev == b.dev) continue;
            cross_device = true;
            DS_CHECK(use(a));
            hipError_t e = hipDeviceEnablePeerAccess(b.dev, 0);
            // a refusal is not fatal: hipMemcpyPeerAsync stages through the host without peer access -- but the launches
            // that PULL messages through peer pointers (flush_msgs, tri_exchange) must then stay off
            if (e != hipSuccess) {
                (void)hipGetLastError();
                if (e != hipErrorPeerAccessAlreadyEnabled) peer_ok = false;
            }
        }
    // several slabs with their own streams in this process (dotsocp_create_multi): one issuing thread per slab (defer.h) --
    // OPT-IN (DOTSOCP_HOST_THREADS=1) until a box with several devices has shown both bit-equal results and a gain: the one
    // configuration that could be measured, all slabs on one device, is slower with the threads (8 slabs on 64^3: 1.26 vs
    // 1.06-1.17 ms per iteration -- they contend for the one submission queue and add hand-off latency)
    {
        const char *e = getenv("DOTSOCP_HOST_THREADS");
        const bool want = e && atoi(e) != 0;
        if (want && count > 1 && !remote() && multi_device) {
            defer.reset(new DeferCtx());
            for (auto &s : slabs) {
                const int w = defer->add_worker(s.dev);
                defer->map_stream(s.st, w);
                defer->map_stream(s.st_z, w);
            }
        }
    }
    return 0;
}

int Solver::attach_rccl(const unsigned char *id, int rk, int wd) {
    DS_ARG(id != nullptr, "unique id is NULL");
    DS_ARG(wd >= 1 && rk >= 0 && rk < wd, "bad rank / world");
    DS_ARG(wd <= DS_MAX_WORLD, "at most 64 slabs");
    DS_ARG(wd <= nt / 2, "world must not exceed nt/2 time slabs");
    if (begun || world != 1 || !slabs.empty()) {
        set_error("attach_rccl() must directly follow create(..., nslabs = 1)");
        return DOTSOCP_ESTATE;
    }
    if (!fused) { set_error("time slabs need the fused dataflow (unset DOTSOCP_FUSED=0)"); return DOTSOCP_EINVAL; }
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    Rccl &api = rccl_api();
    DS_CHECK(api.load());
    ncclUniqueId uid;
    static_assert(sizeof(uid) == 128, "ncclUniqueId is expected to be 128 bytes");
    memcpy(&uid, id, sizeof uid);
    ncclComm_t comm = nullptr;
    DS_NCCL(api.CommInitRank(&comm, wd, uid, rk));
    nccl = comm;
    world = wd;
    rank = rk;
    if (!getenv("DOTSOCP_OVERLAP")) overlap = wd > 1;
    DS_CHECK(ensure_alloc());
    DS_HIP(ds_stream_synchronize(stream));
    if (wd > 1) {
        // handshake: the communicator spans `wd` ranks and the neighbours are the ranks this slab expects (also opens
        // the neighbour connections before the first timed iteration)
        // (on the stream that carries every later message of this communicator: RCCL sees ONE stream)
        const hipStream_t cs = comm_z ? stream_z : stream;
        double h[4] = {1.0, (double)rk, 0.0, -1.0};
        double *d = nullptr;
        DS_CHECK(dmalloc(&d, 4));
        DS_HIP(ds_memcpy_async(d, h, sizeof h, hipMemcpyHostToDevice, cs));
        DS_NCCL(api.AllReduce(d, d + 2, 1, ncclDouble, ncclSum, comm, cs));
        DS_NCCL(api.GroupStart());
        ++open_groups;
        if (rk + 1 < wd) DS_NCCL_G(api.Send(d + 1, 1, ncclDouble, rk + 1, comm, cs));
        if (rk > 0) DS_NCCL_G(api.Recv(d + 3, 1, ncclDouble, rk - 1, comm, cs));
        --open_groups;
        DS_NCCL(api.GroupEnd());
        DS_HIP(ds_memcpy_async(h, d, sizeof h, hipMemcpyDeviceToHost, cs));
        DS_HIP(ds_stream_synchronize(cs));
        dfree(d);
        if (h[2] != (double)wd || (rk > 0 && h[3] != (double)(rk - 1))) {
            set_error("RCCL handshake failed: %g ranks answered (expected %d), left neighbour says %g (expected %d)", h[2], wd,
                      h[3], rk - 1);
            return DOTSOCP_ECOMM;
        }
    }
    return 0;
}

}  // namespace dotsocp
