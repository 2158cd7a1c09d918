// Device-resident inPALM/ALG2 loop state (B1 boundary of include/dotsocp.h).
#pragma once
#include <chrono>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "hostmem.h"
#include "kernels.h"
#include "schedule.h"

namespace dotsocp {

// Device allocations of the solver state go through guard.hip: with DOTSOCP_CANARY=1 in the environment every buffer
// gets a guard band of NaN-pattern words on both sides, checked by canary_check() (finish(), destroy()) -- an
// out-of-bounds WRITE of a tile kernel on a partial tile changes a guard word, an out-of-bounds READ pulls NaNs
// into the iterates.  Without the variable freed buffers are kept in a per-device cache and handed out again (guard.hip;
// DOTSOCP_DEVICE_CACHE=0: plain hipMalloc / hipFree).
//
// DOTSOCP_POISON=1 (read per call; a switch for tests): a payload that holds floating-point numbers (`fp`) is handed out
// filled with POISON_WORD, a quiet NaN, instead of the zeros that fresh or reused device memory usually shows -- a kernel
// that reads a slot nothing has written yet then changes its results (tests/test_gpu_poison.py).  Payloads of integers
// (indices, counters, flags) are never poisoned: a poisoned word read as an index would be a wild address.
constexpr unsigned long long POISON_WORD = 0x7ff8bad0bad0bad0ull;
int guarded_malloc(void **p, size_t bytes, bool fp = false);
void guarded_free(void *p);
bool poison_enabled();
// fills a floating-point region of a buffer that was allocated unpoisoned because it also holds integers (no-op unless
// DOTSOCP_POISON=1); synchronises like guarded_malloc
int poison_region(void *p, size_t bytes);
// the device block cache behind them (guard.hip): hipFree everything it holds; returns the bytes given back
long long device_cache_release();
// bytes the cache holds on device `dev` (dev < 0: on all devices)
long long device_cache_held(int dev);
// number of live buffers whose guard bands were overwritten (0 when the canaries are off); `report` receives a
// description of the first few.  Synchronises the current device.
int canary_check(std::string *report);
bool canary_enabled();
// DOTSOCP_STRESS_STREAMS=1: random stalls in front of the work of every slab stream (guard.hip)
bool stream_stress_enabled();
void stream_stress(hipStream_t st);

template <class T> struct is_fp_payload { static constexpr bool value = std::is_floating_point<T>::value; };
template <> struct is_fp_payload<double2> { static constexpr bool value = true; };

template <class T>
inline int dmalloc(T **p, i64 n, bool fp = is_fp_payload<T>::value) {
    *p = nullptr;
    if (n <= 0) n = 1;
    return guarded_malloc((void **)p, sizeof(T) * (size_t)n, fp);
}

inline void dfree(void *p) {
    if (p) guarded_free(p);
}

// Resources that live once per HIP device and are shared by the slabs placed on it.
struct DevRes {
    int dev = 0;
    DctPlan *py = nullptr, *px = nullptr, *pt = nullptr;
    double *cy = nullptr, *cx = nullptr, *ct = nullptr;   // DCT eigenvalue tables
};

// One time slab (common.h: Grid).  Single-GPU runs have exactly one; `nslabs` > 1 keeps several in
// one process -- every slab with its own device (dotsocp_create_multi: slab r on device (first + r) mod #devices;
// dotsocp_create: all on one device), its own pair of streams and peer copies between neighbours as
// "communication"; with an RCCL communicator attached the process holds the single slab `rank` of `world`.
#define DS_XEV 8
enum SlabEvent { EV_FORK = 0, EV_JOIN, EV_HALO, EV_CJOIN, EV_TRI, EV_MSG, EV_GOT, EV_X0 };
struct Slab {
    int index = 0;              // global slab number
    int dev = 0;                // HIP device this slab lives on
    hipStream_t st = nullptr;   // main stream of the slab (slab 0: Solver::stream)
    hipStream_t st_z = nullptr; // second stream: carries the slab's communication in time-slab mode (Solver::comm_z)
    // the slab's events (created by alloc_slabs, destroyed by free_slabs): fork / join / halo of the second stream; CJOIN:
    // synchronous communication on it is done (Solver::comm_leave); TRI: this slab's interface message is written
    // (Solver::tri_exchange); MSG / GOT: batched exchanges, "my messages are written" / "I have pulled mine"; X0 ..: ordering
    // of cross-slab copies (Solver::xcopy), used round-robin
    hipEvent_t ev[EV_X0 + DS_XEV] = {nullptr};
    int xev_next = 0;
    DevRes *res = nullptr;      // plans / tables of `dev`
    double *h_sums = nullptr;   // pinned host copy of this slab's KKT partial sums [S_COUNT]
    Grid g;
    // Every device buffer of the slab is allocated through alloc() / zalloc() and owned by this list, whichever file asks
    // (alloc_slabs, tri_alloc, palm_begin, acc_alloc); the named pointers below are views that kernels read, loops swap
    // and nobody frees.  Solver::free_slabs() releases the list.
    std::vector<void *> owned;
    template <class T> int alloc(T **p, i64 n) {
        DS_CHECK(dmalloc(p, n));
        owned.push_back(*p);
        return 0;
    }
    int zalloc(double **p, i64 n) {     // ... zeroed on the slab's main stream
        DS_CHECK(alloc(p, n));
        DS_HIP(hipMemsetAsync(*p, 0, sizeof(double) * (size_t)(n > 0 ? n : 1), st));
        return 0;
    }
    double *phi = nullptr;      // NphiAlloc (owned nodes + halo layer)
    double *q = nullptr;        // NqAlloc
    double *alpha = nullptr;    // NqAlloc
    double *z = nullptr;        // 10 * Nz
    double *beta = nullptr;     // 10 * Nz
    double *c = nullptr;        // Nphi
    bool c_ends = false;        // every layer of c but global layer 0 and nt - 1 is all-zero bits (Solver::detect_c_ends, at begin())
    double *weight = nullptr;   // NqAlloc (weighted only)
    double *w0 = nullptr, *w1 = nullptr;   // Poisson work arrays (slab layout)
    // Poisson t-axis: this slab's pencil = columns [l0, l0+nl) of the ny*nx (y, x) columns, all nt nodes
    i64 l0 = 0, nl = 0;
    double *pencil = nullptr, *pencil2 = nullptr;   // nl * nt each (pencil2: dense / RCCL staging)
    double *stage = nullptr;                        // Nphi (RCCL pack buffer)
    // halos received from the LEFT neighbour (nullptr on the first slab)
    double *u0_prev = nullptr, *tail_bx = nullptr, *tail_by = nullptr;
    double *a0_prev = nullptr, *a0w_prev = nullptr, *btail_bx = nullptr, *btail_by = nullptr;
    // staging for what this slab sends to the RIGHT neighbour (nullptr on the last slab)
    double *send_plane = nullptr, *send_plane2 = nullptr, *send_bx = nullptr, *send_by = nullptr;
    KktWork kw{};
    // fused path (fused.hip): q^{k-1}, adjoint sums, ping-pong beta, tile-boundary side buffers
    double *q_old = nullptr, *q2 = nullptr, *beta2 = nullptr, *sx = nullptr, *sy = nullptr;
    double *q3 = nullptr, *p2 = nullptr, *sxp = nullptr, *syp = nullptr;    // PALM, one pass over beta per iteration (solver_palm.hip)
    // ... on time slabs: the second gather's share of the neighbour's first edge layer (sent to the right / received from the left)
    double *send_pbx = nullptr, *send_pby = nullptr, *ptail_bx = nullptr, *ptail_by = nullptr;
    double *alpha2 = nullptr;   // ping-pong partner of alpha (q-step that also forms the next rhs)
    double *sx2 = nullptr, *sy2 = nullptr;   // ping-pong partners of sx / sy (the early cone pass; allocated at its first use)
    // Behind k_qcone, which wrote alpha^{k+1} to alpha2, q^{k+1} to q_old (exit form; the steady form stores none), the new
    // sums to q / sx2 / sy2 and the multipliers to beta2: q holds q^{k+1}, q2 / sx / sy the new sums, and q_old the old
    // sums -- a dead buffer, as the next q-step expects
    void rotate_after_qcone() {
        std::swap(alpha, alpha2);
        double *const sums = q;
        q = q_old; q_old = q2; q2 = sums;
        std::swap(sx, sx2);
        std::swap(sy, sy2);
        std::swap(beta, beta2);
    }
    // partitioned tridiagonal t-solve (tri.hip): messages to / from the owners of the modes, zero-mode work line
    double *tri_send = nullptr, *tri_recv = nullptr, *tri_bsend = nullptr, *tri_brecv = nullptr, *tri_zero = nullptr;
    double *carry = nullptr;    // 4 layer planes: hand-off between the chunk launches of a cone pass (FusedArgs::carry_in / _out)
    FusedGeom fg{};
    // acc-ADMM loop (solver_acc.hip): x^+ of the iteration (q^+ lives in q_old, beta^+ in beta2) and the
    // Halpern anchors / previous extrapolation points
    double *phi_p = nullptr, *alpha_p = nullptr, *z_p = nullptr;
    double *phi_a = nullptr, *q_a = nullptr, *alpha_a = nullptr, *z_a = nullptr, *beta_a = nullptr;
    // solution report (report.hip; allocated at its first use): bin edges, per-tile layer sums [ntl][3][tiles], their totals
    // [ntl][3], the 64-bit counters [RC_COUNT]
    double *rep_edges = nullptr, *rep_part = nullptr, *rep_sums = nullptr;
    unsigned long long *rep_counts = nullptr;
    // the geodesic's profile (geodesic.hip; allocated at its first use): geodesic_doubles / geodesic_counts of the slab
    double *geo_buf = nullptr;
    unsigned long long *geo_cnt = nullptr;
    // particle transport (advect.hip; allocated at its first use): a ring of two velocity layers, slot (global node & 1) at
    // adv_vel + 2 * plane * slot = [vX | vY]; adv_have: the global node each slot holds (-1: none)
    double *adv_vel = nullptr;
    i64 adv_have[2] = {-1, -1};
};

// every slab this process holds, with the slab's device made current first (member functions returning int)
#define FOR_SLABS(s) for (auto &s : slabs) if (int rc_use__ = use(s)) return rc_use__; else

// nodes [t0, t1) of slab `rank`; pencil j of `world`: columns [l0, l1) of the plane's (y, x) columns (solver_slabs.hip)
int dotsocp_slab_range_impl(i64 nt, int world, int rank, i64 *t0, i64 *t1);
void pencil_range(i64 plane, int world, int j, i64 *l0, i64 *l1);

enum Phase { PH_RHS = 0, PH_POISSON, PH_PROJ, PH_QSTEP, PH_BETA, PH_KKT, PH_FUSED_A, PH_FUSED_B, PH_MATERIALISE,
             PH_COMM, PH_INTERP, PH_ACC_CONE, PH_ACC_GATHER, PH_QSTEP0, PH_TRANSPOSE, PH_CONE_CARRY, PH_QCONE, PH_VELOCITY, PH_ADVECT,
             PH_DEPOSIT, PH_FRAME_L1, PH_ADVECT_PATH, PH_MAP_FINAL, PH_HL_PASS_X, PH_HL_PASS_Y, PH_HL_REDUCE,
             PH_SL_PASS_X, PH_SL_PASS_Y, PH_SL_NODE, PH_COUNT };

struct Solver {
    // ================ devices, streams, slabs: solver_slabs.hip ================
    dotsocp_problem prob{};
    int device = 0;
    i64 ny = 0, nx = 0, nt = 0;     // internal dims (1-D problems: ny = nx1d, nx = 1)
    // streams of slab 0 (created by init() on `device`; the other in-process slabs create their own): the main stream
    // carries everything but the overlapped cone pass, and all RCCL communication
    hipStream_t stream = nullptr;
    hipStream_t stream_z = nullptr;    // cone pass when it overlaps the phi step
    bool multi_device = false;         // dotsocp_create_multi: slab r on device (device + r) mod #devices
    int ndev_visible = 1;
    std::vector<DevRes *> devres;      // one per device in use
    int cur_dev = -1;                  // device made current by use() (-1: unknown)
    std::vector<Slab> slabs;        // the slabs held by THIS process
    // one host thread per slab issues that slab's launches while run() is active (defer.h); null: the caller's thread
    // issues everything (one slab, one process per GPU, DOTSOCP_HOST_THREADS=0)
    std::unique_ptr<DeferCtx> defer;
    int world = 1;                  // total number of slabs
    int rank = 0;                   // RCCL mode: this process's slab
    void *nccl = nullptr;           // ncclComm_t when a communicator is attached
    double *h_sums = nullptr;       // pinned host buffer [S_COUNT + 1] (RCCL mode: reduced sums + clock)
    double *d_red = nullptr;        // device buffer for the cross-rank reduction [S_COUNT + 1]
    bool fused = true;       // DOTSOCP_FUSED=0 selects the unfused reference dataflow (z stored, 3 cone passes)
    bool overlap = false;    // DOTSOCP_OVERLAP=0/1 overrides (default: on in time-slab mode)
    bool tri_tsolve = true;  // time-slab Poisson solve by partitioned tridiagonal systems (tri.hip); DOTSOCP_TSOLVE=dct:
                             // slab <-> pencil transposes around the t-axis DCT instead
    bool peer_ok = true;         // every pair of devices in use can address each other's memory (alloc_slabs)
    bool cross_device = false;   // some pair of this process's slabs lives on different devices (alloc_slabs)
    ~Solver();
    int init(const dotsocp_problem *p, int device, int nslabs, bool multi_dev = false);
    int attach_rccl(const unsigned char *id, int rank, int world);
    int use(const Slab &s);            // hipSetDevice(s.dev) unless it already is the current one
    int use_dev(int d);
    int sync_all();                    // host waits for every stream of every slab
    DevRes *res_for(int dev);          // plans + tables on `dev` (created on first request)
    i64 column_pad() const;
    i64 row_pitch() const;             // row pitch of this context's device arrays (ny unless the single slab is pitched)
    int alloc_slabs(int first, int count);
    int ensure_alloc();
    void free_slabs();
    bool multi() const { return world > 1; }
    bool remote() const { return nccl != nullptr; }

    // ================ messages between slabs: solver_comm.hip ================
    // in-process slabs: dst (on `to`) <- src (on `from`), ordered after everything enqueued so far on both slabs'
    // main streams and before everything enqueued later on either (what one shared stream used to give for free)
    int xcopy(Slab &from, const double *src, Slab &to, double *dst, i64 count);
    int xcopy2d(Slab &from, const double *src, size_t spitch, Slab &to, double *dst, size_t dpitch, size_t width,
                size_t height);
    // Time slabs: every message between slabs travels on the slab's SECOND stream (RCCL calls, pull launches, peer copies),
    // kernels stay on the main stream.  A communication step is bracketed by comm_enter() / comm_leave(): the second
    // stream first waits for what the main stream holds (fork), and the main stream then waits for the messages (join) --
    // the synchronous form every caller gets by default.  Solver::step() instead runs the iteration's exchanges
    // asynchronously (comm_async): it forks, issues the exchange, marks an event on the second stream, enqueues kernels
    // that do not need the message on the main stream and lets the main stream wait for the mark only in front of the
    // first kernel that does -- the messages travel while kernels run, and no two kernels ever compete for the compute
    // units (measured: a cone pass on a second stream stretched the whole-CU DCT passes beside it from 60 to 400 us)
    bool comm_z = false;               // communication on the second streams (time-slab mode; DOTSOCP_OVERLAP=0: on the main stream)
    bool comm_async = false;           // inside an asynchronous exchange of step(): comm_enter / comm_leave do nothing
    int comm_depth = 0;
    hipStream_t cst(const Slab &s) const { return comm_z ? s.st_z : s.st; }
    int comm_enter();
    int comm_leave();
    int comm_fork();                               // second streams wait for the main streams
    int comm_mark(SlabEvent ev);                   // record on the second streams
    int comm_wait(SlabEvent ev);                   // main streams wait
    int open_groups = 0;            // ncclGroupStart calls not yet matched by ncclGroupEnd (comm.h: DS_NCCL_G)
    // every slab with a neighbour in direction `dir` (+1 right, -1 left) sends `count` doubles
    // from src(slab) to dst(neighbour)
    typedef std::function<double *(Slab &)> Sel;
    int shift(int dir, const Sel &src, const Sel &dst, i64 count);
    int shift_edge_halo(const Sel &base);      // first owned bx / by layers of base(s) -> halo layer of the left slab
    int group_begin();
    int group_end();
    // slabs of one process: the copies of the shift() calls between group_begin() and group_end() (a lone shift() is a
    // group of one) are collected and pulled by ONE launch per receiving slab (flush_msgs)
    struct Msg { int from, to; const double *src; double *dst; i64 count; };
    std::vector<Msg> msgs;
    int msg_depth = 0;
    bool pull_default(const char *env_var) const;
    bool msg_batching() const;
    int flush_msgs();
    // the q halo / u0 tail of the newest iterate have not been exchanged yet: step() issues the exchange behind the
    // fork so that the cone chunks that do not read the halo overlap it; every other reader calls ensure_halo()
    bool halo_pending = false;
    bool u0_fresh = false;   // u0_prev holds w.*q0 - alpha0 of the CURRENT iterate of the left neighbour
    bool u0_made = false;    // send_plane holds the u0 tail of the current iterate (written by the q-step itself)
    int make_u0_tail();
    int exchange_u0_tail();
    int exchange_q_halo(bool with_u0);
    int ensure_halo();       // run the q-halo exchange the last q-step left pending (halo_pending)
    int make_tails();        // time slabs: finalise the adjoint sums of the last owned cell for the right neighbour
    int send_tails();        // ... adjoint tails -> right
    int send_phi_head();     // ... first phi layer -> left
    int ship_tails();        // all three, one group (nothing without time slabs)
    int transpose(bool forward);
    // hooks of the asynchronous schedule inside the partitioned t-solve: `fill` runs on the main streams while the first
    // interface exchange travels, `behind` right after the second one has been issued
    struct PhiHooks { std::function<int()> fill, behind; };
    int tri_alloc();
    int tri_exchange(bool back);
    int poisson_t_tridiag(const PhiHooks *hooks);

    // ================ host <-> device fields, outputs, report, multilevel transfer: solver_io.hip ================
    i64 field_len(int field) const;
    // rows of `rowlen` doubles between a device array with rows `pitch` apart and an array in the reference layout: a host
    // array (dir = ROWS_DOWN / ROWS_UP; `false` / `true` of the callers), or one on device `src_dev` that is read
    // (ROWS_FROM_DEV; a peer copy where that is not the current device)
    enum { ROWS_DOWN = 0, ROWS_UP = 1, ROWS_FROM_DEV = 2 };
    int copy_rows(double *dev, double *host, i64 rowlen, i64 pitch, i64 nrows, int dir, hipStream_t st, int src_dev = -1);
    int upload(int field, const double *host);
    int upload_layers(int field, const double *host, i64 t0, i64 n);
    int download(int field, double *host);
    // model.weight <- `src`: the weight of this grid in the reference layout on device `src_dev` (a level of a weight
    // pyramid, weights.h); every slab takes its layers.  Replaces upload(DOTSOCP_F_WEIGHT, ...).
    int upload_weight_from(const double *src, int src_dev, i64 src_ny, i64 src_nx, i64 src_nt);
    // c is zero off its two end layers (model.c of initialize.m:42-50): the q-step, k_rhs and the sigma fix skip the rest
    bool c_ends_on = true;       // DOTSOCP_C_ENDS=0: load all of c
    int detect_c_ends();
    // what every reader of the node density stages (outputs, report, velocity)
    int stage_left_tail();
    int stage_rho_ends(Slab &s, const double *rho0, const double *rho1);
    int canary_after();          // DOTSOCP_CANARY=1: the guard bands, checked while the buffers of a call are live
    int recover_outputs(const double *rho0, const double *rho1, double *rho, double *Ex, double *Ey, double *q0,
                        double *bx, double *by);
    int jump_from(Solver &coarse);
    // mass / negativity / f(q) histograms / cost of the finished solve in one pass over alpha and q (report.hip);
    // layer_mass, layer_neg: nt doubles each or NULL
    int solution_report(const double *rho0, const double *rho1, dotsocp_report *rep, double *layer_mass, double *layer_neg);
    // the profile of the finished solve per time node in one pass over alpha (geodesic.hip, geodesic_summary.h); sums
    // (nt x DOTSOCP_GEO_SUMS), rho_max, n_support (nt each): host, each may be NULL
    int geodesic_profile(const double *rho0, const double *rho1, dotsocp_geodesic *res, double *sums, double *rho_max, i64 *n_support);
    // frames (and arrows) of the density evolution (render.hip).  Engine coordinates: mvX is the component along the second
    // array index, mvY along the first; a 1-D problem lives in Y (capi.hip hands its mvx over as mvY, its skip_x as skip_y)
    int render_evolution(const double *rho0, const double *rho1, const dotsocp_render_opts *o, const i64 *frame_nodes,
                         const double *levels, const unsigned char *lut, const unsigned char *barrier, unsigned char *image,
                         double *mvX, double *mvY, dotsocp_render_info *info);

    // ================ velocity and particles along it: solver_particles.hip ================
    // v = E / rho at the nodes and particles along it (advect.hip).  Coordinates of the engine: X along the second array
    // index, Y along the first; a 1-D problem lives in Y (capi.hip hands its x over as y).
    int velocity_stage(const double *rho0, const double *rho1);          // rho0 / rho1 / a_prev in place, rings empty
    int velocity_layer(Slab &s, i64 tg, double floor);                   // the slab's ring holds global node layer tg
    int recover_velocity(const double *rho0, const double *rho1, double floor, double *vX, double *vY);
    int advect_particles(const double *rho0, const double *rho1, const dotsocp_advect_opts *o, double *x, double *y,
                         double *traj_x, double *traj_y, i64 *n_clamped);
    // the same march with the particles' mass deposited at the requested nodes, or with the path sums and one reduction at its end
    int push_mass(const double *rho0, const double *rho1, const dotsocp_push_opts *o, double *x, double *y, const double *mass,
                  const i64 *frame_nodes, double *frames, i64 *n_clamped, double *unit, double *l1);
    int map_report(const double *rho0, const double *rho1, const dotsocp_advect_opts *o, double *x, double *y, const double *mass,
                   dotsocp_map_report_t *rep, double *disp, double *len, double *action);

    // ================ the dual lower bound on W2^2: solver_dual.hip ================
    // Hopf-Lax transforms of phi's first and last node layer and the sums of the Kantorovich dual (hopflax.hip), on the first
    // slab's device; H, B (ny x nx doubles), arg_fwd, arg_bwd (ny x nx ints): host, each may be NULL
    int dual_bound(const double *rho0, const double *rho1, dotsocp_dual *res, double *H, double *B, int *arg_fwd, int *arg_bwd);

    // ================ the upper bound on W2^2: solver_upper.hip ================
    // Sinkhorn sweeps of soft Hopf-Lax transforms from phi's first node layer, rounded to a feasible plan (softlax.hip), on
    // the first slab's device; f_start and the output arrays (ny x nx doubles; defects: max_sweeps): host, each may be NULL
    int upper_bound(const double *rho0, const double *rho1, const double *f_start, const dotsocp_upper_opts *o, dotsocp_upper *res,
                    double *f, double *g, double *E, double *er, double *ec, double *defects);
    // dotsocp_upper_map: the bound and the barycentric map of its plan; frames at time nodes with l1 against rho there
    int upper_map(const double *rho0, const double *rho1, const double *f_start, const dotsocp_upper_opts *o, dotsocp_upper *res,
                  double *f, double *g, double *E, double *er, double *ec, double *defects, dotsocp_plan_map_t *map_res, double *Dx,
                  double *Dy, double *C, double *row, double *spread, const i64 *frame_nodes, i64 nf, double *frames, double *l1);

    // ================ the inPALM loop and its profiling: solver.hip ================
    // ---- loop state (mirrors solver_socp_inPALM.m:11-135) ----
    bool begun = false, finished = false, stopped = false;
    dotsocp_opts opts{};
    bool checkPrimDualFeas = true;
    double time_limit = 3600.0;
    double sigma = 1.0, sigmaScale = 1.0;
    double cScale = 1.0, dScale = 1.0, D = 1.0, E = 1.0;
    double norm_c = 0.0, norm_d = 0.0;
    double h = 1.0;
    int rescale = 0, use_feasOrg = 0;
    double maxFeas = 0.0, relGap = 0.0, tol_feasOrg = 0.0;
    double lastSigmaIt = 0.0;
    i64 it = 0;
    LoopCoef lc{};
    std::vector<double> hist_kkt, hist_time, hist_iter, hist_gap;   // kkt stored row-wise (7 per entry)
    std::chrono::steady_clock::time_point t_begin;
    double elapsed_prev = 0.0;
    double elapsed_agreed = 0.0;    // multi-process: max over ranks at the last KKT check
    // ---- the fused dataflow: what is pending, what is valid ----
    bool deferred = false;   // fused path: beta still holds beta^{k-1}; z is not materialised
    bool z_valid = true;     // s.z holds the z of the last completed iteration
    bool z_prev_ok = false;  // s.beta2 / s.q_old still hold (beta^k, q^k): z can be regenerated (MODE_Z)
    bool rhs_valid = false;  // w0 holds A'(w.*q - alpha) + c of the current iterate (left there by the q-step)
    // The gamma form.  Between two plain iterations the cone pass stores gamma^k = beta^k + tau z^{k+1} where it would
    // store beta^k; the next pass forms beta^{k+1} = gamma^k - tau (BF q^{k+1} + d) from the q it reads anyway -- no q_old,
    // no second projection.  Every other reader of beta or z needs the beta form: an iteration known (at its start) to be
    // followed by one writes beta (schedule.h: cone_writes_beta; plan_step decides it as StepPlan::pass_gout).
    bool cone_carry = true;      // DOTSOCP_CONE_CARRY=0: every deferred pass reads and writes beta
    bool beta_gamma = false;     // s.beta holds gamma (deferred only)
    i64 run_left = -1;           // iterations the current run() call still has, counting this one (set by run(); negative: no bound)
    // The early cone pass.  A gamma-reading pass needs q^{k+1} and gamma^k only -- not phi -- so the q-step of an iteration
    // whose own pass left gamma runs the NEXT iteration's pass in the same kernel, on the q it holds in registers
    // (qstep_march.hip: k_qcone; one slab, inPALM / ALG2, unweighted).  plan_step names the form (StepPlan::qcone_candidate),
    // step() drops it if the time limit has passed, and the bookkeeping of that pass is done where the launch is issued
    // (phase_q).  The form is handed to the next iteration's plan, which schedules no launch and reports a form that
    // contradicts its own schedule (StepPlan::error).
    // After the steady form q^{k+1} is not in memory (q_valid): by the schedule every reader of q follows an exit form.
    int qcone = -1;              // DOTSOCP_QCONE: 0 never, 1 wherever eligible, 2 as 1 with the two kernels back to back
                                 // (the schedule alone); unset (-1): on grids of at least 2048 tiles
    bool q_valid = true;         // s.q holds q of the last q-step
    int early_pass = QCONE_NONE; // the form in which the cone pass of the NEXT iteration has run
    StepIn step_in() const;      // the facts plan_step() decides this iteration from (schedule.h)
    int need_q(const char *who) const;
    bool time_limit_passed() const;
    i64 timeout_at = -1;         // DOTSOCP_TEST_TIMEOUT_AT (test hook): the time limit counts as passed from this iteration on
    bool timeout_pending = false;   // the time limit passed in an iteration that wrote gamma: the next one checks and stops
    int need_beta_form(const char *who) const;
    // fused path: scalings of beta that the next pass over beta applies on load (saves a 20 Nz pass); at most two wait
    ScaleOps bops{0, 1.0, 1.0, 1.0, 1.0};
    ScaleOps zp_ops{0, 1.0, 1.0, 1.0, 1.0};    // the ops that were pending on the kept beta^k (beta2) when it was read
    int push_beta_op(double mul, double div);
    int flush_beta();
    // same for alpha after a sigma update on the folded KKT path: the next q-step divides on load (one slot in use)
    ScaleOps aops{0, 1.0, 1.0, 1.0, 1.0};
    int flush_alpha();
    int sigma_scale_folded(double factor);
    // the multiplier step is still pending: (q^{k-1}, q^k, beta^{k-1}) and the pending ops of beta; callers add outputs
    FusedArgs pending_step_args(const Slab &s) const;
    // KKT sums of the last check (Solver::kkt_block) and the sigma they were taken with: the rescale block of the
    // NEXT iteration finds its five norms there instead of making its own passes over the state
    double last_S[S_COUNT] = {0};
    double last_S_sigma = 1.0;
    i64 last_S_it = -1;
    bool norm_cache = true;  // DOTSOCP_NORM_CACHE=0: the rescale block always makes its own passes for its norms
    bool kkt_fold = true;    // DOTSOCP_KKT_FOLD=0: KKT sums by the separate node / edge launches on every path
    KktCoef kkt_coef() const;
    int clear_partials(Slab &s);     // zero every region of the slab's KKT partial sums (on its main stream)
    int begin(const dotsocp_opts *o);
    int begin_method(const dotsocp_opts *o, int method, const dotsocp_acc_opts *acc);
    int run(i64 n_iters, i64 *done);
    int finish(dotsocp_result *res);
    int step(bool *brk);
    int rescale_block();
    int poisson_all(const PhiHooks *hooks = nullptr);
    int poisson_phi();               // test support: poisson_all() on the phi field, before begin()
    int phase_phi(const PhiHooks *hooks = nullptr);
    // part 0: all chunks; 1: all but the last chunk; 2: the last chunk (the only one that reads the q halo)
    int phase_z(const StepPlan &plan, int part);
    // part 0: whole q-step; 1: all chunks but the last; 2: the last chunk (the one that reads the phi halo), then finish;
    // early: the QCONE_* form of the next iteration's cone pass that rides along
    int phase_q(const StepPlan &plan, int part, int early = QCONE_NONE);
    int phase_mult();
    int materialise();
    int ensure_z();
    int kkt_sums(double *S, bool folded = false);
    int reduce_sums(double *S);
    int norms_light(double *S);
    int kkt_block(bool adjustSigmaYes, bool timed_out, bool *brk, bool folded = false);
    int scale_state(double a_mul, double a_div, double q_div, bool with_c);
    void update_coef();
    double elapsed() const;
    // ---- profiling (HIP events on slab 0's main stream; on_z: its second stream); slab 0 stands for all (lockstep) ----
    bool profiling = false;
    struct Pending { hipEvent_t a, b; int phase; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> event_pool;
    double phase_ms[PH_COUNT] = {0};
    i64 phase_launches[PH_COUNT] = {0};
    void prof_begin(int phase, bool on_z = false);
    void prof_end(int phase, bool on_z = false);
    int prof_flush();

    // ================ loop variants (include/dotsocp.h: DOTSOCP_METHOD_*): solver_acc.hip, solver_palm.hip ================
    int method = DOTSOCP_METHOD_INPALM;
    // acc-ADMM (solver_socp_accADMM.m:12-34,157-163)
    i64 acc_restart = 100, acc_k = 0;
    double acc_rho = 2.0, acc_theta = 2.0;
    bool acc_halpern = true;
    bool acc_gather_valid = false;     // q2 / sx / sy hold F*B*(z + beta) of the current state
    bool acc_swapped = false;          // state and x^+ pointers are exchanged (during the KKT block / after a stop)
    bool acc_post = true;              // Halpern: after a KKT check z and beta take ONE pass (k_acc_cone modes 1 / 3) instead of
                                       // scalings, anchor copies, extrapolation passes and the gather pass (DOTSOCP_ACC_POST=0: off)
    bool acc_light = false;            // inside that iteration's KKT block: the sigma update leaves z, beta and their anchors alone
    double acc_factor = 1.0;           // factor of that block's sigma update (1: none)
    int acc_alloc();
    int acc_begin(const dotsocp_acc_opts *acc);
    int acc_step(bool *brk);
    int acc_rescale_block();
    int acc_set_anchors();
    void acc_swap_state();
    int acc_on_sigma_factor(double factor);
    AccCoef acc_coef() const;
    // PALM (solver_palm.hip)
    bool palm_fast = true;     // one pass over beta per iteration (DOTSOCP_PALM_FAST=0: the two-pass dataflow)
    bool palm_p_valid = false; // p2 / sxp / syp hold the second gather of the last cone pass
    int palm_begin();
    int palm_step(bool *brk);
};

// Device scratch of one call: released once every stream of the context is idle, on the error paths too
struct DeviceScratch {
    Solver &S;
    std::vector<double *> bufs;
    explicit DeviceScratch(Solver &s) : S(s) {}
    // on the current device; fp = false: the buffer holds integer regions too and stays as it comes under DOTSOCP_POISON=1
    // (the caller names its floating-point regions with poison_region())
    int alloc(double **p, i64 n, bool fp = true) { DS_CHECK(dmalloc(p, n, fp)); bufs.push_back(*p); return 0; }
    ~DeviceScratch() {
        if (bufs.empty()) return;
        S.cur_dev = -1;
        (void)S.sync_all();
        for (double *b : bufs) dfree(b);
    }
};

}  // namespace dotsocp
