/*
 * dotsocp.h -- C ABI of libdotsocp, the MI355X (gfx950) implementation of the
 * inPALM/ADMM SOCP iteration loop of chlhnu/DOT-SOCP.
 *
 * Two drop-in boundaries:
 *
 *   B2  operator level -- the five MEX operators the reference ships as binaries.
 *       Host pointers in MATLAB column-major layout; like the MEX files, the FIRST
 *       argument is overwritten in place.  A MEX gateway binds them one-to-one
 *       (dot-socp_amd/mex/).
 *
 *   B1  solver level -- [runHist, sigma] = solver_socp_inPALM(var, opts, model)
 *       (socp/dot2d/algorithms/solver_socp_inPALM.m:1, the dot1d twin, and
 *       socp/wdot2d/algorithms/solver_wsocp_inPALM.m:1).  The device owns the whole
 *       loop state between create() and destroy(); the caller uploads the fields of
 *       VarHandle / ModelHandle once, runs, and downloads the iterates.
 *
 * All functions return 0 on success and a negative DOTSOCP_E* code otherwise;
 * dotsocp_last_error() returns a thread-local description.  No exceptions cross the
 * ABI.  There is NO CPU fallback: without a HIP device every compute entry point
 * fails with DOTSOCP_ENODEVICE.
 *
 * Layout conventions (identical to the reference): grid ny x nx x nt, y fastest, then
 * x, then t;  Nphi = ny*nx*nt, Nz = ny*nx*(nt-1), Nbx = ny*(nx-1)*nt,
 * Nby = (ny-1)*nx*nt, Nq = Nz+Nbx+Nby;  q = [q0; bx; by];  z, beta = Nz x 10
 * column-major (1-D problems: grid nx x nt, q = [q0; bx], z = Nz x 6).
 */
#ifndef DOTSOCP_H
#define DOTSOCP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef long long dotsocp_i64;

enum {
    DOTSOCP_OK = 0,
    DOTSOCP_EINVAL = -1,     /* bad argument (sizes, NULL, unknown field)            */
    DOTSOCP_ENODEVICE = -2,  /* no HIP device / HIP runtime error at initialisation  */
    DOTSOCP_EHIP = -3,       /* a HIP call or kernel failed                          */
    DOTSOCP_ESTATE = -4,     /* call sequence violated (e.g. run() before begin())   */
    DOTSOCP_ECOMM = -5       /* RCCL / communicator failure                          */
};

const char *dotsocp_last_error(void);
const char *dotsocp_version(void);
/* number of visible HIP devices (0 when there is none; never fails) */
int dotsocp_device_count(void);
/* Device buffers of destroyed contexts are kept (per device) and reused by the next context that asks for buffers of
 * their size: on this platform a hipMalloc that follows the release of tens of GB takes seconds.  This call returns
 * them to the driver (bytes released); DOTSOCP_DEVICE_CACHE=0 in the environment disables the cache altogether. */
dotsocp_i64 dotsocp_release_cache(void);

/* ===================================================================================
 * B2 -- operator level, HOST pointers (replaces the reference MEX binaries)
 * =================================================================================== */

/* mexProjSoc(out, in)  -- socp/{dot1d,dot2d,wdot2d}/utils/mexProjSoc.mexa64;
 * call sites socp/dot2d/algorithms/solver_socp_inPALM.m:199,240.
 * Row-wise projection of the M x K column-major matrix `in` onto {x1 >= ||x_2..K||}. */
int dotsocp_proj_soc(double *out, const double *in, dotsocp_i64 M, dotsocp_i64 K);

/* mexBFd(z, q, nt, nx, ny, scale, dF)  -- socp/dot2d/utils/mexBFd.mexa64;
 * call sites solver_socp_inPALM.m:133,187,212,242.   z <- B F q + d  (Nz x 10).
 * Slots whose edge lies outside the domain are not written (keep the caller's value). */
int dotsocp_bfd(double *z, const double *q, dotsocp_i64 nt, dotsocp_i64 nx, dotsocp_i64 ny,
                double scale, double dF);

/* mexBFdConj(q, z, nt, nx, ny, scale)  -- socp/dot2d/utils/mexBFdConj.mexa64;
 * call sites solver_socp_inPALM.m:205,225; socp/dot2d/utils/jump_nextLevel.m:16.
 * q <- F* B* z  (Nq). */
int dotsocp_bfd_conj(double *q, const double *z, dotsocp_i64 nt, dotsocp_i64 nx, dotsocp_i64 ny,
                     double scale);

/* mexBFd1d(z, q, nt, nx, scale, dF)  -- socp/dot1d/utils/mexBFd1d.mexa64;
 * call sites socp/dot1d/algorithms/solver_socp_inPALM.m:132,186,211,241.  z is Nz x 6. */
int dotsocp_bfd1d(double *z, const double *q, dotsocp_i64 nt, dotsocp_i64 nx, double scale, double dF);

/* mexBFdConj1d(q, z, nt, nx, scale)  -- socp/dot1d/utils/mexBFdConj1d.mexa64;
 * call sites socp/dot1d/algorithms/solver_socp_inPALM.m:204,224. */
int dotsocp_bfd_conj1d(double *q, const double *z, dotsocp_i64 nt, dotsocp_i64 nx, double scale);

/* res = oper_poisson3dim(kernelScale * initialize_FFTkernel(nt,nx,ny), rhs)
 * -- socp/dot2d/utils/oper_poisson3dim.m:4, initialize_FFTkernel.m:6-15,
 *    mirt_dctn.m / mirt_idctn.m (orthonormal DCT-II / DCT-III along every axis);
 *    call site solver_socp_inPALM.m:96,194.   For a 1-D problem pass ny = nx1d, nx = 1
 *    (socp/dot1d/utils/oper_poisson.m:4).  rhs and res hold ny*nx*nt doubles.
 *    Lengths: a power of two may have up to 2^20 points on every axis (dotsocp_dct_levels), any other length up to
 *    2^19 - 1 (dotsocp_cdft_levels); a longer one is refused with DOTSOCP_EINVAL before anything is launched. */
int dotsocp_oper_poisson(double *res, const double *rhs, dotsocp_i64 ny, dotsocp_i64 nx,
                         dotsocp_i64 nt, double kernelScale);

/* a <- dctn(a) (inverse = 0) or idctn(a) (inverse = 1) of an ny x nx x nt array
 * -- socp/dot2d/utils/mirt_dctn.m:64-141, mirt_idctn.m:59-128.  Power-of-two lengths up to 2^20 on every axis: in
 *    one pass while the line fits the LDS, by a two-level FFT beyond (dotsocp_dct_levels); other lengths up to
 *    2^19 - 1 (dotsocp_cdft_levels); longer: DOTSOCP_EINVAL. */
int dotsocp_dctn(double *a, dotsocp_i64 ny, dotsocp_i64 nx, dotsocp_i64 nt, int inverse);

/* Test support: a <- the DCT-II (inverse = 0) or DCT-III (inverse = 1) of a along ONE axis (0: y, 1: x, 2: t), the other
 * two axes untouched -- exactly the pass dotsocp_dctn makes along that axis: the same length checks, the same plan for
 * the length, the same source and destination buffers.  Different lines of the axis can so carry different data with a
 * known result (tests/test_gpu_dct_probes.py).  Not a reference operator. */
int dotsocp_dct_axis(double *a, dotsocp_i64 ny, dotsocp_i64 nx, dotsocp_i64 nt, int axis, int inverse);

/* Same operators on DEVICE pointers (no PCIe traffic), enqueued on `stream`
 * (a hipStream_t, NULL = default stream).  Used by the parity tests and by bench.py. */
int dotsocp_proj_soc_dev(double *d_out, const double *d_in, dotsocp_i64 M, dotsocp_i64 K, void *stream);
int dotsocp_bfd_dev(double *d_z, const double *d_q, dotsocp_i64 nt, dotsocp_i64 nx, dotsocp_i64 ny,
                    double scale, double dF, void *stream);
int dotsocp_bfd_conj_dev(double *d_q, const double *d_z, dotsocp_i64 nt, dotsocp_i64 nx, dotsocp_i64 ny,
                         double scale, void *stream);

/* ===================================================================================
 * B1 -- solver level (replaces solver_socp_inPALM.m / solver_wsocp_inPALM.m)
 * =================================================================================== */

typedef struct dotsocp_ctx dotsocp_ctx;

/* Discrete model + scaling state on entry: the scalar fields of VarHandle / ModelHandle
 * (socp/dot2d/utils/VarHandle.m:3-17, ModelHandle.m:3-16) after InitialScaling
 * (socp/dot2d/solver_dotsocp2d.m:304-365). */
typedef struct {
    int dim;               /* 2: grid ny x nx x nt; 1: grid nx x nt (ny ignored)            */
    int weighted;          /* 1: solver_wsocp_inPALM semantics, model.weight uploaded       */
    dotsocp_i64 ny, nx, nt;
    double D, E;           /* var.D, var.E                                                   */
    double cScale, dScale; /* var.cScale, var.dScale                                         */
    double normc, normd;   /* model.normc, model.normd                                       */
} dotsocp_problem;

/* opts struct read by the loop (solver_socp_inPALM.m:20-37,64-68) */
typedef struct {
    double tau;                 /* 1.9 inPALM, 1.0 ALG2 (solver_dotsocp2d.m:100-101,133-137) */
    double sigma;               /* initial penalty                                          */
    double tol;
    dotsocp_i64 maxit;
    int ifCheckStepByStep;
    int checkPrimDualFeas;      /* -1 = reference default (true; weighted: false)           */
    int scaling;                /* enables the in-loop rescale block (:64-77,138-190)        */
    double time_limit;          /* seconds; <= 0 means the reference default 3600           */
} dotsocp_opts;

/* Loop variants behind the same boundary: which reference solver file the loop follows. */
enum {
    DOTSOCP_METHOD_INPALM = 0,  /* solver_socp_inPALM.m / solver_wsocp_inPALM.m (ALG2: tau = 1)     */
    DOTSOCP_METHOD_PALM = 1,    /* solver_socp_PALM.m (2-D unweighted only)                          */
    DOTSOCP_METHOD_ACCADMM = 2  /* solver_socp_accADMM.m / solver_wsocp_accADMM.m (2-D only)         */
};

/* extra options of the accelerated ADMM (solver_socp_accADMM.m:12-34); <= 0 selects the reference default */
typedef struct {
    dotsocp_i64 restart;        /* opts.restart, default 100                                         */
    double rho;                 /* opts.rho, default 2                                               */
    double theta;               /* opts.theta, default 2 (== 2: Halpern iteration)                   */
} dotsocp_acc_opts;

/* Field selectors for upload / download */
enum {
    DOTSOCP_F_PHI = 0,   /* Nphi                                  var.phi        */
    DOTSOCP_F_Q = 1,     /* Nq                                    var.q          */
    DOTSOCP_F_ALPHA = 2, /* Nq                                    var.alpha      */
    DOTSOCP_F_Z = 3,     /* Nz x 10 (1-D: Nz x 6)                 var.z          */
    DOTSOCP_F_BETA = 4,  /* Nz x 10 (1-D: Nz x 6)                 var.beta       */
    DOTSOCP_F_C = 5,     /* Nphi                                  model.c        */
    DOTSOCP_F_WEIGHT = 6 /* Nq (weighted only)                    model.weight   */
};

/* Loop outputs (solver_socp_inPALM.m:329-357) */
typedef struct {
    double sigma;          /* returned `sigma` = sigma / sigmaScale (:357)                  */
    double sigma_internal; /* sigma used to un-scale alpha,beta on download (:335-336)      */
    double cScale, dScale; /* var.cScale / var.dScale after in-loop rescales (:344-345)     */
    double times[7];       /* Step_1_1_FFT, Step_1_2_ProjSOC, Step_2_Q_Step,
                              Step_3_Multiplier, KKT, Total_Time, Iters (:339-341)          */
    dotsocp_i64 iters;     /* iterations executed                                           */
    dotsocp_i64 hist_len;  /* runHist.len                                                   */
    int stopped;           /* 1 when the stop criterion (:287-290) fired                    */
    double time_extra;     /* acc-ADMM: 'Interp' (solver_socp_accADMM.m:438-439); PALM: 'Step_1_Q_Step' */
} dotsocp_result;

/* `device` = HIP device ordinal.  `nslabs` >= 1 splits the time axis into that many slabs that live in this one
 * process ON THAT ONE DEVICE (the multi-GPU algorithm -- halo exchange and the t-axis coupling of the Poisson
 * solve -- with the slabs sharing the device's pair of streams, one after the other, and pull launches as messages): a
 * rehearsal / diagnostic mode.  Multi-GPU runs use either
 *   - dotsocp_create_multi(): ONE process, slab r on device (first_device + r) mod #visible devices, neighbour layers
 *     and the interface values of the t-solve travel as peer copies (hipMemcpyPeerAsync over xGMI), per-device KKT
 *     partial sums are added up on the host.  This is what a single MATLAB process (solver_dotsocp2d.m:208 calls
 *     the loop synchronously from the interpreter thread) uses: opts.ngpu of the MEX gateway.  With fewer devices
 *     than slabs, slabs share devices (every slab keeps its OWN pair of streams, also on one device: that is what the
 *     tests of the cross-slab ordering run).  upload / download /
 *     recover_outputs take and return the GLOBAL fields, exactly as with one slab.  STATUS: every loop is verified with
 *     2 .. 8 slabs on concurrent streams of ONE device (the build's boxes have one GPU); slabs on DIFFERENT devices
 *     (hipDeviceEnablePeerAccess, hipMemcpyPeerAsync, cross-device stream waits) have never run on hardware.  Between
 *     different devices messages travel as event-ordered peer copies by default; the launches that pull them through
 *     peer pointers are opt-in there (DOTSOCP_MSG_BATCH=1, DOTSOCP_TRI_GATHER=1), and so is one issuing host thread per
 *     slab (DOTSOCP_HOST_THREADS=1); or
 *   - one process per GPU: dotsocp_create(prob, device, 1) + dotsocp_attach_rccl() (bench.py, torch.distributed). */
dotsocp_ctx *dotsocp_create(const dotsocp_problem *prob, int device, int nslabs);
dotsocp_ctx *dotsocp_create_multi(const dotsocp_problem *prob, int first_device, int ngpu);
void dotsocp_destroy(dotsocp_ctx *ctx);

/* One process per GPU: this process owns time slab `rank` of `world`.  `unique_id` is the
 * 128-byte ncclUniqueId produced by dotsocp_rccl_unique_id() on rank 0 and broadcast by
 * the host (torch.distributed / MPI / MATLAB parallel pool).  Must be called right after
 * create() (before any upload).  With a communicator attached, upload/download take and
 * return the LOCAL slab of each field (dotsocp_slab_range()). */
int dotsocp_rccl_unique_id(unsigned char id[128]);
int dotsocp_attach_rccl(dotsocp_ctx *ctx, const unsigned char id[128], int rank, int world);

/* Time-slab partition used by the multi-GPU mode (pure host arithmetic, no device):
 * nodes [*t0, *t1) of the nt time nodes belong to slab `rank`; its staggered cells are
 * [*t0, min(*t1, nt-1)). */
int dotsocp_slab_range(dotsocp_i64 nt, int world, int rank, dotsocp_i64 *t0, dotsocp_i64 *t1);

/* Number of doubles of the GLOBAL field `field` (DOTSOCP_F_*) of problem `prob` in the reference layout -- what
 * upload() reads and download() writes for a context without an RCCL communicator.  Pure host arithmetic (no
 * device); -1 for an unknown field or a grid with nt < 2.  The MEX gateways check their mxArrays against it
 * before any pointer reaches the library. */
dotsocp_i64 dotsocp_field_len(const dotsocp_problem *prob, int field);

/* Which transform the DCT passes use for an axis of length n (pure host arithmetic, no device; honours the switches
 * DOTSOCP_PFA, DOTSOCP_CDFT, DOTSOCP_CDFT_MIN, DOTSOCP_CDFT_LONG_MIN): 0 none (n <= 1), 1 power-of-two FFT, 2 prime-factor
 * FFT, 3 Rader (257), 4 Bluestein (other lengths up to 1024 in the LDS, from 4101 up to 2^19 - 1 with a two-level
 * convolution: dotsocp_cdft_levels), 5 dense DCT-matrix product. */
int dotsocp_dct_algorithm(dotsocp_i64 n);

/* How the convolution-based transform of a length n runs (pure host arithmetic, no device).  0: no convolution transform
 * (power of two, prime-factor length, dense product, or DOTSOCP_CDFT=0); 1: Rader / Bluestein with the whole convolution
 * in LDS (257 and the Bluestein lengths up to 1024); 2: Bluestein with the convolution of length 2^ceil(log2(2n-1)) as a
 * two-level FFT through a scratch array -- every length from DOTSOCP_CDFT_LONG_MIN (never below 129; default 4101) up
 * to 2^19 - 1 that is neither a power of two nor a prime-factor length, on every axis.  A longer length that is not a
 * power of two is refused with DOTSOCP_EINVAL by dotsocp_dctn, dotsocp_oper_poisson and dotsocp_create before anything
 * is launched. */
int dotsocp_cdft_levels(dotsocp_i64 n);

/* How many passes through memory the transform of an axis of length n takes along `axis` (0: y, the contiguous axis;
 * 1: x; 2: t).  Pure host arithmetic, no device.  0: no transform (n <= 1); 1: one pass, the whole line in LDS (or one
 * of the other transform families); 2: the two-level FFT for power-of-two lines that do not fit the LDS -- from 4096
 * along y and 16384 along x / t, or from DOTSOCP_DCT_LONG_MIN (never below 256) along every axis, up to 2^20;
 * negative: unsupported (a power of two above 2^20: dotsocp_dctn, dotsocp_oper_poisson and dotsocp_create refuse it
 * with DOTSOCP_EINVAL before anything is launched).  dotsocp_dct_algorithm answers 1 (FFT) for every power of two. */
int dotsocp_dct_levels(dotsocp_i64 n, int axis);

/* May the single slab solve the t axis of its Poisson step as tridiagonal systems (tri.hip: k_tsolve_single / k_tsolve_pipe)
 * on an ny x nx x nt grid (1-D: ny = nx1d, nx = 1)?  1 if the powers rho^t of the mode with the largest
 * a' = 4 ((ny-1)^2 + (nx-1)^2) / (nt-1)^2 stay >= 2^-500 over a piece of ceil(nt / NSUB) <= 64 rows; 0 if not (1-D grids
 * whose space step is far finer than the time step, or nt > 512): the solve then takes the transform passes along t,
 * as with DOTSOCP_TSOLVE=dct.  Pure host arithmetic, no device. */
int dotsocp_tsolve_tri_safe(dotsocp_i64 ny, dotsocp_i64 nx, dotsocp_i64 nt);

/* Test support: which kernels the Poisson solve of a single slab launches on an ny x nx x nt grid (1-D: ny = nx1d, nx = 1)
 * whose rows are `pitch` doubles apart (dotsocp_row_pitch(ny) in a context; <= ny: unpitched), on HIP device `device`.
 * Pure host arithmetic on the functions the launchers themselves switch on; the one HIP call is the query of the
 * device's CU count (cached; 256 is assumed where it cannot be asked).  Honours the switches the launchers honour
 * (DOTSOCP_DCT_PIPE, DOTSOCP_TS_PIPE, DOTSOCP_TSOLVE, DOTSOCP_DCT_LONG_MIN and those of dotsocp_dct_algorithm).  What a
 * query by shape cannot know is the alignment of the arrays: it assumes the 16-byte alignment every allocation of
 * the library has (arrays of a caller's own, as dotsocp_dct_axis copies them, are allocations of the library too).
 *   dotsocp_dct_pass_kernel: the DCT-II / DCT-III pass along `axis` (0: y, 1: x, 2: t as a plain transform pass).
 *   dotsocp_tsolve_kernel:   the t step between the forward and the inverse x / y passes.
 * Negative: a bad argument. */
#define DOTSOCP_PASS_NONE 0        /* length 1: a copy */
#define DOTSOCP_PASS_POW2_WAVE 1   /* power of two inside the LDS, one wave per row: k_dct_axis0, k_dct_strided */
#define DOTSOCP_PASS_POW2_WG 2     /* ... the whole workgroup per tile: k_dct_axis0_wg, k_dct_strided_wg */
#define DOTSOCP_PASS_POW2_PIPE 3   /* ... persistent workgroups fed by LDS-DMA: k_dct_axis0_pipe, k_dct_strided_pipe */
#define DOTSOCP_PASS_POW2_LONG 4   /* power of two beyond the LDS: the two-level transform */
#define DOTSOCP_PASS_OTHER 5       /* another family (dotsocp_dct_algorithm) */
#define DOTSOCP_TSOLVE_TRI 1          /* tridiagonal systems, one tile per workgroup: k_tsolve_single */
#define DOTSOCP_TSOLVE_TRI_PIPE 2     /* ... pipelined: k_tsolve_pipe */
#define DOTSOCP_TSOLVE_FUSED 3        /* DCT-II, division, DCT-III in one pass: k_dct_strided<2, .> */
#define DOTSOCP_TSOLVE_FUSED_PIPE 4   /* ... pipelined: k_dct_tsolve_pipe */
#define DOTSOCP_TSOLVE_FUSED_PFA 5    /* ... of a prime-factor length: k_pfa_strided */
#define DOTSOCP_TSOLVE_PASSES 6       /* forward pass, spectral division, inverse pass */
int dotsocp_dct_pass_kernel(int device, dotsocp_i64 ny, dotsocp_i64 nx, dotsocp_i64 nt, dotsocp_i64 pitch, int axis);
int dotsocp_tsolve_kernel(int device, dotsocp_i64 ny, dotsocp_i64 nx, dotsocp_i64 nt, dotsocp_i64 pitch);
/* Row pitch (doubles) of the device arrays of a context whose rows hold ny doubles.  Pure host arithmetic. */
dotsocp_i64 dotsocp_row_pitch(dotsocp_i64 ny);

/* The schedule of the cone pass's gamma form (pure host arithmetic, no device).  Between two plain inPALM iterations
 * the cone pass leaves gamma = beta + tau z in the multiplier array instead of beta; only the next cone pass can read
 * that.  dotsocp_cone_writes_beta: 1 if the pass of iteration `it` must leave beta -- the iteration ends in a KKT check
 * (ifCheckStepByStep, the IfAdjustSigma cadence of solver_socp_inPALM.m:361-379 counted from `last_sigma_it`, it ==
 * maxit), is the last of its run() call, or the rescale block of iteration it + 1 will read the state -- else 0.
 * dotsocp_rescale_due: 1 if the rescale block of iteration `it` (:138-151) takes its norms or rescales, given the loop
 * state it finds (`rescale` = the counter of :64-68, maxFeas / relGap of the last KKT check). */
int dotsocp_cone_writes_beta(dotsocp_i64 it, double last_sigma_it, dotsocp_i64 maxit, int check_step_by_step,
                             int last_of_run, int rescale, double maxFeas, double relGap);
int dotsocp_rescale_due(dotsocp_i64 it, int rescale, double maxFeas, double relGap);
/* The early cone pass (pure host arithmetic, no device): may the q-step of iteration `it` also run the cone pass of
 * iteration it + 1, and in which form?  0: no -- the pass of `it` writes beta (dotsocp_cone_writes_beta), a reader of beta
 * or q follows it.  Otherwise the pass of `it` left gamma, so `it` has no check and every argument is what iteration
 * it + 1 will find: 1 (steady) the early pass writes gamma and q is not stored, 2 (exit) it writes beta and q, because
 * dotsocp_cone_writes_beta(it + 1, ..., next_last_of_run, ...) holds.  The solver adds what only it knows: one slab,
 * inPALM / ALG2 without a weight, no time limit passed, the switch DOTSOCP_QCONE. */
int dotsocp_qcone_form(dotsocp_i64 it, double last_sigma_it, dotsocp_i64 maxit, int check_step_by_step, int last_of_run,
                       int next_last_of_run, int rescale, double maxFeas, double relGap);

int dotsocp_upload(dotsocp_ctx *ctx, int field, const double *host);
int dotsocp_download(dotsocp_ctx *ctx, int field, double *host);
/* Extension for drivers: time layers [t0, t0 + n) of a NODE field (DOTSOCP_F_PHI, DOTSOCP_F_C) from a host buffer that
 * holds just those n layers of ny*nx doubles (with an RCCL communicator: layers of this process's slab); the other layers
 * keep their contents (zeros after create).  model.c of socp/dot2d/utils/initialize.m:42-50 is zero except for its first
 * and last layer, so a driver hands over two layers instead of a grid-sized vector. */
int dotsocp_upload_layers(dotsocp_ctx *ctx, int field, const double *host, dotsocp_i64 t0, dotsocp_i64 n);

/* solver_socp_inPALM.m:11-135 (setup), :136-325 (loop; `n_iters` < 0 = until maxit /
 * stop), :329-357 (outputs).  run() may be called repeatedly; the trajectory is identical
 * to a single call.  After finish(), download PHI/Q/Z/ALPHA/BETA gives var.* of :332-336
 * (alpha and beta multiplied by sigma). */
int dotsocp_begin(dotsocp_ctx *ctx, const dotsocp_opts *opts);
/* Same as dotsocp_begin for another loop file of the reference: DOTSOCP_METHOD_*; `acc` may be NULL
 * (reference defaults) and is read for DOTSOCP_METHOD_ACCADMM only.  run / finish / downloads are
 * unchanged; result.times follows the inPALM order with the variant's extra column in time_extra.
 * All three loops run on time slabs (nslabs > 1 or dotsocp_attach_rccl). */
int dotsocp_begin_method(dotsocp_ctx *ctx, const dotsocp_opts *opts, int method, const dotsocp_acc_opts *acc);
int dotsocp_run(dotsocp_ctx *ctx, dotsocp_i64 n_iters, dotsocp_i64 *done);
int dotsocp_finish(dotsocp_ctx *ctx, dotsocp_result *res);

/* Driver outputs on the device: recoverOrgVar (socp/dot2d/solver_dotsocp2d.m:368-386) +
 * recover_RhoE (utils/recover_RhoE.m:14-25; wdot2d: alpha = weight .* alpha, :11) + recover_q
 * (utils/recover_q.m:12-22) from the device-resident alpha and q, so that only the outputs cross PCIe.  Call
 * after finish().  rho0, rho1: model.rho0 / rho1 (ny x nx, host).  Outputs (host, column-major, any may be NULL):
 * rho, Ex, Ey: ny x nx x nt;  q0, bx, by: ny x nx x (nt-1).  1-D problems: rho, Ex: nx x nt; q0, bx: nx x (nt-1);
 * Ey, by ignored.  Works on time slabs too: in-process slabs (nslabs / dotsocp_create_multi) fill the global arrays;
 * with an RCCL communicator attached every rank gets its own slab of them (node layers [t0, t1) of rho, Ex, Ey,
 * cell layers of q0, bx, by; rho0 / rho1 are read on the first / last rank only). */
int dotsocp_recover_outputs(dotsocp_ctx *ctx, const double *rho0, const double *rho1, double *rho, double *Ex,
                            double *Ey, double *q0, double *bx, double *by);

/* Solution report on the device: what the reference's demos compute from the downloaded outputs --
 * check_massConservation (utils/check_massConservation.m:16-27), hist_negative_density, hist_violation_q_{1d,2d}
 * (utils/hist_positive_value.m:28-55) and the transport cost -- formed in ONE pass over the device-resident alpha and q;
 * no grid-sized array is written or crosses PCIe.  rho, Ex, Ey, q0, bx, by at a node / cell are the values
 * dotsocp_recover_outputs would write, bit for bit, and
 *   fq = (q0 + .5 (bx^2 + by^2)) / (1 + |q0| + sqrt(bx^2 + by^2))          1-D: (q0 + .5 bx^2) / (1 + |q0| + |bx|).
 * Histogram of y = -rho resp. y = fq over the edges of dotsocp_report_edges: bin j counts edges[j] <= y < edges[j+1],
 * the last bin also y == edges[DOTSOCP_REPORT_BINS] (MATLAB histcounts with explicit edges, compared on y itself, not on
 * log10(y)); y < edges[0], y > edges[last] and non-finite y are in no bin.  The layer sums are added in an order that
 * depends on (ny, nx) alone and `cost` in layer order: two calls give the same bits, and so does a context cut into
 * time slabs. */
#define DOTSOCP_REPORT_BINS 49              /* hist_positive_value.m:28-30: 50 edges 10^linspace(-8,-1,50) */
#define DOTSOCP_REPORT_RHO_FLOOR 1e-8       /* nodes with rho <= floor do not enter `cost` */
typedef struct {
    dotsocp_i64 n_nodes, n_cells;           /* ny*nx*nt, ny*nx*(nt-1)  (1-D: nx*nt, nx*(nt-1)) */
    double mass_err, neg_err;               /* max_t |mean(rho(:,:,t)) - 1|, max_t |mean(min(rho(:,:,t),0))|
                                               check_massConservation.m:16-27 (integralL2 = layer mean) */
    double rho_min;  dotsocp_i64 rho_neg;   /* min over finite rho (+Inf if there is none); count of rho < 0 */
    dotsocp_i64 rho_hist[DOTSOCP_REPORT_BINS];   /* y = -rho          hist_negative_density.m:14 */
    double fq_max;   dotsocp_i64 fq_pos;    /* max over finite fq (-Inf if there is none); count of fq > 0 */
    dotsocp_i64 fq_hist[DOTSOCP_REPORT_BINS];    /* y = fq            hist_violation_q_2d.m:4 / _1d.m:4 */
    double cost;                            /* (1/n_nodes) * sum over nodes with rho > floor of (Ex^2 [+ Ey^2]) / rho */
    dotsocp_i64 nonfinite;                  /* NaN / Inf among the rho and fq values (0 for a healthy solve) */
} dotsocp_report;

/* The DOTSOCP_REPORT_BINS + 1 bin edges 10^linspace(-8, -1, 50).  Pure host arithmetic, no device. */
int dotsocp_report_edges(double edges[DOTSOCP_REPORT_BINS + 1]);
/* Call after finish().  rho0, rho1: model.rho0 / rho1 (ny x nx, host) as for dotsocp_recover_outputs.  layer_mass /
 * layer_neg (nt doubles each, or NULL): mean(rho(:,:,t)) and mean(min(rho(:,:,t), 0)) of every time layer.  Works on
 * one slab, `nslabs` slabs and dotsocp_create_multi (per-slab partial results are combined on the host).
 * DOTSOCP_ESTATE before finish(); DOTSOCP_EINVAL for a NULL rho0, rho1 or rep, and for a context with an RCCL
 * communicator attached (rank-local reports are not provided). */
int dotsocp_solution_report(dotsocp_ctx *ctx, const double *rho0, const double *rho1, dotsocp_report *rep,
                            double *layer_mass /* nt or NULL */, double *layer_neg /* nt or NULL */);

/* The geodesic's profile: what separates a geodesic from a curve that merely joins rho0 to rho1, per time node, in ONE pass
 * over the device-resident alpha (and the weight; q is not read); nothing grid-sized is written or crosses PCIe.
 * rho, Ex, Ey at a node are the values dotsocp_recover_outputs writes, bit for bit.  Coordinates: X = (double)i / (double)(nx - 1)
 * along the SECOND array index, Y = (double)j / (double)(ny - 1) along the first; 1-D: X along the only axis, every Y / Ey
 * term is 0.  Eleven sums per node layer t over its nodes, each term formed in IEEE doubles without contraction:
 *   0 mass  rho               3 mxx  (rho*X)*X        6 px   Ex          9 ent  rho > 0 ? rho*log(rho) : 0
 *   1 mx    rho*X             4 myy  (rho*Y)*Y        7 py   Ey         10 sq   rho*rho
 *   2 my    rho*Y             5 mxy  (rho*X)*Y        8 kin  rho > DOTSOCP_REPORT_RHO_FLOOR ? (Ex*Ex + Ey*Ey)/rho : 0
 * added in the order of dotsocp_solution_report's layer sums (it depends on (ny, nx) alone: two calls, any slab split and
 * any row pitch give the same bits; sums of row 0 are the sums behind its layer_mass, those of row 8 the ones behind its cost).
 * rho_max[t]: the largest finite rho of the layer (-Inf if there is none; a -0.0 counts as +0.0); n_support[t]: nodes with
 * rho > DOTSOCP_REPORT_RHO_FLOOR.
 * The summary (csrc/geodesic_summary.h states every operation and the NaN rule), with a[t] = (layer sum a)[t] / (double)(ny*nx):
 *   cost             (kin sums added in layer order) / (double)n_nodes: the bits of dotsocp_solution_report's cost
 *   energy_min, energy_max   over kin[t];  speed_spread = cost > 0 ? (energy_max - energy_min) / cost : 0
 *   com_defect       max_t |c[t] - ((1 - s) c[0] + s c[nt-1])|, c = (mx / mass, my / mass), s = (double)t / (double)(nt - 1)
 *   momentum_defect  max_t |(px[t], py[t]) - ((mx, my)[nt-1] - (mx, my)[0])|        (d/dt of the first moment is the momentum)
 *   entropy_defect   max(0, max over inner t of -((ent[t-1] + ent[t+1]) - 2 ent[t]))  (0: the entropy is convex in t)
 *   peak_excess      max(0, max_t rho_max[t] - max(rho_max[0], rho_max[nt-1]))
 *   nonfinite        layers whose mass is not finite */
#define DOTSOCP_GEO_SUMS 11
typedef struct {
    dotsocp_i64 nt, n_nodes;
    double cost, energy_min, energy_max, speed_spread, com_defect, momentum_defect, entropy_defect, peak_excess;
    dotsocp_i64 nonfinite;
} dotsocp_geodesic;
/* Call after finish() (DOTSOCP_ESTATE before it); inPALM / ALG2, PALM and acc-ADMM contexts, weighted and 1-D ones; one
 * slab, `nslabs` slabs and dotsocp_create_multi (per-slab layer rows are combined on the host in layer order).  rho0, rho1
 * as for dotsocp_solution_report.  sums: the layer sums as the kernel adds them (not divided by ny*nx).  DOTSOCP_EINVAL for
 * a NULL rho0, rho1 or res, and for a context with an RCCL communicator attached; a refused call leaves every output
 * untouched. */
int dotsocp_geodesic_profile(dotsocp_ctx *ctx, const double *rho0, const double *rho1, dotsocp_geodesic *res,
                             double *sums      /* nt x DOTSOCP_GEO_SUMS, quantity q of layer t at sums[t + nt*q], or NULL */,
                             double *rho_max   /* nt or NULL */, dotsocp_i64 *n_support /* nt or NULL */);

/* Where the mass goes: the velocity v = E / rho of the solved flow (the arrows of utils/show_movement_2d.m:31-40, masked
 * where rho is small) and particles carried along it -- the transport (Monge) map -- from the device-resident alpha.
 *
 * Inputs.  rho, Ex, Ey at the nodes (y, x, t) are the values dotsocp_recover_outputs writes, bit for bit (weight of
 *   wdot2d, rho0 / rho1 on the first / last layer included).
 * Coordinates.  Unit square, t in [0, 1].  x in [0, 1] runs along the SECOND array index (nx columns, node i at
 *   i / (nx - 1)), y along the first (ny rows); Ex is the x component; E = +rho v; v in domain lengths per unit time.
 * Velocity at a node.  ok = rho > rho_floor;  qx = Ex / rho;  vx = (ok && isfinite(qx)) ? qx : 0;  vy likewise: the
 *   field is finite everywhere, a NaN density gives v = 0.
 * Interpolation (clamp(u): u < 0 -> 0, u > 1 -> 1).  fx = x * (double)(nx - 1);  i = min((i64)floor(fx), nx - 2);
 *   a = fx - (double)i;  fy, j, c likewise with ny.  In one layer F:
 *       f0 = (1 - c) * F[j, i] + c * F[j + 1, i];   f1 = (1 - c) * F[j, i + 1] + c * F[j + 1, i + 1];
 *       lay = (1 - a) * f0 + a * f1
 *   and between the layers k, k + 1 of a time interval  v = (1 - b) * lay_k + b * lay_{k+1}  (both always evaluated).
 *   1-D drops y, j, c: lay = (1 - a) * F[i] + a * F[i + 1].
 * Integration.  Classical RK4, nsub >= 1 steps per time interval;  dt = dir / (double)((nt - 1) * nsub), hh = 0.5 * dt,
 *   h6 = dt / 6.0.  Forward (dir = +1): interval k = 0 .. nt - 2, sub-step s = 0 .. nsub - 1, stage fractions
 *   b = (double)(2 s + m) / (double)(2 nsub), m = 0, 1, 1, 2.  Backward (dir = -1): intervals nt - 2 down to 0, each
 *   entered at node k + 1, b = (double)(2 (nsub - s) - m) / (double)(2 nsub).
 *       k1 = v(x, y; b0)
 *       k2 = v(clamp(x + hh * k1x), clamp(y + hh * k1y); b1)
 *       k3 = v(clamp(x + hh * k2x), clamp(y + hh * k2y); b1)
 *       k4 = v(clamp(x + dt * k3x), clamp(y + dt * k3y); b2)
 *       x  = clamp(x + h6 * (((k1x + 2 * k2x) + 2 * k3x) + k4x))          (y likewise)
 *   Seeds outside [0, 1] are clamped before the first step; a non-finite seed is DOTSOCP_EINVAL.  n_clamped counts the
 *   particles for which the clamp at the END of some step changed a coordinate, each once.
 * The kernels are built without contraction of a * b + c, so a restatement of the above in IEEE doubles (advect.py)
 * gives the same bits.
 *
 * Both calls: after finish() (DOTSOCP_ESTATE before); inPALM / ALG2, PALM, acc-ADMM, weighted and 1-D contexts; one
 * slab, `nslabs` slabs and dotsocp_create_multi (the slab that owns cell layer k runs interval k, the particles travel
 * from slab to slab).  DOTSOCP_EINVAL: a NULL rho0 / rho1 / o / x, a NULL y on a 2-D context, n < 1, nsub < 1, a
 * direction other than +1 / -1, a context with an RCCL communicator attached. */
/* v = E / rho at the nodes; host arrays ny x nx x nt (1-D: nx x nt, vy ignored); either may be NULL */
int dotsocp_recover_velocity(dotsocp_ctx *ctx, const double *rho0, const double *rho1, double rho_floor,
                             double *vx, double *vy);

typedef struct { dotsocp_i64 n; int nsub; int direction; double rho_floor; } dotsocp_advect_opts;
/* x, y (n doubles, in: seeds, out: positions at t = 1, or t = 0 for direction -1; y NULL for 1-D);
 * traj_x / traj_y: n x nt column-major, position at every time NODE, indexed by node in both directions, or NULL;
 * n_clamped may be NULL */
int dotsocp_advect_particles(dotsocp_ctx *ctx, const double *rho0, const double *rho1, const dotsocp_advect_opts *o,
                             double *x, double *y, double *traj_x, double *traj_y, dotsocp_i64 *n_clamped);

/* Where the mass goes, literally: every particle of dotsocp_advect_particles carries a mass, and at the requested time
 * nodes the masses are deposited on the grid -- the push-forward of the seeded measure by the flow map, the displacement
 * (McCann) interpolant drawn next to the Eulerian rho layers.  With the masses rho0[j, i] on all nodes, l1 at node nt - 1
 * is the defect of the map: how far T#rho0 is from rho1.
 *
 * Trajectories.  Exactly those of dotsocp_advect_particles with the same rho0, rho1, n, nsub, direction, rho_floor and
 *   seeds: final x / y and n_clamped carry the same bits.
 * Deposit by integer accumulation: no result depends on the particle order, the launch shape or the slab split, and
 *   every frame holds the same number of units.
 *   Unit.       frexp((double)n * max_p mass[p]) = (f, e);  unit = 2^(e - 50).  The total stays below 2^51 units: every
 *               count converts to a double exactly.  (DOTSOCP_EINVAL if the product overflows or unit is not a normal double.)
 *   Units.      M_p = llrint(mass[p] / unit)                               (round half to even, = numpy.rint)
 *   Weights.    At a frame node the particle at (x, y) takes (i, a) and (j, c) as the velocity interpolation above does.
 *                   d00 = llrint(((1 - c) * (1 - a)) * (double)M_p)   -> count[j, i]
 *                   d10 = llrint((c * (1 - a)) * (double)M_p)         -> count[j + 1, i]
 *                   d01 = llrint(((1 - c) * a) * (double)M_p)         -> count[j, i + 1]
 *                   d11 = M_p - d00 - d10 - d01                       -> count[j + 1, i + 1]
 *               The last corner takes the remainder (it can be -1): a particle deposits exactly M_p units.  1-D:
 *               d0 = llrint((1 - a) * (double)M_p) -> count[i],  d1 = M_p - d0 -> count[i + 1].
 *   Counts.     SIGNED 64-bit sums of the above (64-bit integer atomic adds; two's-complement wrap is exact).  A count
 *               is reported as it is, also when a remainder of -1 falls on a node nothing else reaches.
 *   Frame.      frames[j, i, k] = (double)count[j, i] * unit  at node frame_nodes[k]; sum(count) = sum_p M_p in every frame.
 * l1[k] = mean over the ny * nx nodes of |frames[:, :, k] - rho(:, :, frame_nodes[k])|, rho as dotsocp_recover_outputs
 *   writes it; summed in the fixed order of dotsocp_solution_report's layer sums, so two calls and any slab split give the
 *   same bits.
 * The deposit is built without contraction of a * b + c: advect.push_forward restates it in numpy with the same bits.
 *
 * Valid where dotsocp_advect_particles is (after finish(); all loops, weighted, 1-D; one slab, `nslabs` slabs,
 * dotsocp_create_multi: the slab that owns a frame's node deposits it into a plane on its own device, the planes are
 * gathered on the host).  DOTSOCP_EINVAL: what dotsocp_advect_particles refuses, a NULL mass / frame_nodes / frames,
 * nf < 1, frame_nodes not strictly ascending in [0, nt), a mass that is negative or not finite, all masses zero. */
typedef struct { dotsocp_i64 n; int nsub; int direction; double rho_floor; dotsocp_i64 nf; } dotsocp_push_opts;
/* x, y: as for dotsocp_advect_particles (in: seeds, out: final positions; y NULL for 1-D).  mass: n doubles.
 * frame_nodes: nf node indices.  frames: ny x nx x nf doubles, y fastest (1-D: nx x nf).  n_clamped, unit (1 double),
 * l1 (nf doubles) may be NULL. */
int dotsocp_push_mass(dotsocp_ctx *ctx, const double *rho0, const double *rho1, const dotsocp_push_opts *o,
                      double *x, double *y, const double *mass, const dotsocp_i64 *frame_nodes, double *frames,
                      dotsocp_i64 *n_clamped, double *unit, double *l1);

/* How good the map is as a transport map: what it costs, whether the particles travel straight lines at constant speed,
 * and how that compares with the Eulerian `cost` of dotsocp_solution_report -- three numbers per particle from the march
 * of dotsocp_advect_particles, reduced on the device.  Over the whole march (total time 1) exact arithmetic gives
 * disp^2 <= len^2 <= action, the first with equality iff the path is straight, the second iff the speed is constant; for
 * the optimal map all three are |T(x) - x|^2 and their mass-weighted mean is W2^2.
 *
 * Trajectories.  Exactly those of dotsocp_advect_particles with the same rho0, rho1, n, nsub, direction, rho_floor and
 *   seeds: final x / y and n_clamped carry the same bits.
 * Per particle (no contraction of a * b + c; positions after the seed clamp and after the clamp at the END of a step, so
 *   a particle pressed against a wall adds only what it actually moved):
 *     start:      x0 = clamp(seed_x);  y0 = clamp(seed_y);  sq = 0.0;  len = 0.0
 *     every RK4 step, (xo, yo) the position before it and (x, y) the one after its end clamp, in march order (across
 *     intervals and slabs):
 *                 ex = x - xo;  ey = y - yo;  s2 = ex * ex + ey * ey  (1-D: s2 = ex * ex);
 *                 sq = sq + s2;  len = len + sqrt(s2)
 *     end:        dx = x - x0;  dy = y - y0;  disp2 = dx * dx + dy * dy  (1-D: dx * dx);  disp = sqrt(disp2);
 *                 action = sq * (double)((nt - 1) * nsub);  len2 = len * len;
 *                 r = 1.0 - disp / len;  detour = (len > 0.0 && r > 0.0) ? r : 0.0
 *   sqrt is the correctly rounded IEEE square root.
 * Masses.  One per particle, finite, >= 0, not all zero (the rules of dotsocp_push_mass); mass == NULL: every m_p = 1.0.
 * Sums.  S[q] = sum_p t_p with t_p = m_p, m_p * disp2_p, m_p * len2_p, m_p * action_p, m_p * disp_p, m_p * len_p, each added
 *   by the same tree, which depends on n alone (two calls and any slab split give the same bits):
 *     1. the particles are padded with terms +0.0 to a multiple of 256; block B holds particles 256 B .. 256 B + 255, its
 *        wavefront w the 64 of them from 64 w on;
 *     2. wavefront: for off = 32, 16, 8, 4, 2, 1:  t[l] = t[l] + t[l + off] for l < off;  the wavefront's sum is t[0];
 *     3. block: ((w0 + w1) + w2) + w3;
 *     4. blocks: thread u = 0 .. 255 adds  v_u = 0.0;  v_u = v_u + block[u + 256 k], k = 0, 1, ..  while u + 256 k is a
 *        block;  then for off = 128, 64, .., 1:  v[u] = v[u] + v[u + off] for u < off;  the total is v[0]
 *        (the tree of dotsocp_solution_report's layer sums over its tiles).
 *   mass = S[0];  cost_map = S[1] / mass;  cost_length = S[2] / mass;  cost_action = S[3] / mass;  disp_mean = S[4] / mass;
 *   len_mean = S[5] / mass.  No floating-point atomic anywhere.
 * Order-free (integer atomics): disp_max, len_max, detour_max over ALL n particles (geometry, not mass); n_still = particles
 *   with len == 0.0; detour_hist = counts of detour_p over the edges of dotsocp_report_edges with the bin rule of
 *   dotsocp_solution_report (edges[j] <= y < edges[j+1], the last bin also y == edges[last], values below edges[0] -- a
 *   straight path's 0 among them -- in no bin); detour_over = count of detour_p > edges[last] = 0.1: paths more than
 *   about 10 % longer than straight.
 * advect.map_report restates all of it in numpy with the same bits.
 *
 * Valid where dotsocp_advect_particles is (after finish(); all loops, weighted, 1-D; one slab, `nslabs` slabs,
 * dotsocp_create_multi: sq and len travel with the particles, the slab that holds them after the last interval receives
 * the seeds and masses and reduces).  DOTSOCP_EINVAL: what dotsocp_advect_particles refuses, a NULL rep, a mass that is
 * negative or not finite, all masses zero. */
typedef struct {
    dotsocp_i64 n, n_clamped, n_still;
    double mass;                                 /* sum of the masses */
    double cost_map, cost_length, cost_action;   /* mass-weighted means of disp^2 <= len^2 <= action */
    double disp_mean, len_mean;                  /* mass-weighted means of disp, len */
    double disp_max, len_max, detour_max;        /* over all n particles */
    dotsocp_i64 detour_hist[DOTSOCP_REPORT_BINS];
    dotsocp_i64 detour_over;
} dotsocp_map_report_t;
/* o, x, y: as for dotsocp_advect_particles (x, y in: seeds, out: final positions; y NULL for 1-D).  mass: n doubles or NULL.
 * disp, len, action: n doubles each, the per-particle values; each may be NULL. */
int dotsocp_map_report(dotsocp_ctx *ctx, const double *rho0, const double *rho1, const dotsocp_advect_opts *o,
                       double *x, double *y, const double *mass, dotsocp_map_report_t *rep, double *disp, double *len,
                       double *action);

/* A lower bound on the transport cost from the potential: every other judgement of a solve (KKT history, report, map
 * report) lives inside the discretised dynamic problem; this one certifies the quantity asked for.  For ANY function psi0 on
 * the nodes and psi1(y) = min_x psi0(x) + |x - y|^2 / 2 one has psi1(y) - psi0(x) <= |x - y|^2 / 2 for every pair of nodes,
 * hence 2 (sum psi1 b - sum psi0 a) <= W2^2(a, b) for the node histograms a = rho0 / sum(rho0), b = rho1 / sum(rho1) --
 * whatever state the solve is in.  With psi0 = phi(t = 0) this is the Hopf-Lax transform of the potential to t = 1; the
 * mirror transform of phi(t = 1) back to t = 0 gives a second bound.  What is certified is the DISCRETE STATIC cost
 * between the node histograms (it differs from the continuous W2^2 by O(h)), up to the rounding of the sums.
 *
 * One axis of n nodes, h = 1.0 / (double)(n - 1), w = (0.5 * h) * h:
 *     forward    out[j] = min_i ( in[i] + (double)((i - j)^2) * w )        backward   out[i] = max_j ( in[j] - (double)((i - j)^2) * w )
 *   the square exactly in integers; each candidate one product and then one sum or difference, separately rounded; on ties
 *   the SMALLEST index wins; the value is the candidate at the winning index (so the sign of a zero follows the index).
 *   Before the transform every non-finite input (NaN, +-Inf) counts as +Inf (forward) resp. -Inf (backward); a line without a
 *   finite entry gives index 0.
 * Two axes: the pass along x (every row y: T(y, x'), winner ix(y, x')) followed by the pass along y on its result (every
 *   column x': value at (y', x'), winner iy(y', x')).  The winning node of (y', x') is (iy, ix[iy, x']), returned as the flat
 *   index iy + ny * ix[iy, x'] (y fastest, int32).  1-D problems: one pass, the index itself.
 * Inputs.  phi0, phi1: the first and last node layer of phi in original units, dScale * phi (recoverOrgVar,
 *   solver_dotsocp2d.m:368-386: one product per entry).  rho0, rho1 (ny x nx, host; 1-D: nx) as for dotsocp_solution_report.
 * Results.  H = forward(phi0), B = backward(phi1).  Every sum below runs over the nodes in memory order (y fastest) and is
 *   added by the tree of dotsocp_map_report ("Sums", the node index in the place of the particle index): two calls and any
 *   slab split give the same bits.  m0 = sum rho0, m1 = sum rho1, and with  a0 = (sum phi0 rho0) / m0,
 *   a1 = (sum phi1 rho1) / m1:
 *     dual_raw  = 2.0 * (a1 - a0)
 *     bound_fwd = 2.0 * ((sum H rho1) / m1 - a0)          bound_bwd = 2.0 * (a1 - (sum B rho0) / m0)
 *     bound     = bound_bwd > bound_fwd ? bound_bwd : bound_fwd
 *   The Hopf-Lax gap at t = 1, g = phi1 - H: gap1_max / gap1_min over the finite g (a -0.0 counts as +0.0; -Inf / +Inf if there
 *   is none), gap1_mean = (sum |g| rho1) / m1; the same for g = phi0 - B at t = 0 with rho0 and m0 (gap0_*).
 *     map_cost_bwd = (sum rho0 d2) / m0,  d2 = ex * ex + ey * ey,  ex = (double)(x - tx) * hx,  ey = (double)(y - ty) * hy
 *   (1-D: d2 = ex * ex) with (ty, tx) the backward winner of node (y, x), hx = 1.0 / (double)(nx - 1), hy likewise: the cost of
 *   the map the potential itself names.  nonfinite = the non-finite entries of phi0 and phi1; the sums take phi as it is.
 *   No contraction of a * b + c anywhere: dual.py restates all of it in numpy with the same bits.
 * Optional outputs (host; each is written only when its pointer is not NULL): H, B: ny x nx doubles; arg_fwd, arg_bwd: ny x nx
 *   ints, the flat winners.  1-D: nx entries each.
 *
 * After finish() (DOTSOCP_ESTATE before); inPALM / ALG2, PALM and acc-ADMM contexts, 1-D and 2-D; one slab, `nslabs` slabs and
 * dotsocp_create_multi (phi1 lives on the last slab: that one layer is brought to the first slab's device, where all the
 * work runs).  DOTSOCP_EINVAL, with res and the optional outputs untouched: a NULL rho0 / rho1 / res, a context with an RCCL
 * communicator attached, a weighted context (its cost is not the Euclidean one: the bound would be wrong), an axis of more
 * than 2^20 nodes, m0 or m1 not positive and finite. */
typedef struct {
    dotsocp_i64 n_nodes;                    /* ny * nx (1-D: nx) */
    dotsocp_i64 nonfinite;                  /* NaN / Inf among phi0 and phi1 (0 for a healthy solve) */
    double mass0, mass1;                    /* m0, m1 */
    double dual_raw, bound_fwd, bound_bwd, bound;
    double gap1_max, gap1_min, gap1_mean;   /* phi1 - H at t = 1 */
    double gap0_max, gap0_min, gap0_mean;   /* phi0 - B at t = 0 */
    double map_cost_bwd;
} dotsocp_dual;
int dotsocp_dual_bound(dotsocp_ctx *ctx, const double *rho0, const double *rho1, dotsocp_dual *res, double *H, double *B,
                       int *arg_fwd, int *arg_bwd);

/* An upper bound on the same quantity, so that bound <= W2^2(a, b) <= upper brackets it with both ends certified: a few
 * log-domain Sinkhorn sweeps for the cost c(x, y) = |x - y|^2 / 2 at a temperature eps of a fraction of h^2, started from the
 * solve's own potential, rounded to an exactly feasible plan by the scheme of Altschuler, Weed and Rigollet.  The Gaussian
 * kernel factorises over the axes, so one Sinkhorn update is the soft-min version of the two min-plus passes above -- a
 * log-sum-exp in the place of the min -- and the row masses, the column masses and the cost sum P c of the plan are node sums
 * of such transforms: no n x n object exists.  What is certified is again the discrete static cost between the node
 * histograms, up to the rounding of the sums.
 *
 * Setting.  a = rho0 / m0, b = rho1 / m1 (one division per node), m0 = sum rho0, m1 = sum rho1; every sum runs over the nodes
 *   in memory order by the tree of dotsocp_map_report ("Sums").  eps = (eps_h2 * hx) * hy (1-D: (eps_h2 * hx) * hx),
 *   hx = 1.0 / (double)(nx - 1), ieps = 1.0 / eps.  Per axis of n nodes w = (0.5 * h) * h as above.
 * Soft pass along one axis, with a prior mean pm (zeros where none is named).  For output j over the candidates
 *   c_i = in[i] + (double)((i - j)^2) * w, the square exact in integers, non-finite inputs counting as +Inf:
 *     m = min_i c_i                                         (the forward pass above)
 *     s = sum_i e_i,   q = sum_i e_i * ((double)((i - j)^2) * w + pm[i]),   e_i = exp((m - c_i) * ieps)
 *   both added in ascending i into one accumulator per output that starts at 0.0 -- tiles and chunks change no bit;
 *     out[j] = m - eps * log(s),   mean[j] = q / s;     a line without a finite entry: out = +Inf, mean = 0.
 *   A term may be skipped only where e_i is exactly +0.0 (the argument of exp below -746).
 * Two axes: the pass along x (every row y, no prior mean) and then the pass along y on its values with its means as the
 *   prior mean: mean(j) is the softmax-weighted mean of |x_i - y_j|^2 / 2.  1-D problems: one pass.  The whole transform:
 *   S(in) -> (value, mean).  No contraction of a * b + c anywhere; the device's exp and log are the only operations that
 *   upper.py, which restates all of it in numpy, does not reproduce bit for bit.
 * Sweeps.  la = -(eps * log(a)), lb = -(eps * log(b)); a zero mass gives +Inf: that node drops out.  Start: f = -(dScale *
 *   phi(t = 0)) (start = 1), f_start (start = 2) or zeros (start = 0); a non-finite entry of the start is counted
 *   (nonfinite) and counts as 0.0.  One sweep: g = S(la - f), f_new = S(lb - g),
 *     defect_k = sum_i (a_i > 0 ? a_i * |exp((f_i - f_new_i) * ieps) - 1.0| : 0.0)
 *   -- the L1 distance of the plan's row sums from a; it may be +Inf --, then f = f_new.  The sweeps stop after max_sweeps of
 *   them, or behind the first with defect_k <= defect_tol (one scalar travels to the host per sweep).  Then g = S(la - f).
 * Rounding.  f~ = S(lb - g), f' = f~ < f ? f~ : f;   (g~, E) = S(la - f'), g' = g~ < g ? g~ : g;   f^ = S(lb - g').  The kept
 *   plan P_ij = a_i b_j exp((f'_i + g'_j - c_ij) / eps) has the row sums r_i = a_i * exp((f'_i - f^_i) * ieps) and the column
 *   sums k_j = b_j * exp((g'_j - g~_j) * ieps) (0.0 where the mass is zero), both below the marginals; what is missing is
 *   er_i = max(a_i - r_i, 0.0), ec_j = max(b_j - k_j, 0.0).  Node sums: kept = sum k_j, cost_kept = sum k_j * E_j, and with
 *   the node coordinates px = (double)x * hx, py = (double)y * hy (1-D: px = 0.0), p2 = px * px + py * py:
 *   R0, R1x, R1y, R2 = sum er * (1, px, py, p2) and C0, C1x, C1y, C2 = the same of ec.
 *     fill = R0 < C0 ? R0 : C0
 *     cost_fill = fill > 0 ? 0.5 * ((R2 * C0 + R0 * C2) - 2.0 * (R1x * C1x + R1y * C1y)) / fill : 0.0
 *     upper = 2.0 * (cost_kept + cost_fill)
 *   The plan P + er ec^T / fill has the marginals a and b for ANY f, g, so upper is a bound whatever state the solve is in.
 * Results.  f, g: f', g';  E;  er, ec: ny x nx doubles each (1-D: nx);  defects: max_sweeps doubles, NaN behind the last
 *   sweep made;  defect_first / defect_last: of the first / last sweep made (NaN without one);  zero0 / zero1: the nodes
 *   with rho0 == 0 / rho1 == 0.  Every optional output (all but res) is written only when its pointer is not NULL.
 *
 * dotsocp_plan_bound is stateless like dotsocp_image_density: host arrays ny x nx, y fastest (1-D: ny = 1), on HIP device
 * `device`.  dotsocp_upper_bound runs on the first slab's device of a finished context and is valid where
 * dotsocp_dual_bound is (DOTSOCP_ESTATE before finish()).  DOTSOCP_EINVAL, with all outputs untouched: what
 * dotsocp_dual_bound refuses (a NULL rho0 / rho1 / res, a weighted context, an RCCL communicator, an axis of fewer than 2 or
 * more than 2^20 nodes, m0 or m1 not positive and finite), a NULL opts, an entry of rho0 or rho1 that is negative or not
 * finite, eps_h2 not positive and finite, max_sweeps < 0, start outside 0 .. 2, start = 2 without f_start, and for the
 * stateless call start = 1. */
typedef struct {
    double eps_h2;                  /* eps in units of hx * hy; 0.25 is a good start */
    dotsocp_i64 max_sweeps;
    double defect_tol;              /* stop behind the first sweep with defect <= defect_tol (0: never early) */
    int start;                      /* 0: zeros, 1: -(dScale * phi(t = 0)), 2: f_start */
} dotsocp_upper_opts;
typedef struct {
    dotsocp_i64 n_nodes, sweeps, zero0, zero1, nonfinite;
    double eps, mass0, mass1;
    double upper, cost_kept, cost_fill, kept, fill;
    double defect_first, defect_last;
} dotsocp_upper;
int dotsocp_plan_bound(const double *rho0, const double *rho1, dotsocp_i64 ny, dotsocp_i64 nx, const double *f_start,
                       const dotsocp_upper_opts *o, dotsocp_upper *res, double *f, double *g, double *E, double *er,
                       double *ec, double *defects, int device);
int dotsocp_upper_bound(dotsocp_ctx *ctx, const double *rho0, const double *rho1, const double *f_start,
                        const dotsocp_upper_opts *o, dotsocp_upper *res, double *f, double *g, double *E, double *er,
                        double *ec, double *defects);

/* The transport map of that plan.  The bound above builds a feasible plan and returns its cost; the plan also determines a
 * map, again without any n x n object: T(x_i) = E[y | x_i], the barycentric projection of the plan P + er ec^T / fill, and
 * the displacement interpolant ((1 - tau) Id + tau T)# rho0 as frames.  The map is a projection: it is NOT measure preserving
 * (T# rho0 is close to rho1 only as far as the plan is close to a deterministic one); `spread` says how far it is.
 *
 * Moment pass.  The soft pass of dotsocp_plan_bound ("Soft pass") with two more accumulators of the same kind beside s and q,
 *   both from 0.0 and added in ascending i, with h = 1.0 / (double)(n - 1):
 *     qa = sum_i e_i * ((double)(i - j) * h)      candidate minus output along the pass's axis, the difference exact
 *     qb = sum_i e_i * pb[i]                      a prior displacement of the other axis, carried through
 *   da[j] = qa / s, db[j] = qb / s, 0 on a line without a finite entry.  A term is skipped where the plain pass skips it.  out
 *   and mean carry the bits of the plain pass.  Two axes: the pass along x gives (value, mean, da); the pass along y takes its
 *   mean as pm and its da as pb:  kc = mean, kdy = da, kdx = db.  1-D: one pass, kc = mean, kdy = da, kdx = 0.
 * Map.  dotsocp_plan_bound runs as it is, except that the last transform f^ = S(lb - g') is a moment pass: its softmax
 *   weights at source node i are the conditional law of the kept plan P, so kc, kdx, kdy are the kept row's mean cost and mean
 *   displacement.  The fill row er_i ec^T / fill has closed-form moments from the sums of "Rounding":
 *     kappa = fill > 0 ? C0 / fill : 0.0;   mx = C1x / C0, my = C1y / C0, m2 = C2 / C0  (each 0.0 if C0 == 0)
 *   Per source node i in memory order, with px, py, p2 as above:
 *     wk = r_i;  wf = er_i * kappa;  row = wk + wf                                (the row sum of the plan)
 *     fdx = mx - px;  fdy = my - py;  fc = 0.5 * ((m2 - 2.0 * (px * mx + py * my)) + p2)
 *     Dx = (wk * kdx + wf * fdx) / row;  Dy = (wk * kdy + wf * fdy) / row;  C = (wk * kc + wf * fc) / row
 *     d2 = Dx * Dx + Dy * Dy;  spread_i = 2.0 * C - d2  (not clamped);  disp = sqrt(d2)
 *   row == 0 (a node without mass): Dx = Dy = C = spread_i = disp = 0.  T(x_i) = x_i + (Dx, Dy); C is the conditional mean
 *   cost, spread_i the trace of the conditional covariance of y given x_i.  Sums (the tree of "Sums", no floating-point atomic):
 *     rows = sum row;  map_cost = sum row * d2;  spread = sum row * spread_i;  cost_rows = 2.0 * sum row * C;
 *     disp_mean = sum row * disp;  disp_max = max disp  (order-free: an integer atomic on the bit pattern)
 *   Exact arithmetic gives rows = 1, cost_rows = upper and cost_rows = map_cost + spread: the certified bound splits into the
 *   cost of a deterministic map and the blur around it (the entropic blur plus whatever splitting the histograms force).
 * Frames.  unit: the rule of dotsocp_push_mass with n = the node count and the largest entry of rho0 (as given, not
 *   normalised: a frame compares with rho directly);  M_i = llrint(rho0_i / unit).  For every tau_k the particle of node i
 *   stands at  X = clamp(px + tau_k * Dx),  Y = clamp(py + tau_k * Dy)  (clamp to [0, 1]) and deposits its M_i units by the
 *   weights and counts of dotsocp_push_mass;  frames[:, :, k] = (double)count * unit.  Every frame holds sum M_i units.
 *   n_clamped: the nodes with M_i > 0 whose position a clamp changed in some frame, each once.
 * No contraction of a * b + c anywhere; upper.barycentric_map and upper.plan_frames restate all of it in numpy.
 *
 * dotsocp_plan_map is dotsocp_plan_bound with the map: res and its six optional arrays come back with the same bits.  Dx, Dy,
 * C, row, spread: ny x nx doubles each, y fastest, each optional (1-D: the displacement comes back in Dx, Dy is ignored).
 * taus: nf doubles in [0, 1], any order, repeats allowed;  frames: ny x nx x nf;  nf = 0 with both NULL is allowed.
 * DOTSOCP_EINVAL, with all outputs untouched: what dotsocp_plan_bound refuses, a NULL map_res, nf < 0, nf > 0 without taus or
 * without frames, a tau that is not finite or outside [0, 1] (dotsocp_upper_map: nf > 0 without frame_nodes, a frame node outside
 * [0, nt)), a rho0 for which the unit rule fails. */
typedef struct {
    double rows, map_cost, spread, cost_rows, disp_mean, disp_max;
    dotsocp_i64 n_clamped;          /* 0 without frames */
    double unit;
} dotsocp_plan_map_t;
int dotsocp_plan_map(const double *rho0, const double *rho1, dotsocp_i64 ny, dotsocp_i64 nx, const double *f_start,
                     const dotsocp_upper_opts *o, dotsocp_upper *res, double *f, double *g, double *E, double *er,
                     double *ec, double *defects, dotsocp_plan_map_t *map_res, double *Dx, double *Dy, double *C,
                     double *row, double *spread, const double *taus, dotsocp_i64 nf, double *frames, int device);
/* The context call: valid exactly where dotsocp_upper_bound is, and equal to dotsocp_plan_map where both apply (start = 1
 * against f_start = -(dScale * phi(t = 0))).  The frames stand at time nodes: tau_k = (double)frame_nodes[k] / (double)(nt - 1),
 * nodes in [0, nt), any order, repeats allowed.  l1[k] (nf doubles, may be NULL) = the mean over the nodes of
 * |frames[:, :, k] - rho(:, :, frame_nodes[k])|, formed by the kernel and in the order of dotsocp_push_mass's l1 on the slab
 * that owns the node (the counts plane travels there through the host): the distance between the dynamic solve's density and
 * the static displacement interpolant. */
int dotsocp_upper_map(dotsocp_ctx *ctx, const double *rho0, const double *rho1, const double *f_start,
                      const dotsocp_upper_opts *o, dotsocp_upper *res, double *f, double *g, double *E, double *er,
                      double *ec, double *defects, dotsocp_plan_map_t *map_res, double *Dx, double *Dy, double *C,
                      double *row, double *spread, const dotsocp_i64 *frame_nodes, dotsocp_i64 nf, double *frames,
                      double *l1);

/* Pictures of the density evolution on the device: what utils/show_evolution_2d.m, show_movement_2d.m and
 * export_evolution_2d.m draw from the downloaded outputs -- gray or colour-mapped frames, filled log-spaced levels, the
 * arrows of the flux -- formed from the device-resident alpha.  A frame reads the two alpha layers around its node; what
 * crosses PCIe is one byte (three with a colour table) per pixel.  rho, Ex, Ey at a node are the values
 * dotsocp_recover_outputs writes, bit for bit.
 *
 * Range.  vmax = the maximum of rho over all nodes of all nt layers (rho0 and rho1 included) that are finite and not set
 *   in `barrier`; rho_min = the minimum over the same set (a -0.0 counts as +0.0; +Inf if the set is empty); nonfinite =
 *   the unmasked nodes whose rho is NaN or +-Inf; masked = the masked nodes (all layers).  The reference sets barrier nodes
 *   to Inf BEFORE it takes the maximum (show_evolution_2d.m:36,52), which makes its own scale infinite; that is not
 *   followed here.  opts.vmax > 0 fixes the scale (to compare runs): then only rho_min and the counts come from the pass.
 *   A scale that is not a positive finite number is DOTSOCP_EINVAL; nothing is written.
 * Index of a node, by opts.mode (no contraction of a * b + c; render.py restates it with the same bits):
 *   DOTSOCP_RENDER_LINEAR    imshow(rho, [0, vmax]) (show_evolution_2d.m:56):  i = 0 for rho <= 0 or NaN, else
 *                            i = min(255, floor((rho / vmax) * 256.0)): one IEEE division, one product; +Inf gives 255.
 *   DOTSOCP_RENDER_INVERTED  vmax - rho (export_evolution_2d.m:91-92):  255 - i of the linear mode.
 *   DOTSOCP_RENDER_LEVELS    contourf / contour of rho * (255 / vmax) over exp(linspace(0, log(255), n))
 *                            (show_evolution_2d.m:58-65), filled, no lines:  s = rho * k with k = 255.0 / vmax formed once
 *                            on the host;  i = the number of levels[j] <= s, in 0 .. nlevels; NaN gives 0.  `levels`:
 *                            nlevels strictly ascending doubles, 1 <= nlevels <= 254, made by the caller (render.log_levels);
 *                            the device evaluates no exp and compares against these doubles.
 *   In every mode a node set in `barrier` gets opts.barrier_index (0 .. 255) instead.
 * Picture.  nf frame nodes in [0, nt), in any order, repeats allowed.  image: uint8 [nf][ny][nx][channels], x fastest --
 *   the row-major picture every image writer takes, an image row being a fixed y, as imshow(rho(:,:,t)) shows it.
 *   channels = 1: the index itself;  channels = 3: lut[3 * i + 0 .. 2] of the caller's 256 x 3 table (any table: gray, a
 *   ramp, a colour map of the caller's).  1-D problems: image [nf][nx][channels]; with all nodes requested this is the
 *   space-time diagram.
 * Arrows (show_movement_2d.m:31-33,45-46,56), asked for with skip_y >= 1 and skip_x >= 1 (both 0: none).  mvx, mvy:
 *   doubles [nf][mx][my], y fastest, my = ceil(ny / skip_y), mx = ceil(nx / skip_x): Ex, Ey at the nodes y = 0, skip_y, ..,
 *   x = 0, skip_x, .. of every frame node -- the bits of dotsocp_recover_outputs, except +0.0 where
 *   rho < vmax * mask_frac (strict; the product is formed once on the host; the reference's mask_frac is 0.01; a NaN rho
 *   keeps its arrow).  The reference derives both skips from nx (:21,27); here there is one per axis.  1-D problems: mvx
 *   alone, [nf][mx], with skip_x along the axis (skip_y >= 1 is only the request), my = 1.
 * barrier: ny x nx bytes, y fastest (1-D: nx), non-zero = masked; or NULL.
 *
 * After finish() (DOTSOCP_ESTATE before); inPALM / ALG2, PALM, acc-ADMM, weighted and 1-D contexts; one slab, `nslabs`
 * slabs and dotsocp_create_multi: a frame is rendered by the slab that owns its node and lands at its position in the
 * request.  DOTSOCP_EINVAL, before anything is written: a NULL rho0 / rho1 / opts / frame_nodes / image (info may be NULL), nf < 1, a
 * frame node outside [0, nt), a mode other than the three, nlevels outside 1 .. 254 or a NULL `levels` in LEVELS mode,
 * levels not strictly ascending (a NaN among them), channels other than 1 or 3, channels = 3 without lut, barrier_index
 * outside 0 .. 255, a negative skip, exactly one skip zero, arrows without mvx (2-D: or mvy), a context with an RCCL
 * communicator attached. */
enum { DOTSOCP_RENDER_LINEAR = 0, DOTSOCP_RENDER_INVERTED = 1, DOTSOCP_RENDER_LEVELS = 2 };
typedef struct {
    int mode;                       /* DOTSOCP_RENDER_* */
    int channels;                   /* 1 or 3 */
    dotsocp_i64 nf;                 /* frame nodes */
    int nlevels;                    /* LEVELS mode: 1 .. 254 */
    int barrier_index;              /* index of the nodes set in `barrier`, 0 .. 255 */
    double vmax;                    /* > 0: the scale; else the maximum found */
    dotsocp_i64 skip_y, skip_x;     /* arrows: both >= 1; none: both 0 */
    double mask_frac;               /* arrows vanish where rho < vmax * mask_frac */
} dotsocp_render_opts;
typedef struct {
    double vmax, rho_min;           /* the scale used; min over the finite unmasked rho */
    dotsocp_i64 nonfinite, masked;
    dotsocp_i64 my, mx;             /* arrow nodes per frame along y, x (0 without arrows) */
} dotsocp_render_info;
int dotsocp_render_evolution(dotsocp_ctx *ctx, const double *rho0, const double *rho1, const dotsocp_render_opts *opts,
                             const dotsocp_i64 *frame_nodes, const double *levels, const unsigned char *lut,
                             const unsigned char *barrier, unsigned char *image, double *mvx, double *mvy,
                             dotsocp_render_info *info);

/* Multilevel transfer on the device: socp/dot2d/utils/jump_nextLevel.m:5-16 with
 * interpolate.m:20-84, between the finished context `coarse` and the context `fine` of the next level (created
 * from the fine level's InitialScaling scalars, c and weight uploaded, begin() not yet called; grid
 * 2 (n - 1) + 1 per dimension).  Fills phi, q, alpha, z, beta of `fine` exactly as recoverOrgVar ->
 * jump_nextLevel -> InitialScaling -> upload would.  Either context may be cut into in-process time slabs
 * (dotsocp_create / dotsocp_create_multi, any two slab counts and placements): a fine slab gathers the coarse
 * layers it interpolates from out of the coarse slabs that own them (peer copies).  Contexts with an RCCL
 * communicator attached are refused (DOTSOCP_EINVAL): their levels exchange state through the host. */
int dotsocp_jump_next_level(dotsocp_ctx *coarse, dotsocp_ctx *fine);

/* Weight pyramid: model.weight of every level of one weighted multilevel solve (socp/wdot2d/solver_wdotsocp2d.m:173-191),
 * resident on the device.  The finest level is filled once -- from a host array, or from the two 2-D arrays the barrier
 * and radial generators repeat over t -- the coarser ones are restricted from it on the device, and each level's context
 * takes its weight by a device-to-device copy: no grid-sized weight array is built, restricted or reduced on the host.
 * A level is stored in the reference layout [q0; bx; by] of its grid. */
typedef struct dotsocp_weights dotsocp_weights;

/* Grid of the FINEST level and the number of levels.  Level levels-1 is the finest; level l-1 has (n+1)/2 points per axis
 * of level l.  levels > 1 needs 2^k*m+1 sizes on every axis down to the coarsest level (ny, nx, nt >= 2 always).
 * NULL + last_error otherwise (and without a device). */
dotsocp_weights *dotsocp_weights_create(int device, dotsocp_i64 ny, dotsocp_i64 nx, dotsocp_i64 nt, int levels);
void dotsocp_weights_destroy(dotsocp_weights *w);

/* Pure host arithmetic, no device: Nq of level `level`.  -1 for a bad level, or a grid that cannot be halved that often. */
dotsocp_i64 dotsocp_weights_len(dotsocp_i64 ny, dotsocp_i64 nx, dotsocp_i64 nt, int levels, int level);

/* Finest level from a host array in the reference layout [q0; bx; by] ... */
int dotsocp_weights_set(dotsocp_weights *w, const double *weight);
/* ... or from weightX (ny x (nx-1)) and weightY ((ny-1) x nx), column-major, repeated over the nt time nodes, with 1 on
 * every time edge (examples/wdot2d/get_weight_by_barrier.m:20-33, gene_weight_circle.m).  Either call invalidates the
 * coarser levels. */
int dotsocp_weights_set_space(dotsocp_weights *w, const double *weightX, const double *weightY);

/* Fill levels levels-2 .. 0 (DOTSOCP_ESTATE before a set).  log_mean = 0: socp/wdot2d/utils/downSample_q.m:4-21;
 * log_mean = 1: downSample_barrier.m:4-21 (restriction of log(weight), then exp). */
int dotsocp_weights_restrict(dotsocp_weights *w, int log_mean);

/* mean(log10(weight + 1e-10)) of a level (solver_wdotsocp2d.m:312-316).  The order of the additions is fixed: two calls
 * give the same bits.  A level that has not been filled: DOTSOCP_ESTATE (also for download / upload_weight_from). */
int dotsocp_weights_log10_mean(dotsocp_weights *w, int level, double *mean);

int dotsocp_weights_download(dotsocp_weights *w, int level, double *host);

/* model.weight of `ctx` <- level `level`, device to device; replaces dotsocp_upload(ctx, DOTSOCP_F_WEIGHT, ...).  Serves
 * one slab, `nslabs` slabs on one device and dotsocp_create_multi (each slab takes its layers, by peer copies where the
 * devices differ: straight into place, or -- rows pitched -- through a staging buffer on the slab's device.  STATUS: as
 * for dotsocp_create_multi, copies between DIFFERENT devices have never run on hardware; DOTSOCP_WEIGHT_STAGE=1 takes
 * the staged form on one device).  DOTSOCP_EINVAL: an unweighted or 1-D context, a grid that is not the level's, a context with an RCCL
 * communicator attached; DOTSOCP_ESTATE: after begin(). */
int dotsocp_upload_weight_from(dotsocp_ctx *ctx, dotsocp_weights *w, int level);

/* ===================================================================================
 * Problems given as pictures (csrc/image.hip, csrc/image_table.h; twins: dot-socp_amd/images.py)
 * ===================================================================================
 * MATLAB's imresize(img, [h_out w_out]) -- bicubic (a = -0.5), antialiased when shrinking, separable -- and the densities
 * the reference's image-based examples build with it (examples/dot2d/get_example_from_images.m, gene_example5.m,
 * gene_example_DOTmark_4stitch.m).  Pictures are column-major like everything else: h fastest, then w, planes slowest.
 * The calls take HOST pointers; the work runs on the device in one go, the result is downloaded once.
 *
 * One pass along an axis: out[r] = sum_k weights[r][k] * in[indices[r][k]], k ascending, product and sum separately
 * rounded (no fused multiply-add).  The axis with the smaller scale n_out / n_in goes first, on a tie the rows.  uint8
 * pictures store r = floor(acc), r + 1 if acc - r >= 0.5, clamped to 0 .. 255, after EACH pass; double pictures store acc.
 * A pass of scale 1 runs like any other (its table is the identity).
 *
 * The table of a pass: s = n_out / n_in; kernel f = 1.5|x|^3 - 2.5|x|^2 + 1 on [0, 1], -0.5|x|^3 + 2.5|x|^2 - 4|x| + 2 on
 * (1, 2], width 4; for s < 1 the kernel s f(s x) of width 4 / s.  Output x = 1 .. n_out sits at u = x / s + 0.5 (1 - 1 / s),
 * takes P = ceil(width) + 2 positions from floor(u - width / 2) on, weights f(u - position) divided by their sum (Neumaier's compensated
 * sum, positions ascending: a row then sums to 1 within 2 ulp however many taps it has), positions
 * mirrored through [1 .. n_in, n_in .. 1]; columns that are zero in every row are dropped.  Pure host arithmetic, no device.
 * dotsocp_imresize_taps returns P, the room per row that dotsocp_imresize_table needs (n_out * P doubles resp. ints); the
 * table is stored [n_out][*taps] with the taps that remain, indices 0-based.  Lengths: 1 .. DOTSOCP_IMG_MAX_LEN. */
#define DOTSOCP_IMG_U8 0
#define DOTSOCP_IMG_F64 1
#define DOTSOCP_IMG_MAX_LEN 65536
int dotsocp_imresize_taps(dotsocp_i64 n_in, dotsocp_i64 n_out);
int dotsocp_imresize_table(dotsocp_i64 n_in, dotsocp_i64 n_out, double *weights, int *indices, int *taps);

/* out (h_out x w_out x planes) <- imresize(in (h_in x w_in x planes)); dtype DOTSOCP_IMG_U8 (unsigned char) or
 * DOTSOCP_IMG_F64 (double), planes 1 .. 4.  DOTSOCP_EINVAL, with `out` untouched: a length outside 1 .. DOTSOCP_IMG_MAX_LEN,
 * planes outside 1 .. 4, NULL, out == in, another dtype, a device ordinal out of range.  No device: DOTSOCP_ENODEVICE. */
int dotsocp_imresize(void *out, const void *in, int dtype, dotsocp_i64 h_in, dotsocp_i64 w_in, dotsocp_i64 planes,
                     dotsocp_i64 h_out, dotsocp_i64 w_out, int device);

#define DOTSOCP_IMG_SINGLE 0
#define DOTSOCP_IMG_STITCH4 1
typedef struct {
    const unsigned char *pix;      /* h x w x planes */
    dotsocp_i64 h, w, planes;      /* planes 1 (gray) or 3 (R, G, B) */
} dotsocp_image;
typedef struct {
    dotsocp_i64 ny, nx;            /* the density's grid, each 2 .. DOTSOCP_IMG_MAX_LEN */
    int layout;                    /* DOTSOCP_IMG_SINGLE: one picture; DOTSOCP_IMG_STITCH4: four */
    int reverse;                   /* SINGLE only: (255 - v) / 255 instead of v */
    double lower_bound;            /* finite, > -1 */
} dotsocp_image_opts;

/* rho (ny x nx doubles) <- the normalised density of the picture(s).
 *   SINGLE   uint8 resize to (ny - 1) x (nx - 1) per plane; three planes: gray = 0.298936021293775 R + 0.587043074451121 G +
 *            0.114020904255103 B, added in that order and rounded like a uint8 pass (rgb2gray AFTER the resize,
 *            get_example_from_images.m:11-20); reverse or not; one zero row and one zero column appended.
 *   STITCH4  gray first if three planes; each picture resized as uint8 to floor(nx / 2) x floor(ny / 2) -- the reference
 *            passes nx as the height (gene_example_DOTmark_4stitch.m:55,70-76) --, converted to double, placed [1 2; 3 4];
 *            where the stitched size is not ny x nx, a double resize to ny x nx (which overshoots on binary pictures:
 *            negative entries, as in the reference).
 * Then rho = ((nx ny / sum(rho)) rho + lower_bound) / (1 + lower_bound) (examples/dot2d/get_example.m:45; lower_bound 0:
 * the bits of get_example_from_images.m:31).  The sum is added in the order of dotsocp_map_report ("Sums": blocks of 256
 * consecutive entries in memory order, the rest padded with +0.0).  Errors as for dotsocp_imresize, with `rho` untouched;
 * also DOTSOCP_EINVAL: nimg that does not fit the layout, reverse with STITCH4. */
int dotsocp_image_density(const dotsocp_image_opts *o, const dotsocp_image *imgs, int nimg, double *rho, int device);

/* runHist.{kkt (len x 7, column-major), time, iter, pdGap} (:350-354); any pointer may be NULL */
int dotsocp_get_history(dotsocp_ctx *ctx, double *kkt, double *time, double *iter, double *pdGap);

/* Per-step device times (HIP events on the launch stream): feeds result.times[0..4] (the reference's tic/toc
 * columns Step_1_1_FFT .. KKT, solver_socp_inPALM.m:339-341) and dotsocp_kernel_time().  Off by default; may be
 * switched at any time outside run() -- before begin() to cover the whole solve (the MEX gateways do that), or
 * between two run() calls to cover only what follows (bench.py switches it on after its warm-up iterations).
 * dotsocp_kernel_time: average device time in ms of the named kernel family over the profiled launches since
 * begin(), and their count; names: "rhs", "poisson", "cone_proj", "qstep", "beta", "kkt", "cone_fused_a",
 * "cone_fused_b", "materialise", "comm", "interp", "acc_cone", "acc_gather", "qstep_first", "transpose", "cone_carry"
 * (the cone passes that read gamma and no q^{k-1}; "cone_fused_b" keeps the passes that move 8 (20 Nz + 3 Nq) bytes),
 * "qcone" (a q-step with the next iteration's gamma-reading cone pass in the same kernel: counted here alone),
 * "velocity_layer", "advect" (the launches of dotsocp_recover_velocity / dotsocp_advect_particles on the first slab),
 * "deposit", "frame_l1" (the per-frame launches of dotsocp_push_mass on the first slab), "advect_path" (the accumulating
 * march of dotsocp_map_report on the first slab: counted here, not under "advect"), "map_final" (its one reduction, when
 * the first slab runs it: one slab, or direction -1), "hl_pass_x", "hl_pass_y", "hl_reduce" (the min-plus passes along x and y and the
 * reduction of dotsocp_dual_bound), "sl_pass_x", "sl_pass_y", "sl_node" (the soft passes along x and y and the node kernels,
 * their reductions included, of dotsocp_upper_bound). */
int dotsocp_set_profiling(dotsocp_ctx *ctx, int on);
int dotsocp_kernel_time(dotsocp_ctx *ctx, const char *name, double *avg_ms, dotsocp_i64 *launches);

/* Guard bands (debugging aid): with DOTSOCP_CANARY=1 in the environment every device buffer of
 * the solver state is allocated between two bands of NaN-pattern words.  dotsocp_finish() fails with DOTSOCP_EHIP if a
 * band was overwritten (message: which buffer, how many words, where), dotsocp_destroy() reports to stderr, and this
 * call checks all live buffers of the process at any time: returns the number of damaged buffers (0 = clean, also
 * when the canaries are off) and sets dotsocp_last_error() accordingly.  An out-of-bounds READ shows up as NaNs. */
int dotsocp_canary_check(void);

/* Uninitialised-read poison (test switch): with DOTSOCP_POISON=1 in the environment (read per allocation) every device
 * buffer of floating-point numbers is handed out filled with the quiet NaN 0x7ff8bad0bad0bad0 instead of the zeros that
 * fresh or reused device memory usually shows; buffers of integers (indices, counters, flags) are left alone.  A kernel
 * that reads a slot nothing has written then changes its results (tests/test_gpu_poison.py).
 * dotsocp_debug_alloc_peek: test hook -- allocates n doubles as the library allocates its buffers, copies them to `out`
 * as they were handed out, and frees them; no kernel of the library runs on them.
 * dotsocp_debug_cache_held: test hook -- bytes the device block cache holds on `device` (device < 0: on all devices). */
int dotsocp_debug_alloc_peek(dotsocp_i64 n, double *out);
dotsocp_i64 dotsocp_debug_cache_held(int device);

/* Test support: phi <- idctn(dctn(phi) ./ (D^2 * initialize_FFTkernel)) by the loop's own Poisson solve
 * (Solver::poisson_all, the function every iteration calls), on the slabs of the context as created: one slab, `nslabs`
 * on one device, dotsocp_create_multi, or an attached RCCL rank -- so the partitioned tridiagonal solve along t and the
 * slab <-> pencil transposes can be probed as operators.  Upload DOTSOCP_F_PHI, call, download DOTSOCP_F_PHI; blocks
 * until the solve is complete.  Valid between create and begin (DOTSOCP_ESTATE afterwards); may be repeated. */
int dotsocp_poisson_phi(dotsocp_ctx *ctx);

/* Blocks until all work enqueued by this context has completed. */
int dotsocp_synchronize(dotsocp_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* DOTSOCP_H */
