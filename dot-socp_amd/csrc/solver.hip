// Host side of the device-resident inPALM / ALG2 loop.  The scalar control flow (sigma rule,
// rescale triggers, KKT ratios, stop test) restates socp/dot2d/algorithms/solver_socp_inPALM.m
// (and solver_wsocp_inPALM.m for the weighted variant) line by line; all array work is done by the
// kernels of cone.hip / fused.hip / stencil.hip / qstep_march.hip / dct*.hip / kkt.hip on the slab's HIP streams.
//
// Time-slab mode (world > 1): the grid is cut along t (common.h: Grid).  Per iteration a slab
// exchanges six ny x nx layers with its neighbours (u0 tail, phi head, adjoint tails, bx/by heads)
// and the Poisson solve couples the slabs along t (tri.hip, or slab <-> pencil transposes): solver_comm.hip.  The same code
// runs with all slabs in one process -- each slab on its own device with its own streams, peer copies between
// them (dotsocp_create_multi; on one device: dotsocp_create(..., nslabs)) -- or with one slab per process (RCCL).
#include "solver.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "comm.h"

namespace dotsocp {

// --------------------------------------------------------------------------------------
// begin: solver_socp_inPALM.m:11-135
// --------------------------------------------------------------------------------------
void Solver::update_coef() {
    lc.s = E / D;                       // scaleBF (:58)
    lc.sf = edge_factor(lc.s);
    lc.dF = E / dScale;                 // scaleD (:59,183)
    const double ht = 1.0 / (double)(nt - 1);
    lc.at = D * (1.0 / ht);             // D .* grad, entries 1/ht (initialize.m:68; solver_dotsocp2d.m:338)
    lc.ax = (nx > 1) ? D * (1.0 / (1.0 / (double)(nx - 1))) : 0.0;
    lc.ay = (ny > 1) ? D * (1.0 / (1.0 / (double)(ny - 1))) : 0.0;
    lc.tau = opts.tau;
    const double tmp = (E / D) * (E / D);   // oper_q.m:14
    if (prob.weighted) { lc.c1 = 2.0 * tmp; lc.c2 = tmp; }
    else { lc.c1 = 1.0 + 2.0 * tmp; lc.c2 = 1.0 + tmp; }
    lc.dinv1 = 1.0 / lc.c1;
    lc.dinv2 = 1.0 / lc.c2;
}

// Every reader of beta other than a CONE_GIN pass: by the schedule of step() none ever meets gamma
int Solver::need_beta_form(const char *who) const {
    if (!beta_gamma) return 0;
    set_error("internal: %s met the gamma form of beta", who);
    return DOTSOCP_ESTATE;
}

// Every reader of q outside k_qcone: by the schedule each follows a q-step that stored q (solver.h: the early cone pass)
int Solver::need_q(const char *who) const {
    if (q_valid) return 0;
    set_error("internal: %s met a q that was never stored", who);
    return DOTSOCP_ESTATE;
}

int Solver::flush_beta() {
    DS_CHECK(need_beta_form("flush_beta"));
    if (bops.empty()) return 0;
    FOR_SLABS(s) {
        DS_CHECK(launch_scale(s.beta, 10 * s.g.Nc, bops.mul, bops.div, s.st));
        if (bops.n > 1) DS_CHECK(launch_scale(s.beta, 10 * s.g.Nc, bops.mul2, bops.div2, s.st));
    }
    bops.clear();
    return 0;
}

// beta <- beta * mul / div, executed by the next pass that reads beta (two operations can wait)
int Solver::push_beta_op(double mul, double div) {
    if (bops.push(mul, div)) return 0;
    DS_CHECK(flush_beta());
    bops.push(mul, div);
    return 0;
}

FusedArgs Solver::pending_step_args(const Slab &s) const {
    FusedArgs a{};
    a.q_old = s.q_old;
    a.q = s.q;
    a.beta_in = s.beta;
    a.bops = bops;
    return a;
}

int Solver::clear_partials(Slab &s) {
    DS_HIP(ds_memset_async(s.kw.partials, 0, sizeof(double) * s.kw.maxBlocks * S_COUNT, s.st));
    return 0;
}

int Solver::flush_alpha() {
    if (aops.empty()) return 0;
    FOR_SLABS(s) DS_CHECK(launch_scale(s.alpha, s.g.NqAlloc, aops.mul, aops.div, s.st));
    aops.clear();
    return 0;
}

// sigma update on the folded KKT path (one slab, fused dataflow): alpha, beta, c <- x / factor (solver_socp_inPALM.m:
// 312-314) without a pass over alpha or q -- beta and alpha stay as they are and are divided on load by their next
// reader (cone pass resp. q-step), and the right-hand side of the next phi-step is corrected with the r = A' alpha - c
// the q-step stored: A'(w.*q - alpha / f) + c / f = (rhs + r) - r / f.  c is divided in that same small pass.
int Solver::sigma_scale_folded(double factor) {
    DS_CHECK(flush_alpha());
    DS_CHECK(ensure_halo());
    u0_made = false;
    DS_CHECK(push_beta_op(1.0, factor));
    if (multi()) {
        // time slabs: the u0 tail for the right neighbour is formed from alpha in memory before the next q-step runs
        FOR_SLABS(s) DS_CHECK(launch_scale(s.alpha, s.g.NqAlloc, 1.0, factor, s.st));
    } else {
        aops.push(1.0, factor);
    }
    u0_fresh = false;
    FOR_SLABS(s) DS_CHECK(launch_rhs_sigma_fix(s.g, s.w0, s.w1, s.c, factor, s.st, c_ends_on && s.c_ends));
    return 0;
}

int Solver::scale_state(double a_mul, double a_div, double q_div, bool with_c) {
    DS_CHECK(need_beta_form("scale_state"));
    DS_CHECK(need_q("scale_state"));
    DS_CHECK(flush_alpha());
    if (begun) DS_CHECK(ensure_halo());
    u0_made = false;
    u0_fresh = false;      // q0 / alpha0 change: the u0 tail held by the right neighbour is stale
    rhs_valid = false;     // ... and so is the right-hand side the last q-step left in w0
    if (fused && begun) {
        // beta: applied by the next pass that reads it
        DS_CHECK(push_beta_op(a_mul, a_div));
    }
    FOR_SLABS(s) {
        const Grid &g = s.g;
        if (with_c) DS_CHECK(launch_scale(s.c, g.Nphi, a_mul, a_div, s.st));
        if (!acc_light) DS_CHECK(launch_scale(s.alpha, g.NqAlloc, a_mul, a_div, s.st));
        // (acc_light: acc-ADMM's sigma update with the extrapolating cone pass to follow, which divides beta itself)
        if (!(fused && begun) && !acc_light) DS_CHECK(launch_scale(s.beta, 10 * g.Nc, a_mul, a_div, s.st));
        if (q_div != 1.0) {
            DS_CHECK(launch_scale(s.q, g.NqAlloc, 1.0, q_div, s.st));
            // fused dataflow: a z that is not materialised is not scaled either -- it is regenerated from the scaled
            // q and beta when somebody asks for it (the kept beta^k / q^k pair of the last KKT pass no longer matches)
            if (!(fused && begun) || z_valid) DS_CHECK(launch_scale(s.z, 10 * g.Nc, 1.0, q_div, s.st));
        }
    }
    if (q_div != 1.0 && fused && begun && !z_valid) z_prev_ok = false;
    return 0;
}

int Solver::begin_method(const dotsocp_opts *o, int m, const dotsocp_acc_opts *acc) {
    if (begun) { set_error("begin() called twice"); return DOTSOCP_ESTATE; }
    if (m == DOTSOCP_METHOD_INPALM) return begin(o);
    DS_ARG(m == DOTSOCP_METHOD_ACCADMM || m == DOTSOCP_METHOD_PALM, "unknown method");
    DS_ARG(prob.dim == 2, "the reference has PALM and acc-ADMM loops for 2-D problems only");
    DS_ARG(!(m == DOTSOCP_METHOD_PALM && prob.weighted), "the reference has no weighted PALM loop");
    method = m;
    int rc = begin(o);
    if (rc != 0) { method = DOTSOCP_METHOD_INPALM; return rc; }
    return (m == DOTSOCP_METHOD_PALM) ? palm_begin() : acc_begin(acc);
}

int Solver::begin(const dotsocp_opts *o) {
    DS_ARG(o != nullptr, "opts is NULL");
    DS_ARG(o->maxit >= 0, "opts.maxit < 0");
    DS_ARG(o->sigma > 0, "opts.sigma must be positive");
    if (begun) { set_error("begin() called twice"); return DOTSOCP_ESTATE; }
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    DS_CHECK(ensure_alloc());
    if (method == DOTSOCP_METHOD_ACCADMM) {
        DS_CHECK(acc_alloc());
        fused = false;       // z is a stored state variable of this loop: the generic helpers take their "z in memory" paths
    }
    opts = *o;
    cone_carry = true;
    if (const char *e = getenv("DOTSOCP_CONE_CARRY")) cone_carry = (atoi(e) != 0);     // read per begin(), like the others
    c_ends_on = true;
    if (const char *e = getenv("DOTSOCP_C_ENDS")) c_ends_on = (atoi(e) != 0);
    if (c_ends_on) DS_CHECK(detect_c_ends());
    // test hook: the time limit counts as passed from this iteration on (tests/test_gpu_cone_carry.py takes the
    // "time limit in a gamma iteration" branch of step() at a chosen iteration instead of at a wall-clock moment)
    timeout_at = -1;
    if (const char *e = getenv("DOTSOCP_TEST_TIMEOUT_AT")) timeout_at = atoll(e);
    qcone = -1;
    if (const char *e = getenv("DOTSOCP_QCONE")) qcone = atoi(e);
    if (qcone < -1 || qcone > 2) qcone = -1;
    q_valid = true;
    early_pass = QCONE_NONE;
    beta_gamma = false;
    run_left = -1;
    timeout_pending = false;
    checkPrimDualFeas = (o->checkPrimDualFeas < 0) ? !prob.weighted : (o->checkPrimDualFeas != 0);   // :20-24 / wsocp :25-29
    time_limit = (o->time_limit > 0) ? o->time_limit : 3600.0;                                        // :26-30
    sigma = o->sigma;
    lastSigmaIt = -INFINITY;
    cScale = prob.cScale; dScale = prob.dScale; D = prob.D; E = prob.E;                                // :54-59
    use_feasOrg = 0;
    tol_feasOrg = 5 * o->tol;
    rescale = o->scaling ? 1 : 0;                                                                      // :64-68
    maxFeas = INFINITY; relGap = INFINITY;
    h = 1.0 / ((double)nx * (double)ny * (double)nt);                                                  // :84
    norm_c = prob.normc; norm_d = prob.normd;                                                          // :100-101
    update_coef();
    // alpha /= sigma, beta /= sigma, c /= sigma                                                       // :102-104
    DS_CHECK(scale_state(1.0, sigma, 1.0, true));
    DS_CHECK(exchange_q_halo(false));
    sigmaScale = 1.0;
    it = 0;
    stopped = false;
    deferred = false;
    z_valid = true;
    z_prev_ok = false;
    rhs_valid = false;
    last_S_it = -1;
    hist_kkt.clear(); hist_time.clear(); hist_iter.clear(); hist_gap.clear();
    for (int i = 0; i < PH_COUNT; ++i) { phase_ms[i] = 0; phase_launches[i] = 0; }
    if (canary_enabled() && getenv("DOTSOCP_CANARY_SELFTEST")) {
        // test hook: one double written right behind model.c, the way a kernel overrunning its last tile would
        Slab &s0 = slabs[0];
        DS_CHECK(use(s0));
        const double v = 1.0;
        DS_HIP(ds_memcpy_async(s0.c + s0.g.Nphi, &v, sizeof v, hipMemcpyHostToDevice, s0.st));
        DS_HIP(ds_stream_synchronize(s0.st));
    }
    begun = true;
    elapsed_prev = 0.0;
    elapsed_agreed = 0.0;
    t_begin = std::chrono::steady_clock::now();
    return 0;
}

// --------------------------------------------------------------------------------------
// the four steps of one iteration
// --------------------------------------------------------------------------------------
// phi = idctn(dctn(rhs) ./ kernel), kernel = D^2 * initialize_FFTkernel  (:96,194); rhs is in w0
int Solver::poisson_all(const PhiHooks *hooks) {
    const i64 plane = slabs[0].g.plane;
    const bool tp2 = dct_plan_has_tsolve(devres[0]->pt);
    FOR_SLABS(s) {
        const Grid &g = s.g;
        DS_CHECK(launch_dct_axis(s.res->py, s.w0, s.w1, g.ny, g.nx, g.ntl, 0, 0, s.st, g.py));
        DS_CHECK(launch_dct_axis(s.res->px, s.w1, s.w0, g.ny, g.nx, g.ntl, 1, 0, s.st, g.py));
    }
    bool tri = multi() && tri_tsolve && world <= DS_MAX_WORLD;
    for (auto &s : slabs) tri = tri && s.g.ntl <= TRI_EXTRA;
    if (tri) {
        DS_CHECK(poisson_t_tridiag(hooks));
    } else {
    if (hooks && hooks->fill) {
        prof_end(PH_POISSON);
        DS_CHECK(hooks->fill());
        prof_begin(PH_POISSON);
    }
    if (hooks && hooks->behind) DS_CHECK(hooks->behind());
    if (multi()) {       // timed on its own (inside "poisson") so that the scaling runs show what the all-to-alls cost
        prof_begin(PH_TRANSPOSE);
        DS_CHECK(transpose(true));
        prof_end(PH_TRANSPOSE);
    }
    FOR_SLABS(s) {
        double *p = multi() ? s.pencil : s.w0;
        double *p2 = multi() ? s.pencil2 : s.w1;
        if (!multi()) {
            // the single slab: rows may be pitched (common.h), the (y, x) columns of a layer are ny lines in each of nx rows
            // (DOTSOCP_TSOLVE=dct: the transform passes for every length)
            DS_CHECK(launch_poisson_t_single(s.res->pt, s.g, D * D, s.res->cy, s.res->cx, s.res->ct, p, p2, s.g.py, s.st, tri_tsolve));
        } else if (tp2) {
            DS_CHECK(launch_dct_t_solve(s.res->pt, p, p, s.g.py, plane, s.l0, s.nl, nt, D * D, s.res->cy, s.res->cx, s.res->ct, s.st));
        } else {
            DS_CHECK(launch_dct_axis(s.res->pt, p, p2, s.nl, 1, nt, 2, 0, s.st));
            DS_CHECK(launch_spectral_divide_pencil(p2, s.g.py, s.l0, s.nl, nt, D * D, s.res->cy, s.res->cx, s.res->ct, s.st));
            DS_CHECK(launch_dct_axis(s.res->pt, p2, p, s.nl, 1, nt, 2, 1, s.st));
        }
    }
    if (multi()) {
        prof_begin(PH_TRANSPOSE);
        DS_CHECK(transpose(false));
        prof_end(PH_TRANSPOSE);
    }
    }
    FOR_SLABS(s) {
        const Grid &g = s.g;
        DS_CHECK(launch_dct_axis(s.res->px, s.w0, s.w1, g.ny, g.nx, g.ntl, 1, 1, s.st, g.py));
        DS_CHECK(launch_dct_axis(s.res->py, s.w1, s.phi, g.ny, g.nx, g.ntl, 0, 1, s.st, g.py));
    }
    return 0;
}

// Test support (dotsocp_poisson_phi): phi <- the loop's own Poisson solve of phi, on whatever slabs this context holds.
// Between create and begin only: the loop's state is not touched, w0 / w1 and the solve's messages are free then.
int Solver::poisson_phi() {
    if (begun) { set_error("poisson_phi() must precede begin()"); return DOTSOCP_ESTATE; }
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    DS_CHECK(ensure_alloc());
    D = prob.D;                      // what begin() sets; poisson_all() divides by D^2 * kernel
    FOR_SLABS(s) DS_HIP(ds_memcpy_async(s.w0, s.phi, sizeof(double) * (size_t)s.g.Nphi, hipMemcpyDeviceToDevice, s.st));
    DS_CHECK(poisson_all(nullptr));
    return sync_all();
}

int Solver::phase_phi(const PhiHooks *hooks) {
    DS_CHECK(ensure_halo());
    if (multi() && !u0_fresh) {      // normally shipped with the q halo at the end of the previous iteration
        DS_CHECK(make_u0_tail());
        prof_begin(PH_COMM, comm_z);
        DS_CHECK(exchange_u0_tail());
        prof_end(PH_COMM, comm_z);
    }
    prof_begin(PH_RHS);
    if (!rhs_valid) {
        DS_CHECK(need_q("phase_phi"));
        DS_CHECK(flush_alpha());
        FOR_SLABS(s) DS_CHECK(launch_rhs(s.g, lc, s.q, s.alpha, s.c, s.weight, s.u0_prev, s.w0, s.st, c_ends_on && s.c_ends));
    } else if (multi()) {
        // the q-step left rhs in w0; its first layer still lacks the left neighbour's last cell
        FOR_SLABS(s)
            if (!s.g.first) DS_CHECK(launch_rhs_fixup(s.g, lc, s.u0_prev, s.w0, s.st));
    }
    rhs_valid = false;
    prof_end(PH_RHS);
    prof_begin(PH_POISSON);
    DS_CHECK(poisson_all(hooks));
    prof_end(PH_POISSON);
    return 0;                        // the phi head travels with the adjoint tails (ship_tails)
}

// part 0 / 1 / 2 of a launch in C chunks (phase_z, phase_q): all of them, all but the last, the last
static void part_chunks(int part, i64 C, i64 *z0, i64 *zc) {
    *z0 = (part == 2) ? C - 1 : 0;
    *zc = (part == 0) ? C : ((part == 1) ? C - 1 : 1);
}

// The cone pass needs q^k and beta only -- not phi^{k+1}.  Time slabs: it runs in chunks of time cells, one launch per
// chunk in ascending order (the "t + 1" cone entries of a chunk's last cell travel to the next launch through s.carry),
// and only the last chunk reads the q halo -- step() puts the others in front of the halo's arrival (part 1) and the
// last one beside the first interface exchange of the Poisson solve (part 2).  A pass that ran inside the last q-step
// (StepPlan::cone_launch is false) is not launched again: step() does not call this.
int Solver::phase_z(const StepPlan &plan, int part) {
    DS_CHECK(need_q("phase_z"));
    if (part != 1) DS_CHECK(ensure_halo());     // the last chunk reads the q halo (part 1 never does)
    if (!fused) {
        prof_begin(PH_PROJ);
        FOR_SLABS(s) DS_CHECK(launch_cone_proj(s.g, lc, s.q, s.beta, s.z, s.st));
        prof_end(PH_PROJ);
        return 0;
    }
    // flavour of the deferred pass (kernels.h): reads gamma if the last pass left it, writes what the plan scheduled.  The
    // passes that do not read q_old move fewer bytes and are timed as a phase of their own.
    const bool gin = beta_gamma, gout = plan.pass_gout;
    if (gin && (!deferred || !bops.empty())) {
        set_error("internal: gamma form %s", deferred ? "with a pending scaling of beta" : "without a pending multiplier step");
        return DOTSOCP_ESTATE;
    }
    const int flavour = (gin ? CONE_GIN : 0) | (gout ? CONE_GOUT : 0);
    const int ph = deferred ? (gin ? PH_CONE_CARRY : PH_FUSED_B) : PH_FUSED_A;
    z_valid = false;          // the fused pass forms z^{k+1} in registers only
    z_prev_ok = false;        // ... and (mode B) overwrites the kept beta^{k-1}
    prof_begin(ph);
    FOR_SLABS(s) {
        FusedArgs a{};
        a.q = s.q;
        a.q2 = s.q2;
        a.sx = s.sx;
        a.sy = s.sy;
        a.beta_in = s.beta;
        a.bops = bops;
        const i64 C = s.fg.chunks;
        i64 z0, zc;
        part_chunks(part, C, &z0, &zc);
        if (deferred) {
            // beta^k = beta^{k-1} + tau (z^k - BF q^k - d) folded into this iteration's projection
            a.q_old = s.q_old;
            a.beta_out = s.beta2;
        }
        const int mode = deferred ? 1 : 0;
        if (s.carry && C > 1) {
            for (i64 z = z0; z < z0 + zc; ++z) {
                a.carry_in = (z > 0) ? s.carry : nullptr;
                a.carry_out = (z + 1 < C) ? s.carry : nullptr;
                DS_CHECK(launch_cone_fused(mode, s.g, lc, s.fg, a, s.st, z, 1, flavour));
            }
        } else {
            DS_CHECK(launch_cone_fused(mode, s.g, lc, s.fg, a, s.st, z0, zc, flavour));
        }
        if (deferred && part != 1) std::swap(s.beta, s.beta2);
    }
    prof_end(ph);
    if (part == 1) return 0;
    if (deferred) {
        bops.clear();                 // mode B rewrote beta with the scaling applied
        beta_gamma = gout;
    }
    return 0;
}

KktCoef Solver::kkt_coef() const {
    KktCoef k;
    k.sigma = sigma;
    k.kappa = sigma * cScale * D;
    k.dsD = dScale / D;
    k.dsE = dScale / E;
    return k;
}

// plan.fold: the iteration ends with a KKT check and the q-step runs in its KKT variant
int Solver::phase_q(const StepPlan &plan, int part, int early) {
    const bool kkt = plan.fold;
    if (!fused) DS_CHECK(flush_alpha());
    if (early != QCONE_NONE && (part != 0 || kkt || multi() || !fused || !deferred || !beta_gamma || !bops.empty())) {
        set_error("internal: early cone pass in a state it does not serve");
        return DOTSOCP_ESTATE;
    }
    const bool egout = (early == QCONE_STEADY);
    const int ph = (early != QCONE_NONE) ? PH_QCONE : PH_QSTEP;
    prof_begin(ph);
    FOR_SLABS(s) {
        hipStream_t st = s.st;
        if (early != QCONE_NONE && qcone != 2) {
            // reads the sums in q2 / sx / sy and gamma; q^{k+1} goes to the buffer that held q^{k-1} (exit form only), the new
            // sums to the buffer that holds q^k -- dead: the pass of this iteration has run, a gamma-reading pass reads no
            // q_old and the q-step never reads q -- and to the partners of sx / sy
            if (!s.sx2) {
                DS_CHECK(s.zalloc(&s.sx2, s.fg.sx_len));
                DS_CHECK(s.zalloc(&s.sy2, s.fg.sy_len));
            }
            QConeArgs a{};
            a.phi = s.phi; a.q2v = s.q2; a.sx = s.sx; a.sy = s.sy; a.cvec = s.c; a.alpha_in = s.alpha; a.gamma_in = s.beta;
            a.alpha_out = s.alpha2; a.rhs = s.w0; a.q_out = s.q_old; a.beta_out = s.beta2;
            a.q2_out = s.q; a.sx_out = s.sx2; a.sy_out = s.sy2;
            a.ap_on = aops.n; a.ap_mul = aops.mul; a.ap_div = aops.div;
            a.c_ends = (c_ends_on && s.c_ends) ? 1 : 0;
            DS_CHECK(launch_qcone(s.g, lc, s.fg, a, egout, st));
            s.rotate_after_qcone();
        } else if (!fused) {
            DS_CHECK(launch_qstep(s.g, lc, s.phi, s.z, s.beta, s.weight, s.tail_bx, s.tail_by, s.q, s.alpha, s.st));
        } else {
            // q^{k+1} goes to the buffer that held q^{k-1}; q^k is kept for the deferred beta update
            // ... and the right-hand side of the next phi-step is formed in the same pass (alpha ping-pongs)
            i64 z0, zc;
            part_chunks(part, qstep_rhs_chunks(s.g, s.fg), &z0, &zc);
            QStepExtra ex{};
            ex.aops = aops;
            ex.c_ends = (c_ends_on && s.c_ends) ? 1 : 0;
            if (multi() && !s.g.last && part != 1) ex.u0_tail = s.send_plane;
            if (kkt) {
                const KktCoef k = kkt_coef();
                ex.partials = kkt_qstep_partials(s.g, s.kw);
                ex.resid = s.w1;                   // free between the Poisson solves
                ex.kappa = k.kappa; ex.dsD = k.dsD;
            }
            DS_CHECK(launch_qstep_rhs(s.g, lc, s.fg, s.phi, s.q2, s.sx, s.sy, s.weight, s.tail_bx, s.tail_by, s.c,
                                      s.q_old, s.alpha, s.alpha2, s.w0, st, z0, zc, 1, &ex));
            if (part != 1) std::swap(s.alpha, s.alpha2);
            if (part != 1) std::swap(s.q, s.q_old);
            if (early != QCONE_NONE) {
                // DOTSOCP_QCONE=2: the same schedule with the two kernels back to back
                FusedArgs a{};
                a.q = s.q; a.q2 = s.q2; a.sx = s.sx; a.sy = s.sy;
                a.beta_in = s.beta; a.beta_out = s.beta2;
                a.bops = bops;
                DS_CHECK(launch_cone_fused(1, s.g, lc, s.fg, a, s.st, 0, s.fg.chunks, CONE_GIN | (egout ? CONE_GOUT : 0)));
                std::swap(s.beta, s.beta2);
            }
        }
    }
    prof_end(ph);
    if (part == 1) return 0;
    q_valid = true;
    if (early != QCONE_NONE) {
        // the bookkeeping of the next iteration's cone pass, which its plan will not launch
        q_valid = !egout || qcone == 2;
        beta_gamma = egout;
        z_valid = false;
        z_prev_ok = false;
    }
    early_pass = early;
    u0_made = multi() && fused;
    if (fused) aops.clear();                 // the q-step wrote the scaled alpha into the ping-pong partner
    rhs_valid = fused;
    // the halo exchange waits for the next consumer: the next step() runs it beside the first cone chunks
    if (multi() && fused && comm_z && cone_split_enabled()) halo_pending = true;
    else DS_CHECK(exchange_q_halo(true));
    return 0;
}

int Solver::phase_mult() {
    if (fused) {
        deferred = true;     // the multiplier step is executed by the next fused pass (or by materialise())
        return 0;
    }
    prof_begin(PH_BETA);
    FOR_SLABS(s) DS_CHECK(launch_beta_update(s.g, lc, s.q, s.z, s.beta, s.st));
    prof_end(PH_BETA);
    return 0;
}

// Fused path only: execute the pending multiplier step and store z (solver_socp_inPALM.m:199,
// 212-215) so that beta, z are the iterates the KKT block, the rescale block and the outputs see.
int Solver::materialise() {
    if (!fused || !deferred) return 0;
    DS_CHECK(need_beta_form("materialise"));
    DS_CHECK(need_q("materialise"));
    DS_CHECK(ensure_halo());
    prof_begin(PH_MATERIALISE);
    FOR_SLABS(s) {
        FusedArgs a = pending_step_args(s);
        a.beta_out = s.beta;
        a.z_out = s.z;
        DS_CHECK(launch_cone_fused(2, s.g, lc, s.fg, a, s.st));
    }
    prof_end(PH_MATERIALISE);
    bops.clear();
    deferred = false;
    z_valid = true;
    return 0;
}

// z of the last completed iteration in s.z (outputs, rescale block, unfused-style cell sums)
int Solver::ensure_z() {
    if (!fused || z_valid) return 0;
    DS_CHECK(need_beta_form("ensure_z"));
    DS_CHECK(need_q("ensure_z"));
    if (deferred) return materialise();
    if (!z_prev_ok) {
        set_error("internal: z cannot be regenerated");
        return DOTSOCP_ESTATE;
    }
    DS_CHECK(ensure_halo());
    prof_begin(PH_MATERIALISE);
    FOR_SLABS(s) {
        FusedArgs a{};
        a.q_old = s.q_old;
        a.q = s.q;
        a.beta_in = s.beta2;      // beta^k, kept by the KKT pass
        a.z_out = s.z;
        a.bops = zp_ops;
        DS_CHECK(launch_cone_fused(3, s.g, lc, s.fg, a, s.st));
    }
    prof_end(PH_MATERIALISE);
    z_valid = true;
    return 0;
}

// folded: this iteration's q-step ran in its KKT variant (phase_q(.., true)): region 0 of the partial sums holds its
// share, the cell pass adds the F*B*beta terms of the edges, and no node / edge launch follows
int Solver::kkt_sums(double *S, bool folded) {
    DS_CHECK(need_beta_form("kkt_sums"));
    DS_CHECK(need_q("kkt_sums"));
    DS_CHECK(ensure_halo());
    const KktCoef k = kkt_coef();
    if (method == DOTSOCP_METHOD_ACCADMM && folded) {
        // acc-ADMM, one slab: the cone pass of the iteration has taken the cell sums and the F*B*beta^+ terms of every entry
        // (launch_acc_cone_kkt: regions 1-3, buffer cleared before it); left are the sums made of phi^+, q^+, alpha^+, c
        FOR_SLABS(s) DS_CHECK(launch_kkt_nodual(s.g, lc, k, s.phi, s.q, s.alpha, s.c, s.weight, s.kw, s.st));
        return reduce_sums(S);
    }
    if (!folded) {
        DS_CHECK(flush_alpha());
        // the launches below write per-workgroup partial sums into four regions; grids of different
        // shapes may use a region on different calls, so stale entries are cleared first
        FOR_SLABS(s) DS_CHECK(clear_partials(s));
    }
    // ---- cell part (region 1 of the partial sums) ----
    int rest = folded ? 0 : (1 | 4 | 8);
    if (fused && deferred) {
        // pending multiplier step + cell sums in one pass; beta^k stays in beta2 so that z can be regenerated
        FOR_SLABS(s) {
            FusedArgs a = pending_step_args(s);
            a.beta_out = s.beta2;
            if (folded) { a.q2 = s.q2; a.sx = s.sx; a.sy = s.sy; }      // scratch for the gather of beta on tile borders
            DS_CHECK(launch_kkt_cells_update(s.g, lc, k, s.fg, a, s.phi, s.alpha, s.weight, s.kw, s.st, folded, s.q));
            std::swap(s.beta, s.beta2);
        }
        // the kept beta^k (now in beta2) is still unscaled in memory: remember its pending op for MODE_Z
        zp_ops = bops;
        bops.clear();
        deferred = false;
        z_valid = false;
        z_prev_ok = true;
    } else {
        if (folded) { set_error("internal: folded KKT sums without a pending multiplier step"); return DOTSOCP_ESTATE; }
        DS_CHECK(ensure_z());
        DS_CHECK(flush_beta());
        rest |= 2;
    }
    if (multi()) {
        const i64 plane = slabs[0].g.plane;
        u0_made = false;                      // launch_kkt_tail reuses send_plane
        FOR_SLABS(s)
            if (!s.g.last)
                DS_CHECK(launch_kkt_tail(s.g, s.alpha, s.beta, s.weight, s.send_plane, s.send_plane2, s.send_bx, s.send_by,
                                         s.st));
        DS_CHECK(group_begin());
        DS_CHECK(shift(+1, [](Slab &s) { return s.send_plane; }, [](Slab &s) { return s.a0_prev; }, plane));
        DS_CHECK(shift(+1, [](Slab &s) { return s.send_plane2; }, [](Slab &s) { return s.a0w_prev; }, plane));
        DS_CHECK(shift(+1, [](Slab &s) { return s.send_bx; }, [](Slab &s) { return s.btail_bx; }, slabs[0].g.bxLayer));
        DS_CHECK(shift(+1, [](Slab &s) { return s.send_by; }, [](Slab &s) { return s.btail_by; }, slabs[0].g.byLayer));
        DS_CHECK(group_end());
    }
    FOR_SLABS(s) {
        KktHalo halo{s.a0_prev, s.a0w_prev, s.btail_bx, s.btail_by};
        if (rest) DS_CHECK(launch_kkt(s.g, lc, k, s.phi, s.q, s.alpha, s.z, s.beta, s.c, s.weight, halo, s.kw, rest, s.st));
        // folded path on a slab that is not the first: its first node / edge layer, now that the left neighbour's last
        // cell has arrived (the q-step, the cell pass and the border launches skipped that layer)
        if (folded && !s.g.first)
            DS_CHECK(launch_kkt(s.g, lc, k, s.phi, s.q, s.alpha, s.z, s.beta, s.c, s.weight, halo, s.kw, 1 | 4 | 8, s.st, true,
                                s.w1));
    }
    return reduce_sums(S);
}

// The partial sums every slab holds -> S[0 .. S_COUNT) summed over the slabs (host, in slab order) resp. over the ranks
// (all-reduce); S[S_COUNT] = the wall clock (one slab per process: the maximum over the ranks)
int Solver::reduce_sums(double *S) {
    for (int i = 0; i <= S_COUNT; ++i) S[i] = 0.0;
    FOR_SLABS(s) {
        DS_CHECK(launch_kkt_final(s.g, s.kw, s.st));
        if (remote()) break;
        DS_HIP(ds_memcpy_async(s.h_sums, s.kw.sums, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost, s.st));
    }
    if (!remote()) {        // all slabs are enqueued before the host waits for the first; summed in slab order
        FOR_SLABS(s) {
            DS_HIP(ds_stream_synchronize(s.st));
            for (int i = 0; i < S_COUNT; ++i) S[i] += s.h_sums[i];
        }
    }
    S[S_COUNT] = elapsed();
    if (remote()) {
        // sum the partial sums over the ranks; slot S_COUNT carries the wall clock (max via a second reduce)
        Rccl &api = rccl_api();
        Slab &s = slabs[0];
        DS_CHECK(comm_enter());
        const hipStream_t cs = cst(s);
        DS_NCCL(api.AllReduce(s.kw.sums, d_red, S_COUNT, ncclDouble, ncclSum, (ncclComm_t)nccl, cs));
        h_sums[S_COUNT] = S[S_COUNT];
        DS_HIP(ds_memcpy_async(d_red + S_COUNT, h_sums + S_COUNT, sizeof(double), hipMemcpyHostToDevice, cs));
        DS_NCCL(api.AllReduce(d_red + S_COUNT, d_red + S_COUNT, 1, ncclDouble, ncclMax, (ncclComm_t)nccl, cs));
        DS_HIP(ds_memcpy_async(h_sums, d_red, sizeof(double) * (S_COUNT + 1), hipMemcpyDeviceToHost, cs));
        DS_CHECK(comm_leave());
        DS_HIP(ds_stream_synchronize(stream));
        for (int i = 0; i <= S_COUNT; ++i) S[i] = h_sums[i];
    }
    elapsed_agreed = S[S_COUNT];
    return 0;
}

// The five norms of solver_socp_inPALM.m:140-141 for an iterate whose multiplier step is still pending (the state between
// two iterations of the fused loop): one pass over beta that stores nothing, three sums of squares.  S as from kkt_sums().
int Solver::norms_light(double *S) {
    DS_CHECK(need_beta_form("norms_light"));
    DS_CHECK(need_q("norms_light"));
    DS_CHECK(ensure_halo());
    DS_CHECK(flush_alpha());
    const KktCoef k = kkt_coef();
    FOR_SLABS(s) {
        DS_CHECK(clear_partials(s));
        const FusedArgs a = pending_step_args(s);
        DS_CHECK(launch_norms(s.g, lc, k, s.fg, a, s.phi, s.alpha, s.weight, s.kw, s.st));
    }
    return reduce_sums(S);
}

// solver_socp_inPALM.m:138-190
int Solver::rescale_block() {
    bool scaleYes = false;
    double normPhis = 0, normAlps = 0;
    auto norms = [&](double &nPhis, double &nAlps) -> int {
        double S[S_COUNT + 1];
        double sig = sigma;
        if (method == DOTSOCP_METHOD_INPALM && fused && last_S_it == it - 1 && norm_cache) {
            // The previous iteration ended with a KKT check: its sums ARE the squared norms of phi, q, z, alpha, beta
            // of the current iterate.  A sigma update in between divided alpha and beta by `factor` and multiplied
            // sigma by it, so sigma * ||alpha|| is what it was with the sigma of the check -- no pass over the state.
            for (int i = 0; i < S_COUNT; ++i) S[i] = last_S[i];
            sig = last_S_sigma;
        } else if (method == DOTSOCP_METHOD_INPALM && fused && deferred && norm_cache) {
            DS_CHECK(norms_light(S));          // nothing is materialised, the multiplier step stays pending
        } else {
            DS_CHECK(materialise());
            DS_CHECK(ensure_z());
            DS_CHECK(kkt_sums(S));
        }
        const double sh = sqrt(h);
        const double normPhi = sh * sqrt(S[S_PHI2]), normQ = sh * sqrt(S[S_Q2]), normZ = sh * sqrt(S[S_Z2]);
        const double normAlpha = sig * (sh * sqrt(S[S_ALPHA2])), normBeta = sig * (sh * sqrt(S[S_BETA2]));
        nPhis = std::max(std::max(normPhi, normQ), normZ);
        nAlps = std::max(normAlpha, normBeta);
        return 0;
    };
    if (rescale_due(it, rescale, maxFeas, relGap)) DS_CHECK(need_beta_form("rescale_block"));
    if (norm_check_due(it, rescale)) {
        DS_CHECK(norms(normPhis, normAlps));
        const double ratio = std::max(normAlps, normPhis) / std::min(normAlps, normPhis);
        if (ratio > 1.2) scaleYes = true;
    }
    if (!(rescale_trigger(it, rescale, maxFeas, relGap) || scaleYes)) return 0;
    if (!scaleYes) DS_CHECK(norms(normPhis, normAlps));
    // A multiplier step that is still pending belongs to the OLD scaling (z^k = Pi(BF q^{k-1} + d - beta^{k-1}) with the old
    // d and the unscaled q, beta): it is executed before anything is rescaled.  (Right after a KKT check nothing is
    // pending; the every-100-iterations check took its norms without touching the state.)
    DS_CHECK(materialise());
    const double dScale2 = normPhis, cScale2 = normAlps;
    sigma = sigma * (cScale2 / dScale2);
    norm_c = norm_c / cScale2;
    if (!prob.weighted) norm_d = norm_d / dScale2;      // solver_wsocp_inPALM.m has no norm_d
    // c, alpha, beta <- x * dScale2 / cScale2^2 ; q, z <- x / dScale2
    DS_CHECK(scale_state(dScale2, cScale2 * cScale2, dScale2, true));
    if (method == DOTSOCP_METHOD_PALM) {                 // solver_socp_PALM.m:191 tmp_q = A phi is scaled: scale phi
        FOR_SLABS(s) DS_CHECK(launch_scale(s.phi, s.g.NphiAlloc, 1.0, dScale2, s.st));
    }
    dScale = dScale2 * dScale;
    cScale = cScale2 * cScale;
    sigmaScale = sigmaScale * (cScale2 / dScale2);
    update_coef();                                       // scaleD = E / dScale (:183); z2 is regenerated on the fly
    rescale += 1;
    return 0;
}

// the time-out predicate of step(): the same expression in front of a q-step that could run an early pass and behind the body
bool Solver::time_limit_passed() const {
    // with one slab per process a per-rank clock could split the ranks: see kkt_block()
    return timeout_pending || (remote() ? false : (elapsed() > time_limit || (timeout_at > 0 && it >= timeout_at)));
}

// What plan_step() decides this iteration from, read at the top of step() behind the rescale block
StepIn Solver::step_in() const {
    StepIn in{};
    in.s = SchedState{it, opts.maxit, lastSigmaIt, opts.ifCheckStepByStep != 0, rescale, maxFeas, relGap, run_left};
    in.fused = fused; in.deferred = deferred; in.cone_carry = cone_carry; in.kkt_fold = kkt_fold;
    in.beta_gamma = beta_gamma; in.timeout_pending = timeout_pending; in.early = early_pass;
    const Slab &s0 = slabs[0];
    in.qcone_eligible = qcone != 0 && fused && !multi() && !prob.weighted && method == DOTSOCP_METHOD_INPALM &&
                        s0.g.ncl >= 1 && s0.fg.XB == 4 &&
                        (qcone > 0 || s0.fg.nyblk * s0.fg.nxblk >= 2048);   // unset: grids whose cone pass runs as one chunk
    // Time slabs, messages on the second streams (solver.h: comm_z): kernels on the main streams in an order that leaves
    // every message time to travel while kernels that do not need it run.
    in.inter = comm_z && multi() && fused;
    in.can_split_z = in.can_split_q = in.inter && cone_split_enabled();
    for (auto &s : slabs) {
        in.can_split_z = in.can_split_z && s.fg.chunks >= 2;
        in.can_split_q = in.can_split_q && qstep_rhs_chunks(s.g, s.fg) >= 2;
    }
    return in;
}

static const double kUpdateRule[11][2] = {   // :39-51
    {1.1, 1.10}, {1.2, 1.15}, {1.5, 1.20}, {2, 1.26}, {2.5, 1.28}, {3.33, 1.32},
    {5, 1.35}, {10, 1.40}, {20, 1.60}, {40, 1.80}, {50, 2.00}};

static double get_factor(double xi) {   // adjust_lagrangianParam.m:49-60
    double factor = 1.0;
    for (int i = 0; i < 11; ++i) {
        if (xi >= kUpdateRule[i][0]) factor = kUpdateRule[i][1];
        else break;
    }
    return factor;
}

static void adjust_lagrangian_param(double &sigma, double xi, double &factor) {   // adjust_lagrangianParam.m:14-39
    factor = 1.0;
    if (xi >= 1) factor = get_factor(xi);
    else if (xi < 1) factor = 1.0 / get_factor(1.0 / xi);
    if (factor != 1.0) {
        const double old = sigma;
        sigma = std::max(std::min(sigma * factor, 1e3), 1e-3);
        factor = sigma / old;
    }
}

// solver_socp_inPALM.m:222-323
int Solver::kkt_block(bool adjustSigmaYes, bool timed_out, bool *brk, bool folded) {
    double S[S_COUNT + 1];
    prof_begin(PH_KKT);
    DS_CHECK(kkt_sums(S, folded));
    prof_end(PH_KKT);
    // one slab per process: the ranks must take the time-limit decision together, so it is taken
    // here from the maximum of their wall clocks (time-outs are detected at KKT checks only)
    if (remote()) timed_out = elapsed_agreed > time_limit;
    for (int i = 0; i < S_COUNT; ++i) last_S[i] = S[i];
    last_S_sigma = sigma;
    last_S_it = it;
    const double sh = sqrt(h);
    auto nrm = [&](int i) { return sh * sqrt(S[i]); };
    const double norm_q = nrm(S_Q2), norm_z = nrm(S_Z2), norm_Aphi = nrm(S_APHI2);
    const double norm_alpha = sigma * nrm(S_ALPHA2), norm_beta = sigma * nrm(S_BETA2);
    const double norm_FBbeta = sigma * nrm(S_FBBETA2);
    const double primFea1 = nrm(S_PRIM1), primFea2 = nrm(S_PRIM2);
    const double dualFea1 = sigma * nrm(S_DUAL1), dualFea2 = sigma * nrm(S_DUAL2);
    const double complem = nrm(S_COMPLEM);
    const double dotcomplem = nrm(S_DOTCOMP), normRho = nrm(S_RHO2), norm_rhoFq = nrm(S_RHOFQ2);
    const double mRhoB = nrm(S_MRHOB), normM = nrm(S_M2), normRhoB = nrm(S_RHOB2);
    const double kc = 1.0;
    const double den2 = prob.weighted ? (norm_q + norm_z) : norm_d;        // wsocp :256,265
    double org[7], res[5];
    org[0] = primFea1 / (kc * D / dScale + norm_Aphi + norm_q);
    org[1] = primFea2 / (kc * E / dScale + den2);
    org[2] = dualFea1 / (kc / cScale + norm_c);
    org[3] = complem / (kc * E / dScale + norm_z + norm_beta);
    org[4] = dualFea2 / (kc / cScale / D + norm_FBbeta + norm_alpha);
    org[5] = dotcomplem / (kc + normRho + norm_rhoFq);
    org[6] = mRhoB / (kc + normM + normRhoB);
    res[0] = primFea1 / (kc + norm_Aphi + norm_q);
    res[1] = primFea2 / (kc + den2);
    res[2] = dualFea1 / (kc + norm_c);
    res[3] = complem / (kc + norm_z + norm_beta);
    res[4] = dualFea2 / (kc + norm_FBbeta + norm_alpha);
    const double priVal = (sigma * cScale * dScale * h) * S[S_QALPHA];
    const double dualVal = (sigma * cScale * dScale * h) * S[S_CPHI];
    const double pdGap = fabs(priVal - dualVal) / (1 + fabs(priVal) + fabs(dualVal));
    for (int i = 0; i < 7; ++i) hist_kkt.push_back(org[i]);
    hist_time.push_back(remote() ? elapsed_agreed : elapsed());
    hist_iter.push_back((double)it);
    hist_gap.push_back(pdGap);
    // stop criterion (:287-290); stopCondition = [1,3,6,7] or [1,3,6] (:117-121)
    double mstop = std::max(std::max(org[0], org[2]), org[5]);
    if (checkPrimDualFeas) mstop = std::max(mstop, org[6]);
    if (mstop < opts.tol || timed_out) {
        *brk = true;
        return 0;
    }
    const double maxRes = *std::max_element(res, res + 5);
    if (maxRes < tol_feasOrg) use_feasOrg = 1;                              // :293-295
    if (adjustSigmaYes) {                                                   // :298-316
        lastSigmaIt = (double)it;
        double resiPri, resiDual;
        if (use_feasOrg) { resiPri = std::max(org[0], org[1]); resiDual = std::max(org[2], org[4]); }
        else { resiPri = std::max(res[0], res[1]); resiDual = std::max(res[2], res[4]); }
        double factor;
        adjust_lagrangian_param(sigma, resiPri / resiDual, factor);
        if (factor != 1.0) {
            if (folded && rhs_valid && method != DOTSOCP_METHOD_ACCADMM) DS_CHECK(sigma_scale_folded(factor));
            else DS_CHECK(scale_state(1.0, factor, 1.0, true));
            if (method == DOTSOCP_METHOD_ACCADMM) DS_CHECK(acc_on_sigma_factor(factor));
        }
    }
    if (rescale > 0) {                                                      // :319-322
        maxFeas = maxRes;
        relGap = pdGap;
    }
    return 0;
}

int Solver::step(bool *brk) {
    *brk = false;
    if (method == DOTSOCP_METHOD_ACCADMM) return acc_step(brk);
    if (method == DOTSOCP_METHOD_PALM) return palm_step(brk);
    it += 1;
    DS_CHECK(rescale_block());
    // the whole schedule of the iteration (schedule.h); the time limit is the one trigger it cannot know: a check it asks for
    // takes the unfolded path
    const StepIn in = step_in();
    const StepPlan plan = plan_step(in);
    if (plan.error) {
        set_error("internal: the early cone pass wrote %s, the schedule asks for %s", early_pass == QCONE_STEADY ? "gamma" : "beta",
                  plan.pass_gout ? "gamma" : "beta");
        return DOTSOCP_ESTATE;
    }
    // an exchange issued on the second streams without the join: fork, messages, mark
    auto async_comm = [&](const std::function<int()> &fn, SlabEvent ev) -> int {
        DS_CHECK(comm_fork());
        comm_async = true;
        const int rc = fn();
        comm_async = false;
        DS_CHECK(rc);
        return comm_mark(ev);
    };
    if (in.inter) {
        // [E2 + E1] the q halo and the u0 tail of the last q-step travel while the cone chunks in front of the last one
        // -- which alone reads the halo -- run
        const bool pend = halo_pending;
        if (pend) {
            DS_CHECK(make_u0_tail());
            DS_CHECK(async_comm([&]() { return ensure_halo(); }, EV_HALO));
        }
        if (plan.split_z) DS_CHECK(phase_z(plan, 1));
        if (pend) DS_CHECK(comm_wait(EV_HALO));
        if (!plan.split_z && plan.cone_launch) DS_CHECK(phase_z(plan, 0));
        // The phi-step.  The last cone chunk (and the finalising of its adjoint tails) runs while the second streams carry
        // the latency-bound middle of the Poisson solve (poisson_t_tridiag); the tails [E4] leave right behind that and
        // travel beside the rest of the solve and the front of the q-step
        PhiHooks hooks;
        hooks.fill = [&]() -> int {
            if (plan.split_z) DS_CHECK(phase_z(plan, 2));
            return make_tails();
        };
        hooks.behind = [&]() -> int { return async_comm([&]() { return send_tails(); }, EV_JOIN); };
        DS_CHECK(phase_phi(&hooks));
    } else {
        DS_CHECK(phase_phi());
        if (plan.cone_launch) DS_CHECK(phase_z(plan, 0));
    }
    if (plan.fold) {
        // every region of partial sums is cleared before the q-step writes region 0; kkt_sums() then only adds the cell,
        // border and (time slabs) first-layer launches
        FOR_SLABS(s) DS_CHECK(clear_partials(s));
    }
    if (in.inter) {
        // [E3] the phi head travels (behind the tails) while every chunk of the q-step but the last -- the only reader of
        // the phi halo -- runs; the tails (read by the first chunk) have had the second half of the phi-step to arrive
        DS_CHECK(async_comm([&]() { return send_phi_head(); }, EV_HALO));
        DS_CHECK(comm_wait(EV_JOIN));
        if (plan.split_q) DS_CHECK(phase_q(plan, 1));
        DS_CHECK(comm_wait(EV_HALO));
        DS_CHECK(phase_q(plan, plan.split_q ? 2 : 0));
    } else {
        DS_CHECK(ship_tails());      // time slabs: phi head -> left, adjoint tails -> right
        // the check a passed time limit asks for needs the state between two iterations: no early pass then
        const bool early_ok = plan.qcone_candidate != QCONE_NONE && !time_limit_passed();
        DS_CHECK(phase_q(plan, 0, early_ok ? plan.qcone_candidate : QCONE_NONE));
    }
    DS_CHECK(phase_mult());
    const bool timed_out = time_limit_passed();
    timeout_pending = false;
    if (timed_out && timeout_check_waits(beta_gamma, early_pass != QCONE_NONE)) {
        timeout_pending = true;      // taken at the end of the next iteration that writes beta, which then stops
        return 0;
    }
    if (plan.kkt_due || timed_out)                                                        // :221
        DS_CHECK(kkt_block(plan.adjust_sigma, timed_out, brk, plan.fold));
    return 0;
}

int Solver::run(i64 n_iters, i64 *done) {
    if (!begun || finished) { set_error("run() needs begin() and must precede finish()"); return DOTSOCP_ESTATE; }
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    // while the loop runs, whatever enqueues work on a slab's streams is issued by that slab's own host thread (defer.h)
    struct DeferScope {
        DeferCtx *ctx;
        int err = 0;
        explicit DeferScope(DeferCtx *c) : ctx(c) { if (ctx) { g_defer = ctx; ctx->begin(); } }
        int close() { if (ctx) { err = ctx->end(); g_defer = nullptr; ctx = nullptr; } return err; }
        ~DeferScope() { (void)close(); }
    } scope(defer.get());
    i64 n = 0;
    while (it < opts.maxit && !stopped) {
        if (n_iters >= 0 && n >= n_iters) break;
        bool brk = false;
        run_left = (n_iters >= 0) ? n_iters - n : -1;
        DS_CHECK(step(&brk));
        if (brk) stopped = true;
        ++n;
    }
    DS_CHECK(need_beta_form("the end of run()"));
    DS_CHECK(need_q("the end of run()"));
    if (early_pass != QCONE_NONE) { set_error("internal: an early cone pass is pending at the end of run()"); return DOTSOCP_ESTATE; }
    DS_CHECK(ensure_halo());          // callers between run() calls see exchanged halos
    DS_CHECK(sync_all());
    DS_CHECK(prof_flush());
    if (const int derr = scope.close()) {
        set_error("a HIP call issued by a slab thread failed: %s", hipGetErrorString((hipError_t)derr));
        return DOTSOCP_EHIP;
    }
    if (done) *done = n;
    return 0;
}

int Solver::finish(dotsocp_result *res) {
    if (!begun) { set_error("finish() before begin()"); return DOTSOCP_ESTATE; }
    cur_dev = -1;
    DS_CHECK(use_dev(device));
    DS_CHECK(ensure_z());
    DS_CHECK(flush_beta());
    DS_CHECK(flush_alpha());
    DS_CHECK(sync_all());
    DS_CHECK(prof_flush());
    if (canary_enabled()) {        // DOTSOCP_CANARY=1: no kernel of this solve wrote outside its buffers
        std::string rep;
        const int bad = canary_check(&rep);
        cur_dev = -1;
        if (bad) {
            set_error("canary: %d device buffer(s) written out of bounds: %s", bad, rep.c_str());
            return DOTSOCP_EHIP;
        }
    }
    finished = true;
    if (res) {
        memset(res, 0, sizeof *res);
        res->sigma = sigma / sigmaScale;        // :357
        res->sigma_internal = sigma;
        res->cScale = cScale;
        res->dScale = dScale;
        // device time per step (HIP events) when profiling is on; Total_Time is host wall time
        res->times[0] = (phase_ms[PH_RHS] + phase_ms[PH_POISSON]) * 1e-3;
        res->times[1] = (phase_ms[PH_PROJ] + phase_ms[PH_FUSED_A] + phase_ms[PH_FUSED_B] + phase_ms[PH_CONE_CARRY]) * 1e-3;
        res->times[2] = phase_ms[PH_QSTEP] * 1e-3;
        res->times[3] = (phase_ms[PH_BETA] + phase_ms[PH_MATERIALISE]) * 1e-3;
        res->times[4] = phase_ms[PH_KKT] * 1e-3;
        res->times[5] = elapsed();
        res->times[6] = (double)it;
        res->iters = it;
        res->hist_len = (i64)hist_iter.size();
        res->stopped = stopped ? 1 : 0;
        if (method == DOTSOCP_METHOD_PALM) res->time_extra = phase_ms[PH_QSTEP0] * 1e-3;   // 'Step_1_Q_Step'
        if (method == DOTSOCP_METHOD_ACCADMM) {
            // Step_1_Q_Step, Step_2_Multiplier (folded into the cone pass), Step_3_1_FFT, Step_3_2_ProjSOC, KKT, Interp
            res->times[0] = (phase_ms[PH_RHS] + phase_ms[PH_POISSON]) * 1e-3;
            res->times[1] = phase_ms[PH_ACC_CONE] * 1e-3;
            res->times[2] = (phase_ms[PH_QSTEP] + phase_ms[PH_ACC_GATHER]) * 1e-3;
            res->times[3] = 0.0;
            res->time_extra = phase_ms[PH_INTERP] * 1e-3;
        }
    }
    return 0;
}
// --------------------------------------------------------------------------------------
// profiling helpers
// --------------------------------------------------------------------------------------
void Solver::prof_begin(int phase, bool on_z) {
    if (!profiling) return;
    (void)use_dev(device);
    hipStream_t st = on_z ? stream_z : stream;
    Pending p;
    p.phase = phase;
    auto get = [&]() {
        hipEvent_t e;
        if (!event_pool.empty()) { e = event_pool.back(); event_pool.pop_back(); }
        else (void)hipEventCreate(&e);
        return e;
    };
    p.a = get();
    p.b = get();
    (void)ds_event_record(p.a, st);
    pending.push_back(p);
}

void Solver::prof_end(int phase, bool on_z) {
    if (!profiling) return;
    (void)use_dev(device);
    hipStream_t st = on_z ? stream_z : stream;
    for (auto it2 = pending.rbegin(); it2 != pending.rend(); ++it2)
        if (it2->phase == phase) { (void)ds_event_record(it2->b, st); break; }
}

int Solver::prof_flush() {
    if (!profiling || pending.empty()) return 0;
    DS_CHECK(use_dev(device));
    DS_HIP(ds_stream_synchronize(stream_z));
    DS_HIP(ds_stream_synchronize(stream));
    for (auto &p : pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            phase_ms[p.phase] += ms;
            phase_launches[p.phase] += 1;
        }
        event_pool.push_back(p.a);
        event_pool.push_back(p.b);
    }
    pending.clear();
    return 0;
}

double Solver::elapsed() const {
    return elapsed_prev + std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
}

}  // namespace dotsocp
