// The schedule of one inPALM / ALG2 iteration: which iterations end in a KKT check, what the cone pass reads and leaves in
// the multiplier array (solver.h: the gamma form), whether the q-step also runs the next iteration's pass (solver.h: the
// early cone pass).  Every predicate is stated here once; plan_step() decides an iteration at the top of Solver::step() and
// the phases execute the plan.  Plain host arithmetic without HIP and without a clock: tests/san/sched_check.cpp drives it.
// (Not called sched.h: this directory is on the include path of host builds, where that name would shadow POSIX <sched.h>.)
#pragma once

namespace dotsocp {

inline bool if_adjust_sigma(double iter, double last_iter) {   // IfAdjustSigma (solver_socp_inPALM.m:361-379)
    const double passed = iter - last_iter;
    if (iter < 20 && passed >= 3) return true;
    if (iter < 50 && passed >= 6) return true;
    if (iter < 100 && passed >= 10) return true;
    if (iter < 200 && passed >= 15) return true;
    if (iter < 500 && passed >= 25) return true;
    return passed >= 40;
}
// Iteration `it` ends in a KKT check known at its start (:220-221; the loops add their time-limit terms).  Inside a loop
// it <= maxit holds; cone_writes_beta asks about it + 1 as well, hence >=.
inline bool check_scheduled(long long it, double lastSigmaIt, long long maxit, bool stepByStep) {
    return stepByStep || if_adjust_sigma((double)it, lastSigmaIt) || it >= maxit;
}
// The rescale block of iteration `it` (:138-151): the norm check every 100 iterations, the two rescales by feasibility;
// rescale_due: it takes its norms or rescales, given the state it finds -- it reads beta and q
inline bool norm_check_due(long long it, int rescale) { return rescale >= 3 && (it % 100) == 0; }
inline bool rescale_trigger(long long it, int rescale, double maxFeas, double relGap) {
    return (rescale == 1 && maxFeas < 2e-2 && it >= 10 && relGap < 5e-2) ||
           (rescale == 2 && maxFeas < 5e-3 && it >= 50 && relGap < 1e-2);
}
inline bool rescale_due(long long it, int rescale, double maxFeas, double relGap) {
    return norm_check_due(it, rescale) || rescale_trigger(it, rescale, maxFeas, relGap);
}

// What the schedule of iteration `it` depends on; all but `it` and run_left changes at KKT checks and rescales only
struct SchedState {
    long long it, maxit;
    double lastSigmaIt;
    bool checkStepByStep;
    int rescale;
    double maxFeas, relGap;
    long long run_left;     // iterations this run() call still has, counting `it`; negative: no bound
};
// the state iteration it + 1 finds if `it` has no check and it + 1 does not rescale
inline SchedState next_iteration(SchedState s) {
    s.it += 1;
    if (s.run_left > 0) s.run_left -= 1;
    return s;
}
// The cone pass of iteration `it` must leave beta (not gamma) behind: the iteration ends in a KKT check, ends the run()
// call (the caller may read anything), or the next iteration's rescale block reads beta.
inline bool cone_writes_beta(const SchedState &s) {
    return check_scheduled(s.it, s.lastSigmaIt, s.maxit, s.checkStepByStep) || (s.run_left >= 0 && s.run_left <= 1) ||
           rescale_due(s.it + 1, s.rescale, s.maxFeas, s.relGap);
}
// The q-step of iteration `it` also runs the cone pass of it + 1.  QCONE_NONE: the pass of `it` writes beta, so a reader
// of beta or q follows it; else the form of the early pass is the schedule of it + 1: QCONE_EXIT if that pass must leave
// beta (and q in memory), QCONE_STEADY if it leaves gamma.
enum { QCONE_NONE = 0, QCONE_STEADY = 1, QCONE_EXIT = 2 };
inline int qcone_form(const SchedState &s) {
    if (cone_writes_beta(s)) return QCONE_NONE;
    return cone_writes_beta(next_iteration(s)) ? QCONE_EXIT : QCONE_STEADY;
}
// A check asked for by the time limit is not scheduled, and it reads beta and q: it waits for the end of the next iteration
// that writes beta while the multiplier array holds gamma, or while an early pass has already moved the state into the
// middle of the next iteration (whatever that pass wrote).
inline bool timeout_check_waits(bool gamma_left, bool early_pending) { return gamma_left || early_pending; }

struct StepIn {             // what Solver::step() knows at its top, behind the rescale block
    SchedState s;
    bool fused, deferred, cone_carry, kkt_fold;
    bool beta_gamma;        // the multiplier array holds gamma (as the last pass left it, an early one included)
    bool timeout_pending;   // the time limit passed in an iteration whose check had to wait
    int early;              // QCONE_*: the form in which the last q-step ran this iteration's cone pass
    bool qcone_eligible;    // all that is static about the early pass: switch, one slab, unweighted, method, tile shape and count
    bool inter;             // time slabs with the messages on the second streams
    bool can_split_z, can_split_q;   // every slab's cone pass / q-step has a last chunk to set apart
};
struct StepPlan {
    bool adjust_sigma, kkt_due, fold, split_z, split_q;
    bool cone_launch;       // false: the pass ran inside the last q-step
    bool pass_gout;         // the pass writes gamma (it reads what the array holds)
    bool gamma_after;       // the multiplier array behind this iteration's pass
    int qcone_candidate;    // the form this q-step's early pass takes if the clock in front of it allows one
    bool error;             // the early pass handed over contradicts this iteration's schedule
};

inline StepPlan plan_step(const StepIn &in) {
    StepPlan p{};
    const SchedState &s = in.s;
    p.adjust_sigma = if_adjust_sigma((double)s.it, s.lastSigmaIt);                         // :220
    // A pending timed-out check runs (folded) at the end of this iteration -- unless a steady early pass has already run
    // this iteration's pass and left gamma and no q: then it waits once more (no further early pass is issued past the limit).
    p.kkt_due = check_scheduled(s.it, s.lastSigmaIt, s.maxit, s.checkStepByStep) ||
                (in.timeout_pending && !timeout_check_waits(in.early == QCONE_STEADY, false));
    // (cone_writes_beta covers every term of kkt_due but the pending time-out)
    p.pass_gout = in.cone_carry && in.fused && in.deferred && !p.kkt_due && !cone_writes_beta(s);
    // fused dataflow: the q-step of a checking iteration accumulates its share of the KKT sums itself
    p.fold = p.kkt_due && in.kkt_fold && in.fused;
    p.split_z = in.inter && in.can_split_z;
    p.split_q = in.inter && in.can_split_q;
    p.cone_launch = (in.early == QCONE_NONE);
    p.error = !p.cone_launch && (p.split_z || !in.fused || !in.deferred || p.pass_gout != (in.early == QCONE_STEADY));
    if (p.error) return p;
    // a deferred pass stores what it was scheduled to; a first pass (nothing pending) and an early one leave the array's form
    p.gamma_after = (p.cone_launch && in.deferred) ? p.pass_gout : in.beta_gamma;
    // behind a pass that left gamma nothing waits on beta: no scaling is pending (the pass applied it), no check follows
    if (in.qcone_eligible && !p.fold && in.deferred && p.gamma_after) p.qcone_candidate = qcone_form(s);
    return p;
}

}  // namespace dotsocp
