// The planner of the inPALM loop (dot-socp_amd/csrc/schedule.h) driven as Solver::step() / Solver::run() drive it, without a
// device: plan_step() for iterations 1..400, the early form, what the multiplier array holds and a pending time-out carried
// from one plan to the next; KKT checks and the rescale block change the state as in tests/test_qcone_schedule.py.  Over
// that test's grid (maxit, step-by-step checks, run() in pieces, scaling / feasibility) and, beyond it, with a time limit
// that passes at iteration T, seen in front of the q-step or only behind the body:
//   - every reader of beta or q (KKT check, rescale block, end of run()) finds the beta form, a stored q, no early pass pending;
//   - an early pass is only handed to an iteration whose plan agrees with it (StepPlan::error is never set);
//   - step-by-step checks: no early pass at all; the plain 400-iteration run: > 200 steady and >= 10 exit forms;
//   - the stopping check comes at most two iterations after the limit passed; seen at 6 on the default cadence the checks
//     are [1, 4, 7], and with DOTSOCP_CONE_CARRY=0 the loop stops at 6.
#include <cmath>
#include <cstdio>
#include <vector>

#include "schedule.h"

using namespace dotsocp;

static int failed = 0, checked = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        ++checked;                                        \
        if (!(cond)) {                                    \
            ++failed;                                     \
            printf("FAILED %s: ", #cond);                 \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
        }                                                 \
    } while (0)

struct Case {
    long long maxit;
    bool step_by_step;
    std::vector<long long> runs;    // run(n) calls; run(-1) follows them
    bool scaling;
    long long feas1, feas2;         // from these iterations on a check finds the first / second rescale's feasibility (-1: never)
    bool cone_carry, qcone;
    long long limit_at;             // the time limit passes at this iteration (-1: never) ...
    bool limit_in_front;            // ... and its q-step sees it (else only the sample behind the body does)
};

struct Outcome {
    std::vector<long long> checks;
    long long n_steady = 0, n_exit = 0, stopped_at = -1;
};

static Outcome drive(const Case &c, const char *name) {
    Outcome out;
    // ---- the loop state of Solver (begin())
    long long it = 0;
    double lastSigmaIt = -INFINITY, maxFeas = INFINITY, relGap = INFINITY;
    int rescale = c.scaling ? 1 : 0;
    bool deferred = false, beta_gamma = false, q_valid = true, timeout_pending = false, stopped = false;
    int early = QCONE_NONE;
    auto reader = [&](const char *who) {
        CHECK(!beta_gamma && q_valid && early == QCONE_NONE, "%s: %s at iteration %lld: gamma %d, q stored %d, early form %d", name, who,
              it, (int)beta_gamma, (int)q_valid, early);
    };
    std::vector<long long> runs = c.runs;
    runs.push_back(-1);
    for (const long long n_iters : runs) {
        long long n = 0;
        while (it < c.maxit && it < 400 && !stopped) {             // Solver::run()
            if (n_iters >= 0 && n >= n_iters) break;
            ++n;
            it += 1;                                               // Solver::step()
            // ---- the rescale block: the norm check leaves the multiplier step pending, a rescale executes it
            if (rescale_due(it, rescale, maxFeas, relGap)) {
                reader("rescale block");
                if (rescale_trigger(it, rescale, maxFeas, relGap) || it % 200 == 0) {
                    rescale += 1;
                    deferred = false;
                }
            }
            StepIn in{};
            in.s = SchedState{it, c.maxit, lastSigmaIt, c.step_by_step, rescale, maxFeas, relGap, n_iters >= 0 ? n_iters - (n - 1) : -1};
            in.fused = true;
            in.deferred = deferred;
            in.cone_carry = c.cone_carry;
            in.kkt_fold = true;
            in.beta_gamma = beta_gamma;
            in.timeout_pending = timeout_pending;
            in.early = early;
            in.qcone_eligible = c.qcone;
            const StepPlan p = plan_step(in);
            CHECK(!p.error, "%s: iteration %lld was handed the early form %d, its own schedule writes %s", name, it, early,
                  p.pass_gout ? "gamma" : "beta");
            if (p.error) return out;
            // ---- the cone pass: launched now (it reads q from memory), or run by the last q-step
            if (p.cone_launch) {
                CHECK(q_valid, "%s: the cone pass of iteration %lld met a q that was never stored", name, it);
                CHECK(!beta_gamma || deferred, "%s: iteration %lld reads gamma without a pending multiplier step", name, it);
                if (deferred) beta_gamma = p.pass_gout;
            } else {
                CHECK(deferred && beta_gamma == (early == QCONE_STEADY), "%s: early pass of iteration %lld", name, it);
            }
            CHECK(p.gamma_after == beta_gamma, "%s: iteration %lld leaves gamma %d, planned %d", name, it, (int)beta_gamma, (int)p.gamma_after);
            CHECK(!p.fold || p.kkt_due, "%s: iteration %lld folds without a check", name, it);
            // ---- the q-step; the clock is sampled in front of it only for a candidate
            const bool past = c.limit_at > 0 && it >= c.limit_at;
            const bool seen_in_front = timeout_pending || (past && (c.limit_in_front || it > c.limit_at));
            early = (p.qcone_candidate != QCONE_NONE && !seen_in_front) ? p.qcone_candidate : QCONE_NONE;
            if (early != QCONE_NONE) {
                CHECK(!p.fold && deferred && beta_gamma, "%s: early pass in a state it does not serve, iteration %lld", name, it);
                beta_gamma = (early == QCONE_STEADY);
            }
            q_valid = early != QCONE_STEADY;
            out.n_steady += early == QCONE_STEADY;
            out.n_exit += early == QCONE_EXIT;
            deferred = true;                                       // phase_mult()
            // ---- the tail: the clock again, and the check
            const bool timed_out = timeout_pending || past;
            timeout_pending = false;
            if (timed_out && timeout_check_waits(beta_gamma, early != QCONE_NONE)) {
                timeout_pending = true;
                continue;
            }
            if (!(p.kkt_due || timed_out)) continue;
            reader("KKT check");
            out.checks.push_back(it);
            deferred = false;                                      // the check executes the pending multiplier step
            if (timed_out) {
                stopped = true;
                out.stopped_at = it;
                continue;
            }
            if (p.adjust_sigma) lastSigmaIt = (double)it;
            if (rescale == 1 && c.feas1 >= 0 && it >= c.feas1) maxFeas = relGap = 1e-2;
            if (rescale == 2 && c.feas2 >= 0 && it >= c.feas2) maxFeas = relGap = 1e-3;
        }
        reader("the end of run()");
    }
    CHECK(stopped || !timeout_pending || it < c.maxit, "%s: the loop ended at maxit with a time-out check still waiting", name);
    return out;
}

int main() {
    const std::vector<std::vector<long long>> splits = {{}, {7, 5}, std::vector<long long>(30, 1), {2, 3, 1, 40, 1, 1, 99, 100, 57}};
    const long long feas[5][3] = {{0, -1, -1}, {1, 7, 33}, {1, 3, 58}, {1, 64, 64}, {1, 9, -1}};
    char name[160];
    for (const long long maxit : {400LL, 37LL})
        for (const bool sbs : {false, true})
            for (size_t k = 0; k < splits.size(); ++k)
                for (const auto &f : feas)
                    for (const bool carry : {true, false})
                        for (const bool qcone : {true, false}) {
                            // ---- no time limit: the grid of tests/test_qcone_schedule.py
                            Case c{maxit, sbs, splits[k], f[0] != 0, f[1], f[2], carry, qcone, -1, false};
                            snprintf(name, sizeof name, "maxit %lld sbs %d split %zu feas %lld/%lld carry %d qcone %d", maxit, (int)sbs, k,
                                     f[1], f[2], (int)carry, (int)qcone);
                            const Outcome o = drive(c, name);
                            CHECK(o.stopped_at < 0, "%s: stopped without a time limit", name);
                            if (sbs || !carry || !qcone) CHECK(o.n_steady == 0 && o.n_exit == 0, "%s: %lld steady, %lld exit", name, o.n_steady, o.n_exit);
                            else if (maxit == 400 && k == 0) CHECK(o.n_steady > 200 && o.n_exit >= 10, "%s: %lld steady, %lld exit", name, o.n_steady, o.n_exit);
                            // ---- the time limit passes at iteration T
                            for (long long T = 1; T <= 40; ++T)
                                for (const bool in_front : {true, false}) {
                                    Case ct = c;
                                    ct.limit_at = T;
                                    ct.limit_in_front = in_front;
                                    snprintf(name, sizeof name, "maxit %lld sbs %d split %zu feas %lld/%lld carry %d qcone %d limit at %lld (%s)",
                                             maxit, (int)sbs, k, f[1], f[2], (int)carry, (int)qcone, T, in_front ? "in front" : "behind");
                                    const Outcome t = drive(ct, name);
                                    if (T <= maxit) {
                                        const long long bound = T + 2 < maxit ? T + 2 : maxit;
                                        CHECK(t.stopped_at >= T && t.stopped_at <= bound, "%s: stopped at %lld", name, t.stopped_at);
                                        CHECK(!t.checks.empty() && t.checks.back() == t.stopped_at, "%s: the last check is not the stop", name);
                                        if (!carry) CHECK(t.stopped_at == T, "%s: without the gamma form the stop is immediate, got %lld", name, t.stopped_at);
                                    }
                                }
                        }
    // ---- the numbers DESIGN.md and tests/test_gpu_cone_carry.py pin: default cadence, the limit seen at iteration 6
    for (const bool qcone : {true, false}) {
        const Outcome o = drive(Case{400, false, {}, false, -1, -1, true, qcone, 6, true}, "limit at 6");
        CHECK(o.checks == std::vector<long long>({1, 4, 7}) && o.stopped_at == 7, "limit at 6 (qcone %d): stopped at %lld after %zu checks",
              (int)qcone, o.stopped_at, o.checks.size());
        const Outcome p = drive(Case{400, false, {}, false, -1, -1, false, qcone, 6, true}, "limit at 6, no carry");
        CHECK(p.checks == std::vector<long long>({1, 4, 6}) && p.stopped_at == 6, "limit at 6, cone_carry off (qcone %d): stopped at %lld",
              (int)qcone, p.stopped_at);
    }
    // ---- the ABI's two flags as run_left (capi.hip): last -> 1, next last -> 2, neither -> no bound
    const SchedState plain{5, 400, 4.0, false, 0, INFINITY, INFINITY, -1};
    SchedState s = plain;
    CHECK(qcone_form(s) == QCONE_STEADY, "plain iteration 5");
    s.run_left = 2;
    CHECK(qcone_form(s) == QCONE_EXIT && !cone_writes_beta(s), "iteration 6 ends the run");
    s.run_left = 1;
    CHECK(qcone_form(s) == QCONE_NONE && cone_writes_beta(s), "iteration 5 ends the run");
    CHECK(check_scheduled(401, 400.0, 400, false) && !check_scheduled(399, 398.0, 400, false), "it >= maxit");
    printf("%d checked, %d failed\n", checked, failed);
    return failed ? 1 : 0;
}
