// The stopping rule of the s-step GMRES (gmres_sstep.hip) as host arithmetic alone: plain C++17, no HIP, no device access.
// The solver forms trial solutions xt and their true residuals (its trial() / commit(), the device work) and reports three
// events; the rule answers what to do with xt and how to go on.
//
// The recurrence residual of a block basis of condition kappa is good to about eps * kappa, so a convergence claim of the
// recurrence (rec <= tol_abs) is checked against the true residual ta of the trial solution before it is accepted.
#pragma once
#include <algorithm>

namespace fedd {

struct StopRule {
    enum Keep {
        NONE,        // xt is not wanted
        COMMIT,      // x <- xt (r and ||r||^2 already belong to it)
        RECOMPUTE    // x stays: r, ||r||^2 of x again
    };
    enum Next { GO_ON, RESTART, STOP };
    struct Answer {
        Keep keep;
        Next next;
    };

    const double rtol, beta0;
    const double T;                 // rtol * beta0: the target of the true residual
    double tol_abs;                 // target of the recurrence residual; tightened when the true residual lags behind it
    double last_true;               // true residual of x
    int floor_restarts = 0;         // restarts taken because the true residual stopped following the recurrence
    int nfail = 0;                  // claims of the recurrence that the true residual did not confirm
    double best_fail = 1e300;       // ... and the smallest true residual among them
    int stalls = 0;
    int s_cur;                      // block length from here on
    int its = 0;
    double relres;
    bool done = false;
    int floor = 0;                  // fedd_gmres_status: 1 = rounding floor of b - A x reached, 2 = no progress in three cycles
    double rec_relres = -1.0;       // floor 1: the recurrence residual beside the true one that is reported

    StopRule(double rtol_, double beta0_, int s_start)
        : rtol(rtol_), beta0(beta0_), T(rtol_ * beta0_), tol_abs(rtol_ * beta0_), last_true(beta0_), s_cur(s_start),
          relres(1.0) {}

    // measured on the Laplace cubes (monomial basis): the recurrence parts from the true residual near 1e-11 for s = 8 and
    // near 2e-13 for s = 4.  Below those floors a claim fails its check and costs a restart, so tight tolerances take
    // shorter blocks from the start.  (tol_blocks false lifts the cap: runs that are held to an iteration count instead of
    // a tolerance)
    static int s_tol(bool tol_blocks, double rtol) { return !tol_blocks || rtol >= 1e-9 ? 16 : (rtol >= 1e-11 ? 5 : 3); }

    // recurrence residual after a new column: does it claim convergence?
    bool column(double rec) {
        relres = rec / beta0;
        return rec <= tol_abs;
    }
    // x was projected at the start of a cycle: ta is its true residual
    void projected(double ta) {
        last_true = ta;
        relres = ta / beta0;
    }
    // the block basis became dependent after sa_eff columns: shorter blocks from here on
    void cut(int sa_eff) { s_cur = std::max(1, sa_eff); }

    // a claim of the recurrence (rec <= tol_abs) with `cols` columns of this cycle
    Answer claim(int cols, double rec, double ta) {
        if (ta <= T) {
            its += cols;
            relres = ta / beta0;
            return stop(COMMIT);
        }
        if (nfail >= 1 && ta >= 0.5 * best_fail && ta <= 100.0 * rtol * beta0) {
            its += cols;
            if (floor_restarts < 1) {
                // the true residual has stopped following the recurrence.  That is either the rounding floor of b - A x or
                // only the floor of THIS cycle's recurrence (a cycle is good to about eps * kappa(block basis) relative to
                // the residual it started from): one restart from the true residual tells them apart -- a new cycle reaches
                // the target if it is reachable (the effect of iterative refinement)
                ++floor_restarts;
                const Keep keep = keep_if_better(ta, false);
                nfail = 0;
                best_fail = 1e300;
                tol_abs = rtol * beta0;
                return restart(keep);
            }
            // the recurrence keeps falling, the true residual of the computed x does not follow any more: b - A x has
            // reached its rounding floor (badly scaled systems, tolerances near 1e-13).  The one-vector solvers stop on the
            // recurrence alone; here the iteration ends once the floor is evident.  What is reported is the TRUE residual
            // (it may exceed rtol by up to 100x: the caller sees that); fedd_gmres_status tells that the floor was reached
            // and gives the recurrence residual beside it.
            relres = ta / beta0;
            floor = 1;
            rec_relres = rec / beta0;
            return stop(COMMIT);
        }
        ++nfail;
        best_fail = std::min(best_fail, ta);
        if (ta > 4.0 * std::max(rec, 1e-300) || !(ta < last_true)) {
            // the recurrence has lost touch with the true residual: keep what was gained, restart
            its += cols;
            const Keep keep = keep_if_better(ta, true);
            s_cur = std::max(1, s_cur / 2);
            return restart(keep);
        }
        tol_abs *= 0.9 * rtol * beta0 / ta;
        return Answer{NONE, GO_ON};
    }

    // the Krylov space is exhausted after k vectors (or numerically so): the true residual decides
    Answer breakdown(int k, double ta) {
        its += k;
        const Keep keep = keep_if_better(ta, true);
        return last_true <= T ? stop(keep) : restart(keep);
    }

    // cycle used up (restart length or iteration limit) with `cols` columns
    Answer cycle_used_up(int cols, double ta) {
        its += cols;
        if (ta < 0.999 * last_true) stalls = 0;
        else ++stalls;
        const Keep keep = keep_if_better(ta, false);
        const Answer a = restart(keep);   // (three stalls are noted even where the target is met)
        return last_true <= T ? stop(keep) : a;
    }

private:
    // x <- xt if its true residual is the smaller one, else x stays (count_stall: ... and that counts as a cycle without progress)
    Keep keep_if_better(double ta, bool count_stall) {
        const bool better = ta < last_true;
        if (better) last_true = ta;
        else if (count_stall) ++stalls;
        relres = last_true / beta0;
        return better ? COMMIT : RECOMPUTE;
    }
    Answer stop(Keep keep) {
        done = true;
        return Answer{keep, STOP};
    }
    // a new cycle, unless three cycles in a row made no progress: then the caller gets the residual reached
    Answer restart(Keep keep) {
        if (stalls < 3) return Answer{keep, RESTART};
        floor = 2;
        return Answer{keep, STOP};
    }
};

}  // namespace fedd
