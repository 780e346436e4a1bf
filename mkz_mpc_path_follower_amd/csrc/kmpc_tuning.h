/* kmpc_tuning.h -- the ONE definition of every solver constant this project tuned beyond Ipopt's published defaults (those stay where they are used).
 * Plain C, no includes: the kernels read it through kmpc_common.h, the CPU checker compiles it as C99.  -DKMPC_...= builds can A/B each value. */
#ifndef KMPC_TUNING_H
#define KMPC_TUNING_H

/* Non-convex phase (ipm::solve in kmpc_ipm.h).  Chosen on the pooled worst-of-4096 statistics of 48 seeded 4096-problem batches:
 * shift growth after a failed first trial 8 -> 3 (the first trial is last/3, so x3 returns to the shift that worked last iteration instead of
 * overshooting it 2.7-fold), barrier floor in shifted iterations rd/1000 -> rd/100 (-> rd/40 later in round 3).
 * The barrier floors are stated as the factor the kernels multiply the scaled dual infeasibility by; the CPU checker divides by 1.0 / KMPC_IKRD and
 * 1.0 / KMPC_IKRD_NC, which are exactly 1000.0 and 40.0 in fp64. */
#ifndef KMPC_IKRD
#define KMPC_IKRD 1e-3
#endif
#ifndef KMPC_IKRD_NC
#define KMPC_IKRD_NC 2.5e-2   /* (rd/100 until the hybrid strategy switched at the first failure; re-measured on 12 pooled batches: rd/40) */
#endif
#ifndef KMPC_DW_GROW
#define KMPC_DW_GROW 3
#endif
/* The rest of the shift schedule: the first shift of a solve relative to max |sc H_jj| (Ipopt's 1e-4 / x100 lands 1-2 decades above what is needed); the
 * divisor from the last shift that worked to the next first trial; the first-trial successes in a row after which the unshifted matrix is tried first
 * again (a decaying shift slows the end game of the solves that have left the non-convex region). */
#ifndef KMPC_DW_FIRST
#define KMPC_DW_FIRST 1e-2
#endif
#ifndef KMPC_DW_DECAY
#define KMPC_DW_DECAY 3
#endif
#ifndef KMPC_ZERO_AFTER
#define KMPC_ZERO_AFTER 2
#endif
/* Hybrid indefinite-Hessian strategy: failed exact factorisations before shift mode replaces the Gauss-Newton fallback.  One up to N = 28 on cold starts
 * (pooled worst of 4096: 25.75 -> 23.52 at N = 20, mean unchanged); two at long horizons (mean +4.6 % at N = 50) and on warm starts (shift mode stalls at mu = 1e-6). */
#ifndef KMPC_SHIFT_AFTER
#define KMPC_SHIFT_AFTER(N, warm) (((N) >= 32 || (warm)) ? 2 : 1)
#endif
/* Iterations spent on the duality-gap bound once Ipopt's test has been met (below mu ~ 1e-11 round-off defeats the line search). */
#ifndef KMPC_MAX_POLISH
#define KMPC_MAX_POLISH 1
#endif
/* A trial point is also accepted when the PREDICTED decrease of the merit function is below the noise of its evaluation, KMPC_NOISE_ACCEPT * eps * |phi|
 * (the cost is resolved to ~50-70 eps: e = x - x_ref carries eps |x| with |x| >> |e|; Ipopt's 10 eps slack is not enough): near a low-cost optimum the
 * Armijo test otherwise fails on rounding alone and the search backtracks max_ls times (~100 wasted roll-outs on ~0.25 % of the problems) */
#ifndef KMPC_NOISE_ACCEPT
#define KMPC_NOISE_ACCEPT 100
#endif
/* barrier floor without its mu_cur cap after an accepted step shorter than this (kmpc_ipm.h, the Mehrotra barrier update): un-sticks warm starts from a wrong point */
#ifndef KMPC_UNSTICK
#define KMPC_UNSTICK 1e-4
#endif
/* Degenerate complementarity pairs (slack and multiplier vanish together -- structurally the last acceleration input a_{N-1}, which only the rate cost
 * ties to a_{N-2}: whenever the acceleration saturates to the end of the horizon its bound is active with a zero multiplier).  Newton's method treats such
 * a pair as a double root: s and lambda halve per iteration (x0.375 with Mehrotra's corrector), five to eight iterations of end game.  A pair seen
 * shrinking that way enters the KKT matrix with theta * lambda/s (theta < 1 lengthens its step: s+ = 0.13 s at theta = 0.6; below 0.45 the corrected
 * step overshoots the bound and the fraction-to-the-boundary rule cuts EVERY component).  K stays positive definite and the right-hand side is the
 * barrier gradient, so the direction is a descent direction of phi_mu as before.  CPU port, 12 x 4096 seeded problems at N = 20: mean iterations 7.45 ->
 * 7.10, E[worst of 4096] 21.7 -> 19.6; same minima (costs agree to 2e-8).  0.75: 20.1; 0.5: 19.4; 0.4: 25.6. */
#ifndef KMPC_DEGEN_THETA
#define KMPC_DEGEN_THETA 0.6
#endif
/* Run-time guard of the slack iterates (kmpc_ipm.h, ipm::solve): an iterate is reported Optimal only if every live slack agrees with the freshly
 * evaluated b -/+ a_f^T U to this tolerance, relative to max(1, |bound|, |a_f^T U|).  Rounding alone: <= 2.7e-15 (fp64) / <= 1.6e-6 (fp32) measured over
 * seeded draws of up to 262 144 problems at N = 8 ... 50, every kernel family (tools/drift_probe.py -> profiles/r4_slack_drift.txt) -- the tolerances sit
 * five / two decades above that, and two / one decade below the drift that moved round 3's non-KKT "Optimal" (complementarity 9e-3). */
#ifndef KMPC_DRIFT_TOL_F64
#define KMPC_DRIFT_TOL_F64 1e-9
#endif
#ifndef KMPC_DRIFT_TOL_F32
#define KMPC_DRIFT_TOL_F32 1e-4
#endif

#endif
