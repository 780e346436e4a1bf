/*
 * include/kmpc.h -- C ABI of the MI355X batched kinematic-bicycle MPC solver.
 *
 * Drop-in boundary for ONE path of govvijaycal/mkz_mpc_path_follower: the per-step
 * nonlinear MPC solve that scripts/mpc_cmd_pub.jl:115-141 delegates to the Julia module
 * scripts/mpc_utils/MKZMPCPathFollower.jl (JuMP model + Ipopt).  The reference has no FFI
 * for this path (it is an in-process Julia module with global state); the entry points
 * below are what a binding for it would bind -- each cites the module function / global
 * it replaces.  INTEGRATION.md shows the Julia `ccall` and Python `ctypes` stubs.
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; `stream` is a hipStream_t passed as void*
 *     (NULL = the device's default stream, exactly as in HIP; work is ordered on that stream).
 *   - every function returns 0 on success, <0 on error (kmpc_last_error() has the text).
 *   - the caller owns every buffer; the library keeps no pointer after a call returns
 *     (for the async device entry point: after the stream work completes).
 *   - one handle = one device + one stream; calls on a handle are not re-entrant.
 *   - units as in the reference: x,y [m], psi [rad], v [m/s], acc [m/s^2], d_f [rad, tyre angle].
 *   - input pairs are ordered (acc, d_f) = (MPC_cmd.accel_cmd, MPC_cmd.steer_angle_cmd)
 *     (msg/MPC_cmd.msg:2-3).  NOTE the reference's update_current_input() takes them
 *     steer-first (MKZMPCPathFollower.jl:151); the Python mirror keeps that quirk, the C ABI
 *     does not.
 */
#ifndef KMPC_H
#define KMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMPC_ABI_VERSION 8

/* per-problem status, replaces the Symbol returned by solve_model() (MKZMPCPathFollower.jl:176,182) */
enum {
    KMPC_OPTIMAL = 0,          /* :Optimal                                   */
    KMPC_ITERATION_LIMIT = 1,  /* :UserLimit (Ipopt max_cpu_time cap, :29)   */
    KMPC_INFEASIBLE = 2,       /* :Infeasible (e.g. v0 outside [v_min,v_max], Q5) */
    KMPC_NUMERICAL_ERROR = 3   /* :Error                                     */
};

enum { KMPC_F64 = 0, KMPC_F32 = 1 };

/* error codes */
enum {
    KMPC_OK = 0,
    KMPC_ERR_ARG = -1,      /* bad argument / unsupported configuration */
    KMPC_ERR_HIP = -2,      /* a HIP runtime call failed */
    KMPC_ERR_NODEVICE = -3  /* no gfx950 device / code object not loadable */
};

/* Replaces the module-level constants of MKZMPCPathFollower.jl:28-48 and the Ipopt options of :29. */
typedef struct kmpc_config {
    int32_t N;          /* horizon (:34, default 8); supported 2..56.  Compile-time-horizon kernels: one wave per problem for N = 8, 12,
                           16, 20, 24, 28 (N = 8, the reference's own horizon, also FOUR problems per wave: one per 16-lane row); one
                           four-wave workgroup per problem for N = 32, 36, 40, 44, 48, 50; any other horizon runs the generic kernel
                           (runtime N, matrices in LDS) */
    int32_t dtype;      /* KMPC_F64 / KMPC_F32: arithmetic AND device-buffer element type */
    double dt;          /* :33  0.20 */
    double dt_control;  /* :28  0.10 */
    double L_a, L_b;    /* :31-32 */
    double steer_max, steer_dmax;  /* :41-42 */
    double a_max, a_dmax;          /* :44-45 */
    double v_min, v_max;           /* :47-48 */
    /* solver options (Ipopt defaults where an equivalent exists) */
    int32_t max_iter;    /* cap on linearise+factor iterations (deterministic stand-in for max_cpu_time) */
    int32_t hessian;     /* 0 Gauss-Newton, 1 exact condensed Hessian with GN fallback */
    double tol;          /* Ipopt tol (scaled optimality error), 1e-8 */
    double mu_init;      /* barrier parameter of a cold start (default 1.0; Ipopt's is 0.1) */
    double bound_relax;  /* Ipopt bound_relax_factor, 1e-8 */
    double warm_push;    /* weight of the interior point blended into a warm start (default 1e-5) */
    double warm_mu;      /* mu_init used with a warm start (default 1e-6) */
    int32_t max_ls;      /* back-tracking trial points per iteration */
    int32_t kernel_variant; /* 0 = auto: the compile-time-horizon kernel built for N (see N; at N = 8 batches of 1024 problems or more run the
                               four-problems-per-wave kernel), else the generic one; 1 = always the generic kernel; 2 = as 0 but never the
                               four-per-wave kernel (one wave / one workgroup per problem at every batch size); 3 = the Frenet model's
                               four-problems-per-wave kernel at every batch size: accepted only with model = 1 and N = 8 (both dtypes),
                               KMPC_ERR_ARG otherwise.  Opt-in: with model = 1, N = 8 the values 0 and 2 keep the one-wave kernel.  Measured
                               in fp64: 1.97 x the one-wave kernel at B = 262 144, 1.17 x at 4096, 0.62 x at 1024 */
    int32_t mu_strategy;    /* barrier update: 0 = Ipopt's default monotone (Fiacco-McCormick), 1 = Mehrotra predictor-corrector
                               (Ipopt's adaptive family; default) */
    int32_t indef_strategy; /* exact Hessian not positive definite: 0 = Gauss-Newton fallback (held for 2 iterations), 1 = Ipopt-style
                               delta_w shift of the exact Hessian, 2 = hybrid (0 until a failure of the exact factorisation -- the first one on cold starts with N <= 28, the second one on
                               longer horizons and on warm starts --, 1 from then on);
                               2 is the default */
    int32_t schedule;       /* order in which the problems of a batch start on the GPU: 0 = index order, 1 (default) = longest
                               predicted first (key = |v0 - reference speed| + 0.3 * net heading change of the reference), which
                               shortens the tail of a launch whose time is set by its slowest problems.  Results do not depend on it.
                               Calls on one handle must be stream-ordered (the permutation workspace belongs to the handle). */
    int32_t model;          /* 0 (default) = MKZMPCPathFollower.jl, Cartesian states (x, y, psi, v); 1 = MKZMPCPathFollowerFrenet.jl,
                               Frenet-frame states (s, e_y, e_psi, v) with a cubic curvature polynomial (kmpc_solve_batch_frenet;
                               horizons N <= 24, N = 28 with kernel_variant 0 or 2: the compile-time-horizon kernels carry the functor
                               for N = 8, 12, ..., 28; and N = 32, 36, 40, 44, 48, 50 with kernel_variant 0 or 2 in fp64 only: the
                               four-wave kernel; N = 8 also with kernel_variant 3: four problems per wave, kmpc_quad.hip).  kmpc_create picks
                               the cost defaults of the chosen module. */
    int32_t start;          /* cold-start point of the inputs (a warm start overrides it): 0 (default) = feed-forward guess inside the bounds
                               (accelerations approach the reference speed, steering the curvature feed-forward); 1 = the reference's own
                               start, every primal 0 (MKZMPCPathFollower.jl:65-72, Q9), moved strictly inside the first-step rate interval
                               around u_prev and the speed rows where 0 is not.  The program is non-convex: the two may end in different
                               local minima on a few problems per thousand (tests/test_certify.py counts them). */
} kmpc_config;

typedef struct kmpc_handle kmpc_handle;

int32_t kmpc_abi_version(void);

/* fills the defaults of MKZMPCPathFollower.jl:28-48 for horizon N and element type dtype */
int32_t kmpc_config_default(kmpc_config *cfg, int32_t N, int32_t dtype);

/* Replaces the module load (`import MKZMPCPathFollower`, mpc_cmd_pub.jl:45-47; model build :29-123).
 * device = HIP device ordinal.  Cost weights start at the module defaults (:51-59). */
int32_t kmpc_create(const kmpc_config *cfg, int32_t device, kmpc_handle **out);
int32_t kmpc_destroy(kmpc_handle *h);

/* Replaces update_cost(cx,cy,cp,cv,cda,cdd,ca,cd) (:158-169), same argument order:
 * C_x, C_y, C_psi, C_v, C_dacc, C_ddf, C_acc, C_df. */
int32_t kmpc_set_cost(kmpc_handle *h, const double w[8]);
int32_t kmpc_get_cost(kmpc_handle *h, double w[8]);

/* The hot path.  Replaces, for B independent problems at once,
 *   update_init_cond (:132-138)     -> z0       [B,4]       x0,y0,psi0,v0
 *   update_reference (:142-147)     -> ref      [B,N+1,3]   x_r,y_r,psi_r per stage (mpc_path layout
 *                                                           xs/ys/psis interleaved; stage 0 unused, Q3)
 *                                      v_target [B]
 *   update_current_input (:151-154) -> u_prev   [B,2]       acc_current, d_f_current
 *   solve_model (:173-183)          -> out_u0   [B,2]       acc_opt[1], d_f_opt[1]
 *                                      out_status [B] int32
 *   get_solver_results (:188-207)   -> out_U    [B,N,2]     acc_opt, d_f_opt       (optional, NULL to skip)
 *                                      out_X    [B,N+1,4]   x,y,psi,v predictions  (optional)
 * plus out_cost [B] (objective :97-103 at the returned inputs), out_viol [B] (max violation of
 * the bounds :65-86, <= bound_relax when feasible), out_iters [B] int32 (optional).
 * warm_U [B,N,2] (optional): if warm != 0 it is read as the starting inputs (JuMP re-solves from the
 * previous primal values, Q9); it is always overwritten with the solution when non-NULL.
 * All pointers are DEVICE pointers of the handle's dtype (status/iters int32); the call is
 * asynchronous on `stream`.  Outputs are always written and always finite and within the input
 * bounds, so a caller that ignores status -- as mpc_cmd_pub.jl:121-132 does -- still gets a command. */
int32_t kmpc_solve_batch(kmpc_handle *h, int32_t B, const void *z0, const void *ref,
                         const void *v_target, const void *u_prev, void *warm_U, int32_t warm,
                         void *out_u0, int32_t *out_status, void *out_cost, void *out_viol,
                         int32_t *out_iters, void *out_U, void *out_X, void *stream);

/* The hot path of the Frenet-frame variant (handle created with cfg.model = 1).  Replaces, for B problems,
 *   update_init_cond(s, ey, epsi, vel)      (MKZMPCPathFollowerFrenet.jl:132-138) -> z0      [B,4]  s0, ey0, epsi0, v0
 *   update_reference(path, k_coeffs, v_des) (:142-147)                            -> k_poly  [B,4]  K(s) coefficients, highest
 *                                                                                    degree first (:38-39); v_target [B]
 *   update_current_input / solve_model / get_solver_results as in kmpc_solve_batch; out_X [B,N+1,4] = s, ey, epsi, v.
 * Cost weights: kmpc_set_cost with (0, C_ey, C_epsi, C_ev, C_dacc, C_ddf, C_acc, C_df) -- update_cost (:158-169) has no x slot. */
int32_t kmpc_solve_batch_frenet(kmpc_handle *h, int32_t B, const void *z0, const void *k_poly, const void *v_target,
                                const void *u_prev, void *warm_U, int32_t warm, void *out_u0, int32_t *out_status,
                                void *out_cost, void *out_viol, int32_t *out_iters, void *out_U, void *out_X, void *stream);

/* ---- per-problem cost weights and limits ----------------------------------------------------------------------------------------------
 * Replaces, PER PROBLEM of a batch, update_cost(...) (MKZMPCPathFollower.jl:158-169) and the model constants steer_max, steer_dmax, a_max,
 * a_dmax, v_min, v_max (:41-48), which kmpc_set_cost / kmpc_config set once for a whole handle: weight sweeps, fleets with different speed or
 * actuator limits and per-vehicle gain scheduling in ONE launch.  params [B,16], DEVICE, scalars of the handle's dtype (128 B per problem in
 * fp64, 64 B in fp32: whole lines), record of problem b:
 *   [0..7]   C_x, C_y, C_psi, C_v, C_dacc, C_ddf, C_acc, C_df   (update_cost order; Frenet handles: slot 0 is the unused x slot, as in
 *                                                                kmpc_set_cost -- checked for validity, otherwise ignored)
 *   [8] steer_max  [9] steer_dmax  [10] a_max  [11] a_dmax  [12] v_min  [13] v_max        [14], [15] reserved, must be 0
 * Everything else (dt, dt_control, L_a, L_b, tolerances, strategies, the horizon) stays with the handle.  A record is valid under the checks
 * kmpc_create and kmpc_set_cost apply to the same fields: all finite, weights >= 0, a_max, a_dmax, steer_dmax > 0, 0 < steer_max < 1.5,
 * v_max > v_min, reserved slots 0.  A problem with an invalid record ends with status KMPC_NUMERICAL_ERROR, iters 0, u0 = (0, 0), cost = viol = 0,
 * out_U / out_X rows 0 (its warm_U row is left as it was) and does not disturb any other problem of the batch; a valid record under which the
 * problem is infeasible (v0 outside [v_min, v_max], say) reports KMPC_INFEASIBLE exactly as the handle's limits would.
 * NOT checked, here as in kmpc_create: 0.6 a_max < a_dmax, which the proof that the feed-forward start point is strictly feasible needs
 * (first finding); a record that breaks it may cost iterations or end Infeasible.
 * Same dispatch as the plain calls (kernel_variant, batch-size thresholds, start-order pre-pass, whose key reads neither weights nor limits),
 * every back-end (kernel_variant = 3 included), through kernel instantiations of their own: the plain entry points run the code they ran
 * before.  A record holding the handle's own values gives the plain call's results bit for bit.  params == NULL IS the plain call.
 * Out of scope: the packed-record and host-pointer entry points take no per-problem parameters. */
/* the handle's current weights and limits in record order (HOST, doubles): the record of a problem that changes nothing */
int32_t kmpc_get_problem_params(kmpc_handle *h, double rec[16]);
int32_t kmpc_solve_batch_params(kmpc_handle *h, int32_t B, const void *z0, const void *ref, const void *v_target,
                                const void *u_prev, const void *params, void *warm_U, int32_t warm,
                                void *out_u0, int32_t *out_status, void *out_cost, void *out_viol,
                                int32_t *out_iters, void *out_U, void *out_X, void *stream);
int32_t kmpc_solve_batch_frenet_params(kmpc_handle *h, int32_t B, const void *z0, const void *k_poly, const void *v_target,
                                       const void *u_prev, const void *params, void *warm_U, int32_t warm,
                                       void *out_u0, int32_t *out_status, void *out_cost, void *out_viol,
                                       int32_t *out_iters, void *out_U, void *out_X, void *stream);

/* ---- packed records (ABI v8) -----------------------------------------------------------------------------------------
 * The same hot path on ONE 64-byte-aligned input record and ONE 64-byte output record per problem instead of four input and five output
 * arrays: with the start-order permutation adjacent workgroups read non-adjacent problems, and 8 ... 32-byte entries of separate arrays are
 * fetched as whole lines (counter traffic 3.3 x the algorithmic bytes at B = 262 144, fp32; 2.1 x with records); a record is a whole number of 64-byte lines.
 *   input record (scalars of the handle's dtype):  [0..3] z0 = x, y, psi, v   (update_init_cond, MKZMPCPathFollower.jl:132-138)
 *                                                  [4]    v_target           (update_reference's v_des, :142-147)
 *                                                  [5..6] u_prev = acc, d_f  (update_current_input, :151-154; accel first)
 *                                                  [7]    unused
 *                                                  [8 + 3 k + (0, 1, 2)] x_ref, y_ref, psi_ref of stage k = 0..N  (update_reference)
 *                                                  zero padding up to kmpc_record_bytes(N, dtype)
 *   output record (64 bytes):  u0 = (acc_opt[1], d_f_opt[1]) (solve_model, :179-182), cost, viol (scalars of the dtype), then status and iters (int32).
 * warm_U / out_U / out_X as in kmpc_solve_batch (optional).  Results are bit-identical to kmpc_solve_batch on the same problems. */
int64_t kmpc_record_bytes(int32_t N, int32_t dtype);   /* stride of the input records in bytes (a multiple of 64), -1 for bad arguments */
/* device kernel: the four arrays of kmpc_solve_batch -> packed input records (for callers that hold the arrays) */
int32_t kmpc_pack_records(kmpc_handle *h, int32_t B, const void *z0, const void *ref, const void *v_target, const void *u_prev,
                          void *records, void *stream);
int32_t kmpc_solve_batch_packed(kmpc_handle *h, int32_t B, const void *records, void *warm_U, int32_t warm, void *out_records,
                                void *out_U, void *out_X, void *stream);

/* Same with HOST pointers: copies in, solves, copies out, synchronises.  This is the form the
 * reference's single-problem API (B = 1) maps onto.  Batches of up to 16 problems run on a pinned, device-mapped host buffer of the
 * handle (the kernel reads its inputs from and writes its outputs to host memory: no copy launches) and the call busy-waits on a completion
 * counter in that buffer (a CPU core spins for the length of the solve, ~50 us; falls back to the stream after 2 ms); larger batches are
 * staged through device memory.  Results are bit-identical either way. */
int32_t kmpc_solve_batch_host(kmpc_handle *h, int32_t B, const void *z0, const void *ref,
                              const void *v_target, const void *u_prev, void *warm_U, int32_t warm,
                              void *out_u0, int32_t *out_status, void *out_cost, void *out_viol,
                              int32_t *out_iters, void *out_U, void *out_X);

/* text of the last error on this handle (or of the last failed kmpc_create when h == NULL) */
const char *kmpc_last_error(kmpc_handle *h);

/* ---- diagnostics used by tests/ (device pointers, handle dtype) ------------------------------ */
/* condensed Hessian H [B,2N,2N] (full symmetric, unscaled), gradient g [B,2N], cost J [B] at U [B,N,2], as the generic kernel (run-time horizon)
 * computes them.  On a model = 1 handle `ref` carries k_poly [B,4] as in kmpc_solve_batch_frenet and the kernel's own Frenet functor runs
 * (N <= 24; a larger N is refused). */
int32_t kmpc_debug_condense(kmpc_handle *h, int32_t B, const void *z0, const void *ref,
                            const void *v_target, const void *U, int32_t hessian, void *H, void *g,
                            void *J, void *stream);
/* The KKT pipeline of the kernel a solve of this handle runs at this B (kmpc_select; where that is the generic kernel, the compile-time-horizon
 * kernel of the handle's horizon instead: N = 8, 12, ..., 28 one wave per problem; N = 32, 36, ..., 48 and 50 four waves; N = 8 also four problems
 * per wave -- the Cartesian model from B >= 1024 with the default kernel_variant, the Frenet model with kernel_variant = 3).  On a model = 1 handle
 * `ref` carries k_poly [B,4] as in kmpc_solve_batch_frenet (four waves: fp64 only).  At inputs U [B,N,2], two-sided form weights w [B,5N-2] (>= 0; order: 2N input boxes,
 * 2(N-1) rate forms, N speed forms), objective scaling sc > 0 and shift reg >= 0 it assembles
 *     K = sc * H(U) + A^T diag(w) A + reg * I      (H: exact condensed Hessian if hessian = 1, Gauss-Newton if 0)
 * in registers, factors it (blocked Cholesky on the matrix cores; 16 column steps in the four-per-wave kernel) and solves once through the block
 * substitutions:
 *     K_out [B,2N,2N] full symmetric, g [B,2N] = grad J(U), x [B,2N] = K^-1 (b - sc*g), ok [B] int32 (0: K not positive definite) */
int32_t kmpc_debug_kkt(kmpc_handle *h, int32_t B, const void *z0, const void *ref, const void *v_target, const void *u_prev,
                       const void *U, const void *w, const void *b, double sc, double reg, int32_t hessian, void *K_out, void *g,
                       void *x, int32_t *ok, void *stream);
/* raw v_mfma_{f64,f32}_16x16x4 probe: a[64], b[64] lane operands -> d[64*4] lane-major results */
int32_t kmpc_debug_mfma_probe(kmpc_handle *h, const void *a, const void *b, void *d, void *stream);

/* ---- batched look-ahead waypoints: the step before the solve ------------------------------------
 * Replaces GPSRefTrajectory of scripts/gps_utils/ref_gps_traj.py: the constructor's path arrays
 * (:87-106; projection and arclength are computed by the host, see ref_traj.py) and
 * get_waypoints(X_init, Y_init, yaw_init[, v_target]) (:131-142, 172-218) for B vehicles at once. */
typedef struct kmpc_path kmpc_path;

/* HOST arrays of length M: time stamps, X, Y (m), psi (rad) and cumulative distance of the recorded path
 * (columns 0, 4, 5, 3, 6 of GPSRefTrajectory.trajectory, :106); they are copied to `device`. */
int32_t kmpc_path_create(int32_t device, int32_t M, const double *t, const double *X, const double *Y,
                         const double *psi, const double *cdist, kmpc_path **out);
int32_t kmpc_path_destroy(kmpc_path *p);

/* DEVICE pointers, fp64: pose [B,3] = (X_init, Y_init, yaw_init); v_target [B] (target-velocity mode,
 * waypoints start ONE step ahead, :175) or NULL (time mode, start at the closest point, :191);
 * ref_out [B,horizon+1,3] = (x_ref, y_ref, psi_ref) per stage -- the layout kmpc_solve_batch takes;
 * stop_out [B] int32 (stop_cmd, :182-184); closest_out [B] int32 or NULL (index of the nearest sample).
 * Asynchronous on `stream`. */
int32_t kmpc_waypoints_batch(kmpc_path *p, int32_t B, int32_t horizon, double traj_dt, const double *pose,
                             const double *v_target, double *ref_out, int32_t *stop_out, int32_t *closest_out,
                             void *stream);
const char *kmpc_path_last_error(kmpc_path *p);

/* ---- fleets on several recorded paths: a path and a tracking mode per vehicle ---------------------------------------------------------
 * The reference ships three recorded paths (the .mat files under paths/) and two tracking modes, and its launch file pairs each path with its own start pose
 * (launch/sim_path_follow.launch:13, 22-30); one GPSRefTrajectory holds one path (ref_gps_traj.py:87-106) and one node runs one mode
 * (mpc_cmd_pub.jl:99-112).  A kmpc_pathset holds P such paths in ONE device allocation, and kmpc_waypoints_fleet is get_waypoints (:131-142,
 * 172-218) for B vehicles of which each follows its own path in its own mode: one launch for a fleet that mixes routes, modes and speeds. */
typedef struct kmpc_pathset kmpc_pathset;

/* HOST: M[P] sample counts; t, X, Y, psi, cdist concatenated in path order (sum of M doubles each; the columns kmpc_path_create takes, every
 * path's cdist starting at 0, :95-100); copied to `device`.  P >= 1, every M[p] >= 2, sum of M < 2^31, else KMPC_ERR_ARG -- checked before
 * any device call, so a machine without a GPU answers KMPC_ERR_ARG to bad arguments and KMPC_ERR_NODEVICE to good ones. */
int32_t kmpc_pathset_create(int32_t device, int32_t P, const int32_t *M, const double *t, const double *X, const double *Y,
                            const double *psi, const double *cdist, kmpc_pathset **out);
int32_t kmpc_pathset_destroy(kmpc_pathset *ps);

/* DEVICE pointers: pose [B,3] fp64 = (X_init, Y_init, yaw_init); path_id [B] int32; time_mode [B] uint8 or NULL; v_target [B] fp64 or NULL;
 * ref_out [B,horizon+1,3], stop_out [B] int32 as kmpc_waypoints_batch; closest_out [B] int32 or NULL (index of the nearest sample within the
 * vehicle's OWN path, -1 if refused).
 * Modes: time_mode == NULL mirrors kmpc_waypoints_batch -- every vehicle in target-velocity mode (waypoints start ONE step ahead, :175) if
 * v_target != NULL, every vehicle in time mode (start at the closest point, :191) if v_target == NULL.  time_mode != NULL needs v_target
 * (KMPC_ERR_ARG otherwise); a non-zero entry puts that vehicle in time mode and its v_target[b] is then not read.
 * Vehicle b's rows are, bit for bit, those of kmpc_waypoints_batch on path path_id[b] alone in b's mode; the stop flag (:182-184) compares with
 * the last sample of b's own path, and no read leaves b's own segment.  A vehicle whose path_id is < 0 or >= P is refused: stop_out 1 (the node's
 * stop latch brakes it, mpc_cmd_pub.jl:100-103, 148-153), closest_out -1, every waypoint row its own pose (x, y, yaw; a non-finite component
 * becomes 0); it does not disturb any other vehicle.  A non-finite pose on a valid path gives closest index 0, as in kmpc_waypoints_batch.
 * Same bounds on B, horizon and traj_dt as kmpc_waypoints_batch; B = 0 succeeds without a launch.  Asynchronous on `stream`; path_id and
 * time_mode are read by the launch and not kept. */
int32_t kmpc_waypoints_fleet(kmpc_pathset *ps, int32_t B, int32_t horizon, double traj_dt, const double *pose,
                             const int32_t *path_id, const uint8_t *time_mode, const double *v_target,
                             double *ref_out, int32_t *stop_out, int32_t *closest_out, void *stream);
const char *kmpc_pathset_last_error(kmpc_pathset *ps);

/* ---- tracking errors on the recorded paths and a running score per vehicle -----------------------------------------------------------------
 * Replaces, for B vehicles at once and on the device, the numerical part of scripts/analysis/plot_path_tracking_error.py: compute_path_errors
 * (:21-34, nearest recorded sample and the distance to it) and the yaw error there through fix_heading (:36-43, :155-162); it adds the signed
 * distance to the POLYLINE through the samples and, in `score`, the figures of a closed-loop run (rms and largest errors, settle index, live
 * periods, largest command steps, the period of the stop latch) without a device -> host copy per period.
 *   state  DEVICE fp64, row b at state + b * state_stride doubles, X, Y, psi first: the plant's state [B,8] of kmpc_sim_advance_batch
 *          (state_stride 8) or a pose [B,3] (state_stride 3); state_stride >= 3
 *   settle_tol  finite, >= 0 [m]
 * Command side of the period, DEVICE, all four or all NULL (NULL: a geometry-only call, as for the initial state):
 *   status [B] int32, iters [B] int32 (kmpc_solve_batch's), cmd [B,2] fp64 (kmpc_command_batch's), stop_latch [B] uint8 (after it)
 * Outputs of the call, DEVICE, each optional (NULL to skip):
 *   err_out [B,4] fp64: e_ct   signed distance to the polyline: nearest point over the segments i -> i+1 with w = p - P_i, d = P_{i+1} - P_i,
 *                              s = clamp(w.d / max(|d|^2, 1e-18), 0, 1), e = |w - s d|; the sign is that of d x w on the winning segment (>= 0
 *                              counts as positive): positive when the vehicle is to the LEFT of the direction of travel
 *                       e_near distance to the nearest sample (error_xy, :30-32)
 *                       e_psi  psi_path[closest] - psi through fix_heading: the first of p, p + 2 pi, p - 2 pi of smallest magnitude
 *                       s_along cdist[seg] + s (cdist[seg+1] - cdist[seg])
 *   seg_out [B] int32: the winning segment, 0 .. M-2 (the lowest index among exactly equal distances)
 *   closest_out [B] int32: nearest sample, bit-identical to kmpc_waypoints_batch's closest_out
 * score [B,16] fp64 DEVICE in/out or NULL: the running record, 128 bytes per vehicle.  Over every scored state: */
enum {
    KMPC_SCORE_N = 0,             /* states scored */
    KMPC_SCORE_SUM_ECT2 = 1,      /* sum of e_ct^2 */
    KMPC_SCORE_MAX_ECT = 2,       /* max |e_ct| */
    KMPC_SCORE_SUM_EPSI2 = 3,     /* sum of e_psi^2 */
    KMPC_SCORE_MAX_EPSI = 4,      /* max |e_psi| */
    KMPC_SCORE_MAX_ENEAR = 5,     /* max e_near */
    KMPC_SCORE_SETTLE_INDEX = 6,  /* 1 + index (count of states scored before it) of the last scored state with |e_ct| >= settle_tol, 0 if none */
    KMPC_SCORE_N_REFUSED = 7,     /* refused states */
    /* over live periods only: command side given and stop_latch[b] == 0 */
    KMPC_SCORE_N_LIVE = 8,        /* live periods */
    KMPC_SCORE_N_NONOPT = 9,      /* ... with status != KMPC_OPTIMAL */
    KMPC_SCORE_SUM_ITERS = 10,    /* sum of iters */
    KMPC_SCORE_MAX_DACC = 11,     /* max |acc - last live acc|; the first live command is compared with (0, 0) */
    KMPC_SCORE_MAX_DDF = 12,      /* max |d_f - last live d_f| */
    KMPC_SCORE_LAST_ACC = 13,     /* the last live command: the record is self-contained */
    KMPC_SCORE_LAST_DF = 14,
    KMPC_SCORE_LATCH_INDEX = 15,  /* live periods scored before the first period with stop_latch[b] != 0: the index of that period (when no
                                     state of the vehicle was refused before it); -1 until then */
    KMPC_SCORE_WORDS = 16
};
/* s_along of the last scored state is not a word of the record: it is the last call's err_out[b][3].
 * A fresh record is all zeros except KMPC_SCORE_LATCH_INDEX = -1: kmpc_track_score_init writes B of them to HOST memory (copy them to the device),
 * or write the constant yourself; no kernel is needed.
 * Refused states: a path_id outside [0, P), a non-finite X, Y or psi, and (never with finite paths and kmpc_command_batch's commands) a
 * non-finite error or live command.  err_out row 0, seg_out = closest_out = -1, only KMPC_SCORE_N_REFUSED moves; no sample and no table entry is
 * read for a bad path_id; no other vehicle's outputs change.  Every word written is finite.
 * Argument checks come before any use of the handle and any device call: a NULL path / set, B < 0, state_stride < 3, settle_tol not finite or
 * < 0, a command side only partly given, and with B > 0 a NULL state (or path_id) return KMPC_ERR_ARG, text in kmpc_last_error(NULL), also on a
 * machine without a GPU.  B = 0 succeeds without a launch.  Asynchronous on `stream`. */
int32_t kmpc_track_score_init(double *score_host, int32_t B);
int32_t kmpc_track_score_batch(kmpc_path *p, int32_t B, const double *state, int32_t state_stride, double settle_tol,
                               const int32_t *status, const int32_t *iters, const double *cmd, const uint8_t *stop_latch,
                               double *err_out, int32_t *seg_out, int32_t *closest_out, double *score, void *stream);
/* the same for a fleet: vehicle b on path path_id[b] [B] int32 DEVICE of the set; its rows are, bit for bit, kmpc_track_score_batch's on that path alone */
int32_t kmpc_track_score_fleet(kmpc_pathset *ps, int32_t B, const double *state, int32_t state_stride, const int32_t *path_id,
                               double settle_tol, const int32_t *status, const int32_t *iters, const double *cmd,
                               const uint8_t *stop_latch, double *err_out, int32_t *seg_out, int32_t *closest_out, double *score,
                               void *stream);

/* ---- curvature- and grip-limited target speeds: a speed plan per vehicle --------------------------------------------------------------------
 * The reference node drives every corner at one constant target_vel (scripts/mpc_cmd_pub.jl:58-62) and has no such stage; the defaults below are
 * therefore this project's own.  Two calls: the curvature table of a set of paths, once per set and window, and the plan, once per period --
 * "how fast may vehicle b be at its nearest sample i so that it can still brake, at A_BRAKE, to what every sample ahead allows":
 * v^2 <= v_lim,j^2 + 2 a (s_j - s_i) for every j >= i of its own path, the backward braking pass of a speed profile as a min-reduction.
 *
 * kmpc_pathset_curvature: kappa_out [sum M] fp64 DEVICE, caller-owned, in the set's sample order (path p's samples at off_p .. off_p + M_p - 1).
 * For sample i of its path, with indices inside THAT path only, s = cdist, psi the recorded heading and h = 0.5 * window:
 *     ia = the smallest index with s[ia] >= s[i] - h        ib = the largest index with s[ib] <= s[i] + h        (binary searches; ia <= i <= ib)
 *     den = s[ib] - s[ia]
 *     kappa[i] = den > 0 ? fix_heading(psi[ib] - psi[ia]) / den : 0
 * fix_heading as in the track score: the first of p, p + 2 pi, p - 2 pi of smallest magnitude.  Every operation is rounded once (no contraction);
 * the table is bit-identical to the same expressions in numpy.  The heading difference, not a circle through three recorded positions: GPS jitter
 * and near-stationary samples make the latter useless on recorded paths.  No read leaves the sample's own path.  cdist must be non-decreasing
 * within a path (kmpc_pathset_create's own cumulative distance is).  window finite and > 0.
 *
 * kmpc_speed_plan_fleet, DEVICE pointers:
 *   kappa   [sum M] fp64: the table above (or the caller's own, in the same order; finite)
 *   state   fp64, row b at state + b * state_stride doubles, X and Y first; state_stride >= 2: the plant's [B,8], an estimate [B,4], a pose [B,3]
 *   path_id [B] int32, v_cap [B] fp64 (the speed the vehicle would drive without a plan: finite, >= 0)
 *   rows    [B,8] fp64, 64 bytes per vehicle, row of vehicle b: */
enum {
    KMPC_PLAN_A_LAT = 0,       /* lateral acceleration the plan allows in a corner [m/s^2]: > 0; +inf = no cornering limit */
    KMPC_PLAN_A_BRAKE = 1,     /* deceleration the plan counts on ahead of a limit [m/s^2]: > 0 and finite */
    KMPC_PLAN_V_FLOOR = 2,     /* the plan never asks for less than min(v_cap, V_FLOOR) [m/s]: >= 0 and finite */
    KMPC_PLAN_END_STOP = 3,    /* non-zero: the path's last sample has limit 0 (brake to a stop at the end); 0: it has its cornering limit */
                               /* words 4 ... 7 are read by nobody */
    KMPC_PLAN_WORDS = 8
};
/* The default row is (2.0, 0.7, 1.0, 0, 0, 0, 0, 0): kmpc_speed_plan_default writes B of them to HOST memory.
 * Arithmetic, per vehicle, i = the nearest sample with kmpc_waypoints_fleet's argmin (the same device function), M its path's sample count:
 *     vcap2 = v_cap * v_cap
 *     lim_j = min(vcap2, A_LAT / max(|kappa_j|, 1e-9));   if END_STOP != 0 and j == M - 1: lim_j = 0
 *     c_j   = lim_j + (2 * A_BRAKE) * (s_j - s_i)          the product, then the sum, each rounded once
 *     w     = min over j = i ... M - 1 of c_j,   jb = the lowest j that attains it
 *     v_plan = (w == vcap2) ? v_cap : min(v_cap, max(V_FLOOR, sqrt(w)))
 * The select on w == vcap2 makes an unlimited vehicle's output v_cap itself, bit for bit.  The kernel stops at the first 64-sample chunk whose
 * first sample has (2 * A_BRAKE) * (s_j - s_i), in the same arithmetic, >= the minimum so far: s is non-decreasing and every limit is >= 0, so
 * no later term can be smaller -- the result is that of the full pass.
 * Outputs: v_plan_out [B] fp64; info_out [B,4] fp64 or NULL = (w, s_jb - s_i, kappa_jb, sqrt(lim_i)); closest_out [B] int32 or NULL = i, for a
 * finite pose bit-identical to kmpc_waypoints_fleet's closest_out.
 * Refused vehicles: a path_id outside [0, P); a non-finite X or Y; v_cap non-finite or < 0; a row word out of the range above or NaN; a
 * non-finite w or info word (v_cap^2 overflowing with no cornering limit; a NaN table entry or sample among those the pass visits).  v_plan_out 0,
 * info_out row 0, closest_out -1; no sample and no table entry is read for a bad path_id; no other vehicle's outputs change.  Every word written
 * is finite.
 * Argument checks come before any use of the handle and any device call: a NULL set, a window not finite or <= 0, a NULL kappa_out; B < 0,
 * state_stride < 2, and with B > 0 a NULL kappa, state, path_id, v_cap, rows or v_plan_out return KMPC_ERR_ARG, text in kmpc_last_error(NULL),
 * also on a machine without a GPU.  B = 0 succeeds without a launch.  Asynchronous on `stream`; nothing is kept of the arguments. */
int32_t kmpc_pathset_curvature(kmpc_pathset *ps, double window, double *kappa_out, void *stream);
int32_t kmpc_speed_plan_default(double *rows_host, int32_t B);   /* HOST: B default rows; KMPC_ERR_ARG for B < 0 or, with B > 0, NULL */
int32_t kmpc_speed_plan_fleet(kmpc_pathset *ps, int32_t B, const double *kappa, const double *state, int32_t state_stride,
                              const int32_t *path_id, const double *v_cap, const double *rows,
                              double *v_plan_out, double *info_out, int32_t *closest_out, void *stream);

/* ---- road profile per path sample: grip, bank, grade, speed limits ----------------------------------------------------------------------------
 * The road row of kmpc_sim_advance_road and the plan row above describe the road as one row per vehicle for a whole run.  A road profile describes
 * it per PLACE: a table with one row per recorded sample of a path set, in the set's sample order, like the curvature table.  Two consumers read
 * it, each through its own call and each from a table of its own: the plant's table is the truth (kmpc_road_profile_fleet composes it into the road
 * row the plant reads, once per period), the plan's table is the map (kmpc_speed_plan_fleet_profile).  A map that knows nothing is the neutral table.
 *
 * profile [sum M, 8] fp64 DEVICE, caller-owned, 64 bytes per sample, row of sample g = off_p + i (sample i of path p): */
enum {
    KMPC_PROFILE_MU_SCALE = 0, /* multiplies both friction coefficients / the plan's A_LAT at this sample: > 0 and finite; 1 = neutral */
    KMPC_PROFILE_A_LONG = 1,   /* added to the road row's A_LONG at this sample [m/s^2] (grade): finite */
    KMPC_PROFILE_A_LAT = 2,    /* added to the road row's A_LAT at this sample [m/s^2] (bank): finite */
    KMPC_PROFILE_V_LIMIT = 3,  /* posted speed limit [m/s], read by the plan only: >= 0; +inf = none */
                               /* words 4 ... 7 are read by nobody */
    KMPC_PROFILE_WORDS = 8
};
/* The neutral row is (1, 0, 0, +inf, 0, 0, 0, 0): kmpc_road_profile_default writes n of them to HOST memory.  DF_OFFSET and ACC_GAIN belong to the
 * vehicle, not to the road: the profile has no word for them.
 *
 * kmpc_road_profile_fleet, DEVICE pointers: profile as above; state, state_stride and path_id as kmpc_speed_plan_fleet's; road_base [B,8] fp64, the
 * caller's road rows (KMPC_ROAD_*); road_out [B,8] fp64, the rows the plant reads; closest_out [B] int32 or NULL.
 * Per vehicle, i = the nearest sample with kmpc_waypoints_fleet's argmin (the same device function) within its own path, r = the profile's row at
 * off[path] + i, each operation rounded once:
 *     road_out[MU_F]   = road_base[MU_F] * r[MU_SCALE]        road_out[MU_R]  = road_base[MU_R] * r[MU_SCALE]        (inf stays inf)
 *     road_out[A_LONG] = road_base[A_LONG] + r[A_LONG]        road_out[A_LAT] = road_base[A_LAT] + r[A_LAT]
 *     words 4 ... 7 of road_out = words 4 ... 7 of road_base, bit for bit
 *     closest_out = i, for a finite pose bit-identical to kmpc_waypoints_fleet's closest_out
 * The profile is piecewise constant by nearest sample: no interpolation.  With the neutral table road_out equals road_base as numbers; only a -0.0
 * in A_LONG / A_LAT may come back as +0.0.
 * Refused vehicles: a path_id outside [0, P) or a non-finite X or Y.  road_out row = road_base row bit for bit (the vehicle drives on its own base
 * road), closest_out -1; no sample and no table entry is read for a bad path_id; no other vehicle's outputs change.
 * The kernel cannot validate the table: a bad table word reaches the vehicles whose nearest sample holds it, and only those.  Validate on the host.
 * road_out must not be road_base (the scaling would compound call after call): equal pointers return KMPC_ERR_ARG.
 * Argument checks come before any device call: a NULL set, B < 0, state_stride < 2, and with B > 0 a NULL profile, state, path_id, road_base or
 * road_out return KMPC_ERR_ARG, text in kmpc_last_error(NULL), also on a machine without a GPU.  B = 0 succeeds without a launch.  Asynchronous on
 * `stream`; nothing is kept of the arguments.
 *
 * kmpc_speed_plan_fleet_profile: kmpc_speed_plan_fleet with a map.  Rows, refusals, outputs, the early exit and the select on w == vcap2 are that
 * call's; only the limit of a sample differs, with profile_j the map's row of sample j of the vehicle's own path:
 *     a_j   = A_LAT * profile_j[MU_SCALE]                                                          one rounding; inf stays inf
 *     lim_j = min(vcap2, a_j / max(|kappa_j|, 1e-9), profile_j[V_LIMIT] * profile_j[V_LIMIT]);     each rounded once; END_STOP as above
 * A NaN in MU_SCALE or V_LIMIT of a sample the pass visits refuses the vehicle, as a NaN kappa entry does.  A_LONG, A_LAT and words 4 ... 7 of the
 * map are not read.  Every limit is still >= 0 for a valid table, so the early exit stays exact.  With the neutral table every output word is
 * bit-identical to kmpc_speed_plan_fleet's (A_LAT * 1 and min(., inf) are exact).  Argument checks as kmpc_speed_plan_fleet's, and with B > 0 a
 * NULL profile returns KMPC_ERR_ARG. */
int32_t kmpc_road_profile_default(double *rows_host, int32_t n);   /* HOST: n neutral rows; KMPC_ERR_ARG for n < 0 or, with n > 0, NULL */
int32_t kmpc_road_profile_fleet(kmpc_pathset *ps, int32_t B, const double *profile, const double *state, int32_t state_stride,
                                const int32_t *path_id, const double *road_base, double *road_out, int32_t *closest_out, void *stream);
int32_t kmpc_speed_plan_fleet_profile(kmpc_pathset *ps, int32_t B, const double *kappa, const double *profile, const double *state,
                                      int32_t state_stride, const int32_t *path_id, const double *v_cap, const double *rows,
                                      double *v_plan_out, double *info_out, int32_t *closest_out, void *stream);

/* ---- closed-loop simulator --------------------------------------------------------
 * Replaces, for B simulated vehicles at once, `n_updates` passes of VehicleSimulator._update_vehicle_model
 * (scripts/vehicle_simulator.py:58-107: dynamic bicycle, linear tyres, 10 Euler sub-steps of 1 ms per pass, heading
 * wrapped to [-pi, pi)) including the actuator lag of _update_low_level_control (:109-113).  n_updates = 10 is one
 * 10 Hz control period of mpc_cmd_pub.jl:87.
 *   state [B,8] fp64 DEVICE, in/out: X, Y, psi, vx, vy, wz, acc, df   (the simulator's attributes, :18-34;
 *                                    state_est publishes x=X, y=Y, psi, v=vx, a=acc, df -- :41-48)
 *   cmd   [B,2] fp64 DEVICE: accel_cmd, steer_angle_cmd of MPC_cmd (:52-55)
 * Asynchronous on `stream` (NULL = the device's default stream).  Errors: negative code, text in kmpc_last_error(NULL). */
int32_t kmpc_sim_advance_batch(int32_t device, int32_t B, void *state, const void *cmd, int32_t n_updates, void *stream);

/* ---- a plant per vehicle, with a command delay ------------------------------------------------------------------------------------------
 * kmpc_sim_advance_batch with the simulator's constants (vehicle_simulator.py:61-67, :112-113) read per vehicle: a closed-loop fleet whose
 * vehicles differ in mass, geometry, tyres and actuators, and whose commands arrive late.
 *   state [B,8], cmd [B,2]   exactly as in kmpc_sim_advance_batch
 *   plant [B,8] fp64 DEVICE, 64 bytes per vehicle, row of vehicle b: */
enum {
    KMPC_PLANT_LF = 0,         /* lf: centre of gravity -> front axle [m] (:61) */
    KMPC_PLANT_LR = 1,         /* lr: centre of gravity -> rear axle [m] (:62) */
    KMPC_PLANT_M = 2,          /* m: mass [kg] (:64) */
    KMPC_PLANT_IZ = 3,         /* Iz: yaw inertia [kg m^2] (:65) */
    KMPC_PLANT_C_ALPHA_F = 4,  /* front cornering stiffness [N/rad] (:66) */
    KMPC_PLANT_C_ALPHA_R = 5,  /* rear cornering stiffness [N/rad] (:67) */
    KMPC_PLANT_K_ACC = 6,      /* gain of the acceleration lag [1/s] (:112) */
    KMPC_PLANT_K_DF = 7,       /* gain of the steering lag [1/s] (:113) */
    KMPC_PLANT_WORDS = 8
};
/*   cmd_delay [B] int32 DEVICE or NULL (= 0 for every vehicle): the command's latency in model updates of 10 ms
 *   cmd_held  [B,2] fp64 DEVICE in/out, required with cmd_delay (optional without it): the command in force before this call
 * Vehicle b runs its first d = min(max(cmd_delay[b], 0), n_updates) updates towards cmd_held[b] and the remaining n_updates - d towards
 * cmd[b]; cmd[b] is then stored into cmd_held[b] (when cmd_held is given).  d == n_updates is a full-period latency.  Delays LONGER than one
 * call need a queue: kmpc_sim_advance_queue below (here there is one held command per vehicle).
 * Arithmetic: operation for operation kmpc_sim_advance_batch's, the literals replaced by the row's values; 1 / m and 1 / Iz are divided once per
 * call and multiplied as the source does.  A row written by kmpc_plant_default with no delay gives kmpc_sim_advance_batch's state bit for bit.
 * The reference's two quirks stay: the rear slip angle uses lf (:77) and vx has no Fyf sin(df) / m term (:84 under Python 2).
 * Row contents cannot be checked from the host: a non-finite or non-positive m or Iz (and any non-finite word) poisons that vehicle's state
 * alone -- one thread per vehicle, no lane reads another's row.  Validate rows where they are written (Python: vehicle_sim.plant_params).
 * Argument checks as kmpc_sim_advance_batch, before any device call: B < 0, n_updates < 0, and with B > 0 a NULL state, cmd or plant, or a
 * cmd_delay without cmd_held, return KMPC_ERR_ARG (text in kmpc_last_error(NULL)); B == 0 or n_updates == 0 succeeds without a launch (cmd_held
 * is then left as it was).  Asynchronous on `stream`. */
int32_t kmpc_plant_default(double *row8);   /* HOST: the reference's constants in row order (lag gains 5.0); KMPC_ERR_ARG for NULL */
int32_t kmpc_sim_advance_plant(int32_t device, int32_t B, void *state, const void *cmd, const void *plant, const int32_t *cmd_delay,
                               void *cmd_held, int32_t n_updates, void *stream);

/* ---- latency in the closed loops: definitions ---------------------------------------------------------------------------------------------
 * An UPDATE is 10 ms of plant time; a PERIOD is one call of the plant, n = n_updates updates (10 in the loops); the ABSOLUTE update of update
 * `up` of period p is tau = p n + up.  The command issued in period j under a command delay of d updates acts from absolute update j n + d
 * on, so the command IN FORCE at tau is that of period
 *     j(tau, d) = floor((tau - d) / n)          (floor towards -infinity)
 * and j < 0 means (0, 0), the simulator's command before the first period (vehicle_simulator.py:21-22).
 * A RING [D,B,2] (or [D,B,4]) is fp64 DEVICE memory in which slot j mod D -- the B rows at ring + (j mod D) * B * 2 (or 4) doubles -- holds
 * period j: one thread per vehicle reads and writes it coalesced.  Rings need no initial contents: no slot is read before it was written.
 *
 * ---- plant with a command queue: delays longer than one call ------------------------------------------------------------------------------
 * kmpc_sim_advance_plant with its one held command replaced by a ring of the last `depth` periods' commands.
 *   state, cmd, plant, cmd_delay, n_updates   exactly as in kmpc_sim_advance_plant (cmd_delay NULL = 0 for every vehicle)
 *   cmd_queue [depth,B,2] ring, in/out         period: the index of this call (>= 0); the caller counts one per call, from 0
 * Per vehicle b: cmd[b] is stored into slot period mod depth; d = min(max(cmd_delay[b], 0), (depth - 1) n), q = d / n, r = d % n (integer);
 * update `up` runs towards the command of period  period - q - (up < r ? 1 : 0)  -- that is j(period n + up, d) -- and towards (0, 0) where that
 * period is negative.  The sub-step arithmetic is kmpc_sim_advance_plant's, operation for operation: the call leaves the state that
 * kmpc_sim_advance_plant leaves when given cmd = the command of period - q, cmd_held = that of period - q - 1 and a delay of r, bit for bit; with
 * depth = 2 and every delay <= n it is kmpc_sim_advance_plant on the same arguments, call after call.
 * Argument checks as kmpc_sim_advance_plant's, before any device call, and depth < 2, period < 0 or a NULL cmd_queue return KMPC_ERR_ARG;
 * B == 0 or n_updates == 0 succeeds without a launch (the queue is then not written).  Asynchronous on `stream`. */
int32_t kmpc_sim_advance_queue(int32_t device, int32_t B, void *state, const void *cmd, const void *plant, const int32_t *cmd_delay,
                               void *cmd_queue, int32_t depth, int64_t period, int32_t n_updates, void *stream);

/* ---- grip and road: tyre limits, bank, grade, steering offset ------------------------------------------------------------------------------
 * kmpc_sim_advance_queue with a ROAD ROW per vehicle and grip bookkeeping.  The reference's tyres are linear and unbounded
 * (vehicle_simulator.py:80-81: Fy = C_alpha * alpha), its road is flat and level and its steering has no offset; a plant that cannot run out of
 * grip cannot show what a controller does when the road does not deliver the lateral force a corner asks for.
 *   state, cmd, plant, cmd_delay, cmd_queue, depth, period, n_updates   exactly as in kmpc_sim_advance_queue, with its clamping and checks
 *   road [B,8] fp64 DEVICE, 64 bytes per vehicle, row of vehicle b: */
enum {
    KMPC_ROAD_MU_F = 0,        /* friction coefficient at the front axle; +inf = no limit */
    KMPC_ROAD_MU_R = 1,        /* friction coefficient at the rear axle; +inf = no limit */
    KMPC_ROAD_A_LONG = 2,      /* specific force along the body x axis [m/s^2]: a grade theta gives -g sin(theta) */
    KMPC_ROAD_A_LAT = 3,       /* specific force along the body y axis, left positive [m/s^2]: bank, steady crosswind */
    KMPC_ROAD_DF_OFFSET = 4,   /* added to the actuator's tyre angle where the tyre model reads it [rad]: misalignment */
    KMPC_ROAD_ACC_GAIN = 5,    /* the acceleration that acts is gain x the actuator state acc */
                               /* words 6 and 7 are read by nobody */
    KMPC_ROAD_WORDS = 8
};
/*   road_stat [B,4] fp64 DEVICE in/out, or NULL: accumulated over calls (the caller zeroes it), row of vehicle b: */
enum {
    KMPC_ROAD_STAT_SAT_F = 0,  /* sub-steps in which the front force was clipped */
    KMPC_ROAD_STAT_SAT_R = 1,  /* the same for the rear */
    KMPC_ROAD_STAT_UTIL_F = 2, /* the largest front utilisation |C_alpha_f alpha_f| / lim_f so far */
    KMPC_ROAD_STAT_UTIL_R = 3, /* the same for the rear */
    KMPC_ROAD_STAT_WORDS = 4
};
/* The neutral row is (inf, inf, 0, 0, 0, 1, 0, 0): kmpc_road_default writes it.
 * Arithmetic: each sub-step is kmpc_sim_advance_queue's (that is kmpc_sim_advance_plant's), operation for operation, with these changes only
 * (g = 9.81 as a literal; no product and sum are contracted into one rounding anywhere in the plant):
 *   before the loop, once per call like 1 / m:
 *       lim_f = MU_F * (m * 9.81 * lr / (lf + lr))        lim_r = MU_R * (m * 9.81 * lf / (lf + lr))         (mu x the static axle loads)
 *   in the sub-step:
 *       dfe  = df + DF_OFFSET      replaces df in alpha_f = dfe - atan2(vy + lf wz, vx), in cos(dfe), and in the range test fabs(dfe) <= 0.6 that
 *                                  picks between the short polynomial and the library's cos
 *       acce = ACC_GAIN * acc      replaces acc in vx's derivative
 *       Fyf  = clip(C_alpha_f * alpha_f, lim_f),  Fyr = clip(C_alpha_r * alpha_r, lim_r)  with
 *       clip(x, lim) = x > lim ? lim : (x < -lim ? -lim : x)     compare-and-select: inside the limit x keeps its own bits, and a NaN passes through
 *                                                                 (fmin / fmax would swallow it)
 *   the two specific forces enter as statements of their own, after the parent's expressions have been rounded as they are today:
 *       vx0 = vx + deltaT * (acce + wz * vy);                                vx_n = fmax(0, vx0 + deltaT * A_LONG)
 *       vy0 = vy + deltaT * (1/m * (Fyf * cos(dfe) + Fyr) - wz * vx);        vy_c = vy0 + deltaT * A_LAT
 *     so a zero term adds nothing; the standstill rule (vy, wz = 0 unless vx_n > 1e-6) follows as before.  The actuator lags act on acc and df
 *     themselves, not on acce and dfe.
 *   bookkeeping: a sub-step counts as clipped at an axle when x > lim or x < -lim held there; the utilisation of a call is the largest |x| of its
 *     sub-steps divided by lim (the same number as the largest |x| / lim: division by one positive limit is monotone; an infinite limit gives 0
 *     by the division itself), and road_stat keeps  count + this call's count  and  the larger of its word and this call's utilisation (a NaN
 *     utilisation is not larger).  road_stat is read and written once per call, after the last sub-step.
 * The reference's two quirks stay: lf in the rear slip angle and no Fyf sin(df) / m term in vx.
 * Not modelled: a longitudinal grip limit and combined slip (the solver's a_max is 1 m/s^2, far inside mu g for any mu worth sweeping), load
 * transfer (the axle loads are the static ones).  The rows are plain device memory.  A limit, a bank or a grade that varies
 * along the path comes from a road profile (kmpc_road_profile_fleet, above): it composes this row once per period, on the device.  Random gusts
 * and a wandering steering offset come from the Gauss-Markov stage (kmpc_wander_batch, below), which composes A_LONG, A_LAT and DF_OFFSET.
 * Contract: with the neutral row in every vehicle the call leaves the state that kmpc_sim_advance_queue leaves on the same arguments, bit for
 * bit, and road_stat untouched (count + 0, and 0 is not larger).  A row cannot be checked from the host: a non-finite word, a mu <= 0 or a NaN
 * anywhere poisons that vehicle's state or statistics alone -- one thread per vehicle, no lane reads another's row.  Validate rows where they
 * are written (Python: vehicle_sim.road_params).
 * Argument checks as kmpc_sim_advance_queue's, before any device call, and with B > 0 a NULL road returns KMPC_ERR_ARG (text in
 * kmpc_last_error(NULL)); B == 0 or n_updates == 0 succeeds without a launch.  Asynchronous on `stream`. */
int32_t kmpc_road_default(double *row8);   /* HOST: the neutral row (inf, inf, 0, 0, 0, 1, 0, 0); KMPC_ERR_ARG for NULL */
int32_t kmpc_sim_advance_road(int32_t device, int32_t B, void *state, const void *cmd, const void *plant, const void *road,
                              const int32_t *cmd_delay, void *cmd_queue, int32_t depth, int64_t period, int32_t n_updates, void *road_stat,
                              void *stream);

/* ---- low-level controller (L0 actuation) and a pedal-driven plant ---------------------------------------------------------------------------
 * On the reference's vehicle MPC_cmd never acts as an acceleration and a tyre angle: the 50 Hz node src/LowLevelController.cpp (with PidControl.h
 * and LowPass.h; SURVEY.md section 2, component 11) turns it into a throttle fraction, a brake torque and a steering-wheel angle.  One TICK is one
 * recvSteeringReport (:205-226) followed by one controlCallback (:111-198) with sys_enable_ true, for one vehicle, in fp64, no product and sum
 * contracted, with the parameter row `llc` [B,8] fp64 DEVICE, row of vehicle b: */
enum {
    KMPC_LLC_KP = 0,              /* proportional gain of the throttle loop (:49: 0.8) */
    KMPC_LLC_KI = 1,              /* integral gain (:50: 0.4) */
    KMPC_LLC_ACCEL_MAX = 2,       /* the command is clamped to [-DECEL_MAX, ACCEL_MAX] (:71-72, :123-128: 1.0, 1.0) [m/s^2] */
    KMPC_LLC_DECEL_MAX = 3,
    KMPC_LLC_STEER_RATIO = 4,     /* steering wheel angle per tyre angle as the CONTROLLER believes it (:66: 14.8) */
    KMPC_LLC_MASS = 5,            /* the mass the brake law multiplies by (.h:116 BASE_VEHICLE_MASS = 1847.78 at fuel level 0, :118) [kg] */
    KMPC_LLC_BRAKE_DEADBAND = 6,  /* no brake unless the clamped command is below minus this (.h:114: 0.1) [m/s^2] */
    KMPC_LLC_WHEEL_RADIUS = 7,    /* the radius the brake law multiplies by (.h:115: 0.33) [m] */
    KMPC_LLC_WORDS = 8
};
/* and the record `llc_rec` [B,16] fp64 DEVICE in/out, 128 bytes per vehicle; all zeros is the reference's freshly constructed node: */
enum {
    KMPC_LLCREC_INT = 0,          /* PidControl::int_val_ */
    KMPC_LLCREC_LPF = 1,          /* lpf_accel_'s last_val_: the low-passed measured acceleration [m/s^2] */
    KMPC_LLCREC_READY = 2,        /* lpf_accel_'s ready_ (0 or 1) */
    KMPC_LLCREC_V_LAST = 3,       /* actual_.linear.x: the speed of the previous report [m/s] */
    KMPC_LLCREC_TH_CMD = 4,       /* last published throttle fraction, 0 ... 1 */
    KMPC_LLCREC_BR_CMD = 5,       /* last published brake torque [N m] */
    KMPC_LLCREC_WHEEL_CMD = 6,    /* last published steering-wheel angle [rad] */
    KMPC_LLCREC_ACC_CMD = 7,      /* the clamped acceleration command ac of the last tick (req_accel) */
    KMPC_LLCREC_TH = 8,           /* the plant's throttle actuator state (kmpc_sim_advance_drive only) */
    KMPC_LLCREC_BR = 9,           /* the plant's brake actuator state [N m] (kmpc_sim_advance_drive only) */
    KMPC_LLCREC_TICKS = 10,       /* ticks so far */
    KMPC_LLCREC_N_TH_SAT = 11,    /* ticks whose PI output exceeded 1 */
    KMPC_LLCREC_N_DEADBAND = 12,  /* ticks with -BRAKE_DEADBAND <= ac < 0: neither pedal, the car coasts */
    KMPC_LLCREC_N_BRAKE = 13,     /* ticks with ac < -BRAKE_DEADBAND */
    KMPC_LLCREC_SUM_ERR2 = 14,    /* sum over ticks of (ac - LPF)^2 */
    KMPC_LLCREC_MAX_ERR = 15,     /* largest |ac - LPF| */
    KMPC_LLCREC_WORDS = 16
};
/* A tick with the report's speed v and the command (acc_des, df_des), every line one rounding per operation, left to right:
 *   report (:207-219, LowPass.h:53-61)
 *       raw = 50.0 * (v - V_LAST)
 *       LPF = READY != 0 ? a * raw + b * LPF : raw;   READY = 1;   V_LAST = v
 *         with a = 1 / (0.5 / 0.02 + 1) and b = 0.5 / 0.02 / (0.5 / 0.02 + 1)          (LowPass::setParams(0.5, 0.02), LowPass.h:48-51, :47)
 *   clamp (:123-128)
 *       ac = acc_des > ACCEL_MAX ? ACCEL_MAX : (acc_des < -DECEL_MAX ? -DECEL_MAX : acc_des)
 *       e  = ac - LPF                                                                   (:145, :148)
 *   throttle, ac >= 0 (:147-148; PidControl::step(e, 0.02), PidControl.h:63-79, gains (KP, KI, 0), range (0, 1), :55-56)
 *       integral = INT + e * 0.02;   y = KP * e + KI * INT                              (the OLD integrator)
 *       y > 1: y = 1, N_TH_SAT += 1;   else y < 0: y = 0;   else INT = integral          (conditional integration, PidControl.h:70-76)
 *       TH_CMD = y
 *     The derivative term kd * (e - last_error) / 0.02 is dropped: kd = 0 (:55), the term is +-0 and changes no comparison and no non-zero y.
 *   throttle, ac < 0 (:149-152):   INT = 0, TH_CMD = 0;   N_DEADBAND += 1 when ac >= -BRAKE_DEADBAND
 *   brake (:156-160):              BR_CMD = ac < -BRAKE_DEADBAND ? -ac * MASS * WHEEL_RADIUS : 0   [N m];   N_BRAKE += 1 when it brakes
 *   steering wheel (:164, :175-177): w = df_des * STEER_RATIO;  fabs(w) > 8.2: w = w > 0 ? 8.2 : -8.2;   WHEEL_CMD = w
 *   bookkeeping:  ACC_CMD = ac, TICKS += 1, SUM_ERR2 += e * e, MAX_ERR = fabs(e) > MAX_ERR ? fabs(e) : MAX_ERR
 * Not modelled: the 0.2 s command timeout (:113-116; the loops publish every period), the fuel low-pass (:46, :118: MASS is the row's word),
 * pedals_enable_ / steer_enable_ (:181-188: both on), sys_enable_ false.
 * Pinned against the reference: PidControl and LowPass are header-only; their recorded outputs are tests/golden/lowlevel_classes.npz, which the
 * numpy restatement and the kernel reproduce bit for bit.  The callback that composes them needs ROS to compile and is restated by reading.
 *
 * kmpc_llc_step_batch: the node itself for B vehicles, one tick each.
 *   cmd [B,2] fp64 DEVICE: accel_cmd, steer_angle_cmd          speed: DEVICE fp64, vehicle b's at speed + b * speed_stride doubles
 *                                                              (the plant's state + 3 with a stride of 8)
 *   llc [B,8], llc_rec [B,16] as above (TH, BR are left alone)  pedals_out [B,4] or NULL: TH_CMD, BR_CMD, WHEEL_CMD, ac
 * One thread per vehicle; no lane reads another's row: a non-finite word poisons its own vehicle alone.  Argument checks before any device
 * call: B < 0, speed_stride < 1, and with B > 0 a NULL cmd, speed, llc or llc_rec return KMPC_ERR_ARG (text in kmpc_last_error(NULL)); B == 0
 * succeeds without a launch.  Asynchronous on `stream`. */
int32_t kmpc_llc_default(double *row8);   /* HOST: 0.8, 0.4, 1.0, 1.0, 14.8, 1847.78, 0.1, 0.33 (:49-72, .h:113-118); KMPC_ERR_ARG for NULL */
int32_t kmpc_llc_step_batch(int32_t device, int32_t B, const void *cmd, const void *speed, int32_t speed_stride, const void *llc, void *llc_rec,
                            void *pedals_out, void *stream);

/* kmpc_sim_advance_drive: kmpc_sim_advance_road with the controller in the loop and a powertrain that turns pedals into force.
 *   state, cmd, plant, road, cmd_delay, cmd_queue, depth, period, n_updates, road_stat   exactly as in kmpc_sim_advance_road, with its clamping
 *   llc [B,8], llc_rec [B,16] as above                 drive [B,8] fp64 DEVICE, row of vehicle b: */
enum {
    KMPC_DRIVE_F_PEAK = 0,        /* largest traction force [N] */
    KMPC_DRIVE_P_MAX = 1,         /* largest traction power [W] */
    KMPC_DRIVE_K_TH = 2,          /* gain of the throttle actuator's lag [1/s] */
    KMPC_DRIVE_K_BR = 3,          /* gain of the brake actuator's lag [1/s] */
    KMPC_DRIVE_C_ROLL = 4,        /* rolling resistance [m/s^2] */
    KMPC_DRIVE_C_DRAG = 5,        /* air resistance per unit mass [1/m]: C_DRAG vx^2 */
    KMPC_DRIVE_STEER_RATIO = 6,   /* the TRUE steering ratio (KMPC_LLC_STEER_RATIO is the controller's belief) */
    KMPC_DRIVE_WHEEL_RADIUS = 7,  /* the TRUE wheel radius [m] */
    KMPC_DRIVE_WORDS = 8
};
/* kmpc_drive_default writes 6000, 120e3, 5, 5, 0.15, 4e-4, 14.8, 0.33.  These are this project's choice: the reference has no powertrain model
 * (its simulator's first-order lag acc += 5 (acc_des - acc) dt delivers every commanded acceleration exactly).  With them the linearised PI loop
 * has a phase margin of about 70 degrees (crossover near 3.7 rad/s against lags of 0.2 s and 0.5 s).
 * Per absolute update tau = period * n_updates + up (the caller counts periods from 0 and keeps n_updates, as for the queue):
 *   tau even (50 Hz against the 100 Hz updates): one tick, before the update's sub-steps, on v = the state's vx as it is then and the command in
 *       force for that update -- the queue's selection, so cmd_delay is the MPC -> L0 transport delay.  It sets the targets held until the next
 *       tick, TH_CMD, BR_CMD and df_eff = WHEEL_CMD / drive.STEER_RATIO (a call that begins on an odd tau takes df_eff from the record).
 *   once per update:  Fmax = min(F_PEAK, P_MAX / max(vx, 1.0)), by compare-and-select (vx > 1 ? vx : 1;  q < F_PEAK ? q : F_PEAK)
 *   each 1 ms sub-step: kmpc_sim_advance_road's sub-step, unchanged, towards the tyre angle df_eff, with the state's word 6 as the acceleration
 *       that acts (ACC_GAIN, A_LONG and the floor vx >= 0 act on it as there); then, with vx_n the new speed and deltaT = 0.001,
 *           TH = K_TH * (TH_CMD - TH) * deltaT + TH          BR = K_BR * (BR_CMD - BR) * deltaT + BR
 *           acc_n = 1/m * (TH * Fmax - BR * 1/r) - (vx_n > 1e-6 ? C_ROLL + C_DRAG * vx_n * vx_n : 0)          (the NEW TH, BR)
 *       replaces the acceleration lag; 1/m is the PLANT's (KMPC_PLANT_M), 1/r = 1 / drive.WHEEL_RADIUS divided once per call; KMPC_PLANT_K_ACC is
 *       not read.  State word 6 is thus the powertrain's net longitudinal acceleration: what state_est.a and estimator_input="actuator" read.
 *       A braked vehicle stops at vx = 0 and stays there.
 * The record is read once before and written once after the loop; TH and BR are its words 8 and 9.  A fresh record (all zeros) differentiates its
 * first report against V_LAST = 0, as the reference does from rest: a loop that starts at speed sets V_LAST first.
 * A row cannot be checked from the host: a non-finite word or a zero radius poisons its own vehicle alone (Python: vehicle_sim.check_drive_rows,
 * check_llc_rows).  Argument checks as kmpc_sim_advance_road's, before any device call, and with B > 0 a NULL drive, llc or llc_rec returns
 * KMPC_ERR_ARG (text in kmpc_last_error(NULL)); B == 0 or n_updates == 0 succeeds without a launch.  Asynchronous on `stream`. */
int32_t kmpc_drive_default(double *row8);   /* HOST: 6000, 120e3, 5, 5, 0.15, 4e-4, 14.8, 0.33; KMPC_ERR_ARG for NULL */
int32_t kmpc_sim_advance_drive(int32_t device, int32_t B, void *state, const void *cmd, const void *plant, const void *road, const void *drive,
                               const void *llc, void *llc_rec, const int32_t *cmd_delay, void *cmd_queue, int32_t depth, int64_t period,
                               int32_t n_updates, void *road_stat, void *stream);

/* ---- measurement stage: what the controller sees of the plant ------------------------------------------------------------------------------
 * The reference's vehicle builds state_est from a GPS fix, an IMU yaw and the steering report's speed (scripts/state_publisher.py); its simulator
 * publishes the truth (vehicle_simulator.py:40-48).  kmpc_sense_batch puts additive Gaussian noise and a bias on the four channels the MPC reads.
 *   state  [B,8] fp64 DEVICE: the plant's state (X, Y, psi, vx first)
 *   sensor [B,8] fp64 DEVICE, row of vehicle b: */
enum {
    KMPC_SENSOR_SIGMA_X = 0, KMPC_SENSOR_SIGMA_Y = 1, KMPC_SENSOR_SIGMA_PSI = 2, KMPC_SENSOR_SIGMA_V = 3,   /* standard deviations [m, m, rad, m/s] */
    KMPC_SENSOR_BIAS_X = 4, KMPC_SENSOR_BIAS_Y = 5, KMPC_SENSOR_BIAS_PSI = 6, KMPC_SENSOR_BIAS_V = 7,
    KMPC_SENSOR_WORDS = 8
};
/*   est [B,4] fp64 DEVICE out: x, y, psi, v with est_c = (truth_c + bias_c) + sigma_c * n_c; a channel whose sigma is 0 skips the noise term, so
 *                              est_c = truth_c + bias_c bit for bit.  psi outside [-pi, pi) is wrapped into it as the plant wraps (:101); a psi
 *                              inside passes unchanged.  v is floored at 0.
 * The normals are a pure function of (seed, id_base + b, period): not of B, the launch geometry or the shard a vehicle runs in (a shard's
 * id_base is its first vehicle's index in the whole fleet).  To reproduce them:
 *   generator  Philox4x32-10 (Salmon et al., SC'11; Random123), key (seed & 0xffffffff, seed >> 32),
 *              counter (gid lo, gid hi, period lo, period hi) with gid = id_base + b  ->  words w0..w3
 *   uniforms   u_i = (w_i + 0.5) * 2^-32  (exact in fp64, never 0 or 1)
 *   normals    n0 = sqrt(-2 ln u0) cos(t), n1 = sqrt(-2 ln u0) sin(t), t = 6.283185307179586 * u1  ->  x, y;   n2, n3 from (u2, u3)  ->  psi, v
 * log / sqrt / cos / sin are the device library's (a few ulp from another libm's).  A non-finite state or row word gives a non-finite (or, for v,
 * 0) estimate of that vehicle alone.
 * Argument checks before any device call: B, period or id_base < 0, and with B > 0 a NULL state, sensor or est, return KMPC_ERR_ARG (text in
 * kmpc_last_error(NULL)); B == 0 succeeds without a launch.  Asynchronous on `stream`. */
int32_t kmpc_sense_batch(int32_t device, int32_t B, const void *state, const void *sensor, uint64_t seed, int64_t period, int64_t id_base,
                         void *est, void *stream);

/* ---- stale fixes: kmpc_sense_batch on the truth of an earlier period ------------------------------------------------------------------------
 *   state, sensor, seed, period, id_base, est   exactly as in kmpc_sense_batch
 *   meas_delay [B] int32 DEVICE: the age of the fix in WHOLE control periods      truth_ring [depth,B,4] ring, in/out (depth >= 1)
 * Per vehicle b: this period's truth x, y, psi, vx (state words 0..3) is stored into slot period mod depth; L = min(max(meas_delay[b], 0),
 * min(depth - 1, period)); the truth of period period - L is measured: est_c = (truth_c + bias_c) + sigma_c * n_c with THIS period's bias and
 * normals -- the Philox counter stays (id_base + b, period): noise belongs to the moment of emission -- then kmpc_sense_batch's wrap and floor.
 * Before the ring is filled (period < meas_delay) a vehicle sees period 0's state.  L = 0 is kmpc_sense_batch bit for bit.  The caller passes
 * consecutive periods from 0 (a gap leaves slots of other periods in the ring).  Latency INSIDE a period (a fix some updates old) is out of
 * scope: the plant's state exists between calls only.
 * Argument checks as kmpc_sense_batch's, and depth < 1 or, with B > 0, a NULL meas_delay or truth_ring return KMPC_ERR_ARG.  Asynchronous. */
int32_t kmpc_sense_delayed_batch(int32_t device, int32_t B, const void *state, const void *sensor, uint64_t seed, int64_t period,
                                 int64_t id_base, const int32_t *meas_delay, void *truth_ring, int32_t depth, void *est, void *stream);

/* ---- sensor faults: outages, outliers, held fixes ------------------------------------------------------------------------------------------
 * scripts/state_publisher.py keeps the last GPS fix, IMU yaw and steering-report speed and republishes them at 100 Hz whether they are fresh or
 * not (its time_valid check is commented out).  kmpc_sense_faults_batch is kmpc_sense_batch (kmpc_sense_delayed_batch with a ring) with three
 * sources that can fall silent -- GPS -> x, y; IMU -> psi; SPD, the steering report -> v -- and GPS outliers.  One thread per vehicle, fp64.
 *   state, sensor, seed, period, id_base   exactly as in kmpc_sense_batch
 *   meas_delay, truth_ring, depth          both NULL (depth is then ignored), or exactly as in kmpc_sense_delayed_batch
 *   faults [B,16] fp64 DEVICE, row of vehicle b: */
enum {
    KMPC_FAULT_P_LOSE_GPS = 0, KMPC_FAULT_P_LOSE_IMU = 1, KMPC_FAULT_P_LOSE_SPD = 2,         /* probability per period that a delivering source falls silent */
    KMPC_FAULT_P_REGAIN_GPS = 3, KMPC_FAULT_P_REGAIN_IMU = 4, KMPC_FAULT_P_REGAIN_SPD = 5,   /* probability per period that a silent source delivers again */
    KMPC_FAULT_WIN_FROM_GPS = 6, KMPC_FAULT_WIN_FROM_IMU = 7, KMPC_FAULT_WIN_FROM_SPD = 8,   /* first period of a scheduled silence */
    KMPC_FAULT_WIN_LEN_GPS = 9, KMPC_FAULT_WIN_LEN_IMU = 10, KMPC_FAULT_WIN_LEN_SPD = 11,    /* its length in periods; 0 = none */
    KMPC_FAULT_P_OUTLIER = 12,       /* probability that a delivered GPS fix is an outlier */
    KMPC_FAULT_OUTLIER_SIGMA = 13,   /* standard deviation [m] of an outlier fix on x and y, in place of SIGMA_X, SIGMA_Y */
    KMPC_FAULT_MAX_AGE = 14,         /* periods a source may be silent before the vehicle counts as blind; +inf = never */
                                     /* word 15 is read by nobody */
    KMPC_FAULT_WORDS = 16
};
/*   kmpc_sense_faults_default writes B neutral rows (0,0,0, 1,1,1, 0,0,0, 0,0,0, 0, 0, +inf, 0) to HOST memory.
 *   fault_rec [B,16] fp64 DEVICE in/out, record of vehicle b; all zeros (hipMemset) = fresh; counters are fp64 words as in the score record: */
enum {
    KMPC_FAULTREC_HELD_X = 0, KMPC_FAULTREC_HELD_Y = 1, KMPC_FAULTREC_HELD_PSI = 2, KMPC_FAULTREC_HELD_V = 3,   /* the last delivered value of each channel */
    KMPC_FAULTREC_COUNT = 4,         /* calls so far; 0 = fresh */
    KMPC_FAULTREC_CHAIN = 5,         /* 0 ... 7: bit s = source s silent by the random chain (s = 0 GPS, 1 IMU, 2 SPD) */
    KMPC_FAULTREC_AGE_GPS = 6, KMPC_FAULTREC_AGE_IMU = 7, KMPC_FAULTREC_AGE_SPD = 8,   /* periods since the source last delivered, 0 = this period */
    KMPC_FAULTREC_N_SILENT_GPS = 9, KMPC_FAULTREC_N_SILENT_IMU = 10, KMPC_FAULTREC_N_SILENT_SPD = 11,   /* silent periods so far */
    KMPC_FAULTREC_LONGEST_GPS = 12, KMPC_FAULTREC_LONGEST_IMU = 13, KMPC_FAULTREC_LONGEST_SPD = 14,     /* the longest silence so far [periods] */
    KMPC_FAULTREC_N_OUTLIER = 15,
    KMPC_FAULTREC_WORDS = 16
};
enum {   /* flags_out bits */
    KMPC_FAULT_FLAG_SILENT_GPS = 1, KMPC_FAULT_FLAG_SILENT_IMU = 2, KMPC_FAULT_FLAG_SILENT_SPD = 4,   /* bit s: source s silent in this period */
    KMPC_FAULT_FLAG_OUTLIER = 8,     /* the delivered GPS fix is an outlier */
    KMPC_FAULT_FLAG_BLIND = 16,      /* a source has been silent for more than MAX_AGE periods */
    KMPC_FAULT_FLAG_FRESH = 32,      /* the record was fresh */
    KMPC_FAULT_FLAG_RESET = 64       /* the record was unusable and taken as fresh (FRESH is set too) */
};
/*   z_out [B,4] fp64 DEVICE out: the measured value, a quiet NaN in the channels of a silent source -- what kmpc_estimate_batch and
 *                                kmpc_observe_batch read (a non-finite channel is a dropout: the filter coasts)
 *   held_out [B,4] fp64 DEVICE out: the measured value, the record's HELD_c in the channels of a silent source -- what state_publisher.py publishes
 *   flags_out [B] int32 DEVICE out or NULL          blind_out [B] uint8 DEVICE out or NULL: 1 when any AGE_s > MAX_AGE after this call's update
 * Per vehicle b, with gid = id_base + b and p = period:
 *   DRAWS  the noise draw is kmpc_sense_batch's.  The fault draw is a second Philox4x32-10 call with the same key and the counter
 *     (gid lo, gid hi, p lo, p hi ^ 0x80000000) -- periods are below 2^63, so no measurement draw has that bit -- words w0..w3,
 *     u_i = (w_i + 0.5) * 2^-32; u0, u1, u2 drive the chains of GPS, IMU, SPD and u3 decides the outlier.
 *   RESET  a record whose COUNT is non-finite or negative, or whose CHAIN is not one of 0 ... 7, is taken as fresh (RESET | FRESH).
 *   FRESH RECORD (COUNT == 0, or reset): its other words are not read and count as zero.  Every source delivers, there is no outlier and
 *     CHAIN = 0, whatever the row says: the publisher itself waits until every source has reported once, and a fresh filter then initialises
 *     from a complete z.
 *   OTHERWISE, per source s with was_silent_s = bit s of CHAIN:
 *     chain_s = was_silent_s ? !(u_s < P_REGAIN_s) : (u_s < P_LOSE_s)
 *     sched_s = WIN_LEN_s > 0 && p >= WIN_FROM_s && p < WIN_FROM_s + WIN_LEN_s        (p converted to fp64, the sum rounded once)
 *     silent_s = chain_s || sched_s;  only chain_s is stored, so a schedule does not disturb the chain
 *     outlier = !silent_GPS && u3 < P_OUTLIER
 *     A NaN word compares false: a NaN probability or window does nothing.
 *   MEASUREMENT  m = kmpc_sense_batch's est of this period's truth -- with a ring, kmpc_sense_delayed_batch's of the truth of period - L, its
 *     ring write included -- under the vehicle's sensor row with SIGMA_X and SIGMA_Y replaced by OUTLIER_SIGMA when `outlier`.  Noise and silence
 *     belong to the moment of emission, period p.  z_out_c = silent ? NaN : m_c;  held_out_c = silent ? HELD_c : m_c  (c's source).
 *   RECORD  HELD_c = held_out_c;  AGE_s = silent_s ? AGE_s + 1 : 0;  N_SILENT_s += silent_s;  LONGEST_s = AGE_s > LONGEST_s ? AGE_s : LONGEST_s;
 *     N_OUTLIER += outlier;  COUNT += 1;  CHAIN = sum of chain_s << s.  blind = any AGE_s > MAX_AGE (a NaN MAX_AGE: never).
 *   CONTAINMENT  no lane reads another vehicle's row or record: a bad row, a poisoned record or a non-finite truth affects that vehicle alone.
 * With the neutral row z_out and held_out are kmpc_sense_batch's est (kmpc_sense_delayed_batch's with a ring) bit for bit, call after call, and
 * the flags show at most FRESH.  A vehicle's whole fault history is a function of (seed, gid, its row, the periods called): not of B, the launch
 * geometry or the shard.  Row contents cannot be checked from the host (Python: vehicle_sim.check_fault_rows).
 * Argument checks before any device call: B, period or id_base < 0; with B > 0 a NULL state, sensor, faults, fault_rec, z_out or held_out; one
 * of meas_delay and truth_ring without the other; depth < 1 with a ring: KMPC_ERR_ARG (text in kmpc_last_error(NULL)).  B == 0 succeeds without
 * a launch.  Asynchronous on `stream`. */
int32_t kmpc_sense_faults_default(double *rows_host, int32_t B);   /* HOST; KMPC_ERR_ARG for B < 0 or, with B > 0, NULL rows */
int32_t kmpc_sense_faults_batch(int32_t device, int32_t B, const void *state, const void *sensor, const void *faults, uint64_t seed,
                                int64_t period, int64_t id_base, const int32_t *meas_delay, void *truth_ring, int32_t depth, void *fault_rec,
                                void *z_out, void *held_out, int32_t *flags_out, uint8_t *blind_out, void *stream);

/* ---- coloured noise and gusts: a Gauss-Markov stage ("wander") ----------------------------------------------------------------------------
 * kmpc_sense_batch's noise is white and a road row is a constant.  kmpc_wander_batch keeps eight first-order Gauss-Markov processes per vehicle
 * -- a GPS error that wanders, a gust, a gyro's random walk -- advances them once per control period and composes them into the rows the
 * measurement and plant kernels already read: a sensor row's biases and a road row's A_LONG, A_LAT and DF_OFFSET.  Those kernels do not change.
 * One thread per vehicle, fp64.  The channels: */
enum {
    KMPC_WANDER_CH_X = 0, KMPC_WANDER_CH_Y = 1, KMPC_WANDER_CH_PSI = 2, KMPC_WANDER_CH_V = 3,   /* measurement error on x, y, psi, v [m, m, rad, m/s] */
    KMPC_WANDER_CH_A_LONG = 4,      /* added to the road row's A_LONG [m/s^2] */
    KMPC_WANDER_CH_A_LAT = 5,       /* added to the road row's A_LAT [m/s^2]: a lateral gust */
    KMPC_WANDER_CH_DF_OFFSET = 6,   /* added to the road row's DF_OFFSET [rad] */
    KMPC_WANDER_CH_FREE = 7,        /* advanced like the others, composed into nothing: the caller's */
    KMPC_WANDER_CHANNELS = 8
};
/*   wander [B,24] fp64 DEVICE, row of vehicle b: three groups of eight words, one word per channel c (word = group + c): */
enum {
    KMPC_WANDER_S0 = 0,             /* words 0 ... 7: standard deviation of the first value, >= 0 */
    KMPC_WANDER_A = 8,              /* words 8 ... 15: carry-over per period, in [0, 1] */
    KMPC_WANDER_Q = 16,             /* words 16 ... 23: standard deviation of the innovation per period, >= 0 */
    KMPC_WANDER_WORDS = 24
};
/*   kmpc_wander_default writes B neutral rows to HOST memory: all 24 words 0 (A = 0 too), every channel off.
 *   wander_rec [B,16] fp64 DEVICE in/out, record of vehicle b; all zeros (hipMemset) = fresh: */
enum {
    KMPC_WANDERREC_X = 0,           /* words 0 ... 7: X_c, the current value of channel c.  This is the stage's output: there is no separate x_out */
    KMPC_WANDERREC_COUNT = 8,       /* calls so far; 0 = fresh */
                                    /* words 9 ... 15 are written back as read, whatever the record's state */
    KMPC_WANDERREC_WORDS = 16
};
/*   seed, period, id_base        as in kmpc_sense_batch; period < 2^62
 *   sensor_base, sensor_out      both NULL, or [B,8] fp64 DEVICE sensor rows (KMPC_SENSOR_*): the caller's rows and the rows the sense kernels read
 *   road_base, road_out          both NULL, or [B,8] fp64 DEVICE road rows (KMPC_ROAD_*): the caller's rows and the rows the plant (or
 *                                kmpc_road_profile_fleet, as its road_base) reads
 * Per vehicle b, with gid = id_base + b and p = period; no product and sum are contracted, every operation is rounded once:
 *   DRAWS  two Philox4x32-10 calls with kmpc_sense_batch's key.  Call j (0 or 1) has the counter
 *     (gid lo, gid hi, p lo, p hi ^ (j == 0 ? 0x40000000 : 0xC0000000)).  With p < 2^62 the top two bits of p hi are clear, so the four domains --
 *     00 the measurement draw, 10 the fault draw, 01 and 11 these -- never share a counter.  Uniforms and Box-Muller exactly as in
 *     kmpc_sense_batch: u_i = (w_i + 0.5) * 2^-32;  n_(4j) = sqrt(-2 ln u0) cos(t), n_(4j+1) = sqrt(-2 ln u0) sin(t), t = 6.283185307179586 * u1;
 *     n_(4j+2), n_(4j+3) likewise from (u2, u3).  Call j thus gives the normals of channels 4j ... 4j+3.
 *   OFF  a channel with S0_c == 0 && Q_c == 0 is off: its X_c is written +0.0, its composed word is the base word bit for bit (no add), and it
 *     need not draw (a call none of whose four channels is on is skipped).  Every other channel is active (a NaN S0 or Q compares false: active).
 *   RESET  a record whose COUNT is non-finite or negative is taken as fresh.
 *   FRESH RECORD (COUNT == 0, or reset):  X_c = S0_c * n_c;  COUNT = 1.  The record's X words are not read.
 *   OTHERWISE  X_c = A_c * X_c + Q_c * n_c  (product, product, sum);  COUNT = COUNT + 1.
 *   COMPOSITION (each pair that is given)
 *     sensor_out words 0 ... 3 (the sigmas) = sensor_base's, bit for bit;  sensor_out[BIAS_X + c] = sensor_base[BIAS_X + c] + X_c for an active
 *     channel c = 0 ... 3, sensor_base's bits for one that is off.
 *     road_out[A_LONG] = road_base[A_LONG] + X_4, road_out[A_LAT] = road_base[A_LAT] + X_5, road_out[DF_OFFSET] = road_base[DF_OFFSET] + X_6 where
 *     the channel is active, road_base's bits where it is off;  road_out words 0, 1, 5, 6, 7 = road_base's, bit for bit.
 *     out == base is refused: the sum would compound call after call (kmpc_road_profile_fleet's rule).
 * Properties:
 *   - With the neutral row in every vehicle both outputs equal their bases bit for bit and every X is +0.0.
 *   - A vehicle's whole history is a function of (seed, gid, its row, the periods called): not of B, the launch geometry or the shard.
 *   - A = 1, Q = 0 keeps the first draw for ever: 1 * X + 0 * n is exact, except that a -0.0 becomes +0.0 in the second call.
 *   - Q = S0 * sqrt(1 - A^2) makes the process stationary with standard deviation S0 and correlation A^k at lag k: A = exp(-dt / tau) for a
 *     correlation time tau.  S0 = 0, A = 1, Q > 0 is a random walk.  A = 0 is white noise.
 *   - The kernel cannot validate a row (Python: vehicle_sim.check_wander_rows): a non-finite word poisons that vehicle's X and composed words
 *     alone.  No lane reads another vehicle's words.
 *   - The noise belongs to the moment of emission: a delayed or faulty sense reads this period's composed bias, as it reads this period's
 *     normals.  A value is held for one control period, like the road profile's.
 * Argument checks before any device call (they answer on a machine without a GPU): B, period or id_base < 0, period >= 2^62; with B > 0 a NULL
 * wander or wander_rec; one of a pair without the other; out == base: KMPC_ERR_ARG (text in kmpc_last_error(NULL)).  B == 0 succeeds without a
 * launch.  Asynchronous on `stream`. */
int32_t kmpc_wander_default(double *rows_host, int32_t B);   /* HOST: B rows of 24 zeros; KMPC_ERR_ARG for B < 0 or, with B > 0, NULL rows */
int32_t kmpc_wander_batch(int32_t device, int32_t B, const void *wander, void *wander_rec, uint64_t seed, int64_t period, int64_t id_base,
                          const void *sensor_base, void *sensor_out, const void *road_base, void *road_out, void *stream);

/* ---- delay compensation: the controller's side -------------------------------------------------------------------------------------------
 * The controller keeps a log of the commands it sent and its own ASSUMED delays -- buffers of its own, not the plant's or the sensor's, so that
 * a run can have a delay mismatch.
 *   cmd_hist [depth,B,2] ring: period p's command is written (by the caller: a [B,2] copy into slot p mod depth) AFTER the command stage of
 *                              period p, so a call in period p sees periods p - depth ... p - 1
 *   cmd_delay [B] int32 DEVICE: assumed command delay in updates       meas_delay [B] int32 DEVICE: assumed age of the measurement in periods
 *   max_cmd_delay, max_meas_delay >= 0: caps.  Per vehicle d = min(max(cmd_delay[b], 0), max_cmd_delay) and
 *                              Lm = min(max(meas_delay[b], 0), min(max_meas_delay, period))
 *   depth >= max_meas_delay + ceil(max_cmd_delay / n) + 1, else KMPC_ERR_ARG: then no slot is read that the log does not hold
 *   period >= 0, n = n_updates >= 1
 * kmpc_cmd_in_force_batch -> u_out [B,2]: the input of the estimator's predict step in period p.  The measurement belongs to update (p - Lm) n,
 *   the filter steps over the period before that update, and u_out is the command in force at that period's midpoint:
 *   tau = (p - Lm - 1) n + n / 2 (integer division), u_out = the logged command of period j(tau, d), (0, 0) for j < 0.  A pure selection: exact.
 * kmpc_predict_ahead_batch -> z_out [B,4] (may be z itself): z [B,4] is the estimate x, y, psi, v, valid at update tau0 = (p - Lm) n.  For
 *   tau = tau0 ... p n + d - 1, in this order, one Euler step of the solver's bicycle (the PREDICT state equations of kmpc_estimate_batch below,
 *   with dt = h = 0.01) under (acc, d_f) = the logged command of period j(tau, d):
 *     beta = atan(L_b / (L_a + L_b) * tan(d_f)); sb = sin(beta)      -- recomputed only when j(tau, d) differs from the step before
 *     s = sin(psi + beta), c = cos(psi + beta)                        (psi, v: before the step)
 *     x += h * (v * c);  y += h * (v * s);  psi = wrap(psi + h * (v / L_b * sb));  v = v + h * acc, 0 when that is < 0
 *   Every operation is rounded on its own (no FP contraction); wrap as in kmpc_estimate_batch; tan / atan / sin / cos are the device library's.
 *   That is Lm n + d steps: z_out is the state at the update from which THIS period's command acts.  Lm = d = 0 copies z bit for bit.  A
 *   non-finite z (or logged command) poisons that vehicle's z_out alone: one thread per vehicle.
 * Argument checks before any device call: B < 0, period < 0, n_updates < 1, a negative cap, depth too small, L_a or L_b not finite and > 0
 * (predict-ahead), and with B > 0 a NULL buffer return KMPC_ERR_ARG (text in kmpc_last_error(NULL)); B == 0 succeeds without a launch.
 * Asynchronous on `stream`. */
int32_t kmpc_cmd_in_force_batch(int32_t device, int32_t B, const void *cmd_hist, int32_t depth, int64_t period, int32_t n_updates,
                                const int32_t *cmd_delay, const int32_t *meas_delay, int32_t max_cmd_delay, int32_t max_meas_delay, void *u_out,
                                void *stream);
int32_t kmpc_predict_ahead_batch(int32_t device, int32_t B, const void *z, const void *cmd_hist, int32_t depth, int64_t period,
                                 int32_t n_updates, const int32_t *cmd_delay, const int32_t *meas_delay, int32_t max_cmd_delay,
                                 int32_t max_meas_delay, double L_a, double L_b, void *z_out, void *stream);

/* ---- state estimator: between the measurement stage and the solver ---------------------------------------------------------------------------
 * The reference hands the MPC raw measurements (scripts/state_publisher.py republishes the GPS fix, the IMU yaw and the steering report's speed).
 * kmpc_estimate_batch filters them: one call is one period of an extended Kalman filter on the SOLVER's model (MKZMPCPathFollower.jl's Euler
 * bicycle, with L_a and L_b of the solver's kmpc_config) for every vehicle, H = I, R diagonal.  One thread per vehicle, fp64, no FP contraction.
 *   rec [B,16] fp64 DEVICE in/out, 128 bytes per vehicle, record of vehicle b: */
enum {
    KMPC_EST_X = 0, KMPC_EST_Y = 1, KMPC_EST_PSI = 2, KMPC_EST_V = 3,      /* the estimate xh [m, m, rad in [-pi, pi), m/s >= 0] */
    KMPC_EST_PXX = 4, KMPC_EST_PXY = 5, KMPC_EST_PXPSI = 6, KMPC_EST_PXV = 7,   /* upper triangle of the covariance P, row-major */
    KMPC_EST_PYY = 8, KMPC_EST_PYPSI = 9, KMPC_EST_PYV = 10,
    KMPC_EST_PPSIPSI = 11, KMPC_EST_PPSIV = 12,
    KMPC_EST_PVV = 13,
    KMPC_EST_COUNT = 14,       /* calls that updated the record; 0 = fresh */
    KMPC_EST_SKIPPED = 15,     /* channel measurements skipped so far */
    KMPC_EST_WORDS = 16
};
/*   A fresh record is all zeros (hipMemset); word 14 == 0 is what makes it fresh.
 *   params [B,8] fp64 DEVICE, row of vehicle b: standard deviations, squared by the kernel (q2_c = q_c * q_c, r2_c = r_c * r_c) */
enum {
    KMPC_ESTPAR_Q_X = 0, KMPC_ESTPAR_Q_Y = 1, KMPC_ESTPAR_Q_PSI = 2, KMPC_ESTPAR_Q_V = 3,   /* process noise per call [m, m, rad, m/s] */
    KMPC_ESTPAR_R_X = 4, KMPC_ESTPAR_R_Y = 5, KMPC_ESTPAR_R_PSI = 6, KMPC_ESTPAR_R_V = 7,   /* measurement noise [m, m, rad, m/s] */
    KMPC_ESTPAR_WORDS = 8
};
enum {   /* flags_out bits */
    KMPC_EST_FLAG_SKIP_X = 1, KMPC_EST_FLAG_SKIP_Y = 2, KMPC_EST_FLAG_SKIP_PSI = 4, KMPC_EST_FLAG_SKIP_V = 8,   /* bit c: channel c skipped */
    KMPC_EST_FLAG_INIT = 16,   /* the record was initialised by this call */
    KMPC_EST_FLAG_RESET = 32   /* the record held or produced a non-finite word and was reset to fresh */
};
/*   z [B,4] fp64 DEVICE: the measurement x, y, psi, v (kmpc_sense_batch's est, or the truth); a non-finite word is a dropout of that channel
 *   u fp64 DEVICE, row b at u + b * u_stride doubles (u_stride >= 2): (acc, d_f) in force since the last call -- sim.state + 6 with stride 8 (the
 *     actuator states state_est publishes) or a [B,2] command buffer with stride 2
 *   dt, L_a, L_b, gate: fleet-wide; dt the time between calls [s] (> 0), L_a, L_b the solver model's axle distances [m] (> 0), gate >= 0 the
 *     innovation gate in standard deviations (0 = no gate)
 *   est_out [B,4] fp64 DEVICE out (may be z itself)     innov_out [B,4] fp64 DEVICE out or NULL     flags_out [B] int32 DEVICE out or NULL
 * Arithmetic, every operation rounded on its own, sums left to right, wrap(a) = a when -pi <= a < pi, else fmod(a + pi, 2 pi) (+ 2 pi when
 * negative) - pi with pi = 3.141592653589793 (the plant's and the sensor's wrap); tan / atan / sin / cos / sqrt are the device library's:
 *   FIRST CALL (word 14 == 0): no predict.  All four z finite: xh = z and P = diag(r2) bit for bit (off-diagonals 0), word 14 = 1, word 15 = 0,
 *     est_out = z, innov_out = 0, flags = INIT.  Otherwise the record is written as all zeros (it stays fresh), est_out = z, innov_out = 0 and
 *     flags carries bit c for every non-finite z_c.
 *   PREDICT  beta = atan(L_b / (L_a + L_b) * tan(d_f)); s = sin(psi + beta), c = cos(psi + beta), sb = sin(beta)   (psi, v: before the step)
 *     F = I + {F_x,psi = -(dt * (v * s)), F_x,v = dt * c, F_y,psi = dt * (v * c), F_y,v = dt * s, F_psi,v = dt * (sb / L_b)}
 *     x += dt * (v * c);  y += dt * (v * s);  psi = wrap(psi + dt * (v / L_b * sb));  v = v + dt * acc, 0 when that is < 0
 *     A = F P: A_ij = P_ij + F_i,psi * P_psi,j + F_i,v * P_v,j (the terms F has), then P_ij = A_ij + F_j,psi * A_i,psi + F_j,v * A_i,v for i <= j
 *     only, and P_cc += q2_c last.  The lower triangle is never formed: P is symmetric by construction.
 *   UPDATE, channels c = x, y, psi, v in this order, each on the result of the one before:
 *     nu = z_c - xh_c (c = psi: wrap(nu));  S = P_cc + r2_c
 *     skipped -- bit c set, word 15 += 1, innov_out_c = 0, nothing else changes -- when z_c is non-finite, when S is not a finite number > 0, or
 *     when gate > 0 and nu * nu > gate * gate * S; otherwise
 *     K_i = P_ic / S (IEEE division, P_ic before this channel);  xh_i += K_i * nu;  P_ij -= K_i * P_cj for i <= j (P_cj before this channel);
 *     innov_out_c = nu / sqrt(S)
 *     After v: psi = wrap(psi); v = 0 when v < 0; word 14 += 1.
 *   CONTAINMENT  if any word of the record is then non-finite, the record is written as all zeros (fresh: the next call initialises from its z),
 *     est_out = z, innov_out = 0 and flags = the skipped bits | RESET.  A record that arrives with a non-finite word ends here too.  One thread
 *     per vehicle, no lane reads another vehicle's words: a poisoned record, row or measurement costs that vehicle one re-initialisation.
 *   est_out = xh otherwise.
 * Row contents cannot be checked from the host; validate them where they are written (Python: vehicle_sim.Estimator: finite, q >= 0, r > 0).
 * Argument checks before any device call: B < 0, u_stride < 2, dt, L_a or L_b not finite and > 0, gate not finite and >= 0, and with B > 0 a
 * NULL rec, z, u, params or est_out return KMPC_ERR_ARG (text in kmpc_last_error(NULL)); B == 0 succeeds without a launch.  Asynchronous on
 * `stream`. */
int32_t kmpc_estimate_batch(int32_t device, int32_t B, void *rec, const void *z, const void *u, int32_t u_stride, const void *params, double dt,
                            double L_a, double L_b, double gate, void *est_out, void *innov_out, int32_t *flags_out, void *stream);

/* ---- disturbance observer and command offset: offset-free closed loops -----------------------------------------------------------------------
 * A bank, a steering offset or a grade is a CONSTANT error of the solver's model; kmpc_estimate_batch trusts that model and is dragged along.
 * kmpc_observe_batch is kmpc_estimate_batch's filter on the model augmented with three constant disturbances, seven states
 *   xh = (x, y, psi, v, dpsi, ddelta, da):  dpsi  the course offset [rad]: direction of travel - heading - beta (crab angle under bank, yaw-sensor bias)
 *                                           ddelta the steering offset [rad], added to the input d_f
 *                                           da    the acceleration offset [m/s^2], added to the input acc (grade; gain error at steady state)
 * and kmpc_cmd_offset_batch subtracts the two input disturbances from the command on its way to the plant.  No solve kernel is involved: the
 * correction enters through est_out (the state waypoints, fit and solve read) and through the command.
 *   rec [B,40] fp64 DEVICE in/out, 320 bytes per vehicle, record of vehicle b: */
enum {
    KMPC_OBS_X = 0, KMPC_OBS_Y = 1, KMPC_OBS_PSI = 2, KMPC_OBS_V = 3,   /* as KMPC_EST_X ... KMPC_EST_V */
    KMPC_OBS_DPSI = 4, KMPC_OBS_DDELTA = 5, KMPC_OBS_DA = 6,            /* the disturbance estimates */
    KMPC_OBS_P = 7,            /* words 7 ... 34: upper triangle of the 7 x 7 covariance, row-major: P_ij (i <= j) at 7 + 7 i - i (i - 1) / 2 + (j - i) */
    KMPC_OBS_COUNT = 35,       /* calls that updated the record; 0 = fresh */
    KMPC_OBS_SKIPPED = 36,     /* channel measurements skipped so far */
                               /* words 37 ... 39 are written 0 and read by nobody */
    KMPC_OBS_WORDS = 40
};
/*   A fresh record is all zeros (hipMemset); word 35 == 0 is what makes it fresh.
 *   params [B,16] fp64 DEVICE, row of vehicle b: standard deviations, squared by the kernel (q2_i = q_i * q_i, r2_c = r_c * r_c, p02 = p0 * p0) */
enum {
    KMPC_OBSPAR_Q_X = 0, KMPC_OBSPAR_Q_Y = 1, KMPC_OBSPAR_Q_PSI = 2, KMPC_OBSPAR_Q_V = 3,   /* process noise per call [m, m, rad, m/s] */
    KMPC_OBSPAR_Q_DPSI = 4, KMPC_OBSPAR_Q_DDELTA = 5, KMPC_OBSPAR_Q_DA = 6,                 /* random walk of the disturbances per call */
    KMPC_OBSPAR_R_X = 7, KMPC_OBSPAR_R_Y = 8, KMPC_OBSPAR_R_PSI = 9, KMPC_OBSPAR_R_V = 10,  /* measurement noise [m, m, rad, m/s] */
    KMPC_OBSPAR_P0_DPSI = 11, KMPC_OBSPAR_P0_DDELTA = 12, KMPC_OBSPAR_P0_DA = 13,           /* initial standard deviation of the disturbances */
                               /* words 14 and 15 are read by nobody */
    KMPC_OBSPAR_WORDS = 16
};
/*   z, u, u_stride, dt, L_a, L_b, gate, innov_out, flags_out (KMPC_EST_FLAG_* bits, same values): exactly as in kmpc_estimate_batch.  u is what
 *     the ACTUATORS got (sim.state + 6, stride 8) or the command as sent, after kmpc_cmd_offset_batch: then "input + d" is what acted.
 *   v_min >= 0 [m/s]: below it dpsi and ddelta are frozen (see PREDICT)       psi_cap >= 0 [rad]: cap on the course offset handed to the solver
 *   est_out [B,4] fp64 DEVICE out (may be z itself) = (x, y, wrap(psi + clip(dpsi, psi_cap)), v): the heading the solver's model needs to travel
 *     where the vehicle travels; psi_cap = 0 gives psi itself.  clip(a, cap) = a > cap ? cap : (a < -cap ? -cap : a), compare-and-select as the
 *     road kernel's.            dist_out [B,3] fp64 DEVICE out or NULL = dpsi, ddelta, da (0, 0, 0 when the record leaves the call fresh)
 * Arithmetic: kmpc_estimate_batch's, operation for operation, with every new term APPENDED after the terms stated there; every operation rounded
 * on its own, sums left to right, the same wrap.  Indices: 0 x, 1 y, 2 psi, 3 v, 4 dpsi, 5 ddelta, 6 da.
 *   FIRST CALL (word 35 == 0): no predict.  All four z finite: xh = (z, 0, 0, 0), P = diag(r2_x, r2_y, r2_psi, r2_v, p02_dpsi, p02_ddelta, p02_da)
 *     (off-diagonals 0), word 35 = 1, word 36 = 0, est_out = z bit for bit, dist_out = 0, innov_out = 0, flags = INIT.  Otherwise the record is
 *     written as all zeros, est_out = z, dist_out = 0, innov_out = 0 and flags carries bit c for every non-finite z_c.
 *   PREDICT  (psi, v, dpsi, ddelta, da: before the step)
 *     de = d_f + ddelta;  t = tan(de);  k = L_b / (L_a + L_b);  beta = atan(k * t);  sb = sin(beta);  cb = cos(beta)
 *     th = (psi + dpsi) + beta;  s = sin(th), c = cos(th)
 *     bp = k * (1 + t * t) / (1 + (k * t) * (k * t))                                                       (d beta / d de)
 *     F = I + {F_x,psi = -(dt * (v * s)), F_x,v = dt * c, F_y,psi = dt * (v * c), F_y,v = dt * s, F_psi,v = dt * (sb / L_b),      (the estimator's)
 *              F_x,dpsi = F_x,psi, F_y,dpsi = F_y,psi, F_x,ddelta = F_x,psi * bp, F_y,ddelta = F_y,psi * bp,
 *              F_psi,ddelta = dt * (v / L_b * (cb * bp)), F_v,da = dt}
 *     x += dt * (v * c);  y += dt * (v * s);  psi = wrap(psi + dt * (v / L_b * sb));  v = v + dt * (acc + da), 0 when that is < 0;
 *     dpsi, ddelta, da unchanged
 *     A = F P, rows x, y, psi, v (rows 4 ... 6 of F are identity: A_ij = P_ij there):
 *       A_ij = P_ij + sum over k = psi, v, dpsi, ddelta, da, in this order, of F_i,k * P_k,j, the terms F has in row i only
 *     P_ij = A_ij + sum over k = psi, v, dpsi, ddelta, da, in this order, of F_j,k * A_i,k, the terms F has in row j only, for i <= j <= 3;
 *     P_ij = A_ij for j >= 4;  then P_ii += q2_i last, i = 0 ... 6 -- except that q2_dpsi and q2_ddelta are NOT added when v (before the step) is
 *     < v_min: neither is observable at rest, and P must not grow without bound at a stop line.  The lower triangle is never formed.
 *   UPDATE, channels c = x, y, psi, v as in kmpc_estimate_batch (nu, S, the skip rules, innov_out_c), over seven states:
 *     K_i = P_ic / S;  xh_i += K_i * nu;  P_ij -= K_i * P_cj for i <= j, i, j = 0 ... 6 (P_ic, P_cj before this channel).
 *     After v: psi = wrap(psi); v = 0 when v < 0; word 35 += 1.
 *   CONTAINMENT as kmpc_estimate_batch's, over words 0 ... 36: a record that holds or produces a non-finite word is written as all zeros,
 *     est_out = z, dist_out = 0, innov_out = 0, flags = the skipped bits | RESET.  One thread per vehicle: it costs that vehicle alone.
 * Contract: with p0 = q_dpsi = q_ddelta = q_da = 0 the disturbances and their covariance words stay 0 and every appended term is a product with 0:
 *   words 0 ... 3, the ten words of the 4 x 4 block of P, est_out (any psi_cap), innov_out, flags and both counters equal kmpc_estimate_batch's
 *   on the same inputs AS NUMBERS (a -0 may become +0), call after call.
 * Argument checks before any device call: kmpc_estimate_batch's, and v_min or psi_cap not finite and >= 0 return KMPC_ERR_ARG; with B > 0 a NULL
 * rec, z, u, params or est_out returns KMPC_ERR_ARG (text in kmpc_last_error(NULL)); B == 0 succeeds without a launch.  Asynchronous on `stream`.
 * Row contents cannot be checked from the host (Python: vehicle_sim.DisturbanceObserver validates them: finite, q, q_dist, p0 >= 0, r > 0). */
int32_t kmpc_observe_batch(int32_t device, int32_t B, void *rec, const void *z, const void *u, int32_t u_stride, const void *params, double dt,
                           double L_a, double L_b, double gate, double v_min, double psi_cap, void *est_out, void *dist_out, void *innov_out,
                           int32_t *flags_out, void *stream);

/* kmpc_cmd_offset_batch: between kmpc_command_batch and the plant, in place on cmd [B,2] fp64 DEVICE (accel, steer).
 *   rec [B,40]: kmpc_observe_batch's records, read only (words 5, 6 and 35)      stop_latch [B] uint8 DEVICE or NULL (= none latched)
 *   acc_cap, df_cap >= 0: caps on the two corrections [m/s^2, rad]
 * Per vehicle: ca = clip(da, acc_cap), cd = clip(ddelta, df_cap) (compare-and-select, as above); acc = acc - ca when ca != 0, steer = steer - cd
 * when cd != 0 -- a zero correction leaves the word's bits, so caps of 0 leave cmd as it is.  Skipped, cmd[b] untouched: a latched vehicle (its
 * command is the brake override, not the solver's), a fresh record (word 35 == 0), a non-finite da or ddelta.  The solver's rate-limit anchor
 * u_prev is kmpc_command_batch's and stays the solver's own command.
 * Argument checks before any device call: B < 0, a cap not finite and >= 0, with B > 0 a NULL rec or cmd return KMPC_ERR_ARG; B == 0 succeeds
 * without a launch.  Asynchronous on `stream`. */
int32_t kmpc_cmd_offset_batch(int32_t device, int32_t B, const void *rec, const uint8_t *stop_latch, double acc_cap, double df_cap, void *cmd,
                              void *stream);

/* ---- prediction ahead under estimated disturbances: observer and delay compensation together --------------------------------------------------
 * kmpc_predict_ahead_batch steps the solver's UNDISTURBED bicycle: behind kmpc_observe_batch it forgets over the dead time what the observer
 * learnt (a steering offset of 0.05 rad turns the heading by about 0.035 rad over 0.35 s).  kmpc_predict_ahead_dist_batch is that prediction on
 * the observer's augmented model, started from the observer's record.  One thread per vehicle, fp64, no FP contraction.
 *   rec [B,40] fp64 DEVICE: kmpc_observe_batch's records, read only (words 0 ... 6 and 35)
 *   est [B,4] fp64 DEVICE: the observer's est_out of this period         z_out [B,4] fp64 DEVICE out (may be est itself)
 *   cmd_hist, depth, period, n_updates, cmd_delay, meas_delay, max_cmd_delay, max_meas_delay, L_a, L_b: exactly as in kmpc_predict_ahead_batch,
 *     and so are Lm, d, tau0 = (p - Lm) n, the steps tau = tau0 ... p n + d - 1 and the log lookup j(tau, d).  The log holds the commands AS SENT,
 *     after kmpc_cmd_offset_batch: then "logged command + disturbance" is what acted.
 *   psi_cap >= 0 [rad]: kmpc_observe_batch's, the cap on the course offset handed to the solver
 * START  a live record (word 35 != 0): (x, y, psi, v, dpsi, ddelta, da) = words 0 ... 6 -- psi is the record's heading, NOT est_out's shifted one.
 *   A fresh record (word 35 == 0) has nothing to predict from: z_out = est bit for bit, no step is taken.
 * PER STEP, h = 0.01, (psi, v: before the step), with (acc, d_f) = the logged command of period j(tau, d):
 *     de = d_f + ddelta;  beta = atan(L_b / (L_a + L_b) * tan(de));  sb = sin(beta)    -- recomputed only when j(tau, d) differs from the step before
 *     th = (psi + dpsi) + beta;  s = sin(th), c = cos(th)
 *     x += h * (v * c);  y += h * (v * s);  psi = wrap(psi + h * (v / L_b * sb));  v = v + h * (acc + da), 0 when that is < 0
 *   dpsi, ddelta and da stay constant and UNCLIPPED inside the model (the observer's own predict does not clip them either); kmpc_observe_batch's
 *   freeze rule (v < v_min) concerns the covariance only and has no part here.  Every operation is rounded on its own; wrap and clip are
 *   kmpc_observe_batch's; tan / atan / sin / cos are the device library's.
 * OUTPUT  z_out = (x, y, wrap(psi + clip(dpsi, psi_cap)), v): the heading convention of est_out.
 * Contracts: (a) with Lm = d = 0 no step is taken and z_out is the est_out kmpc_observe_batch wrote with this record, bit for bit (a record
 *   initialised by that very call: as numbers when z_psi was outside [-pi, pi) or -0); a fresh record returns est bit for bit at any delay.
 *   (b) With dpsi = ddelta = da = 0 in a live record, z_out equals kmpc_predict_ahead_batch on words 0 ... 3 AS NUMBERS (a -0 may become +0): every
 *   added term is a sum with 0.  (c) A non-finite word among words 0 ... 6 and 35 of a vehicle's record, or in its logged commands, poisons that
 *   vehicle's z_out alone: one thread per vehicle, no lane reads another vehicle's words.
 * Argument checks before any device call: kmpc_predict_ahead_batch's, and psi_cap not finite and >= 0 returns KMPC_ERR_ARG; with B > 0 a NULL rec,
 * est, cmd_hist, cmd_delay, meas_delay or z_out returns KMPC_ERR_ARG (text in kmpc_last_error(NULL)); B == 0 succeeds without a launch.
 * Asynchronous on `stream`. */
int32_t kmpc_predict_ahead_dist_batch(int32_t device, int32_t B, const void *rec, const void *est, const void *cmd_hist, int32_t depth,
                                      int64_t period, int32_t n_updates, const int32_t *cmd_delay, const int32_t *meas_delay,
                                      int32_t max_cmd_delay, int32_t max_meas_delay, double L_a, double L_b, double psi_cap, void *z_out,
                                      void *stream);

/* ---- command stage of the node's loop, for B vehicles (scripts/mpc_cmd_pub.jl) --------------------------------------
 * What the loop does between solve_model() and the publish: the waypoint helper's stop flag latches (:100-103); a latched vehicle is
 * commanded accel -1.0 / steer 0.0 (:148-153) and keeps its rate-limit anchor; every other vehicle publishes the solver's first input
 * regardless of the solver status (:120-132) and update_current_input() remembers it for the next solve (:140).
 *   u0 [B,2] fp64 DEVICE in: (accel, steer) from kmpc_solve_batch      stop [B] int32 DEVICE in: kmpc_waypoints_batch's flag
 *   stop_latch [B] uint8 DEVICE in/out                                  u_prev [B,2] fp64 DEVICE in/out (acc, steer)
 *   cmd [B,2] fp64 DEVICE out: accel_cmd, steer_angle_cmd of MPC_cmd
 * Asynchronous on `stream`.  Errors as kmpc_sim_advance_batch. */
int32_t kmpc_command_batch(int32_t device, int32_t B, const void *u0, const int32_t *stop, uint8_t *stop_latch, void *u_prev, void *cmd,
                           void *stream);

/* ---- Frenet reference from look-ahead waypoints: the step between kmpc_waypoints_batch and kmpc_solve_batch_frenet ----------------------
 * Replaces, for B vehicles at once, what the Frenet node does with a received path before it solves
 * (scripts/nodes_gazebo_sim/gazebo_sim_mpc_cmd_pub_frenet.jl): convert_msg_to_path_dict (:54-85: path in the vehicle frame, the origin (0, 0)
 * at s = 0 put in front, s = cumulative chord length), get_reference_frenet (scripts/sim_path_utils/nav_msgs_path_frenet.py:76-86: fit_XY_s
 * :62-73 -- np.interp every 0.5 m and two cubic least-squares fits --, compute_curvature_poly :44-59 -- K = (x'y'' - y'x'') / (x'^2 + y'^2)
 * every 0.25 m and a cubic fit of K --, psi_start = atan2(Y'(0), X'(0)) :84) and update_init_cond(0, 0, -psi_start, v) (:128).
 *   pose [B,3] fp64 DEVICE: x, y, yaw of the vehicle            ref [B,horizon+1,3] fp64 DEVICE: kmpc_waypoints_batch's output (x, y global; psi unused)
 *   v [B] fp64 DEVICE or NULL: measured speed                   k_poly [B,4] out: K(s) coefficients, highest degree first (kmpc_solve_batch_frenet's order)
 *   psi_start [B] out                                           z0 [B,4] out or NULL (needs v): (0, 0, -psi_start, v[b])
 *   fit_status [B] int32 out: 0 fitted, 1 refused
 * horizon 2..56.  fp64 only.  A vehicle is refused when its window has fewer than four 0.5 m resample points (s_end <= 1.5 m: np.polyfit is
 * rank-deficient there), when any input or intermediate is non-finite, or when s_end > 8192 m (bounds the work per vehicle; the longest real
 * window is 57 x 0.2 s x 20 m/s = 228 m); it gets fit_status 1, k_poly = 0, psi_start = 0, z0 = (0, 0, 0, v[b]) (0 for a non-finite v[b]).
 * Every output is always written and always finite; a refused vehicle does not disturb any other.
 * Asynchronous on `stream`.  Errors: negative code, text in kmpc_last_error(NULL). */
int32_t kmpc_frenet_reference_batch(int32_t device, int32_t B, int32_t horizon, const double *pose, const double *ref, const double *v,
                                    double *k_poly, double *psi_start, double *z0, int32_t *fit_status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
