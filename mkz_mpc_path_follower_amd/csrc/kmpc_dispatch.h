// kmpc_dispatch.h -- what crosses translation units on the host side: which kernel runs for a configuration (the contract of kmpc_config in
// include/kmpc.h, as ONE function), the lists of compiled horizons it rests on, and the launchers kmpc_api.hip calls.
// The first part is plain C++17 with no HIP types (tests/test_dispatch.py compiles it with the host compiler); the second needs hipcc.
#pragma once
#include <utility>

#include "kmpc_device.h"

// ---- compiled horizons: each list is written here and nowhere else ---------------------------------------------------------------------------------
typedef std::integer_sequence<int, 8, 12, 16, 20, 24, 28> kmpc_fast_horizons;    // one wave per problem: N % 4 == 0 and 2N + 1 <= 64
typedef std::integer_sequence<int, 32, 36, 40, 44, 48, 50> kmpc_wide_horizons;   // four waves: 5 (N = 32, 36), 6 (40, 44) or 7 (48, 50) tile rows, 5N - 2 <= 256
typedef std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7> kmpc_generic_tiles;      // generic kernel: column tiles NT = ceil(2N / 16), N <= 56
typedef std::integer_sequence<int, 1, 2, 3> kmpc_generic_frenet_tiles;           // ... with the Frenet functor: N <= 24
constexpr int KMPC_QUAD_HORIZON = 8;          // four problems per wave: the reference's own horizon only
constexpr int KMPC_FAST_DENSE_MAX_N = 12;     // the one-wave kernel has a build at one more wave per SIMD up to here (kmpc_fast.hip)
constexpr int KMPC_GENERIC_FRENET_MAX_N = 24;
#ifndef KMPC_QUAD_MIN_BATCH
#define KMPC_QUAD_MIN_BATCH 1024   // below this the one-wave-per-problem kernel's shorter single-solve latency wins (measured: tools/quad_probe.py)
#endif
// a launch of more problems than this no longer fits on the chip at once (2 waves x 4 SIMDs x 256 CUs): the start order matters (kmpc_schedule.hip),
// and the denser one-wave build pays for its spills
constexpr int KMPC_CHIP_FILL_BATCH = 2048;

template <int... Ns> constexpr bool kmpc_in(std::integer_sequence<int, Ns...>, int v) { return ((v == Ns) || ...); }
// run-time value -> compile-time value: f(std::integral_constant<int, V>()) for the list's V equal to v, `none` when there is no such entry
template <typename R, int... Ns, typename F> inline R kmpc_dispatch(std::integer_sequence<int, Ns...>, int v, R none, F &&f)
{
    R r = none;
    (void)((v == Ns ? (r = f(std::integral_constant<int, Ns>()), true) : false) || ...);
    return r;
}

// ---- the selection rule ------------------------------------------------------------------------------------------------------------------------------
enum kmpc_backend {
    KMPC_BACKEND_NONE = 0,   // no kernel: kmpc_create refuses the configuration
    KMPC_BACKEND_GENERIC,    // run-time horizon, one wave (kmpc_kernels.hip)
    KMPC_BACKEND_FAST,       // compile-time horizon, one wave (kmpc_fast.hip)
    KMPC_BACKEND_WIDE,       // compile-time horizon, four waves (kmpc_wide.hip)
    KMPC_BACKEND_QUAD        // four problems per wave (kmpc_quad.hip)
};
struct kmpc_selection {
    kmpc_backend backend;
    bool dense;   // KMPC_BACKEND_FAST only: the build at one more wave per SIMD
};
// The kernel for (model, kernel_variant, N, element type, B); per-problem parameters pick the _par_kernel twin of the same answer.  B enters through the
// two thresholds only, so a configuration is acceptable when it has a kernel at B = 1 and at a B above both (kmpc_selectable).
inline kmpc_selection kmpc_select(int model, int kernel_variant, int N, bool fp64, int B)
{
    const bool fast = kmpc_in(kmpc_fast_horizons(), N), wide = kmpc_in(kmpc_wide_horizons(), N);
    if (model == 1) {   // Frenet functor
        if (kernel_variant == 3) return {N == KMPC_QUAD_HORIZON ? KMPC_BACKEND_QUAD : KMPC_BACKEND_NONE, false};   // every B >= 1
        if (kernel_variant != 1 && fast) return {KMPC_BACKEND_FAST, false};
        if (kernel_variant != 1 && wide) return {fp64 ? KMPC_BACKEND_WIDE : KMPC_BACKEND_NONE, false};   // no fp32 four-wave Frenet kernel
        return {N <= KMPC_GENERIC_FRENET_MAX_N ? KMPC_BACKEND_GENERIC : KMPC_BACKEND_NONE, false};
    }
    if (kernel_variant == 3) return {KMPC_BACKEND_NONE, false};   // the Cartesian four-per-wave kernel is picked by batch size, never forced
    if (kernel_variant == 0 && N == KMPC_QUAD_HORIZON && B >= KMPC_QUAD_MIN_BATCH) return {KMPC_BACKEND_QUAD, false};
    if (kernel_variant != 1 && fast) return {KMPC_BACKEND_FAST, N <= KMPC_FAST_DENSE_MAX_N && B > KMPC_CHIP_FILL_BATCH};
    if (kernel_variant != 1 && wide) return {KMPC_BACKEND_WIDE, false};
    return {KMPC_BACKEND_GENERIC, false};
}
inline bool kmpc_selectable(int model, int kernel_variant, int N, bool fp64)
{
    return kmpc_select(model, kernel_variant, N, fp64, 1).backend != KMPC_BACKEND_NONE &&
           kmpc_select(model, kernel_variant, N, fp64, 1 << 30).backend != KMPC_BACKEND_NONE;
}

// ---- launchers (hipcc only) --------------------------------------------------------------------------------------------------------------------------
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

template <typename... P, typename... A>
inline hipError_t kmpc_launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A &... args)
{
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    return hipGetLastError();
}

// solves: one per back-end; `model` and `dense` are what kmpc_select answered, io.par picks the twin.  hipErrorInvalidValue = no such instantiation.
template <typename T> hipError_t kmpc_launch_solve(const KP &, const KIO<T> &, int model, hipStream_t);
template <typename T> hipError_t kmpc_launch_solve_fast(const KP &, const KIO<T> &, int model, bool dense, hipStream_t);
template <typename T> hipError_t kmpc_launch_solve_wide(const KP &, const KIO<T> &, int model, hipStream_t);
template <typename T> hipError_t kmpc_launch_solve_quad(const KP &, const KIO<T> &, int model, hipStream_t);
// diagnostics
template <typename T> hipError_t kmpc_launch_condense(const KP &, const KDbg<T> &, hipStream_t);
template <typename T> hipError_t kmpc_launch_probe(const T *, const T *, T *, hipStream_t);
template <typename T> hipError_t kmpc_launch_fast_kkt(const KP &, const KDbgK<T> &, hipStream_t);
template <typename T> hipError_t kmpc_launch_wide_kkt(const KP &, const KDbgK<T> &, hipStream_t);
// ... of the Frenet functor and of the four-per-wave kernel: the *.blocks.o objects (the four solver units once more with -DKMPC_KKT_BLOCKS; csrc/Makefile)
template <typename T> hipError_t kmpc_launch_condense_frenet(const KP &, const KDbg<T> &, hipStream_t);
template <typename T> hipError_t kmpc_launch_fast_kkt_frenet(const KP &, const KDbgK<T> &, hipStream_t);
hipError_t kmpc_launch_wide_kkt_frenet(const KP &, const KDbgK<double> &, hipStream_t);   // fp64 only, as the solve
template <typename T> hipError_t kmpc_launch_quad_kkt(const KP &, const KDbgK<T> &, int model, hipStream_t);
// start order and packed records (kmpc_schedule.hip)
template <typename T> hipError_t kmpc_launch_schedule(int B, int N, double dt, const T *z0, size_t zs, const T *ref, size_t rs, uint32_t *hist, uint32_t *hist_next,
                                                      uint32_t *tag, int32_t *perm, hipStream_t st);
template <typename T> hipError_t kmpc_launch_pack(int B, int N, int stride, const T *z0, const T *ref, const T *vt, const T *up, T *rec, hipStream_t st);
// closed-loop simulator: the five plants (kmpc_sim.hip; the pedal-driven plant's kernel: kmpc_drive.hip) behind one argument block
// FIXED reads B, state, cmd, n_updates; ROWS also plant, cmd_delay, cmd_log = cmd_held; QUEUE also depth, period, with cmd_log = cmd_queue; ROAD also
// road, road_stat; DRIVE also drive, llc_rows, llc_rec
enum kmpc_plant_kind { KMPC_PLANT_FIXED, KMPC_PLANT_ROWS, KMPC_PLANT_QUEUE, KMPC_PLANT_ROAD, KMPC_PLANT_DRIVE };
struct PlantCall {
    int B, n_updates;
    double *state;             // [B,8] in/out
    const double *cmd;         // [B,2]
    const double *plant;       // [B,8] KMPC_PLANT_*
    const int32_t *cmd_delay;  // [B] or null
    double *cmd_log;           // the held command [B,2] (or null: no delay), or the ring [depth,B,2]
    int depth;                 // periods in the ring
    long long period;
    const double *road;        // [B,8] KMPC_ROAD_*
    double *road_stat;         // [B,4] in/out KMPC_ROAD_STAT_*, or null
    const double *drive;       // [B,8] KMPC_DRIVE_*
    const double *llc_rows;    // [B,8] KMPC_LLC_*
    double *llc_rec;           // [B,16] in/out KMPC_LLCREC_*
};
hipError_t kmpc_launch_plant(kmpc_plant_kind kind, const PlantCall &k, hipStream_t st);
// measurement stage (kmpc_sim.hip), and with sensor faults (kmpc_sense_faults.hip); meas_delay and truth_ring both NULL: no ring
hipError_t kmpc_launch_sense(int B, const double *state, const double *sensor, uint64_t seed, uint64_t period, uint64_t id_base,
                             const int32_t *meas_delay, double *truth_ring, int depth, double *est, hipStream_t st);
hipError_t kmpc_launch_sense_faults(int B, const double *state, const double *sensor, const double *faults, uint64_t seed, uint64_t period,
                                    uint64_t id_base, const int32_t *meas_delay, double *truth_ring, int depth, double *fault_rec, double *z_out,
                                    double *held_out, int32_t *flags_out, uint8_t *blind_out, hipStream_t st);
// Gauss-Markov stage (kmpc_wander.hip); each pair (base, out) both NULL or both given
hipError_t kmpc_launch_wander(int B, const double *wander, double *wander_rec, uint64_t seed, uint64_t period, uint64_t id_base,
                              const double *sensor_base, double *sensor_out, const double *road_base, double *road_out, hipStream_t st);
// low-level controller as a stage of its own (kmpc_drive.hip)
hipError_t kmpc_launch_llc_step(int B, const double *cmd, const double *speed, int speed_stride, const double *llc_rows, double *llc_rec,
                                double *pedals_out, hipStream_t st);
// delay compensation (kmpc_latency.hip)
hipError_t kmpc_launch_cmd_in_force(int B, const double *hist, int depth, long long period, int n, const int32_t *cmd_delay, const int32_t *meas_delay,
                                    int max_cmd_delay, int max_meas_delay, double *u_out, hipStream_t st);
hipError_t kmpc_launch_predict_ahead(int B, const double *z, const double *hist, int depth, long long period, int n, const int32_t *cmd_delay,
                                     const int32_t *meas_delay, int max_cmd_delay, int max_meas_delay, double L_a, double L_b, double *z_out,
                                     hipStream_t st);
// state estimator (kmpc_estimator.hip)
hipError_t kmpc_launch_estimate(int B, double *rec, const double *z, const double *u, int u_stride, const double *params, double dt, double L_a,
                                double L_b, double gate, double *est_out, double *innov_out, int32_t *flags_out, hipStream_t st);
// disturbance observer and command offset (kmpc_observer.hip)
hipError_t kmpc_launch_observe(int B, double *rec, const double *z, const double *u, int u_stride, const double *params, double dt, double L_a,
                               double L_b, double gate, double v_min, double psi_cap, double *est_out, double *dist_out, double *innov_out,
                               int32_t *flags_out, hipStream_t st);
hipError_t kmpc_launch_cmd_offset(int B, const double *rec, const uint8_t *latch, double acc_cap, double df_cap, double *cmd, hipStream_t st);
// prediction ahead under estimated disturbances (kmpc_predict_dist.hip)
hipError_t kmpc_launch_predict_ahead_dist(int B, const double *rec, const double *est, const double *hist, int depth, long long period, int n,
                                          const int32_t *cmd_delay, const int32_t *meas_delay, int max_cmd_delay, int max_meas_delay, double L_a,
                                          double L_b, double psi_cap, double *z_out, hipStream_t st);
hipError_t kmpc_launch_command(int B, const double *u0, const int32_t *stop, uint8_t *latch, double *u_prev, double *cmd, hipStream_t st);

// batched waypoint generation (kmpc_waypoints.hip; scripts/gps_utils/ref_gps_traj.py)
struct WP {
    int M, B, H;         // path samples, vehicles, horizon (H+1 waypoints)
    int use_vtarget;     // 1: arclength grid with per-vehicle v_target, 0: time grid
    double traj_dt;
    const double *t, *X, *Y, *psi, *s;
    const double *pose;  // [B,3] x, y, yaw
    const double *vt;    // [B] or null
    double *ref;         // [B,H+1,3] x, y, psi
    int32_t *stop;       // [B]
    int32_t *closest;    // [B] or null (diagnostic)
};
hipError_t kmpc_launch_waypoints(const WP &w, hipStream_t st);

// the same for a fleet on P recorded paths: a path and a tracking mode per vehicle (kmpc_waypoints_fleet_kernel)
struct WPF {
    int P, B, H;               // paths, vehicles, horizon (H+1 waypoints)
    int total;                 // sum of the paths' sample counts = off[P]
    int all_time;              // read only when time_mode is null: 1 every vehicle on the time grid, 0 every vehicle on the arclength grid
    double traj_dt;
    const double *d;           // t | X | Y | psi | s, each `total` doubles, the paths concatenated
    const int32_t *off;        // [P+1] first sample of each path
    const int32_t *path_id;    // [B]
    const uint8_t *time_mode;  // [B] or null
    const double *pose;        // [B,3] x, y, yaw
    const double *vt;          // [B] or null (not read for a vehicle in time mode)
    double *ref;               // [B,H+1,3] x, y, psi
    int32_t *stop;             // [B]
    int32_t *closest;          // [B] or null: index within the vehicle's own path, -1 if refused
};
hipError_t kmpc_launch_waypoints_fleet(const WPF &w, hipStream_t st);

// tracking errors and the running score record (kmpc_track_score.hip; scripts/analysis/plot_path_tracking_error.py:21-43, 155-162)
struct TS {
    int B, stride;             // vehicles; doubles between two rows of `state` (>= 3)
    double settle_tol;
    const double *state;       // row b: X, Y, psi first (the plant's state [B,8], or pose [B,3])
    const int32_t *status;     // [B]   } the period's command side: all four or none
    const int32_t *iters;      // [B]   }
    const double *cmd;         // [B,2] }
    const uint8_t *latch;      // [B]   }
    double *err;               // [B,4] e_ct, e_near, e_psi, s_along, or null
    int32_t *seg;              // [B] or null
    int32_t *closest;          // [B] or null
    double *score;             // [B,16] in/out or null (layout: include/kmpc.h)
};
struct TSB {                   // one path
    TS w;
    int M;
    const double *X, *Y, *psi, *s;
};
struct TSF {                   // a set of paths, a path per vehicle
    TS w;
    int P, total;
    const double *d;           // t | X | Y | psi | s, each `total` doubles
    const int32_t *off;        // [P+1]
    const int32_t *path_id;    // [B]
};
hipError_t kmpc_launch_track_score(const TSB &k, hipStream_t st);
hipError_t kmpc_launch_track_score_fleet(const TSF &k, hipStream_t st);

// curvature table of a set of paths and a speed plan per vehicle (kmpc_speed_plan.hip)
struct SPC {
    int P, total;              // paths; sum of the paths' sample counts = off[P]
    double h;                  // half the arclength window
    const double *d;           // t | X | Y | psi | s, each `total` doubles
    const int32_t *off;        // [P+1]
    double *kappa;             // [total]
};
struct SPF {
    int P, B, total, stride;   // paths, vehicles, samples in all; doubles between two rows of `state` (>= 2)
    const double *d;           // t | X | Y | psi | s, each `total` doubles
    const int32_t *off;        // [P+1]
    const double *kappa;       // [total] the table kmpc_launch_curvature wrote
    const double *profile;     // [total,8] the map (layout: include/kmpc.h, KMPC_PROFILE_*), or null: the plan without one
    const double *state;       // row b: X, Y first
    const int32_t *path_id;    // [B]
    const double *v_cap;       // [B]
    const double *rows;        // [B,8] (layout: include/kmpc.h, KMPC_PLAN_*)
    double *v_plan;            // [B]
    double *info;              // [B,4] w, s_jb - s_i, kappa_jb, sqrt(lim_i), or null
    int32_t *closest;          // [B] or null: index within the vehicle's own path, -1 if refused
};
hipError_t kmpc_launch_curvature(const SPC &k, hipStream_t st);
hipError_t kmpc_launch_speed_plan_fleet(const SPF &w, hipStream_t st);

// the road under each vehicle, from a profile of a set of paths (kmpc_road_profile.hip)
struct RPF {
    int P, B, total, stride;   // paths, vehicles, samples in all; doubles between two rows of `state` (>= 2)
    const double *d;           // t | X | Y | psi | s, each `total` doubles
    const int32_t *off;        // [P+1]
    const double *profile;     // [total,8] (layout: include/kmpc.h, KMPC_PROFILE_*)
    const double *state;       // row b: X, Y first
    const int32_t *path_id;    // [B]
    const double *road_base;   // [B,8] the caller's road rows (KMPC_ROAD_*)
    double *road_out;          // [B,8] what the plant reads; never road_base
    int32_t *closest;          // [B] or null: index within the vehicle's own path, -1 if refused
};
hipError_t kmpc_launch_road_profile_fleet(const RPF &w, hipStream_t st);

// car following: a leader, a gap and a speed cap per vehicle (kmpc_follow.hip; layouts: include/kmpc_follow.h)
struct FL {
    int B, s_stride, speed_stride;   // vehicles; doubles between two vehicles' arclengths and between two vehicles' speeds (each >= 1)
    const double *s_along;           // vehicle b's arclength on its path at s_along[b * s_stride]
    const double *speed;             // vehicle b's speed at speed[b * speed_stride]
    const int32_t *path_id;          // [B] or null: one path
    const uint8_t *present;          // [B] or null: everybody on the road
    const double *rows;              // [B,8] KMPC_FOLLOW_*
    const double *v_cap;             // [B]
    double *v_cap_out;               // [B]; may be v_cap
    double *gap_out;                 // [B,2] gap, the leader's speed, or null
    int32_t *leader_out;             // [B] or null: -1 = none
    double *stat;                    // [B,8] in/out KMPC_FOLLOWSTAT_*, or null
};
hipError_t kmpc_launch_follow_fleet(const FL &w, hipStream_t st);

// lanes: a lane and a lateral offset per vehicle, leaders by lane, lane changes (kmpc_lanes.hip; layouts: include/kmpc_lanes.h)
struct LN {
    int B, k, s_stride, e_stride, speed_stride;   // vehicles, the period's index; doubles between two vehicles' words (each >= 1)
    double dt;                       // the period [s]
    const double *s_along, *e_ct, *speed;
    const int32_t *path_id;          // [B] or null: one path
    const uint8_t *present;          // [B] or null: everybody on the road
    const double *follow_rows;       // [B,8] KMPC_FOLLOW_*
    const double *lane_rows;         // [B,8] KMPC_LANE_*
    const double *v_cap;             // [B]
    double *v_cap_out;               // [B]; may be v_cap
    const uint32_t *occ_in;          // [B] the snapshot every vehicle reads
    uint32_t *occ_out;               // [B] never occ_in
    double *rec;                     // [B,16] in/out KMPC_LANEREC_*
    double *gap_out;                 // [B,2] or null
    int32_t *leader_out;             // [B] or null
    double *nbr_out;                 // [B,4,2] or null
};
hipError_t kmpc_launch_lane_step(const LN &w, hipStream_t st);
// the lateral shift of a waypoint table (kmpc_lanes.hip)
struct RO {
    int B, H1, offset_stride;
    double *ref;                     // [B,H1,3] X, Y, psi, shifted in place
    const double *offset;            // vehicle b's offset at offset[b * offset_stride]
};
hipError_t kmpc_launch_ref_offset(const RO &w, hipStream_t st);

// range sensor and leader tracker behind kmpc_follow_fleet (kmpc_range.hip; layouts: include/kmpc_range.h)
struct RG {
    int B, true_stride, known_stride;   // vehicles; doubles between two vehicles' speeds (each >= 1)
    double dt;                       // the period [s]
    uint64_t seed, period, id_base;  // the draws' key and counter
    const double *truth;             // [B,2] the true gap, the leader's true speed (kmpc_follow_fleet's gap_out)
    const int32_t *leader;           // [B] -1 = none (kmpc_follow_fleet's leader_out)
    const double *speed_true;        // follower b's speed at speed_true[b * true_stride]
    const double *speed_known;       // ... as its controller knows it, at speed_known[b * known_stride]; may be speed_true
    const double *follow_rows;       // [B,8] KMPC_FOLLOW_*
    const double *range_rows;        // [B,16] KMPC_RANGE_*
    const double *v_cap;             // [B]
    double *v_cap_out;               // [B]; may be v_cap
    double *rec;                     // [B,16] in/out KMPC_RANGEREC_*
    double *meas_out;                // [B,4] z_r, z_v, detected, COAST, or null
};
hipError_t kmpc_launch_range_follow(const RG &w, hipStream_t st);

// the order of a fleet by (path, arclength) and the searches along it (kmpc_order.hip; include/kmpc_order.h).  The workspace, laid out once for
// kmpc_order_bytes, kmpc_order_fleet and kmpc_order_lane_step_fleet: byte offsets of its regions (each a multiple of 256) and the launch geometry
// that sizes them.  Monotone in B and in lanes_max; B == 0 needs nothing.
struct OrderLayout {
    size_t key_lo, key_hi, idx, hist, blk, flags;           // the sort: keys by vehicle, the second index buffer, digit counts, block reductions, flags
    size_t nxt, prv, first, last, carry_next, carry_prev;   // the lanes: tables [lanes_max,B], block marks and carries [lanes_max,lane_blocks]
    size_t bytes;
    int key_blocks, sort_blocks, chunk, lane_blocks;
};
inline OrderLayout kmpc_order_layout(int B, int lanes_max)
{
    OrderLayout o = {};
    if (B <= 0) return o;
    const size_t n = (size_t)B, lm = (size_t)lanes_max;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t kb = (n + 255) / 256, big = (size_t)1 << 21;
    o.key_blocks = (int)(kb < 1024 ? kb : 1024);
    o.chunk = n <= big ? 2048 : (int)up((n + 1023) / 1024);     // positions per workgroup of a sort pass: at most 1024 workgroups
    o.sort_blocks = (int)((n + (size_t)o.chunk - 1) / (size_t)o.chunk);
    o.lane_blocks = (int)kb;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += up(bytes); return at; };
    o.key_lo = take(8 * n); o.key_hi = take(4 * n); o.idx = take(4 * n);
    o.hist = take(4 * 256 * (n <= big ? (n + 2047) / 2048 : (size_t)1024));
    o.blk = take(32 * (size_t)o.key_blocks); o.flags = take(256);
    o.nxt = take(4 * n * lm); o.prv = take(4 * n * lm);
    o.first = take(4 * kb * lm); o.last = take(4 * kb * lm); o.carry_next = take(4 * kb * lm); o.carry_prev = take(4 * kb * lm);
    o.bytes = off;
    return o;
}
struct OS {                          // kmpc_order_fleet
    int B, s_stride, speed_stride;
    const double *s_along, *speed;
    const int32_t *path_id;          // [B] or null
    const uint8_t *present;          // [B] or null
    int32_t *order_out;              // [B]: also the first of the two index buffers of the sort
    int32_t *count_out;              // [1] or null
    uint64_t *key_lo;                // [B] by vehicle: the low 64 bits of its key
    uint32_t *key_hi;                // [B] by vehicle: the high 32 bits
    int32_t *idx;                    // [B] the second index buffer
    uint32_t *hist;                  // [256,sort_blocks] a pass's digit counts, scanned in place
    uint64_t *blk;                   // [key_blocks,4] OR and AND of the keys, the usable count, per workgroup of the key kernel
    uint32_t *flags;                 // [0] bit p: digit p is the same for the whole fleet; [1] the usable count
    int key_blocks, sort_blocks, chunk;
};
hipError_t kmpc_launch_order(const OS &w, hipStream_t st);
struct OF {                          // kmpc_order_follow_fleet
    FL f;
    const int32_t *order;            // [B]
};
hipError_t kmpc_launch_order_follow(const OF &k, hipStream_t st);
struct OL {                          // kmpc_order_lane_step_fleet
    LN l;
    const int32_t *order;            // [B]
    int lanes_max, lane_blocks;
    int32_t *nxt, *prv;              // [lanes_max,B] next / previous position whose vehicle is usable and occupies the lane, -1 = none
    int32_t *first, *last, *carry_next, *carry_prev;   // [lanes_max,lane_blocks]
};
hipError_t kmpc_launch_order_lane_step(const OL &k, hipStream_t st);

// batched Frenet reference: vehicle-frame path, curvature-polynomial fit, initial condition (kmpc_frenet_ref.hip;
// scripts/nodes_gazebo_sim/gazebo_sim_mpc_cmd_pub_frenet.jl:54-85, scripts/sim_path_utils/nav_msgs_path_frenet.py:44-86)
struct FR {
    int B, H;            // vehicles, horizon (H+1 waypoints, 2 <= H <= 56)
    const double *pose;  // [B,3] x, y, yaw
    const double *ref;   // [B,H+1,3] x, y, psi (psi unused)
    const double *v;     // [B] or null
    double *k_poly;      // [B,4] highest degree first
    double *psi;         // [B] psi_start
    double *z0;          // [B,4] (0, 0, -psi_start, v) or null
    int32_t *status;     // [B] 0 fitted, 1 refused
};
hipError_t kmpc_launch_frenet_ref(const FR &f, hipStream_t st);
#endif
