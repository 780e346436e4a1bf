/*
 * include/kmpc_follow.h -- car following in the closed loops: a leader and a gap per vehicle.
 *
 * An extension of the C ABI of include/kmpc.h, exported from the same library and under the same conventions (return codes, kmpc_last_error,
 * caller-owned buffers, `stream` a hipStream_t passed as void*).  include/kmpc.h's own list of entry points and its ABI version do not change; the
 * three entry points below are this header's.
 *
 * Every loop stage so far makes ONE vehicle's world more real; the vehicles of a fleet do not exist for each other.  kmpc_follow_fleet tells each
 * vehicle who is ahead of it on its own recorded path and how fast it may go because of that: per vehicle and per period, the nearest usable vehicle
 * ahead by arclength (the LEADER), the bumper-to-bumper gap, and a speed cap from a car-following law.  The reference has no such stage.
 */
#ifndef KMPC_FOLLOW_H
#define KMPC_FOLLOW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*   rows [B,8] fp64 DEVICE, row of vehicle b (the FOLLOWER's own words: its leader's row is not read): */
enum {
    KMPC_FOLLOW_D_MIN = 0,       /* standstill gap [m]; any finite value */
    KMPC_FOLLOW_T_HEADWAY = 1,   /* time headway [s], >= 0 */
    KMPC_FOLLOW_A_BRAKE = 2,     /* deceleration the law counts on [m/s^2], > 0 */
    KMPC_FOLLOW_K_GAP = 3,       /* gap-feedback gain [1/s], >= 0 */
    KMPC_FOLLOW_LENGTH = 4,      /* vehicle length [m], >= 0: taken off the arclength difference to the leader */
                                 /* words 5 ... 7 are read by nobody */
    KMPC_FOLLOW_WORDS = 8
};
/*   kmpc_follow_default writes B default rows (5.0, 1.0, 0.7, 0.5, 4.9, 0, 0, 0) to HOST memory.
 *   stat [B,8] fp64 DEVICE in/out or NULL, record of vehicle b, read and written once per call; kmpc_follow_stat_init writes B fresh records
 *   (all words 0, MIN_GAP +inf) to HOST memory: */
enum {
    KMPC_FOLLOWSTAT_N = 0,             /* calls */
    KMPC_FOLLOWSTAT_N_LEADER = 1,      /* calls with a leader */
    KMPC_FOLLOWSTAT_N_BOUND = 2,       /* calls in which the law's speed was below v_cap (the cap bound) */
    KMPC_FOLLOWSTAT_N_CONTACT = 3,     /* calls with gap < 0 */
    KMPC_FOLLOWSTAT_MIN_GAP = 4,       /* smallest gap so far [m]; fresh: +inf */
    KMPC_FOLLOWSTAT_MAX_CLOSING = 5,   /* largest v_b - v_j so far [m/s] over the calls with a leader; fresh: 0 (a vehicle that never closed in keeps 0) */
                                       /* words 6, 7 are read by nobody and written back as read */
    KMPC_FOLLOWSTAT_WORDS = 8
};
/*   s_along, s_stride     vehicle b's arclength on its path at s_along[b * s_stride] (the track score's err_out + 3 with stride 4); s_stride >= 1
 *   speed, speed_stride   vehicle b's speed at speed[b * speed_stride] (the plant's state + 3 with stride 8); speed_stride >= 1
 *   path_id               [B] int32 DEVICE or NULL: every vehicle on one path
 *   present               [B] uint8 DEVICE or NULL: 0 = not on the road -- the vehicle has no leader and is nobody's leader
 *   v_cap, v_cap_out      [B] fp64 DEVICE; may be the same buffer
 *   gap_out               [B,2] fp64 DEVICE or NULL: gap, the leader's speed
 *   leader_out            [B] int32 DEVICE or NULL: the leader's index, -1 = none
 *
 * USABLE  vehicle j is usable when s_j and v_j are finite, present[j] != 0 (or present is NULL) and path_id[j] >= 0 (or path_id is NULL).
 * LEADER  of a usable b: among the usable j != b with path_id[j] == path_id[b] that are AHEAD -- s_j > s_b, or s_j == s_b and j < b (of two
 *   vehicles at one arclength exactly one yields) -- the one with the smallest difference s_j - s_b (one rounded subtraction); among equal
 *   differences the lowest j.  A vehicle that is not usable has no leader; a candidate whose difference overflows to +inf is not taken.
 * LAW  fp64, no product and sum contracted, every operation rounded once, compare-and-select throughout (a NaN stays in its own vehicle).  With the
 *   follower's own row and the leader j:
 *     gap    = (s_j - s_b) - LENGTH         g = gap - D_MIN         gp = g > 0 ? g : 0
 *     at     = A_BRAKE * T_HEADWAY
 *     v_safe = sqrt((at * at + v_j * v_j) + (2 * A_BRAKE) * gp) - at     (Gipps: b may still stop behind a leader that brakes at A_BRAKE)
 *     v_gap  = v_j + K_GAP * (g - T_HEADWAY * v_b)                       (constant time headway; may fall below v_j)
 *     v_f    = v_gap < v_safe ? v_gap : v_safe;     v_f = v_f > 0 ? v_f : 0
 *     v_cap_out[b] = v_f < v_cap[b] ? v_f : v_cap[b]                     (BOUND when the first arm is taken)
 *     gap_out[b] = (gap, v_j);  leader_out[b] = j
 *   WITHOUT A LEADER  v_cap_out[b] = v_cap[b], bit for bit;  gap_out[b] = (+inf, 0);  leader_out[b] = -1.
 * STAT  N += 1 in every call.  With a leader: N_LEADER += 1;  N_BOUND += 1 when bound;  N_CONTACT += 1 when gap < 0;
 *   MIN_GAP = gap < MIN_GAP ? gap : MIN_GAP;  c = v_b - v_j, MAX_CLOSING = c > MAX_CLOSING ? c : MAX_CLOSING.
 * Properties:
 *   - The search is exact and deterministic: every follower sees every vehicle of the fleet (O(B^2) comparisons), ties are decided by the rule
 *     above and by nothing else -- not by launch geometry, not by an atomic.  Relabelling the vehicles relabels the leaders.
 *   - The kernel cannot refuse a row (Python: ref_traj.check_follow_rows): a non-finite word changes that vehicle's own outputs alone.  A vehicle
 *     with a non-finite s or speed is no leader; its followers take the next vehicle ahead.
 *   - Same path only, arclength only: no lateral offset, no lanes; two paths that share a road do not see each other.
 * Argument checks before any device call (they answer on a machine without a GPU): B < 0; s_stride or speed_stride < 1; with B > 0 a NULL s_along,
 * speed, rows, v_cap or v_cap_out: KMPC_ERR_ARG (text in kmpc_last_error(NULL)).  B == 0 succeeds without a launch.  Asynchronous on `stream`. */
int32_t kmpc_follow_default(double *rows_host, int32_t B);     /* HOST; KMPC_ERR_ARG for B < 0 or, with B > 0, NULL rows */
int32_t kmpc_follow_stat_init(double *stat_host, int32_t B);   /* HOST; KMPC_ERR_ARG for B < 0 or, with B > 0, NULL stat */
int32_t kmpc_follow_fleet(int32_t device, int32_t B, const double *s_along, int32_t s_stride, const double *speed, int32_t speed_stride,
                          const int32_t *path_id, const uint8_t *present, const double *rows, const double *v_cap, double *v_cap_out,
                          double *gap_out, int32_t *leader_out, double *stat, void *stream);

#ifdef __cplusplus
}
#endif
#endif
