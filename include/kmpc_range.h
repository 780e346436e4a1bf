/*
 * include/kmpc_range.h -- a range sensor and a leader tracker per vehicle: car following on a MEASURED gap.
 *
 * An extension of the C ABI of include/kmpc.h, exported from the same library and under the same conventions (return codes, kmpc_last_error,
 * caller-owned buffers, `stream` a hipStream_t passed as void*).  include/kmpc.h's, include/kmpc_follow.h's and include/kmpc_lanes.h's lists of
 * entry points and the ABI version do not change; the three entry points below are this header's.
 *
 * kmpc_follow_fleet (include/kmpc_follow.h) reads the truth: the leader's arclength and speed and the follower's own speed, whatever the
 * controller is allowed to know.  kmpc_range_follow_batch runs BEHIND it, on the gap_out and leader_out it wrote: per vehicle a range sensor
 * (range limit, bias, seeded noise on range and on the leader's speed, dropouts), a two-state Kalman tracker on (gap, leader speed) that coasts
 * through dropouts and starts afresh when the leader changes, and include/kmpc_follow.h's law on what the tracker believes, with the follower's
 * own speed as its controller knows it.  The search stays kmpc_follow_fleet's.  The reference has no such stage.
 */
#ifndef KMPC_RANGE_H
#define KMPC_RANGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*   range_rows [B,16] fp64 DEVICE, row of vehicle b (its own words: no other vehicle's row is read); kmpc_range_default writes B default rows, a
 *   plain automotive radar (120, 0.25, 0.12, 0, 0, 1, 5, 0.01, 0.25, 0.0625, 0.0144, 0 ...), to HOST memory.  SIGMA_* is what the sensor does,
 *   R_* is what the filter believes: separate words. */
enum {
    KMPC_RANGE_RANGE_MAX = 0,   /* a leader farther than this is not seen [m], > 0; +inf: no limit */
    KMPC_RANGE_SIGMA_R = 1,     /* noise on the range [m], >= 0 */
    KMPC_RANGE_SIGMA_V = 2,     /* noise on the leader's speed [m/s], >= 0 */
    KMPC_RANGE_BIAS_R = 3,      /* bias of the range [m] */
    KMPC_RANGE_P_DROP = 4,      /* probability that a leader in range is not reported in a period, 0 ... 1 */
    KMPC_RANGE_FILTER = 5,      /* 0: the track is the last measurement; otherwise (1): the Kalman update below */
    KMPC_RANGE_COAST_MAX = 6,   /* whole periods a track may go without a detection before it is given up, 0 ... 1000 */
    KMPC_RANGE_Q_GAP = 7,       /* process noise added to P00 per period [m^2], >= 0 */
    KMPC_RANGE_Q_V = 8,         /* process noise added to P11 per period [(m/s)^2], >= 0 */
    KMPC_RANGE_R_GAP = 9,       /* measurement variance of the range the filter counts on [m^2], > 0 */
    KMPC_RANGE_R_V = 10,        /* measurement variance of the speed the filter counts on [(m/s)^2], > 0 */
                                /* words 11 ... 15 are read by nobody */
    KMPC_RANGE_WORDS = 16
};
/*   The NEUTRAL row: RANGE_MAX = +inf, SIGMA_R = SIGMA_V = BIAS_R = P_DROP = 0, FILTER = 0.  Behind kmpc_follow_fleet, with speed_known the
 *   pointer of speed_true, it gives kmpc_follow_fleet's own v_cap_out bit for bit (finite follow rows).
 *   rec [B,16] fp64 DEVICE in/out, record of vehicle b, read and written by its own vehicle only, once per call; kmpc_range_rec_init writes B
 *   fresh records (TRACK_ID -1, every other word 0) to HOST memory: */
enum {
    KMPC_RANGEREC_GAP_HAT = 0,     /* tracked gap [m] */
    KMPC_RANGEREC_V_HAT = 1,       /* tracked leader speed [m/s] */
    KMPC_RANGEREC_P00 = 2,         /* covariance of (GAP_HAT, V_HAT): gap-gap */
    KMPC_RANGEREC_P01 = 3,         /*   gap-speed */
    KMPC_RANGEREC_P11 = 4,         /*   speed-speed */
    KMPC_RANGEREC_TRACK_ID = 5,    /* the tracked leader's index as fp64; -1 (any value < 0): no track */
    KMPC_RANGEREC_COAST = 6,       /* periods since the track's last detection */
    KMPC_RANGEREC_N = 7,           /* calls */
    KMPC_RANGEREC_N_DETECT = 8,    /* calls with a detection */
    KMPC_RANGEREC_N_DROP = 9,      /* calls with a leader in range that was dropped */
    KMPC_RANGEREC_N_OUT = 10,      /* calls with a leader beyond RANGE_MAX */
    KMPC_RANGEREC_N_NEW = 11,      /* tracks started */
    KMPC_RANGEREC_N_LOST = 12,     /* tracks given up */
    KMPC_RANGEREC_N_BOUND = 13,    /* calls in which the law's speed was below v_cap */
    KMPC_RANGEREC_SUM_EGAP2 = 14,  /* sum of (GAP_HAT - true gap)^2 over the calls that end with a track and a finite error */
    KMPC_RANGEREC_MAX_EGAP = 15,   /* largest |GAP_HAT - true gap| over the same calls */
    KMPC_RANGEREC_WORDS = 16
};
/*   truth                 [B,2] fp64 DEVICE: kmpc_follow_fleet's gap_out -- the true gap, the leader's true speed v_j
 *   leader                [B] int32 DEVICE: kmpc_follow_fleet's leader_out, -1 = none
 *   speed_true, stride    the plant's speed of follower b at speed_true[b * speed_true_stride]; stride >= 1
 *   speed_known, stride   the follower's speed as its controller knows it at speed_known[b * speed_known_stride]; may be speed_true itself
 *   follow_rows           [B,8] fp64 DEVICE, KMPC_FOLLOW_* (include/kmpc_follow.h): the follower's own row; LENGTH is not read (the gap is given)
 *   seed, period, id_base the draws' key and counter; 0 <= period < 2^61; vehicle b draws as vehicle id_base + b (a shard of a larger fleet)
 *   v_cap, v_cap_out      [B] fp64 DEVICE; may be the same buffer
 *   meas_out              [B,4] fp64 DEVICE or NULL: z_r, z_v (NaN when nothing was detected), detected (1 or 0), COAST after the call
 *
 * THE PERIOD of vehicle b.  fp64, no product and sum contracted, every operation rounded once (the gains are correctly rounded quotients),
 * compare-and-select throughout: a NaN stays in its own vehicle.  Written x = a + b * c, the product is rounded first.  gap, v_j = truth[b];
 * L = leader[b]; v_t, v_k = the two own speeds; cap = v_cap[b]; T = rec[TRACK_ID] as read.
 * 1 DRAWS  one Philox4x32-10 block, the generator of the measurement stage (include/kmpc.h): counter (gid lo, gid hi, period lo,
 *     period hi ^ 0x20000000) with gid = id_base + b, key = seed (the tags 0, 0x80000000, 0x40000000 and 0xC0000000 belong to the measurements,
 *     the faults and the Gauss-Markov stage) -> words w0 ... w3.  (n0, n1) = Box-Muller of (w0, w1) as there: u_i = (w_i + 0.5) * 2^-32,
 *     r = sqrt(-2 log u_0), a = 6.283185307179586 * u_1, n0 = r cos a, n1 = r sin a.  u = (w2 + 0.5) * 2^-32.  w3 is not used.  A vehicle's
 *     draws depend on (seed, id_base + b, period) alone: not on B, on the launch geometry or on the shard.
 * 2 DETECTION  valid = L >= 0 and gap, v_j, v_t, v_k all finite;  inr = valid and gap <= RANGE_MAX;  drop = inr and u < P_DROP;
 *     det = inr and not drop.  N_OUT += 1 when valid and not inr;  N_DROP += 1 when drop;  N_DETECT += 1 when det;  N += 1 always.
 * 3 MEASUREMENT  z_r = gap;  BIAS_R != 0: z_r = z_r + BIAS_R;  SIGMA_R != 0: z_r = z_r + SIGMA_R * n0.
 *     e = v_k - v_t;  z_v = e != 0 ? v_j + e : v_j;  SIGMA_V != 0: z_v = z_v + SIGMA_V * n1.   (a range-rate radar and the vehicle's own idea of
 *     its speed: the neutral row with v_k == v_t carries the truth's own bits)
 * 4 TRACK  new = det and T != L (L as fp64).
 *     new:  (GAP_HAT, V_HAT) = (z_r, z_v);  (P00, P01, P11) = (R_GAP, 0, R_V);  COAST = 0;  TRACK_ID = L;  N_NEW += 1.  No update follows.
 *     not new and T >= 0 -- PREDICT, from the words as read:
 *         GAP_HAT = GAP_HAT + dt * (V_HAT - v_k)
 *         t = dt * P11;  P00 = (P00 + dt * (2 * P01 + t)) + Q_GAP;  P01 = P01 + t;  P11 = P11 + Q_V
 *       then, det (so T == L) -- UPDATE:
 *         FILTER == 0:  (GAP_HAT, V_HAT) = (z_r, z_v);  P stays as predicted.
 *         FILTER != 0:  two scalar updates in sequence, each from the words the step before left:
 *           range  S = P00 + R_GAP;  k0 = P00 / S;  k1 = P01 / S;  y = z_r - GAP_HAT
 *                  GAP_HAT = GAP_HAT + k0 * y;  V_HAT = V_HAT + k1 * y
 *                  P11 = P11 - k1 * P01;  P01 = P01 - k0 * P01;  P00 = P00 - k0 * P00       (in this order: each right side reads old words)
 *           speed  S = P11 + R_V;  k0 = P01 / S;  k1 = P11 / S;  y = z_v - V_HAT
 *                  GAP_HAT = GAP_HAT + k0 * y;  V_HAT = V_HAT + k1 * y
 *                  P00 = P00 - k0 * P01;  P01 = P01 - k1 * P01;  P11 = P11 - k1 * P11       (likewise)
 *         COAST = 0.
 *       not det:  COAST = COAST + 1;  the track is LOST when COAST > COAST_MAX, or T != L, or v_k is not finite:  TRACK_ID = -1;  N_LOST += 1
 *         (the other words stay as predicted; nobody reads them before a new track overwrites them).
 *     not new and T < 0:  the record's words 0 ... 6 stay as read.
 *     After this step a vehicle with a track has TRACK_ID == L.
 * 5 LAW  with a track (TRACK_ID >= 0), include/kmpc_follow.h's law on g = GAP_HAT - D_MIN, v_j := V_HAT, v_b := v_k and the follower's own row:
 *         gp = g > 0 ? g : 0;  at = A_BRAKE * T_HEADWAY
 *         v_safe = sqrt((at * at + V_HAT * V_HAT) + (2 * A_BRAKE) * gp) - at
 *         v_gap  = V_HAT + K_GAP * (g - T_HEADWAY * v_k)
 *         v_f = v_gap < v_safe ? v_gap : v_safe;  v_f = v_f > 0 ? v_f : 0
 *         v_cap_out[b] = v_f < cap ? v_f : cap;  N_BOUND += 1 when the first arm is taken.
 *     WITHOUT A TRACK  v_cap_out[b] = cap, bit for bit.
 * 6 ERROR  with a track: e = GAP_HAT - gap;  e finite:  SUM_EGAP2 = SUM_EGAP2 + e * e;  MAX_EGAP = |e| > MAX_EGAP ? |e| : MAX_EGAP.
 * 7 meas_out[b] = (det ? z_r : NaN, det ? z_v : NaN, det ? 1 : 0, COAST).
 * Properties:
 *   - Association is perfect: the track knows its leader's index.  No false targets, no delay of the range fix, no field of view; arclength
 *     geometry only; fp64 only.
 *   - The kernel cannot refuse a row (Python: ref_traj.check_range_rows): a non-finite word changes that vehicle's own outputs alone.
 * Argument checks before any device call (they answer on a machine without a GPU): B < 0; a stride < 1; dt not finite or <= 0; period < 0 or
 * >= 2^61; with B > 0 a NULL truth, leader, speed_true, speed_known, follow_rows, range_rows, v_cap, v_cap_out or rec: KMPC_ERR_ARG (text in
 * kmpc_last_error(NULL)).  B == 0 succeeds without a launch.  Asynchronous on `stream`. */
int32_t kmpc_range_default(double *rows_host, int32_t B);   /* HOST; KMPC_ERR_ARG for B < 0 or, with B > 0, NULL rows */
int32_t kmpc_range_rec_init(double *rec_host, int32_t B);   /* HOST; KMPC_ERR_ARG for B < 0 or, with B > 0, NULL rec */
int32_t kmpc_range_follow_batch(int32_t device, int32_t B, double dt, const double *truth, const int32_t *leader, const double *speed_true,
                                int32_t speed_true_stride, const double *speed_known, int32_t speed_known_stride, const double *follow_rows,
                                const double *range_rows, uint64_t seed, int64_t period, int64_t id_base, const double *v_cap, double *v_cap_out,
                                double *rec, double *meas_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
