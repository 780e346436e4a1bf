/*
 * include/kmpc_lanes.h -- lanes in the closed loops: a lane and a lateral offset per vehicle, leaders by lane, overtaking.
 *
 * An extension of the C ABI of include/kmpc.h, exported from the same library and under the same conventions (return codes, kmpc_last_error,
 * caller-owned buffers, `stream` a hipStream_t passed as void*).  include/kmpc.h's and include/kmpc_follow.h's lists of entry points and the ABI
 * version do not change; the four entry points below are this header's.
 *
 * Car following (include/kmpc_follow.h) lets a fast vehicle behind a slow one only queue.  kmpc_lane_step_fleet gives every vehicle a lane of its
 * recorded path -- lane L's centre runs L * WIDTH to the LEFT of the recorded line -- finds its leader among the vehicles in its own lane(s),
 * decides lane changes from the neighbours in the adjacent lanes, and ramps a commanded lateral offset; kmpc_ref_offset_batch shifts a period's
 * waypoint table by that offset, which reaches both solver models.  The reference has no such stage.
 */
#ifndef KMPC_LANES_H
#define KMPC_LANES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*   lane_rows [B,8] fp64 DEVICE, row of vehicle b (its own words: no other vehicle's row is read); kmpc_lane_default writes B default rows
 *   (1, 3.5, 1.0, 0.5, 20, 0.5, 1, 0) to HOST memory: */
enum {
    KMPC_LANE_N_LANES = 0,      /* lanes of the vehicle's road, integer-valued, 1 ... 32 */
    KMPC_LANE_WIDTH = 1,        /* lane width [m], > 0 */
    KMPC_LANE_V_LAT = 2,        /* speed of the offset ramp [m/s], > 0 */
    KMPC_LANE_GAIN = 3,         /* smallest speed advantage that justifies a move left [m/s], >= 0 */
    KMPC_LANE_HOLD = 4,         /* periods after a change before the next decision, integer-valued, >= 0 */
    KMPC_LANE_CLEAR_TOL = 5,    /* tolerance [m] for releasing the old lane, >= 0 */
    KMPC_LANE_KEEP_RIGHT = 6,   /* 0 or 1: move back right when that costs no speed */
                                /* word 7 is read by nobody */
    KMPC_LANE_WORDS = 8
};
/*   rec [B,16] fp64 DEVICE in/out, record of vehicle b, read and written by its own vehicle only, once per call; kmpc_lane_rec_init writes B fresh
 *   records (all words 0, MIN_GAP +inf: lane 0, not changing, offset 0) to HOST memory: */
enum {
    KMPC_LANEREC_LANE = 0,          /* the lane the vehicle is in, or is moving to */
    KMPC_LANEREC_LANE_FROM = 1,     /* the lane it is leaving; == LANE when it is not changing */
    KMPC_LANEREC_OFFSET = 2,        /* commanded lateral offset [m], left positive: ramps to LANE * WIDTH */
    KMPC_LANEREC_HOLD_LEFT = 3,     /* periods until the next decision */
    KMPC_LANEREC_N = 4,             /* words 4 ... 9: KMPC_FOLLOWSTAT_N ... MAX_CLOSING of include/kmpc_follow.h, for the own-band leader */
    KMPC_LANEREC_N_LEADER = 5,
    KMPC_LANEREC_N_BOUND = 6,
    KMPC_LANEREC_N_CONTACT = 7,
    KMPC_LANEREC_MIN_GAP = 8,
    KMPC_LANEREC_MAX_CLOSING = 9,
    KMPC_LANEREC_N_CHANGES = 10,    /* lane changes decided */
    KMPC_LANEREC_SUM_ELANE2 = 11,   /* sum of (e_ct - OFFSET)^2 over the calls in which it was finite */
    KMPC_LANEREC_MAX_ELANE = 12,    /* largest |e_ct - OFFSET| so far */
                                    /* words 13 ... 15 are read by nobody and written back as read */
    KMPC_LANEREC_WORDS = 16
};
/*   s_along, s_stride     vehicle b's arclength at s_along[b * s_stride] (the track score's err_out + 3 with stride 4); s_stride >= 1
 *   e_ct, e_stride        vehicle b's signed cross-track error, LEFT positive, at e_ct[b * e_stride] (err_out + 0 with stride 4); e_stride >= 1
 *   speed, speed_stride   vehicle b's speed at speed[b * speed_stride]; speed_stride >= 1
 *   path_id, present      as in kmpc_follow_fleet, each may be NULL
 *   follow_rows           [B,8] KMPC_FOLLOW_* of include/kmpc_follow.h;  lane_rows [B,8] KMPC_LANE_*
 *   v_cap, v_cap_out      [B] fp64 DEVICE; may be the same buffer
 *   occ_in, occ_out       [B] uint32 DEVICE, the OCCUPANCY: bit L set when the vehicle occupies lane L; a vehicle in the middle of a change occupies
 *                         both lanes.  This is the only thing a vehicle reads of another vehicle's lane state, and it reads it from occ_in, a
 *                         snapshot nobody writes during the call; every vehicle writes its own word of occ_out.  occ_in == occ_out is refused:
 *                         a workgroup would read lane words another workgroup is writing in the same launch.  Fresh value: 1.
 *   gap_out, leader_out   [B,2] / [B] or NULL, as in kmpc_follow_fleet, for the own-band leader
 *   nbr_out               [B,4,2] fp64 or NULL: (gap, speed) of left-ahead, left-behind, right-ahead, right-behind; (+inf, 0) where there is none
 *   k, dt                 the period's index (>= 0: its parity orders the decisions) and length [s] (finite, > 0)
 *
 * bit(x) of a record's lane word x: 1 << (int)x when 0 <= x <= 31, else 0 (a lane word that is not a lane occupies nothing).
 * USABLE and AHEAD are include/kmpc_follow.h's words; BEHIND is the complement: s_j < s_b, or s_j == s_b and j > b.
 * fp64 throughout, every operation rounded once, no product and sum contracted, compare-and-select (a NaN stays in its own vehicle).
 *
 * THE PERIOD of vehicle b.  A vehicle that is not usable gets the outputs of a vehicle without a leader (v_cap_out = v_cap bit for bit, gap_out
 * (+inf, 0), leader_out -1, every nbr_out entry (+inf, 0)), is nobody's neighbour and decides nothing: N += 1, the rest of its record as read
 * (its ramp is held), occ_out[b] = occ_in[b].  For a usable vehicle, with its own lane row and follow row:
 *  1 RELEASE   when LANE_FROM != LANE and OFFSET == LANE * WIDTH and |e_ct - OFFSET| <= CLEAR_TOL:  LANE_FROM = LANE.  (The ramp of step 5 lands
 *              on the product's own bits, so the equality is exact.)
 *  2 SEARCHES  five, in one pass over the usable j != b with path_id[j] == path_id[b], the band test on occ_in[j]:
 *                own-ahead                 occ_in[j] & (bit(LANE) | bit(LANE_FROM)),  j AHEAD
 *                left-ahead, left-behind   occ_in[j] & bit(LANE + 1), only when LANE + 1 < N_LANES;  j AHEAD / BEHIND
 *                right-ahead, right-behind occ_in[j] & bit(LANE - 1), only when LANE >= 1;           j AHEAD / BEHIND
 *              the winner of each has the smallest |s_j - s_b| (one rounded subtraction); among equal differences the lowest j; a difference
 *              that overflows to +inf is not taken.
 *  3 LAW       kmpc_follow_fleet's law and record on the own-ahead winner j (difference d = s_j - s_b):
 *                gap = d - LENGTH   g = gap - D_MIN   gp = g > 0 ? g : 0   at = A_BRAKE * T_HEADWAY
 *                rad = (at * at + v_j * v_j) + (2 * A_BRAKE) * gp          v_safe = sqrt(rad) - at
 *                v_gap = v_j + K_GAP * (g - T_HEADWAY * v_b)    v_f = v_gap < v_safe ? v_gap : v_safe;  v_f = v_f > 0 ? v_f : 0
 *                bound = v_f < v_cap[b];   v_own = v_cap_out[b] = bound ? v_f : v_cap[b]
 *              without a winner v_own = v_cap[b], bound false.  N, N_LEADER, N_BOUND, N_CONTACT, MIN_GAP, MAX_CLOSING as KMPC_FOLLOWSTAT_*.
 *  4 DECISION  only when LANE_FROM == LANE, HOLD_LEFT == 0 and N_LANES > 1; a move LEFT only in even k, a move RIGHT only in odd k (two vehicles
 *              two lanes apart can then never take the lane between them in one period: the later one sees the earlier one's double occupancy).
 *              For a side with ahead-winner a (difference d_a, speed v_a) and behind-winner r (difference d_r = s_b - s_r, speed v_r):
 *                v_side      the law's v_own against a (same formulas, same v_cap);  v_cap[b] without a
 *                safe_front  no a, or   gap_a >= D_MIN  and  (v_b + at) * (v_b + at) <= rad_a          (rad of the law with a as the leader)
 *                safe_rear   no r, or   gap_r >= D_MIN  and  (v_r + at) * (v_r + at) <= (at * at + v_b * v_b) + (2 * A_BRAKE) * gp_r
 *                            with gap_r = d_r - LENGTH, gp_r = max(gap_r - D_MIN, 0) -- all with b's OWN follow row
 *              (the squared Gipps inequality: no square root enters a safety test).
 *                LEFT   when the left lane exists, k is even, bound, v_left - v_own >= GAIN, safe_front and safe_rear
 *                RIGHT  when the right lane exists, k is odd, KEEP_RIGHT != 0, v_right >= v_own, safe_front and safe_rear
 *              On a move: LANE_FROM = LANE, LANE = LANE +- 1, HOLD_LEFT = HOLD, N_CHANGES += 1.
 *              Otherwise (no move, decided or not): h = HOLD_LEFT - 1, HOLD_LEFT = h > 0 ? h : 0.
 *  5 RAMP      target = LANE * WIDTH, step = V_LAT * dt, t = target - OFFSET:  OFFSET = target when |t| <= step, else OFFSET +- step towards it.
 *  6 ERROR     e = e_ct - OFFSET with the OFFSET in force BEFORE step 5; when e is finite SUM_ELANE2 += e * e and MAX_ELANE = max(MAX_ELANE, |e|).
 *  7 OUTPUTS   occ_out[b] = bit(LANE) | bit(LANE_FROM) after the decision; gap_out[b] = (gap, v_j), leader_out[b] = j of step 3; nbr_out[b] the four
 *              side winners' (difference - LENGTH, speed).
 * Properties: the searches are exact and deterministic as kmpc_follow_fleet's (O(B^2), no atomics, no workspace, one launch); with N_LANES == 1,
 * lane 0 and fresh occupancy everywhere v_cap_out, gap_out, leader_out and words 4 ... 9 of the record are kmpc_follow_fleet's bit for bit.  The
 * kernel cannot refuse a row (Python: ref_traj.check_lane_rows): a bad word poisons its own vehicle alone.
 * Limits: lanes are offsets of ONE recorded path; the speed along an offset line differs by 1 - kappa * d and nothing corrects for it; the range
 * sensor is perfect.
 *
 * kmpc_ref_offset_batch: for every point h of vehicle b's table ref [B,H1,3] (X, Y, psi), with d = offset[b * offset_stride]:
 *   X -= d * sin(psi), Y += d * cos(psi) (product and sum rounded separately); psi untouched; a row with d == 0 keeps its bits.
 *
 * Argument checks before any device call (they answer on a machine without a GPU): kmpc_lane_step_fleet: B < 0, k < 0, a stride < 1, dt not
 * finite or <= 0; with B > 0 a NULL s_along, e_ct, speed, follow_rows, lane_rows, v_cap, v_cap_out, occ_in, occ_out or rec, or occ_in == occ_out.
 * kmpc_ref_offset_batch: B < 0, H1 < 1, B * H1 >= 2^31, offset_stride < 1; with B > 0 a NULL ref or offset.  All KMPC_ERR_ARG (text in kmpc_last_error(NULL)).
 * B == 0 succeeds without a launch.  Asynchronous on `stream`. */
int32_t kmpc_lane_default(double *rows_host, int32_t B);    /* HOST; KMPC_ERR_ARG for B < 0 or, with B > 0, NULL rows */
int32_t kmpc_lane_rec_init(double *rec_host, int32_t B);    /* HOST; KMPC_ERR_ARG for B < 0 or, with B > 0, NULL rec */
int32_t kmpc_lane_step_fleet(int32_t device, int32_t B, int32_t k, double dt, const double *s_along, int32_t s_stride, const double *e_ct,
                             int32_t e_stride, const double *speed, int32_t speed_stride, const int32_t *path_id, const uint8_t *present,
                             const double *follow_rows, const double *lane_rows, const double *v_cap, double *v_cap_out, const uint32_t *occ_in,
                             uint32_t *occ_out, double *rec, double *gap_out, int32_t *leader_out, double *nbr_out, void *stream);
int32_t kmpc_ref_offset_batch(int32_t device, int32_t B, int32_t H1, double *ref, const double *offset, int32_t offset_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif
