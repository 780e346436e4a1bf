// kmpc_lanes_law.h -- what every lane search of include/kmpc_lanes.h shares around its five winners: the vehicle's own words with the release of
// step 1 and its three band masks, and steps 3 ... 7 (the law on the own-ahead winner, the sides, the decision, the ramp, the record, the outputs).
// kmpc_lanes.hip (the pair search) and kmpc_order.hip (the searches along the order) include it, so that the period exists once; device code only,
// _rn intrinsics throughout: no product and sum share a rounding.
#ifndef KMPC_LANES_LAW_H
#define KMPC_LANES_LAW_H

#include "../../include/kmpc_lanes.h"    // KMPC_LANE_*, KMPC_LANEREC_*
#include "kmpc_follow_law.h"             // follow_key; KMPC_FOLLOW_*: the follow row's layout

#pragma clang fp contract(off)

constexpr int LANES_SEARCHES = 5;        // own-ahead, left-ahead, left-behind, right-ahead, right-behind

// bit(x) of a record's lane word: a word that is not a lane occupies nothing
__device__ __forceinline__ unsigned lane_bit(const double x) { return (x >= 0.0 && x <= 31.0) ? 1u << (int)x : 0u; }

// the following law of include/kmpc_follow.h against a vehicle `diff` ahead at speed v_j, with the follower's own row
struct LaneLaw {
    double gap, rad, v_out;
    bool bound;
};
__device__ __forceinline__ LaneLaw lane_law(const double diff, const double v_b, const double v_j, const double d_min, const double t_h,
                                            const double a_b, const double k_gap, const double length, const double at, const double cap)
{
    LaneLaw o;
    o.gap = __dsub_rn(diff, length);
    const double g = __dsub_rn(o.gap, d_min), gp = g > 0.0 ? g : 0.0;
    o.rad = __dadd_rn(__dadd_rn(__dmul_rn(at, at), __dmul_rn(v_j, v_j)), __dmul_rn(__dmul_rn(2.0, a_b), gp));
    const double v_safe = __dsub_rn(__dsqrt_rn(o.rad), at);
    const double v_gap = __dadd_rn(v_j, __dmul_rn(k_gap, __dsub_rn(g, __dmul_rn(t_h, v_b))));
    double v_f = v_gap < v_safe ? v_gap : v_safe;
    v_f = v_f > 0.0 ? v_f : 0.0;
    o.bound = v_f < cap;
    o.v_out = o.bound ? v_f : cap;
    return o;
}

// vehicle b as the searches see it: a key no candidate has (-2) when it is not usable, so that it finds nobody; its lane words after the release
// of step 1, and the three band masks.  The default is a vehicle past the fleet's end
struct LaneOwn {
    double s_b = 0.0, lane = 0.0, from = 0.0, offset = 0.0, e_b = 0.0, n_lanes = 0.0;
    int key_b = -2;
    unsigned own = 0u, lbit = 0u, rbit = 0u;
    bool has_left = false, has_right = false;
};
__device__ __forceinline__ LaneOwn lane_own(const LN &w, const unsigned b)
{
    LaneOwn o;
    o.s_b = w.s_along[(size_t)b * w.s_stride];
    o.key_b = follow_key(w, b, o.s_b, -2);
    const double *rec = w.rec + KMPC_LANEREC_WORDS * (size_t)b, *lr = w.lane_rows + KMPC_LANE_WORDS * (size_t)b;
    o.lane = rec[KMPC_LANEREC_LANE]; o.from = rec[KMPC_LANEREC_LANE_FROM]; o.offset = rec[KMPC_LANEREC_OFFSET];
    o.e_b = w.e_ct[(size_t)b * w.e_stride];
    o.n_lanes = lr[KMPC_LANE_N_LANES];
    const bool release = o.from != o.lane && o.offset == __dmul_rn(o.lane, lr[KMPC_LANE_WIDTH]) && fabs(__dsub_rn(o.e_b, o.offset)) <= lr[KMPC_LANE_CLEAR_TOL];
    o.from = release ? o.lane : o.from;
    const double up = __dadd_rn(o.lane, 1.0);
    o.has_left = up < o.n_lanes;
    o.has_right = o.lane >= 1.0;
    o.own = lane_bit(o.lane) | lane_bit(o.from);
    o.lbit = o.has_left ? lane_bit(up) : 0u;
    o.rbit = o.has_right ? lane_bit(__dsub_rn(o.lane, 1.0)) : 0u;
    return o;
}

// steps 3 ... 7 of vehicle b's period from its five winners bj[] at the rounded differences best[]; writes all of b's outputs and its record
__device__ __forceinline__ void lane_finish(const LN &w, const unsigned b, const LaneOwn &o, const double (&best)[LANES_SEARCHES],
                                            const int (&bj)[LANES_SEARCHES])
{
    double lane = o.lane, from = o.from;
    const double offset = o.offset, e_b = o.e_b, n_lanes = o.n_lanes;
    const int key_b = o.key_b;
    const bool has_left = o.has_left, has_right = o.has_right;
    double *rec = w.rec + KMPC_LANEREC_WORDS * (size_t)b;
    const double cap = w.v_cap[b];
    double v_own = cap, gap = INFINITY, v_j = 0.0;
    double nbr[8] = {INFINITY, 0.0, INFINITY, 0.0, INFINITY, 0.0, INFINITY, 0.0};
    unsigned occ = w.occ_in[b];
    if (key_b != -2) {
        const double *fr = w.follow_rows + KMPC_FOLLOW_WORDS * (size_t)b, *lr = w.lane_rows + KMPC_LANE_WORDS * (size_t)b;
        const double d_min = fr[KMPC_FOLLOW_D_MIN], t_h = fr[KMPC_FOLLOW_T_HEADWAY], a_b = fr[KMPC_FOLLOW_A_BRAKE], k_gap = fr[KMPC_FOLLOW_K_GAP];
        const double length = fr[KMPC_FOLLOW_LENGTH];
        const double v_b = w.speed[(size_t)b * w.speed_stride];
        const double at = __dmul_rn(a_b, t_h);
        // 3: the law and the record on the own-ahead winner
        double n_leader = rec[KMPC_LANEREC_N_LEADER], n_bound = rec[KMPC_LANEREC_N_BOUND], n_contact = rec[KMPC_LANEREC_N_CONTACT];
        double min_gap = rec[KMPC_LANEREC_MIN_GAP], max_closing = rec[KMPC_LANEREC_MAX_CLOSING];
        bool bound = false;
        if (bj[0] >= 0) {
            v_j = w.speed[(size_t)bj[0] * w.speed_stride];
            const LaneLaw l = lane_law(best[0], v_b, v_j, d_min, t_h, a_b, k_gap, length, at, cap);
            gap = l.gap; bound = l.bound; v_own = l.v_out;
            const double closing = __dsub_rn(v_b, v_j);
            n_leader = __dadd_rn(n_leader, 1.0);
            n_bound = bound ? __dadd_rn(n_bound, 1.0) : n_bound;
            n_contact = gap < 0.0 ? __dadd_rn(n_contact, 1.0) : n_contact;
            min_gap = gap < min_gap ? gap : min_gap;
            max_closing = closing > max_closing ? closing : max_closing;
        }
        // 4: the sides (left: searches 1, 2; right: 3, 4) and the decision
        const double vb_at = __dadd_rn(v_b, at), lhs_front = __dmul_rn(vb_at, vb_at);
        double v_side[2];
        bool safe[2];
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int qa = 1 + 2 * side, qr = 2 + 2 * side;
            v_side[side] = cap;
            bool sf = true, sr = true;
            if (bj[qa] >= 0) {
                const double v_a = w.speed[(size_t)bj[qa] * w.speed_stride];
                const LaneLaw l = lane_law(best[qa], v_b, v_a, d_min, t_h, a_b, k_gap, length, at, cap);
                v_side[side] = l.v_out;
                sf = l.gap >= d_min && lhs_front <= l.rad;
                nbr[4 * side] = l.gap; nbr[4 * side + 1] = v_a;
            }
            if (bj[qr] >= 0) {
                const double v_r = w.speed[(size_t)bj[qr] * w.speed_stride];
                const double gap_r = __dsub_rn(best[qr], length);
                const double g = __dsub_rn(gap_r, d_min), gp = g > 0.0 ? g : 0.0;
                const double rad = __dadd_rn(__dadd_rn(__dmul_rn(at, at), __dmul_rn(v_b, v_b)), __dmul_rn(__dmul_rn(2.0, a_b), gp));
                const double vr_at = __dadd_rn(v_r, at);
                sr = gap_r >= d_min && __dmul_rn(vr_at, vr_at) <= rad;
                nbr[4 * side + 2] = gap_r; nbr[4 * side + 3] = v_r;
            }
            safe[side] = sf && sr;
        }
        const double hold_left = rec[KMPC_LANEREC_HOLD_LEFT];
        const bool decide = from == lane && hold_left == 0.0 && n_lanes > 1.0, even = (w.k & 1) == 0;
        const bool go_left = decide && has_left && even && bound && __dsub_rn(v_side[0], v_own) >= lr[KMPC_LANE_GAIN] && safe[0];
        const bool go_right = decide && has_right && !even && lr[KMPC_LANE_KEEP_RIGHT] != 0.0 && v_side[1] >= v_own && safe[1];
        const bool move = go_left || go_right;
        const double h = __dsub_rn(hold_left, 1.0);
        const double lane_new = go_left ? __dadd_rn(lane, 1.0) : (go_right ? __dsub_rn(lane, 1.0) : lane);
        from = move ? lane : from;
        lane = lane_new;
        // 5: the ramp; 6: the lane error against the offset in force before it
        const double target = __dmul_rn(lane, lr[KMPC_LANE_WIDTH]), step = __dmul_rn(lr[KMPC_LANE_V_LAT], w.dt), t = __dsub_rn(target, offset);
        const double offset_new = fabs(t) <= step ? target : (t > 0.0 ? __dadd_rn(offset, step) : __dsub_rn(offset, step));
        const double e = __dsub_rn(e_b, offset), ae = fabs(e);
        const bool e_ok = stage::finite(e);
        const double sum_e2 = rec[KMPC_LANEREC_SUM_ELANE2], max_e = rec[KMPC_LANEREC_MAX_ELANE];
        rec[KMPC_LANEREC_LANE] = lane; rec[KMPC_LANEREC_LANE_FROM] = from; rec[KMPC_LANEREC_OFFSET] = offset_new;
        rec[KMPC_LANEREC_HOLD_LEFT] = move ? lr[KMPC_LANE_HOLD] : (h > 0.0 ? h : 0.0);
        rec[KMPC_LANEREC_N_LEADER] = n_leader; rec[KMPC_LANEREC_N_BOUND] = n_bound; rec[KMPC_LANEREC_N_CONTACT] = n_contact;
        rec[KMPC_LANEREC_MIN_GAP] = min_gap; rec[KMPC_LANEREC_MAX_CLOSING] = max_closing;
        rec[KMPC_LANEREC_N_CHANGES] = move ? __dadd_rn(rec[KMPC_LANEREC_N_CHANGES], 1.0) : rec[KMPC_LANEREC_N_CHANGES];
        rec[KMPC_LANEREC_SUM_ELANE2] = e_ok ? __dadd_rn(sum_e2, __dmul_rn(e, e)) : sum_e2;
        rec[KMPC_LANEREC_MAX_ELANE] = (e_ok && ae > max_e) ? ae : max_e;
        occ = lane_bit(lane) | lane_bit(from);
    }
    rec[KMPC_LANEREC_N] = __dadd_rn(rec[KMPC_LANEREC_N], 1.0);
    w.v_cap_out[b] = v_own;
    w.occ_out[b] = occ;
    if (w.gap_out) {
        w.gap_out[2 * (size_t)b] = gap;
        w.gap_out[2 * (size_t)b + 1] = v_j;
    }
    if (w.leader_out) w.leader_out[b] = key_b != -2 ? bj[0] : -1;
    if (w.nbr_out) {
#pragma unroll
        for (int i = 0; i < 8; ++i) w.nbr_out[8 * (size_t)b + i] = nbr[i];
    }
}
#endif
