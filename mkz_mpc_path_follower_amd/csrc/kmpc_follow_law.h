// kmpc_follow_law.h -- what every leader search of include/kmpc_follow.h shares once it has its winner: who is usable, and the following law with
// its record.  kmpc_follow.hip (the pair search) and kmpc_order.hip (the search along the order) include it, so that the law exists once; device
// code only, _rn intrinsics throughout: no product and sum share a rounding.
#ifndef KMPC_FOLLOW_LAW_H
#define KMPC_FOLLOW_LAW_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmpc_follow.h"   // KMPC_FOLLOW_*, KMPC_FOLLOWSTAT_*: the row layouts
#include "kmpc_dispatch.h"
#include "kmpc_stage.h"                  // stage::finite

#pragma clang fp contract(off)

// vehicle j's key: its path id (0 without path ids) when it is usable, `none` when it is not.  W: FL or LN, which name these words alike
template <typename W> __device__ __forceinline__ int follow_key(const W &w, const unsigned j, const double s, const int none)
{
    const double v = w.speed[(size_t)j * w.speed_stride];
    const int pid = w.path_id ? w.path_id[j] : 0;
    const bool here = w.present ? w.present[j] != 0 : true;
    return (stage::finite(s) && stage::finite(v) && here && pid >= 0) ? pid : none;
}

// the law and the record of follower b behind leader bj at the rounded difference `best`; bj < 0: no leader.  Writes all of b's outputs
__device__ __forceinline__ void follow_finish(const FL &w, const unsigned b, const double best, const int bj)
{
    const double cap = w.v_cap[b];
    double v_out = cap, gap = INFINITY, v_j = 0.0;
    double *st = w.stat ? w.stat + KMPC_FOLLOWSTAT_WORDS * (size_t)b : nullptr;
    double n_leader = 0.0, n_bound = 0.0, n_contact = 0.0, min_gap = 0.0, max_closing = 0.0;
    if (st) {
        n_leader = st[KMPC_FOLLOWSTAT_N_LEADER]; n_bound = st[KMPC_FOLLOWSTAT_N_BOUND]; n_contact = st[KMPC_FOLLOWSTAT_N_CONTACT];
        min_gap = st[KMPC_FOLLOWSTAT_MIN_GAP]; max_closing = st[KMPC_FOLLOWSTAT_MAX_CLOSING];
    }
    if (bj >= 0) {
        const double *row = w.rows + KMPC_FOLLOW_WORDS * (size_t)b;
        const double d_min = row[KMPC_FOLLOW_D_MIN], t_h = row[KMPC_FOLLOW_T_HEADWAY], a_b = row[KMPC_FOLLOW_A_BRAKE], k_gap = row[KMPC_FOLLOW_K_GAP];
        const double v_b = w.speed[(size_t)b * w.speed_stride];
        v_j = w.speed[(size_t)bj * w.speed_stride];
        gap = __dsub_rn(best, row[KMPC_FOLLOW_LENGTH]);
        const double g = __dsub_rn(gap, d_min), gp = g > 0.0 ? g : 0.0;
        const double at = __dmul_rn(a_b, t_h);
        const double rad = __dadd_rn(__dadd_rn(__dmul_rn(at, at), __dmul_rn(v_j, v_j)), __dmul_rn(__dmul_rn(2.0, a_b), gp));
        const double v_safe = __dsub_rn(__dsqrt_rn(rad), at);
        const double v_gap = __dadd_rn(v_j, __dmul_rn(k_gap, __dsub_rn(g, __dmul_rn(t_h, v_b))));
        double v_f = v_gap < v_safe ? v_gap : v_safe;
        v_f = v_f > 0.0 ? v_f : 0.0;
        const bool bound = v_f < cap;
        v_out = bound ? v_f : cap;
        const double closing = __dsub_rn(v_b, v_j);
        n_leader = __dadd_rn(n_leader, 1.0);
        n_bound = bound ? __dadd_rn(n_bound, 1.0) : n_bound;
        n_contact = gap < 0.0 ? __dadd_rn(n_contact, 1.0) : n_contact;
        min_gap = gap < min_gap ? gap : min_gap;
        max_closing = closing > max_closing ? closing : max_closing;
    }
    w.v_cap_out[b] = v_out;
    if (w.gap_out) {
        w.gap_out[2 * (size_t)b] = gap;
        w.gap_out[2 * (size_t)b + 1] = v_j;
    }
    if (w.leader_out) w.leader_out[b] = bj;
    if (st) {
        st[KMPC_FOLLOWSTAT_N] = __dadd_rn(st[KMPC_FOLLOWSTAT_N], 1.0);
        st[KMPC_FOLLOWSTAT_N_LEADER] = n_leader; st[KMPC_FOLLOWSTAT_N_BOUND] = n_bound; st[KMPC_FOLLOWSTAT_N_CONTACT] = n_contact;
        st[KMPC_FOLLOWSTAT_MIN_GAP] = min_gap; st[KMPC_FOLLOWSTAT_MAX_CLOSING] = max_closing;
    }
}
#endif
