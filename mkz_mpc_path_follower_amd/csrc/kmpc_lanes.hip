// kmpc_lanes.hip -- lanes (kmpc_lane_step_fleet, kmpc_ref_offset_batch), gfx950 only: per vehicle a lane and a commanded lateral offset, the leader
// among the vehicles of its own lane(s), the neighbours in the adjacent lanes, the lane-change decision and the offset ramp of
// include/kmpc_lanes.h; and the lateral shift of a period's waypoint table.
//
// The hot path is the five-way pair search, in kmpc_follow.hip's shape: a workgroup of sixteen waves owns 64 followers, one per lane of a wave and
// the SAME 64 in each of its waves; the candidates stream through LDS in tiles of 1024 -- each thread fetches one candidate and stores its
// arclength, its KEY (the path id of a usable vehicle, -1 of one that is nobody's neighbour) and its OCCUPANCY word of the snapshot occ_in; the
// next tile's words are fetched before the current tile is scanned.  Wave q scans the q-th 64 candidates of the tile with wave-uniform LDS reads;
// the follower's s, key, its three band masks and its five (difference, j) pairs stay in registers.  Inside a wave the candidates come in rising
// j, so `difference < best` alone keeps the lowest j among equal differences.
// The waves' partial winners meet in LDS.  All five searches at once would be 16 waves x 64 followers x 5 x 12 bytes = 60 KB beside the tile; they
// are combined IN TURNS instead, one search at a time through the tile's own 12 KB (two barriers per turn, ten in all, against B / 1024 tiles of
// scanning), by the full rule (smaller difference, then lower j).  No atomics, no second launch, no workspace: the result is a function of the
// inputs alone.  The law, the decision, the ramp and the record run on wave 0's lanes with _rn intrinsics: no product and sum share a rounding.
// Plain C++: vector stores, no inline assembly, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmpc_follow.h"   // KMPC_FOLLOW_*: the follow row's layout
#include "../../include/kmpc_lanes.h"    // KMPC_LANE_*, KMPC_LANEREC_*
#include "kmpc_dispatch.h"
#include "kmpc_stage.h"                  // stage::finite

#pragma clang fp contract(off)

constexpr int LANES_LANES = 64;                          // followers per workgroup
constexpr int LANES_WAVES = 16;                          // waves per workgroup: each scans its sixteenth of every tile
constexpr int LANES_TILE = LANES_LANES * LANES_WAVES;    // candidates per tile = threads per workgroup
constexpr int LANES_SEARCHES = 5;                        // own-ahead, left-ahead, left-behind, right-ahead, right-behind

// vehicle j's key: its path id (0 without path ids) when it is usable, `none` when it is not
__device__ __forceinline__ int lane_key(const LN &w, const unsigned j, const double s, const int none)
{
    const double v = w.speed[(size_t)j * w.speed_stride];
    const int pid = w.path_id ? w.path_id[j] : 0;
    const bool here = w.present ? w.present[j] != 0 : true;
    return (stage::finite(s) && stage::finite(v) && here && pid >= 0) ? pid : none;
}

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

__global__ __launch_bounds__(LANES_TILE) void kmpc_lane_step_kernel(LN w)
{
    __shared__ double t_s[LANES_TILE];        // the tile; after the search, one search's partial differences at a time
    __shared__ int t_key[LANES_TILE];         //           after the search, one search's partial winners at a time
    __shared__ unsigned t_occ[LANES_TILE];
    const unsigned tid = threadIdx.x, lane_id = tid & 63u, wave = tid >> 6, nB = (unsigned)w.B;   // B < 2^31: no unsigned sum below wraps
    const unsigned b = blockIdx.x * LANES_LANES + lane_id;
    // the follower: a key no candidate has (-2) when it is not usable or past the fleet's end, so that it finds nobody; its lane words after the
    // release of step 1, and the three band masks
    double s_b = 0.0, lane = 0.0, from = 0.0, offset = 0.0, e_b = 0.0, n_lanes = 0.0;
    int key_b = -2;
    unsigned own = 0u, lbit = 0u, rbit = 0u;
    bool has_left = false, has_right = false;
    if (b < nB) {
        s_b = w.s_along[(size_t)b * w.s_stride];
        key_b = lane_key(w, b, s_b, -2);
        const double *rec = w.rec + KMPC_LANEREC_WORDS * (size_t)b, *lr = w.lane_rows + KMPC_LANE_WORDS * (size_t)b;
        lane = rec[KMPC_LANEREC_LANE]; from = rec[KMPC_LANEREC_LANE_FROM]; offset = rec[KMPC_LANEREC_OFFSET];
        e_b = w.e_ct[(size_t)b * w.e_stride];
        n_lanes = lr[KMPC_LANE_N_LANES];
        const bool release = from != lane && offset == __dmul_rn(lane, lr[KMPC_LANE_WIDTH]) && fabs(__dsub_rn(e_b, offset)) <= lr[KMPC_LANE_CLEAR_TOL];
        from = release ? lane : from;
        const double up = __dadd_rn(lane, 1.0);
        has_left = up < n_lanes;
        has_right = lane >= 1.0;
        own = lane_bit(lane) | lane_bit(from);
        lbit = has_left ? lane_bit(up) : 0u;
        rbit = has_right ? lane_bit(__dsub_rn(lane, 1.0)) : 0u;
    }
    double best[LANES_SEARCHES];
    int bj[LANES_SEARCHES];
#pragma unroll
    for (int q = 0; q < LANES_SEARCHES; ++q) {
        best[q] = INFINITY;
        bj[q] = -1;
    }
    // this thread's candidate of the first tile; inside the loop the NEXT tile's is fetched before the scan
    double s_j = 0.0;
    int key_j = -1;
    unsigned occ_j = 0u;
    if (tid < nB) {
        s_j = w.s_along[(size_t)tid * w.s_stride];
        key_j = lane_key(w, tid, s_j, -1);
        occ_j = w.occ_in[tid];
    }
    for (unsigned base = 0; base < nB; base += LANES_TILE) {
        __syncthreads();   // every wave is done with the previous tile
        t_s[tid] = s_j;
        t_key[tid] = key_j;
        t_occ[tid] = occ_j;
        __syncthreads();
        const unsigned jn = base + LANES_TILE + tid;   // < 2^31 + 2^11: no wrap
        s_j = 0.0;
        key_j = -1;
        occ_j = 0u;
        if (jn < nB) {
            s_j = w.s_along[(size_t)jn * w.s_stride];
            key_j = lane_key(w, jn, s_j, -1);
            occ_j = w.occ_in[jn];
        }
        const unsigned c0 = wave * LANES_LANES;
#pragma unroll 4
        for (unsigned c = 0; c < LANES_LANES; ++c) {
            const double sc = t_s[c0 + c];
            const int kc = t_key[c0 + c];
            const unsigned oc = t_occ[c0 + c];
            const unsigned jc = base + c0 + c;
            const double d = fabs(__dsub_rn(sc, s_b));   // |s_j - s_b|: the rounding is symmetric, one subtraction serves both directions
            // ahead: s_j > s_b, or the same arclength and a lower index; behind: the complement without b itself.  A candidate past the fleet's
            // end has key -1
            const bool same = kc == key_b;
            const bool ahead = same && (sc > s_b || (sc == s_b && jc < b));
            const bool behind = same && (sc < s_b || (sc == s_b && jc > b));
            const bool t0 = ahead && (oc & own) != 0u && d < best[0];
            const bool t1 = ahead && (oc & lbit) != 0u && d < best[1];
            const bool t2 = behind && (oc & lbit) != 0u && d < best[2];
            const bool t3 = ahead && (oc & rbit) != 0u && d < best[3];
            const bool t4 = behind && (oc & rbit) != 0u && d < best[4];
            best[0] = t0 ? d : best[0]; bj[0] = t0 ? (int)jc : bj[0];
            best[1] = t1 ? d : best[1]; bj[1] = t1 ? (int)jc : bj[1];
            best[2] = t2 ? d : best[2]; bj[2] = t2 ? (int)jc : bj[2];
            best[3] = t3 ? d : best[3]; bj[3] = t3 ? (int)jc : bj[3];
            best[4] = t4 ? d : best[4]; bj[4] = t4 ? (int)jc : bj[4];
        }
    }
    // the waves' shares interleave in j: one search at a time through the tile's words, wave 0 combines by the full rule
#pragma unroll
    for (int q = 0; q < LANES_SEARCHES; ++q) {
        __syncthreads();   // the last tile's scan, or wave 0's reads of the previous turn, are done
        t_s[tid] = best[q];
        t_key[tid] = bj[q];
        __syncthreads();
        if (wave == 0) {
            for (unsigned u = 1; u < LANES_WAVES; ++u) {
                const double d = t_s[u * LANES_LANES + lane_id];
                const int j = t_key[u * LANES_LANES + lane_id];
                const bool take = j >= 0 && (bj[q] < 0 || d < best[q] || (d == best[q] && j < bj[q]));
                best[q] = take ? d : best[q];
                bj[q] = take ? j : bj[q];
            }
        }
    }
    if (wave != 0 || b >= nB) return;

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
            const LaneLaw o = lane_law(best[0], v_b, v_j, d_min, t_h, a_b, k_gap, length, at, cap);
            gap = o.gap; bound = o.bound; v_own = o.v_out;
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
                const LaneLaw o = lane_law(best[qa], v_b, v_a, d_min, t_h, a_b, k_gap, length, at, cap);
                v_side[side] = o.v_out;
                sf = o.gap >= d_min && lhs_front <= o.rad;
                nbr[4 * side] = o.gap; nbr[4 * side + 1] = v_a;
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

hipError_t kmpc_launch_lane_step(const LN &w, hipStream_t st)
{
    const unsigned blocks = ((unsigned)w.B + LANES_LANES - 1) / LANES_LANES;
    return kmpc_launch(kmpc_lane_step_kernel, dim3(blocks), dim3(LANES_TILE), 0, st, w);
}

// one thread per waypoint: X -= d sin(psi), Y += d cos(psi); a vehicle with d == 0 keeps its bits
__global__ __launch_bounds__(256) void kmpc_ref_offset_kernel(RO w)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)w.B * (size_t)w.H1;
    if (i >= n) return;
    const double d = w.offset[(i / (size_t)w.H1) * (size_t)w.offset_stride];
    if (d == 0.0) return;
    double *p = w.ref + 3 * i;
    const double psi = p[2];
    p[0] = __dsub_rn(p[0], __dmul_rn(d, sin(psi)));
    p[1] = __dadd_rn(p[1], __dmul_rn(d, cos(psi)));
}

hipError_t kmpc_launch_ref_offset(const RO &w, hipStream_t st)
{
    const size_t n = (size_t)w.B * (size_t)w.H1;
    return kmpc_launch(kmpc_ref_offset_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w);
}
