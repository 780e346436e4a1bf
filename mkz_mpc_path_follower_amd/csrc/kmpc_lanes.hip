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
// inputs alone.  The law, the decision, the ramp and the record (kmpc_lanes_law.h, shared with kmpc_order.hip) run on wave 0's lanes with _rn
// intrinsics: no product and sum share a rounding.  Plain C++: vector stores, no inline assembly, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmpc_lanes_law.h"              // lane_own, lane_finish, follow_key: shared with the searches along the order (kmpc_order.hip)

#pragma clang fp contract(off)

constexpr int LANES_LANES = 64;                          // followers per workgroup
constexpr int LANES_WAVES = 16;                          // waves per workgroup: each scans its sixteenth of every tile
constexpr int LANES_TILE = LANES_LANES * LANES_WAVES;    // candidates per tile = threads per workgroup

__global__ __launch_bounds__(LANES_TILE) void kmpc_lane_step_kernel(LN w)
{
    __shared__ double t_s[LANES_TILE];        // the tile; after the search, one search's partial differences at a time
    __shared__ int t_key[LANES_TILE];         //           after the search, one search's partial winners at a time
    __shared__ unsigned t_occ[LANES_TILE];
    const unsigned tid = threadIdx.x, lane_id = tid & 63u, wave = tid >> 6, nB = (unsigned)w.B;   // B < 2^31: no unsigned sum below wraps
    const unsigned b = blockIdx.x * LANES_LANES + lane_id;
    // the follower (kmpc_lanes_law.h): a key no candidate has (-2) when it is not usable or past the fleet's end, so that it finds nobody; its
    // lane words after the release of step 1, and the three band masks
    const LaneOwn o = b < nB ? lane_own(w, b) : LaneOwn();
    const double s_b = o.s_b;
    const int key_b = o.key_b;
    const unsigned own = o.own, lbit = o.lbit, rbit = o.rbit;
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
        key_j = follow_key(w, tid, s_j, -1);
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
            key_j = follow_key(w, jn, s_j, -1);
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
    lane_finish(w, b, o, best, bj);
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
