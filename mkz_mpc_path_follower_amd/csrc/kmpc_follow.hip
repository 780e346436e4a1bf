// kmpc_follow.hip -- car following (kmpc_follow_fleet), gfx950 only: per vehicle the nearest usable vehicle ahead on its own path, the gap to it and
// a speed cap from the following law of include/kmpc_follow.h.
//
// The hot path is the pair search: every follower sees every vehicle of the fleet, B^2 comparisons.  A workgroup of sixteen waves owns 64
// followers, one per lane, and the SAME 64 in each of its waves.  The candidates stream through LDS in tiles of 1024 -- each thread fetches one
// candidate (s, speed, path, present) and stores its arclength and its KEY: the path id of a usable vehicle, -1 of one that cannot lead; the next
// tile's words are fetched before the current tile is scanned, so that their latency hides behind the scan.  Wave q scans the q-th 64 candidates
// of the tile: the candidate's words are wave-uniform LDS reads (a broadcast, no bank conflict), the follower's own s, key and its best
// (difference, j) so far stay in registers.  Inside a wave the candidates come in rising j, so `difference < best` alone keeps the lowest j among
// equal differences; the waves' partial winners meet once, in LDS, and are combined by the full rule (smaller difference, then lower j).  No
// atomics, no second launch, no workspace: the result is a function of the inputs alone.  Sixteen waves per 64 followers, not one follower per
// thread, because a fleet of a few thousand would otherwise occupy a few CUs for a long serial scan: the scan per wave is B / 16 candidates and
// B / 64 workgroups share the chip (at B = 4096 the call is bound by the latency of four tiles, not by the comparisons).
// The law and the record (kmpc_follow_law.h, shared with kmpc_order.hip) run on wave 0's lanes with _rn intrinsics: no product and sum share a
// rounding.  Plain C++: vector stores, no inline assembly, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmpc_follow_law.h"            // follow_key, follow_finish: shared with the search along the order (kmpc_order.hip)

#pragma clang fp contract(off)

constexpr int FOLLOW_LANES = 64;                           // followers per workgroup
constexpr int FOLLOW_WAVES = 16;                           // waves per workgroup: each scans its sixteenth of every tile
constexpr int FOLLOW_TILE = FOLLOW_LANES * FOLLOW_WAVES;   // candidates per tile = threads per workgroup

__global__ __launch_bounds__(FOLLOW_TILE) void kmpc_follow_fleet_kernel(FL w)
{
    __shared__ double t_s[FOLLOW_TILE];     // the tile; after the search, the waves' partial differences
    __shared__ int t_key[FOLLOW_TILE];      //           after the search, the waves' partial leaders
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, nB = (unsigned)w.B;   // B < 2^31: no unsigned sum below wraps
    const unsigned b = blockIdx.x * FOLLOW_LANES + lane;
    // the follower: a key no candidate has (-2) when it is not usable or past the fleet's end, so that it finds no leader
    double s_b = 0.0;
    int key_b = -2;
    if (b < nB) {
        s_b = w.s_along[(size_t)b * w.s_stride];
        key_b = follow_key(w, b, s_b, -2);
    }
    double best = INFINITY;
    int bj = -1;
    // this thread's candidate of the first tile; inside the loop the NEXT tile's is fetched before the scan
    double s_j = 0.0;
    int key_j = -1;
    if (tid < nB) {
        s_j = w.s_along[(size_t)tid * w.s_stride];
        key_j = follow_key(w, tid, s_j, -1);
    }
    for (unsigned base = 0; base < nB; base += FOLLOW_TILE) {
        __syncthreads();   // every wave is done with the previous tile
        t_s[tid] = s_j;
        t_key[tid] = key_j;
        __syncthreads();
        const unsigned jn = base + FOLLOW_TILE + tid;   // < 2^31 + 2^11: no wrap
        s_j = 0.0;
        key_j = -1;
        if (jn < nB) {
            s_j = w.s_along[(size_t)jn * w.s_stride];
            key_j = follow_key(w, jn, s_j, -1);
        }
        const unsigned c0 = wave * FOLLOW_LANES;
#pragma unroll 8
        for (unsigned c = 0; c < FOLLOW_LANES; ++c) {
            const double sc = t_s[c0 + c];
            const int kc = t_key[c0 + c];
            const unsigned jc = base + c0 + c;
            const double d = __dsub_rn(sc, s_b);
            // ahead: s_j > s_b, or the same arclength and a lower index (never b itself).  A candidate past the fleet's end has key -1
            const bool take = kc == key_b && (sc > s_b || (sc == s_b && jc < b)) && d < best;
            best = take ? d : best;
            bj = take ? (int)jc : bj;
        }
    }
    __syncthreads();
    t_s[tid] = best;
    t_key[tid] = bj;
    __syncthreads();
    if (wave != 0 || b >= nB) return;
    for (unsigned q = 1; q < FOLLOW_WAVES; ++q) {   // the waves' shares interleave in j: the full rule
        const double d = t_s[q * FOLLOW_LANES + lane];
        const int j = t_key[q * FOLLOW_LANES + lane];
        const bool take = j >= 0 && (bj < 0 || d < best || (d == best && j < bj));
        best = take ? d : best;
        bj = take ? j : bj;
    }

    follow_finish(w, b, best, bj);
}

hipError_t kmpc_launch_follow_fleet(const FL &w, hipStream_t st)
{
    const unsigned blocks = ((unsigned)w.B + FOLLOW_LANES - 1) / FOLLOW_LANES;
    return kmpc_launch(kmpc_follow_fleet_kernel, dim3(blocks), dim3(FOLLOW_TILE), 0, st, w);
}
