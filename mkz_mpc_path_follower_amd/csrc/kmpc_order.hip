// kmpc_order.hip -- the order of a fleet by (path, arclength) and the leader searches along it (include/kmpc_order.h), gfx950 only:
// kmpc_order_fleet, kmpc_order_follow_fleet, kmpc_order_lane_step_fleet.  The pair searches of kmpc_follow.hip and kmpc_lanes.hip are the
// specification; what is here gives their results bit for bit in O(B log B).
//
// THE SORT  a stable least-significant-digit radix sort of a 96-bit key per vehicle, eight bits a pass, carrying the vehicle's index alone: the keys
// stay where the key kernel put them, by vehicle, and every pass gathers its digit through the index (the fleet's keys fit the L2 many times over).
// The key of a usable vehicle is (path id, image of the arclength) -- the image is the usual order-preserving one: -0.0 first made +0.0, then all
// bits flipped for a negative value and the sign bit set for the others -- and the key of any other vehicle is (2^31, its index).  The sort starts
// from DESCENDING index, so stability alone gives "index descending among equal arclengths", and the unusable vehicles end up last in ascending
// index.  A pass is three launches: per-workgroup digit counts (LDS atomics on counts, whose order reaches nothing), one exclusive scan over
// (digit, workgroup), and the stable scatter, in which a thread's rank among the equal digits before it comes from ballots inside its wave and
// from per-wave counts in LDS with one writer each.  No global atomic anywhere.  The key kernel also reduces the OR and the AND of all keys; where
// they agree on a digit the whole fleet shares it and the three kernels of that pass return at once -- decided on the device, read by nobody on
// the host.  The passes ping-pong between order_out and one workspace buffer; a last kernel copies when the result landed in the workspace.
//
// THE SEARCHES  one thread per POSITION of the order.  A candidate's rounded difference never decreases along the order, so the winner of the
// pair search -- smallest rounded difference, then lowest index -- is the lowest index in the run of in-band candidates that share the first one's
// rounded difference (order_search).  The follower walks to its successors; the lane stage first builds, per lane below lanes_max, a table of
// the next and of the previous position whose vehicle is usable and occupies that lane (ballots inside a workgroup of 256 positions, the
// workgroups' first and last marks carried across by one wave per lane), and its five searches then jump along those links; a band with a bit
// the tables do not cover walks.  Every entry of `order` is range-checked before it indexes anything, and an entry outside 0 ... B-1 ends the
// search it turns up in (or, as a thread's own position, that thread).  The law, the decision and the records are kmpc_follow_law.h's and
// kmpc_lanes_law.h's, the pair searches' own.  Plain C++: vector stores, no inline assembly, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmpc_lanes_law.h"              // follow_key, follow_finish, lane_own, lane_finish

#pragma clang fp contract(off)

constexpr int ORDER_THREADS = 256;       // threads per workgroup of every kernel here but the two single-workgroup ones
constexpr int ORDER_WAVES = ORDER_THREADS / 64;
constexpr int ORDER_DIGITS = 12;         // 96 bits, eight a pass
constexpr int ORDER_WIDE = 1024;         // threads of the flag kernel and of the scan kernel

// ---------------------------------------------------------------- the sort
// the keys by vehicle, descending index into order_out, and this workgroup's OR / AND of the keys and usable count
__global__ __launch_bounds__(ORDER_THREADS) void kmpc_order_key_kernel(OS w)
{
    __shared__ uint64_t red[4][ORDER_THREADS];
    const unsigned tid = threadIdx.x;
    const size_t nB = (size_t)w.B;
    uint64_t or_lo = 0, and_lo = ~0ull, or_hi = 0, and_hi = 0xffffffffull, cnt = 0;
    for (size_t j = (size_t)blockIdx.x * ORDER_THREADS + tid; j < nB; j += (size_t)gridDim.x * ORDER_THREADS) {
        const double s = w.s_along[j * (size_t)w.s_stride];
        const int key = follow_key(w, (unsigned)j, s, -1);
        uint64_t lo = j;
        uint32_t hi = 0x80000000u;
        if (key >= 0) {
            const uint64_t u = (uint64_t)__double_as_longlong(s == 0.0 ? 0.0 : s);
            lo = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
            hi = (uint32_t)key;
            ++cnt;
        }
        w.key_lo[j] = lo;
        w.key_hi[j] = hi;
        w.order_out[j] = (int32_t)(nB - 1 - j);
        or_lo |= lo; and_lo &= lo; or_hi |= hi; and_hi &= hi;
    }
    red[0][tid] = or_lo; red[1][tid] = and_lo; red[2][tid] = or_hi | (and_hi << 32); red[3][tid] = cnt;
    for (unsigned h = ORDER_THREADS / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) {
            red[0][tid] |= red[0][tid + h];
            red[1][tid] &= red[1][tid + h];
            const uint64_t a = red[2][tid], c = red[2][tid + h];
            red[2][tid] = ((a | c) & 0xffffffffull) | ((a & c) & 0xffffffff00000000ull);
            red[3][tid] += red[3][tid + h];
        }
    }
    if (tid == 0) {
        uint64_t *o = w.blk + 4 * (size_t)blockIdx.x;
        o[0] = red[0][0]; o[1] = red[1][0]; o[2] = red[2][0]; o[3] = red[3][0];
    }
}

// one workgroup: the fleet's OR / AND and count from the key kernel's workgroups -> the mask of the digits the whole fleet shares, the count
__global__ __launch_bounds__(ORDER_WIDE) void kmpc_order_flag_kernel(OS w)
{
    __shared__ uint64_t red[4][ORDER_WIDE];
    const unsigned tid = threadIdx.x;
    const bool have = tid < (unsigned)w.key_blocks;          // key_blocks <= 1024
    const uint64_t *o = w.blk + 4 * (size_t)tid;
    red[0][tid] = have ? o[0] : 0; red[1][tid] = have ? o[1] : ~0ull; red[2][tid] = have ? o[2] : 0xffffffff00000000ull; red[3][tid] = have ? o[3] : 0;
    for (unsigned h = ORDER_WIDE / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) {
            red[0][tid] |= red[0][tid + h];
            red[1][tid] &= red[1][tid + h];
            const uint64_t a = red[2][tid], c = red[2][tid + h];
            red[2][tid] = ((a | c) & 0xffffffffull) | ((a & c) & 0xffffffff00000000ull);
            red[3][tid] += red[3][tid + h];
        }
    }
    if (tid != 0) return;
    const uint64_t d_lo = red[0][0] ^ red[1][0], d_hi = (red[2][0] ^ (red[2][0] >> 32)) & 0xffffffffull;
    unsigned same = 0;
    for (int p = 0; p < ORDER_DIGITS; ++p) {
        const uint64_t d = p < 8 ? (d_lo >> (8 * p)) : (d_hi >> (8 * (p - 8)));
        same |= (d & 255u) == 0 ? 1u << p : 0u;
    }
    w.flags[0] = same;
    w.flags[1] = (uint32_t)red[3][0];
    if (w.count_out) w.count_out[0] = (int32_t)red[3][0];
}

__device__ __forceinline__ unsigned order_digit(const OS &w, const int32_t j, const int p)
{
    return p < 8 ? (unsigned)(w.key_lo[j] >> (8 * p)) & 255u : (w.key_hi[j] >> (8 * (p - 8))) & 255u;
}
// the passes before p that ran decide which buffer holds the indices on entry to pass p
__device__ __forceinline__ bool order_in_ws(const unsigned same, const int p) { return (__popc(~same & ((1u << p) - 1u)) & 1) != 0; }

__global__ __launch_bounds__(ORDER_THREADS) void kmpc_order_hist_kernel(OS w, int p)
{
    __shared__ unsigned h[256];
    const unsigned same = w.flags[0], tid = threadIdx.x;
    if ((same >> p) & 1u) return;
    const int32_t *src = order_in_ws(same, p) ? w.idx : w.order_out;
    h[tid] = 0;
    __syncthreads();
    const size_t nB = (size_t)w.B, begin = (size_t)blockIdx.x * (size_t)w.chunk, end = begin + (size_t)w.chunk < nB ? begin + (size_t)w.chunk : nB;
    for (size_t i = begin + tid; i < end; i += ORDER_THREADS) atomicAdd(&h[order_digit(w, src[i], p)], 1u);   // LDS, counts only
    __syncthreads();
    w.hist[(size_t)tid * (size_t)w.sort_blocks + blockIdx.x] = h[tid];
}

// one workgroup: the exclusive scan of hist over (digit, workgroup), in place
__global__ __launch_bounds__(ORDER_WIDE) void kmpc_order_scan_kernel(OS w, int p)
{
    __shared__ unsigned part[ORDER_WIDE];
    const unsigned tid = threadIdx.x;
    if ((w.flags[0] >> p) & 1u) return;
    const size_t n = 256 * (size_t)w.sort_blocks, per = (n + ORDER_WIDE - 1) / ORDER_WIDE;
    const size_t lo = (size_t)tid * per < n ? (size_t)tid * per : n, hi = lo + per < n ? lo + per : n;
    unsigned sum = 0;
    for (size_t i = lo; i < hi; ++i) sum += w.hist[i];
    part[tid] = sum;
    for (unsigned h = 1; h < ORDER_WIDE; h <<= 1) {          // inclusive scan of the threads' sums
        __syncthreads();
        const unsigned add = tid >= h ? part[tid - h] : 0u;
        __syncthreads();
        part[tid] += add;
    }
    __syncthreads();
    unsigned run = part[tid] - sum;
    for (size_t i = lo; i < hi; ++i) {
        const unsigned c = w.hist[i];
        w.hist[i] = run;
        run += c;
    }
}

__global__ __launch_bounds__(ORDER_THREADS) void kmpc_order_scatter_kernel(OS w, int p)
{
    __shared__ unsigned cnt[ORDER_WAVES][256];
    const unsigned same = w.flags[0], tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if ((same >> p) & 1u) return;
    const bool in_ws = order_in_ws(same, p);
    const int32_t *src = in_ws ? w.idx : w.order_out;
    int32_t *dst = in_ws ? w.order_out : w.idx;
    const size_t nB = (size_t)w.B, begin = (size_t)blockIdx.x * (size_t)w.chunk, end = begin + (size_t)w.chunk < nB ? begin + (size_t)w.chunk : nB;
    unsigned running = w.hist[(size_t)tid * (size_t)w.sort_blocks + blockIdx.x];   // where this workgroup's next vehicle with digit `tid` goes
    const uint64_t below = (1ull << lane) - 1ull;
    for (size_t tile = begin; tile < end; tile += ORDER_THREADS) {
        const size_t i = tile + tid;
        const bool valid = i < end;
        const int32_t j = valid ? src[i] : 0;
        const unsigned d = valid ? order_digit(w, j, p) : 0u;
#pragma unroll
        for (int q = 0; q < ORDER_WAVES; ++q) cnt[q][tid] = 0;
        uint64_t peers = __ballot(valid);                   // the valid lanes of this wave with this thread's digit
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (d >> bit) & 1u;
            const uint64_t m = __ballot(valid && one);
            peers &= one ? m : ~m;
        }
        const unsigned rank = __popcll(peers & below);      // the equal digits before this one in the wave
        __syncthreads();
        if (valid && rank == 0) cnt[wave][d] = __popcll(peers);   // one writer per (wave, digit)
        __syncthreads();
        unsigned at = running;                              // thread `tid` owns digit `tid`: counts -> the waves' first places
#pragma unroll
        for (int q = 0; q < ORDER_WAVES; ++q) {
            const unsigned c = cnt[q][tid];
            cnt[q][tid] = at;
            at += c;
        }
        running = at;
        __syncthreads();
        if (valid) {
            const size_t pos = (size_t)cnt[wave][d] + rank;
            if (pos < nB) dst[pos] = j;
        }
        __syncthreads();                                     // before the next tile clears the counts
    }
}

__global__ __launch_bounds__(ORDER_THREADS) void kmpc_order_finish_kernel(OS w)
{
    const size_t i = (size_t)blockIdx.x * ORDER_THREADS + threadIdx.x;
    if (i < (size_t)w.B && order_in_ws(w.flags[0], ORDER_DIGITS)) w.order_out[i] = w.idx[i];
}

hipError_t kmpc_launch_order(const OS &w, hipStream_t st)
{
    const unsigned per_b = (unsigned)(((size_t)w.B + ORDER_THREADS - 1) / ORDER_THREADS);
    hipError_t e = kmpc_launch(kmpc_order_key_kernel, dim3((unsigned)w.key_blocks), dim3(ORDER_THREADS), 0, st, w);
    if (e == hipSuccess) e = kmpc_launch(kmpc_order_flag_kernel, dim3(1), dim3(ORDER_WIDE), 0, st, w);
    for (int p = 0; p < ORDER_DIGITS && e == hipSuccess; ++p) {
        e = kmpc_launch(kmpc_order_hist_kernel, dim3((unsigned)w.sort_blocks), dim3(ORDER_THREADS), 0, st, w, p);
        if (e == hipSuccess) e = kmpc_launch(kmpc_order_scan_kernel, dim3(1), dim3(ORDER_WIDE), 0, st, w, p);
        if (e == hipSuccess) e = kmpc_launch(kmpc_order_scatter_kernel, dim3((unsigned)w.sort_blocks), dim3(ORDER_THREADS), 0, st, w, p);
    }
    if (e == hipSuccess) e = kmpc_launch(kmpc_order_finish_kernel, dim3(per_b), dim3(ORDER_THREADS), 0, st, w);
    return e;
}

// ---------------------------------------------------------------- the search along the order
// The five words a search needs of vehicle b, and one search from position q.  AHEAD: towards later positions, else towards earlier ones.  ABS: the
// lanes' |s_j - s_b|, else the follower's s_j - s_b (whose zero keeps the winner's sign, as the pair search's does).  tab: the lane tables of this
// direction or null; a band they do not cover (a bit at or above lanes_max), or no tables, walks position by position and tests the band on occ
// (occ null: everybody is in band).  The winner keeps the rounded difference of ITS OWN subtraction, the pair search's `best`.
template <bool AHEAD, bool ABS, typename W>
__device__ __forceinline__ void order_search(const W &w, const int32_t *order, const uint32_t *occ, const int32_t *tab, const int lanes_max,
                                             const unsigned q, const double s_b, const int key_b, const unsigned band, double &best, int &bj)
{
    if (band == 0u) return;
    const size_t nB = (size_t)w.B;
    const bool walk = !tab || (lanes_max < 32 && (band >> lanes_max) != 0u);
    long long r = (long long)q;
    for (;;) {
        if (walk) {
            r += AHEAD ? 1 : -1;
        } else {
            long long t = -1;                                // the nearest link over the band's lanes
            for (unsigned m = band; m != 0u; m &= m - 1u) {
                const int32_t c = tab[(size_t)(__ffs(m) - 1) * nB + (size_t)r];
                if (c >= 0) t = t < 0 ? c : (AHEAD ? (c < t ? c : t) : (c > t ? c : t));
            }
            if (t < 0 || (AHEAD ? t <= r : t >= r)) break;   // none, or a link that does not advance: the tables are not this order's
            r = t;
        }
        if (r < 0 || r >= (long long)nB) break;
        const int32_t j = order[r];
        if ((uint32_t)j >= (uint32_t)nB) break;              // not an entry of an order: the search ends
        const double s_j = w.s_along[(size_t)j * w.s_stride];
        if (follow_key(w, (unsigned)j, s_j, -1) != key_b) break;   // the path's end, or the usable vehicles' end
        if (walk && occ && (occ[j] & band) == 0u) continue;
        const double diff = __dsub_rn(s_j, s_b), d = ABS ? fabs(diff) : diff;
        if (!(d < INFINITY)) break;                          // overflowed: every later candidate's does too
        if (bj >= 0 && d != best) break;                     // the run of the first candidate's rounded difference is over
        if (bj < 0 || j < bj) {
            bj = j;
            best = d;
        }
    }
}

__global__ __launch_bounds__(ORDER_THREADS) void kmpc_order_follow_kernel(OF k)
{
    const FL &w = k.f;
    const size_t q = (size_t)blockIdx.x * ORDER_THREADS + threadIdx.x;
    if (q >= (size_t)w.B) return;
    const int32_t b = k.order[q];
    if ((uint32_t)b >= (uint32_t)w.B) return;
    const double s_b = w.s_along[(size_t)b * w.s_stride];
    const int key_b = follow_key(w, (unsigned)b, s_b, -2);
    double best = INFINITY;
    int bj = -1;
    if (key_b != -2) order_search<true, false>(w, k.order, nullptr, nullptr, 0, (unsigned)q, s_b, key_b, ~0u, best, bj);
    follow_finish(w, (unsigned)b, best, bj);
}

hipError_t kmpc_launch_order_follow(const OF &k, hipStream_t st)
{
    const unsigned blocks = (unsigned)(((size_t)k.f.B + ORDER_THREADS - 1) / ORDER_THREADS);
    return kmpc_launch(kmpc_order_follow_kernel, dim3(blocks), dim3(ORDER_THREADS), 0, st, k);
}

// ---------------------------------------------------------------- the lane tables
// the occupancy word at position q as the tables see it: 0 past the fleet's end, for an entry that is no vehicle and for a vehicle that is not usable
__device__ __forceinline__ unsigned order_occ_at(const OL &k, const size_t q)
{
    const LN &w = k.l;
    if (q >= (size_t)w.B) return 0u;
    const int32_t j = k.order[q];
    if ((uint32_t)j >= (uint32_t)w.B) return 0u;
    return follow_key(w, (unsigned)j, w.s_along[(size_t)j * w.s_stride], -1) >= 0 ? w.occ_in[j] : 0u;
}
// wm[L][wave]: which of the wave's 64 positions occupy lane L
__device__ __forceinline__ void order_wave_masks(const OL &k, uint64_t (*wm)[ORDER_WAVES])
{
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned occ = order_occ_at(k, (size_t)blockIdx.x * ORDER_THREADS + tid);
    for (int L = 0; L < k.lanes_max; ++L) {
        const uint64_t m = __ballot((occ >> L) & 1u);
        if (lane == 0) wm[L][wave] = m;
    }
    __syncthreads();
}

// per workgroup of 256 positions and lane: the first and the last position that occupies it, -1 = none
__global__ __launch_bounds__(ORDER_THREADS) void kmpc_order_lane_mark_kernel(OL k)
{
    __shared__ uint64_t wm[32][ORDER_WAVES];
    order_wave_masks(k, wm);
    const int L = (int)threadIdx.x;
    if (L >= k.lanes_max) return;
    const int base = (int)(blockIdx.x * ORDER_THREADS);     // < B < 2^31
    int first = -1, last = -1;
    for (int q = 0; q < ORDER_WAVES; ++q) {
        const uint64_t m = wm[L][q];
        if (m == 0) continue;
        if (first < 0) first = base + 64 * q + (__ffsll((unsigned long long)m) - 1);
        last = base + 64 * q + 63 - __clzll((long long)m);
    }
    k.first[(size_t)L * k.lane_blocks + blockIdx.x] = first;
    k.last[(size_t)L * k.lane_blocks + blockIdx.x] = last;
}

// one wave per lane: for every workgroup the first occupying position in the workgroups after it and the last in those before it
__global__ __launch_bounds__(64) void kmpc_order_lane_carry_kernel(OL k)
{
    const int lane = (int)threadIdx.x, nb = k.lane_blocks;
    const size_t row = (size_t)blockIdx.x * (size_t)nb;
    int carry = -1;
    for (int base = ((nb - 1) / 64) * 64; base >= 0; base -= 64) {
        const int i = base + lane;
        const int v = i < nb ? k.first[row + i] : -1;
        const uint64_t m = __ballot(v >= 0), above = lane == 63 ? 0ull : m & (~0ull << (lane + 1));
        const int got = __shfl(v, above ? __ffsll((unsigned long long)above) - 1 : 0);
        if (i < nb) k.carry_next[row + i] = above ? got : carry;
        const int head = __shfl(v, m ? __ffsll((unsigned long long)m) - 1 : 0);
        carry = m ? head : carry;
    }
    carry = -1;
    for (int base = 0; base < nb; base += 64) {
        const int i = base + lane;
        const int v = i < nb ? k.last[row + i] : -1;
        const uint64_t m = __ballot(v >= 0), under = m & ((1ull << lane) - 1ull);
        const int got = __shfl(v, under ? 63 - __clzll((long long)under) : 0);
        if (i < nb) k.carry_prev[row + i] = under ? got : carry;
        const int tail = __shfl(v, m ? 63 - __clzll((long long)m) : 0);
        carry = m ? tail : carry;
    }
}

// the tables: per position and lane the next and the previous occupying position
__global__ __launch_bounds__(ORDER_THREADS) void kmpc_order_lane_table_kernel(OL k)
{
    __shared__ uint64_t wm[32][ORDER_WAVES];
    order_wave_masks(k, wm);
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const size_t nB = (size_t)k.l.B, q = (size_t)blockIdx.x * ORDER_THREADS + tid;
    if (q >= nB) return;
    const int base = (int)(blockIdx.x * ORDER_THREADS);
    for (int L = 0; L < k.lanes_max; ++L) {
        const uint64_t m = wm[L][wave];
        const uint64_t above = lane == 63 ? 0ull : m & (~0ull << (lane + 1)), under = m & ((1ull << lane) - 1ull);
        int nx = above ? base + 64 * (int)wave + (__ffsll((unsigned long long)above) - 1) : -1;
        for (int u = (int)wave + 1; u < ORDER_WAVES && nx < 0; ++u)
            if (wm[L][u]) nx = base + 64 * u + (__ffsll((unsigned long long)wm[L][u]) - 1);
        if (nx < 0) nx = k.carry_next[(size_t)L * k.lane_blocks + blockIdx.x];
        int pv = under ? base + 64 * (int)wave + 63 - __clzll((long long)under) : -1;
        for (int u = (int)wave - 1; u >= 0 && pv < 0; --u)
            if (wm[L][u]) pv = base + 64 * u + 63 - __clzll((long long)wm[L][u]);
        if (pv < 0) pv = k.carry_prev[(size_t)L * k.lane_blocks + blockIdx.x];
        k.nxt[(size_t)L * nB + q] = nx;
        k.prv[(size_t)L * nB + q] = pv;
    }
}

__global__ __launch_bounds__(ORDER_THREADS) void kmpc_order_lane_step_kernel(OL k)
{
    const LN &w = k.l;
    const size_t q = (size_t)blockIdx.x * ORDER_THREADS + threadIdx.x;
    if (q >= (size_t)w.B) return;
    const int32_t b = k.order[q];
    if ((uint32_t)b >= (uint32_t)w.B) return;
    const LaneOwn o = lane_own(w, (unsigned)b);
    double best[LANES_SEARCHES];
    int bj[LANES_SEARCHES];
#pragma unroll
    for (int i = 0; i < LANES_SEARCHES; ++i) {
        best[i] = INFINITY;
        bj[i] = -1;
    }
    if (o.key_b != -2) {
        const int32_t *nxt = k.lanes_max > 0 ? k.nxt : nullptr, *prv = k.lanes_max > 0 ? k.prv : nullptr;
        order_search<true, true>(w, k.order, w.occ_in, nxt, k.lanes_max, (unsigned)q, o.s_b, o.key_b, o.own, best[0], bj[0]);
        order_search<true, true>(w, k.order, w.occ_in, nxt, k.lanes_max, (unsigned)q, o.s_b, o.key_b, o.lbit, best[1], bj[1]);
        order_search<false, true>(w, k.order, w.occ_in, prv, k.lanes_max, (unsigned)q, o.s_b, o.key_b, o.lbit, best[2], bj[2]);
        order_search<true, true>(w, k.order, w.occ_in, nxt, k.lanes_max, (unsigned)q, o.s_b, o.key_b, o.rbit, best[3], bj[3]);
        order_search<false, true>(w, k.order, w.occ_in, prv, k.lanes_max, (unsigned)q, o.s_b, o.key_b, o.rbit, best[4], bj[4]);
    }
    lane_finish(w, (unsigned)b, o, best, bj);
}

hipError_t kmpc_launch_order_lane_step(const OL &k, hipStream_t st)
{
    const unsigned blocks = (unsigned)k.lane_blocks;        // ceil(B / 256)
    hipError_t e = hipSuccess;
    if (k.lanes_max > 0) {
        e = kmpc_launch(kmpc_order_lane_mark_kernel, dim3(blocks), dim3(ORDER_THREADS), 0, st, k);
        if (e == hipSuccess) e = kmpc_launch(kmpc_order_lane_carry_kernel, dim3((unsigned)k.lanes_max), dim3(64), 0, st, k);
        if (e == hipSuccess) e = kmpc_launch(kmpc_order_lane_table_kernel, dim3(blocks), dim3(ORDER_THREADS), 0, st, k);
    }
    if (e == hipSuccess) e = kmpc_launch(kmpc_order_lane_step_kernel, dim3(blocks), dim3(ORDER_THREADS), 0, st, k);
    return e;
}
