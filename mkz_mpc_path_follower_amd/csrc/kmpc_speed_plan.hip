// kmpc_speed_plan.hip -- curvature- and grip-limited target speeds on gfx950: a curvature table of a set of recorded paths, and a speed per vehicle.
//
// The reference node drives every corner at one constant target_vel (scripts/mpc_cmd_pub.jl:58-62); it has no such stage.  This one answers, per
// vehicle and per period, "how fast may I be HERE so that I can still brake, at A_BRAKE, to what every sample ahead of me allows": the backward
// braking pass of a speed profile, v^2 <= v_lim,j^2 + 2 a (s_j - s_i), as a min-reduction over the samples j >= i of the vehicle's own path, with
// v_lim,j^2 = min(v_cap^2, A_LAT / |kappa_j|).  The rows (A_LAT, A_BRAKE, V_FLOOR, END_STOP) are per vehicle, so it cannot be a table per path.
//
// kmpc_curvature_kernel: one thread per sample of the set's concatenated allocation.  kappa_i is the difference of the RECORDED HEADING over an
// arclength window around s_i (two binary searches inside the sample's own path), not a three-point circle through recorded positions: GPS jitter
// and near-stationary samples make the latter useless on recorded paths.
// kmpc_speed_plan_fleet_kernel: one wavefront per vehicle, as kmpc_waypoints_fleet_kernel.  The nearest sample i is nearest_sample (kmpc_nearest.h),
// the waypoint kernel's argmin; then lanes take 64 consecutive samples per chunk from i on, keep their own minimum and lowest index, and the wave
// reduces with dpp_min after every chunk so that the loop can stop -- exactly -- at the first chunk whose first sample's braking term alone is >=
// the running minimum (s is non-decreasing and every limit is >= 0: no later term can be smaller, and an equal one loses to the lower index).
// kmpc_speed_plan_fleet_kernel<true> is the plan with a map (kmpc_speed_plan_fleet_profile): the same body, with the limit of sample j read through the
// road profile's row of that sample (MU_SCALE scales A_LAT, V_LIMIT^2 joins the minimum); <false> computes what it computed before the map existed.
// Arithmetic is _rn intrinsics throughout: no product and sum share a rounding, and the outputs match the numpy restatement bit for bit (v_plan and
// sqrt(lim_i) as far as the device's fp64 sqrt is correctly rounded).  Plain C++: vector stores, no inline assembly, no scratch.
#include "../../include/kmpc.h"   // KMPC_PLAN_*, KMPC_PROFILE_*: the row layouts
#include "kmpc_common.h"
#include "kmpc_dispatch.h"
#include "kmpc_nearest.h"
#include "kmpc_stage.h"           // stage::finite

#pragma clang fp contract(off)

// the first of p, p + 2 pi, p - 2 pi of smallest magnitude: fix_heading of the track score (kmpc_track_score.hip; plot_path_tracking_error.py:36-43)
DEV double plan_fix_heading(const double p0)
{
    const double p1 = __dadd_rn(p0, 2.0 * M_PI), p2 = __dsub_rn(p0, 2.0 * M_PI);
    double p = p0;
    if (fabs(p1) < fabs(p)) p = p1;
    if (fabs(p2) < fabs(p)) p = p2;
    return p;
}

__global__ __launch_bounds__(256) void kmpc_curvature_kernel(SPC k)
{
    const unsigned gu = blockIdx.x * 256u + threadIdx.x;   // total < 2^31: no wrap
    if (gu >= (unsigned)k.total) return;
    const int g = (int)gu;
    int lo = 0, hi = k.P;   // the sample's path: the largest p with off[p] <= g (off[0] = 0 <= g < off[P])
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (k.off[mid] <= g) lo = mid; else hi = mid; }
    const int o0 = k.off[lo], M = k.off[lo + 1] - o0, i = g - o0;
    const size_t n = (size_t)k.total;
    const double *psi = k.d + 3 * n + o0, *s = k.d + 4 * n + o0;   // d = t | X | Y | psi | s; from here on indices 0 .. M-1 of the sample's own path only
    const double a = __dsub_rn(s[i], k.h), b = __dadd_rn(s[i], k.h);
    int l = 0, r = i;       // ia: the smallest index with s[ia] >= s[i] - h (np.searchsorted left); s[i] itself qualifies
    while (l < r) { const int mid = (l + r) >> 1; if (s[mid] >= a) r = mid; else l = mid + 1; }
    const int ia = l;
    l = i; r = M - 1;       // ib: the largest index with s[ib] <= s[i] + h (np.searchsorted right, less one); s[i] itself qualifies
    while (l < r) { const int mid = (l + r + 1) >> 1; if (s[mid] <= b) l = mid; else r = mid - 1; }
    const int ib = l;
    const double den = __dsub_rn(s[ib], s[ia]);
    k.kappa[g] = den > 0.0 ? __ddiv_rn(plan_fix_heading(__dsub_rn(psi[ib], psi[ia])), den) : 0.0;
}

// a refused vehicle: v_plan 0, info row 0, closest -1
DEV void plan_refuse(const SPF &w, const int b, const int lane)
{
    if (w.info && lane < 4) w.info[4 * (size_t)b + lane] = 0.0;
    if (lane == 0) {
        w.v_plan[b] = 0.0;
        if (w.closest) w.closest[b] = -1;
    }
}

// v_lim^2 of one sample: min(vcap2, A_LAT / max(|kappa|, 1e-9)) by compare-and-select, so that a NaN table entry reaches w (fmin / fmax would swallow it)
DEV double plan_limit(const double kap, const double a_lat, const double vcap2)
{
    const double ak = fabs(kap);
    const double q = __ddiv_rn(a_lat, ak < 1e-9 ? 1e-9 : ak);
    return vcap2 < q ? vcap2 : q;
}

// the same with a map: a_j = A_LAT * MU_SCALE_j, lim_j = min(vcap2, a_j / max(|kappa_j|, 1e-9), V_LIMIT_j^2), each rounded once.  The second select
// would swallow a NaN of the first (mu, kappa), so `nan` collects the NaNs of both operands: the caller ors it into saw_nan
DEV double plan_limit_profile(const double kap, const double *prow, const double a_lat, const double vcap2, bool &nan)
{
    const double vl = prow[KMPC_PROFILE_V_LIMIT];
    const double m = plan_limit(kap, __dmul_rn(a_lat, prow[KMPC_PROFILE_MU_SCALE]), vcap2), vl2 = __dmul_rn(vl, vl);
    nan |= m != m || vl2 != vl2;
    return m < vl2 ? m : vl2;
}

template <bool PROFILE> __global__ __launch_bounds__(64) void kmpc_speed_plan_fleet_kernel(SPF w)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= w.B) return;
    const int pid = __builtin_amdgcn_readfirstlane(w.path_id[b]);
    const double *st = w.state + (size_t)b * w.stride, *row = w.rows + KMPC_PLAN_WORDS * (size_t)b;
    const double x = uniform_(st[0]), y = uniform_(st[1]), vcap = uniform_(w.v_cap[b]);
    const double a_lat = uniform_(row[KMPC_PLAN_A_LAT]), a_brake = uniform_(row[KMPC_PLAN_A_BRAKE]), v_floor = uniform_(row[KMPC_PLAN_V_FLOOR]);
    const double end_stop = uniform_(row[KMPC_PLAN_END_STOP]);
    // no table entry and no sample is read for a bad path_id, nor for a bad pose, cap or row
    const bool ok = (unsigned)pid < (unsigned)w.P && stage::finite(x) && stage::finite(y) && stage::finite(vcap) && vcap >= 0.0 && a_lat > 0.0 &&
                    a_brake > 0.0 && stage::finite(a_brake) && v_floor >= 0.0 && stage::finite(v_floor) && end_stop == end_stop;
    if (!ok) { plan_refuse(w, b, lane); return; }
    const int o0 = __builtin_amdgcn_readfirstlane(w.off[pid]), o1 = __builtin_amdgcn_readfirstlane(w.off[pid + 1]);
    const int M = o1 - o0;
    const size_t n = (size_t)w.total;
    const double *seg = w.d + o0;                                    // d = t | X | Y | psi | s
    const double *s = seg + 4 * n, *kappa = w.kappa + o0;            // indices 0 .. M-1 of the vehicle's own path
    const double *prof = nullptr;                                    // the map's rows of the vehicle's own path
    if constexpr (PROFILE) prof = w.profile + KMPC_PROFILE_WORDS * (size_t)o0;
    const int i = nearest_sample(seg + n, seg + 2 * n, M, x, y, lane);
    const double s_i = s[i], vcap2 = __dmul_rn(vcap, vcap), two_a = __dmul_rn(2.0, a_brake);
    const bool stop_at_end = end_stop != 0.0;
    // wmin, the wave's minimum so far, is wave-uniform and lives in scalar registers; it is not read before the first chunk has set it (i < M: there
    // is a first chunk), so it starts at 0, an inline constant -- this toolchain encodes a scalar 64-bit move of +inf's bit pattern as a move of 0
    double best = INFINITY, wmin = 0.0;
    int bj = 0x7fffffff;
    bool saw_nan = false;
    for (int base = i; base < M; base += 64) {
        // the exact early exit: every later c_j >= its own braking term >= this one (s non-decreasing, limits >= 0, rounding monotone)
        if (base != i && __dmul_rn(two_a, __dsub_rn(s[base], s_i)) >= wmin) break;
        const int j = base + lane;
        if (j < M) {
            double lim;
            if constexpr (PROFILE) lim = plan_limit_profile(kappa[j], prof + KMPC_PROFILE_WORDS * (size_t)j, a_lat, vcap2, saw_nan);
            else lim = plan_limit(kappa[j], a_lat, vcap2);
            if (stop_at_end && j == M - 1) lim = 0.0;
            const double c = __dadd_rn(lim, __dmul_rn(two_a, __dsub_rn(s[j], s_i)));
            saw_nan |= c != c;
            if (c < best) { best = c; bj = j; }
        }
        wmin = dpp_min(best);
    }
    const double cand = (best == wmin) ? (double)bj : 1e18;
    int jb = (int)dpp_min(cand);
    jb = (jb >= i && jb < M) ? jb : i;                               // never an index outside the path arrays
    const bool any_nan = __builtin_amdgcn_ballot_w64(saw_nan) != 0;
    double lim_i;
    if constexpr (PROFILE) lim_i = plan_limit_profile(kappa[i], prof + KMPC_PROFILE_WORDS * (size_t)i, a_lat, vcap2, saw_nan);   // sample i was visited: no new NaN
    else lim_i = plan_limit(kappa[i], a_lat, vcap2);
    if (stop_at_end && i == M - 1) lim_i = 0.0;
    const double d_bind = __dsub_rn(s[jb], s_i), kappa_bind = kappa[jb], v_here = __dsqrt_rn(lim_i);
    // an unlimited vehicle's speed is v_cap itself, bit for bit, whatever the device's sqrt
    double v = vcap;
    if (!(wmin == vcap2)) {
        v = __dsqrt_rn(wmin);
        v = v_floor > v ? v_floor : v;
        v = vcap < v ? vcap : v;
    }
    // every word written is finite: a non-finite w (an overflowing cap with no cornering limit, a NaN table entry or sample) refuses the vehicle
    if (any_nan || !(stage::finite(wmin) && stage::finite(v) && stage::finite(d_bind) && stage::finite(kappa_bind) && stage::finite(v_here))) {
        plan_refuse(w, b, lane);
        return;
    }
    if (w.info && lane < 4) w.info[4 * (size_t)b + lane] = lane == 0 ? wmin : (lane == 1 ? d_bind : (lane == 2 ? kappa_bind : v_here));
    if (lane == 0) {
        w.v_plan[b] = v;
        if (w.closest) w.closest[b] = i;
    }
}

hipError_t kmpc_launch_curvature(const SPC &k, hipStream_t st)
{
    return kmpc_launch(kmpc_curvature_kernel, dim3((unsigned)(((size_t)k.total + 255) / 256)), dim3(256), 0, st, k);
}

hipError_t kmpc_launch_speed_plan_fleet(const SPF &w, hipStream_t st)
{
    return w.profile ? kmpc_launch(kmpc_speed_plan_fleet_kernel<true>, dim3(w.B), dim3(64), 0, st, w)
                     : kmpc_launch(kmpc_speed_plan_fleet_kernel<false>, dim3(w.B), dim3(64), 0, st, w);
}
