// kmpc_track_score.hip -- batched tracking errors on the recorded paths and a running score record per vehicle, on gfx950.
//
// Replaces, for B vehicles at once and on the device, the numerical part of the reference's scripts/analysis/plot_path_tracking_error.py:
// compute_path_errors (:21-34: nearest recorded sample and the distance to it, `error_xy`) and the yaw error there through fix_heading
// (:36-43, :161); and what the tests compute on the host from downloaded histories (the distance to the POLYLINE through the samples and the
// settle time, largest command steps, live periods and latch period of a closed-loop run).
//
// One wavefront per vehicle, as in kmpc_waypoints.hip.  Lane l visits samples l, l + 64, ... ONCE; in that pass it keeps
//   - the nearest sample with the arithmetic of waypoints_vehicle (no FMA contraction, first occurrence): `closest` is bit-identical to
//     kmpc_waypoints_batch's closest_out;
//   - the nearest point of segment i -> i + 1 (i <= M - 2): w = p - P_i, d = P_{i+1} - P_i, s = clamp(w.d / max(|d|^2, 1e-18), 0, 1),
//     e^2 = |w - s d|^2 (contraction allowed: compared at a tolerance).  P_{i+1} comes from a second load of the same lines, not from the
//     neighbouring lane: a second load has no lane-63 / next-trip case.  Measured at B = 4096: 1.22 x the fleet waypoint call;
//     whether the division or the loads set that time has not been measured.
// Both minima are reduced over the wave with the index as payload (dpp_min of the value, then dpp_min of the index among the equal lanes), the
// winning segment is evaluated once more by every lane (wave-uniform addresses) for the signed distance and the arclength, and lanes 0..15
// update one word each of the vehicle's 128-byte score record (layout: include/kmpc.h).
//
// Two kernels share the per-vehicle body: kmpc_track_score_kernel (one path per launch) and kmpc_track_score_fleet_kernel (path_id[b] out of a
// set of paths; wave-uniform, read once and made scalar, so the base pointers, M and the loop bound live in SGPRs).
#include "../../include/kmpc.h"   // KMPC_SCORE_*: the record layout; KMPC_OPTIMAL
#include "kmpc_common.h"
#include "kmpc_dispatch.h"

// one recorded path as the body sees it (no time stamps: the score does not read them)
struct ScorePath {
    const double *X, *Y, *psi, *s;
    int M;
};

// nearest point of the segment P0 -> P1 to (x, y): squared distance; *s_out the clamped parameter, *cross_out = d x w (> 0: left of the direction of travel)
DEV double segment_dist2(const double x, const double y, const double X0, const double Y0, const double X1, const double Y1, double *s_out, double *cross_out)
{
    const double wx = x - X0, wy = y - Y0, dx = X1 - X0, dy = Y1 - Y0;
    const double L2 = fmax(dx * dx + dy * dy, 1e-18);   // a repeated sample: s = 0, the distance to the sample
    const double s = fmin(fmax((wx * dx + wy * dy) / L2, 0.0), 1.0);
    const double ex = wx - s * dx, ey = wy - s * dy;
    *s_out = s;
    *cross_out = dx * wy - dy * wx;
    return ex * ex + ey * ey;
}

// a refused state: err row 0, seg = closest = -1, only the refused count of the record moves
DEV void score_refuse(const TS &w, const int b, const int lane)
{
    if (w.err && lane < 4) w.err[4 * (size_t)b + lane] = 0.0;
    if (lane == 0) {
        if (w.seg) w.seg[b] = -1;
        if (w.closest) w.closest[b] = -1;
    }
    if (w.score && lane == KMPC_SCORE_N_REFUSED) {
        double *r = w.score + KMPC_SCORE_WORDS * (size_t)b + lane;
        const double old = *r;
        *r = isfinite(old) ? old + 1.0 : 1.0;
    }
}

// One vehicle on one path, by one wavefront.  `pv` is wave-uniform.
DEV void score_vehicle(const ScorePath &pv, const TS &w, const int b, const int lane)
{
    const double *st = w.state + (size_t)b * w.stride;
    const double x = uniform_(st[0]), y = uniform_(st[1]), yaw = uniform_(st[2]);
    if (!(isfinite(x) && isfinite(y) && isfinite(yaw))) { score_refuse(w, b, lane); return; }
    // ---- one pass over X and Y: nearest sample (waypoints_vehicle's arithmetic) and nearest point of the polyline ----------------------
    double best = INFINITY, ebest = INFINITY;
    int bi = 0x7fffffff, ei = 0x7fffffff;
    for (int i = lane; i < pv.M; i += 64) {
        const double Xi = pv.X[i], Yi = pv.Y[i];
        const double dx = __dsub_rn(Xi, x), dy = __dsub_rn(Yi, y);
        const double d = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
        if (d < best) { best = d; bi = i; }
        if (i + 1 < pv.M) {   // segment i -> i + 1
            double s_, c_;
            const double e2 = segment_dist2(x, y, Xi, Yi, pv.X[i + 1], pv.Y[i + 1], &s_, &c_);
            if (e2 < ebest) { ebest = e2; ei = i; }
        }
    }
    const double dmin = dpp_min(best);
    const double cand = (best == dmin) ? (double)bi : 1e18;
    int closest = (int)dpp_min(cand);
    closest = (unsigned)closest < (unsigned)pv.M ? closest : 0;         // never an index outside the path arrays (non-finite samples)
    const double emin = dpp_min(ebest);
    const double ecand = (ebest == emin) ? (double)ei : 1e18;
    int seg = (int)dpp_min(ecand);
    seg = (unsigned)seg < (unsigned)(pv.M - 1) ? seg : 0;               // 0 <= seg <= M - 2
    // ---- the winning segment once more, by every lane: signed distance and arclength -------------------------------------------------------
    double s, cross;
    const double e2 = segment_dist2(x, y, pv.X[seg], pv.Y[seg], pv.X[seg + 1], pv.Y[seg + 1], &s, &cross);
    const double e = sqrt(e2);
    const double e_ct = cross >= 0.0 ? e : -e;                          // sign of d x w: positive to the left of the direction of travel
    const double e_near = sqrt(dmin);                                   // error_xy of compute_path_errors (:30-32)
    const double s0 = pv.s[seg];
    const double s_along = s0 + s * (pv.s[seg + 1] - s0);
    // fix_heading (:36-43) of psi_path[closest] - psi: the first of p, p + 2 pi, p - 2 pi of smallest magnitude
    const double p0 = __dsub_rn(pv.psi[closest], yaw), p1 = __dadd_rn(p0, 2.0 * M_PI), p2 = __dsub_rn(p0, 2.0 * M_PI);
    double e_psi = p0;
    if (fabs(p1) < fabs(e_psi)) e_psi = p1;
    if (fabs(p2) < fabs(e_psi)) e_psi = p2;
    // ---- command side of the period (all four given, or none) ---------------------------------------------------------------------------------
    const bool has_cmd = w.cmd != nullptr;
    bool live = false;
    double acc = 0.0, df = 0.0, nonopt = 0.0, its = 0.0;
    if (has_cmd) {
        live = __builtin_amdgcn_readfirstlane((int)w.latch[b]) == 0;
        if (live) {
            acc = uniform_(w.cmd[2 * (size_t)b]); df = uniform_(w.cmd[2 * (size_t)b + 1]);
            nonopt = __builtin_amdgcn_readfirstlane(w.status[b]) != KMPC_OPTIMAL ? 1.0 : 0.0;
            its = (double)__builtin_amdgcn_readfirstlane(w.iters[b]);
        }
    }
    // every word written is finite: non-finite path samples or a non-finite live command refuse the state
    if (!(isfinite(e_ct) && isfinite(e_near) && isfinite(s_along) && isfinite(e_psi) && isfinite(acc) && isfinite(df))) { score_refuse(w, b, lane); return; }
    if (w.err && lane < 4) w.err[4 * (size_t)b + lane] = lane == 0 ? e_ct : (lane == 1 ? e_near : (lane == 2 ? e_psi : s_along));
    if (lane == 0) {
        if (w.seg) w.seg[b] = seg;
        if (w.closest) w.closest[b] = closest;
    }
    if (!w.score) return;
    // ---- the running record: lanes 0..15 own one word each --------------------------------------------------------------------------------------
    double *rec = w.score + KMPC_SCORE_WORDS * (size_t)b;
    double old = lane < KMPC_SCORE_WORDS ? rec[lane] : 0.0;
    if (!isfinite(old)) old = lane == KMPC_SCORE_LATCH_INDEX ? -1.0 : 0.0;   // a record nobody initialised starts fresh, word by word
    const double n = readlane_(old, KMPC_SCORE_N), n_live = readlane_(old, KMPC_SCORE_N_LIVE);
    const double last_acc = readlane_(old, KMPC_SCORE_LAST_ACC), last_df = readlane_(old, KMPC_SCORE_LAST_DF);
    const double a_ct = fabs(e_ct), a_psi = fabs(e_psi);
    double v = old;
    switch (lane) {
    case KMPC_SCORE_N: v = old + 1.0; break;
    case KMPC_SCORE_SUM_ECT2: v = old + e_ct * e_ct; break;
    case KMPC_SCORE_MAX_ECT: v = fmax(old, a_ct); break;
    case KMPC_SCORE_SUM_EPSI2: v = old + e_psi * e_psi; break;
    case KMPC_SCORE_MAX_EPSI: v = fmax(old, a_psi); break;
    case KMPC_SCORE_MAX_ENEAR: v = fmax(old, e_near); break;
    case KMPC_SCORE_SETTLE_INDEX: v = a_ct >= w.settle_tol ? n + 1.0 : old; break;   // this state's index is n
    default: break;
    }
    if (has_cmd && live) {
        switch (lane) {
        case KMPC_SCORE_N_LIVE: v = old + 1.0; break;
        case KMPC_SCORE_N_NONOPT: v = old + nonopt; break;
        case KMPC_SCORE_SUM_ITERS: v = old + its; break;
        case KMPC_SCORE_MAX_DACC: v = fmax(old, fabs(acc - last_acc)); break;
        case KMPC_SCORE_MAX_DDF: v = fmax(old, fabs(df - last_df)); break;
        case KMPC_SCORE_LAST_ACC: v = acc; break;
        case KMPC_SCORE_LAST_DF: v = df; break;
        default: break;
        }
    } else if (has_cmd && lane == KMPC_SCORE_LATCH_INDEX && old < 0.0) {
        v = n_live;   // the latch came up: live periods scored before it
    }
    if (lane < KMPC_SCORE_WORDS) rec[lane] = v;
}

__global__ __launch_bounds__(64) void kmpc_track_score_kernel(TSB k)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= k.w.B) return;
    const ScorePath pv = {k.X, k.Y, k.psi, k.s, k.M};
    score_vehicle(pv, k.w, b, lane);
}

// A path_id outside [0, P) is a refused state: no table entry and no path sample is read for it.
__global__ __launch_bounds__(64) void kmpc_track_score_fleet_kernel(TSF k)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= k.w.B) return;
    const int pid = __builtin_amdgcn_readfirstlane(k.path_id[b]);
    if ((unsigned)pid >= (unsigned)k.P) { score_refuse(k.w, b, lane); return; }
    const int o0 = __builtin_amdgcn_readfirstlane(k.off[pid]), o1 = __builtin_amdgcn_readfirstlane(k.off[pid + 1]);
    const double *seg = k.d + o0;
    const size_t n = (size_t)k.total;
    const ScorePath pv = {seg + n, seg + 2 * n, seg + 3 * n, seg + 4 * n, o1 - o0};   // d = t | X | Y | psi | s
    score_vehicle(pv, k.w, b, lane);
}

hipError_t kmpc_launch_track_score(const TSB &k, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_track_score_kernel, dim3(k.w.B), dim3(64), 0, st, k);
    return hipGetLastError();
}

hipError_t kmpc_launch_track_score_fleet(const TSF &k, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_track_score_fleet_kernel, dim3(k.w.B), dim3(64), 0, st, k);
    return hipGetLastError();
}
