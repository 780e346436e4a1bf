// kmpc_waypoints.hip -- batched look-ahead waypoint generation on gfx950.
//
// Replaces, for B vehicles at once, GPSRefTrajectory.get_waypoints of the reference
// (scripts/gps_utils/ref_gps_traj.py:131-142, 172-218): nearest recorded point to (x, y) over the
// whole path, N+1 linearly interpolated waypoints on the arclength grid (target-velocity mode,
// starting ONE step ahead, :175) or on the time grid (starting at the closest point, :191), heading
// wrap-around fix against the current yaw (:204-218) and the end-of-path stop flag (:182-184).
//
// One wavefront per vehicle.  The path (t, X, Y, psi, cumulative distance; ~6.7k samples, 270 KB)
// is shared by every vehicle and stays L2 / Infinity-Cache resident; the nearest-point pass streams
// it with coalesced 8-byte loads (lane l reads samples l, l+64, ...), i.e. 107 KB of L2 reads per
// vehicle and no HBM traffic beyond the first touch -- the kernel is L2-bandwidth bound.
// Arithmetic mirrors numpy exactly (no FMA contraction in the distance and in np.interp's
// slope*(x - xp[j]) + fp[j]) so that indices match bit for bit and values to the last ulp.
//
// Two kernels share one per-vehicle body: kmpc_waypoints_kernel (one path and one mode per launch) and kmpc_waypoints_fleet_kernel (a path and a
// mode per vehicle, out of a set of paths held in one allocation).
#include "kmpc_common.h"
#include "kmpc_dispatch.h"
#include "kmpc_interp.h"   // np_interp
#include "kmpc_nearest.h"  // nearest_sample

// one recorded path as the body sees it: five arrays of M samples
struct PathView {
    const double *t, *X, *Y, *psi, *s;
    int M;
};

// One vehicle on one path, by one wavefront: shared by kmpc_waypoints_kernel (the launch's path and mode) and kmpc_waypoints_fleet_kernel (the
// vehicle's own).  `pv` and `use_vtarget` are wave-uniform; vt is read only with use_vtarget.
DEV void waypoints_vehicle(const PathView &pv, const int use_vtarget, const int b, const int lane, const int H, const double traj_dt,
                           const double *pose, const double *vt, double *ref, int32_t *stop, int32_t *closest_out)
{
    const double x = pose[3 * (size_t)b], y = pose[3 * (size_t)b + 1], yaw = pose[3 * (size_t)b + 2];
    // ---- closest recorded point: argmin (X-x)^2 + (Y-y)^2, first occurrence (np.argmin) ---------
    const int closest = nearest_sample(pv.X, pv.Y, pv.M, x, y, lane);   // kmpc_nearest.h: shared with the speed plan
    // ---- look-ahead grid ---------------------------------------------------------------------------
    const int k = lane;
    const bool act = k <= H;
    const double *grid = use_vtarget ? pv.s : pv.t;
    const double start = grid[closest];
    double q;
    if (use_vtarget) q = __dadd_rn(__dmul_rn(__dmul_rn((double)(k + 1), traj_dt), vt[b]), start);  // x*dt*v + start, x = 1..H+1
    else q = __dadd_rn(__dmul_rn((double)k, traj_dt), start);                                      // h*dt + start, h = 0..H
    double xi = 0, yi = 0, pi_ = 0;
    if (act) {
        xi = np_interp(q, grid, pv.X, pv.M);
        yi = np_interp(q, grid, pv.Y, pv.M);
        pi_ = np_interp(q, grid, pv.psi, pv.M);
    }
    // ---- heading wrap-around fix (:204-218) -------------------------------------------------------------
    const double pnext = dpp_mov0<0x130, 0xf>(pi_);  // lane k+1
    const double dd = (k < H) ? fabs(__dsub_rn(pnext, pi_)) : 0.0;
    const double dc = act ? fabs(__dsub_rn(pi_, yaw)) : 0.0;
    const bool check1 = dpp_max(dd) < M_PI, check2 = dpp_max(dc) < M_PI;
    if (!(check1 && check2) && act) {
        const double c0 = pi_, c1 = __dadd_rn(pi_, 2.0 * M_PI), c2 = __dsub_rn(pi_, 2.0 * M_PI);
        const double e0 = fabs(__dsub_rn(c0, yaw)), e1 = fabs(__dsub_rn(c1, yaw)), e2 = fabs(__dsub_rn(c2, yaw));
        double bc = c0, be = e0;               // np.argmin: first minimal candidate in [p, p+2pi, p-2pi]
        if (e1 < be) { bc = c1; be = e1; }
        if (e2 < be) { bc = c2; be = e2; }
        pi_ = bc;
    }
    if (act) {
        double *o = ref + ((size_t)b * (H + 1) + k) * 3;
        o[0] = xi; o[1] = yi; o[2] = pi_;
    }
    if (k == H) stop[b] = (xi == pv.X[pv.M - 1] && yi == pv.Y[pv.M - 1]) ? 1 : 0;  // :182-184, the last sample of the vehicle's own path
    if (lane == 0 && closest_out) closest_out[b] = closest;
}

__global__ __launch_bounds__(64) void kmpc_waypoints_kernel(WP w)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= w.B) return;
    const PathView pv = {w.t, w.X, w.Y, w.psi, w.s, w.M};
    waypoints_vehicle(pv, w.use_vtarget, b, lane, w.H, w.traj_dt, w.pose, w.vt, w.ref, w.stop, w.closest);
}

// A fleet on P recorded paths (the reference ships three, the .mat files under paths/, and pairs each with its own start pose in launch/sim_path_follow.launch:13,22-30):
// vehicle b follows path path_id[b], on the time grid if time_mode[b] != 0 (ref_gps_traj.py:191) and on the arclength grid at v_target[b] otherwise (:175).
// Both are wave-uniform, read once and made scalar, so the segment's base pointers, its sample count and the grid selection live in SGPRs and the argmin
// loop bound and the mode branch are scalar; from there on the vehicle runs waypoints_vehicle on a view of its own segment and reads nothing outside it.
// A path_id outside [0, P) is contained: stop 1 (the loop brakes the vehicle), closest -1, every waypoint row the vehicle's own pose with non-finite
// components replaced by 0; no table entry and no path sample is read for it.
__global__ __launch_bounds__(64) void kmpc_waypoints_fleet_kernel(WPF w)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= w.B) return;
    const int pid = __builtin_amdgcn_readfirstlane(w.path_id[b]);
    if ((unsigned)pid >= (unsigned)w.P) {
        if (lane <= w.H) {
            double *o = w.ref + ((size_t)b * (w.H + 1) + lane) * 3;
            for (int c = 0; c < 3; ++c) {
                const double v = w.pose[3 * (size_t)b + c];
                o[c] = isfinite(v) ? v : 0.0;
            }
        }
        if (lane == 0) {
            w.stop[b] = 1;
            if (w.closest) w.closest[b] = -1;
        }
        return;
    }
    const int o0 = __builtin_amdgcn_readfirstlane(w.off[pid]), o1 = __builtin_amdgcn_readfirstlane(w.off[pid + 1]);
    const bool time_mode = w.time_mode ? __builtin_amdgcn_readfirstlane((int)w.time_mode[b]) != 0 : w.all_time != 0;
    const double *seg = w.d + o0;
    const size_t n = (size_t)w.total;
    const PathView pv = {seg, seg + n, seg + 2 * n, seg + 3 * n, seg + 4 * n, o1 - o0};
    waypoints_vehicle(pv, time_mode ? 0 : 1, b, lane, w.H, w.traj_dt, w.pose, w.vt, w.ref, w.stop, w.closest);
}

hipError_t kmpc_launch_waypoints(const WP &w, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_waypoints_kernel, dim3(w.B), dim3(64), 0, st, w);
    return hipGetLastError();
}

hipError_t kmpc_launch_waypoints_fleet(const WPF &w, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_waypoints_fleet_kernel, dim3(w.B), dim3(64), 0, st, w);
    return hipGetLastError();
}
