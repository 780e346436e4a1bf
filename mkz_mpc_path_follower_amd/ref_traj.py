"""Mirror of the reference's waypoint helper scripts/gps_utils/ref_gps_traj.py (GPSRefTrajectory).

Same constructor data flow (load the recorded path, project lat/lon to the local XY frame, build
the cumulative arclength -- ref_gps_traj.py:33-52, 87-106) and the same
`get_waypoints(X_init, Y_init, yaw_init, v_target=None)` call (:131-142), but the rosparams
(lat0, lon0, yaw0, is_heading_info) are constructor arguments (defaults: launch/path_follow.launch:15-21)
and the look-ahead itself runs on the MI355X for B vehicles at once (kmpc_waypoints_batch);
`get_waypoints` is the B = 1 case.  FleetRefTrajectory holds several recorded paths and gives every vehicle
a path and a tracking mode of its own (kmpc_waypoints_fleet).  No CPU fallback.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._stage import (cap_in, cap_out, check_present, default_row, device_of, fresh_record, host_rows, is_buffer, own_path_id, ptr, record_fields,
                     rows_of, state_view, stream, table_rows)

LAT0, LON0, YAW0 = 37.917929, -122.331798, 0.0  # launch/path_follow.launch:19-21


def latlon_to_XY(lat0, lon0, lat1, lon1):
    """equirectangular projection, ref_gps_traj.py:33-52 (vectorised)"""
    R_earth = 6371000.0
    delta_lat = np.radians(lat1 - lat0)
    delta_lon = np.radians(lon1 - lon0)
    lat_avg = 0.5 * (np.radians(lat1) + np.radians(lat0))
    return R_earth * delta_lon * np.cos(lat_avg), R_earth * delta_lat


def path_arrays(tms, lats, lons, yaws, lat0=LAT0, lon0=LON0):
    """columns of GPSRefTrajectory.trajectory (:106): t, lat, lon, yaw, X, Y, cdist"""
    tms, lats, lons, yaws = (np.ravel(np.asarray(a, dtype=np.float64)) for a in (tms, lats, lons, yaws))
    X, Y = latlon_to_XY(lat0, lon0, lats, lons)
    # :95-100  s_0 = 0, s_i = s_{i-1} + dist(z_i, z_{i-1})  (sequential sum, as in the reference's loop)
    step = np.sqrt((X[1:] - X[:-1]) ** 2 + (Y[1:] - Y[:-1]) ** 2)
    cd = np.zeros_like(X)
    acc = 0.0
    for i, d in enumerate(step):
        acc = d + acc
        cd[i + 1] = acc
    return tms, lats, lons, yaws, X, Y, cd


SCORE_WORDS = 16
SCORE_FIELDS = ("n", "sum_ect2", "max_ect", "sum_epsi2", "max_epsi", "max_enear", "settle_index", "n_refused",
                "n_live", "n_nonopt", "sum_iters", "max_dacc", "max_ddf", "last_acc", "last_df", "latch_index")   # KMPC_SCORE_* of include/kmpc.h, in order


def fresh_score(B, device):
    """[B,16] float64 on `device`: B fresh score records (kmpc_track_score_init: zeros, latch index -1)"""
    return fresh_record("kmpc_track_score_init", B, SCORE_WORDS, device)


def _track_score(lib, entry, handle, device, B_fixed, path_id, state, score, status, iters, cmd, stop_latch, settle_tol, out):
    """argument marshalling shared by GPSRefTrajectory.track_score_batch and FleetRefTrajectory.track_score_batch"""
    st = state_view(state, 3, device, None, "state: expected [B,W] with X, Y, psi in the first three columns, got %s")
    B = st.shape[0]
    if B_fixed is not None and B != B_fixed:
        raise ValueError("state: expected %d rows, got %d" % (B_fixed, B))
    given = [a is not None for a in (status, iters, cmd, stop_latch)]
    if any(given) and not all(given):
        raise ValueError("status, iters, cmd and stop_latch are given all together or not at all")

    def buf(t, shape, dtypes, name):
        if t is None:
            return None
        if not is_buffer(t, dtypes, shape, device):
            raise ValueError("%s: expected a contiguous %s tensor %s on %s" % (name, dtypes[0], shape, device))
        return t
    status, iters = buf(status, (B,), (torch.int32,), "status"), buf(iters, (B,), (torch.int32,), "iters")
    cmd = buf(cmd, (B, 2), (torch.float64,), "cmd")
    stop_latch = buf(stop_latch, (B,), (torch.uint8, torch.bool), "stop_latch")
    score = buf(score, (B, SCORE_WORDS), (torch.float64,), "score")
    o = {} if out is None else out
    for k, shape, dt in (("err", (B, 4), torch.float64), ("seg", (B,), torch.int32), ("closest", (B,), torch.int32)):
        if buf(o.get(k), shape, (dt,), k) is None:
            o[k] = torch.empty(shape, dtype=dt, device=device)
    args = (handle, B, ptr(st), int(st.stride(0)) if B else 3) + (() if path_id is None else (ptr(path_id),)) + \
        (float(settle_tol), ptr(status), ptr(iters), ptr(cmd), ptr(stop_latch), ptr(o["err"]), ptr(o["seg"]), ptr(o["closest"]), ptr(score), stream(device))
    _lib.check(entry(*args))
    return o


class GPSRefTrajectory:
    def __init__(self, mat_filename=None, traj_horizon=8, traj_dt=0.2, lat0=LAT0, lon0=LON0, yaw0=YAW0,
                 use_heading=False, arrays=None, device=0):
        if mat_filename is None and arrays is None:
            raise ValueError("Invalid matfile specified.")  # :68-69
        if use_heading:
            raise NotImplementedError("is_heading_info=True is read but never used by the reference (:75)")
        self.traj_horizon, self.traj_dt = int(traj_horizon), float(traj_dt)  # :77-78
        if arrays is None:
            import scipy.io as sio
            dd = sio.loadmat(mat_filename)  # :88
            arrays = dict(t=dd["t"], lat=dd["lat"], lon=dd["lon"], psi=dd["psi"])
        t, lat, lon, psi, X, Y, cd = path_arrays(arrays["t"], arrays["lat"], arrays["lon"], arrays["psi"], lat0, lon0)
        self.trajectory = np.column_stack((t, lat, lon, psi, X, Y, cd))  # :106
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("GPSRefTrajectory needs an MI355X; no CPU fallback")
        self.device = torch.device("cuda", device)
        h = C.c_void_p()
        cols = [np.ascontiguousarray(self.trajectory[:, i]) for i in (0, 4, 5, 3, 6)]
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        _lib.check(self._lib.kmpc_path_create(int(device), len(t), dp(cols[0]), dp(cols[1]), dp(cols[2]), dp(cols[3]),
                                              dp(cols[4]), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.kmpc_path_destroy(self._h)
            self._h = None

    __del__ = close

    def get_global_trajectory_reference(self): return self.trajectory  # :116-117
    def get_Xs(self): return self.trajectory[:, 4]
    def get_Ys(self): return self.trajectory[:, 5]
    def get_psis(self): return self.trajectory[:, 3]

    def get_waypoints_batch(self, pose, v_target=None, want_closest=False):
        """pose [B,3] (X_init, Y_init, yaw_init), v_target [B] or None -> ref [B,H+1,3] (device), stop [B] int32"""
        pose = torch.as_tensor(pose, dtype=torch.float64, device=self.device).contiguous()
        if pose.dim() != 2 or pose.shape[1] != 3:
            raise ValueError("pose: expected [B,3], got %s" % (tuple(pose.shape),))
        B = pose.shape[0]
        vt = None if v_target is None else torch.as_tensor(v_target, dtype=torch.float64, device=self.device).contiguous()
        if vt is not None and tuple(vt.shape) != (B,):
            raise ValueError("v_target: expected [%d], got %s" % (B, tuple(vt.shape)))
        ref = torch.empty((B, self.traj_horizon + 1, 3), dtype=torch.float64, device=self.device)
        stop = torch.empty((B,), dtype=torch.int32, device=self.device)
        closest = torch.empty((B,), dtype=torch.int32, device=self.device) if want_closest else None
        rc = self._lib.kmpc_waypoints_batch(self._h, B, self.traj_horizon, self.traj_dt, ptr(pose), ptr(vt), ptr(ref), ptr(stop), ptr(closest),
                                            stream(self.device))
        if rc != 0:
            raise _lib.KmpcError(self._lib.kmpc_path_last_error(self._h).decode())
        return (ref, stop, closest) if want_closest else (ref, stop)

    def track_score_batch(self, state, score=None, status=None, iters=None, cmd=None, stop_latch=None, settle_tol=0.5, out=None):
        """Tracking errors of B vehicles on this path and, with `score` [B,16] (fresh_score), the running record (kmpc_track_score_batch).
        state: device tensor [B,W], X, Y, psi first -- the plant's state [B,8] as it is (no copy) or a pose [B,3].  status, iters (int32 [B]),
        cmd [B,2], stop_latch (uint8 / bool [B]): the period's command side, all or none.  -> dict err [B,4] (e_ct, e_near, e_psi, s_along),
        seg [B], closest [B] (int32); `out` may carry these tensors from an earlier call.  Asynchronous on torch's current stream."""
        return _track_score(self._lib, self._lib.kmpc_track_score_batch, self._h, self.device, None, None, state, score, status, iters, cmd,
                            stop_latch, settle_tol, out)

    # :131-142 -- same signature and return tuple as the reference
    def get_waypoints(self, X_init, Y_init, yaw_init, v_target=None):
        ref, stop = self.get_waypoints_batch([[X_init, Y_init, yaw_init]], None if v_target is None else [v_target])
        r = ref[0].cpu().numpy()
        return r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy(), bool(stop[0].item())


class FleetRefTrajectory:
    """B vehicles on several recorded paths: vehicle b follows paths[path_id[b]], on the time grid (ref_gps_traj.py:191) if time_mode[b] != 0 and on
    the arclength grid at its own v_target[b] (:175) otherwise -- one kmpc_waypoints_fleet launch for the whole fleet.

    paths: a list of what GPSRefTrajectory takes for ONE path -- a .mat file name, or an `arrays` dict with t, lat, lon, psi and optionally lat0, lon0
    (the projection origin of that path; launch/path_follow.launch:19-20 by default).  trajectories[p] is path p's [M_p,7] array (:106).
    path_id (int32, [B]) and time_mode (uint8, [B], or None) are device tensors and public: the launch reads them as they are, so the caller may edit
    them in place between steps (re-route a vehicle, switch its mode).  time_mode = None mirrors GPSRefTrajectory: every vehicle in target-velocity
    mode when get_waypoints_batch is given v_target, every vehicle in time mode when it is not.
    A vehicle whose path_id is outside [0, len(paths)) is refused by the kernel: stop flag 1, closest index -1, every waypoint its own pose."""

    def __init__(self, paths, path_id, time_mode=None, traj_horizon=8, traj_dt=0.2, device=0):
        if not len(paths):
            raise ValueError("FleetRefTrajectory: at least one path")
        self.traj_horizon, self.traj_dt = int(traj_horizon), float(traj_dt)
        self.trajectories = []
        for src in paths:
            if isinstance(src, str):
                import scipy.io as sio
                dd = sio.loadmat(src)  # :88
                src = dict(t=dd["t"], lat=dd["lat"], lon=dd["lon"], psi=dd["psi"])
            cols = path_arrays(src["t"], src["lat"], src["lon"], src["psi"], float(src.get("lat0", LAT0)), float(src.get("lon0", LON0)))
            self.trajectories.append(np.column_stack(cols))  # :106
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("FleetRefTrajectory needs an MI355X; no CPU fallback")
        self.device = torch.device("cuda", device)
        self.path_id = torch.as_tensor(path_id, device=self.device).to(torch.int32).contiguous()
        if self.path_id.dim() != 1:
            raise ValueError("path_id: expected [B], got %s" % (tuple(self.path_id.shape),))
        self.time_mode = None
        if time_mode is not None:
            self.time_mode = torch.as_tensor(time_mode, device=self.device).to(torch.uint8).contiguous()
            if self.time_mode.shape != self.path_id.shape:
                raise ValueError("time_mode: expected %s, got %s" % (tuple(self.path_id.shape), tuple(self.time_mode.shape)))
        M = np.array([len(tr) for tr in self.trajectories], dtype=np.int32)
        cols = [np.ascontiguousarray(np.concatenate([tr[:, i] for tr in self.trajectories])) for i in (0, 4, 5, 3, 6)]
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        h = C.c_void_p()
        rc = self._lib.kmpc_pathset_create(int(device), len(M), M.ctypes.data_as(C.POINTER(C.c_int32)), dp(cols[0]), dp(cols[1]), dp(cols[2]),
                                           dp(cols[3]), dp(cols[4]), C.byref(h))
        if rc != 0:
            raise _lib.KmpcError(self._lib.kmpc_pathset_last_error(None).decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.kmpc_pathset_destroy(self._h)
            self._h = None

    __del__ = close

    def get_waypoints_batch(self, pose, v_target=None, want_closest=False):
        """pose [B,3], v_target [B] or None -> ref [B,H+1,3] (device), stop [B] int32 [, closest [B] int32: index within the vehicle's own path]"""
        pose = torch.as_tensor(pose, dtype=torch.float64, device=self.device).contiguous()
        B = self.path_id.shape[0]
        if tuple(pose.shape) != (B, 3):
            raise ValueError("pose: expected [%d,3], got %s" % (B, tuple(pose.shape)))
        vt = None if v_target is None else torch.as_tensor(v_target, dtype=torch.float64, device=self.device).contiguous()
        if vt is not None and tuple(vt.shape) != (B,):
            raise ValueError("v_target: expected [%d], got %s" % (B, tuple(vt.shape)))
        tm = self.time_mode
        if tm is not None:
            if vt is None:
                raise ValueError("a fleet with per-vehicle modes needs v_target (it is not read for the vehicles in time mode)")
            if not is_buffer(tm, torch.uint8, (B,), self.device):
                raise ValueError("time_mode must stay a contiguous uint8 tensor [%d] on %s (write into it in place)" % (B, self.device))
        # own_path_id's check, written out: every loop makes this call every period, and through the helper it measured 19.5 us against the
        # parent's 19.4 us per call at B = 4096 in both of two alternating runs (profiles/fleet_front_ab.txt)
        pid = self.path_id   # a plain attribute: what reaches the kernel is a raw pointer
        if not is_buffer(pid, torch.int32, (B,), self.device):
            raise ValueError("path_id must stay a contiguous int32 tensor [%d] on %s (write into it in place)" % (B, self.device))
        ref = torch.empty((B, self.traj_horizon + 1, 3), dtype=torch.float64, device=self.device)
        stop = torch.empty((B,), dtype=torch.int32, device=self.device)
        closest = torch.empty((B,), dtype=torch.int32, device=self.device) if want_closest else None
        rc = self._lib.kmpc_waypoints_fleet(self._h, B, self.traj_horizon, self.traj_dt, ptr(pose), ptr(pid), ptr(tm), ptr(vt), ptr(ref), ptr(stop),
                                            ptr(closest), stream(self.device))
        if rc != 0:
            raise _lib.KmpcError(self._lib.kmpc_pathset_last_error(self._h).decode())
        return (ref, stop, closest) if want_closest else (ref, stop)

    def track_score_batch(self, state, score=None, status=None, iters=None, cmd=None, stop_latch=None, settle_tol=0.5, out=None):
        """GPSRefTrajectory.track_score_batch for the fleet: vehicle b against paths[path_id[b]] (kmpc_track_score_fleet).  A vehicle whose
        path_id is outside the set, or whose X, Y or psi is not finite, is refused: err row 0, seg = closest = -1, only its refused count moves."""
        B = self.path_id.shape[0]
        pid = own_path_id(self.path_id, B, self.device)
        return _track_score(self._lib, self._lib.kmpc_track_score_fleet, self._h, self.device, B, pid, state, score, status, iters, cmd,
                            stop_latch, settle_tol, out)


PLAN_WORDS = 8
PLAN_FIELDS = ("a_lat", "a_brake", "v_floor", "end_stop")   # KMPC_PLAN_* words 0 ... 3 of include/kmpc.h, in row order (4 ... 7 are read by nobody)


def speed_plan_default():
    """the default plan row (2.0, 0.7, 1.0, 0, 0, 0, 0, 0) as a numpy row [8], from kmpc_speed_plan_default"""
    return default_row("kmpc_speed_plan_default", PLAN_WORDS)


def check_speed_plan_rows(rows):
    """[B,8] host rows -> ValueError unless a_lat > 0 (+inf: no cornering limit), a_brake > 0 and finite, v_floor >= 0 and finite and end_stop is
    not NaN.  The kernel refuses such a vehicle (v_plan 0) on its own; this says so where the rows are written."""
    rows = host_rows(rows)
    if rows.ndim != 2 or rows.shape[1] != PLAN_WORDS:
        raise ValueError("speed plan rows: [B,8] (%s, four unused words), got %s" % (", ".join(PLAN_FIELDS), rows.shape))
    with np.errstate(invalid="ignore"):
        ok = (rows[:, 0] > 0.0) & (rows[:, 1] > 0.0) & np.isfinite(rows[:, 1]) & (rows[:, 2] >= 0.0) & np.isfinite(rows[:, 2]) & ~np.isnan(rows[:, 3])
    if not ok.all():
        raise ValueError("speed plan rows: a_lat > 0 (+inf: no limit), a_brake > 0 and finite, v_floor >= 0 and finite, end_stop not NaN "
                         "(vehicle(s) %s)" % rows_of(~ok))
    return rows


def speed_plan_params(B, device=0, **overrides):
    """[B,8] float64 plan rows on `device`: the default row, with each override (`a_lat=`, `a_brake=`, `v_floor=`, `end_stop=`) a scalar or one
    value per vehicle.  Validated on the host (check_speed_plan_rows) before anything reaches the device."""
    return torch.as_tensor(check_speed_plan_rows(table_rows("speed_plan_params", PLAN_FIELDS, speed_plan_default(), B, overrides))).to(device_of(device))


class SpeedPlanner:
    """A curvature- and grip-limited target speed per vehicle of a FleetRefTrajectory (kmpc_pathset_curvature once, here; kmpc_speed_plan_fleet
    per call of plan()).  A one-path fleet covers the single-path case.

    kappa [sum M]: the curvature table of the fleet's paths at `window` m, a device tensor, in the order of fleet.trajectories.
    rows [B,8] (speed_plan_params): a public device tensor, read by every plan() as it is -- edit it in place between steps, like fleet.path_id.
    The vehicle's path is fleet.path_id[b] at the time of the call.  A vehicle the kernel refuses (include/kmpc.h) gets v_plan 0.
    profile: a vehicle_sim.RoadProfile built on the same fleet -- the MAP: the plan scales A_LAT by the sample's MU_SCALE and honours its V_LIMIT
    (kmpc_speed_plan_fleet_profile).  It is the planner's own table, not the plant's; without one plan() calls kmpc_speed_plan_fleet as before."""

    def __init__(self, fleet, window=4.0, rows=None, profile=None):
        if not isinstance(fleet, FleetRefTrajectory):
            raise ValueError("SpeedPlanner plans on a FleetRefTrajectory (a one-path fleet covers a single path); a %s is not one"
                             % type(fleet).__name__)
        window = float(window)
        if not (math.isfinite(window) and window > 0.0):
            raise ValueError("window: finite and > 0 [m], got %r" % (window,))
        self.fleet, self.window, self.device = fleet, window, fleet.device
        self.B = int(fleet.path_id.shape[0])
        self._lib = fleet._lib
        self.kappa = torch.empty((sum(len(tr) for tr in fleet.trajectories),), dtype=torch.float64, device=self.device)
        _lib.check(self._lib.kmpc_pathset_curvature(fleet._h, window, ptr(self.kappa), stream(self.device)))
        self.rows = speed_plan_params(self.B, self.device) if rows is None else rows
        self._check_rows()
        if profile is not None:
            from .vehicle_sim import RoadProfile
            if not (isinstance(profile, RoadProfile) and profile.fleet is fleet):
                raise ValueError("profile: a RoadProfile built on the planner's own fleet")
        self.profile = profile
        self.info = self.closest = None   # [B,4] (w, s_jb - s_i, kappa_jb, sqrt(lim_i)) and [B] of the last plan(want_info=True)

    def _check_rows(self):
        if not is_buffer(self.rows, torch.float64, (self.B, PLAN_WORDS), self.device):
            raise ValueError("rows must be a contiguous float64 tensor [%d,8] on %s (speed_plan_params; write into it in place)" % (self.B, self.device))

    def plan(self, state, v_cap, out=None, want_info=False):
        """state: device tensor [B,W], X and Y first (the plant's [B,8], an estimate [B,4], a pose [B,3]: no copy); v_cap [B] -> v_plan [B] (`out`
        or a new tensor).  want_info=True also fills self.info [B,4] and self.closest [B].  Asynchronous on torch's current stream."""
        dev, B = self.device, self.B
        st = state_view(state, 2, dev, B, "state: expected [%d,W] with X, Y in the first two columns, got %s")
        vc = cap_in(v_cap, B, dev)
        self._check_rows()
        pid = own_path_id(self.fleet.path_id, B, dev)
        out = cap_out(out, B, dev)
        if want_info and self.info is None:
            self.info = torch.empty((B, 4), dtype=torch.float64, device=dev)
            self.closest = torch.empty((B,), dtype=torch.int32, device=dev)
        tail = (ptr(st), int(st.stride(0)) if B else 2, ptr(pid), ptr(vc), ptr(self.rows), ptr(out), ptr(self.info) if want_info else None,
                ptr(self.closest) if want_info else None, stream(dev))
        if self.profile is not None:
            self.profile._own()
            _lib.check(self._lib.kmpc_speed_plan_fleet_profile(self.fleet._h, B, ptr(self.kappa), ptr(self.profile.table), *tail))
        else:
            _lib.check(self._lib.kmpc_speed_plan_fleet(self.fleet._h, B, ptr(self.kappa), *tail))
        return out


FOLLOW_WORDS, FOLLOW_STAT_WORDS = 8, 8
FOLLOW_FIELDS = ("d_min", "t_headway", "a_brake", "k_gap", "length")   # KMPC_FOLLOW_* words 0 ... 4 of include/kmpc_follow.h, in row order (5 ... 7 are read by nobody)
FOLLOW_STAT_FIELDS = ("n", "n_leader", "n_bound", "n_contact", "min_gap", "max_closing")   # KMPC_FOLLOWSTAT_* words 0 ... 5, in order


def follow_default():
    """the default following row (5.0, 1.0, 0.7, 0.5, 4.9, 0, 0, 0) as a numpy row [8], from kmpc_follow_default"""
    return default_row("kmpc_follow_default", FOLLOW_WORDS)


def check_follow_rows(rows):
    """[B,8] host rows -> ValueError unless words 0 ... 4 are finite, t_headway >= 0, a_brake > 0, k_gap >= 0 and length >= 0 (d_min: any finite
    value).  The kernel cannot refuse a row -- a bad word poisons that vehicle's own cap -- so this says so where the rows are written."""
    rows = host_rows(rows)
    if rows.ndim != 2 or rows.shape[1] != FOLLOW_WORDS:
        raise ValueError("follow rows: [B,8] (%s, three unused words), got %s" % (", ".join(FOLLOW_FIELDS), rows.shape))
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(rows[:, 0:5]).all(1) & (rows[:, 1] >= 0.0) & (rows[:, 2] > 0.0) & (rows[:, 3] >= 0.0) & (rows[:, 4] >= 0.0)
    if not ok.all():
        raise ValueError("follow rows: every word finite, t_headway >= 0, a_brake > 0, k_gap >= 0, length >= 0 (vehicle(s) %s)" % rows_of(~ok))
    return rows


def follow_params(B, device=0, **overrides):
    """[B,8] float64 following rows on `device`: the default row, with each override (`d_min=`, `t_headway=`, `a_brake=`, `k_gap=`, `length=`) a
    scalar or one value per vehicle.  Validated on the host (check_follow_rows) before anything reaches the device."""
    return torch.as_tensor(check_follow_rows(table_rows("follow_params", FOLLOW_FIELDS, follow_default(), B, overrides))).to(device_of(device))


def fresh_follow_stat(B, device):
    """[B,8] float64 on `device`: B fresh following records (kmpc_follow_stat_init: zeros, smallest gap +inf)"""
    return fresh_record("kmpc_follow_stat_init", B, FOLLOW_STAT_WORDS, device)


RANGE_WORDS, RANGE_REC_WORDS = 16, 16
RANGE_FIELDS = ("range_max", "sigma_r", "sigma_v", "bias_r", "p_drop", "filter", "coast_max", "q_gap", "q_v", "r_gap", "r_v")   # KMPC_RANGE_* words 0 ... 10 of include/kmpc_range.h, in row order (11 ... 15 are read by nobody)
RANGE_REC_FIELDS = ("gap_hat", "v_hat", "p00", "p01", "p11", "track_id", "coast", "n", "n_detect", "n_drop", "n_out", "n_new", "n_lost", "n_bound",
                    "sum_egap2", "max_egap")   # KMPC_RANGEREC_* words 0 ... 15, in order


def range_default():
    """the default sensor row, a plain automotive radar (120, 0.25, 0.12, 0, 0, 1, 5, 0.01, 0.25, 0.0625, 0.0144, 0 ...), as a numpy row [16], from
    kmpc_range_default"""
    return default_row("kmpc_range_default", RANGE_WORDS)


def range_neutral():
    """the neutral sensor row [16]: no range limit, no noise, no bias, no dropouts, no filter, no coasting -- behind kmpc_follow_fleet the stage
    then gives that kernel's own cap bit for bit.  The words the neutral stage does not read (Q_*, R_*) keep their defaults."""
    row = range_default()
    row[0:7] = (np.inf, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    return row


def check_range_rows(rows):
    """[B,16] host rows -> ValueError unless words 0 ... 10 are finite (range_max may be +inf), range_max > 0, both sigmas >= 0, 0 <= p_drop <= 1,
    filter is 0 or 1, coast_max is a whole number in 0 ... 1000, q_gap and q_v >= 0, r_gap and r_v > 0.  The kernel cannot refuse a row -- a bad
    word poisons that vehicle's own cap -- so this says so where the rows are written."""
    rows = host_rows(rows)
    if rows.ndim != 2 or rows.shape[1] != RANGE_WORDS:
        raise ValueError("range rows: [B,16] (%s, five unused words), got %s" % (", ".join(RANGE_FIELDS), rows.shape))
    with np.errstate(invalid="ignore"):
        ok = (np.isfinite(rows[:, 1:11]).all(1) & (rows[:, 0] > 0.0) & (rows[:, 1] >= 0.0) & (rows[:, 2] >= 0.0) & (rows[:, 4] >= 0.0)
              & (rows[:, 4] <= 1.0) & ((rows[:, 5] == 0.0) | (rows[:, 5] == 1.0)) & (rows[:, 6] == np.floor(rows[:, 6])) & (rows[:, 6] >= 0.0)
              & (rows[:, 6] <= 1000.0) & (rows[:, 7] >= 0.0) & (rows[:, 8] >= 0.0) & (rows[:, 9] > 0.0) & (rows[:, 10] > 0.0))
    if not ok.all():
        raise ValueError("range rows: every word finite (range_max may be +inf), range_max > 0, sigma_r and sigma_v >= 0, 0 <= p_drop <= 1, filter 0 "
                         "or 1, coast_max a whole number in 0 ... 1000, q_gap and q_v >= 0, r_gap and r_v > 0 (vehicle(s) %s)" % rows_of(~ok))
    return rows


def range_params(B, device=0, **overrides):
    """[B,16] float64 sensor rows on `device`: the default row, with each override (RANGE_FIELDS) a scalar or one value per vehicle.  Validated on
    the host (check_range_rows) before anything reaches the device."""
    return torch.as_tensor(check_range_rows(table_rows("range_params", RANGE_FIELDS, range_default(), B, overrides))).to(device_of(device))


def fresh_range_rec(B, device):
    """[B,16] float64 on `device`: B fresh track records (kmpc_range_rec_init: no track, zeros)"""
    return fresh_record("kmpc_range_rec_init", B, RANGE_REC_WORDS, device)


class RangeSensor:
    """A range sensor and a leader tracker per vehicle (kmpc_range_follow_batch, include/kmpc_range.h), for Follower(radar=): range limit, bias,
    seeded noise on range and on the leader's speed, dropouts, and a two-state Kalman track on (gap, leader speed) that coasts through dropouts.
    `seed`: the draws' key; vehicle b draws as vehicle id_base + b of period k, whatever B or the shard.

    rows [B,16] (range_params), rec [B,16] (RANGE_REC_FIELDS), meas [B,4] (z_r, z_v -- NaN when nothing was detected --, detected, coast of the
    last call): public device tensors, the first two read by every call as they are -- edit them in place between steps.  reset() starts the
    record afresh, summary() downloads it."""

    def __init__(self, B, device=0, rows=None, seed=0, id_base=0):
        self.B, self.device = int(B), device_of(device)
        self.seed, self.id_base = int(seed), int(id_base)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed: an integer in 0 ... 2^64 - 1")
        self.rows = range_params(self.B, self.device) if rows is None else rows
        self._check()
        self.meas = torch.zeros((self.B, 4), dtype=torch.float64, device=self.device)
        self.reset()

    def _check(self):
        if not is_buffer(self.rows, torch.float64, (self.B, RANGE_WORDS), self.device):
            raise ValueError("rows must be a contiguous float64 tensor [%d,16] on %s (range_params; write into it in place)" % (self.B, self.device))

    def reset(self):
        """a fresh record for every vehicle: no track"""
        self.rec = fresh_range_rec(self.B, self.device)

    def summary(self):
        """the record as named numpy fields [B] (one synchronising download): RANGE_REC_FIELDS, the track id, coast and the counts as integers"""
        return record_fields(self.rec, RANGE_REC_FIELDS, ("track_id", "coast", "n", "n_detect", "n_drop", "n_out", "n_new", "n_lost", "n_bound"))


SEARCHES = ("pairs", "sorted")


def check_search(search):
    """search= of Follower and Lanes: "pairs" (the exact pair search) or "sorted" (the search along the order, include/kmpc_order.h)"""
    if search not in SEARCHES:
        raise ValueError("search= must be one of %s, got %r" % (" / ".join(repr(s) for s in SEARCHES), search))
    return search


def order_buffers(lib, B, lanes_max, device):
    """what a sorted search owns, allocated once: order [B] int32, the usable count [1] int32, a workspace of kmpc_order_bytes(B, lanes_max)"""
    n = C.c_int64()
    _lib.check(lib.kmpc_order_bytes(int(B), int(lanes_max), C.byref(n)))
    return (torch.empty((B,), dtype=torch.int32, device=device), torch.zeros((1,), dtype=torch.int32, device=device),
            torch.empty((max(int(n.value), 1),), dtype=torch.uint8, device=device))


class _FleetSearch:
    """What Follower and Lanes share: the waypoint helper they stand on and the fleet's size, search= with the buffers of the sorted one, the
    geometry-only score call that places the vehicles, the kmpc_order_fleet call, and the `gap` / `leader_speed` views.  The two stages differ in
    the words of their refusals, which they pass in, and in their kernels: cap() and step() stay their own."""

    gap = property(lambda self: self.gap_leader[:, 0])
    leader_speed = property(lambda self: self.gap_leader[:, 1])

    def _init_helper(self, grt, name, verb, rows, makers):
        """grt: the helper; `name` and `verb`: "Follower", "follows" / "Lanes", "run", for the refusals.  On a GPSRefTrajectory (one path, no
        path_id) the first of `rows` that is a [B,W] tensor gives the fleet's size; `makers` names what builds such rows."""
        if not isinstance(grt, (FleetRefTrajectory, GPSRefTrajectory)):
            raise ValueError("%s %s on a GPSRefTrajectory or a FleetRefTrajectory; a %s is neither" % (name, verb, type(grt).__name__))
        self.fleet, self.device, self._lib = grt, grt.device, grt._lib
        self._one_path = isinstance(grt, GPSRefTrajectory)
        if self._one_path:
            given = [r for r in rows if isinstance(r, torch.Tensor) and r.dim() == 2]
            if not given:
                raise ValueError("%s on a GPSRefTrajectory: rows [B,8] (%s) are required, their length is the fleet's size" % (name, makers))
            self.B = int(given[0].shape[0])
        else:
            self.B = int(grt.path_id.shape[0])
        self._track = None                                                                  # the geometry-only score call's err, seg, closest
        self._on_path = torch.empty((self.B,), dtype=torch.bool, device=self.device)        # placed by the score call (and `present`, where given)

    def _init_search(self, search, lanes_max=0):
        """search=; `order` [B] int32, the count word and the workspace of the sorted one are allocated once, here"""
        self.search = check_search(search)
        if search == "sorted":
            self.order, self._count, self._ws = order_buffers(self._lib, self.B, lanes_max, self.device)

    def _path_id(self):
        """the helper's path_id as the kernels read it; None on a one-path helper"""
        return None if self._one_path else own_path_id(self.fleet.path_id, self.B, self.device)

    def _place(self, st, present):
        """one geometry-only track_score_batch call -> err [B,4] (e_ct, e_near, e_psi, s_along); a vehicle it refuses, or that `present` marks 0, is
        not on the road (self._on_path)"""
        self._track = self.fleet.track_score_batch(st, score=None, out=self._track)
        torch.ge(self._track["seg"], 0, out=self._on_path)
        if present is not None:
            torch.logical_and(self._on_path, present, out=self._on_path)
        return self._track["err"]

    def _sort(self, err, st, pid):
        """kmpc_order_fleet: the fleet's order by (path, arclength), into self.order, for the search along it"""
        dev = self.device
        _lib.check(self._lib.kmpc_order_fleet(dev.index, self.B, ptr(err[:, 3]), 4, ptr(st[:, 3]), int(st.stride(0)), ptr(pid), ptr(self._on_path),
                                              ptr(self.order), ptr(self._count), ptr(self._ws), self._ws.numel(), stream(dev)))


class Follower(_FleetSearch):
    """Car following on a waypoint helper's recorded paths (kmpc_follow_fleet, include/kmpc_follow.h): per vehicle the nearest vehicle ahead on
    its own path by arclength, the gap to it, and a speed cap from the following law.  `grt`: a FleetRefTrajectory (the vehicle's path is
    grt.path_id[b] at the time of the call) or a GPSRefTrajectory (one path; `rows` is then required, its length is the fleet's size).

    rows [B,8] (follow_params): a public device tensor, read by every cap() as it is -- edit it in place between steps, like fleet.path_id.
    After a cap(): `gap` [B] (+inf without a leader), `leader_speed` [B] (0 without), `leader` [B] int32 (-1 without); `stat` [B,8] is the
    running record (FOLLOW_STAT_FIELDS; reset() starts it afresh, summary() downloads it).

    radar=RangeSensor(B, ...): the law no longer reads the truth.  cap() runs the search as before -- `stat`, `gap`, `leader_speed` and `leader` stay
    the record of the TRUTH: contacts and the smallest gap are physical facts -- and keeps that call's cap as `v_ideal` [B], what a perfect sensor
    would have said; then kmpc_range_follow_batch (include/kmpc_range.h) measures, tracks and applies the law to what the track believes, with the
    follower's own speed from `known`: that is the cap returned.  `gap_seen`, `v_lead_seen` [B]: the track's gap and leader speed (+inf and 0
    without a track).  Without radar= the class makes exactly the library calls it made without the argument.

    search="pairs": kmpc_follow_fleet's exact pair search, O(B^2) -- the default, and the faster one for a few thousand vehicles.  search="sorted":
    every cap() orders the fleet by (path, arclength) (kmpc_order_fleet) and searches along that order (kmpc_order_follow_fleet;
    include/kmpc_order.h), O(B log B) with the same results bit for bit; `order` [B] int32, the count word and the workspace are allocated once,
    here.  The radar works unchanged behind either: it reads `gap_leader` and `leader`."""

    def __init__(self, grt, rows=None, radar=None, search="pairs"):
        self._init_helper(grt, "Follower", "follows", (rows,), "follow_params")
        self.rows = follow_params(self.B, self.device) if rows is None else rows
        self._check_rows()
        dev, B = self.device, self.B
        self.gap_leader = torch.empty((B, 2), dtype=torch.float64, device=dev)   # gap, the leader's speed: what the kernel writes
        self.gap_leader[:, 0] = float("inf")
        self.gap_leader[:, 1] = 0.0
        self.leader = torch.full((B,), -1, dtype=torch.int32, device=dev)
        if radar is not None and not (isinstance(radar, RangeSensor) and radar.B == B and radar.device == dev):
            raise ValueError("radar= must be a ref_traj.RangeSensor for %d vehicles on %s" % (B, dev))
        self.radar = radar
        self.v_ideal = torch.empty((B,), dtype=torch.float64, device=dev) if radar is not None else None
        self._init_search(search)
        self.reset()

    def _seen(self, field, none):
        if self.radar is None:
            raise ValueError("gap_seen and v_lead_seen are a radar's: this Follower has none (radar=RangeSensor(...))")
        rec = self.radar.rec
        word = rec[:, RANGE_REC_FIELDS.index(field)]
        return torch.where(rec[:, RANGE_REC_FIELDS.index("track_id")] >= 0.0, word, torch.full_like(word, none))

    gap_seen = property(lambda self: self._seen("gap_hat", float("inf")))
    v_lead_seen = property(lambda self: self._seen("v_hat", 0.0))

    def _check_rows(self):
        if not is_buffer(self.rows, torch.float64, (self.B, FOLLOW_WORDS), self.device):
            raise ValueError("rows must be a contiguous float64 tensor [%d,8] on %s (follow_params; write into it in place)" % (self.B, self.device))

    def reset(self):
        """a fresh record for every vehicle (and, with a radar, no track)"""
        self.stat = fresh_follow_stat(self.B, self.device)
        if self.radar is not None:
            self.radar.reset()

    def summary(self):
        """the record as named numpy fields [B] (one synchronising download): FOLLOW_STAT_FIELDS, the four counts as integers"""
        return record_fields(self.stat, FOLLOW_STAT_FIELDS, ("n", "n_leader", "n_bound", "n_contact"))

    def cap(self, state, v_cap, out=None, present=None, known=None, k=None, dt=None):
        """state: device tensor [B,W], X, Y, psi, v first (the plant's [B,8] as it is: no copy); v_cap [B] -> v [B] (`out`, which may be v_cap
        itself, or a new tensor): v_cap, lowered where the vehicle ahead demands it.  present [B] (uint8 / bool) or None: 0 = not on the road.
        One geometry-only track_score_batch call for the arclengths, then kmpc_follow_fleet; a vehicle the score call refuses (a path id
        outside the set, a pose that is not finite) is not on the road.  With a radar: known [B,W] (v in column 3: the state the controllers
        read; None: `state`), k (the period's index: the draws' counter) and dt (the period [s]) -- k and dt are then required.
        Asynchronous on torch's current stream."""
        dev, B = self.device, self.B
        radar = self.radar
        if radar is None:
            if known is not None or k is not None or dt is not None:
                raise ValueError("known=, k= and dt= are read by a radar: this Follower has none (radar=RangeSensor(...))")
        else:
            if k is None or dt is None:
                raise ValueError("a Follower with a radar needs the period's index k= (the draws' counter) and its length dt= [s] in every cap()")
            k, dt = int(k), float(dt)
            if not (k >= 0 and 0.0 < dt < float("inf")):
                raise ValueError("k >= 0 and a finite dt > 0, got k=%d, dt=%r" % (k, dt))
            kn = state_view(state if known is None else known, 4, dev, B, "known: expected [%d,W] with v in column 3, got %s")
            radar._check()
            if not is_buffer(radar.rec, torch.float64, (B, RANGE_REC_WORDS), dev):
                raise ValueError("radar.rec must stay a contiguous float64 tensor [%d,16] on %s (reset() gives a fresh one)" % (B, dev))
        st = state_view(state, 4, dev, B, "state: expected [%d,W] with X, Y, psi, v in the first four columns, got %s")
        vc = cap_in(v_cap, B, dev)
        self._check_rows()
        pid = self._path_id()
        check_present(present, B, dev)
        if not is_buffer(self.stat, torch.float64, (B, FOLLOW_STAT_WORDS), dev):
            raise ValueError("stat must stay a contiguous float64 tensor [%d,8] on %s (reset() gives a fresh one)" % (B, dev))
        out = cap_out(out, B, dev)
        if B == 0:
            return out
        err = self._place(st, present)
        args = (dev.index, B, ptr(err[:, 3]), 4, ptr(st[:, 3]), int(st.stride(0)), ptr(pid), ptr(self._on_path))
        outs = (ptr(self.rows), ptr(vc), ptr(out if radar is None else self.v_ideal), ptr(self.gap_leader), ptr(self.leader), ptr(self.stat))
        if self.search == "pairs":
            _lib.check(self._lib.kmpc_follow_fleet(*args, *outs, stream(dev)))
        else:
            self._sort(err, st, pid)
            _lib.check(self._lib.kmpc_order_follow_fleet(*args, *outs, ptr(self.order), stream(dev)))
        if radar is not None:
            _lib.check(self._lib.kmpc_range_follow_batch(dev.index, B, dt, ptr(self.gap_leader), ptr(self.leader), ptr(st[:, 3]), int(st.stride(0)),
                                                         ptr(kn[:, 3]), int(kn.stride(0)), ptr(self.rows), ptr(radar.rows), radar.seed, k,
                                                         radar.id_base, ptr(vc), ptr(out), ptr(radar.rec), ptr(radar.meas), stream(dev)))
        return out


LANE_WORDS, LANE_REC_WORDS = 8, 16
LANE_FIELDS = ("n_lanes", "width", "v_lat", "gain", "hold", "clear_tol", "keep_right")   # KMPC_LANE_* words 0 ... 6 of include/kmpc_lanes.h, in row order (7 is read by nobody)
LANE_REC_FIELDS = ("lane", "lane_from", "offset", "hold_left", "n", "n_leader", "n_bound", "n_contact", "min_gap", "max_closing", "n_changes",
                   "sum_elane2", "max_elane")   # KMPC_LANEREC_* words 0 ... 12, in order


def lane_default():
    """the default lane row (1, 3.5, 1.0, 0.5, 20, 0.5, 1, 0) as a numpy row [8], from kmpc_lane_default"""
    return default_row("kmpc_lane_default", LANE_WORDS)


def check_lane_rows(rows):
    """[B,8] host rows -> ValueError unless words 0 ... 6 are finite, n_lanes is an integer in 1 ... 32, width > 0, v_lat > 0, gain >= 0, hold an
    integer >= 0, clear_tol >= 0 and keep_right 0 or 1.  The kernel cannot refuse a row -- a bad word poisons that vehicle's own lane -- so this
    says so where the rows are written."""
    rows = host_rows(rows)
    if rows.ndim != 2 or rows.shape[1] != LANE_WORDS:
        raise ValueError("lane rows: [B,8] (%s, one unused word), got %s" % (", ".join(LANE_FIELDS), rows.shape))
    with np.errstate(invalid="ignore"):
        ok = (np.isfinite(rows[:, 0:7]).all(1) & (rows[:, 0] >= 1.0) & (rows[:, 0] <= 32.0) & (rows[:, 0] == np.floor(rows[:, 0]))
              & (rows[:, 1] > 0.0) & (rows[:, 2] > 0.0) & (rows[:, 3] >= 0.0) & (rows[:, 4] >= 0.0) & (rows[:, 4] == np.floor(rows[:, 4]))
              & (rows[:, 5] >= 0.0) & ((rows[:, 6] == 0.0) | (rows[:, 6] == 1.0)))
    if not ok.all():
        raise ValueError("lane rows: every word finite, n_lanes an integer in 1 ... 32, width > 0, v_lat > 0, gain >= 0, hold an integer >= 0, "
                         "clear_tol >= 0, keep_right 0 or 1 (vehicle(s) %s)" % rows_of(~ok))
    return rows


def lane_params(B, device=0, **overrides):
    """[B,8] float64 lane rows on `device`: the default row, with each override (`n_lanes=`, `width=`, `v_lat=`, `gain=`, `hold=`, `clear_tol=`,
    `keep_right=`) a scalar or one value per vehicle.  Validated on the host (check_lane_rows) before anything reaches the device."""
    return torch.as_tensor(check_lane_rows(table_rows("lane_params", LANE_FIELDS, lane_default(), B, overrides))).to(device_of(device))


def fresh_lane_rec(B, device):
    """[B,16] float64 on `device`: B fresh lane records (kmpc_lane_rec_init: lane 0, not changing, offset 0, counters 0, smallest gap +inf)"""
    return fresh_record("kmpc_lane_rec_init", B, LANE_REC_WORDS, device)


class Lanes(_FleetSearch):
    """Lanes on a waypoint helper's recorded paths (kmpc_lane_step_fleet, kmpc_ref_offset_batch; include/kmpc_lanes.h): per vehicle a lane and a
    commanded lateral offset (lane L's centre runs L * width to the LEFT of the recorded line), the leader among the vehicles in its own lane(s)
    with the following law's cap, the neighbours in the adjacent lanes, the lane-change decision and the offset ramp.  `grt`: a FleetRefTrajectory
    or a GPSRefTrajectory (one path; `follow_rows` or `lane_rows` is then required, its length is the fleet's size), as for Follower.
    `lane0` [B]: the starting lanes (integers inside each vehicle's n_lanes); a vehicle started in lane L has offset L * width.

    rows [B,8] (lane_params), follow_rows [B,8] (follow_params), rec [B,16] (LANE_REC_FIELDS): public device tensors, read by every step() as
    they are -- edit them in place between steps.  Views after a step(): `lane` [B], `offset` [B] (columns of rec), `gap` [B] (+inf without a
    leader), `leader_speed` [B], `leader` [B] int32 (-1 without), `neighbours` [B,4,2] (gap and speed of left-ahead, left-behind, right-ahead,
    right-behind; (+inf, 0) where there is none).  Limits: lanes are offsets of ONE recorded path; the speed along an offset line differs by
    1 - kappa * d and nothing corrects for it; the range sensor is perfect.

    search="pairs": kmpc_lane_step_fleet's exact pair search, O(B^2), the default.  search="sorted": every step() orders the fleet
    (kmpc_order_fleet) and runs kmpc_order_lane_step_fleet (include/kmpc_order.h), O(B log B) with the same results bit for bit.  lanes_max: the
    lanes its per-lane tables cover, 0 ... 32; None sizes them from the largest n_lanes in `lane_rows` here, at construction (one download; none
    later).  A vehicle whose lanes reach beyond lanes_max is still searched exactly, by a walk.  `order`, the count word and the workspace are
    allocated once, here."""

    def __init__(self, grt, follow_rows=None, lane_rows=None, lane0=None, search="pairs", lanes_max=None):
        self._init_helper(grt, "Lanes", "run", (follow_rows, lane_rows), "follow_params or lane_params")
        dev, B = self.device, self.B
        self.follow_rows = follow_params(B, dev) if follow_rows is None else follow_rows
        self.rows = lane_params(B, dev) if lane_rows is None else lane_rows
        self._check_rows()
        if lane0 is None:
            self._lane0 = np.zeros(B)
        else:
            self._lane0 = np.asarray(lane0.detach().cpu().numpy() if isinstance(lane0, torch.Tensor) else lane0, dtype=np.float64)
            n_lanes = self.rows[:, 0].cpu().numpy()
            if self._lane0.shape != (B,) or not ((self._lane0 == np.floor(self._lane0)) & (self._lane0 >= 0.0) & (self._lane0 < n_lanes)).all():
                raise ValueError("lane0: one integer lane per vehicle [%d], each inside 0 ... n_lanes - 1 of its lane row" % B)
        self.gap_leader = torch.empty((B, 2), dtype=torch.float64, device=dev)   # gap, the leader's speed: what the kernel writes
        self.leader = torch.empty((B,), dtype=torch.int32, device=dev)
        self.neighbours = torch.empty((B, 4, 2), dtype=torch.float64, device=dev)
        self._occ = [torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(2)]   # the occupancy words (uint32 bit patterns), ping-ponged
        if check_search(search) == "sorted":
            if lanes_max is None:
                n_max = float(self.rows[:, 0].max().item()) if B > 0 else 1.0
                lanes_max = int(min(max(n_max, 1.0), 32.0)) if n_max == n_max else 32
            if not (isinstance(lanes_max, int) and 0 <= lanes_max <= 32):
                raise ValueError("lanes_max: an integer in 0 ... 32 or None, got %r" % (lanes_max,))
            self.lanes_max = lanes_max
        elif lanes_max is not None:
            raise ValueError("lanes_max= sizes the tables of search=\"sorted\"; the pair search has none")
        self._init_search(search, lanes_max or 0)
        self.reset()

    lane = property(lambda self: self.rec[:, 0])
    offset = property(lambda self: self.rec[:, 2])
    occupancy = property(lambda self: self._occ[self._cur])

    def _check_rows(self):
        if not is_buffer(self.rows, torch.float64, (self.B, LANE_WORDS), self.device):
            raise ValueError("rows must be a contiguous float64 tensor [%d,8] on %s (lane_params; write into it in place)" % (self.B, self.device))
        if not is_buffer(self.follow_rows, torch.float64, (self.B, FOLLOW_WORDS), self.device):
            raise ValueError("follow_rows must be a contiguous float64 tensor [%d,8] on %s (follow_params; write into it in place)"
                             % (self.B, self.device))

    def reset(self):
        """a fresh record for every vehicle, in its starting lane at that lane's offset; nobody changing, no leader seen yet"""
        rec = fresh_lane_rec(self.B, "cpu").numpy()
        rec[:, 0] = rec[:, 1] = self._lane0
        rec[:, 2] = self._lane0 * self.rows[:, 1].cpu().numpy()
        self.rec = torch.from_numpy(rec).to(self.device)
        self._occ[0].copy_(torch.from_numpy((1 << self._lane0.astype(np.int64)).astype(np.uint32).view(np.int32)))
        self._cur = 0
        self.gap_leader[:, 0] = float("inf")
        self.gap_leader[:, 1] = 0.0
        self.leader.fill_(-1)
        self.neighbours[:, :, 0] = float("inf")
        self.neighbours[:, :, 1] = 0.0

    def summary(self):
        """the record as named numpy fields [B] (one synchronising download): LANE_REC_FIELDS, the lanes and the counts as integers, plus
        rms_elane (already divided by the number of calls; 0 where none was)"""
        out = record_fields(self.rec, LANE_REC_FIELDS, ("lane", "lane_from", "hold_left", "n", "n_leader", "n_bound", "n_contact", "n_changes"))
        out["rms_elane"] = np.sqrt(out["sum_elane2"] / np.maximum(out["n"], 1))
        return out

    def step(self, state, v_cap, k, dt, out=None, present=None):
        """one control period of the stage.  state: device tensor [B,W], X, Y, psi, v first (the plant's [B,8] as it is: no copy); v_cap [B] -> v [B]
        (`out`, which may be v_cap itself, or a new tensor): v_cap, lowered where the leader in the vehicle's own lane(s) demands it.  k: the
        period's index (left moves are decided in even, right moves in odd periods); dt: the period [s].  present [B] (uint8 / bool) or None.
        One geometry-only track_score_batch call for s_along and e_ct, then kmpc_lane_step_fleet; a vehicle the score call refuses is not on
        the road.  Asynchronous on torch's current stream."""
        dev, B = self.device, self.B
        st = state_view(state, 4, dev, B, "state: expected [%d,W] with X, Y, psi, v in the first four columns, got %s")
        vc = cap_in(v_cap, B, dev)
        self._check_rows()
        pid = self._path_id()
        check_present(present, B, dev)
        if not is_buffer(self.rec, torch.float64, (B, LANE_REC_WORDS), dev):
            raise ValueError("rec must stay a contiguous float64 tensor [%d,16] on %s (reset() gives a fresh one)" % (B, dev))
        out = cap_out(out, B, dev)
        if B == 0:
            return out
        err = self._place(st, present)
        occ_in, occ_out = self._occ[self._cur], self._occ[1 - self._cur]
        args = (dev.index, B, int(k), float(dt), ptr(err[:, 3]), 4, ptr(err[:, 0]), 4, ptr(st[:, 3]), int(st.stride(0)), ptr(pid),
                ptr(self._on_path), ptr(self.follow_rows), ptr(self.rows), ptr(vc), ptr(out), ptr(occ_in), ptr(occ_out), ptr(self.rec),
                ptr(self.gap_leader), ptr(self.leader), ptr(self.neighbours))
        if self.search == "pairs":
            _lib.check(self._lib.kmpc_lane_step_fleet(*args, stream(dev)))
        else:
            self._sort(err, st, pid)
            _lib.check(self._lib.kmpc_order_lane_step_fleet(*args, ptr(self.order), self.lanes_max, ptr(self._ws), self._ws.numel(), stream(dev)))
        self._cur = 1 - self._cur
        return out

    def shift(self, ref):
        """ref [B,H+1,3] (X, Y, psi: a waypoint call's table) -> the same tensor, every point moved by the vehicle's commanded offset to the left
        of its heading (kmpc_ref_offset_batch on rec's offset column by stride: no copy); psi untouched.  One offset holds for the whole horizon."""
        B = self.B
        if not (isinstance(ref, torch.Tensor) and ref.dim() == 3 and is_buffer(ref, torch.float64, (B, ref.shape[1], 3), self.device)):
            raise ValueError("ref: expected a contiguous float64 tensor [%d,H+1,3] on %s" % (B, self.device))
        if not is_buffer(self.rec, torch.float64, (B, LANE_REC_WORDS), self.device):
            raise ValueError("rec must stay a contiguous float64 tensor [%d,16] on %s (reset() gives a fresh one)" % (B, self.device))
        if B == 0 or ref.shape[1] == 0:
            return ref
        _lib.check(self._lib.kmpc_ref_offset_batch(self.device.index, B, int(ref.shape[1]), ptr(ref), ptr(self.rec[:, 2]), LANE_REC_WORDS,
                                                   stream(self.device)))
        return ref
