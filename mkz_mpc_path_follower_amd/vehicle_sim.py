"""Batched mirror of scripts/vehicle_simulator.py (VehicleSimulator): the dynamic-bicycle plant the reference's
sim_path_follow.launch runs against the MPC node.  Attribute names and update methods follow the reference
(X, Y, psi, vx, vy, wz, acc, df, acc_des, df_des; `_mpc_cmd_callback`, `_update_vehicle_model`), but every
attribute is a length-B device tensor and the ODE runs on the MI355X (kmpc_sim_advance_batch).  No CPU fallback.

Monte-Carlo runs: `plant=plant_params(B, m=..., C_alpha_f=...)` gives every vehicle its own constants and `cmd_delay` a command latency in
model updates of 10 ms (kmpc_sim_advance_plant); `SensorModel` is the measurement stage between the plant and the controller
(kmpc_sense_batch).  Without them the simulator runs the kernel and computes the results it always did.  `Estimator` is the stage after the
sensor: an extended Kalman filter per vehicle on the solver's model (kmpc_estimate_batch), so that the controller is fed a filtered state.

Latency: `VehicleSimulator(cmd_queue_depth=D)` keeps the last D periods' commands, so that `cmd_delay` may exceed one call (kmpc_sim_advance_queue);
`SensorModel(meas_delay=, depth=)` measures the truth of an earlier period (kmpc_sense_delayed_batch); `LatencyCompensator` is the controller's
answer: a log of the commands sent and assumed delays of its own, from which it picks the filter's input and predicts the estimate ahead to the
moment the next command acts (kmpc_cmd_in_force_batch, kmpc_predict_ahead_batch).

Offset-free loops: `DisturbanceObserver` takes the estimator's place: the same filter on the model augmented with a course offset, a steering offset
and an acceleration offset (kmpc_observe_batch), and `offset()` takes the two input offsets out of the command (kmpc_cmd_offset_batch).
Under dead time its partner is `LatencyCompensator(disturbances=True)`, whose `predict_disturbed()` predicts ahead on that augmented model from the
observer's record (kmpc_predict_ahead_dist_batch).

Grip and road: `VehicleSimulator(road=road_params(B, mu=0.5, a_lat=1.5, ...))` gives every vehicle a road row -- friction limits per axle, specific
forces of grade and bank, a steering offset, an acceleration gain (kmpc_sim_advance_road) -- and counts, per vehicle and axle, the sub-steps in
which the tyre force was clipped (`road_stat`, `road_summary()`).  The neutral row computes what the command-queue plant computes, bit for bit.
`VehicleSimulator(road=, road_profile=RoadProfile(fleet, table))` makes the road a property of the place: a table with one row per recorded sample of
the fleet's paths (grip scale, grade, bank; road_profile_table / road_profile_patch / check_road_profile) is composed with the caller's rows
(`road_base`) into `road` at the top of every plant call (kmpc_road_profile_fleet), without a host round trip.

L0 actuation: `LowLevelController` is the reference's 50 Hz node src/LowLevelController.cpp for B vehicles (kmpc_llc_step_batch: clamp, throttle PI on
a low-passed differentiated speed, brake torque below a deadband, steering-wheel angle), and `VehicleSimulator(drive=drive_params(B, ...), llc=)`
puts it inside the plant, in front of a powertrain that turns pedals into force (kmpc_sim_advance_drive): the command then no longer acts as an
acceleration.  `llc.summary()` downloads the controller's counters.  Without `drive=` every code path is the one that ran before.

Coloured noise and gusts: `Wander(B, wander_params(B, sigma=..., tau=..., walk=...))` keeps eight Gauss-Markov processes per vehicle and, once per
period, adds them to a sensor row's biases and a road row's a_long, a_lat, df_offset (kmpc_wander_batch), on the device.  The closed loops take it
as `wander=`; the sense and plant kernels read the composed rows as they read the caller's before.
"""
import numpy as np
import torch

from . import _lib
from ._stage import (default_row, device_of, fill_blocks, host_rows, is_buffer, is_state_view, own_path_id, ptr, record_fields, rows_of, stream,
                     table_rows)
from .messages import StateEst

X0, Y0, PSI0 = -300.0, -450.0, 1.0  # vehicle_simulator.py:28-30 (rosparam defaults)

PLANT_FIELDS = ("lf", "lr", "m", "Iz", "C_alpha_f", "C_alpha_r", "k_acc", "k_df")   # KMPC_PLANT_* of include/kmpc.h, in row order
SENSOR_FIELDS = ("sigma_x", "sigma_y", "sigma_psi", "sigma_v", "bias_x", "bias_y", "bias_psi", "bias_v")   # KMPC_SENSOR_*
ROAD_FIELDS = ("mu_f", "mu_r", "a_long", "a_lat", "df_offset", "acc_gain")   # KMPC_ROAD_* words 0 ... 5, in row order (6 and 7 are read by nobody)
ESTIMATOR_FIELDS = ("x", "y", "psi", "v", "pxx", "pxy", "pxpsi", "pxv", "pyy", "pypsi", "pyv", "ppsipsi", "ppsiv", "pvv", "count", "skipped")   # KMPC_EST_*
ESTIMATOR_PARAM_FIELDS = ("q_x", "q_y", "q_psi", "q_v", "r_x", "r_y", "r_psi", "r_v")   # KMPC_ESTPAR_*
OBSERVER_FIELDS = ("x", "y", "psi", "v", "dpsi", "ddelta", "da")   # KMPC_OBS_* words 0 ... 6; 7 ... 34 the covariance, 35 count, 36 skipped
OBSERVER_PARAM_FIELDS = ("q_x", "q_y", "q_psi", "q_v", "q_dpsi", "q_ddelta", "q_da", "r_x", "r_y", "r_psi", "r_v", "p0_dpsi", "p0_ddelta", "p0_da")   # KMPC_OBSPAR_*
LLC_FIELDS = ("kp", "ki", "accel_max", "decel_max", "steer_ratio", "mass", "brake_deadband", "wheel_radius")   # KMPC_LLC_*
DRIVE_FIELDS = ("f_peak", "p_max", "k_th", "k_br", "c_roll", "c_drag", "steer_ratio", "wheel_radius")   # KMPC_DRIVE_*
LLC_RECORD_FIELDS = ("int", "lpf", "ready", "v_last", "th_cmd", "br_cmd", "wheel_cmd", "acc_cmd", "th", "br", "ticks", "n_th_sat", "n_deadband",
                     "n_brake", "sum_err2", "max_err")   # KMPC_LLCREC_*
EST_SKIP_X, EST_SKIP_Y, EST_SKIP_PSI, EST_SKIP_V, EST_INIT, EST_RESET = 1, 2, 4, 8, 16, 32   # KMPC_EST_FLAG_*


def _int_per_vehicle(name, v, B, lo, hi=None):
    """a scalar or one integer per vehicle within [lo, hi] -> int32 [B] on the host (ValueError otherwise)"""
    d = torch.as_tensor(v).detach().cpu()
    if d.is_floating_point() or d.dtype == torch.bool or d.dim() > 1 or (d.dim() == 1 and d.shape[0] != B):
        raise ValueError("%s: an integer or one per vehicle [%d], got %r" % (name, B, v))
    d = d.to(torch.int64).expand(B)
    if B and (int(d.min()) < lo or (hi is not None and int(d.max()) > hi)):
        raise ValueError("%s: within %d ... %s, got %d ... %d" % (name, lo, "any" if hi is None else hi, int(d.min()), int(d.max())))
    return d.to(torch.int32).contiguous()


def plant_default():
    """the reference's constants (vehicle_simulator.py:61-67, :112-113) as a numpy row [8], from kmpc_plant_default: they live in the library"""
    return default_row("kmpc_plant_default", 8)


def check_plant_rows(rows):
    """[B,8] host rows -> ValueError unless all are finite, lf, lr, m, Iz, C_alpha_f, C_alpha_r > 0 and the lag gains >= 0 (the kernel cannot
    refuse a row: a bad m or Iz poisons that vehicle's state)"""
    rows = host_rows(rows)
    if rows.ndim != 2 or rows.shape[1] != 8:
        raise ValueError("plant rows: [B,8] (%s), got %s" % (", ".join(PLANT_FIELDS), rows.shape))
    if not np.isfinite(rows).all():
        raise ValueError("plant rows: non-finite value in vehicle(s) %s" % rows_of(~np.isfinite(rows).all(1)))
    if not (rows[:, 0:6] > 0.0).all():
        raise ValueError("plant rows: lf, lr, m, Iz, C_alpha_f, C_alpha_r must be > 0 (vehicle(s) %s)" % rows_of(~(rows[:, 0:6] > 0.0).all(1)))
    if not (rows[:, 6:8] >= 0.0).all():
        raise ValueError("plant rows: the lag gains k_acc, k_df must be >= 0 (vehicle(s) %s)" % rows_of(~(rows[:, 6:8] >= 0.0).all(1)))
    return rows


def plant_params(B, device=0, **overrides):
    """[B,8] float64 plant rows on `device`: the reference's constants, with each override (`m=`, `C_alpha_f=`, ... : PLANT_FIELDS) a scalar or
    one value per vehicle.  Validated on the host (check_plant_rows) before anything reaches the device."""
    return torch.as_tensor(check_plant_rows(table_rows("plant_params", PLANT_FIELDS, plant_default(), B, overrides))).to(device_of(device))


def road_default():
    """the neutral road row (inf, inf, 0, 0, 0, 1, 0, 0) as a numpy row [8], from kmpc_road_default"""
    return default_row("kmpc_road_default", 8)


def check_road_rows(rows):
    """[B,8] host rows -> ValueError unless no word is NaN, mu_f, mu_r > 0 (+inf: no limit), every other word is finite and acc_gain > 0 (the
    kernel cannot refuse a row: a bad one poisons that vehicle)"""
    rows = host_rows(rows)
    if rows.ndim != 2 or rows.shape[1] != 8:
        raise ValueError("road rows: [B,8] (%s, two unused words), got %s" % (", ".join(ROAD_FIELDS), rows.shape))
    if np.isnan(rows).any():
        raise ValueError("road rows: NaN in vehicle(s) %s" % rows_of(np.isnan(rows).any(1)))
    if not (rows[:, 0:2] > 0.0).all():
        raise ValueError("road rows: mu_f, mu_r must be > 0 (+inf: no limit) (vehicle(s) %s)" % rows_of(~(rows[:, 0:2] > 0.0).all(1)))
    if not np.isfinite(rows[:, 2:8]).all():
        raise ValueError("road rows: only mu_f, mu_r may be infinite (vehicle(s) %s)" % rows_of(~np.isfinite(rows[:, 2:8]).all(1)))
    if not (rows[:, 5] > 0.0).all():
        raise ValueError("road rows: acc_gain must be > 0 (vehicle(s) %s)" % rows_of(~(rows[:, 5] > 0.0)))
    return rows


def road_params(B, device=0, **overrides):
    """[B,8] float64 road rows on `device`: the neutral row, with each override (`mu=` for both axles, `mu_f=`, `mu_r=`, `a_long=`, `a_lat=`,
    `df_offset=`, `acc_gain=`) a scalar or one value per vehicle.  Validated on the host (check_road_rows) before anything reaches the device."""
    rows = table_rows("road_params", ROAD_FIELDS, road_default(), B, overrides, groups={"mu": (0, 1)},
                      conflict="%s= sets both axles; give mu_f= and mu_r= instead of combining them with it")
    return torch.as_tensor(check_road_rows(rows)).to(device_of(device))


FAULT_WORDS = 16
FAULT_FIELDS = ("p_lose_gps", "p_lose_imu", "p_lose_spd", "p_regain_gps", "p_regain_imu", "p_regain_spd", "win_from_gps", "win_from_imu", "win_from_spd",
                "win_len_gps", "win_len_imu", "win_len_spd", "p_outlier", "outlier_sigma", "max_age")   # KMPC_FAULT_* words 0 ... 14 (15 is read by nobody)
FAULT_RECORD_FIELDS = ("held_x", "held_y", "held_psi", "held_v", "count", "chain", "age_gps", "age_imu", "age_spd", "n_silent_gps", "n_silent_imu",
                       "n_silent_spd", "longest_gps", "longest_imu", "longest_spd", "n_outlier")   # KMPC_FAULTREC_*
FAULT_SILENT_GPS, FAULT_SILENT_IMU, FAULT_SILENT_SPD, FAULT_OUTLIER, FAULT_BLIND, FAULT_FRESH, FAULT_RESET = 1, 2, 4, 8, 16, 32, 64   # KMPC_FAULT_FLAG_*


def fault_default():
    """the neutral fault row (0,0,0, 1,1,1, 0,0,0, 0,0,0, 0, 0, inf, 0) as a numpy row [16], from kmpc_sense_faults_default"""
    return default_row("kmpc_sense_faults_default", FAULT_WORDS)


def check_fault_rows(rows):
    """[B,16] host rows -> ValueError unless no word is NaN, the seven probabilities lie in [0, 1], the windows' starts and lengths are non-negative
    whole numbers, outlier_sigma is finite and >= 0, and max_age >= 0 (+inf: never blind) (the kernel cannot refuse a row)"""
    rows = host_rows(rows)
    if rows.ndim != 2 or rows.shape[1] != FAULT_WORDS:
        raise ValueError("fault rows: [B,16] (%s, one unused word), got %s" % (", ".join(FAULT_FIELDS), rows.shape))
    if np.isnan(rows).any():
        raise ValueError("fault rows: NaN in vehicle(s) %s" % rows_of(np.isnan(rows).any(1)))
    prob = rows[:, [0, 1, 2, 3, 4, 5, 12]]
    if not ((prob >= 0.0) & (prob <= 1.0)).all():
        raise ValueError("fault rows: p_lose_*, p_regain_* and p_outlier are probabilities in [0, 1] (vehicle(s) %s)"
                         % rows_of(~((prob >= 0.0) & (prob <= 1.0)).all(1)))
    win = rows[:, 6:12]
    ok = np.isfinite(win) & (win >= 0.0)
    ok &= np.where(ok, win, 0.0) == np.floor(np.where(ok, win, 0.0))
    if not ok.all():
        raise ValueError("fault rows: win_from_* and win_len_* are non-negative whole numbers of periods (vehicle(s) %s)" % rows_of(~ok.all(1)))
    if not (np.isfinite(rows[:, 13]) & (rows[:, 13] >= 0.0)).all():
        raise ValueError("fault rows: outlier_sigma must be finite and >= 0 (vehicle(s) %s)" % rows_of(~(np.isfinite(rows[:, 13]) & (rows[:, 13] >= 0.0))))
    if not (rows[:, 14] >= 0.0).all():
        raise ValueError("fault rows: max_age must be >= 0 (+inf: never blind) (vehicle(s) %s)" % rows_of(~(rows[:, 14] >= 0.0)))
    if not np.isfinite(rows[:, 15]).all():
        raise ValueError("fault rows: word 15 must be finite (vehicle(s) %s)" % rows_of(~np.isfinite(rows[:, 15])))
    return rows


def fault_params(B, device=0, **overrides):
    """[B,16] float64 fault rows on `device`: the neutral row, with each override (FAULT_FIELDS; also `p_lose=`, `p_regain=`, `win_from=`, `win_len=`
    for all three sources) a scalar or one value per vehicle.  Validated on the host (check_fault_rows) before anything reaches the device."""
    groups = {"p_lose": (0, 1, 2), "p_regain": (3, 4, 5), "win_from": (6, 7, 8), "win_len": (9, 10, 11)}   # the words of the gps, imu, spd sources
    rows = table_rows("fault_params", FAULT_FIELDS, fault_default(), B, overrides, groups=groups,
                      conflict="%s= sets all three sources; give the per-source words instead of combining them with it")
    return torch.as_tensor(check_fault_rows(rows)).to(device_of(device))


WANDER_CHANNELS, WANDER_WORDS, WANDER_RECORD_WORDS = 8, 24, 16
WANDER_CHANNEL_NAMES = ("x", "y", "psi", "v", "a_long", "a_lat", "df_offset", "free")   # KMPC_WANDER_CH_*
WANDER_FIELDS = tuple(g + "_" + c for g in ("s0", "a", "q") for c in WANDER_CHANNEL_NAMES)   # KMPC_WANDER_S0 / _A / _Q + channel: words 0 ... 23
WANDER_RECORD_FIELDS = tuple("x_" + c for c in WANDER_CHANNEL_NAMES) + ("count",)   # KMPC_WANDERREC_* words 0 ... 8 (9 ... 15 are written back as read)


def wander_default():
    """the neutral wander row (24 zeros: every channel off) as a numpy row [24], from kmpc_wander_default"""
    return default_row("kmpc_wander_default", WANDER_WORDS)


def check_wander_rows(rows):
    """[B,24] host rows -> ValueError unless every word is finite, S0 >= 0, Q >= 0 and A in [0, 1] (the kernel cannot refuse a row: a bad one
    poisons that vehicle's processes)"""
    rows = host_rows(rows)
    if rows.ndim != 2 or rows.shape[1] != WANDER_WORDS:
        raise ValueError("wander rows: [B,24] (S0, A, Q of the channels %s), got %s" % (", ".join(WANDER_CHANNEL_NAMES), rows.shape))
    if not np.isfinite(rows).all():
        raise ValueError("wander rows: non-finite value in vehicle(s) %s" % rows_of(~np.isfinite(rows).all(1)))
    s0, a, q = rows[:, 0:8], rows[:, 8:16], rows[:, 16:24]
    if not ((s0 >= 0.0) & (q >= 0.0)).all():
        raise ValueError("wander rows: the standard deviations S0 and Q must be >= 0 (vehicle(s) %s)" % rows_of(~((s0 >= 0.0) & (q >= 0.0)).all(1)))
    if not ((a >= 0.0) & (a <= 1.0)).all():
        raise ValueError("wander rows: the carry-over A lies in [0, 1] (vehicle(s) %s)" % rows_of(~((a >= 0.0) & (a <= 1.0)).all(1)))
    return rows


def wander_rows(B, dt=0.1, sigma=0.0, tau=0.0, walk=0.0):
    """[B,24] host rows from physical parameters, each of `sigma`, `tau`, `walk` a scalar, 8 values (one per channel: WANDER_CHANNEL_NAMES) or [B,8].
    A stationary channel has the standard deviation `sigma` and the correlation time `tau` [s]: S0 = sigma, A = exp(-dt / tau) -- tau = inf gives
    A = 1, Q = 0, a random constant; tau = 0 gives A = 0, white noise -- and Q = sigma * sqrt(1 - A * A).  A channel with a `walk` rate r > 0
    [unit / sqrt(s)] is a random walk from 0: S0 = 0, A = 1, Q = r * sqrt(dt); its sigma must be 0.  sigma = 0 and walk = 0: the channel is off.
    `dt` is the control period [s].  Validated (check_wander_rows)."""
    B = int(B)
    if not (np.isfinite(dt) and dt > 0.0):
        raise ValueError("wander_rows: dt is the control period, finite and > 0, got %r" % (dt,))
    par = {}
    for name, v in (("sigma", sigma), ("tau", tau), ("walk", walk)):
        v = np.asarray(v, dtype=np.float64)
        if v.shape not in ((), (WANDER_CHANNELS,), (B, WANDER_CHANNELS)):
            raise ValueError("wander_rows: %s is a scalar, 8 values (one per channel) or [%d,8], got %s" % (name, B, v.shape))
        if np.isnan(v).any() or (v < 0.0).any() or (name != "tau" and np.isinf(v).any()):
            raise ValueError("wander_rows: %s must be >= 0%s" % (name, "" if name == "tau" else " and finite"))
        par[name] = np.broadcast_to(v, (B, WANDER_CHANNELS))
    sg, tau, wk = par["sigma"], par["tau"], par["walk"]
    if ((wk > 0.0) & (sg > 0.0)).any():
        raise ValueError("wander_rows: a channel is stationary (sigma, tau) or a random walk (walk), not both")
    with np.errstate(divide="ignore"):
        a = np.where(tau == 0.0, 0.0, np.exp(-dt / np.where(tau == 0.0, 1.0, tau)))
    rows = np.zeros((B, WANDER_WORDS))
    rows[:, 0:8] = np.where(wk > 0.0, 0.0, sg)
    rows[:, 8:16] = np.where(wk > 0.0, 1.0, a)
    rows[:, 16:24] = np.where(wk > 0.0, wk * np.sqrt(dt), sg * np.sqrt(1.0 - a * a))
    return check_wander_rows(rows)


def wander_params(B, device=0, dt=0.1, sigma=0.0, tau=0.0, walk=0.0):
    """wander_rows(B, dt, sigma, tau, walk) as a float64 tensor [B,24] on `device`"""
    return torch.as_tensor(wander_rows(B, dt=dt, sigma=sigma, tau=tau, walk=walk)).to(device_of(device))


class Wander:
    """The Gauss-Markov stage: eight first-order processes per vehicle -- errors on the measured x, y, psi, v that wander, gusts on the road row's
    a_long, a_lat and df_offset, and one free channel -- advanced once per control period and composed into the rows the sense and plant kernels
    read (kmpc_wander_batch; include/kmpc.h states the arithmetic).  `rows` [B,24] (WANDER_FIELDS: wander_params / wander_rows) are validated on the
    host.  `params` [B,24] and `rec` [B,16] (WANDER_RECORD_FIELDS; all zeros = fresh) are plain device tensors the caller may edit between calls;
    `x` is a view of rec[:, 0:8], the current values: the stage's output.  Vehicle b's history depends only on (seed, id_base + b, its row, the
    periods called): a shard passes its first vehicle's index as id_base.  `sensor_active` / `road_active`: whether any of the channels 0 ... 3 /
    4 ... 6 is on in any of the rows given here (what the closed loops check their sensor= and road= against)."""

    def __init__(self, B, rows, seed=0, id_base=0, device=0):
        self._lib = _lib.load()
        self.B, self.seed, self.id_base = int(B), int(seed), int(id_base)
        if not (0 <= self.seed < 2 ** 64 and 0 <= self.id_base and self.id_base + self.B < 2 ** 63):
            raise ValueError("Wander: seed in [0, 2^64), id_base >= 0")
        rows = check_wander_rows(rows)
        if rows.shape[0] != self.B:
            raise ValueError("Wander: rows is [%d,24], got %s" % (self.B, rows.shape))
        on = (rows[:, 0:8] != 0.0) | (rows[:, 16:24] != 0.0)
        self.sensor_active, self.road_active = bool(on[:, 0:4].any()), bool(on[:, 4:7].any())
        self.device = device_of(device)
        self.params = torch.as_tensor(np.ascontiguousarray(rows)).to(self.device)
        self.rec = torch.zeros((self.B, WANDER_RECORD_WORDS), dtype=torch.float64, device=self.device)

    x = property(lambda s: s.rec[:, 0:WANDER_CHANNELS])

    def reset(self):
        """every record fresh: the next step() draws first values again"""
        self.rec.zero_()

    def step(self, period, sensor_base=None, sensor_out=None, road_base=None, road_out=None):
        """advances every process to control period `period` (0 <= period < 2^62) and composes: sensor_out [B,8] = sensor_base with x[:, 0:4] added
        to the biases, road_out [B,8] = road_base with x[:, 4:7] added to a_long, a_lat, df_offset (each pair both None or both given; an out is
        never its base) -> x [B,8], the view of `rec`.  Asynchronous on torch's current stream."""
        own = ((self.params, WANDER_WORDS, "params"), (self.rec, WANDER_RECORD_WORDS, "rec"))
        for t, w, name in own + tuple((t, 8, name) for t, name in ((sensor_base, "sensor_base"), (sensor_out, "sensor_out"), (road_base, "road_base"),
                                                                   (road_out, "road_out")) if t is not None):
            if not is_buffer(t, torch.float64, (self.B, w), self.device):
                raise ValueError("%s: a contiguous float64 tensor [%d,%d] on %s" % (name, self.B, w, self.device))
        if self.device.type != "cuda":
            raise RuntimeError("Wander.step runs on an MI355X; no CPU fallback (device %s)" % self.device)
        _lib.check(self._lib.kmpc_wander_batch(self.device.index, self.B, ptr(self.params), ptr(self.rec), self.seed, int(period), self.id_base,
                                               ptr(sensor_base), ptr(sensor_out), ptr(road_base), ptr(road_out), stream(self.device)))
        return self.x

    def summary(self):
        """the records so far, one download -> dict of numpy arrays: x [B,8] (the current values), count [B] int64 and one [B] array per channel
        named by WANDER_RECORD_FIELDS"""
        out = record_fields(self.rec, WANDER_RECORD_FIELDS, ("count",))
        out["x"] = np.column_stack([out[k] for k in WANDER_RECORD_FIELDS[:WANDER_CHANNELS]])
        return out


PROFILE_WORDS = 8
PROFILE_FIELDS =("mu_scale", "a_long", "a_lat", "v_limit")   # KMPC_PROFILE_* words 0 ... 3 of include/kmpc.h, in row order (4 ... 7 are read by nobody)


def road_profile_default():
    """the neutral profile row (1, 0, 0, inf, 0, 0, 0, 0) as a numpy row [8], from kmpc_road_profile_default"""
    return default_row("kmpc_road_profile_default", PROFILE_WORDS)


def check_road_profile(table):
    """[n,8] host rows -> ValueError unless no word is NaN, mu_scale > 0 and finite, a_long and a_lat finite, v_limit >= 0 (+inf: none) and every
    other word finite (the kernels cannot refuse a row: a bad one reaches the vehicles whose nearest sample holds it)"""
    table = host_rows(table)
    if table.ndim != 2 or table.shape[1] != PROFILE_WORDS:
        raise ValueError("road profile: [n,8] (%s, four unused words), got %s" % (", ".join(PROFILE_FIELDS), table.shape))
    if np.isnan(table).any():
        raise ValueError("road profile: NaN in sample(s) %s" % rows_of(np.isnan(table).any(1)))
    if not ((table[:, 0] > 0.0) & np.isfinite(table[:, 0])).all():
        raise ValueError("road profile: mu_scale must be > 0 and finite (sample(s) %s)" % rows_of(~((table[:, 0] > 0.0) & np.isfinite(table[:, 0]))))
    for w in (1, 2):
        if not np.isfinite(table[:, w]).all():
            raise ValueError("road profile: %s must be finite (sample(s) %s)" % (PROFILE_FIELDS[w], rows_of(~np.isfinite(table[:, w]))))
    if not (table[:, 3] >= 0.0).all():
        raise ValueError("road profile: v_limit must be >= 0 (+inf: none) (sample(s) %s)" % rows_of(~(table[:, 3] >= 0.0)))
    if not np.isfinite(table[:, 4:8]).all():
        raise ValueError("road profile: only v_limit may be infinite (sample(s) %s)" % rows_of(~np.isfinite(table[:, 4:8]).all(1)))
    return table


def road_profile_table(fleet):
    """a neutral profile of a FleetRefTrajectory's paths: numpy [sum M, 8], path p's samples at rows off_p ... off_p + M_p - 1, in the order of
    fleet.trajectories (the curvature table's order)"""
    return np.tile(road_profile_default(), (sum(len(tr) for tr in fleet.trajectories), 1))


def road_profile_patch(table, fleet, path, s0, s1, **words):
    """writes the words given (`mu_scale=`, `a_long=`, `a_lat=`, `v_limit=`) into the rows of the samples of path `path` whose cdist lies in
    [s0, s1], in place -> the number of samples written.  Nothing else of the table is touched."""
    for k in words:
        if k not in PROFILE_FIELDS:
            raise ValueError("road_profile_patch: unknown word %r (one of %s)" % (k, ", ".join(PROFILE_FIELDS)))
    path = int(path)
    if not 0 <= path < len(fleet.trajectories):
        raise ValueError("road_profile_patch: path %d of %d" % (path, len(fleet.trajectories)))
    total = sum(len(tr) for tr in fleet.trajectories)
    if not (isinstance(table, np.ndarray) and table.dtype == np.float64 and table.shape == (total, PROFILE_WORDS)):
        raise ValueError("road_profile_patch: a float64 numpy table [%d,8] (road_profile_table), got %s" % (total, getattr(table, "shape", type(table))))
    off = sum(len(tr) for tr in fleet.trajectories[:path])
    s = fleet.trajectories[path][:, 6]
    idx = off + np.flatnonzero((s >= s0) & (s <= s1))
    for k, v in words.items():
        table[idx, PROFILE_FIELDS.index(k)] = float(v)
    return len(idx)


class RoadProfile:
    """A road profile of a FleetRefTrajectory's paths on the device: one row per recorded sample (grip scale, grade, bank, speed limit; include/kmpc.h,
    KMPC_PROFILE_*).  The same class serves as the truth (VehicleSimulator(road_profile=): the plant's road under each vehicle, once per period,
    kmpc_road_profile_fleet) and as the map (SpeedPlanner(profile=): kmpc_speed_plan_fleet_profile); the two are separate objects with separate tables.

    table [sum M, 8]: validated on the host (check_road_profile), then a public device tensor, read by every call as it is -- edit it in place with
    copy_ between steps (the kernels cannot validate it: check_road_profile first)."""

    def __init__(self, fleet, table=None):
        from .ref_traj import FleetRefTrajectory
        if not isinstance(fleet, FleetRefTrajectory):
            raise ValueError("RoadProfile is built on a FleetRefTrajectory (a one-path fleet covers a single path); a %s is not one" % type(fleet).__name__)
        self.fleet, self.device, self._lib = fleet, fleet.device, fleet._lib
        self.B = int(fleet.path_id.shape[0])
        self.total = sum(len(tr) for tr in fleet.trajectories)
        rows = road_profile_table(fleet) if table is None else host_rows(table)
        if np.shape(rows) != (self.total, PROFILE_WORDS):
            raise ValueError("road profile: [%d,8] rows, one per sample of the fleet's paths (road_profile_table), got %s" % (self.total, np.shape(rows)))
        self.table = torch.as_tensor(np.ascontiguousarray(check_road_profile(rows))).to(self.device).contiguous()
        self.closest = None   # [B] of the last apply(want_closest=True)

    def _own(self):
        if not is_buffer(self.table, torch.float64, (self.total, PROFILE_WORDS), self.device):
            raise ValueError("table must stay a contiguous float64 tensor [%d,8] on %s (write into it with copy_)" % (self.total, self.device))

    def apply(self, state, road_base, out, want_closest=False):
        """state: device tensor [B,W], X and Y first (no copy); road_base [B,8], the caller's road rows; out [B,8], never road_base itself -> out: the
        rows the plant reads this period.  want_closest=True also fills self.closest [B].  Asynchronous on torch's current stream."""
        dev, B = self.device, self.B
        self._own()
        if not (isinstance(state, torch.Tensor) and is_state_view(state, 2, dev, B)):   # refused, where the other stages copy
            raise ValueError("state: a float64 tensor [%d,W] on %s with X, Y in the first two columns" % (B, dev))
        for t, name in ((road_base, "road_base"), (out, "out")):
            if not is_buffer(t, torch.float64, (B, 8), dev):
                raise ValueError("%s: a contiguous float64 tensor [%d,8] on %s" % (name, B, dev))
        pid = own_path_id(self.fleet.path_id, B, dev)
        if want_closest and self.closest is None:
            self.closest = torch.empty((B,), dtype=torch.int32, device=dev)
        _lib.check(self._lib.kmpc_road_profile_fleet(self.fleet._h, B, ptr(self.table), ptr(state), int(state.stride(0)) if B else 2, ptr(pid),
                                                     ptr(road_base), ptr(out), ptr(self.closest) if want_closest else None, stream(dev)))
        return out


def llc_default():
    """the reference node's constants (LowLevelController.cpp:49-72, .h:113-118) as a numpy row [8], from kmpc_llc_default"""
    return default_row("kmpc_llc_default", 8)


def check_llc_rows(rows):
    """[B,8] host rows -> ValueError unless all are finite, accel_max, decel_max, steer_ratio, mass, wheel_radius > 0 and kp, ki, brake_deadband
    >= 0 (the kernel cannot refuse a row: a bad one poisons that vehicle)"""
    rows = host_rows(rows)
    if rows.ndim != 2 or rows.shape[1] != 8:
        raise ValueError("llc rows: [B,8] (%s), got %s" % (", ".join(LLC_FIELDS), rows.shape))
    if not np.isfinite(rows).all():
        raise ValueError("llc rows: non-finite value in vehicle(s) %s" % rows_of(~np.isfinite(rows).all(1)))
    pos = rows[:, [2, 3, 4, 5, 7]]
    if not (pos > 0.0).all():
        raise ValueError("llc rows: accel_max, decel_max, steer_ratio, mass, wheel_radius must be > 0 (vehicle(s) %s)" % rows_of(~(pos > 0.0).all(1)))
    nonneg = rows[:, [0, 1, 6]]
    if not (nonneg >= 0.0).all():
        raise ValueError("llc rows: kp, ki, brake_deadband must be >= 0 (vehicle(s) %s)" % rows_of(~(nonneg >= 0.0).all(1)))
    return rows


def llc_params(B, device=0, **overrides):
    """[B,8] float64 controller rows on `device`: the reference's constants, with each override (`kp=`, `mass=`, `brake_deadband=`, ... : LLC_FIELDS)
    a scalar or one value per vehicle.  Validated on the host (check_llc_rows) before anything reaches the device."""
    return torch.as_tensor(check_llc_rows(table_rows("llc_params", LLC_FIELDS, llc_default(), B, overrides))).to(device_of(device))


def drive_default():
    """the powertrain's default row (6000 N, 120 kW, lags 5 1/s, 0.15 m/s^2, 4e-4 1/m, 14.8, 0.33 m) as a numpy row [8], from kmpc_drive_default"""
    return default_row("kmpc_drive_default", 8)


def check_drive_rows(rows):
    """[B,8] host rows -> ValueError unless all are finite, f_peak, p_max, steer_ratio, wheel_radius > 0 and k_th, k_br, c_roll, c_drag >= 0 (the
    kernel cannot refuse a row: a bad one poisons that vehicle)"""
    rows = host_rows(rows)
    if rows.ndim != 2 or rows.shape[1] != 8:
        raise ValueError("drive rows: [B,8] (%s), got %s" % (", ".join(DRIVE_FIELDS), rows.shape))
    if not np.isfinite(rows).all():
        raise ValueError("drive rows: non-finite value in vehicle(s) %s" % rows_of(~np.isfinite(rows).all(1)))
    pos = rows[:, [0, 1, 6, 7]]
    if not (pos > 0.0).all():
        raise ValueError("drive rows: f_peak, p_max, steer_ratio, wheel_radius must be > 0 (vehicle(s) %s)" % rows_of(~(pos > 0.0).all(1)))
    if not (rows[:, 2:6] >= 0.0).all():
        raise ValueError("drive rows: k_th, k_br, c_roll, c_drag must be >= 0 (vehicle(s) %s)" % rows_of(~(rows[:, 2:6] >= 0.0).all(1)))
    return rows


def drive_params(B, device=0, **overrides):
    """[B,8] float64 powertrain rows on `device`: the default row, with each override (`f_peak=`, `c_drag=`, `steer_ratio=`, ... : DRIVE_FIELDS) a
    scalar or one value per vehicle.  Validated on the host (check_drive_rows) before anything reaches the device."""
    return torch.as_tensor(check_drive_rows(table_rows("drive_params", DRIVE_FIELDS, drive_default(), B, overrides))).to(device_of(device))


class LowLevelController:
    """The reference's 50 Hz low-level controller (src/LowLevelController.cpp) for B vehicles: one step() is one tick -- a speed report, then the
    control callback -- of every vehicle (kmpc_llc_step_batch; include/kmpc.h states the arithmetic).  Keyword arguments are LLC_FIELDS overrides,
    a scalar or one value per vehicle.  `params` [B,8] and `rec` [B,16] (LLC_RECORD_FIELDS; all zeros = the freshly constructed node) are plain
    device tensors the caller may edit between calls.  `v0`: the speed the vehicles already have (reset(v0)): a fresh record differentiates the
    first report against 0, as the reference does from rest, so a loop that starts at speed must say so.
    VehicleSimulator(drive=, llc=this) runs the same tick inside the plant; step() is the stage alone, for a caller with a plant of its own."""

    def __init__(self, B, device=0, v0=None, **overrides):
        self._lib = _lib.load()
        self.B = int(B)
        rows = check_llc_rows(table_rows("LowLevelController", LLC_FIELDS, llc_default(), self.B, overrides))
        if v0 is not None:
            v0 = np.asarray(v0, dtype=np.float64)
            if v0.shape not in ((), (self.B,)) or not np.isfinite(v0).all():
                raise ValueError("LowLevelController: v0 is a finite scalar or one speed per vehicle [%d]" % self.B)
        self.device = device_of(device)
        self.params = torch.as_tensor(rows).to(self.device)
        self.rec = torch.zeros((self.B, 16), dtype=torch.float64, device=self.device)
        self.reset(v0)

    def reset(self, v=None):
        """every record fresh; V_LAST = v (a scalar or [B]) when given"""
        self.rec.zero_()
        if v is not None:
            self.rec[:, 3] = torch.as_tensor(v, dtype=torch.float64, device=self.device)

    def _own(self):
        for t, w in ((self.params, 8), (self.rec, 16)):
            if not is_buffer(t, torch.float64, (self.B, w), self.device):
                raise ValueError("params [B,8] and rec [B,16] must stay contiguous float64 tensors on %s (write into them with copy_)" % self.device)

    def step(self, cmd, speed, out=None):
        """cmd [B,2] (accel, steer); speed [B]: a contiguous tensor or a column view such as sim.state[:, 3] (no copy is made)
        -> pedals [B,4]: throttle fraction, brake torque [N m], steering-wheel angle [rad], the clamped acceleration command"""
        self._own()
        ped = out if out is not None else torch.empty((self.B, 4), dtype=torch.float64, device=self.device)
        for t, w in ((cmd, 2), (ped, 4)):
            if not is_buffer(t, torch.float64, (self.B, w), self.device):
                raise ValueError("cmd [B,2] and out [B,4] must be contiguous float64 tensors on %s" % self.device)
        if not (isinstance(speed, torch.Tensor) and speed.dtype == torch.float64 and tuple(speed.shape) == (self.B,) and speed.device == self.device
                and (self.B <= 1 or speed.stride(0) >= 1)):
            raise ValueError("speed: float64 [B] on %s, rows a fixed distance >= 1 apart (a [B] buffer or sim.state[:, 3])" % self.device)
        stride = speed.stride(0) if self.B > 1 else 1
        _lib.check(self._lib.kmpc_llc_step_batch(self.device.index, self.B, ptr(cmd), ptr(speed), int(stride), ptr(self.params), ptr(self.rec), ptr(ped),
                                                 stream(self.device)))
        return ped

    def summary(self):
        """the record so far, one download -> dict of numpy arrays [B]: every LLC_RECORD_FIELDS word (the counters as int64) and rms_err, the root
        mean square of ac - LPF over the ticks"""
        out = record_fields(self.rec, LLC_RECORD_FIELDS, ("ticks", "n_th_sat", "n_deadband", "n_brake"))
        with np.errstate(all="ignore"):
            out["rms_err"] = np.sqrt(out["sum_err2"] / np.maximum(out["ticks"], 1))
        return out


class VehicleSimulator:
    dt_model = 0.01  # :24

    def __init__(self, B=1, X0=X0, Y0=Y0, Psi0=PSI0, device=0, plant=None, cmd_delay=None, cmd_queue_depth=None, road=None, drive=None, llc=None,
                 road_profile=None):
        """plant: [B,8] rows (plant_params) -- a plant per vehicle; cmd_delay: a scalar or one per vehicle, model updates of 10 ms by which a new
        command takes effect late (clamped to one call's n_updates; the command in force until then is `cmd_held`, 0 at the start).  Giving
        either runs kmpc_sim_advance_plant (the other defaults to the reference's constants / no delay); `plant`, `cmd_delay` (int32 [B]) and
        `cmd_held` [B,2] are then plain device tensors the caller may edit between steps.  Giving neither changes nothing.
        cmd_queue_depth=D (an integer >= 2): a ring `cmd_queue` [D,B,2] of the last D periods' commands replaces `cmd_held`
        (kmpc_sim_advance_queue), so that cmd_delay may exceed one call: it is clamped to (D - 1) n_updates.  The simulator then counts its calls
        in `period` (slot period mod D holds that call's command); every call of a run must use the same n_updates.
        road: [B,8] rows (road_params) -- grip limits, grade, bank, steering offset and acceleration gain per vehicle (kmpc_sim_advance_road).  It
        implies the queue path (cmd_queue_depth defaults to 2, which equals the held-command plant call after call) and allocates `road_stat` [B,4];
        `road` and `road_stat` are plain device tensors the caller may edit between steps (a wet patch that belongs to a place: road_profile=), and
        road_summary() downloads the grip bookkeeping.
        drive: [B,8] rows (drive_params) -- a powertrain per vehicle behind a LowLevelController `llc` (default: LowLevelController(B) with the
        reference's constants, its V_LAST at 0): the command passes through the controller's 50 Hz tick and acts as throttle and brake
        (kmpc_sim_advance_drive).  It implies the road and queue path (road defaults to the neutral rows); `drive`, `llc.params` and `llc.rec` are
        plain device tensors the caller may edit between steps.  A run that starts at speed calls llc.reset(v) first.
        road_profile: a RoadProfile for B vehicles on this device -- the road under each vehicle, per recorded sample of its path (the truth).  It
        implies road= (neutral rows by default).  The caller's rows then live in `road_base`; `road` is what the plant reads, rewritten from
        `road_base`, `state` and the profile's table at the top of every _update_vehicle_model call with n_updates > 0 (kmpc_road_profile_fleet: one
        more launch per period, no host round trip).  Without road_profile= there is no `road_base` and no such launch."""
        if road_profile is not None:   # checked before the GPU is touched
            if not (isinstance(road_profile, RoadProfile) and road_profile.B == int(B)):
                raise ValueError("road_profile: a RoadProfile for %d vehicles" % int(B))
            if road is None:
                road = np.tile(road_default(), (int(B), 1))
        drive_rows = None
        if llc is not None and drive is None:
            raise ValueError("llc= belongs to drive=: the controller acts on the plant only through the powertrain (drive_params)")
        if drive is not None:   # checked before the GPU is touched
            drive_rows = host_rows(drive)
            if np.shape(drive_rows) != (int(B), 8):
                raise ValueError("drive: [%d,8] rows (drive_params), got %s" % (int(B), np.shape(drive_rows)))
            drive_rows = check_drive_rows(drive_rows)
            if llc is not None and not (isinstance(llc, LowLevelController) and llc.B == int(B)):
                raise ValueError("llc: a LowLevelController for %d vehicles" % int(B))
            if road is None:
                road = np.tile(road_default(), (int(B), 1))
        road_rows = None
        if road is not None:   # checked before the GPU is touched, like the depth
            road_rows = host_rows(road)
            if np.shape(road_rows) != (int(B), 8):
                raise ValueError("road: [%d,8] rows (road_params), got %s" % (int(B), np.shape(road_rows)))
            road_rows = check_road_rows(road_rows)
            if cmd_queue_depth is None:
                cmd_queue_depth = 2
        self.cmd_queue_depth = None
        if cmd_queue_depth is not None:   # checked first: a bad depth is a ValueError on any machine
            if isinstance(cmd_queue_depth, bool) or not isinstance(cmd_queue_depth, (int, np.integer)) or cmd_queue_depth < 2:
                raise ValueError("cmd_queue_depth: an integer >= 2 (periods of commands kept), got %r" % (cmd_queue_depth,))
            self.cmd_queue_depth = int(cmd_queue_depth)
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("VehicleSimulator needs an MI355X; no CPU fallback")
        self.device = torch.device("cuda", device)
        self.B = int(B)
        # [B,8]: X, Y, psi, vx, vy, wz, acc, df   (:18-34; velocities and actuators start at 0)
        self.state = torch.zeros((self.B, 8), dtype=torch.float64, device=self.device)
        self.state[:, 0] = torch.as_tensor(X0, dtype=torch.float64, device=self.device)
        self.state[:, 1] = torch.as_tensor(Y0, dtype=torch.float64, device=self.device)
        self.state[:, 2] = torch.as_tensor(Psi0, dtype=torch.float64, device=self.device)
        self.cmd = torch.zeros((self.B, 2), dtype=torch.float64, device=self.device)  # acc_des, df_des (:21-22)
        self.plant = self.cmd_delay = self.cmd_held = self.cmd_queue = self.road = self.road_stat = self.drive = self.llc = None
        self.road_base = self.road_profile = None
        self.road_mid = None   # [B,8] with a Wander in front of a road profile: what the profile reads in road_base's place (wander_road_buffers)
        self.period = 0
        if plant is not None or cmd_delay is not None or cmd_queue_depth is not None:
            if plant is None:
                self.plant = plant_params(self.B, self.device)
            else:
                rows = host_rows(plant)
                if np.shape(rows) != (self.B, 8):
                    raise ValueError("plant: [%d,8] rows (plant_params), got %s" % (self.B, np.shape(rows)))
                self.plant = torch.as_tensor(check_plant_rows(rows)).to(self.device).contiguous()
            d = torch.as_tensor(0 if cmd_delay is None else cmd_delay).detach().cpu()
            if d.is_floating_point() or d.dim() > 1 or (d.dim() == 1 and d.shape[0] != self.B):
                raise ValueError("cmd_delay: an integer or one per vehicle [%d] (model updates of 10 ms)" % self.B)
            self.cmd_delay = d.to(torch.int32).expand(self.B).contiguous().to(self.device)
            if self.cmd_queue_depth is None:
                self.cmd_held = torch.zeros((self.B, 2), dtype=torch.float64, device=self.device)
            else:
                self.cmd_queue = torch.zeros((self.cmd_queue_depth, self.B, 2), dtype=torch.float64, device=self.device)
            if road_rows is not None:
                self.road = torch.as_tensor(road_rows).to(self.device).contiguous()
                self.road_stat = torch.zeros((self.B, 4), dtype=torch.float64, device=self.device)
                if road_profile is not None:
                    if road_profile.device != self.device:
                        raise ValueError("road_profile on %s, plant on %s" % (road_profile.device, self.device))
                    self.road_profile, self.road_base = road_profile, self.road
                    self.road = self.road_base.clone()
            if drive_rows is not None:
                self.drive = torch.as_tensor(drive_rows).to(self.device).contiguous()
                self.llc = llc if llc is not None else LowLevelController(self.B, device=self.device)
                if self.llc.device != self.device:
                    raise ValueError("llc on %s, plant on %s" % (self.llc.device, self.device))

    # views named as in the reference
    X = property(lambda s: s.state[:, 0]); Y = property(lambda s: s.state[:, 1]); psi = property(lambda s: s.state[:, 2])
    vx = property(lambda s: s.state[:, 3]); vy = property(lambda s: s.state[:, 4]); wz = property(lambda s: s.state[:, 5])
    acc = property(lambda s: s.state[:, 6]); df = property(lambda s: s.state[:, 7])
    acc_des = property(lambda s: s.cmd[:, 0]); df_des = property(lambda s: s.cmd[:, 1])

    def _mpc_cmd_callback(self, accel_cmd, steer_angle_cmd):  # :51-55, for all vehicles
        self.cmd[:, 0] = torch.as_tensor(accel_cmd, dtype=torch.float64, device=self.device)
        self.cmd[:, 1] = torch.as_tensor(steer_angle_cmd, dtype=torch.float64, device=self.device)

    def _update_vehicle_model(self, n_updates=1):
        """n_updates passes of :58-107 (each 10 Euler sub-steps of 1 ms + the actuator lag :109-113)"""
        dev, B = self.device, self.B
        for t, w in ((self.state, 8), (self.cmd, 2)):  # `state` and `cmd` are plain attributes: what reaches the kernel is a raw pointer
            if not is_buffer(t, torch.float64, (B, w), dev):
                raise ValueError("state [B,8] / cmd [B,2] must stay contiguous float64 tensors on %s (write into them with copy_)" % dev)
        head = (dev.index, B, ptr(self.state), ptr(self.cmd))   # what every plant call begins with
        if self.plant is None:
            rc = self._lib.kmpc_sim_advance_batch(*head, int(n_updates), stream(dev))
        elif self.cmd_queue_depth is not None:
            for t, shape, dt in ((self.plant, (B, 8), torch.float64), (self.cmd_delay, (B,), torch.int32),
                                 (self.cmd_queue, (self.cmd_queue_depth, B, 2), torch.float64)):
                if not is_buffer(t, dt, shape, dev):
                    raise ValueError("plant [B,8] / cmd_queue [D,B,2] float64 and cmd_delay [B] int32 must stay contiguous tensors on %s "
                                     "(write into them with copy_)" % dev)
            queue = (ptr(self.cmd_delay), ptr(self.cmd_queue), self.cmd_queue_depth, int(self.period), int(n_updates))   # ... and the ring, in every queue call
            if self.road is not None:
                for t, w in ((self.road, 8), (self.road_stat, 4)):
                    if not is_buffer(t, torch.float64, (B, w), dev):
                        raise ValueError("road [B,8] / road_stat [B,4] must stay contiguous float64 tensors on %s (write into them with copy_)" % dev)
                if self.road_profile is not None and int(n_updates) > 0:   # the road under each vehicle, from where it is now
                    self.road_profile.apply(self.state, self.road_base if self.road_mid is None else self.road_mid, self.road)
                if self.drive is not None:
                    if not is_buffer(self.drive, torch.float64, (B, 8), dev):
                        raise ValueError("drive [B,8] must stay a contiguous float64 tensor on %s (write into it with copy_)" % dev)
                    self.llc._own()
                    rc = self._lib.kmpc_sim_advance_drive(*head, ptr(self.plant), ptr(self.road), ptr(self.drive), ptr(self.llc.params), ptr(self.llc.rec),
                                                          *queue, ptr(self.road_stat), stream(dev))
                else:
                    rc = self._lib.kmpc_sim_advance_road(*head, ptr(self.plant), ptr(self.road), *queue, ptr(self.road_stat), stream(dev))
            else:
                rc = self._lib.kmpc_sim_advance_queue(*head, ptr(self.plant), *queue, stream(dev))
            if rc == 0 and int(n_updates) > 0:
                self.period += 1
        else:
            for t, shape, dt in ((self.plant, (B, 8), torch.float64), (self.cmd_delay, (B,), torch.int32), (self.cmd_held, (B, 2), torch.float64)):
                if not is_buffer(t, dt, shape, dev):
                    raise ValueError("plant [B,8] / cmd_held [B,2] float64 and cmd_delay [B] int32 must stay contiguous tensors on %s "
                                     "(write into them with copy_)" % dev)
            rc = self._lib.kmpc_sim_advance_plant(*head, ptr(self.plant), ptr(self.cmd_delay), ptr(self.cmd_held), int(n_updates), stream(dev))
        _lib.check(rc)

    def wander_road_buffers(self):
        """where a Wander composes the road: -> (base, out), the caller's rows and the rows the stage writes.  Without a road profile the caller's
        rows move to `road_base` and `road` (what the plant reads) is the stage's output; with one the stage acts first, base -> wander ->
        `road_mid` -> profile -> `road`, so each affected word is (base + x) + the profile's word.  ValueError without road=."""
        if self.road is None:
            raise ValueError("a wander with road channels needs a simulator with road= (road_params)")
        if self.road_profile is not None:
            if self.road_mid is None:
                self.road_mid = self.road_base.clone()
            return self.road_base, self.road_mid
        if self.road_base is None:
            self.road_base, self.road = self.road, self.road.clone()
        return self.road_base, self.road

    def road_summary(self):
        """the grip bookkeeping so far, one download -> dict of numpy arrays [B]: sat_f, sat_r (sub-steps in which the front / rear force was
        clipped) and util_f, util_r (the largest |C_alpha alpha| / limit); None without road="""
        if self.road_stat is None:
            return None
        st = self.road_stat.detach().cpu().numpy()
        return dict(sat_f=st[:, 0].astype(np.int64), sat_r=st[:, 1].astype(np.int64), util_f=st[:, 2].copy(), util_r=st[:, 3].copy())

    def state_est(self, i=0):
        """the state_est message of vehicle i (:40-48)"""
        s = self.state[i].cpu().numpy()
        return StateEst(x=float(s[0]), y=float(s[1]), psi=float(s[2]), v=float(s[3]), a=float(s[6]), df=float(s[7]))


class SensorModel:
    """The measurement stage between the plant and the controller: est = truth + bias + sigma * n on x, y, psi, v (kmpc_sense_batch), what
    scripts/state_publisher.py's GPS fix, IMU yaw and steering-report speed do to state_est on the real vehicle.  `sigma`, `bias`: a scalar,
    four values (x, y, psi, v) or [B,4].  `params` [B,8] (SENSOR_FIELDS) is a plain device tensor the caller may edit between calls.  Vehicle b's
    noise depends only on (seed, id_base + b, period): a shard of a larger fleet passes its first vehicle's index (dist.shard_range's lo) as id_base.
    `meas_delay` (an integer or one per vehicle, whole control periods, 0 ... depth - 1): the fix is that old when it is read
    (kmpc_sense_delayed_batch: the truth of period - meas_delay with this period's noise; period 0's state until the ring is filled); `depth`
    (default: the largest meas_delay + 1) sizes `truth_ring` [depth,B,4].  `meas_delay` [B] int32 is then a plain device tensor too, and sense()
    must be called once per period with consecutive periods from 0.  Without meas_delay the stage is what it was.
    `faults` [B,16] (FAULT_FIELDS: fault_params) gives every vehicle a fault row -- outages of the GPS, the IMU and the steering report by a random
    chain or a scheduled window, GPS outliers, a blind-time limit (kmpc_sense_faults_batch, with the ring when meas_delay is set).  sense() still
    returns the held state, what state_publisher.py would publish (a silent source's channels keep their last delivered value), and fills
    `z` [B,4] (NaN in a silent source's channels: what a filter reads), `flags` [B] int32 (FAULT_* bits), `blind` [B] uint8 and
    `fault_record` [B,16] (FAULT_RECORD_FIELDS; all zeros = fresh), all plain device tensors; `faults` is one too.  Without faults= the class
    calls what it called before."""

    def __init__(self, B, sigma=0.0, bias=0.0, seed=0, id_base=0, device=0, meas_delay=None, depth=None, faults=None):
        self._lib = _lib.load()
        self.B, self.seed, self.id_base = int(B), int(seed), int(id_base)
        if not (0 <= self.seed < 2 ** 64 and 0 <= self.id_base and self.id_base + self.B < 2 ** 63):
            raise ValueError("SensorModel: seed in [0, 2^64), id_base >= 0")
        rows = fill_blocks("SensorModel", np.zeros((self.B, 8)), (("sigma", sigma, 0, 4), ("bias", bias, 4, 4)), "four values (x, y, psi, v)")
        if not np.isfinite(rows).all() or not (rows[:, 0:4] >= 0.0).all():
            raise ValueError("SensorModel: sigma and bias must be finite, sigma >= 0")
        self.device = device_of(device)
        self.params = torch.as_tensor(rows).to(self.device)
        self.params_base = None   # [B,8] in a loop with wander=: the caller's rows; `params` is then rewritten from them every period
        self.meas_delay = self.truth_ring = self.depth = None
        if meas_delay is None and depth is not None:
            raise ValueError("SensorModel: depth belongs to meas_delay")
        if meas_delay is not None:
            d = _int_per_vehicle("SensorModel: meas_delay", meas_delay, self.B, 0)
            need = (int(d.max()) if self.B else 0) + 1
            if depth is None:
                depth = need
            if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or depth < need:
                raise ValueError("SensorModel: depth is an integer >= the largest meas_delay + 1 = %d, got %r" % (need, depth))
            self.depth = int(depth)
            self.meas_delay = d.to(self.device)
            self.truth_ring = torch.zeros((self.depth, self.B, 4), dtype=torch.float64, device=self.device)
        self.faults = self.z = self.flags = self.blind = self.fault_record = None
        if faults is not None:
            rows = check_fault_rows(faults)
            if rows.shape[0] != self.B:
                raise ValueError("SensorModel: faults is [%d,16], got %s" % (self.B, rows.shape))
            self.faults = torch.as_tensor(rows).to(self.device).contiguous()
            self.z = torch.zeros((self.B, 4), dtype=torch.float64, device=self.device)
            self.flags = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
            self.blind = torch.zeros((self.B,), dtype=torch.uint8, device=self.device)
            self.fault_record = torch.zeros((self.B, FAULT_WORDS), dtype=torch.float64, device=self.device)

    def reset_faults(self):
        """every fault record fresh: the next sense() delivers every source"""
        if self.faults is None:
            raise ValueError("SensorModel.reset_faults: this sensor was built without faults=")
        self.fault_record.zero_()
        self.flags.zero_()
        self.blind.zero_()

    def fault_summary(self):
        """the fault records so far, one download -> dict of numpy arrays [B] named by FAULT_RECORD_FIELDS (the counters as int64); None without
        faults="""
        if self.faults is None:
            return None
        return record_fields(self.fault_record, FAULT_RECORD_FIELDS, FAULT_RECORD_FIELDS[4:])

    def _sense_faults(self, state, period, est):
        own = ((self.faults, (self.B, FAULT_WORDS), torch.float64), (self.fault_record, (self.B, FAULT_WORDS), torch.float64),
               (self.z, (self.B, 4), torch.float64), (self.flags, (self.B,), torch.int32), (self.blind, (self.B,), torch.uint8))
        if self.meas_delay is not None:
            own += ((self.meas_delay, (self.B,), torch.int32), (self.truth_ring, (self.depth, self.B, 4), torch.float64))
        for t, shape, dt in own:
            if not is_buffer(t, dt, shape, self.device):
                raise ValueError("faults / fault_record [B,16] and z [B,4] float64, flags [B] int32, blind [B] uint8, meas_delay [B] int32 and "
                                 "truth_ring [depth,B,4] float64 must stay contiguous tensors on %s" % self.device)
        ring = (self.meas_delay, self.truth_ring, self.depth) if self.meas_delay is not None else (None, None, 0)
        _lib.check(self._lib.kmpc_sense_faults_batch(self.device.index, self.B, ptr(state), ptr(self.params), ptr(self.faults), self.seed, int(period),
                                                     self.id_base, ptr(ring[0]), ptr(ring[1]), ring[2], ptr(self.fault_record), ptr(self.z), ptr(est),
                                                     ptr(self.flags), ptr(self.blind), stream(self.device)))
        return est

    def sense(self, state, period, out=None):
        """state [B,8] (the plant's) -> est [B,4] = x, y, psi (wrapped to [-pi, pi)), v (>= 0) as measured in control period `period`"""
        est = out if out is not None else torch.empty((self.B, 4), dtype=torch.float64, device=self.device)
        for t, w in ((state, 8), (self.params, 8), (est, 4)):
            if not is_buffer(t, torch.float64, (self.B, w), self.device):
                raise ValueError("state [B,8], params [B,8] and est [B,4] must be contiguous float64 tensors on %s" % self.device)
        if self.faults is not None:
            return self._sense_faults(state, period, est)
        if self.meas_delay is not None:
            for t, shape, dt in ((self.meas_delay, (self.B,), torch.int32), (self.truth_ring, (self.depth, self.B, 4), torch.float64)):
                if not is_buffer(t, dt, shape, self.device):
                    raise ValueError("meas_delay [B] int32 and truth_ring [depth,B,4] float64 must stay contiguous tensors on %s" % self.device)
            _lib.check(self._lib.kmpc_sense_delayed_batch(self.device.index, self.B, ptr(state), ptr(self.params), self.seed, int(period), self.id_base,
                                                          ptr(self.meas_delay), ptr(self.truth_ring), self.depth, ptr(est), stream(self.device)))
            return est
        _lib.check(self._lib.kmpc_sense_batch(self.device.index, self.B, ptr(state), ptr(self.params), self.seed, int(period), self.id_base, ptr(est),
                                              stream(self.device)))
        return est


def _filter_scalars(name, gate, dt, L_a, L_b):
    """the scalars the estimator and the observer share -> (gate, dt, L_a, L_b) as floats; ValueError unless gate >= 0, the others > 0, all finite"""
    g, d, a, b = float(gate), float(dt), float(L_a), float(L_b)
    if not (np.isfinite([g, d, a, b]).all() and g >= 0.0 and d > 0.0 and a > 0.0 and b > 0.0):
        raise ValueError("%s: gate >= 0, dt > 0, L_a > 0, L_b > 0, all finite (got %r, %r, %r, %r)" % (name, gate, dt, L_a, L_b))
    return g, d, a, b


def _filter_input(flags, u, B, device):
    """what Estimator.update and DisturbanceObserver.update check after their own buffers, in this order: the stage's `flags` [B] int32, then the
    input `u` [B,2], which may be a column view (unit column stride, rows a fixed distance >= 2 apart) -> u's row stride as the kernel takes it"""
    if not is_buffer(flags, torch.int32, (B,), device):
        raise ValueError("flags must stay a contiguous int32 tensor [B] on %s" % device)
    if not (isinstance(u, torch.Tensor) and u.dtype == torch.float64 and tuple(u.shape) == (B, 2) and u.device == device
            and (B == 0 or (u.stride(1) == 1 and (B == 1 or u.stride(0) >= 2)))):
        raise ValueError("u: float64 [B,2] on %s with unit column stride and rows >= 2 apart (a [B,2] buffer or sim.state[:, 6:8])" % device)
    return int(u.stride(0)) if B > 1 else 2


class Estimator:
    """The stage between the sensor and the controller: one extended Kalman filter per vehicle on the solver's kinematic model
    (kmpc_estimate_batch; include/kmpc.h states the arithmetic).  `q`: process standard deviations PER CALL of x, y, psi, v; `r`: measurement
    standard deviations -- each a scalar, four values or [B,4].  `gate` > 0 skips a channel whose innovation exceeds `gate` standard deviations
    (0: no gate); a non-finite measurement is a dropout and the filter coasts.  `dt` is the time between calls (the loops' control period),
    `L_a`, `L_b` the solver model's axle distances (kmpc_config's defaults).
    `params` [B,8] (ESTIMATOR_PARAM_FIELDS), `record` [B,16] (ESTIMATOR_FIELDS; all zeros = fresh) and `flags` [B] int32 (EST_* bits of the last
    call) are plain device tensors the caller may edit between calls; `innov` [B,4] holds the last call's normalised innovations nu / sqrt(S)."""

    def __init__(self, B, q=(0.02, 0.02, 0.01, 0.1), r=(0.2, 0.2, 0.02, 0.1), gate=0.0, dt=0.1, L_a=1.108, L_b=1.742, device=0):
        self._lib = _lib.load()
        self.B = int(B)
        rows = fill_blocks("Estimator", np.zeros((self.B, 8)), (("q", q, 0, 4), ("r", r, 4, 4)), "four values (x, y, psi, v)")
        if not np.isfinite(rows).all() or not (rows[:, 0:4] >= 0.0).all() or not (rows[:, 4:8] > 0.0).all():
            raise ValueError("Estimator: q and r must be finite, q >= 0, r > 0")
        self.gate, self.dt, self.L_a, self.L_b = _filter_scalars("Estimator", gate, dt, L_a, L_b)
        self.device = device_of(device)
        self.params = torch.as_tensor(rows).to(self.device)
        self.record = torch.zeros((self.B, 16), dtype=torch.float64, device=self.device)
        self.flags = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        self.innov = torch.zeros((self.B, 4), dtype=torch.float64, device=self.device)

    @classmethod
    def from_sensor(cls, sensor, q=(0.02, 0.02, 0.01, 0.1), r_floor=(1e-3, 1e-3, 1e-4, 1e-3), **kw):
        """r = the sensor's sigma per vehicle and channel, floored at `r_floor` (a noiseless channel still needs r > 0); B and device are the
        sensor's.  Reads sensor.params once, here (one download)."""
        floor = np.asarray(r_floor, dtype=np.float64)
        if floor.shape not in ((), (4,)) or not np.isfinite(floor).all() or not (floor > 0.0).all():
            raise ValueError("Estimator.from_sensor: r_floor is a positive scalar or four positive values")
        sigma = sensor.params[:, 0:4].detach().cpu().numpy()
        return cls(sensor.B, q=q, r=np.maximum(sigma, floor), device=sensor.device, **kw)

    def reset(self):
        """every record fresh: the next update initialises from its measurement"""
        self.record.zero_()
        self.flags.zero_()
        self.innov.zero_()

    def update(self, z, u, out=None):
        """z [B,4]: this period's measurement x, y, psi, v; u [B,2]: (acc, d_f) in force since the last call -- a contiguous [B,2] tensor or a
        column view such as sim.state[:, 6:8] (rows any fixed distance >= 2 apart: no copy is made) -> est [B,4], the filtered state"""
        est = out if out is not None else torch.empty((self.B, 4), dtype=torch.float64, device=self.device)
        for t, w in ((z, 4), (self.params, 8), (self.record, 16), (est, 4), (self.innov, 4)):
            if not is_buffer(t, torch.float64, (self.B, w), self.device):
                raise ValueError("z [B,4], params [B,8], record [B,16], est [B,4] and innov [B,4] must be contiguous float64 tensors on %s" % self.device)
        stride = _filter_input(self.flags, u, self.B, self.device)
        _lib.check(self._lib.kmpc_estimate_batch(self.device.index, self.B, ptr(self.record), ptr(z), ptr(u), stride, ptr(self.params), self.dt, self.L_a,
                                                 self.L_b, self.gate, ptr(est), ptr(self.innov), ptr(self.flags), stream(self.device)))
        return est


class DisturbanceObserver:
    """The estimator's filter on the solver's model augmented with three constant disturbances (kmpc_observe_batch; include/kmpc.h states the
    arithmetic): a course offset dpsi (crab angle under bank, yaw bias), a steering offset ddelta and an acceleration offset da (grade).  A bank, a
    misaligned steering or a grade is a constant model error that no weight of the controller removes and that `Estimator` makes worse; this stage
    estimates it, hands the solver the heading along which the vehicle really travels (`psi + clip(dpsi, psi_cap)`) and, in `offset()`, takes
    ddelta and da out of the command (kmpc_cmd_offset_batch, capped at `df_cap`, `acc_cap`).
    `q`, `r`: as Estimator's; `q_dist`: random-walk standard deviations PER CALL of dpsi, ddelta, da; `p0`: their initial standard deviations -- a
    scalar, three values or [B,3].  `v_min`: below this estimated speed dpsi and ddelta are frozen (unobservable at rest).
    The defaults are those of the CPU prototype loop (path3 at 6 m/s): with them a bank of 1.5 m/s^2 plus a steering offset of 0.03 rad leaves
    0.022 m beside the path instead of 0.60 m; a larger q_dist follows a change faster and mistakes more of a corner's tyre slip for a disturbance.
    `params` [B,16] (OBSERVER_PARAM_FIELDS), `record` [B,40] (all zeros = fresh), `dist` [B,3] (dpsi, ddelta, da of the last call), `innov` [B,4] and
    `flags` [B] int32 (EST_* bits) are plain device tensors the caller may edit between calls."""

    def __init__(self, B, q=(0.02, 0.02, 0.01, 0.1), q_dist=(0.002, 0.002, 0.02), r=(0.2, 0.2, 0.02, 0.1), p0=(0.05, 0.05, 0.5), gate=0.0, dt=0.1,
                 v_min=1.0, psi_cap=0.2, acc_cap=0.5, df_cap=0.1, L_a=1.108, L_b=1.742, device=0):
        self._lib = _lib.load()
        self.B = int(B)
        rows = fill_blocks("DisturbanceObserver", np.zeros((self.B, 16)), (("q", q, 0, 4), ("q_dist", q_dist, 4, 3), ("r", r, 7, 4), ("p0", p0, 11, 3)))
        if not np.isfinite(rows).all() or not (rows[:, 0:7] >= 0.0).all() or not (rows[:, 7:11] > 0.0).all() or not (rows[:, 11:14] >= 0.0).all():
            raise ValueError("DisturbanceObserver: q, q_dist, r and p0 must be finite, q >= 0, q_dist >= 0, r > 0, p0 >= 0")
        self.gate, self.dt, self.L_a, self.L_b = _filter_scalars("DisturbanceObserver", gate, dt, L_a, L_b)
        self.v_min, self.psi_cap, self.acc_cap, self.df_cap = float(v_min), float(psi_cap), float(acc_cap), float(df_cap)
        caps = [self.v_min, self.psi_cap, self.acc_cap, self.df_cap]
        if not (np.isfinite(caps).all() and min(caps) >= 0.0):
            raise ValueError("DisturbanceObserver: v_min, psi_cap, acc_cap, df_cap >= 0, all finite (got %r, %r, %r, %r)" % (v_min, psi_cap, acc_cap, df_cap))
        self.device = device_of(device)
        self.params = torch.as_tensor(rows).to(self.device)
        self.record = torch.zeros((self.B, 40), dtype=torch.float64, device=self.device)
        self.flags = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        self.innov = torch.zeros((self.B, 4), dtype=torch.float64, device=self.device)
        self.dist = torch.zeros((self.B, 3), dtype=torch.float64, device=self.device)

    def reset(self):
        """every record fresh: the next update initialises from its measurement, with zero disturbances"""
        self.record.zero_()
        self.flags.zero_()
        self.innov.zero_()
        self.dist.zero_()

    def _own(self):
        for t, w in ((self.params, 16), (self.record, 40)):
            if not is_buffer(t, torch.float64, (self.B, w), self.device):
                raise ValueError("params [B,16] and record [B,40] must stay contiguous float64 tensors on %s" % self.device)

    def update(self, z, u, out=None):
        """z [B,4]: this period's measurement x, y, psi, v; u [B,2]: the (acc, d_f) that acted since the last call -- sim.state[:, 6:8] or the command
        as sent, after offset() (as Estimator.update: a column view is not copied) -> est [B,4]: x, y, psi + clip(dpsi, psi_cap), v"""
        est = out if out is not None else torch.empty((self.B, 4), dtype=torch.float64, device=self.device)
        self._own()
        for t, w in ((z, 4), (est, 4), (self.innov, 4), (self.dist, 3)):
            if not is_buffer(t, torch.float64, (self.B, w), self.device):
                raise ValueError("z [B,4], est [B,4], innov [B,4] and dist [B,3] must be contiguous float64 tensors on %s" % self.device)
        stride = _filter_input(self.flags, u, self.B, self.device)
        _lib.check(self._lib.kmpc_observe_batch(self.device.index, self.B, ptr(self.record), ptr(z), ptr(u), stride, ptr(self.params), self.dt, self.L_a,
                                                self.L_b, self.gate, self.v_min, self.psi_cap, ptr(est), ptr(self.dist), ptr(self.innov), ptr(self.flags),
                                                stream(self.device)))
        return est

    def offset(self, cmd, stop_latch=None):
        """cmd [B,2] (accel, steer), in place: accel -= clip(da, acc_cap), steer -= clip(ddelta, df_cap); a vehicle whose `stop_latch` [B] (bool or
        uint8) is set, whose record is fresh or whose estimate is not finite keeps its command -> cmd"""
        self._own()
        if not is_buffer(cmd, torch.float64, (self.B, 2), self.device):
            raise ValueError("cmd must be a contiguous float64 tensor [B,2] on %s" % self.device)
        if stop_latch is not None and not is_buffer(stop_latch, (torch.bool, torch.uint8), (self.B,), self.device):
            raise ValueError("stop_latch must be a contiguous bool or uint8 tensor [B] on %s" % self.device)
        _lib.check(self._lib.kmpc_cmd_offset_batch(self.device.index, self.B, ptr(self.record), ptr(stop_latch), self.acc_cap, self.df_cap, ptr(cmd),
                                                   stream(self.device)))
        return cmd


class LatencyCompensator:
    """The controller's answer to dead time (kmpc_cmd_in_force_batch, kmpc_predict_ahead_batch; include/kmpc.h states the rules).  It keeps a log
    of the commands it sent, `cmd_hist` [depth,B,2] (slot p mod depth: period p's command, written by push() after the command stage), and its own
    ASSUMED delays: `cmd_delay` [B] int32 in model updates of 10 ms and `meas_delay` [B] int32 in whole control periods -- separate tensors from the
    plant's and the sensor's, so that a run can have a delay mismatch.  All three are plain device tensors the caller may edit between periods;
    the delays are clamped into `max_cmd_delay` / `max_meas_delay`, the largest values given here (plain ints; raise them only as far as
    depth >= max_meas_delay + ceil(max_cmd_delay / n_updates) + 1 allows: the library refuses more).  `depth` defaults to exactly that.
    `n_updates`: plant updates per control period; `L_a`, `L_b`: the solver model's axle distances (kmpc_config's defaults).
      filter_input(period)   -> u [B,2]: the command in force over the period before the measurement's moment: the estimator's predict input
      predict(z, period)     -> z [B,4] carried from the measurement's moment, update (period - meas_delay) n, to update period n + cmd_delay, where
                                this period's command begins to act; zero delays return z bit for bit
      push(cmd, period)      logs period's command [B,2]
    `disturbances=True` makes it the partner of a DisturbanceObserver (kmpc_predict_ahead_dist_batch): the closed loops accept observer= together
    with compensator= only then, and
      predict_disturbed(observer, est, period) -> z [B,4]: the same steps on the observer's augmented model, from the observer's record: travel
                                along psi + dpsi + beta, steering d_f + ddelta, acceleration acc + da, the three held constant; the heading
                                returned is est_out's, psi + clip(dpsi, psi_cap).  `est` [B,4] (the observer's est_out) is what a vehicle with a
                                fresh record gets back; zero delays return est_out bit for bit.
    The observer's random walk must slow as the dead time grows (about 0.25 x the default q_dist at 0.35 s)."""

    def __init__(self, B, cmd_delay=0, meas_delay=0, n_updates=10, depth=None, L_a=1.108, L_b=1.742, device=0, disturbances=False):
        if not isinstance(disturbances, (bool, np.bool_)):
            raise ValueError("LatencyCompensator: disturbances is True or False, got %r" % (disturbances,))
        self.disturbances = bool(disturbances)
        self._lib = _lib.load()
        self.B = int(B)
        if isinstance(n_updates, bool) or not isinstance(n_updates, (int, np.integer)) or n_updates < 1:
            raise ValueError("LatencyCompensator: n_updates is an integer >= 1, got %r" % (n_updates,))
        self.n_updates = int(n_updates)
        cd = _int_per_vehicle("LatencyCompensator: cmd_delay (model updates of 10 ms)", cmd_delay, self.B, 0)
        md = _int_per_vehicle("LatencyCompensator: meas_delay (control periods)", meas_delay, self.B, 0)
        self.max_cmd_delay, self.max_meas_delay = (int(cd.max()), int(md.max())) if self.B else (0, 0)
        need = self.max_meas_delay + -(-self.max_cmd_delay // self.n_updates) + 1
        if depth is None:
            depth = need
        if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or depth < need:
            raise ValueError("LatencyCompensator: depth is an integer >= max meas_delay + ceil(max cmd_delay / n_updates) + 1 = %d, got %r" % (need, depth))
        self.depth = int(depth)
        self.L_a, self.L_b = float(L_a), float(L_b)
        if not (np.isfinite([self.L_a, self.L_b]).all() and self.L_a > 0.0 and self.L_b > 0.0):
            raise ValueError("LatencyCompensator: L_a > 0, L_b > 0, finite (got %r, %r)" % (L_a, L_b))
        self.device = device_of(device)
        self.cmd_delay, self.meas_delay = cd.to(self.device), md.to(self.device)
        self.cmd_hist = torch.zeros((self.depth, self.B, 2), dtype=torch.float64, device=self.device)

    def _check(self, period):
        for t, shape, dt in ((self.cmd_delay, (self.B,), torch.int32), (self.meas_delay, (self.B,), torch.int32),
                             (self.cmd_hist, (self.depth, self.B, 2), torch.float64)):
            if not is_buffer(t, dt, shape, self.device):
                raise ValueError("cmd_delay, meas_delay [B] int32 and cmd_hist [depth,B,2] float64 must stay contiguous tensors on %s" % self.device)
        if int(period) < 0:
            raise ValueError("period >= 0")

    def _log(self, period):
        """the command log and the assumed delays as the three kernels take them: cmd_hist, depth, period, n_updates, the delays and their bounds"""
        return (ptr(self.cmd_hist), self.depth, int(period), self.n_updates, ptr(self.cmd_delay), ptr(self.meas_delay), int(self.max_cmd_delay),
                int(self.max_meas_delay))

    def _buf(self, t, w, name):
        if not is_buffer(t, torch.float64, (self.B, w), self.device):
            raise ValueError("%s must be a contiguous float64 tensor [B,%d] on %s" % (name, w, self.device))
        return t

    def filter_input(self, period, out=None):
        self._check(period)
        u = self._buf(out, 2, "out") if out is not None else torch.empty((self.B, 2), dtype=torch.float64, device=self.device)
        _lib.check(self._lib.kmpc_cmd_in_force_batch(self.device.index, self.B, *self._log(period), ptr(u), stream(self.device)))
        return u

    def predict(self, z, period, out=None):
        self._check(period)
        self._buf(z, 4, "z")
        zo = self._buf(out, 4, "out") if out is not None else torch.empty((self.B, 4), dtype=torch.float64, device=self.device)
        _lib.check(self._lib.kmpc_predict_ahead_batch(self.device.index, self.B, ptr(z), *self._log(period), self.L_a, self.L_b, ptr(zo), stream(self.device)))
        return zo

    def check_observer(self, observer):
        """refuse an observer this compensator cannot predict for: another fleet size, device or model geometry"""
        if not self.disturbances:
            raise ValueError("LatencyCompensator: predict_disturbed needs LatencyCompensator(..., disturbances=True)")
        if not isinstance(observer, DisturbanceObserver):
            raise ValueError("LatencyCompensator: observer is a vehicle_sim.DisturbanceObserver, got %r" % (type(observer).__name__,))
        if observer.B != self.B or observer.device != self.device or observer.L_a != self.L_a or observer.L_b != self.L_b:
            raise ValueError("LatencyCompensator: the observer has B=%d on %s with L_a=%r, L_b=%r, the compensator B=%d on %s with L_a=%r, L_b=%r: "
                             "they must agree" % (observer.B, observer.device, observer.L_a, observer.L_b, self.B, self.device, self.L_a, self.L_b))

    def predict_disturbed(self, observer, est, period, out=None):
        self.check_observer(observer)
        self._check(period)
        observer._own()
        self._buf(est, 4, "est")
        zo = self._buf(out, 4, "out") if out is not None else torch.empty((self.B, 4), dtype=torch.float64, device=self.device)
        _lib.check(self._lib.kmpc_predict_ahead_dist_batch(self.device.index, self.B, ptr(observer.record), ptr(est), *self._log(period), self.L_a, self.L_b,
                                                           observer.psi_cap, ptr(zo), stream(self.device)))
        return zo

    def push(self, cmd, period):
        self._check(period)
        self.cmd_hist[int(period) % self.depth].copy_(self._buf(cmd, 2, "cmd"))
