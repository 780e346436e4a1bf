"""Closed loop of launch/sim_path_follow.launch for B vehicles at once, entirely on the device:
state_est (vehicle_sim.VehicleSimulator) -> waypoints (ref_traj.GPSRefTrajectory) -> MPC (solver.BatchMPC, warm-started)
-> MPC_cmd -> simulator.  One `step()` is one pass of the 10 Hz loop of mpc_cmd_pub.jl:88-153 for every vehicle,
followed by 0.1 s of plant time (10 model updates at 100 Hz, vehicle_simulator.py:24-26).

Protocol details kept from the reference node: the command is published regardless of the solver status (Q7); the
rate-limit anchor is the last *command*, not the measured actuator state (:140, Q7); the stop flag of the waypoint
helper latches and overrides the command with accel -1.0 / steer 0.0 (:100-103, :148-153), per vehicle; warm start
from the previous primal solution (JuMP keeps values, Q9).

Fleets on several recorded paths: `grt` may be a ref_traj.FleetRefTrajectory, which gives every vehicle a path and a tracking mode of its own, and
`target_vel` may be a length-B sequence.  The loops then always hand the helper `v_target`; the helper owns the modes.  Re-routing a vehicle
(editing grt.path_id[b]) does NOT clear its stop latch: a vehicle that latched at the end of its old path stays braked until the caller clears
`loop.command_stop[b]`.

Episodes and scores: `run(steps)` runs `steps` periods without a host synchronisation or a device -> host copy and scores every state on the device
(ref_traj.track_score_batch: tracking errors on the vehicle's recorded path and a running record per vehicle, `loop.score` [B,16]);
`score_summary()` downloads the record once.  `step()` alone never scores.

Monte-Carlo runs: `sensor=vehicle_sim.SensorModel(...)` puts a measurement stage between the plant and the controller.  Waypoints, the Frenet fit
and the solve's initial state then read `loop.est` [B,4] (the plant's x, y, psi, v as sensed in period `loop.k`: bias + seeded Gaussian noise per
vehicle) instead of `sim.state`; scoring, the history's `state` and the plant stay on the truth.  A plant per vehicle and a command delay belong
to the simulator (VehicleSimulator(plant=, cmd_delay=)).  Without a sensor the loops take exactly the code path they always took.

State estimation: `estimator=vehicle_sim.Estimator(...)` puts an extended Kalman filter per vehicle between the measurement (the sensor's `loop.est`,
or the truth without a sensor) and the controller.  Waypoints, fit and solve then read `loop.est_filt` [B,4]; `loop.est` stays the raw measurement.
`estimator_input` names the (acc, d_f) the filter predicts with: "actuator" -- `sim.state[:, 6:8]`, the a and df that state_est publishes -- or
"command", the command sent in the previous period (`sim.cmd` before this period's command stage overwrites it).  The estimator's `dt` must be the
control period (plant_updates x 10 ms) and its L_a, L_b the solver's.  Without an estimator nothing changes.

Offset-free loops: `observer=vehicle_sim.DisturbanceObserver(...)` takes the estimator's place in the period -- waypoints, fit and solve read its
`loop.est_filt` [B,4] (the heading shifted by the estimated course offset), `loop.dist` [B,3] is the estimate of (dpsi, ddelta, da) -- and its
`offset()` runs between the command stage and the plant, in place on `sim.cmd`: the plant (and `estimator_input="command"`) sees the corrected
command, the solver's rate-limit anchor `u_prev` stays the solver's own.  `observer=` together with `estimator=` is refused.
Without an observer the loops run the code they ran before.

Offset-free loops under dead time: `observer=` together with `compensator=vehicle_sim.LatencyCompensator(..., disturbances=True)`.  The period is
sense -> observer.update(z, u) -> compensator.predict_disturbed(observer, est_filt, k) -> `loop.est_pred` -> waypoints / fit / solve -> command ->
observer.offset -> compensator.push: the prediction runs on the observer's augmented model (kmpc_predict_ahead_dist_batch: travel along
psi + dpsi + beta, steering d_f + ddelta, acceleration acc + da), and the log holds the command AS SENT, after the offset, so that "logged command +
disturbance" is what acted.  `estimator_input="history"` then feeds the observer the logged command in force (the choice under dead time; it
ignores the actuator lag, which reaches the observer as a small disturbance).  A plain LatencyCompensator with `observer=` stays refused, and so
does `disturbances=True` without `observer=`.  The observer's q_dist must shrink as the dead time grows: about 0.25 x the default at 0.35 s, the
default up to 0.1 s; no automatic rule is built.  `run(history=True)` carries est_filt, dist and est_pred together.

Latency: the plant's command queue and the sensor's stale fixes belong to the simulator and the sensor (VehicleSimulator(cmd_queue_depth=),
SensorModel(meas_delay=)).  `compensator=vehicle_sim.LatencyCompensator(...)` is the controller's side: the period's state passes
sense -> filter -> compensator.predict and becomes `loop.est_pred` [B,4], the state at the update from which this period's command will act (under the
compensator's ASSUMED delays and its log of sent commands); waypoints, fit and solve read it.  After the command stage `compensator.push(sim.cmd, k)`
logs the command.  `estimator_input="history"` feeds the filter `compensator.filter_input(k)`, the logged command in force over the period the filter
steps across (refused without a compensator).  Scoring, the history's `state` and the plant stay on the truth; nothing synchronises.  The
compensator's n_updates must be the loop's plant_updates (checked every period).  Without a compensator the loops take exactly the path they took.

Speed plan: `planner=ref_traj.SpeedPlanner(grt, ...)` (grt a FleetRefTrajectory, every vehicle in target-velocity mode) runs in front of the waypoint
stage, on the state the controller reads (truth, est, est_filt or est_pred), with `v_target` as the cap: `loop.v_plan` [B] replaces `v_target` in BOTH
the waypoint call (the spacing is how the XY model follows a speed at C_v = 0) and the solve of that period.  `v_target` and `des_speed` are not
modified; stop latch, rate-limit anchor, command stage and scoring are untouched.  Without a planner nothing changes.

Sensor faults: with `sensor=SensorModel(..., faults=fault_params(...))` a source can fall silent.  A filter (estimator= or observer=) is then fed
`sensor.z`, NaN in a silent source's channels, and coasts; without a filter the controller reads the held state, the last delivered value of every
channel -- the reference's publisher -- and `loop.est` stays what that publisher would have published.  `blind_stop=True` ORs `sensor.blind` (a
source silent for longer than the row's max_age) into the waypoint helper's stop flags ahead of the command stage, so a blind vehicle latches and
brakes like one at the end of its path.  Loops without faults= run the code they ran before.

L0 actuation: the reference's low-level controller and a pedal-driven powertrain belong to the simulator (VehicleSimulator(drive=, llc=):
kmpc_sim_advance_drive runs the controller's 50 Hz tick inside the plant call).  The loops only call `sim._update_vehicle_model`; `sim.state[:, 6]`
is then the powertrain's net acceleration, which `estimator_input="actuator"` reads as delivered, while `estimator_input="command"` lets an
observer see the difference between what was commanded and what the pedals delivered.

Coloured noise and gusts: `wander=vehicle_sim.Wander(B, wander_params(...))` runs first in every period (kmpc_wander_batch, one launch): eight
Gauss-Markov processes per vehicle are advanced to period `loop.k` and added to the sensor's biases and the road's a_long, a_lat, df_offset.  With a
sensor the caller's sensor rows move to `sensor.params_base` and `sensor.params` -- what the sense kernels read -- is rewritten every period; with a
road the caller's rows are `sim.road_base` and the stage writes `sim.road` (in front of a road profile: base -> wander -> profile -> `sim.road`).
Active measurement channels without sensor=, or active road channels without a simulator built with road=, are refused at construction.
`run(history=True)` adds `wander` [steps,B,8].  Without wander= there is no launch and no tensor more.

Car following: `follower=ref_traj.Follower(grt, ...)` (built on the loop's own waypoint helper, every vehicle in target-velocity mode) makes the
vehicles exist for each other: in front of the speed plan, `follower.cap(sim.state, v_target)` gives `loop.v_follow` [B], v_target lowered where the
vehicle ahead on the same path demands it (kmpc_follow_fleet, include/kmpc_follow.h).  With a planner that is the plan's cap (`planner.plan(st,
v_follow)`), without one it is the period's speed for waypoints and solve.  The range sensor is perfect: the stage reads the truth, `sim.state`, for
the arclengths and both speeds, whatever state the controller reads.  `v_target` and `des_speed` are not modified.  `run(history=True)` adds
`v_follow` [steps,B] and `gap` [steps,B].  Without follower= there is no launch and no tensor more.
A follower with a range sensor, `Follower(grt, rows, radar=ref_traj.RangeSensor(B, ...))`, no longer reads the truth: behind the search,
kmpc_range_follow_batch (include/kmpc_range.h) measures the gap and the leader's speed (range limit, bias, seeded noise, dropouts), tracks them, and
applies the law to what the track believes, with the follower's own speed from the state the CONTROLLER reads (sensed, filtered or predicted,
whichever the loop has) -- `follower.cap(sim.state, v_target, known=st, k=loop.k, dt=plant_updates x 10 ms)`.  `follower.stat` and `gap` stay the
truth's; `follower.v_ideal` is what a perfect sensor would have said.  `run(history=True)` adds `gap_seen` and `v_lead_seen` [steps,B] (+inf and
0 without a track).  A follower without a radar, and lanes=, launch and allocate nothing more (lanes= has no radar: its decision is fused with
its search).

Lanes: `lanes=ref_traj.Lanes(grt, ...)` takes the follower's place (the two together are refused) and gives every vehicle a lateral degree of
freedom: in front of the speed plan, `lanes.step(sim.state, v_target, k, dt)` (kmpc_lane_step_fleet, include/kmpc_lanes.h; dt = plant_updates x
10 ms) finds the leader among the vehicles in the vehicle's own lane(s), decides lane changes and ramps the commanded offset; `loop.v_follow` is its
cap, used as the follower's is.  Between the waypoint call and the solve -- in the Frenet loop before the fit -- `lanes.shift(ref)` moves the
period's waypoints by that offset to the left (kmpc_ref_offset_batch), so both models steer to the lane's line.  The stage reads the truth, as
follower= does.  `loop.score` stays against the RECORDED line (a vehicle in lane 1 shows e_ct near one lane width); the error against the
commanded offset lives in the stage's own record (`lanes.summary()`: sum_elane2, max_elane).  Lanes are offsets of one recorded path: the speed
along an offset line differs by 1 - kappa * d and nothing corrects for it, and a speed plan uses the centre line's curvature.
`run(history=True)` adds `v_follow`, `gap`, `lane` and `lane_offset` [steps,B].  Without lanes= there is no launch and no tensor more.

Large fleets: `Follower(grt, ..., search="sorted")` and `Lanes(grt, ..., search="sorted")` order the fleet once per period and search along the order
(include/kmpc_order.h) instead of searching every pair -- the same results bit for bit, O(B log B), faster from a few tens of thousands of
vehicles on.  The loops take either; nothing else changes, and no host round trip is added.
"""
import time

import numpy as np
import torch

from . import _lib
from ._stage import is_buffer, ptr, record_fields, stream
from .kinematic_mpc_frenet import get_reference_frenet_batch
from .ref_traj import SCORE_FIELDS, FleetRefTrajectory, fresh_score
from .solver import BatchMPC
from .vehicle_sim import Wander

FRENET_WEIGHTS = (0.0, 9.0, 10.0, 0.5, 100.0, 1000.0, 0.0, 0.0)   # MKZMPCPathFollowerFrenet.jl:51-59 in update_cost's 8-slot layout (no x slot)


def _target_speeds(target_vel, B, device):
    """mpc_cmd_pub.jl:58-62, per vehicle: des_speed = target_vel if target_vel > 0 else 0 -> (des_speed, v_target [B] on the device).
    A scalar target_vel gives a float des_speed, a length-B sequence or tensor a tuple of B floats."""
    if isinstance(target_vel, (int, float)):
        des = float(target_vel) if target_vel > 0.0 else 0.0
        return des, torch.full((B,), des, dtype=torch.float64, device=device)
    tv = torch.as_tensor(target_vel, dtype=torch.float64).detach().cpu()
    if tv.dim() == 0:
        return _target_speeds(float(tv), B, device)
    if tuple(tv.shape) != (B,):
        raise ValueError("target_vel: a scalar or one speed per vehicle [%d], got %s" % (B, tuple(tv.shape)))
    tv = torch.where(tv > 0.0, tv, torch.zeros_like(tv))
    return tuple(tv.tolist()), tv.to(device)


class _ScoredLoop:
    """The control period, run() / score / score_summary() of both loops.  A loop provides the one step in which they differ,
    _reference(st) -> (ref, stop, solve, extra): the reference built from the controller's state `st`, the helper's stop flags, the solve as a
    call without arguments -> the solver's output dict, and the entries the loop adds to step()'s dict."""

    def _init_loop(self, params, sensor, estimator, estimator_input, compensator, observer, planner=None, track_with_time=False, blind_stop=False,
                   wander=None, follower=None, lanes=None):
        """what both loops own beside grt, sim, N, B, mpc and the target speeds: buffers, the stop latch, the library, and the stages; and the one
        check of the helper against the plant that both word alike (a loop's own refusals, worded for that loop, come before this call)"""
        dev = self.sim.device
        if self.grt.device != dev:
            raise ValueError("waypoint helper on %s, plant on %s: the loop runs on one device" % (self.grt.device, dev))
        self.u_prev = torch.zeros((self.B, 2), dtype=torch.float64, device=dev)       # (acc, d_f): update_current_input starts at 0
        self.warm_U = torch.zeros((self.B, self.N, 2), dtype=torch.float64, device=dev)
        self.command_stop = torch.zeros((self.B,), dtype=torch.bool, device=dev)   # the stop latch (one byte per vehicle: kmpc_command_batch's uint8)
        self._lib = _lib.load()
        # per-vehicle weights and limits [B,16] (BatchMPC.problem_params), owned by the caller: it may be edited between steps (gain scheduling,
        # a new speed limit); None = the solver handle's values for every vehicle
        self.params = params
        self.have_warm = False
        self.out = None
        self.k = 0
        self._init_sensor(sensor, blind_stop)
        self._init_wander(wander)
        self._init_estimator(estimator, estimator_input, compensator, observer)
        self._init_planner(planner, track_with_time)
        self._init_follower(follower, track_with_time)
        self._init_lanes(lanes, track_with_time)
        self._init_score()

    def _period(self, plant_updates, time_solve):
        """one control period -> step()'s dict: wander -> sense -> filter -> predict -> reference and solve (the loop's own) -> command stage ->
        offset -> log -> plant"""
        self._plant_updates = plant_updates
        if self.wander is not None:   # this period's coloured errors and gusts, into the rows the sense and the plant call below read
            self.wander.step(self.k, *self._wander_rows)
        st = self.sim.state if self.sensor is None else self._sense()
        if self.estimator is not None or self.observer is not None:
            st = self._filter(self.sensor.z if self.faulty else st)   # a faulty sensor's z: NaN where a source is silent, the filter coasts
        if self.compensator is not None:
            st = self._predict(st, plant_updates)
        ref, stop, solve, extra = self._reference(st)
        if self.blind_stop:   # blind for longer than MAX_AGE: latch and brake like a vehicle at the end of its path (on the device, no synchronisation)
            stop = torch.bitwise_or(stop, self.sensor.blind.to(stop.dtype))
        if time_solve:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        self.out = solve()
        solve_s = None
        if time_solve:
            torch.cuda.synchronize()
            solve_s = time.perf_counter() - t0
        self.have_warm = True
        # stop latch (:100-103), command selection (:148-153) and update_current_input (:140, only on the solve branch): one kernel, straight
        # into the plant's command buffer
        cmd = self.sim.cmd
        u0 = self.out["u0"]
        assert is_buffer(u0, torch.float64, (self.B, 2), cmd.device)
        _lib.check(self._lib.kmpc_command_batch(cmd.device.index, self.B, ptr(u0), ptr(stop), ptr(self.command_stop), ptr(self.u_prev), ptr(cmd),
                                                stream(cmd.device)))
        if self.observer is not None:
            self.observer.offset(cmd, self.command_stop)
        if self.compensator is not None:
            self.compensator.push(cmd, self.k)
        self.sim._update_vehicle_model(plant_updates)
        self.k += 1
        return dict(ref=ref, cmd=cmd, status=self.out["status"], iters=self.out["iters"], cost=self.out["cost"], solve_s=solve_s, **extra)

    def _same_fleet(self, name, stage):
        """a stage built for another fleet size or on another device than the plant's is refused, every stage in the same words"""
        if stage.B != self.B or stage.device != self.sim.device:
            raise ValueError("%s for %d vehicles on %s, plant with %d on %s" % (name, stage.B, stage.device, self.B, self.sim.device))

    def _init_path_stage(self, name, stage, track_with_time, does, built, must_have=None):
        """what a stage on the helper's arclength grid (planner=, follower=, lanes=) must be, checked in this order: no time grid; built on this
        loop's own helper (and, `must_have` given, with that method: lanes= is told from a follower by its shift()); for the plant's fleet; every
        vehicle in target-velocity mode.  `does` and `built`: the stage's own words for the first two refusals."""
        if track_with_time:
            raise ValueError("%s= %s: track_with_time must stay False" % (name, does))
        if getattr(stage, "fleet", None) is not self.grt or (must_have is not None and not hasattr(stage, must_have)):
            raise ValueError("%s= must be a ref_traj.%s" % (name, built))
        self._same_fleet(name, stage)
        if getattr(self.grt, "time_mode", None) is not None and bool(self.grt.time_mode.any().item()):
            raise ValueError("%s= needs every vehicle in target-velocity mode: the fleet helper has vehicles in time mode" % name)

    def _init_planner(self, planner, track_with_time):
        if planner is not None:
            self._init_path_stage("planner", planner, track_with_time, "plans a speed along the arclength grid",
                                  "SpeedPlanner built on this loop's own waypoint helper (a FleetRefTrajectory)")
        self.planner = planner
        self.v_plan = None     # [B] the planned speed of the last period (planner given): waypoint spacing and the solver's v_target

    def _init_follower(self, follower, track_with_time):
        if follower is not None:
            self._init_path_stage("follower", follower, track_with_time, "caps a speed on the arclength grid",
                                  "Follower built on this loop's own waypoint helper")
        self.follower = follower
        self.v_follow = None   # [B] v_target under the following law, of the last period (follower given): the plan's cap, or the period's speed

    def _init_lanes(self, lanes, track_with_time):
        if lanes is not None:
            if self.follower is not None:
                raise ValueError("lanes= takes the follower's place (its leaders are found by lane): give no follower=")
            self._init_path_stage("lanes", lanes, track_with_time, "caps a speed on the arclength grid",
                                  "Lanes built on this loop's own waypoint helper", must_have="shift")
        self.lanes = lanes
        self._plant_updates = 10

    def _speed(self, st):
        """the speed this period's waypoints and solve run at: v_target; with a follower loop.v_follow, v_target lowered by the following law on
        the TRUTH (a perfect range sensor) or, when the follower has a radar, on its track of a measured gap; with a planner loop.v_plan, planned
        on the state the controller reads with that as the cap (v_target itself is not modified)"""
        cap = self.v_target
        if self.follower is not None:
            if getattr(self.follower, "radar", None) is None:
                cap = self.v_follow = self.follower.cap(self.sim.state, self.v_target, out=self.v_follow)
            else:   # a measured gap, and the follower's own speed from the state the controller reads; dt as for the lanes
                cap = self.v_follow = self.follower.cap(self.sim.state, self.v_target, out=self.v_follow, known=st, k=self.k,
                                                        dt=0.01 * self._plant_updates)
        elif self.lanes is not None:   # dt: the period the plant is about to run, plant_updates x 10 ms
            cap = self.v_follow = self.lanes.step(self.sim.state, self.v_target, self.k, 0.01 * self._plant_updates, out=self.v_follow)
        if self.planner is None:
            return cap
        self.v_plan = self.planner.plan(st, cap, out=self.v_plan)
        return self.v_plan

    def _init_sensor(self, sensor, blind_stop=False):
        if sensor is not None:
            self._same_fleet("sensor", sensor)
        self.sensor = sensor
        self.faulty = sensor is not None and getattr(sensor, "faults", None) is not None   # SensorModel(faults=): z, flags, blind beside the held state
        if blind_stop and not self.faulty:
            raise ValueError("blind_stop=True reads the sensor's blind flags: give sensor=SensorModel(..., faults=...)")
        self.blind_stop = bool(blind_stop)
        self.est = None   # [B,4] x, y, psi, v as sensed in the last period (sensor given)

    def _init_wander(self, wander):
        """wander=: the Gauss-Markov stage in front of the sense.  The sensor pair is composed whenever the loop has a sensor, the road pair whenever
        the simulator has a road; a channel that is on without its consumer is refused here, on the host rows the stage was built from."""
        self.wander, self._wander_rows = wander, None
        if wander is None:
            return
        if not (isinstance(wander, Wander) and wander.B == self.B and wander.device == self.sim.device):
            raise ValueError("wander= is a vehicle_sim.Wander for %d vehicles on %s" % (self.B, self.sim.device))
        if wander.sensor_active and self.sensor is None:
            raise ValueError("wander= has active measurement channels (x, y, psi, v): give sensor=SensorModel(...), whose biases they are added to")
        if wander.road_active and self.sim.road is None:
            raise ValueError("wander= has active road channels (a_long, a_lat, df_offset): build the simulator with road= (road_params)")
        sensor_pair = road_pair = (None, None)
        if self.sensor is not None:
            if self.sensor.params_base is None:
                self.sensor.params_base, self.sensor.params = self.sensor.params, self.sensor.params.clone()
            sensor_pair = (self.sensor.params_base, self.sensor.params)
        if self.sim.road is not None:
            road_pair = self.sim.wander_road_buffers()
        self._wander_rows = sensor_pair + road_pair

    def _init_estimator(self, estimator, estimator_input, compensator=None, observer=None):
        if observer is not None:
            if estimator is not None:
                raise ValueError("observer= takes the estimator's place: give no estimator=")
            if compensator is not None and not getattr(compensator, "disturbances", False):
                raise ValueError("observer= with compensator= needs LatencyCompensator(..., disturbances=True): the prediction ahead must run on "
                                 "the observer's model")
            self._same_fleet("observer", observer)
            if compensator is not None:
                compensator.check_observer(observer)
        elif compensator is not None and getattr(compensator, "disturbances", False):
            raise ValueError("LatencyCompensator(disturbances=True) predicts on a DisturbanceObserver's model: give observer=")
        self.observer = observer
        self.dist = None       # [B,3] the estimated dpsi, ddelta, da of the last period (observer given): the observer's own tensor
        if estimator_input not in ("actuator", "command", "history"):
            raise ValueError("estimator_input: 'actuator', 'command' or 'history', got %r" % (estimator_input,))
        if estimator_input == "history" and compensator is None:
            raise ValueError("estimator_input='history' reads the compensator's command log: give compensator=")
        if compensator is not None:
            self._same_fleet("compensator", compensator)
        self.compensator = compensator
        self.est_pred = None   # [B,4] the state predicted ahead to where this period's command acts (compensator given)
        self._u_hist = None
        if estimator is not None:
            self._same_fleet("estimator", estimator)
        self.estimator, self.estimator_input = estimator, estimator_input
        self.est_filt = None   # [B,4] the filtered x, y, psi, v of the last period (estimator given)

    def _filter(self, st):
        """this period's measurement `st` (loop.est, or the plant's state without a sensor) -> loop.est_filt [B,4]"""
        z = st if st.shape[1] == 4 else st[:, 0:4].contiguous()
        if self.estimator_input == "history":
            u = self._u_hist = self.compensator.filter_input(self.k, out=self._u_hist)
        else:
            u = self.sim.state[:, 6:8] if self.estimator_input == "actuator" else self.sim.cmd
        if self.observer is not None:
            self.est_filt = self.observer.update(z, u, out=self.est_filt)
            self.dist = self.observer.dist
            return self.est_filt
        self.est_filt = self.estimator.update(z, u, out=self.est_filt)
        return self.est_filt

    def _predict(self, st, plant_updates):
        """what the controller holds of this period (measurement, estimate or the plant's state) -> loop.est_pred [B,4], predicted ahead"""
        if self.compensator.n_updates != int(plant_updates):
            raise ValueError("the compensator counts %d updates per period, this period has %d" % (self.compensator.n_updates, plant_updates))
        z = st if st.shape[1] == 4 else st[:, 0:4].contiguous()
        if self.observer is not None:   # on the observer's augmented model, from its record; z is its est_out
            self.est_pred = self.compensator.predict_disturbed(self.observer, z, self.k, out=self.est_pred)
            return self.est_pred
        self.est_pred = self.compensator.predict(z, self.k, out=self.est_pred)
        return self.est_pred

    def _sense(self):
        """this period's measurement of the plant -> loop.est [B,4]: what waypoints, fit and solve read in place of sim.state[:, 0:4]"""
        self.est = self.sensor.sense(self.sim.state, self.k, out=self.est)
        return self.est

    def _init_score(self):
        self.score = fresh_score(self.B, self.sim.device)   # [B,16], layout KMPC_SCORE_* of include/kmpc.h (ref_traj.SCORE_FIELDS)
        self.track = None                                   # err [B,4], seg [B], closest [B] of the last scored state
        self._score_fresh = True

    def reset_score(self):
        """a fresh record for every vehicle (the next run() from k == 0 scores the initial state again)"""
        self._init_score()

    def _score_state(self, o, settle_tol):
        side = {} if o is None else dict(status=o["status"], iters=o["iters"], cmd=o["cmd"], stop_latch=self.command_stop)
        self.track = self.grt.track_score_batch(self.sim.state, score=self.score, settle_tol=settle_tol, out=self.track, **side)
        self._score_fresh = False

    def _optional_history(self):
        """what run(history=True) records beside state, cmd, status and latch, for the stages this loop has: (key, trailing shape, dtype, source), in
        the order the keys appear in run()'s dict; source() is the tensor a period leaves behind"""
        f64 = torch.float64
        radar = self.follower is not None and getattr(self.follower, "radar", None) is not None
        rows = ((self.sensor is not None, "est", (4,), f64, lambda: self.est),
                (self.faulty, "z", (4,), f64, lambda: self.sensor.z),
                (self.faulty, "fault_flags", (), torch.int32, lambda: self.sensor.flags),
                (self.estimator is not None or self.observer is not None, "est_filt", (4,), f64, lambda: self.est_filt),
                (self.observer is not None, "dist", (3,), f64, lambda: self.dist),
                (self.compensator is not None, "est_pred", (4,), f64, lambda: self.est_pred),
                (self.planner is not None, "v_plan", (), f64, lambda: self.v_plan),
                (self.follower is not None, "v_follow", (), f64, lambda: self.v_follow),
                (self.follower is not None, "gap", (), f64, lambda: self.follower.gap),
                (radar, "gap_seen", (), f64, lambda: self.follower.gap_seen),
                (radar, "v_lead_seen", (), f64, lambda: self.follower.v_lead_seen),
                (self.lanes is not None, "v_follow", (), f64, lambda: self.v_follow),
                (self.lanes is not None, "gap", (), f64, lambda: self.lanes.gap),
                (self.lanes is not None, "lane", (), f64, lambda: self.lanes.lane),
                (self.lanes is not None, "lane_offset", (), f64, lambda: self.lanes.offset),
                (self.wander is not None, "wander", (8,), f64, lambda: self.wander.x))
        return [row[1:] for row in rows if row[0]]

    def run(self, steps, score=True, settle_tol=0.5, history=False, plant_updates=10):
        """`steps` control periods back to back: no host synchronisation and no device -> host copy in here.
        score=True: the initial state is scored geometry-only when the loop has not stepped (k == 0) and its record is fresh; then every
        period's new state is scored with that period's status, iters, command and stop latch.  history=True also records, on the device,
        state [steps+1,B,8] (the state before the first period first), cmd [steps,B,2], status [steps,B], latch [steps,B] and, with a sensor, est [steps,B,4]
        (what was measured of state[j] in period j: what the controller saw, unless an estimator follows) and, with an estimator, est_filt [steps,B,4]
        (what the controller saw then, unless a compensator follows; an observer's est_filt likewise, with dist [steps,B,3]) and, with a compensator, est_pred [steps,B,4] (what the controller saw then)
        and, with a planner, v_plan [steps,B] (the speed period j's waypoints and solve ran at) and, with a faulty sensor (SensorModel(faults=)),
        z [steps,B,4] (NaN where a source was silent: what a filter read; est is then the held state) and fault_flags [steps,B] int32 and, with
        wander=, wander [steps,B,8] (the processes' values in period j: what was added to the biases and the road words then) and, with follower=, v_follow
        [steps,B] (v_target under the following law in period j) and gap [steps,B] (to the leader, from state[j]; +inf without one) and, when the
        follower has a radar, gap_seen and v_lead_seen [steps,B] (the track after period j's call; +inf and 0 without a track) and, with lanes=,
        v_follow and gap likewise (the leader is the one in the vehicle's own lanes), lane [steps,B] and lane_offset [steps,B] (the lane and the
        commanded offset AFTER period j's decision and ramp step: what period j's waypoints were shifted by).
        -> dict of device tensors: score [B,16] (the loop's own, not a copy), err / seg / closest of the last scored state (score=True),
        the history (history=True) and the last period's step() dict as `last` (None for steps == 0)."""
        steps = int(steps)
        if steps < 0:
            raise ValueError("steps >= 0")
        dev = self.sim.device
        hist = None
        if history:
            optional = self._optional_history()
            hist = dict(state=torch.empty((steps + 1, self.B, 8), dtype=torch.float64, device=dev),
                        cmd=torch.empty((steps, self.B, 2), dtype=torch.float64, device=dev),
                        status=torch.empty((steps, self.B), dtype=torch.int32, device=dev),
                        latch=torch.empty((steps, self.B), dtype=torch.bool, device=dev))
            for key, shape, dt, _ in optional:
                hist[key] = torch.empty((steps, self.B) + shape, dtype=dt, device=dev)
            hist["state"][0].copy_(self.sim.state)
        if score and self.k == 0 and self._score_fresh:
            self._score_state(None, settle_tol)
        o = None
        for j in range(steps):
            o = self._period(plant_updates, False)
            if score:
                self._score_state(o, settle_tol)
            if history:
                hist["cmd"][j].copy_(o["cmd"]); hist["status"][j].copy_(o["status"])
                hist["latch"][j].copy_(self.command_stop); hist["state"][j + 1].copy_(self.sim.state)
                for key, _, _, source in optional:
                    hist[key][j].copy_(source())
        out = dict(score=self.score, last=o)
        if score and self.track is not None:
            out.update(self.track)
        if history:
            out.update(hist)
        return out

    def score_summary(self, dt=0.1):
        """the record as named numpy fields [B] (one synchronising download): ref_traj.SCORE_FIELDS, plus rms_ect and rms_epsi (already divided by
        the number of states scored; 0 where none was), t_settle = settle_index * dt, mean_iters over the live periods, and s_along of the last
        scored state (nan before the first)."""
        B = self.B
        tail = self.track["err"][:, 3:4] if self.track is not None else torch.full((B, 1), float("nan"), dtype=torch.float64, device=self.score.device)
        out = record_fields(torch.cat([self.score, tail], 1), SCORE_FIELDS + ("s_along",),
                            ("n", "settle_index", "n_refused", "n_live", "n_nonopt", "sum_iters", "latch_index"))
        n = np.maximum(out["n"], 1)
        out["rms_ect"], out["rms_epsi"] = np.sqrt(out["sum_ect2"] / n), np.sqrt(out["sum_epsi2"] / n)
        out["t_settle"] = out["settle_index"] * dt
        out["mean_iters"] = out["sum_iters"] / np.maximum(out["n_live"], 1)
        return out


class ClosedLoop(_ScoredLoop):
    """`grt`: a GPSRefTrajectory (one path; `track_with_time` picks the mode for the whole fleet) or a FleetRefTrajectory (a path and a mode per
    vehicle; `track_with_time` must stay False).  `target_vel`: a scalar or one target speed per vehicle -- vehicle b's waypoint spacing and its solver's
    v_des.  Re-routing a stop-latched vehicle does not clear its latch: clear `command_stop[b]` yourself."""

    def __init__(self, grt, sim, N=8, target_vel=0.0, track_with_time=False, weights=(9.0, 9.0, 10.0, 0.0, 100.0, 1000.0, 0.0, 0.0),
                 mpc=None, params=None, sensor=None, estimator=None, estimator_input="actuator", compensator=None, observer=None, planner=None,
                 blind_stop=False, wander=None, follower=None, lanes=None, **options):
        if grt.traj_horizon != N:
            raise ValueError("waypoint horizon %d != MPC horizon %d (Q10: the reference passes them separately)" % (grt.traj_horizon, N))
        self.grt, self.sim, self.N = grt, sim, int(N)
        self.B = sim.B
        self.mpc = mpc if mpc is not None else BatchMPC(N=N, dtype=torch.float64, device=sim.device.index, weights=weights, **options)
        # kmpc_command_batch reads the solver's first inputs as [B,2] doubles on the plant's device: a caller-supplied solver must match
        if self.mpc.dtype != torch.float64 or self.mpc.N != self.N or self.mpc.device != sim.device or sim.device.index is None:
            raise ValueError("ClosedLoop needs a float64 BatchMPC with horizon %d on %s (got %s, N=%d, %s)"
                             % (self.N, sim.device, self.mpc.dtype, self.mpc.N, self.mpc.device))
        if track_with_time and isinstance(grt, FleetRefTrajectory):
            raise ValueError("a FleetRefTrajectory owns the tracking modes (its time_mode): track_with_time must stay False")
        self.track_with_time = track_with_time
        self.des_speed, self.v_target = _target_speeds(target_vel, self.B, sim.device)  # mpc_cmd_pub.jl:58-62
        self._init_loop(params, sensor, estimator, estimator_input, compensator, observer, planner, track_with_time, blind_stop, wander, follower, lanes)

    def step(self, plant_updates=10, time_solve=False):
        """time_solve=True brackets the solve with device synchronisations and returns its wall time (`solve_s`)"""
        return self._period(plant_updates, time_solve)

    def _reference(self, st):
        pose = st[:, 0:3].contiguous()
        vt = self._speed(st)
        ref, stop = self.grt.get_waypoints_batch(pose, None if self.track_with_time else vt)
        if self.lanes is not None:
            self.lanes.shift(ref)
        z0 = st[:, 0:4].contiguous()                                                # x, y, psi, v = vx  (state_est, :43-46 of the simulator)
        return ref, stop, lambda: self.mpc.solve(z0, ref, vt, self.u_prev, warm_U=self.warm_U, warm=self.have_warm, out=self.out,
                                                 params=self.params), {}


class ClosedLoopFrenet(_ScoredLoop):
    """One `step()` = one pass of the Frenet node's loop (gazebo_sim_mpc_cmd_pub_frenet.jl:112-153) for every vehicle, then 0.1 s of plant:
    waypoints ahead of the vehicle at the target speed -> path in the vehicle frame, curvature polynomial and psi_start
    (get_reference_frenet_batch; :54-85, :105) -> update_init_cond(0, 0, -psi_start, v) (:128) -> warm-started solve -> command stage -> plant.
    Stop latch, rate-limit anchor and publish-whatever-the-status as in ClosedLoop.  Target-velocity mode only: the Frenet cost has no
    along-path term and the node has a fixed des_speed (:38).  A vehicle whose fit is refused (fit_status 1: see get_reference_frenet_batch) solves
    for a straight path with zero heading error -- in the loop that happens only to stop-latched vehicles, whose command is overridden.
    `grt` may be a FleetRefTrajectory and `target_vel` one speed per vehicle, as in ClosedLoop; a fleet helper with a vehicle in time mode is refused
    (checked once, here).  Re-routing a stop-latched vehicle does not clear its latch: clear `command_stop[b]` yourself."""

    def __init__(self, grt, sim, N=8, target_vel=0.0, weights=FRENET_WEIGHTS, mpc=None, params=None, track_with_time=False, sensor=None, estimator=None,
                 estimator_input="actuator", compensator=None, observer=None, planner=None, blind_stop=False, wander=None, follower=None,
                 lanes=None, **options):
        des_speed, v_target = _target_speeds(target_vel, sim.B, sim.device)
        if track_with_time or not all(v > 0.0 for v in (des_speed if isinstance(des_speed, tuple) else (des_speed,))):
            raise ValueError("ClosedLoopFrenet runs in target-velocity mode only: target_vel > 0 and no time tracking (got target_vel=%r, "
                             "track_with_time=%r)" % (target_vel, track_with_time))
        if isinstance(grt, FleetRefTrajectory) and grt.time_mode is not None and bool(grt.time_mode.any().item()):
            raise ValueError("ClosedLoopFrenet runs in target-velocity mode only: the fleet helper has vehicles in time mode")
        if grt.traj_horizon != N:
            raise ValueError("waypoint horizon %d != MPC horizon %d" % (grt.traj_horizon, N))
        self.grt, self.sim, self.N = grt, sim, int(N)
        self.B = sim.B
        self.mpc = mpc if mpc is not None else BatchMPC(N=N, dtype=torch.float64, device=sim.device.index, weights=weights, model=1, **options)
        if (self.mpc.dtype != torch.float64 or self.mpc.N != self.N or self.mpc.device != sim.device or sim.device.index is None
                or self.mpc.cfg.model != 1):
            raise ValueError("ClosedLoopFrenet needs a float64 model=1 BatchMPC with horizon %d on %s (got %s, model=%d, N=%d, %s)"
                             % (self.N, sim.device, self.mpc.dtype, self.mpc.cfg.model, self.mpc.N, self.mpc.device))
        self.des_speed, self.v_target = des_speed, v_target
        self._init_loop(params, sensor, estimator, estimator_input, compensator, observer, planner, track_with_time, blind_stop, wander, follower, lanes)

    def step(self, plant_updates=10, time_solve=False):
        """as ClosedLoop.step; the returned dict also carries `k_poly` [B,4] and `fit_status` [B]"""
        return self._period(plant_updates, time_solve)

    def _reference(self, st):
        pose = st[:, 0:3].contiguous()
        vt = self._speed(st)
        ref, stop = self.grt.get_waypoints_batch(pose, vt)
        if self.lanes is not None:
            self.lanes.shift(ref)
        k_poly, _psi, z0, fit_status = get_reference_frenet_batch(pose, ref, st[:, 3].contiguous())
        return ref, stop, lambda: self.mpc.solve_frenet(z0, k_poly, vt, self.u_prev, warm_U=self.warm_U, warm=self.have_warm, out=self.out,
                                                        params=self.params), dict(k_poly=k_poly, fit_status=fit_status)
