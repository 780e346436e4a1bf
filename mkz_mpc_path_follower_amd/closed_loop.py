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
"""
import ctypes as C

import torch

from . import _lib
from .kinematic_mpc_frenet import get_reference_frenet_batch
from .ref_traj import FleetRefTrajectory
from .solver import BatchMPC

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


class ClosedLoop:
    """`grt`: a GPSRefTrajectory (one path; `track_with_time` picks the mode for the whole fleet) or a FleetRefTrajectory (a path and a mode per
    vehicle; `track_with_time` must stay False).  `target_vel`: a scalar or one target speed per vehicle -- vehicle b's waypoint spacing and its solver's
    v_des.  Re-routing a stop-latched vehicle does not clear its latch: clear `command_stop[b]` yourself."""

    def __init__(self, grt, sim, N=8, target_vel=0.0, track_with_time=False, weights=(9.0, 9.0, 10.0, 0.0, 100.0, 1000.0, 0.0, 0.0),
                 mpc=None, params=None, **options):
        if grt.traj_horizon != N:
            raise ValueError("waypoint horizon %d != MPC horizon %d (Q10: the reference passes them separately)" % (grt.traj_horizon, N))
        self.grt, self.sim, self.N = grt, sim, int(N)
        self.B = sim.B
        self.mpc = mpc if mpc is not None else BatchMPC(N=N, dtype=torch.float64, device=sim.device.index, weights=weights, **options)
        # kmpc_command_batch reads the solver's first inputs as [B,2] doubles on the plant's device: a caller-supplied solver must match
        if self.mpc.dtype != torch.float64 or self.mpc.N != self.N or self.mpc.device != sim.device or sim.device.index is None:
            raise ValueError("ClosedLoop needs a float64 BatchMPC with horizon %d on %s (got %s, N=%d, %s)"
                             % (self.N, sim.device, self.mpc.dtype, self.mpc.N, self.mpc.device))
        if grt.device != sim.device:
            raise ValueError("waypoint helper on %s, plant on %s: the loop runs on one device" % (grt.device, sim.device))
        if track_with_time and isinstance(grt, FleetRefTrajectory):
            raise ValueError("a FleetRefTrajectory owns the tracking modes (its time_mode): track_with_time must stay False")
        self.track_with_time = track_with_time
        dev = sim.device
        self.des_speed, self.v_target = _target_speeds(target_vel, self.B, dev)  # mpc_cmd_pub.jl:58-62
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

    def step(self, plant_updates=10, time_solve=False):
        """time_solve=True brackets the solve with device synchronisations and returns its wall time (`solve_s`)"""
        import time
        st = self.sim.state
        pose = st[:, 0:3].contiguous()
        ref, stop = self.grt.get_waypoints_batch(pose, None if self.track_with_time else self.v_target)
        z0 = st[:, 0:4].contiguous()                                                # x, y, psi, v = vx  (state_est, :43-46 of the simulator)
        if time_solve:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        self.out = self.mpc.solve(z0, ref, self.v_target, self.u_prev, warm_U=self.warm_U, warm=self.have_warm, out=self.out, params=self.params)
        solve_s = None
        if time_solve:
            torch.cuda.synchronize()
            solve_s = time.perf_counter() - t0
        self.have_warm = True
        # stop latch (:100-103), command selection (:148-153) and update_current_input (:140, only on the solve branch): one kernel, straight
        # into the plant's command buffer
        cmd = self.sim.cmd
        u0 = self.out["u0"]
        assert u0.dtype == torch.float64 and u0.is_contiguous() and u0.device == cmd.device and u0.shape == (self.B, 2)
        stream = C.c_void_p(torch.cuda.current_stream(cmd.device).cuda_stream)
        _lib.check(self._lib.kmpc_command_batch(cmd.device.index, self.B, C.c_void_p(u0.data_ptr()), C.c_void_p(stop.data_ptr()),
                                                C.c_void_p(self.command_stop.data_ptr()), C.c_void_p(self.u_prev.data_ptr()),
                                                C.c_void_p(cmd.data_ptr()), stream))
        self.sim._update_vehicle_model(plant_updates)
        self.k += 1
        return dict(ref=ref, cmd=cmd, status=self.out["status"], iters=self.out["iters"], cost=self.out["cost"], solve_s=solve_s)


class ClosedLoopFrenet:
    """One `step()` = one pass of the Frenet node's loop (gazebo_sim_mpc_cmd_pub_frenet.jl:112-153) for every vehicle, then 0.1 s of plant:
    waypoints ahead of the vehicle at the target speed -> path in the vehicle frame, curvature polynomial and psi_start
    (get_reference_frenet_batch; :54-85, :105) -> update_init_cond(0, 0, -psi_start, v) (:128) -> warm-started solve -> command stage -> plant.
    Stop latch, rate-limit anchor and publish-whatever-the-status as in ClosedLoop.  Target-velocity mode only: the Frenet cost has no
    along-path term and the node has a fixed des_speed (:38).  A vehicle whose fit is refused (fit_status 1: see get_reference_frenet_batch) solves
    for a straight path with zero heading error -- in the loop that happens only to stop-latched vehicles, whose command is overridden.
    `grt` may be a FleetRefTrajectory and `target_vel` one speed per vehicle, as in ClosedLoop; a fleet helper with a vehicle in time mode is refused
    (checked once, here).  Re-routing a stop-latched vehicle does not clear its latch: clear `command_stop[b]` yourself."""

    def __init__(self, grt, sim, N=8, target_vel=0.0, weights=FRENET_WEIGHTS, mpc=None, params=None, track_with_time=False, **options):
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
        if grt.device != sim.device:
            raise ValueError("waypoint helper on %s, plant on %s: the loop runs on one device" % (grt.device, sim.device))
        self.des_speed, self.v_target = des_speed, v_target
        dev = sim.device
        self.u_prev = torch.zeros((self.B, 2), dtype=torch.float64, device=dev)
        self.warm_U = torch.zeros((self.B, self.N, 2), dtype=torch.float64, device=dev)
        self.command_stop = torch.zeros((self.B,), dtype=torch.bool, device=dev)
        self._lib = _lib.load()
        self.params = params
        self.have_warm = False
        self.out = None
        self.k = 0

    def step(self, plant_updates=10, time_solve=False):
        """as ClosedLoop.step; the returned dict also carries `k_poly` [B,4] and `fit_status` [B]"""
        import time
        st = self.sim.state
        pose = st[:, 0:3].contiguous()
        ref, stop = self.grt.get_waypoints_batch(pose, self.v_target)
        k_poly, _psi, z0, fit_status = get_reference_frenet_batch(pose, ref, st[:, 3].contiguous())
        if time_solve:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        self.out = self.mpc.solve_frenet(z0, k_poly, self.v_target, self.u_prev, warm_U=self.warm_U, warm=self.have_warm, out=self.out,
                                         params=self.params)
        solve_s = None
        if time_solve:
            torch.cuda.synchronize()
            solve_s = time.perf_counter() - t0
        self.have_warm = True
        cmd = self.sim.cmd
        u0 = self.out["u0"]
        assert u0.dtype == torch.float64 and u0.is_contiguous() and u0.device == cmd.device and u0.shape == (self.B, 2)
        stream = C.c_void_p(torch.cuda.current_stream(cmd.device).cuda_stream)
        _lib.check(self._lib.kmpc_command_batch(cmd.device.index, self.B, C.c_void_p(u0.data_ptr()), C.c_void_p(stop.data_ptr()),
                                                C.c_void_p(self.command_stop.data_ptr()), C.c_void_p(self.u_prev.data_ptr()),
                                                C.c_void_p(cmd.data_ptr()), stream))
        self.sim._update_vehicle_model(plant_updates)
        self.k += 1
        return dict(ref=ref, cmd=cmd, status=self.out["status"], iters=self.out["iters"], cost=self.out["cost"], solve_s=solve_s,
                    k_poly=k_poly, fit_status=fit_status)
