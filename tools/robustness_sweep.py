"""What the path follower tolerates: one closed-loop run of 4096 vehicles over a grid of plant mismatch, GPS noise and command latency, scored on the
device (-> profiles/robustness_sweep.txt).  An example of the Monte-Carlo surface (vehicle_sim.plant_params / SensorModel / cmd_delay and the loops'
`sensor=`), not a test: the numbers are findings.

Grid, 4 x 4 x 4 x 4 = 256 cells of 16 vehicles: mass x (0.85, 1.0, 1.15, 1.3); both cornering stiffnesses x (0.6, 0.8, 1.0, 1.2); GPS sigma on x and y
(0, 0.1, 0.2, 0.5) m; command delay (0, 2, 4, 8) model updates of 10 ms.  The 16 vehicles of a cell are spread over the three recorded paths of
tests/golden at 6 m/s (target-velocity mode, N = 8, the node's weights), starting on the path at speed.

--estimator puts vehicle_sim.Estimator (an extended Kalman filter per vehicle, r = the sensor's sigma) between the sensor and the controller
(-> profiles/robustness_sweep_estimator.txt) and also prints, per GPS sigma, the rms position error of what the controller saw against the truth.

--latency is a sweep of its own (-> profiles/robustness_sweep_latency.txt): nominal plant, no noise, estimator on; command delay (0, 10, 20, 30)
updates x age of the fix (0, 1, 2) periods, each cell once as it is and once with vehicle_sim.LatencyCompensator assuming the true delays
(the estimator fed from the command log, the estimate predicted ahead to where the command acts).

--road is a sweep of its own too (-> profiles/robustness_sweep_road.txt): nominal plant, no noise, no delay, the truth fed to the controller; the
road row of vehicle_sim.road_params per vehicle: friction coefficient (inf, 1.0, 0.7, 0.5, 0.35, 0.25) on both axles x target speed (6, 8) m/s x
lateral specific force (0, 0.75, 1.5) m/s^2 (bank) x steering offset (0, 0.015, 0.03) rad.

--observer is the road sweep's bank / offset / grade cells once more (-> profiles/robustness_sweep_observer.txt): no grip limit, 6 m/s, lateral
specific force (0, 0.75, 1.5) m/s^2 x steering offset (0, 0.015, 0.03) rad x longitudinal specific force (0, -0.5) m/s^2, each cell once as it is and
once with vehicle_sim.DisturbanceObserver (its defaults) in the loop: the existing figure next to the observer's.

--observer-latency is the observer sweep's cells under dead time (-> profiles/robustness_sweep_observer_latency.txt): total dead time 0.1 / 0.2 /
0.35 s (command delay 10 / 10 / 25 updates, fix 0 / 1 / 1 periods old) x the observer's q_dist at 1 / 0.5 / 0.25 of its default, each cell three ways:
Estimator + LatencyCompensator, DisturbanceObserver alone, and DisturbanceObserver + LatencyCompensator(disturbances=True).

--actuation is the sweep of the L0 layer (-> profiles/robustness_sweep_actuation.txt): the pedal-driven plant behind vehicle_sim.LowLevelController
(VehicleSimulator(drive=, llc=)), no noise, no delay, neutral road, on the three paths at 6 m/s: the controller's brake deadband (0, 0.1, 0.2) m/s^2
x plant mass x (0.85, 1, 1.3) x F_PEAK (2500, 6000) N x error of the controller's steering ratio (0, +5 %, -5 %), each cell once as it is and once
with vehicle_sim.DisturbanceObserver (its defaults, estimator_input="command": it compares what was commanded with what the speed did).

--speed-plan is the road sweep's mu x target-speed cells on a level road without offset (-> profiles/robustness_sweep_speed_plan.txt), each cell once as it
is and once with planner=ref_traj.SpeedPlanner (rows a_lat = 0.6 mu g, a_brake 0.7, v_floor 1.0): the --road columns plus the mean speed.

--road-profile is the road as a property of the PLACE (-> profiles/robustness_sweep_road_profile.txt): the --speed-plan starts at 6 and 8 m/s on a base
road of mu = 1.0, with vehicle_sim.RoadProfile scaling the grip by MU_SCALE (0.7, 0.5, 0.35, 0.25) on the corner patches only (the samples within
10 m of arclength of a sample with |kappa| >= 0.03 at window 4 m), each cell three ways: no plan, planner= with a map that knows nothing (the neutral
table), planner= with map = truth (rows a_lat = 0.6 g, a_brake 0.7, v_floor 1.0): the --speed-plan columns.  Then an observer block: a bank of
1.5 m/s^2 on alternating 100 m stretches (through the profile) against the same bank held constant (through road=), at 6 m/s without a grip limit,
each without and with vehicle_sim.DisturbanceObserver.

--outage is the sweep of sensor faults (-> profiles/robustness_sweep_outage.txt): SensorModel(faults=vehicle_sim.fault_params(...)), nominal plant,
no delay, the road sweep's 48 starts at 6 m/s: GPS window length (0, 10, 30, 100) periods, its start drawn per vehicle, x IMU bias (0, 0.02) rad, each
cell once on the held fix (no filter: what scripts/state_publisher.py publishes) and once with estimator= (fed z: it dead-reckons on heading and
speed); one outlier row (P_OUTLIER 0.05, OUTLIER_SIGMA 3 m on a GPS of sigma 0.1 m; the estimator with gate 0 against gate 4); one blind_stop row
(MAX_AGE 30: a vehicle blind for longer latches and brakes).

--wander is the sweep of coloured noise and gusts (-> profiles/robustness_sweep_wander.txt): wander=vehicle_sim.Wander, nominal plant, no delay, the
road sweep's 48 starts at 6 m/s: a GPS error of sigma (0.1, 0.2, 0.5) m as white noise against the same sigma coloured with tau (2, 10, 30) s, each without
and with estimator=; a lateral gust of sigma (0.5, 1.0) m/s^2 and tau (0.5, 2, 10) s without observer=, with it at its default q_dist and at 4 x; a
heading random walk (0, 0.003, 0.01) rad/sqrt(s) on top of GPS outages of 30 and 100 periods with estimator=.

--platoon is the sweep of car following (-> profiles/robustness_sweep_platoon.txt): follower=ref_traj.Follower, platoons of eight on the three paths,
the leader's target stepping 6 -> 3 -> 6 m/s: T_HEADWAY (0.5, 1.0, 1.5) s x command delay (0, 0.1, 0.3) s x GPS sigma (0, 0.2) m, each cell once as it
is and once with estimator= and compensator=: smallest gap, contacts, the speed dip of the last follower over that of the first, solves not Optimal.

--overtake is the sweep of the lane stage (-> profiles/robustness_sweep_overtake.txt): lanes=ref_traj.Lanes on two lanes, platoons of six on the three
paths, a slow vehicle (3 m/s) in front and five at 6 m/s behind it, under --platoon's cells and both of its ways: contacts, smallest own-lane gap, lane
changes, how many of the fast vehicles end ahead of the slow one and back in lane 0, their mean speed, solves not Optimal.

--radar is the sweep of the range sensor (-> profiles/robustness_sweep_radar.txt): follower=ref_traj.Follower(radar=ref_traj.RangeSensor), --platoon's
platoons of eight at T_HEADWAY 1 s without command delay, GPS sigma 0.2 m and speed sigma 0.1 m/s (the law's own speed is the sensed one): SIGMA_R
(0, 0.25, 0.5, 1) m x P_DROP (0, 0.1, 0.3) x RANGE_MAX (+inf, 30, 15) m x FILTER (0, 1): smallest true gap, contacts, the dip ratio, the rms change
of v_follow from period to period (noise passed to the command), the rms of GAP_HAT - gap, the share of Optimal solves; and a standing leader 100 m
ahead of a 6 m/s follower per RANGE_MAX: where it stops.

usage: python tools/robustness_sweep.py [--estimator] [out.txt] [steps]
       python tools/robustness_sweep.py --radar [out.txt]
       python tools/robustness_sweep.py --platoon [out.txt]
       python tools/robustness_sweep.py --overtake [out.txt]
       python tools/robustness_sweep.py --wander [out.txt] [steps]
       python tools/robustness_sweep.py --outage [out.txt] [steps]
       python tools/robustness_sweep.py --road-profile [out.txt] [steps]
       python tools/robustness_sweep.py --speed-plan [out.txt] [steps]
       python tools/robustness_sweep.py --actuation [out.txt] [steps]
       python tools/robustness_sweep.py --observer [out.txt] [steps]
       python tools/robustness_sweep.py --observer-latency [out.txt] [steps]
       python tools/robustness_sweep.py --latency [out.txt] [steps]
       python tools/robustness_sweep.py --road [out.txt] [steps]
"""
import itertools
import sys

import numpy as np
import torch

import _timing as T
from _timing import say
from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop  # noqa: E402
from mkz_mpc_path_follower_amd.ref_traj import FleetRefTrajectory  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import Estimator, LatencyCompensator, SensorModel, VehicleSimulator, plant_default, plant_params  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import road_params  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver  # noqa: E402

MASS, STIFF, SIGMA, DELAY = (0.85, 1.0, 1.15, 1.3), (0.6, 0.8, 1.0, 1.2), (0.0, 0.1, 0.2, 0.5), (0, 2, 4, 8)
PER_CELL, VT = 16, 6.0


def main():
    use_estimator = "--estimator" in sys.argv[1:]
    argv = [a for a in sys.argv if a != "--estimator"]
    steps = int(argv[2]) if len(argv) > 2 else 150
    paths = [T.path_dict(f) for f in T.FILES]
    cells = list(itertools.product(range(4), repeat=4))
    B = len(cells) * PER_CELL
    cell = np.repeat(np.arange(len(cells)), PER_CELL)
    ix = np.array(cells)[cell]                      # [B,4] grid indices: mass, stiffness, sigma, delay
    rng = np.random.default_rng(0)
    pid = np.tile(np.arange(PER_CELL) % 3, len(cells))
    fleet = FleetRefTrajectory(paths, pid, traj_horizon=8, traj_dt=0.2)
    frac = np.tile(rng.uniform(0.02, 0.45, PER_CELL), len(cells))     # the same 16 starts in every cell
    pose = np.empty((B, 3))
    for b in range(B):
        tr = fleet.trajectories[pid[b]]
        i = int(frac[b] * len(tr))
        pose[b] = tr[i, 4], tr[i, 5], tr[i, 3]
    d0 = plant_default()
    st = np.array(STIFF)[ix[:, 1]]
    sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2],
                           plant=plant_params(B, m=d0[2] * np.array(MASS)[ix[:, 0]], C_alpha_f=d0[4] * st, C_alpha_r=d0[5] * st),
                           cmd_delay=np.array(DELAY)[ix[:, 3]])
    sim.state[:, 3] = VT
    sigma = np.zeros((B, 4))
    sigma[:, 0] = sigma[:, 1] = np.array(SIGMA)[ix[:, 2]]
    sensor = SensorModel(B, sigma=sigma, seed=2024)
    if use_estimator:
        loop = ClosedLoop(fleet, sim, N=8, target_vel=VT, sensor=sensor, estimator=Estimator.from_sensor(sensor))
        hist = loop.run(steps, history=True)
    else:
        loop = ClosedLoop(fleet, sim, N=8, target_vel=VT, sensor=sensor)
        loop.run(steps)
    s = loop.score_summary()
    finite = bool(torch.isfinite(sim.state).all().item())
    say("%s: %d vehicles, %d periods of 0.1 s at %.0f m/s on three paths; every state finite: %s; latched vehicles: %d"
        % (torch.cuda.get_device_name(0), B, steps, VT, finite, int((s["latch_index"] >= 0).sum())))
    say("per factor level, over all other factors: median / 95th percentile of rms e_ct [m], largest |e_ct| [m], periods not Optimal per 1000")

    def row(label, sel):
        say("   %-28s %7.3f %7.3f %8.3f %8.2f" % (label, np.median(s["rms_ect"][sel]), np.percentile(s["rms_ect"][sel], 95), s["max_ect"][sel].max(),
                                                1000.0 * s["n_nonopt"][sel].sum() / max(1, s["n_live"][sel].sum())))
    for f, (name, levels, fmt) in enumerate((("mass x", MASS, "%.2f"), ("cornering stiffness x", STIFF, "%.1f"), ("GPS sigma [m]", SIGMA, "%.1f"),
                                             ("delay [10 ms updates]", DELAY, "%d"))):
        for lv in range(4):
            row("%s %s" % (name, fmt % levels[lv]), ix[:, f] == lv)
    say("cells (mass x, stiffness x, sigma, delay): the nominal one, then the five with the largest median rms e_ct")
    med = np.array([np.median(s["rms_ect"][cell == c]) for c in range(len(cells))])
    nominal = cells.index((1, 2, 0, 0))
    for c in [nominal] + list(np.argsort(-med)[:5]):
        m, k, g, dl = cells[c]
        row("(%.2f, %.1f, %.1f, %d)" % (MASS[m], STIFF[k], SIGMA[g], DELAY[dl]), cell == c)
    if use_estimator:
        truth = hist["state"][:steps, :, 0:2]
        e_raw = ((hist["est"][:, :, 0:2] - truth) ** 2).sum(2).mean(0).sqrt().cpu().numpy()
        e_filt = ((hist["est_filt"][:, :, 0:2] - truth) ** 2).sum(2).mean(0).sqrt().cpu().numpy()
        say("with the estimator (q = 0.02 m, 0.02 m, 0.01 rad, 0.1 m/s per period, r = sigma floored at 1e-3 m): median rms position error of the measurement "
            "-> of what the controller saw [m]; filter resets: %d" % int((loop.estimator.flags & 32).sum().item()))
        for lv in range(4):
            sel = ix[:, 2] == lv
            say("   GPS sigma [m] %.1f              %7.3f -> %7.3f" % (SIGMA[lv], np.median(e_raw[sel]), np.median(e_filt[sel])))
    T.finish(argv)


LAT_CMD, LAT_FIX, LAT_PER_CELL = (0, 10, 20, 30), (0, 1, 2), 48


def latency_main():
    """one loop of 4 x 3 x 2 cells of 48 vehicles.  An uncompensated vehicle is one whose compensator assumes no delay: its prediction returns the
    estimate bit for bit and its filter input is the previous period's command (estimator_input="command" without a compensator)."""
    argv = [a for a in sys.argv if a != "--latency"]
    steps = int(argv[2]) if len(argv) > 2 else 150
    paths = [T.path_dict(f) for f in T.FILES]
    cells = list(itertools.product(range(4), range(3), range(2)))
    B = len(cells) * LAT_PER_CELL
    cell = np.repeat(np.arange(len(cells)), LAT_PER_CELL)
    ix = np.array(cells)[cell]                      # [B,3] grid indices: command delay, fix age, compensated
    rng = np.random.default_rng(0)
    pid = np.tile(np.arange(LAT_PER_CELL) % 3, len(cells))
    fleet = FleetRefTrajectory(paths, pid, traj_horizon=8, traj_dt=0.2)
    frac = np.tile(rng.uniform(0.02, 0.45, LAT_PER_CELL), len(cells))     # the same 48 starts in every cell
    pose = np.empty((B, 3))
    for b in range(B):
        tr = fleet.trajectories[pid[b]]
        i = int(frac[b] * len(tr))
        pose[b] = tr[i, 4], tr[i, 5], tr[i, 3]
    cd, fa, comp = np.array(LAT_CMD)[ix[:, 0]], np.array(LAT_FIX)[ix[:, 1]], ix[:, 2]
    sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2], cmd_delay=cd, cmd_queue_depth=4)
    sim.state[:, 3] = VT
    sensor = SensorModel(B, meas_delay=fa)
    compensator = LatencyCompensator(B, cmd_delay=cd * comp, meas_delay=fa * comp)
    loop = ClosedLoop(fleet, sim, N=8, target_vel=VT, sensor=sensor, estimator=Estimator.from_sensor(sensor), estimator_input="history",
                      compensator=compensator)
    loop.run(steps)
    s = loop.score_summary()
    finite = bool(torch.isfinite(sim.state).all().item())
    say("%s: %d vehicles, %d periods of 0.1 s at %.0f m/s on three paths, nominal plant, no noise, estimator on; every state finite: %s; "
        "latched vehicles: %d; filter resets: %d" % (torch.cuda.get_device_name(0), B, steps, VT, finite, int((s["latch_index"] >= 0).sum()),
                                                      int((loop.estimator.flags & 32).sum().item())))
    say("per cell of %d vehicles: median / 95th percentile of rms e_ct [m], largest |e_ct| [m], periods not Optimal per 1000 -- as it is, then compensated"
        % LAT_PER_CELL)

    def fig(sel):
        return (np.median(s["rms_ect"][sel]), np.percentile(s["rms_ect"][sel], 95), s["max_ect"][sel].max(),
                1000.0 * s["n_nonopt"][sel].sum() / max(1, s["n_live"][sel].sum()))
    for c in range(4):
        for f in range(3):
            base = (ix[:, 0] == c) & (ix[:, 1] == f)
            say("   command delay %2d updates, fix %d periods old   %7.3f %7.3f %8.3f %8.2f   ->  %7.3f %7.3f %8.3f %8.2f"
                % ((LAT_CMD[c], LAT_FIX[f]) + fig(base & (ix[:, 2] == 0)) + fig(base & (ix[:, 2] == 1))))
    T.finish(argv)


ROAD_MU, ROAD_VT, ROAD_LAT, ROAD_OFFSET, ROAD_PER_CELL = (float("inf"), 1.0, 0.7, 0.5, 0.35, 0.25), (6.0, 8.0), (0.0, 0.75, 1.5), (0.0, 0.015, 0.03), 48


def road_main():
    """one loop of 6 x 2 x 3 x 3 cells of 48 vehicles, each cell the same 48 starts: on the path, heading along it, already at the cell's speed"""
    argv = [a for a in sys.argv if a != "--road"]
    steps = int(argv[2]) if len(argv) > 2 else 150
    paths = [T.path_dict(f) for f in T.FILES]
    cells = list(itertools.product(range(6), range(2), range(3), range(3)))
    B = len(cells) * ROAD_PER_CELL
    cell = np.repeat(np.arange(len(cells)), ROAD_PER_CELL)
    ix = np.array(cells)[cell]                      # [B,4] grid indices: mu, speed, lateral force, steering offset
    rng = np.random.default_rng(0)
    pid = np.tile(np.arange(ROAD_PER_CELL) % 3, len(cells))
    fleet = FleetRefTrajectory(paths, pid, traj_horizon=8, traj_dt=0.2)
    frac = np.tile(rng.uniform(0.02, 0.45, ROAD_PER_CELL), len(cells))
    pose = np.empty((B, 3))
    for b in range(B):
        tr = fleet.trajectories[pid[b]]
        i = int(frac[b] * len(tr))
        pose[b] = tr[i, 4], tr[i, 5], tr[i, 3]
    vt = np.array(ROAD_VT)[ix[:, 1]]
    sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2],
                           road=road_params(B, mu=np.array(ROAD_MU)[ix[:, 0]], a_lat=np.array(ROAD_LAT)[ix[:, 2]], df_offset=np.array(ROAD_OFFSET)[ix[:, 3]]))
    sim.state[:, 3] = torch.as_tensor(vt, device=sim.device)
    loop = ClosedLoop(fleet, sim, N=8, target_vel=vt)
    loop.run(steps)
    s, grip = loop.score_summary(), sim.road_summary()
    slid = (grip["sat_f"] + grip["sat_r"]) > 0
    finite = bool(torch.isfinite(sim.state).all().item())
    say("%s: %d vehicles, %d periods of 0.1 s on three paths, nominal plant, no noise, no delay; every state finite: %s; latched vehicles: %d"
        % (torch.cuda.get_device_name(0), B, steps, finite, int((s["latch_index"] >= 0).sum())))
    head = "median / 95th percentile of rms e_ct [m], largest |e_ct| [m], share of vehicles that ever saturated [%], periods not Optimal per 1000"

    def row(label, sel):
        say("   %-44s %7.3f %7.3f %8.3f %7.1f %8.2f" % (label, np.median(s["rms_ect"][sel]), np.percentile(s["rms_ect"][sel], 95), s["max_ect"][sel].max(),
                                                        100.0 * slid[sel].mean(), 1000.0 * s["n_nonopt"][sel].sum() / max(1, s["n_live"][sel].sum())))
    say("per factor level, over all other factors: " + head)
    for f, (name, levels, fmt) in enumerate((("mu", ROAD_MU, "%.2f"), ("target speed [m/s]", ROAD_VT, "%.0f"), ("lateral force [m/s^2]", ROAD_LAT, "%.2f"),
                                             ("steering offset [rad]", ROAD_OFFSET, "%.3f"))):
        for lv in range(len(levels)):
            row("%s %s" % (name, fmt % levels[lv]), ix[:, f] == lv)
    say("mu x target speed on a level road without offset (%d vehicles per line): " % ROAD_PER_CELL + head)
    for v in range(2):
        for m in range(6):
            row("mu %.2f at %.0f m/s" % (ROAD_MU[m], ROAD_VT[v]), (ix[:, 0] == m) & (ix[:, 1] == v) & (ix[:, 2] == 0) & (ix[:, 3] == 0))
    say("lateral force x steering offset without a grip limit, both speeds (%d vehicles per line): " % (2 * ROAD_PER_CELL) + head)
    for a in range(3):
        for o in range(3):
            row("%.2f m/s^2, %.3f rad" % (ROAD_LAT[a], ROAD_OFFSET[o]), (ix[:, 0] == 0) & (ix[:, 2] == a) & (ix[:, 3] == o))
    say("largest utilisation |C_alpha alpha| / limit, median per mu at 6 and 8 m/s (level road, no offset), front / rear")
    for m in range(1, 6):
        sel = [(ix[:, 0] == m) & (ix[:, 1] == v) & (ix[:, 2] == 0) & (ix[:, 3] == 0) for v in range(2)]
        say("   mu %.2f   %6.2f / %-6.2f   %6.2f / %-6.2f" % (ROAD_MU[m], np.median(grip["util_f"][sel[0]]), np.median(grip["util_r"][sel[0]]),
                                                           np.median(grip["util_f"][sel[1]]), np.median(grip["util_r"][sel[1]])))
    T.finish(argv)


def speed_plan_main():
    """two loops of the road sweep's mu x target-speed cells (6 x 2 cells of 48 vehicles, level road, no offset, the same starts): without and with
    planner= (ref_traj.SpeedPlanner, rows a_lat = 0.6 mu g -- 2.0 without a grip limit --, a_brake 0.7, v_floor 1.0, window 4 m)"""
    from mkz_mpc_path_follower_amd.ref_traj import SpeedPlanner, speed_plan_params
    argv = [a for a in sys.argv if a != "--speed-plan"]
    steps = int(argv[2]) if len(argv) > 2 else 150
    paths = [T.path_dict(f) for f in T.FILES]
    cells = list(itertools.product(range(6), range(2)))
    B = len(cells) * ROAD_PER_CELL
    ix = np.array(cells)[np.repeat(np.arange(len(cells)), ROAD_PER_CELL)]      # [B,2] grid indices: mu, speed
    rng = np.random.default_rng(0)
    pid = np.tile(np.arange(ROAD_PER_CELL) % 3, len(cells))
    frac = np.tile(rng.uniform(0.02, 0.45, ROAD_PER_CELL), len(cells))          # the road sweep's starts
    mu, vt = np.array(ROAD_MU)[ix[:, 0]], np.array(ROAD_VT)[ix[:, 1]]
    a_lat = np.where(np.isfinite(mu), 0.6 * np.where(np.isfinite(mu), mu, 1.0) * 9.81, 2.0)
    res = []
    for planned in (False, True):
        fleet = FleetRefTrajectory(paths, pid, traj_horizon=8, traj_dt=0.2)
        pose = np.empty((B, 3))
        for b in range(B):
            tr = fleet.trajectories[pid[b]]
            i = int(frac[b] * len(tr))
            pose[b] = tr[i, 4], tr[i, 5], tr[i, 3]
        sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2], road=road_params(B, mu=mu))
        sim.state[:, 3] = torch.as_tensor(vt, device=sim.device)
        planner = SpeedPlanner(fleet, window=4.0, rows=speed_plan_params(B, a_lat=a_lat, a_brake=0.7, v_floor=1.0)) if planned else None
        loop = ClosedLoop(fleet, sim, N=8, target_vel=vt, planner=planner)
        out = loop.run(steps, history=True)
        s, grip = loop.score_summary(), sim.road_summary()
        res.append(dict(s=s, slid=(grip["sat_f"] + grip["sat_r"]) > 0, finite=bool(torch.isfinite(sim.state).all().item()),
                        speed=out["state"][:, :, 3].mean(0).cpu().numpy(),
                        late=(out["v_plan"][0].cpu().numpy() < vt) if planned else np.zeros(B, dtype=bool)))
    say("%s: 2 x %d vehicles, %d periods of 0.1 s on three paths, nominal plant, no noise, no delay, level road, no offset; every state finite: %s / %s; "
        "latched vehicles: %d / %d (without / with the planner)" % (torch.cuda.get_device_name(0), B, steps, res[0]["finite"], res[1]["finite"],
                                                                    int((res[0]["s"]["latch_index"] >= 0).sum()), int((res[1]["s"]["latch_index"] >= 0).sum())))
    say("planner rows: a_lat = 0.6 mu g (2.0 at mu = inf), a_brake 0.7, v_floor 1.0, window 4 m.  `late`: vehicles whose first planned speed is below the "
        "speed they start at -- they start inside or just before a corner, where the plan can only brake late")
    head = ("median / 95th percentile of rms e_ct [m], largest |e_ct| [m], share of vehicles that ever saturated [%], periods not Optimal per 1000, "
            "mean speed [m/s]")
    say("mu x target speed (%d vehicles per line), plain | planned | late: " % ROAD_PER_CELL + head)

    def cols(r, sel):
        s = r["s"]
        return (np.median(s["rms_ect"][sel]), np.percentile(s["rms_ect"][sel], 95), s["max_ect"][sel].max(), 100.0 * r["slid"][sel].mean(),
                1000.0 * s["n_nonopt"][sel].sum() / max(1, s["n_live"][sel].sum()), r["speed"][sel].mean())
    for v in range(2):
        for m in range(6):
            sel = (ix[:, 0] == m) & (ix[:, 1] == v)
            say("   %-20s %7.3f %7.3f %8.3f %6.1f %7.2f %6.2f  | %7.3f %7.3f %8.3f %6.1f %7.2f %6.2f  | %2d"
                % (("mu %.2f at %.0f m/s" % (ROAD_MU[m], ROAD_VT[v]),) + cols(res[0], sel) + cols(res[1], sel) + (int(res[1]["late"][sel].sum()),)))
    say("the same without the late starters (largest |e_ct| [m] plain | planned, vehicles left)")
    for v in range(2):
        for m in range(6):
            sel = (ix[:, 0] == m) & (ix[:, 1] == v) & ~res[1]["late"]
            say("   %-20s %8.3f | %8.3f   %2d" % ("mu %.2f at %.0f m/s" % (ROAD_MU[m], ROAD_VT[v]), res[0]["s"]["max_ect"][sel].max(),
                                                 res[1]["s"]["max_ect"][sel].max(), int(sel.sum())))
    T.finish(argv)


RP_SCALE, RP_KAPPA, RP_REACH, RP_BANK, RP_STRETCH = (0.7, 0.5, 0.35, 0.25), 0.03, 10.0, 1.5, 100.0


def road_profile_main():
    """three loops of 4 x 2 cells of 48 vehicles (MU_SCALE on the corner patches x target speed; the road sweep's starts): no plan, plan with the
    neutral map, plan with map = truth.  A table is per path, so every MU_SCALE level drives on its own copy of the three paths (12 paths in the set).
    Then four loops of 48 vehicles at 6 m/s: bank alternating by place / constant x without / with observer=."""
    from mkz_mpc_path_follower_amd.ref_traj import SpeedPlanner, speed_plan_params
    from mkz_mpc_path_follower_amd.vehicle_sim import RoadProfile, road_profile_patch, road_profile_table
    argv = [a for a in sys.argv if a != "--road-profile"]
    steps = int(argv[2]) if len(argv) > 2 else 150
    paths = [T.path_dict(f) for f in T.FILES]
    cells = list(itertools.product(range(len(RP_SCALE)), range(2)))
    B = len(cells) * ROAD_PER_CELL
    ix = np.array(cells)[np.repeat(np.arange(len(cells)), ROAD_PER_CELL)]      # [B,2] grid indices: MU_SCALE, speed
    rng = np.random.default_rng(0)
    base_pid = np.tile(np.arange(ROAD_PER_CELL) % 3, len(cells))
    pid = 3 * ix[:, 0] + base_pid                                              # copy ix[:, 0] of path base_pid
    frac = np.tile(rng.uniform(0.02, 0.45, ROAD_PER_CELL), len(cells))          # the road sweep's starts
    vt = np.array(ROAD_VT)[ix[:, 1]]

    def truth_table(fleet):
        """MU_SCALE level k on the corner patches of copy k of each path -> (numpy table, samples patched per path of one copy)"""
        kappa = SpeedPlanner(fleet, window=4.0).kappa.cpu().numpy()
        tab, off, n = road_profile_table(fleet), 0, []
        for p, tr in enumerate(fleet.trajectories):
            s, kap = tr[:, 6], kappa[off:off + len(tr)]
            tight = s[np.fabs(kap) >= RP_KAPPA]
            k = np.searchsorted(tight, s)
            near = np.minimum(np.abs(s - tight[np.clip(k - 1, 0, len(tight) - 1)]), np.abs(s - tight[np.clip(k, 0, len(tight) - 1)])) <= RP_REACH
            tab[off + np.flatnonzero(near), 0] = RP_SCALE[p // 3]
            n.append(int(near.sum()))
            off += len(tr)
        return tab, n[:3]
    res, patched = [], None
    for planned, knows in ((False, False), (True, False), (True, True)):
        fleet = FleetRefTrajectory(paths * len(RP_SCALE), pid, traj_horizon=8, traj_dt=0.2)
        truth, patched = truth_table(fleet)
        pose = np.empty((B, 3))
        for b in range(B):
            tr = fleet.trajectories[pid[b]]
            i = int(frac[b] * len(tr))
            pose[b] = tr[i, 4], tr[i, 5], tr[i, 3]
        sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2], road=road_params(B, mu=1.0), road_profile=RoadProfile(fleet, truth))
        sim.state[:, 3] = torch.as_tensor(vt, device=sim.device)
        planner = None
        if planned:
            planner = SpeedPlanner(fleet, window=4.0, rows=speed_plan_params(B, a_lat=0.6 * 9.81, a_brake=0.7, v_floor=1.0),
                                   profile=RoadProfile(fleet, truth if knows else None))
        loop = ClosedLoop(fleet, sim, N=8, target_vel=vt, planner=planner)
        out = loop.run(steps, history=True)
        s, grip = loop.score_summary(), sim.road_summary()
        res.append(dict(s=s, slid=(grip["sat_f"] + grip["sat_r"]) > 0, finite=bool(torch.isfinite(sim.state).all().item()),
                        speed=out["state"][:, :, 3].mean(0).cpu().numpy(),
                        late=(out["v_plan"][0].cpu().numpy() < vt) if planned else np.zeros(B, dtype=bool)))
    say("%s: 3 x %d vehicles, %d periods of 0.1 s on three paths, nominal plant, no noise, no delay, level road; base road mu = 1.0, MU_SCALE on the corner "
        "patches only (%s samples of the three paths, within %.0f m of |kappa| >= %.2f); every state finite: %s / %s / %s; latched vehicles: %d / %d / %d "
        "(no plan / plan with the neutral map / plan with map = truth)"
        % ((torch.cuda.get_device_name(0), B, steps, " + ".join(str(n) for n in patched), RP_REACH, RP_KAPPA) + tuple(r["finite"] for r in res)
           + tuple(int((r["s"]["latch_index"] >= 0).sum()) for r in res)))
    say("planner rows: a_lat = 0.6 g, a_brake 0.7, v_floor 1.0, window 4 m; the map scales a_lat by its MU_SCALE.  `late`: vehicles whose first speed planned "
        "on the true map is below the speed they start at")
    head = ("median / 95th percentile of rms e_ct [m], largest |e_ct| [m], share of vehicles that ever saturated [%], periods not Optimal per 1000, "
            "mean speed [m/s]")
    say("MU_SCALE x target speed (%d vehicles per line), no plan | neutral map | map = truth | late: " % ROAD_PER_CELL + head)

    def cols(r, sel):
        s = r["s"]
        return (np.median(s["rms_ect"][sel]), np.percentile(s["rms_ect"][sel], 95), s["max_ect"][sel].max(), 100.0 * r["slid"][sel].mean(),
                1000.0 * s["n_nonopt"][sel].sum() / max(1, s["n_live"][sel].sum()), r["speed"][sel].mean())
    for v in range(2):
        for m in range(len(RP_SCALE)):
            sel = (ix[:, 0] == m) & (ix[:, 1] == v)
            say("   %-22s %7.3f %7.3f %8.3f %6.1f %7.2f %6.2f  | %7.3f %7.3f %8.3f %6.1f %7.2f %6.2f  | %7.3f %7.3f %8.3f %6.1f %7.2f %6.2f  | %2d"
                % (("scale %.2f at %.0f m/s" % (RP_SCALE[m], ROAD_VT[v]),) + cols(res[0], sel) + cols(res[1], sel) + cols(res[2], sel)
                   + (int(res[2]["late"][sel].sum()),)))
    say("the same without the late starters (largest |e_ct| [m] no plan | neutral map | map = truth, vehicles left)")
    for v in range(2):
        for m in range(len(RP_SCALE)):
            sel = (ix[:, 0] == m) & (ix[:, 1] == v) & ~res[2]["late"]
            say("   %-22s %8.3f | %8.3f | %8.3f   %2d" % (("scale %.2f at %.0f m/s" % (RP_SCALE[m], ROAD_VT[v]),) + tuple(r["s"]["max_ect"][sel].max() for r in res)
                                                         + (int(sel.sum()),)))
    # ---- the observer under a bank that comes and goes
    nb, osteps = ROAD_PER_CELL, 200
    opid = np.arange(nb) % 3
    ofrac = frac[:nb]
    obs = {}
    for alternating in (True, False):
        for with_observer in (False, True):
            fleet = FleetRefTrajectory(paths, opid, traj_horizon=8, traj_dt=0.2)
            pose = np.empty((nb, 3))
            for b in range(nb):
                tr = fleet.trajectories[opid[b]]
                i = int(ofrac[b] * len(tr))
                pose[b] = tr[i, 4], tr[i, 5], tr[i, 3]
            kw = dict(road=road_params(nb, a_lat=RP_BANK))
            if alternating:
                tab = road_profile_table(fleet)
                for p, tr in enumerate(fleet.trajectories):
                    for a in np.arange(0.0, tr[-1, 6], 2.0 * RP_STRETCH):
                        road_profile_patch(tab, fleet, p, a, a + RP_STRETCH, a_lat=RP_BANK)
                kw = dict(road=road_params(nb), road_profile=RoadProfile(fleet, tab))
            sim = VehicleSimulator(nb, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2], **kw)
            sim.state[:, 3] = VT
            loop = ClosedLoop(fleet, sim, N=8, target_vel=VT, observer=DisturbanceObserver(nb) if with_observer else None)
            loop.run(osteps)
            s = loop.score_summary()
            obs[(alternating, with_observer)] = (np.median(s["rms_ect"]), s["max_ect"].max(), 1000.0 * s["n_nonopt"].sum() / max(1, s["n_live"].sum()),
                                                 bool(torch.isfinite(sim.state).all().item()))
    say("observer block: %d vehicles on the three paths at %.0f m/s, %d periods, no grip limit; A_LAT %.1f m/s^2 on alternating %.0f m stretches (on from "
        "s = 0, through the profile) | held constant (through road=): median rms e_ct [m], largest |e_ct| [m], periods not Optimal per 1000, every state finite"
        % (nb, VT, osteps, RP_BANK, RP_STRETCH))
    for w in (False, True):
        a, c = obs[(True, w)], obs[(False, w)]
        say("   %-28s %6.3f %6.3f %6.2f %s  | %6.3f %6.3f %6.2f %s" % (("with DisturbanceObserver" if w else "without an observer",) + a + c))
    T.finish(argv)


OBS_LONG = (0.0, -0.5)


def observer_main():
    """two loops of 3 x 3 x 2 cells of 48 vehicles (the road sweep's starts, all at 6 m/s, no grip limit): without and with observer=.  Each loop is
    scored in two halves: the whole run carries the start and the corners, the second half is what stays."""
    argv = [a for a in sys.argv if a != "--observer"]
    steps = int(argv[2]) if len(argv) > 2 else 200
    paths = [T.path_dict(f) for f in T.FILES]
    cells = list(itertools.product(range(3), range(3), range(2)))
    B = len(cells) * ROAD_PER_CELL
    ix = np.array(cells)[np.repeat(np.arange(len(cells)), ROAD_PER_CELL)]     # [B,3] grid indices: lateral force, steering offset, longitudinal force
    rng = np.random.default_rng(0)
    pid = np.tile(np.arange(ROAD_PER_CELL) % 3, len(cells))
    fleet = FleetRefTrajectory(paths, pid, traj_horizon=8, traj_dt=0.2)
    frac = np.tile(rng.uniform(0.02, 0.45, ROAD_PER_CELL), len(cells))
    pose = np.empty((B, 3))
    for b in range(B):
        tr = fleet.trajectories[pid[b]]
        i = int(frac[b] * len(tr))
        pose[b] = tr[i, 4], tr[i, 5], tr[i, 3]
    res = {}
    for with_observer in (False, True):
        sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2],
                               road=road_params(B, a_lat=np.array(ROAD_LAT)[ix[:, 0]], df_offset=np.array(ROAD_OFFSET)[ix[:, 1]], a_long=np.array(OBS_LONG)[ix[:, 2]]))
        sim.state[:, 3] = VT
        loop = ClosedLoop(fleet, sim, N=8, target_vel=VT, observer=DisturbanceObserver(B) if with_observer else None)
        loop.run(steps // 2)
        first = loop.score_summary()
        loop.reset_score()
        loop.run(steps - steps // 2)
        second = loop.score_summary()
        n1, n2 = first["n"], second["n"]
        res[with_observer] = dict(rms=np.sqrt((first["sum_ect2"] + second["sum_ect2"]) / np.maximum(n1 + n2, 1)), rms2=second["rms_ect"],
                                  max=np.maximum(first["max_ect"], second["max_ect"]), nonopt=first["n_nonopt"] + second["n_nonopt"],
                                  live=first["n_live"] + second["n_live"], v=sim.state[:, 3].cpu().numpy(),
                                  dist=loop.dist.cpu().numpy() if with_observer else None, finite=bool(torch.isfinite(sim.state).all().item()),
                                  latched=int((second["latch_index"] >= 0).sum()))
    say("%s: 2 x %d vehicles, %d periods of 0.1 s on three paths at %.0f m/s, nominal plant, no noise, no delay, no grip limit; every state finite: %s / %s; "
        "latched vehicles: %d / %d (without / with the observer)" % (torch.cuda.get_device_name(0), B, steps, VT, res[False]["finite"], res[True]["finite"],
                                                                  res[False]["latched"], res[True]["latched"]))
    say("per cell (%d vehicles), without | with DisturbanceObserver: median rms e_ct over the run [m], over its second half [m], largest |e_ct| [m], periods "
        "not Optimal per 1000, median speed at the end [m/s]; then the medians of dpsi-hat [rad], ddelta-hat [rad], da-hat [m/s^2]" % ROAD_PER_CELL)
    for c, (a, o, g) in enumerate(cells):
        sel = (ix[:, 0] == a) & (ix[:, 1] == o) & (ix[:, 2] == g)
        part = []
        for w in (False, True):
            r = res[w]
            part.append("%6.3f %6.3f %6.3f %6.2f %6.3f" % (np.median(r["rms"][sel]), np.median(r["rms2"][sel]), r["max"][sel].max(),
                                                          1000.0 * r["nonopt"][sel].sum() / max(1, r["live"][sel].sum()), np.median(r["v"][sel])))
        d = np.median(res[True]["dist"][sel], 0)
        say("   %.2f m/s^2, %.3f rad, %+.1f m/s^2   %s | %s   %+.4f %+.4f %+.4f" % (ROAD_LAT[a], ROAD_OFFSET[o], OBS_LONG[g], part[0], part[1], d[0], d[1], d[2]))
    T.finish(argv)


OL_DEAD = ((10, 0), (10, 1), (25, 1))     # command delay [updates], age of the fix [periods]: 0.1, 0.2, 0.35 s
OL_SCALE = (1.0, 0.5, 0.25)
OL_PER_CELL = 12
OL_WAYS = ("estimator + compensator", "observer alone", "observer + compensator")


def observer_latency_main():
    """three loops of 3 x 3 x 2 road cells x 3 dead times x 3 q_dist scales of 12 vehicles (the road sweep's first 12 starts, all at 6 m/s, no grip
    limit): the plant's queue and the sensor's stale fix per vehicle, the controller assuming the true delays.  Scored in two halves as --observer."""
    argv = [a for a in sys.argv if a != "--observer-latency"]
    steps = int(argv[2]) if len(argv) > 2 else 200
    paths = [T.path_dict(f) for f in T.FILES]
    cells = list(itertools.product(range(3), range(3), range(2), range(3), range(3)))
    B = len(cells) * OL_PER_CELL
    ix = np.array(cells)[np.repeat(np.arange(len(cells)), OL_PER_CELL)]     # [B,5]: lateral force, steering offset, longitudinal force, dead time, q_dist scale
    rng = np.random.default_rng(0)
    pid = np.tile(np.arange(OL_PER_CELL) % 3, len(cells))
    fleet = FleetRefTrajectory(paths, pid, traj_horizon=8, traj_dt=0.2)
    frac = np.tile(rng.uniform(0.02, 0.45, ROAD_PER_CELL)[:OL_PER_CELL], len(cells))
    pose = np.empty((B, 3))
    for b in range(B):
        tr = fleet.trajectories[pid[b]]
        i = int(frac[b] * len(tr))
        pose[b] = tr[i, 4], tr[i, 5], tr[i, 3]
    cd, md = np.array(OL_DEAD)[ix[:, 3], 0], np.array(OL_DEAD)[ix[:, 3], 1]
    q_dist = np.array(OL_SCALE)[ix[:, 4]][:, None] * np.array((0.002, 0.002, 0.02))[None, :]      # DisturbanceObserver's default, scaled per vehicle
    res = {}
    for way in OL_WAYS:
        sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2], cmd_delay=cd, cmd_queue_depth=4,
                               road=road_params(B, a_lat=np.array(ROAD_LAT)[ix[:, 0]], df_offset=np.array(ROAD_OFFSET)[ix[:, 1]], a_long=np.array(OBS_LONG)[ix[:, 2]]))
        sim.state[:, 3] = VT
        sensor = SensorModel(B, meas_delay=md)
        if way == "estimator + compensator":
            kw = dict(estimator=Estimator.from_sensor(sensor), compensator=LatencyCompensator(B, cmd_delay=cd, meas_delay=md), estimator_input="history")
        elif way == "observer alone":
            kw = dict(observer=DisturbanceObserver(B, q_dist=q_dist))
        else:
            kw = dict(observer=DisturbanceObserver(B, q_dist=q_dist), compensator=LatencyCompensator(B, cmd_delay=cd, meas_delay=md, disturbances=True),
                      estimator_input="history")
        loop = ClosedLoop(fleet, sim, N=8, target_vel=VT, sensor=sensor, **kw)
        loop.run(steps // 2)
        first = loop.score_summary()
        loop.reset_score()
        loop.run(steps - steps // 2)
        second = loop.score_summary()
        n1, n2 = first["n"], second["n"]
        res[way] = dict(rms=np.sqrt((first["sum_ect2"] + second["sum_ect2"]) / np.maximum(n1 + n2, 1)), rms2=second["rms_ect"],
                        max=np.maximum(first["max_ect"], second["max_ect"]), nonopt=first["n_nonopt"] + second["n_nonopt"],
                        live=first["n_live"] + second["n_live"], finite=bool(torch.isfinite(sim.state).all().item()),
                        latched=int((second["latch_index"] >= 0).sum()))
    say("%s: 3 x %d vehicles, %d periods of 0.1 s on three paths at %.0f m/s, nominal plant, no noise, no grip limit; the controller assumes the true delays; "
        "every state finite: %s; latched vehicles: %s; periods not Optimal per 1000: %s (%s)"
        % (torch.cuda.get_device_name(0), B, steps, VT, " / ".join(str(res[w]["finite"]) for w in OL_WAYS), " / ".join(str(res[w]["latched"]) for w in OL_WAYS),
           " / ".join("%.2f" % (1000.0 * res[w]["nonopt"].sum() / max(1, res[w]["live"].sum())) for w in OL_WAYS), " / ".join(OL_WAYS)))
    head = "median rms e_ct over the run [m], over its second half [m], largest |e_ct| [m]: " + " | ".join(OL_WAYS)

    def row(label, sel):
        say("   %-52s %s" % (label, " | ".join("%6.3f %6.3f %7.3f" % (np.median(res[w]["rms"][sel]), np.median(res[w]["rms2"][sel]), res[w]["max"][sel].max())
                                               for w in OL_WAYS)))
    dead = ["%.2f s" % (0.01 * c + 0.1 * m) for c, m in OL_DEAD]
    say("dead time x q_dist scale, over all road cells (%d vehicles per line; the estimator's lines differ by nothing but the cell): " % (18 * OL_PER_CELL) + head)
    for t in range(3):
        for q in range(3):
            row("%s, q_dist x %.2f" % (dead[t], OL_SCALE[q]), (ix[:, 3] == t) & (ix[:, 4] == q))
    say("dead time x q_dist scale, the disturbed corner 1.50 m/s^2 with 0.030 rad, level and on the grade (%d vehicles per line): " % (2 * OL_PER_CELL) + head)
    for t in range(3):
        for q in range(3):
            row("%s, q_dist x %.2f" % (dead[t], OL_SCALE[q]), (ix[:, 0] == 2) & (ix[:, 1] == 2) & (ix[:, 3] == t) & (ix[:, 4] == q))
    say("per road cell at 0.35 s and q_dist x 0.25 (%d vehicles per line): " % OL_PER_CELL + head)
    for a, o, g in itertools.product(range(3), range(3), range(2)):
        row("%.2f m/s^2, %.3f rad, %+.1f m/s^2" % (ROAD_LAT[a], ROAD_OFFSET[o], OBS_LONG[g]),
            (ix[:, 0] == a) & (ix[:, 1] == o) & (ix[:, 2] == g) & (ix[:, 3] == 2) & (ix[:, 4] == 2))
    say("per road cell at 0.10 s and q_dist x 1.00 (%d vehicles per line): " % OL_PER_CELL + head)
    for a, o, g in itertools.product(range(3), range(3), range(2)):
        row("%.2f m/s^2, %.3f rad, %+.1f m/s^2" % (ROAD_LAT[a], ROAD_OFFSET[o], OBS_LONG[g]),
            (ix[:, 0] == a) & (ix[:, 1] == o) & (ix[:, 2] == g) & (ix[:, 3] == 0) & (ix[:, 4] == 0))
    T.finish(argv)


ACT_DEADBAND, ACT_MASS, ACT_FPEAK, ACT_RATIO, ACT_PER_CELL = (0.0, 0.1, 0.2), (0.85, 1.0, 1.3), (2500.0, 6000.0), (0.0, 0.05, -0.05), 12


def actuation_main():
    """two loops of 3 x 3 x 2 x 3 cells of 12 vehicles (the road sweep's first 12 starts, all at 6 m/s): without and with observer=.  The tracking
    figures are those of the run's second half; the controller's counters cover the whole run."""
    from mkz_mpc_path_follower_amd.vehicle_sim import LowLevelController, drive_params
    argv = [a for a in sys.argv if a != "--actuation"]
    steps = int(argv[2]) if len(argv) > 2 else 200
    paths = [T.path_dict(f) for f in T.FILES]
    cells = list(itertools.product(range(3), range(3), range(2), range(3)))
    B = len(cells) * ACT_PER_CELL
    ix = np.array(cells)[np.repeat(np.arange(len(cells)), ACT_PER_CELL)]     # [B,4] grid indices: deadband, mass, F_PEAK, ratio error
    rng = np.random.default_rng(0)
    pid = np.tile(np.arange(ACT_PER_CELL) % 3, len(cells))
    fleet = FleetRefTrajectory(paths, pid, traj_horizon=8, traj_dt=0.2)
    frac = np.tile(rng.uniform(0.02, 0.45, ROAD_PER_CELL)[:ACT_PER_CELL], len(cells))
    pose = np.empty((B, 3))
    for b in range(B):
        tr = fleet.trajectories[pid[b]]
        i = int(frac[b] * len(tr))
        pose[b] = tr[i, 4], tr[i, 5], tr[i, 3]
    d0 = plant_default()
    res = {}
    for with_observer in (False, True):
        llc = LowLevelController(B, v0=VT, brake_deadband=np.array(ACT_DEADBAND)[ix[:, 0]], steer_ratio=14.8 * (1.0 + np.array(ACT_RATIO)[ix[:, 3]]))
        sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2], plant=plant_params(B, m=d0[2] * np.array(ACT_MASS)[ix[:, 1]]),
                               drive=drive_params(B, f_peak=np.array(ACT_FPEAK)[ix[:, 2]]), llc=llc)
        sim.state[:, 3] = VT
        kw = dict(observer=DisturbanceObserver(B), estimator_input="command") if with_observer else {}
        loop = ClosedLoop(fleet, sim, N=8, target_vel=VT, **kw)
        loop.run(steps // 2)
        first = loop.score_summary()
        loop.reset_score()
        v_sum = torch.zeros(B, dtype=torch.float64, device=sim.device)
        for _ in range(steps - steps // 2):
            loop.run(1)
            v_sum += sim.state[:, 3]
        second, c = loop.score_summary(), llc.summary()
        res[with_observer] = dict(rms2=second["rms_ect"], max=np.maximum(first["max_ect"], second["max_ect"]), nonopt=first["n_nonopt"] + second["n_nonopt"],
                                  live=first["n_live"] + second["n_live"], v=(v_sum / (steps - steps // 2)).cpu().numpy(), ctl=c,
                                  dist=loop.dist.cpu().numpy() if with_observer else None, finite=bool(torch.isfinite(sim.state).all().item()),
                                  latched=int((second["latch_index"] >= 0).sum()))
    say("%s: 2 x %d vehicles, %d periods of 0.1 s on three paths at %.0f m/s, pedal-driven plant behind the low-level controller, no noise, no delay, "
        "neutral road; every state finite: %s / %s; latched vehicles: %d / %d; periods not Optimal per 1000: %.2f / %.2f (without / with the observer)"
        % (torch.cuda.get_device_name(0), B, steps, VT, res[False]["finite"], res[True]["finite"], res[False]["latched"], res[True]["latched"],
           1000.0 * res[False]["nonopt"].sum() / max(1, res[False]["live"].sum()), 1000.0 * res[True]["nonopt"].sum() / max(1, res[True]["live"].sum())))
    head = ("without | with DisturbanceObserver: median rms e_ct over the second half [m], largest |e_ct| [m], median of the mean speed over the second half "
            "[m/s], share of ticks in the deadband / braking / throttle saturated [%], median rms(ac - a) [m/s^2]; then the median da-hat [m/s^2]")

    def row(label, sel):
        part = []
        for w in (False, True):
            r, c = res[w], res[w]["ctl"]
            t = max(1, c["ticks"][sel].sum())
            part.append("%6.3f %6.3f %6.3f %5.1f %5.1f %5.1f %6.3f" % (np.median(r["rms2"][sel]), r["max"][sel].max(), np.median(r["v"][sel]),
                                                                       100.0 * c["n_deadband"][sel].sum() / t, 100.0 * c["n_brake"][sel].sum() / t,
                                                                       100.0 * c["n_th_sat"][sel].sum() / t, np.median(c["rms_err"][sel])))
        say("   %-34s %s | %s   %+.4f" % (label, part[0], part[1], np.median(res[True]["dist"][sel, 2])))
    say("per factor level, over all other factors: " + head)
    for f, (name, levels, fmt) in enumerate((("brake deadband [m/s^2]", ACT_DEADBAND, "%.1f"), ("plant mass x", ACT_MASS, "%.2f"), ("F_PEAK [N]", ACT_FPEAK, "%.0f"),
                                             ("steering-ratio error", ACT_RATIO, "%+.2f"))):
        for lv in range(len(levels)):
            row("%s %s" % (name, fmt % levels[lv]), ix[:, f] == lv)
    say("per cell without a ratio error (%d vehicles per line): " % ACT_PER_CELL + head)
    for dbi, mi, fi in itertools.product(range(3), range(3), range(2)):
        row("%.1f m/s^2, mass x %.2f, %4.0f N" % (ACT_DEADBAND[dbi], ACT_MASS[mi], ACT_FPEAK[fi]),
            (ix[:, 0] == dbi) & (ix[:, 1] == mi) & (ix[:, 2] == fi) & (ix[:, 3] == 0))
    T.finish(argv)


OUT_LEN, OUT_BIAS, OUT_PER_CELL = (0, 10, 30, 100), (0.0, 0.02), 48


def outage_main():
    """loops of the road sweep's 48 starts at 6 m/s, nominal plant, no delay, 200 periods, SensorModel(faults=):
    the grid, two loops of 4 x 2 cells (GPS window length x IMU bias, the window's start drawn per vehicle in periods 10 ... 39, no noise): the held
    fix (no filter: the reference's publisher) and estimator=; the outlier row, two loops of 48 (GPS sigma 0.1 m, P_OUTLIER 0.05, OUTLIER_SIGMA 3 m):
    the estimator with gate 0 and with gate 4; the blind_stop row, one loop of 3 x 48 (windows 10 / 30 / 100, MAX_AGE 30, estimator=, blind_stop)."""
    from mkz_mpc_path_follower_amd.vehicle_sim import fault_params
    argv = [a for a in sys.argv if a != "--outage"]
    steps = int(argv[2]) if len(argv) > 2 else 200
    paths = [T.path_dict(f) for f in T.FILES]
    rng = np.random.default_rng(0)
    frac48 = rng.uniform(0.02, 0.45, ROAD_PER_CELL)          # the road sweep's starts
    from48 = rng.integers(10, 40, OUT_PER_CELL).astype(float)

    def run(ncells, faults, sigma=0.0, bias=0.0, estimator=False, gate=0.0, blind_stop=False):
        B = ncells * OUT_PER_CELL
        pid = np.tile(np.arange(OUT_PER_CELL) % 3, ncells)
        fleet = FleetRefTrajectory(paths, pid, traj_horizon=8, traj_dt=0.2)
        frac = np.tile(frac48, ncells)
        pose = np.empty((B, 3))
        for b in range(B):
            tr = fleet.trajectories[pid[b]]
            i = int(frac[b] * len(tr))
            pose[b] = tr[i, 4], tr[i, 5], tr[i, 3]
        sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2])
        sim.state[:, 3] = VT
        sensor = SensorModel(B, sigma=sigma, bias=bias, seed=2024, faults=faults(B))
        kw = dict(estimator=Estimator.from_sensor(sensor, gate=gate)) if estimator else {}
        loop = ClosedLoop(fleet, sim, N=8, target_vel=VT, sensor=sensor, blind_stop=blind_stop, **kw)
        loop.run(steps)
        s = loop.score_summary()
        s["finite"] = bool(torch.isfinite(sim.state).all().item())
        s["resets"] = int((loop.estimator.flags & 32).sum().item()) if estimator else 0
        s["skipped"] = int(loop.estimator.record[:, 15].sum().item()) if estimator else 0
        return s, sensor.fault_summary()

    def cols(s, c, sel):
        return (np.median(s["max_ect"][sel]), s["max_ect"][sel].max(), 1000.0 * s["n_nonopt"][sel].sum() / max(1, s["n_live"][sel].sum()),
                int((s["latch_index"][sel] >= 0).sum()), int(c["n_silent_gps"][sel].sum()), int(c["longest_gps"][sel].max()), int(c["n_outlier"][sel].sum()))
    fmt = "%7.3f %8.3f %7.2f %3d %6d %4d %5d"
    cells = list(itertools.product(range(len(OUT_LEN)), range(len(OUT_BIAS))))
    ix = np.array(cells)[np.repeat(np.arange(len(cells)), OUT_PER_CELL)]       # [B,2] grid indices: window length, IMU bias
    bias = np.zeros((len(ix), 4))
    bias[:, 2] = np.array(OUT_BIAS)[ix[:, 1]]
    grid_rows = lambda B: fault_params(B, win_from_gps=np.tile(from48, len(cells)), win_len_gps=np.array(OUT_LEN, dtype=float)[ix[:, 0]])
    held = run(len(cells), grid_rows, bias=bias)
    filt = run(len(cells), grid_rows, bias=bias, estimator=True)
    say("%s: %d periods of 0.1 s at %.0f m/s on three paths, nominal plant, no delay; every state finite: %s / %s (held fix / estimator=); filter resets: %d"
        % (torch.cuda.get_device_name(0), steps, VT, held[0]["finite"], filt[0]["finite"], filt[0]["resets"]))
    head = ("median over vehicles of the largest |e_ct| [m], largest |e_ct| [m], periods not Optimal per 1000, latched vehicles, GPS-silent vehicle-periods, "
            "longest GPS silence [periods], outlier fixes")
    say("GPS window length x IMU bias, no noise, the window's start drawn per vehicle in periods 10 ... 39 (%d vehicles per line), held fix | estimator=: "
        % OUT_PER_CELL + head)
    for c, (w, b) in enumerate(cells):
        sel = (ix[:, 0] == w) & (ix[:, 1] == b)
        say(("   window %3d periods, IMU bias %.2f rad   " + fmt + "  | " + fmt) % ((OUT_LEN[w], OUT_BIAS[b]) + cols(held[0], held[1], sel) + cols(filt[0], filt[1], sel)))
    sig = (0.1, 0.1, 0.0, 0.0)
    out_rows = lambda B: fault_params(B, p_outlier=0.05, outlier_sigma=3.0)
    g0 = run(1, out_rows, sigma=sig, estimator=True, gate=0.0)
    g4 = run(1, out_rows, sigma=sig, estimator=True, gate=4.0)
    every = np.ones(OUT_PER_CELL, bool)
    say("outlier row: GPS sigma 0.1 m, P_OUTLIER 0.05, OUTLIER_SIGMA 3 m, no window, estimator= with gate 0 | gate 4 (%d vehicles): " % OUT_PER_CELL + head
        + "; then the channel measurements the filter skipped")
    say(("   P_OUTLIER 0.05                          " + fmt + "  | " + fmt + "   %d | %d") % (cols(g0[0], g0[1], every) + cols(g4[0], g4[1], every)
                                                                                              + (g0[0]["skipped"], g4[0]["skipped"])))
    bl = (10, 30, 100)
    bix = np.repeat(np.arange(3), OUT_PER_CELL)
    blind = run(3, lambda B: fault_params(B, win_from_gps=np.tile(from48, 3), win_len_gps=np.array(bl, dtype=float)[bix], max_age=30.0), estimator=True,
                blind_stop=True)
    say("blind_stop row: MAX_AGE 30, estimator=, blind_stop=True, no noise, no bias (%d vehicles per line): " % OUT_PER_CELL + head
        + "; then the earliest and latest latch period")
    for k, w in enumerate(bl):
        sel = bix == k
        li = blind[0]["latch_index"][sel]
        li = li[li >= 0]
        say(("   window %3d periods                       " + fmt + "   %s") % ((w,) + cols(blind[0], blind[1], sel)
                                                                                + (("%d ... %d" % (li.min(), li.max())) if len(li) else "-",)))
    T.finish(argv)


WAN_SIGMA, WAN_TAU = (0.1, 0.2, 0.5), (0.0, 2.0, 10.0, 30.0)             # GPS error [m]; its correlation time [s], 0 = white (the sensor's own noise)
WAN_GUST, WAN_GUST_TAU, WAN_QSCALE = (0.5, 1.0), (0.5, 2.0, 10.0), (None, 1.0, 4.0)   # lateral gust [m/s^2], its tau [s]; no observer, q_dist x 1, x 4
WAN_WALK, WAN_WINDOW = (0.0, 0.003, 0.01), (30, 100)                      # heading walk [rad / sqrt(s)]; GPS window [periods]


def wander_main():
    """loops of the road sweep's 48 starts at 6 m/s, nominal plant, no delay, with wander=vehicle_sim.Wander (seed 2024):
    coloured GPS error, two loops of 3 x 4 cells (sigma x tau; tau = 0 is the sensor's white noise, the others the wander's channels x, y with a
    noiseless sensor), without and with estimator= (r = sigma in every cell: what a user who knows the error's size but not its colour sets);
    gusts, three loops of 2 x 3 cells (a_lat channel, sigma x tau) on a road without a grip limit: no observer, observer= at its default q_dist, at 4 x;
    heading walk, one loop of 2 x 3 cells (GPS window x walk rate on the psi channel), estimator=, the window's start drawn per vehicle as in --outage."""
    from mkz_mpc_path_follower_amd.vehicle_sim import Wander, fault_params, wander_params
    argv = [a for a in sys.argv if a != "--wander"]
    steps = int(argv[2]) if len(argv) > 2 else 300
    paths = [T.path_dict(f) for f in T.FILES]
    rng = np.random.default_rng(0)
    frac48 = rng.uniform(0.02, 0.45, ROAD_PER_CELL)          # the road sweep's starts
    from48 = rng.integers(10, 40, ROAD_PER_CELL).astype(float)

    def run(ncells, sigma8, tau8, walk8=0.0, sensor_sigma=0.0, est_r=None, q_scale=None, road=False, faults=None):
        """one loop of ncells x 48 vehicles -> score summary with `finite`, `latched`, and (sensor given) the rms position error of est / est_filt"""
        B = ncells * ROAD_PER_CELL
        pid = np.tile(np.arange(ROAD_PER_CELL) % 3, ncells)
        fleet = FleetRefTrajectory(paths, pid, traj_horizon=8, traj_dt=0.2)
        frac = np.tile(frac48, ncells)
        pose = np.empty((B, 3))
        for b in range(B):
            tr = fleet.trajectories[pid[b]]
            i = int(frac[b] * len(tr))
            pose[b] = tr[i, 4], tr[i, 5], tr[i, 3]
        sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2], road=road_params(B) if road else None)
        sim.state[:, 3] = VT
        kw = dict(wander=Wander(B, wander_params(B, sigma=sigma8, tau=tau8, walk=walk8), seed=2024))
        if not road:
            kw["sensor"] = SensorModel(B, sigma=sensor_sigma, seed=2024, faults=None if faults is None else faults(B))
        if est_r is not None:
            kw["estimator"] = Estimator(B, r=est_r)
        if q_scale is not None:
            kw["observer"] = DisturbanceObserver(B, q_dist=tuple(q_scale * q for q in (0.002, 0.002, 0.02)))
        loop = ClosedLoop(fleet, sim, N=8, target_vel=VT, **kw)
        hist = loop.run(steps, history=not road)
        s = loop.score_summary()
        s["finite"] = bool(torch.isfinite(sim.state).all().item())
        s["latched"] = int((s["latch_index"] >= 0).sum())
        if not road and faults is None:
            truth = hist["state"][:steps, :, 0:2]
            s["e_raw"] = ((hist["est"][:, :, 0:2] - truth) ** 2).sum(2).mean(0).sqrt().cpu().numpy()
            if est_r is not None:
                s["e_filt"] = ((hist["est_filt"][:, :, 0:2] - truth) ** 2).sum(2).mean(0).sqrt().cpu().numpy()
        return s

    say("%s: %d periods of 0.1 s at %.0f m/s on three paths, nominal plant, no delay, %d vehicles per cell (the road sweep's starts), wander seed 2024"
        % (torch.cuda.get_device_name(0), steps, VT, ROAD_PER_CELL))
    # ---- coloured GPS error
    cells = list(itertools.product(range(len(WAN_SIGMA)), range(len(WAN_TAU))))
    ix = np.array(cells)[np.repeat(np.arange(len(cells)), ROAD_PER_CELL)]
    sg, tau = np.array(WAN_SIGMA)[ix[:, 0]], np.array(WAN_TAU)[ix[:, 1]]
    white = tau == 0.0
    sigma8, tau8, ssig = np.zeros((len(ix), 8)), np.zeros((len(ix), 8)), np.zeros((len(ix), 4))
    sigma8[:, 0] = sigma8[:, 1] = np.where(white, 0.0, sg)
    tau8[:, 0] = tau8[:, 1] = tau
    ssig[:, 0] = ssig[:, 1] = np.where(white, sg, 0.0)
    r = np.tile([1e-3, 1e-3, 1e-4, 1e-3], (len(ix), 1))
    r[:, 0] = r[:, 1] = sg
    raw = run(len(cells), sigma8, tau8, sensor_sigma=ssig)
    flt = run(len(cells), sigma8, tau8, sensor_sigma=ssig, est_r=r)
    say("coloured GPS error on x and y, without | with estimator= (r = sigma): every state finite %s / %s, latched vehicles %d / %d" %
        (raw["finite"], flt["finite"], raw["latched"], flt["latched"]))
    say("   per cell: median rms e_ct [m] without | with, their ratio; median rms position error of what the controller saw against the truth [m] without | with, their ratio")
    for c, (a, t) in enumerate(cells):
        sel = (ix[:, 0] == a) & (ix[:, 1] == t)
        e0, e1 = np.median(raw["rms_ect"][sel]), np.median(flt["rms_ect"][sel])
        p0, p1 = np.median(raw["e_raw"][sel]), np.median(flt["e_filt"][sel])
        say("   sigma %.1f m, %-10s   %6.3f | %6.3f  x %4.2f     %6.3f | %6.3f  x %4.2f" %
            (WAN_SIGMA[a], "white" if WAN_TAU[t] == 0.0 else "tau %g s" % WAN_TAU[t], e0, e1, e1 / e0, p0, p1, p1 / p0))
    # ---- gusts
    cells = list(itertools.product(range(len(WAN_GUST)), range(len(WAN_GUST_TAU))))
    ix = np.array(cells)[np.repeat(np.arange(len(cells)), ROAD_PER_CELL)]
    sigma8, tau8 = np.zeros((len(ix), 8)), np.zeros((len(ix), 8))
    sigma8[:, 5], tau8[:, 5] = np.array(WAN_GUST)[ix[:, 0]], np.array(WAN_GUST_TAU)[ix[:, 1]]
    res = [run(len(cells), sigma8, tau8, q_scale=q, road=True) for q in WAN_QSCALE]
    say("lateral gust (a_lat channel), no grip limit, the truth fed to the controller: no observer | observer= at the default q_dist | at 4 x: every state "
        "finite %s, latched vehicles %s" % (" / ".join(str(x["finite"]) for x in res), " / ".join(str(x["latched"]) for x in res)))
    say("   per cell: median rms e_ct [m] three ways, then the largest |e_ct| [m] three ways")
    for c, (a, t) in enumerate(cells):
        sel = (ix[:, 0] == a) & (ix[:, 1] == t)
        say("   sigma %.1f m/s^2, tau %4.1f s   %6.3f | %6.3f | %6.3f     %6.3f | %6.3f | %6.3f" %
            ((WAN_GUST[a], WAN_GUST_TAU[t]) + tuple(np.median(x["rms_ect"][sel]) for x in res) + tuple(x["max_ect"][sel].max() for x in res)))
    # ---- heading random walk on top of a GPS outage
    cells = list(itertools.product(range(len(WAN_WINDOW)), range(len(WAN_WALK))))
    ix = np.array(cells)[np.repeat(np.arange(len(cells)), ROAD_PER_CELL)]
    walk8 = np.zeros((len(ix), 8))
    walk8[:, 2] = np.array(WAN_WALK)[ix[:, 1]]
    rows = lambda B: fault_params(B, win_from_gps=np.tile(from48, len(cells)), win_len_gps=np.array(WAN_WINDOW, dtype=float)[ix[:, 0]])
    out = run(len(cells), 0.0, 0.0, walk8=walk8, est_r=(0.2, 0.2, 0.02, 0.1), faults=rows)
    say("heading random walk (psi channel) on top of a GPS outage, estimator= (its default r), no other noise: every state finite %s, latched vehicles %d"
        % (out["finite"], out["latched"]))
    say("   per cell: median over vehicles of the largest |e_ct| [m], largest |e_ct| [m], median rms e_ct [m]")
    for c, (w, k) in enumerate(cells):
        sel = (ix[:, 0] == w) & (ix[:, 1] == k)
        say("   window %3d periods, walk %.3f rad/sqrt(s)   %7.3f %8.3f %7.3f" %
            (WAN_WINDOW[w], WAN_WALK[k], np.median(out["max_ect"][sel]), out["max_ect"][sel].max(), np.median(out["rms_ect"][sel])))
    T.finish(argv)


PL_T, PL_DELAY, PL_SIGMA, PL_SIZE, PL_SPACING = (0.5, 1.0, 1.5), (0, 10, 30), (0.0, 0.2), 8, 20.0
PL_PHASES = ((6.0, 100), (3.0, 100), (6.0, 150))     # the leader's target [m/s] and for how many periods
PL_WAYS = ("as it is", "estimator + compensator")


def platoon_main():
    """two loops (as it is; estimator= + compensator= assuming the true delay) of 3 x 3 x 2 cells of three platoons of eight, one per recorded path,
    each platoon on its own copy of its path (54 paths in the set), started 20 m apart at 6 m/s, vehicle 0 of a platoon in front.  The leader's
    target steps 6 -> 3 -> 6 m/s (loop.v_target is edited in place between run() calls); the followers' targets stay 6 m/s."""
    from mkz_mpc_path_follower_amd.ref_traj import Follower, follow_params
    argv = [a for a in sys.argv if a != "--platoon"]
    paths = [T.path_dict(f) for f in T.FILES]
    cells = list(itertools.product(range(3), range(3), range(2)))
    n_pl = 3 * len(cells)
    B = n_pl * PL_SIZE
    platoon = np.repeat(np.arange(n_pl), PL_SIZE)               # platoon q: cell q // 3 on a copy of path q % 3
    rank = np.tile(np.arange(PL_SIZE), n_pl)                    # 0 = the leader, in front
    ix = np.array(cells)[platoon // 3]                          # [B,3] grid indices: headway, delay, sigma
    t_h, cd = np.array(PL_T)[ix[:, 0]], np.array(PL_DELAY)[ix[:, 1]]
    sigma = np.zeros((B, 4))
    sigma[:, 0] = sigma[:, 1] = np.array(PL_SIGMA)[ix[:, 2]]
    steps = sum(n for _, n in PL_PHASES)
    res = {}
    for way in PL_WAYS:
        fleet = FleetRefTrajectory([paths[q % 3] for q in range(n_pl)], platoon, traj_horizon=8, traj_dt=0.2)
        pose = np.empty((B, 3))
        for b in range(B):
            tr = fleet.trajectories[platoon[b]]
            i = int(np.searchsorted(tr[:, 6], 5.0 + PL_SPACING * (PL_SIZE - 1 - rank[b])))
            pose[b] = tr[i, 4], tr[i, 5], tr[i, 3]
        sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2], cmd_delay=cd, cmd_queue_depth=5)
        sim.state[:, 3] = PL_PHASES[0][0]
        sensor = SensorModel(B, sigma=sigma, seed=2024)
        kw = {}
        if way != "as it is":
            kw = dict(estimator=Estimator.from_sensor(sensor), compensator=LatencyCompensator(B, cmd_delay=cd, meas_delay=0), estimator_input="history")
        follower = Follower(fleet, rows=follow_params(B, t_headway=t_h))
        loop = ClosedLoop(fleet, sim, N=8, target_vel=PL_PHASES[0][0], sensor=sensor, follower=follower, **kw)
        speed = []
        for v_lead, n in PL_PHASES:
            loop.v_target[torch.as_tensor(rank == 0, device=sim.device)] = v_lead
            speed.append(loop.run(n, history=True)["state"][1:, :, 3])
        speed = torch.cat(speed, 0).cpu().numpy()               # [steps,B]
        n0 = PL_PHASES[0][1]
        dip = speed[n0 - 40:n0].mean(0) - speed[n0:].min(0)     # the settled speed before the step less the lowest speed after it
        res[way] = dict(f=follower.summary(), s=loop.score_summary(), dip=dip, finite=bool(torch.isfinite(sim.state).all().item()))
    say("%s: 2 x %d vehicles in %d platoons of %d on the three paths, %d periods of 0.1 s, nominal plant; the leader's target steps %s m/s after %s "
        "periods; followers at 6 m/s, default following rows but T_HEADWAY; every state finite: %s; latched vehicles: %s (%s)"
        % (torch.cuda.get_device_name(0), B, n_pl, PL_SIZE, steps, " -> ".join("%g" % v for v, _ in PL_PHASES), " / ".join(str(n) for _, n in PL_PHASES[:-1]),
           " / ".join(str(res[w]["finite"]) for w in PL_WAYS), " / ".join(str(int((res[w]["s"]["latch_index"] >= 0).sum())) for w in PL_WAYS),
           " / ".join(PL_WAYS)))
    say("per cell of three platoons, %s: smallest gap [m], vehicle-periods in contact, speed dip of the last follower / of the first (median of the "
        "three platoons; below 1: the dip shrinks down the platoon), periods not Optimal per 1000" % " | ".join(PL_WAYS))
    for c, (t, dl, g) in enumerate(cells):
        sel = (platoon // 3) == c
        part = []
        for w in PL_WAYS:
            r = res[w]
            ratio = [r["dip"][(platoon == q) & (rank == PL_SIZE - 1)][0] / r["dip"][(platoon == q) & (rank == 1)][0] for q in range(3 * c, 3 * c + 3)]
            part.append("%7.3f %5d %6.3f %7.2f" % (r["f"]["min_gap"][sel].min(), r["f"]["n_contact"][sel].sum(), np.median(ratio),
                                                    1000.0 * r["s"]["n_nonopt"][sel].sum() / max(1, r["s"]["n_live"][sel].sum())))
        say("   T %.1f s, delay %.1f s, GPS sigma %.1f m   %s" % (PL_T[t], 0.01 * PL_DELAY[dl], PL_SIGMA[g], " | ".join(part)))
    T.finish(argv)


RD_SIGMA, RD_DROP, RD_RANGE, RD_FILTER = (0.0, 0.25, 0.5, 1.0), (0.0, 0.1, 0.3), (float("inf"), 30.0, 15.0), (0, 1)
RD_STAND_GAP, RD_STAND_STEPS = 100.0, 400


def _paths():
    paths = [T.path_dict(f) for f in T.FILES]
    return paths


def radar_main():
    """one loop of 4 x 3 x 3 x 2 cells of three platoons of eight (--platoon's, T_HEADWAY 1 s, no command delay), every follower with a range sensor
    of its cell's row (the other words default); then one loop of three pairs on path1, a standing leader RD_STAND_GAP m ahead of a 6 m/s follower,
    one pair per RANGE_MAX with a noise-free sensor."""
    from mkz_mpc_path_follower_amd.ref_traj import Follower, RangeSensor, follow_params, range_params
    argv = [a for a in sys.argv if a != "--radar"]
    paths = _paths()
    cells = list(itertools.product(range(4), range(3), range(3), range(2)))
    n_pl = 3 * len(cells)
    B = n_pl * PL_SIZE
    platoon = np.repeat(np.arange(n_pl), PL_SIZE)
    rank = np.tile(np.arange(PL_SIZE), n_pl)
    ix = np.array(cells)[platoon // 3]                          # [B,4] grid indices: sigma_r, p_drop, range_max, filter
    steps = sum(n for _, n in PL_PHASES)
    fleet = FleetRefTrajectory([paths[q % 3] for q in range(n_pl)], platoon, traj_horizon=8, traj_dt=0.2)
    pose = np.empty((B, 3))
    for b in range(B):
        tr = fleet.trajectories[platoon[b]]
        i = int(np.searchsorted(tr[:, 6], 5.0 + PL_SPACING * (PL_SIZE - 1 - rank[b])))
        pose[b] = tr[i, 4], tr[i, 5], tr[i, 3]
    sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2])
    sim.state[:, 3] = PL_PHASES[0][0]
    radar = RangeSensor(B, rows=range_params(B, sigma_r=np.array(RD_SIGMA)[ix[:, 0]], p_drop=np.array(RD_DROP)[ix[:, 1]],
                                             range_max=np.array(RD_RANGE)[ix[:, 2]], filter=np.array(RD_FILTER)[ix[:, 3]]), seed=77)
    follower = Follower(fleet, rows=follow_params(B), radar=radar)
    loop = ClosedLoop(fleet, sim, N=8, target_vel=PL_PHASES[0][0], sensor=SensorModel(B, sigma=(0.2, 0.2, 0.0, 0.1), seed=2024), follower=follower)
    hist = {k: [] for k in ("state", "v_follow", "gap", "gap_seen", "status")}
    for v_lead, n in PL_PHASES:
        loop.v_target[torch.as_tensor(rank == 0, device=sim.device)] = v_lead
        o = loop.run(n, history=True)
        for k in hist:
            hist[k].append(o[k][1:] if k == "state" else o[k])
    h = {k: torch.cat(v, 0).cpu().numpy() for k, v in hist.items()}
    speed = h["state"][:, :, 3]
    n0 = PL_PHASES[0][1]
    dip = speed[n0 - 40:n0].mean(0) - speed[n0:].min(0)
    f, rs = follower.summary(), radar.summary()
    say("%s: %d vehicles in %d platoons of %d on the three paths, %d periods of 0.1 s, nominal plant, default following rows; the leader's target steps "
        "%s m/s after %s periods; GPS sigma 0.2 m, speed sigma 0.1 m/s, no filter on the ego state; every state finite: %s; latched vehicles: %d"
        % (torch.cuda.get_device_name(0), B, n_pl, PL_SIZE, steps, " -> ".join("%g" % v for v, _ in PL_PHASES),
           " / ".join(str(n) for _, n in PL_PHASES[:-1]), bool(torch.isfinite(sim.state).all().item()), int(loop.command_stop.sum().item())))
    say("per cell of three platoons (21 followers): smallest true gap [m], vehicle-periods in contact, speed dip of the last follower / of the first "
        "(median of the three platoons), rms change of v_follow per period [m/s], rms of GAP_HAT - gap [m] over the tracked periods, share of the "
        "followers' periods with a track, share of Optimal solves")
    fol = rank > 0
    for c, (a, d, r, fl) in enumerate(cells):
        sel = (platoon // 3) == c
        fs = sel & fol
        ratio = [dip[(platoon == q) & (rank == PL_SIZE - 1)][0] / dip[(platoon == q) & (rank == 1)][0] for q in range(3 * c, 3 * c + 3)]
        dv = np.diff(h["v_follow"][:, fs], axis=0)
        tracked = np.isfinite(h["gap_seen"][:, fs]) & np.isfinite(h["gap"][:, fs])
        eg = (h["gap_seen"][:, fs] - h["gap"][:, fs])[tracked]
        say("   SIGMA_R %.2f m, P_DROP %.1f, RANGE_MAX %4s m, FILTER %d   %7.3f %5d %6.3f %7.4f %7.4f %6.3f %7.4f"
            % (RD_SIGMA[a], RD_DROP[d], "inf" if np.isinf(RD_RANGE[r]) else "%g" % RD_RANGE[r], RD_FILTER[fl], f["min_gap"][sel].min(),
               f["n_contact"][sel].sum(), np.median(ratio), np.sqrt((dv * dv).mean()), np.sqrt((eg * eg).mean()) if eg.size else float("nan"),
               tracked.mean(), (h["status"][:, sel] == 0).mean()))
    say("tracks started %d, given up %d; detections %d, dropped %d, out of range %d of %d follower-periods"
        % (rs["n_new"].sum(), rs["n_lost"].sum(), rs["n_detect"].sum(), rs["n_drop"].sum(), rs["n_out"].sum(), int(fol.sum()) * steps))
    # a standing leader: stopping distance against range
    n = len(RD_RANGE)
    tr = FleetRefTrajectory([paths[0]] * n, np.repeat(np.arange(n), 2), traj_horizon=8, traj_dt=0.2)
    pose = np.empty((2 * n, 3))
    for b in range(2 * n):
        t = tr.trajectories[b // 2]
        i = int(np.searchsorted(t[:, 6], 5.0 + (RD_STAND_GAP + 4.9 if b % 2 == 0 else 0.0)))      # even: the standing leader, in front
        pose[b] = t[i, 4], t[i, 5], t[i, 3]
    targets = np.tile([0.0, VT], n)
    sim = VehicleSimulator(2 * n, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2])
    sim.state[:, 3] = torch.as_tensor(targets, device=sim.device)
    radar = RangeSensor(2 * n, rows=range_params(2 * n, sigma_r=0.0, sigma_v=0.0, range_max=np.repeat(RD_RANGE, 2)), seed=78)
    follower = Follower(tr, rows=follow_params(2 * n), radar=radar)
    loop = ClosedLoop(tr, sim, N=8, target_vel=list(targets), follower=follower)
    o = loop.run(RD_STAND_STEPS, history=True)
    gap, v = o["gap"].cpu().numpy(), o["state"][1:, :, 3].cpu().numpy()
    f = follower.summary()
    say("a standing leader %g m ahead of a follower at %g m/s on path1, noise-free sensor, default following row (D_MIN 5 m, A_BRAKE 0.7 m/s^2, "
        "T_HEADWAY 1 s), %d periods; every state finite: %s" % (RD_STAND_GAP, VT, RD_STAND_STEPS, bool(torch.isfinite(sim.state).all().item())))
    for q in range(n):
        b = 2 * q + 1
        first = int(np.argmax(np.isfinite(o["gap_seen"][:, b].cpu().numpy())))
        say("   RANGE_MAX %4s m: first seen at a gap of %7.3f m, smallest gap %7.3f m, last gap %7.3f m, last speed %6.3f m/s, periods in contact %d; the "
            "leader moved %.3f m" % ("inf" if np.isinf(RD_RANGE[q]) else "%g" % RD_RANGE[q], gap[first, b], f["min_gap"][b], gap[-1, b], v[-1, b],
                                     f["n_contact"][b], float(np.hypot(*(o["state"][-1, 2 * q, 0:2] - o["state"][0, 2 * q, 0:2]).cpu().numpy()))))
    T.finish(argv)


OV_SIZE, OV_STEPS, OV_SLOW, OV_FAST = 6, 350, 3.0, 6.0


def overtake_main():
    """--platoon's cells (T_HEADWAY x command delay x GPS sigma) and ways, three platoons of six per cell, one per recorded path on its own copy of it,
    started 20 m apart in lane 0 of two lanes: vehicle 0 of a platoon in front with a 3 m/s target, five behind it at 6 m/s.  default lane rows but
    N_LANES = 2.  The stage reads the truth (a perfect range sensor); delay and noise reach it through how well the vehicles hold their lines."""
    from mkz_mpc_path_follower_amd.ref_traj import Lanes, follow_params, lane_params
    argv = [a for a in sys.argv if a != "--overtake"]
    paths = [T.path_dict(f) for f in T.FILES]
    cells = list(itertools.product(range(3), range(3), range(2)))
    n_pl = 3 * len(cells)
    B = n_pl * OV_SIZE
    platoon = np.repeat(np.arange(n_pl), OV_SIZE)
    rank = np.tile(np.arange(OV_SIZE), n_pl)                    # 0 = the slow vehicle, in front
    ix = np.array(cells)[platoon // 3]
    t_h, cd = np.array(PL_T)[ix[:, 0]], np.array(PL_DELAY)[ix[:, 1]]
    sigma = np.zeros((B, 4))
    sigma[:, 0] = sigma[:, 1] = np.array(PL_SIGMA)[ix[:, 2]]
    targets = np.where(rank == 0, OV_SLOW, OV_FAST)
    res = {}
    for way in PL_WAYS:
        fleet = FleetRefTrajectory([paths[q % 3] for q in range(n_pl)], platoon, traj_horizon=8, traj_dt=0.2)
        pose = np.empty((B, 3))
        for b in range(B):
            tr = fleet.trajectories[platoon[b]]
            i = int(np.searchsorted(tr[:, 6], 5.0 + PL_SPACING * (OV_SIZE - 1 - rank[b])))
            pose[b] = tr[i, 4], tr[i, 5], tr[i, 3]
        sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2], cmd_delay=cd, cmd_queue_depth=5)
        sim.state[:, 3] = torch.as_tensor(targets, device=sim.device)
        sensor = SensorModel(B, sigma=sigma, seed=2024)
        kw = {}
        if way != "as it is":
            kw = dict(estimator=Estimator.from_sensor(sensor), compensator=LatencyCompensator(B, cmd_delay=cd, meas_delay=0), estimator_input="history")
        lanes = Lanes(fleet, follow_rows=follow_params(B, t_headway=t_h), lane_rows=lane_params(B, n_lanes=2))
        loop = ClosedLoop(fleet, sim, N=8, target_vel=targets, sensor=sensor, lanes=lanes, **kw)
        speed = loop.run(OV_STEPS, history=True)["state"][1:, :, 3].mean(0).cpu().numpy()
        res[way] = dict(f=lanes.summary(), s=loop.score_summary(), speed=speed, finite=bool(torch.isfinite(sim.state).all().item()))
    say("%s: 2 x %d vehicles in %d platoons of %d on the three paths, two lanes, %d periods of 0.1 s, nominal plant; vehicle 0 of a platoon in front at "
        "%g m/s, the others behind it at %g m/s, %g m apart; default rows but T_HEADWAY and N_LANES = 2; every state finite: %s; latched vehicles: %s (%s)"
        % (torch.cuda.get_device_name(0), B, n_pl, OV_SIZE, OV_STEPS, OV_SLOW, OV_FAST, PL_SPACING, " / ".join(str(res[w]["finite"]) for w in PL_WAYS),
           " / ".join(str(int((res[w]["s"]["latch_index"] >= 0).sum())) for w in PL_WAYS), " / ".join(PL_WAYS)))
    say("per cell of three platoons (15 fast vehicles), %s: smallest own-lane gap [m], vehicle-periods in contact, lane changes, fast vehicles that end "
        "ahead of their slow one and back in lane 0, mean speed of the fast vehicles [m/s], largest |e_lane| [m], periods not Optimal per 1000"
        % " | ".join(PL_WAYS))
    for c, (t, dl, g) in enumerate(cells):
        sel = (platoon // 3) == c
        fast = sel & (rank > 0)
        part = []
        for w in PL_WAYS:
            r = res[w]
            s_slow = r["s"]["s_along"][sel & (rank == 0)][platoon[fast] - 3 * c]
            done = (r["s"]["s_along"][fast] > s_slow) & (r["f"]["lane"][fast] == 0) & (r["f"]["lane_from"][fast] == 0)
            part.append("%7.3f %4d %4d %3d %6.3f %6.3f %7.2f" % (r["f"]["min_gap"][sel].min(), r["f"]["n_contact"][sel].sum(), r["f"]["n_changes"][sel].sum(),
                                                               done.sum(), r["speed"][fast].mean(), r["f"]["max_elane"][sel].max(),
                                                               1000.0 * r["s"]["n_nonopt"][sel].sum() / max(1, r["s"]["n_live"][sel].sum())))
        say("   T %.1f s, delay %.1f s, GPS sigma %.1f m   %s" % (PL_T[t], 0.01 * PL_DELAY[dl], PL_SIGMA[g], " | ".join(part)))
    T.finish(argv)


if __name__ == "__main__":
    if "--radar" in sys.argv[1:]:
        radar_main()
    elif "--overtake" in sys.argv[1:]:
        overtake_main()
    elif "--platoon" in sys.argv[1:]:
        platoon_main()
    elif "--wander" in sys.argv[1:]:
        wander_main()
    elif "--outage" in sys.argv[1:]:
        outage_main()
    elif "--actuation" in sys.argv[1:]:
        actuation_main()
    elif "--observer-latency" in sys.argv[1:]:
        observer_latency_main()
    elif "--observer" in sys.argv[1:]:
        observer_main()
    elif "--road-profile" in sys.argv[1:]:
        road_profile_main()
    elif "--speed-plan" in sys.argv[1:]:
        speed_plan_main()
    elif "--road" in sys.argv[1:]:
        road_main()
    elif "--latency" in sys.argv[1:]:
        latency_main()
    else:
        main()
