"""Timing of the speed plan on one MI355X (-> profiles/speed_plan_timing.txt).

  1. kmpc_speed_plan_fleet next to kmpc_waypoints_fleet of the same build at B = 4096 and B = 262144 on the three fixture paths
     (tests/golden/path{1,2,3}_decimated.npz), path ids interleaved, every vehicle in target-velocity mode, the same poses; the calls go through the
     Python host, so launch overhead is in.  The plan runs its own nearest-sample pass; the ratio is what fusing it
     into the waypoint launch could save at most.  The plan is timed on the default rows at 8 m/s (few samples ahead can bind: the early exit ends
     the pass after the first chunks) and once more with a_brake 0.05 (the braking window exceeds every path: the pass runs to the path's end).
  2. vehicle-steps per second of ONE ClosedLoop of 4096 vehicles on the three paths without and with planner=.
Method: tools/_timing.py.  kmpc_pathset_curvature is timed once (it runs once per path set).

usage: python tools/speed_plan_timing.py [out.txt]
"""
import ctypes as C
import sys

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd import ClosedLoop, FleetRefTrajectory  # noqa: E402
from mkz_mpc_path_follower_amd.ref_traj import SpeedPlanner, speed_plan_params  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator  # noqa: E402

N = T.N


def kernels(paths, B, reps):
    fleet, pose = T.interleaved_fleet(paths, B, np.random.default_rng(1))
    pose_d = torch.as_tensor(pose, device="cuda")
    vt = torch.full((B,), 8.0, dtype=torch.float64, device="cuda")
    short = SpeedPlanner(fleet)
    full = SpeedPlanner(fleet, rows=speed_plan_params(B, a_brake=0.05))
    out = torch.empty((B,), dtype=torch.float64, device="cuda")
    t = T.rotate({"waypoints": (lambda: fleet.get_waypoints_batch(pose_d, vt), reps), "short": (lambda: short.plan(pose_d, vt, out=out), reps),
                  "full": (lambda: full.plan(pose_d, vt, out=out), reps)})
    tw, ts, tf = med(t["waypoints"]), med(t["short"]), med(t["full"])
    limited = int((short.plan(pose_d, vt) < vt).sum().item())
    say("   B = %d (%d of them limited on the default rows):" % (B, limited))
    say("     kmpc_waypoints_fleet, target-velocity mode:                          %8.1f [%8.1f, %8.1f]" % tw)
    say("     kmpc_speed_plan_fleet, default rows (early exit after the first chunks): %8.1f [%8.1f, %8.1f]   %.3f x the waypoint call" % (ts + (ts[0] / tw[0],)))
    say("     kmpc_speed_plan_fleet, a_brake 0.05 (the pass runs to the path's end):   %8.1f [%8.1f, %8.1f]   %.3f x the waypoint call" % (tf + (tf[0] / tw[0],)))
    return fleet


def loops(paths, B=4096, steps=100):
    rng = np.random.default_rng(2)
    _, pose = T.interleaved_fleet(paths, B, rng)
    pid = np.arange(B) % len(paths)
    vt = rng.uniform(3.0, 9.0, B)

    def make(planned):
        fleet = FleetRefTrajectory(paths, pid, traj_horizon=N)
        sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2])
        sim.state[:, 3] = torch.as_tensor(vt, device=sim.device)
        return ClosedLoop(fleet, sim, N=N, target_vel=vt, planner=SpeedPlanner(fleet) if planned else None)

    def last_step(loop, o):
        return int(o["status"].max().item()), float(o["iters"].double().mean().item()), int(o["iters"].max().item())
    kinds = {"without a planner": False, "with planner= (default rows)": True}
    res, last = T.loop_rates(list(kinds), lambda k: make(kinds[k]), B, steps, advance=T.step_periods, after=last_step)
    say("2. ClosedLoop of %d vehicles on the three paths, N = %d, target speeds 3 ... 9 m/s, %d steps per repeat after 20 warm-up steps: M vehicle-steps/s "
        "(median [min, max] of %d)" % (B, N, steps, T.REPEATS))
    for name in kinds:
        say("   %-32s %6.2f [%6.2f, %6.2f]   (worst status of the last step: %d; its solver iterations: mean %.2f, most %d)"
            % ((name,) + med(res[name]) + (max(s for s, _, _ in last[name]),) + last[name][-1][1:]))
    without, with_ = kinds
    say("   ratio of the medians with / without: %.3f" % (med(res[with_])[0] / med(res[without])[0]))


def main():
    paths = [T.path_dict(f) for f in T.FILES]
    say(T.header())
    say("1. per call, N = %d, us (median [min, max] of %d repeats; device events around back-to-back calls through the Python host: 200 at B = 4096, 20 at "
        "B = 262144)" % (N, T.REPEATS))
    fleet = kernels(paths, 4096, 200)
    kernels(paths, 262144, 20)
    kap = torch.empty((sum(len(t) for t in fleet.trajectories),), dtype=torch.float64, device="cuda")
    t = T.event_time(lambda: fleet._lib.kmpc_pathset_curvature(fleet._h, 4.0, C.c_void_p(kap.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)), 200)
    say("   kmpc_pathset_curvature, %d samples in three paths, window 4 m: %.1f us per call (once per path set)" % (kap.shape[0], t))
    loops(paths)
    T.finish(sys.argv)


if __name__ == "__main__":
    main()
