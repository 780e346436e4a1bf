"""Timing of the fleet waypoint kernel and of a fleet on mixed paths on one MI355X (-> profiles/fleet_paths_timing.txt).

  1. kmpc_waypoints_fleet at B = 4096 on the three fixture paths (tests/golden/path{1,2,3}_decimated.npz), path ids interleaved (0, 1, 2, 0, ...) and modes mixed
     (every other vehicle on the time grid), next to kmpc_waypoints_batch of the same build on the longest of the three with the same number of vehicles in
     target-velocity mode; the calls go through the Python host, so launch overhead is in;
  2. vehicle-steps per second of ONE mixed ClosedLoop of 4096 vehicles (FleetRefTrajectory, a third of the fleet per path, modes and target speeds mixed)
     against the same vehicles as THREE single-path loops of 1365 / 1366 / 1365 vehicles with a solver handle each, stepped one after another.
Method: tools/_timing.py.

usage: python tools/fleet_paths_timing.py [out.txt]
"""
import sys

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd import ClosedLoop, FleetRefTrajectory  # noqa: E402
from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory, path_arrays  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator  # noqa: E402

B, N = 4096, 8


def fleet_setup(paths, rng):
    """B vehicles, ids interleaved, every other vehicle in time mode, target speeds 3 ... 9 m/s -> (path_id, time_mode, start poses, target speeds, [M,7] arrays)"""
    pid = np.arange(B) % len(paths)
    tm = (np.arange(B) // len(paths)) % 2
    trs = [np.column_stack(path_arrays(p["t"], p["lat"], p["lon"], p["psi"], p["lat0"], p["lon0"])) for p in paths]
    pose = T.scatter_fleet(trs, pid, rng)
    return pid, tm, pose, rng.uniform(3.0, 9.0, B), trs


def kernels(paths):
    rng = np.random.default_rng(1)
    pid, tm, pose, vt, trs = fleet_setup(paths, rng)
    fleet = FleetRefTrajectory(paths, pid, tm, traj_horizon=N)
    longest = int(np.argmax([len(t) for t in trs]))
    single = GPSRefTrajectory(arrays=paths[longest], traj_horizon=N, lat0=paths[longest]["lat0"], lon0=paths[longest]["lon0"])
    pose_f, vt_d = torch.as_tensor(pose, device="cuda"), torch.as_tensor(vt, device="cuda")
    pose_s = torch.as_tensor(T.scatter(trs[longest], B, rng, 0.6, (1.0, 1.0, 0.2)), device="cuda")
    res = T.rotate({"fleet": (lambda: fleet.get_waypoints_batch(pose_f, vt_d), 200), "single": (lambda: single.get_waypoints_batch(pose_s, vt_d), 200)})
    tf, ts = med(res["fleet"]), med(res["single"])
    say("1. per call at B = %d, N = %d, us (median [min, max] of %d repeats; device events around 200 back-to-back calls through the Python host)" % (B, N, T.REPEATS))
    say("   kmpc_waypoints_fleet, paths of %s samples, ids interleaved, every other vehicle in time mode:  %7.1f [%7.1f, %7.1f]" % ((", ".join(str(len(t)) for t in trs),) + tf))
    say("   kmpc_waypoints_batch, %s (%d samples), target-velocity mode:                              %7.1f [%7.1f, %7.1f]" % ((T.FILES[longest], len(trs[longest])) + ts))
    say("   ratio of the medians fleet / single: %.3f   (single-path kernel's own range: %.3f)" % (tf[0] / ts[0], ts[2] / ts[1]))


def loops(paths, steps=100):
    rng = np.random.default_rng(2)
    pid, tm, pose, vt, _ = fleet_setup(paths, rng)

    def make(sel, sub_paths, ids):
        sim = VehicleSimulator(len(sel), X0=pose[sel, 0], Y0=pose[sel, 1], Psi0=pose[sel, 2])
        sim.state[:, 3] = torch.as_tensor(vt[sel], device=sim.device)
        return ClosedLoop(FleetRefTrajectory(sub_paths, ids, tm[sel], traj_horizon=N), sim, N=N, target_vel=vt[sel])

    def mixed():
        return [make(np.arange(B), paths, pid)]

    def split():
        return [make(np.where(pid == p)[0], [paths[p]], np.zeros((pid == p).sum(), dtype=np.int32)) for p in range(len(paths))]

    def advance(ls, n):     # the loops of a kind one after another, period by period
        for _ in range(n):
            for l in ls:
                o = l.step()
        return o
    kinds = {"one mixed ClosedLoop of %d vehicles" % B: mixed,
             "three single-path loops of %s vehicles, one after another" % "/".join(str((pid == p).sum()) for p in range(3)): split}
    res, worst = T.loop_rates(list(kinds), lambda k: kinds[k](), B, steps, advance=advance, after=lambda ls, o: int(o["status"].max().item()))
    say("2. fleet loop, %d vehicles, N = %d, %d steps per repeat after 20 warm-up steps: M vehicle-steps/s (median [min, max] of %d)" % (B, N, steps, T.REPEATS))
    for name in kinds:
        say("   %-62s %6.2f [%6.2f, %6.2f]   (worst status of the last step: %d)" % ((name,) + med(res[name]) + (max(worst[name]),)))
    one, three = kinds
    say("   ratio of the medians mixed / split: %.2f" % (med(res[one])[0] / med(res[three])[0]))


def main():
    paths = [T.path_dict(f) for f in T.FILES]
    say(T.header())
    kernels(paths)
    loops(paths)
    T.finish(sys.argv)


if __name__ == "__main__":
    main()
