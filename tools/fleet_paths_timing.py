"""Timing of the fleet waypoint kernel and of a fleet on mixed paths on one MI355X (-> profiles/fleet_paths_timing.txt).

  1. kmpc_waypoints_fleet at B = 4096 on the three fixture paths (tests/golden/path{1,2,3}_decimated.npz), path ids interleaved (0, 1, 2, 0, ...) and modes mixed
     (every other vehicle on the time grid), next to kmpc_waypoints_batch of the same build on the longest of the three with the same number of vehicles in
     target-velocity mode: device events around REPS back-to-back calls through the Python host, so launch overhead is in;
  2. vehicle-steps per second of ONE mixed ClosedLoop of 4096 vehicles (FleetRefTrajectory, a third of the fleet per path, modes and target speeds mixed)
     against the same vehicles as THREE single-path loops of 1365 / 1366 / 1365 vehicles with a solver handle each, stepped one after another.
Method of DESIGN.md section 4d: the configurations of a group alternate inside one process, five repeats each, median and range.

usage: python tools/fleet_paths_timing.py [out.txt]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mkz_mpc_path_follower_amd import ClosedLoop, FleetRefTrajectory  # noqa: E402
from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory, path_arrays  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator  # noqa: E402
import scenario as S  # noqa: E402

REPEATS, B, N = 5, 4096, 8
FILES = ("path1_decimated.npz", "path2_decimated.npz", "path3_decimated.npz")
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def path_dict(name):
    arr, lat0, lon0 = S.path_arrays(name)
    return dict(arr, lat0=lat0, lon0=lon0)


def poses(tr, n, rng, frac=0.6):
    idx = rng.integers(0, int(frac * len(tr)), n)
    return np.stack([tr[idx, 4] + rng.uniform(-1, 1, n), tr[idx, 5] + rng.uniform(-1, 1, n), tr[idx, 3] + rng.uniform(-0.2, 0.2, n)], 1)


def event_time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps   # us per call


def fleet_setup(paths, rng):
    """B vehicles, ids interleaved, every other vehicle in time mode, target speeds 3 ... 9 m/s -> (path_id, time_mode, start poses, target speeds, [M,7] arrays)"""
    pid = np.arange(B) % len(paths)
    tm = (np.arange(B) // len(paths)) % 2
    trs = [np.column_stack(path_arrays(p["t"], p["lat"], p["lon"], p["psi"], p["lat0"], p["lon0"])) for p in paths]
    pose = np.empty((B, 3))
    for p, tr in enumerate(trs):
        sel = np.where(pid == p)[0]
        pose[sel] = poses(tr, len(sel), rng)
    return pid, tm, pose, rng.uniform(3.0, 9.0, B), trs


def kernels(paths):
    rng = np.random.default_rng(1)
    pid, tm, pose, vt, trs = fleet_setup(paths, rng)
    fleet = FleetRefTrajectory(paths, pid, tm, traj_horizon=N)
    longest = int(np.argmax([len(t) for t in trs]))
    single = GPSRefTrajectory(arrays=paths[longest], traj_horizon=N, lat0=paths[longest]["lat0"], lon0=paths[longest]["lon0"])
    pose_f, vt_d = torch.as_tensor(pose, device="cuda"), torch.as_tensor(vt, device="cuda")
    pose_s = torch.as_tensor(poses(trs[longest], B, rng), device="cuda")
    tf, ts = [], []
    for _ in range(REPEATS):   # alternating
        tf.append(event_time(lambda: fleet.get_waypoints_batch(pose_f, vt_d), 200))
        ts.append(event_time(lambda: single.get_waypoints_batch(pose_s, vt_d), 200))
    say("1. per call at B = %d, N = %d, us (median [min, max] of %d repeats; device events around 200 back-to-back calls through the Python host)" % (B, N, REPEATS))
    say("   kmpc_waypoints_fleet, paths of %s samples, ids interleaved, every other vehicle in time mode:  %7.1f [%7.1f, %7.1f]" % ((", ".join(str(len(t)) for t in trs),) + med(tf)))
    say("   kmpc_waypoints_batch, %s (%d samples), target-velocity mode:                              %7.1f [%7.1f, %7.1f]" % ((FILES[longest], len(trs[longest])) + med(ts)))
    say("   ratio of the medians fleet / single: %.3f   (single-path kernel's own range: %.3f)" % (med(tf)[0] / med(ts)[0], med(ts)[2] / med(ts)[1]))


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
    kinds = [("one mixed ClosedLoop of %d vehicles" % B, mixed), ("three single-path loops of %s vehicles, one after another" % "/".join(str((pid == p).sum()) for p in range(3)), split)]
    res = {k: [] for k, _ in kinds}
    worst = {k: 0 for k, _ in kinds}
    for _ in range(REPEATS):
        for name, build in kinds:
            ls = build()
            for _w in range(20):
                for l in ls:
                    l.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _s in range(steps):
                for l in ls:
                    o = l.step()
            torch.cuda.synchronize()
            res[name].append(B * steps / (time.perf_counter() - t0) / 1e6)
            worst[name] = max(worst[name], int(o["status"].max().item()))
    say("2. fleet loop, %d vehicles, N = %d, %d steps per repeat after 20 warm-up steps: M vehicle-steps/s (median [min, max] of %d)" % (B, N, steps, REPEATS))
    for name, _ in kinds:
        say("   %-62s %6.2f [%6.2f, %6.2f]   (worst status of the last step: %d)" % ((name,) + med(res[name]) + (worst[name],)))
    say("   ratio of the medians mixed / split: %.2f" % (med(res[kinds[0][0]])[0] / med(res[kinds[1][0]])[0]))


def main():
    paths = [path_dict(f) for f in FILES]
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    kernels(paths)
    loops(paths)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
