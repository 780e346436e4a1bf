"""Timing of the speed plan on one MI355X (-> profiles/speed_plan_timing.txt).

  1. kmpc_speed_plan_fleet next to kmpc_waypoints_fleet of the same build at B = 4096 and B = 262144 on the three fixture paths
     (tests/golden/path{1,2,3}_decimated.npz), path ids interleaved, every vehicle in target-velocity mode, the same poses: device events around REPS
     back-to-back calls through the Python host, so launch overhead is in.  The plan runs its own nearest-sample pass; the ratio is what fusing it
     into the waypoint launch could save at most.  The plan is timed on the default rows at 8 m/s (few samples ahead can bind: the early exit ends
     the pass after the first chunks) and once more with a_brake 0.05 (the braking window exceeds every path: the pass runs to the path's end).
  2. vehicle-steps per second of ONE ClosedLoop of 4096 vehicles on the three paths without and with planner=.
Method of tools/fleet_paths_timing.py: the configurations of a group alternate inside one process, five repeats each, median
and range.  kmpc_pathset_curvature is timed once (it runs once per path set).

usage: python tools/speed_plan_timing.py [out.txt]
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
from mkz_mpc_path_follower_amd.ref_traj import SpeedPlanner, speed_plan_params  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator  # noqa: E402
import scenario as S  # noqa: E402

REPEATS, N = 5, 8
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


def setup(paths, B, rng, frac=0.6):
    """B vehicles, ids interleaved, poses within 1 m of a sample of the first 60 % of the vehicle's path -> fleet, pose [B,3] (host)"""
    pid = np.arange(B) % len(paths)
    fleet = FleetRefTrajectory(paths, pid, traj_horizon=N)
    pose = np.empty((B, 3))
    for p, tr in enumerate(fleet.trajectories):
        sel = np.where(pid == p)[0]
        idx = rng.integers(0, int(frac * len(tr)), len(sel))
        pose[sel] = np.stack([tr[idx, 4] + rng.uniform(-1, 1, len(sel)), tr[idx, 5] + rng.uniform(-1, 1, len(sel)), tr[idx, 3] + rng.uniform(-0.2, 0.2, len(sel))], 1)
    return fleet, pose


def kernels(paths, B, reps):
    rng = np.random.default_rng(1)
    fleet, pose = setup(paths, B, rng)
    pose_d = torch.as_tensor(pose, device="cuda")
    vt = torch.full((B,), 8.0, dtype=torch.float64, device="cuda")
    short = SpeedPlanner(fleet)
    full = SpeedPlanner(fleet, rows=speed_plan_params(B, a_brake=0.05))
    out = torch.empty((B,), dtype=torch.float64, device="cuda")
    tw, ts, tf = [], [], []
    for _ in range(REPEATS):   # alternating
        tw.append(event_time(lambda: fleet.get_waypoints_batch(pose_d, vt), reps))
        ts.append(event_time(lambda: short.plan(pose_d, vt, out=out), reps))
        tf.append(event_time(lambda: full.plan(pose_d, vt, out=out), reps))
    limited = int((short.plan(pose_d, vt) < vt).sum().item())
    say("   B = %d (%d of them limited on the default rows):" % (B, limited))
    say("     kmpc_waypoints_fleet, target-velocity mode:                          %8.1f [%8.1f, %8.1f]" % med(tw))
    say("     kmpc_speed_plan_fleet, default rows (early exit after the first chunks): %8.1f [%8.1f, %8.1f]   %.3f x the waypoint call" % (med(ts) + (med(ts)[0] / med(tw)[0],)))
    say("     kmpc_speed_plan_fleet, a_brake 0.05 (the pass runs to the path's end):   %8.1f [%8.1f, %8.1f]   %.3f x the waypoint call" % (med(tf) + (med(tf)[0] / med(tw)[0],)))
    return fleet


def loops(paths, B=4096, steps=100):
    rng = np.random.default_rng(2)
    _, pose = setup(paths, B, rng)
    pid = np.arange(B) % len(paths)
    vt = rng.uniform(3.0, 9.0, B)

    def make(planned):
        fleet = FleetRefTrajectory(paths, pid, traj_horizon=N)
        sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2])
        sim.state[:, 3] = torch.as_tensor(vt, device=sim.device)
        return ClosedLoop(fleet, sim, N=N, target_vel=vt, planner=SpeedPlanner(fleet) if planned else None)
    kinds = [("without a planner", False), ("with planner= (default rows)", True)]
    res = {k: [] for k, _ in kinds}
    worst = {k: 0 for k, _ in kinds}
    iters = {k: (0.0, 0) for k, _ in kinds}
    for _ in range(REPEATS):
        for name, planned in kinds:
            loop = make(planned)
            for _w in range(20):
                loop.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _s in range(steps):
                o = loop.step()
            torch.cuda.synchronize()
            res[name].append(B * steps / (time.perf_counter() - t0) / 1e6)
            worst[name] = max(worst[name], int(o["status"].max().item()))
            iters[name] = (float(o["iters"].double().mean().item()), int(o["iters"].max().item()))
    say("2. ClosedLoop of %d vehicles on the three paths, N = %d, target speeds 3 ... 9 m/s, %d steps per repeat after 20 warm-up steps: M vehicle-steps/s "
        "(median [min, max] of %d)" % (B, N, steps, REPEATS))
    for name, _ in kinds:
        say("   %-32s %6.2f [%6.2f, %6.2f]   (worst status of the last step: %d; its solver iterations: mean %.2f, most %d)"
            % ((name,) + med(res[name]) + (worst[name],) + iters[name]))
    say("   ratio of the medians with / without: %.3f" % (med(res[kinds[1][0]])[0] / med(res[kinds[0][0]])[0]))


def main():
    paths = [path_dict(f) for f in FILES]
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    say("1. per call, N = %d, us (median [min, max] of %d repeats; device events around back-to-back calls through the Python host: 200 at B = 4096, 20 at "
        "B = 262144)" % (N, REPEATS))
    fleet = kernels(paths, 4096, 200)
    kernels(paths, 262144, 20)
    kap = torch.empty((sum(len(t) for t in fleet.trajectories),), dtype=torch.float64, device="cuda")
    import ctypes as C
    t = event_time(lambda: fleet._lib.kmpc_pathset_curvature(fleet._h, 4.0, C.c_void_p(kap.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)), 200)
    say("   kmpc_pathset_curvature, %d samples in three paths, window 4 m: %.1f us per call (once per path set)" % (kap.shape[0], t))
    loops(paths)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
