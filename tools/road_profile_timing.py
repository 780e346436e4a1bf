"""Timing of the road profile on one MI355X (-> profiles/road_profile_timing.txt).

  1. kmpc_road_profile_fleet next to kmpc_waypoints_fleet of the same build at B = 4096 and B = 262144 on the three fixture paths
     (tests/golden/path{1,2,3}_decimated.npz), path ids interleaved, the same poses: both are dominated by the same nearest-sample pass, so the ratio
     is what reusing another stage's `closest` could save at most.
  2. kmpc_speed_plan_fleet_profile (neutral map: the same limits, so the same early exits) and this build's kmpc_speed_plan_fleet next to
     kmpc_speed_plan_fleet of a library built from the PARENT commit (KMPC_PARENT_LIB names it; loaded into the same process next to this build's, its
     own path set made from the same arrays), on the default rows at 8 m/s and with a_brake 0.05 (the pass runs to the path's end).  Without
     KMPC_PARENT_LIB the parent's columns are left out and said to be.
  3. vehicle-steps per second of ONE ClosedLoop of 4096 vehicles on the three paths (VehicleSimulator(road=)) without and with road_profile=.
Method of tools/speed_plan_timing.py: device events around back-to-back calls through the Python host (launch overhead is
in), the configurations of a group alternate inside one process, five repeats each after a warm-up call, median and range.

usage: [KMPC_PARENT_LIB=parent/libkmpc_hip.so] python tools/road_profile_timing.py [out.txt]
"""
import ctypes as C
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
from mkz_mpc_path_follower_amd.vehicle_sim import RoadProfile, VehicleSimulator, road_params  # noqa: E402
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


class ParentPlan:
    """kmpc_speed_plan_fleet of another build of the library, on a path set of its own made from the fleet's arrays"""

    def __init__(self, path, fleet):
        L = C.CDLL(os.path.abspath(path))
        vp, i32, dp = C.c_void_p, C.c_int32, C.POINTER(C.c_double)
        L.kmpc_pathset_create.argtypes = [i32, i32, C.POINTER(i32), dp, dp, dp, dp, dp, C.POINTER(vp)]
        L.kmpc_pathset_curvature.argtypes = [vp, C.c_double, vp, vp]
        L.kmpc_speed_plan_fleet.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
        M = np.array([len(tr) for tr in fleet.trajectories], dtype=np.int32)
        cols = [np.ascontiguousarray(np.concatenate([tr[:, i] for tr in fleet.trajectories])) for i in (0, 4, 5, 3, 6)]
        h = vp()
        assert L.kmpc_pathset_create(0, len(M), M.ctypes.data_as(C.POINTER(i32)), *[c.ctypes.data_as(dp) for c in cols], C.byref(h)) == 0
        self.L, self.h, self.fleet = L, h, fleet
        self.kappa = torch.empty((int(M.sum()),), dtype=torch.float64, device="cuda")
        assert L.kmpc_pathset_curvature(h, 4.0, vp(self.kappa.data_ptr()), vp(torch.cuda.current_stream().cuda_stream)) == 0

    def plan(self, pose, vt, rows, out):
        p = lambda t: C.c_void_p(t.data_ptr())
        rc = self.L.kmpc_speed_plan_fleet(self.h, pose.shape[0], p(self.kappa), p(pose), int(pose.stride(0)), p(self.fleet.path_id), p(vt), p(rows), p(out), None,
                                          None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        return out


def kernels(paths, B, reps, parent_lib):
    rng = np.random.default_rng(1)
    fleet, pose = setup(paths, B, rng)
    pose_d = torch.as_tensor(pose, device="cuda")
    vt = torch.full((B,), 8.0, dtype=torch.float64, device="cuda")
    prof = RoadProfile(fleet)
    base, road = road_params(B, mu=1.0), torch.empty((B, 8), dtype=torch.float64, device="cuda")
    out = torch.empty((B,), dtype=torch.float64, device="cuda")
    say("   B = %d:" % B)
    tw, tr = [], []
    for _ in range(REPEATS):   # alternating
        tw.append(event_time(lambda: fleet.get_waypoints_batch(pose_d, vt), reps))
        tr.append(event_time(lambda: prof.apply(pose_d, base, road), reps))
    say("     kmpc_waypoints_fleet, target-velocity mode:                    %8.1f [%8.1f, %8.1f]" % med(tw))
    say("     kmpc_road_profile_fleet:                                       %8.1f [%8.1f, %8.1f]   %.3f x the waypoint call" % (med(tr) + (med(tr)[0] / med(tw)[0],)))
    parent = ParentPlan(parent_lib, fleet) if parent_lib else None
    for label, kw in (("default rows (early exit after the first chunks)", {}), ("a_brake 0.05 (the pass runs to the path's end)", dict(a_brake=0.05))):
        rows = speed_plan_params(B, **kw)
        plain, mapped = SpeedPlanner(fleet, rows=rows), SpeedPlanner(fleet, rows=rows, profile=prof)
        t0, t1, tp = [], [], []
        for _ in range(REPEATS):
            if parent:
                tp.append(event_time(lambda: parent.plan(pose_d, vt, rows, out), reps))
            t0.append(event_time(lambda: plain.plan(pose_d, vt, out=out), reps))
            t1.append(event_time(lambda: mapped.plan(pose_d, vt, out=out), reps))
        same = torch.equal(plain.plan(pose_d, vt), mapped.plan(pose_d, vt))
        if parent:
            same = same and torch.equal(plain.plan(pose_d, vt), parent.plan(pose_d, vt, rows, torch.empty_like(out)))
        say("     %s; outputs of all builds and both entries identical: %s" % (label, same))
        if parent:
            say("       kmpc_speed_plan_fleet, parent build:                         %8.1f [%8.1f, %8.1f]" % med(tp))
        ref = med(tp)[0] if parent else med(t0)[0]
        say("       kmpc_speed_plan_fleet, this build:                           %8.1f [%8.1f, %8.1f]   %.3f x %s"
            % (med(t0) + (med(t0)[0] / ref, "the parent's" if parent else "itself (no parent build given: not measured)")))
        say("       kmpc_speed_plan_fleet_profile, neutral map:                  %8.1f [%8.1f, %8.1f]   %.3f x %s"
            % (med(t1) + (med(t1)[0] / ref, "the parent's kmpc_speed_plan_fleet" if parent else "this build's kmpc_speed_plan_fleet")))


def loops(paths, B=4096, steps=100):
    rng = np.random.default_rng(2)
    _, pose = setup(paths, B, rng)
    pid = np.arange(B) % len(paths)
    vt = rng.uniform(3.0, 9.0, B)

    def make(profiled):
        fleet = FleetRefTrajectory(paths, pid, traj_horizon=N)
        sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2], road=road_params(B, mu=1.0),
                               road_profile=RoadProfile(fleet) if profiled else None)
        sim.state[:, 3] = torch.as_tensor(vt, device=sim.device)
        return ClosedLoop(fleet, sim, N=N, target_vel=vt)
    kinds = [("road= alone", False), ("road= and road_profile= (neutral table)", True)]
    res = {k: [] for k, _ in kinds}
    worst = {k: 0 for k, _ in kinds}
    for _ in range(REPEATS):
        for name, profiled in kinds:
            loop = make(profiled)
            for _w in range(20):
                loop.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _s in range(steps):
                o = loop.step()
            torch.cuda.synchronize()
            res[name].append(B * steps / (time.perf_counter() - t0) / 1e6)
            worst[name] = max(worst[name], int(o["status"].max().item()))
    say("3. ClosedLoop of %d vehicles on the three paths, N = %d, road mu = 1.0, target speeds 3 ... 9 m/s, %d steps per repeat after 20 warm-up steps: "
        "M vehicle-steps/s (median [min, max] of %d)" % (B, N, steps, REPEATS))
    for name, _ in kinds:
        say("   %-42s %6.2f [%6.2f, %6.2f]   (worst status of the last step: %d)" % ((name,) + med(res[name]) + (worst[name],)))
    say("   ratio of the medians with / without: %.3f" % (med(res[kinds[1][0]])[0] / med(res[kinds[0][0]])[0]))


def main():
    paths = [path_dict(f) for f in FILES]
    parent_lib = os.environ.get("KMPC_PARENT_LIB")
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    say("1., 2. per call, N = %d, us (median [min, max] of %d repeats; device events around back-to-back calls through the Python host: 200 at B = 4096, "
        "20 at B = 262144); parent build: %s" % (N, REPEATS, "given" if parent_lib else "not given, its columns are not measured"))
    kernels(paths, 4096, 200, parent_lib)
    kernels(paths, 262144, 20, parent_lib)
    loops(paths)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
