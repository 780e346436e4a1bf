"""Timing of the road profile on one MI355X (-> profiles/road_profile_timing.txt).

  1. kmpc_road_profile_fleet next to kmpc_waypoints_fleet of the same build at B = 4096 and B = 262144 on the three fixture paths
     (tests/golden/path{1,2,3}_decimated.npz), path ids interleaved, the same poses: both are dominated by the same nearest-sample pass, so the ratio
     is what reusing another stage's `closest` could save at most.
  2. kmpc_speed_plan_fleet_profile (neutral map: the same limits, so the same early exits) and this build's kmpc_speed_plan_fleet next to
     kmpc_speed_plan_fleet of a library built from the PARENT commit (KMPC_PARENT_LIB names it; loaded into the same process next to this build's, its
     own path set made from the same arrays), on the default rows at 8 m/s and with a_brake 0.05 (the pass runs to the path's end).  Without
     KMPC_PARENT_LIB the parent's columns are left out and said to be.
  3. vehicle-steps per second of ONE ClosedLoop of 4096 vehicles on the three paths (VehicleSimulator(road=)) without and with road_profile=.
Method: tools/_timing.py; the calls go through the Python host, so launch overhead is in.

usage: [KMPC_PARENT_LIB=parent/libkmpc_hip.so] python tools/road_profile_timing.py [out.txt]
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd import ClosedLoop, FleetRefTrajectory  # noqa: E402
from mkz_mpc_path_follower_amd.ref_traj import SpeedPlanner, speed_plan_params  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import RoadProfile, VehicleSimulator, road_params  # noqa: E402

N = T.N


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
    fleet, pose = T.interleaved_fleet(paths, B, np.random.default_rng(1))
    pose_d = torch.as_tensor(pose, device="cuda")
    vt = torch.full((B,), 8.0, dtype=torch.float64, device="cuda")
    prof = RoadProfile(fleet)
    base, road = road_params(B, mu=1.0), torch.empty((B, 8), dtype=torch.float64, device="cuda")
    out = torch.empty((B,), dtype=torch.float64, device="cuda")
    say("   B = %d:" % B)
    t = T.rotate({"waypoints": (lambda: fleet.get_waypoints_batch(pose_d, vt), reps), "profile": (lambda: prof.apply(pose_d, base, road), reps)})
    tw, tr = med(t["waypoints"]), med(t["profile"])
    say("     kmpc_waypoints_fleet, target-velocity mode:                    %8.1f [%8.1f, %8.1f]" % tw)
    say("     kmpc_road_profile_fleet:                                       %8.1f [%8.1f, %8.1f]   %.3f x the waypoint call" % (tr + (tr[0] / tw[0],)))
    parent = ParentPlan(parent_lib, fleet) if parent_lib else None
    for label, kw in (("default rows (early exit after the first chunks)", {}), ("a_brake 0.05 (the pass runs to the path's end)", dict(a_brake=0.05))):
        rows = speed_plan_params(B, **kw)
        plain, mapped = SpeedPlanner(fleet, rows=rows), SpeedPlanner(fleet, rows=rows, profile=prof)
        cases = {"parent": (lambda: parent.plan(pose_d, vt, rows, out), reps)} if parent else {}
        cases.update(plain=(lambda: plain.plan(pose_d, vt, out=out), reps), mapped=(lambda: mapped.plan(pose_d, vt, out=out), reps))
        t = {k: med(v) for k, v in T.rotate(cases).items()}
        t0, t1 = t["plain"], t["mapped"]
        same = torch.equal(plain.plan(pose_d, vt), mapped.plan(pose_d, vt))
        if parent:
            same = same and torch.equal(plain.plan(pose_d, vt), parent.plan(pose_d, vt, rows, torch.empty_like(out)))
        say("     %s; outputs of all builds and both entries identical: %s" % (label, same))
        if parent:
            say("       kmpc_speed_plan_fleet, parent build:                         %8.1f [%8.1f, %8.1f]" % t["parent"])
        ref = t["parent"][0] if parent else t0[0]
        say("       kmpc_speed_plan_fleet, this build:                           %8.1f [%8.1f, %8.1f]   %.3f x %s"
            % (t0 + (t0[0] / ref, "the parent's" if parent else "itself (no parent build given: not measured)")))
        say("       kmpc_speed_plan_fleet_profile, neutral map:                  %8.1f [%8.1f, %8.1f]   %.3f x %s"
            % (t1 + (t1[0] / ref, "the parent's kmpc_speed_plan_fleet" if parent else "this build's kmpc_speed_plan_fleet")))


def loops(paths, B=4096, steps=100):
    rng = np.random.default_rng(2)
    _, pose = T.interleaved_fleet(paths, B, rng)
    pid = np.arange(B) % len(paths)
    vt = rng.uniform(3.0, 9.0, B)

    def make(profiled):
        fleet = FleetRefTrajectory(paths, pid, traj_horizon=N)
        sim = VehicleSimulator(B, X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2], road=road_params(B, mu=1.0),
                               road_profile=RoadProfile(fleet) if profiled else None)
        sim.state[:, 3] = torch.as_tensor(vt, device=sim.device)
        return ClosedLoop(fleet, sim, N=N, target_vel=vt)
    kinds = {"road= alone": False, "road= and road_profile= (neutral table)": True}
    res, worst = T.loop_rates(list(kinds), lambda k: make(kinds[k]), B, steps, advance=T.step_periods, after=lambda loop, o: int(o["status"].max().item()))
    say("3. ClosedLoop of %d vehicles on the three paths, N = %d, road mu = 1.0, target speeds 3 ... 9 m/s, %d steps per repeat after 20 warm-up steps: "
        "M vehicle-steps/s (median [min, max] of %d)" % (B, N, steps, T.REPEATS))
    for name in kinds:
        say("   %-42s %6.2f [%6.2f, %6.2f]   (worst status of the last step: %d)" % ((name,) + med(res[name]) + (max(worst[name]),)))
    without, with_ = kinds
    say("   ratio of the medians with / without: %.3f" % (med(res[with_])[0] / med(res[without])[0]))


def main():
    paths = [T.path_dict(f) for f in T.FILES]
    parent_lib = os.environ.get("KMPC_PARENT_LIB")
    say(T.header())
    say("1., 2. per call, N = %d, us (median [min, max] of %d repeats; device events around back-to-back calls through the Python host: 200 at B = 4096, "
        "20 at B = 262144); parent build: %s" % (N, T.REPEATS, "given" if parent_lib else "not given, its columns are not measured"))
    kernels(paths, 4096, 200, parent_lib)
    kernels(paths, 262144, 20, parent_lib)
    loops(paths)
    T.finish(sys.argv)


if __name__ == "__main__":
    main()
