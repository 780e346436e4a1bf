"""Timing of the Frenet reference kernel and of the Frenet fleet loop on one MI355X (-> profiles/frenet_closed_loop.txt).

  1. kmpc_frenet_reference_batch per call at B = 1, 4096, 65 536 for N = 8 and 50, next to kmpc_waypoints_batch on the same poses (device events around
     REPS back-to-back calls, so launch overhead is in; windows from the waypoint kernel on tests/golden/path1_decimated.npz, target speeds 1.2 ... 20 m/s);
  2. ClosedLoopFrenet vehicle-steps per second at B = 4096, N = 8, kernel_variant 2 and 3, with the Cartesian ClosedLoop in the same run as the yardstick;
  3. the host route the kernel replaces: the waypoints copied to the host, numpy get_reference_frenet per vehicle, k_poly / z0 copied back, at B = 64.
Method of DESIGN.md section 4d: the configurations of a group alternate inside one process, five repeats each, median and range.

usage: python tools/frenet_loop_timing.py [out.txt]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mkz_mpc_path_follower_amd import ClosedLoopFrenet, get_reference_frenet_batch  # noqa: E402
from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop  # noqa: E402
from mkz_mpc_path_follower_amd.kinematic_mpc_frenet import get_reference_frenet  # noqa: E402
from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator  # noqa: E402
import frenet_scenario as FS  # noqa: E402

REPEATS = 5
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def poses(tr, B, rng, frac=0.6):
    idx = rng.integers(0, int(frac * len(tr)), B)
    return np.stack([tr[idx, 4] + rng.uniform(-1, 1, B), tr[idx, 5] + rng.uniform(-1, 1, B), tr[idx, 3] + rng.uniform(-0.2, 0.2, B)], 1)


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


def fit_kernel(arr, lat0, lon0):
    say("1. per call, us (median [min, max] of %d repeats; device events around back-to-back calls through the Python host)" % REPEATS)
    say("   %-4s %-7s %-28s %-28s" % ("N", "B", "kmpc_frenet_reference_batch", "kmpc_waypoints_batch"))
    rng = np.random.default_rng(1)
    cases = []
    for N in (8, 50):
        grt = GPSRefTrajectory(arrays=arr, traj_horizon=N, traj_dt=0.2, lat0=lat0, lon0=lon0)
        tr = grt.get_global_trajectory_reference()
        for B in (1, 4096, 65536):
            pose = torch.as_tensor(poses(tr, B, rng, 0.5 if N == 50 else 0.6), device="cuda")
            vt = torch.as_tensor(rng.uniform(1.2, 20.0, B), device="cuda")
            ref, _ = grt.get_waypoints_batch(pose, vt)
            st = get_reference_frenet_batch(pose, ref, vt)[3]
            cases.append(dict(N=N, B=B, grt=grt, pose=pose, vt=vt, ref=ref, refused=int(st.sum().item()), fit=[], wp=[]))
    for _ in range(REPEATS):
        for c in cases:   # alternating
            reps = 200 if c["B"] <= 4096 else 50
            c["fit"].append(event_time(lambda: get_reference_frenet_batch(c["pose"], c["ref"], c["vt"]), reps))
            c["wp"].append(event_time(lambda: c["grt"].get_waypoints_batch(c["pose"], c["vt"]), reps))
    for c in cases:
        say("   %-4d %-7d %8.1f [%7.1f, %7.1f]    %8.1f [%7.1f, %7.1f]    (refused windows: %d)" % ((c["N"], c["B"]) + med(c["fit"]) + med(c["wp"]) + (c["refused"],)))


def fleet(arr, lat0, lon0, B=4096, N=8, vt=5.0, steps=100):
    say("2. fleet loop, B = %d, N = %d, path1 at %.0f m/s, %d steps per repeat after 20 warm-up steps: M vehicle-steps/s (median [min, max] of %d)"
        % (B, N, vt, steps, REPEATS))
    grt = GPSRefTrajectory(arrays=arr, traj_horizon=N, traj_dt=0.2, lat0=lat0, lon0=lon0)
    tr = grt.get_global_trajectory_reference()
    start = poses(tr, B, np.random.default_rng(2))

    def make(kind):
        sim = VehicleSimulator(B, X0=start[:, 0], Y0=start[:, 1], Psi0=start[:, 2])
        sim.state[:, 3] = vt
        if kind == "cartesian":
            return ClosedLoop(grt, sim, N=N, target_vel=vt)
        return ClosedLoopFrenet(grt, sim, N, vt, kernel_variant=kind)
    kinds = [("ClosedLoopFrenet kernel_variant=2", 2), ("ClosedLoopFrenet kernel_variant=3", 3), ("ClosedLoop (Cartesian, yardstick)", "cartesian")]
    res = {k: [] for k, _ in kinds}
    worst = {k: 0 for k, _ in kinds}
    for _ in range(REPEATS):
        for name, kind in kinds:
            loop = make(kind)
            for _w in range(20):
                loop.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _s in range(steps):
                o = loop.step()
            torch.cuda.synchronize()
            res[name].append(B * steps / (time.perf_counter() - t0) / 1e6)
            worst[name] = max(worst[name], int(o["status"].max().item()))
    for name, _ in kinds:
        say("   %-36s %6.2f [%6.2f, %6.2f]   (worst status of the last step: %d)" % ((name,) + med(res[name]) + (worst[name],)))


def host_route(arr, lat0, lon0, B=64, N=8):
    say("3. the host route at B = %d, N = %d: waypoints to the host, numpy get_reference_frenet per vehicle, k_poly / z0 back to the device" % (B, N))
    grt = GPSRefTrajectory(arrays=arr, traj_horizon=N, traj_dt=0.2, lat0=lat0, lon0=lon0)
    tr = grt.get_global_trajectory_reference()
    rng = np.random.default_rng(3)
    pose = torch.as_tensor(poses(tr, B, rng), device="cuda")
    vt = torch.as_tensor(rng.uniform(3.0, 12.0, B), device="cuda")
    ref, _ = grt.get_waypoints_batch(pose, vt)

    def host():
        p, r, v = pose.cpu().numpy(), ref.cpu().numpy(), vt.cpu().numpy()
        K, z = np.empty((B, 4)), np.zeros((B, 4))
        for b in range(B):
            K[b], ps, _, _ = get_reference_frenet(FS.vehicle_frame_path(p[b], r[b, :, 0], r[b, :, 1]))
            z[b] = (0.0, 0.0, -ps, v[b])
        out = torch.as_tensor(K, device="cuda"), torch.as_tensor(z, device="cuda")
        torch.cuda.synchronize()
        return out
    th, td = [], []
    for _ in range(REPEATS):
        t0 = time.perf_counter(); host(); th.append((time.perf_counter() - t0) * 1e6)
        td.append(event_time(lambda: get_reference_frenet_batch(pose, ref, vt), 200))
    m = med(th)
    say("   host route   %9.0f [%9.0f, %9.0f] us per batch = %.0f us per vehicle" % (m + (m[0] / B,)))
    say("   device call  %9.1f [%9.1f, %9.1f] us per batch" % med(td))


def main():
    arr, lat0, lon0 = FS.path_arrays("path1_decimated.npz")
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    fit_kernel(arr, lat0, lon0)
    fleet(arr, lat0, lon0)
    host_route(arr, lat0, lon0)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
