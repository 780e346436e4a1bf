"""Timing of the Frenet reference kernel and of the Frenet fleet loop on one MI355X (-> profiles/frenet_closed_loop.txt).

  1. kmpc_frenet_reference_batch per call at B = 1, 4096, 65 536 for N = 8 and 50, next to kmpc_waypoints_batch on the same poses (the calls go through
     the Python host, so launch overhead is in; windows from the waypoint kernel on tests/golden/path1_decimated.npz, target speeds 1.2 ... 20 m/s);
  2. ClosedLoopFrenet vehicle-steps per second at B = 4096, N = 8, kernel_variant 2 and 3, with the Cartesian ClosedLoop in the same run as the yardstick;
  3. the host route the kernel replaces: the waypoints copied to the host, numpy get_reference_frenet per vehicle, k_poly / z0 copied back, at B = 64
     (one wall-clock measurement per repeat, in turn with the device call).
Method: tools/_timing.py.

usage: python tools/frenet_loop_timing.py [out.txt]
"""
import sys
import time

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd import ClosedLoopFrenet, get_reference_frenet_batch  # noqa: E402
from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop  # noqa: E402
from mkz_mpc_path_follower_amd.kinematic_mpc_frenet import get_reference_frenet  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator  # noqa: E402
import frenet_scenario as FS  # noqa: E402

POSES = dict(frac=0.6, jitter=(1.0, 1.0, 0.2))


def fit_kernel():
    say("1. per call, us (median [min, max] of %d repeats; device events around back-to-back calls through the Python host)" % T.REPEATS)
    say("   %-4s %-7s %-28s %-28s" % ("N", "B", "kmpc_frenet_reference_batch", "kmpc_waypoints_batch"))
    rng = np.random.default_rng(1)
    cases = []
    for N in (8, 50):
        grt, tr = T.single_path(N)
        for B in (1, 4096, 65536):
            pose = torch.as_tensor(T.scatter(tr, B, rng, **dict(POSES, frac=0.5 if N == 50 else 0.6)), device="cuda")
            vt = torch.as_tensor(rng.uniform(1.2, 20.0, B), device="cuda")
            ref, _ = grt.get_waypoints_batch(pose, vt)
            st = get_reference_frenet_batch(pose, ref, vt)[3]
            cases.append(dict(N=N, B=B, grt=grt, pose=pose, vt=vt, ref=ref, refused=int(st.sum().item())))
    run = {}
    for i, c in enumerate(cases):
        reps = 200 if c["B"] <= 4096 else 50
        run[i, "fit"] = (lambda c=c: get_reference_frenet_batch(c["pose"], c["ref"], c["vt"]), reps)
        run[i, "wp"] = (lambda c=c: c["grt"].get_waypoints_batch(c["pose"], c["vt"]), reps)
    res = T.rotate(run)
    for i, c in enumerate(cases):
        say("   %-4d %-7d %8.1f [%7.1f, %7.1f]    %8.1f [%7.1f, %7.1f]    (refused windows: %d)"
            % ((c["N"], c["B"]) + med(res[i, "fit"]) + med(res[i, "wp"]) + (c["refused"],)))


def fleet(B=4096, N=8, vt=5.0, steps=100):
    say("2. fleet loop, B = %d, N = %d, path1 at %.0f m/s, %d steps per repeat after 20 warm-up steps: M vehicle-steps/s (median [min, max] of %d)"
        % (B, N, vt, steps, T.REPEATS))
    grt, tr = T.single_path(N)
    start = T.scatter(tr, B, np.random.default_rng(2), **POSES)

    def make(kind):
        sim = VehicleSimulator(B, X0=start[:, 0], Y0=start[:, 1], Psi0=start[:, 2])
        sim.state[:, 3] = vt
        if kind == "cartesian":
            return ClosedLoop(grt, sim, N=N, target_vel=vt)
        return ClosedLoopFrenet(grt, sim, N, vt, kernel_variant=kind)
    kinds = {"ClosedLoopFrenet kernel_variant=2": 2, "ClosedLoopFrenet kernel_variant=3": 3, "ClosedLoop (Cartesian, yardstick)": "cartesian"}
    res, worst = T.loop_rates(list(kinds), lambda k: make(kinds[k]), B, steps, advance=T.step_periods, after=lambda loop, o: int(o["status"].max().item()))
    for name in kinds:
        say("   %-36s %6.2f [%6.2f, %6.2f]   (worst status of the last step: %d)" % ((name,) + med(res[name]) + (max(worst[name]),)))


def host_route(B=64, N=8):
    say("3. the host route at B = %d, N = %d: waypoints to the host, numpy get_reference_frenet per vehicle, k_poly / z0 back to the device" % (B, N))
    grt, tr = T.single_path(N)
    rng = np.random.default_rng(3)
    pose = torch.as_tensor(T.scatter(tr, B, rng, **POSES), device="cuda")
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
    for _ in range(T.REPEATS):     # not T.rotate(): the host route is ONE call by the wall clock, ending with a synchronisation of its own
        t0 = time.perf_counter(); host(); th.append((time.perf_counter() - t0) * 1e6)
        td.append(T.event_time(lambda: get_reference_frenet_batch(pose, ref, vt), 200))
    m = med(th)
    say("   host route   %9.0f [%9.0f, %9.0f] us per batch = %.0f us per vehicle" % (m + (m[0] / B,)))
    say("   device call  %9.1f [%9.1f, %9.1f] us per batch" % med(td))


def main():
    say(T.header())
    fit_kernel()
    fleet()
    host_route()
    T.finish(sys.argv)


if __name__ == "__main__":
    main()
