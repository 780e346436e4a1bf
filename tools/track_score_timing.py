"""Timing of the tracking-score kernel and of scored episodes on one MI355X (-> profiles/track_score_timing.txt).

  1. kmpc_track_score_fleet next to kmpc_waypoints_fleet at B = 4096 on the three fixture paths, path ids interleaved: device events around 200 back-to-back
     calls through the Python host, so launch overhead is in.  The score call runs with its command side and the record, as in a scored period.
  2. ClosedLoop.run(100) of 4096 vehicles scored against the same run unscored (the kernel's cost inside the loop), and against 100 x step() of THIS tree
     (step() and run() share the period's body; the parent commit itself is not measured by this tool).
  3. a scored run(100) + ONE score download against the host route the tests took before: step(), a download of the state, the command, the status and the latch
     and numpy cross_track per vehicle every period (256 vehicles: the host route is slow).
Method of DESIGN.md section 4d: the cases of a group alternate inside one process, five repeats each, median and range.

usage: python tools/track_score_timing.py [out.txt]
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
from mkz_mpc_path_follower_amd.ref_traj import fresh_score, path_arrays  # noqa: E402
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


def setup(paths, nb, rng):
    pid = (np.arange(nb) % len(paths)).astype(np.int32)
    trs = [np.column_stack(path_arrays(p["t"], p["lat"], p["lon"], p["psi"], p["lat0"], p["lon0"])) for p in paths]
    pose = np.empty((nb, 3))
    for p, tr in enumerate(trs):
        sel = np.where(pid == p)[0]
        idx = rng.integers(0, int(0.5 * len(tr)), len(sel))
        pose[sel] = np.stack([tr[idx, 4] + rng.uniform(-1, 1, len(sel)), tr[idx, 5] + rng.uniform(-1, 1, len(sel)), tr[idx, 3] + rng.uniform(-0.2, 0.2, len(sel))], 1)
    return pid, pose, rng.uniform(3.0, 9.0, nb), trs


def make_loop(paths, pid, pose, vt):
    sim = VehicleSimulator(len(pid), X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2])
    sim.state[:, 3] = torch.as_tensor(vt, device=sim.device)
    return ClosedLoop(FleetRefTrajectory(paths, pid, traj_horizon=N), sim, N=N, target_vel=vt)


def kernels(paths):
    rng = np.random.default_rng(1)
    pid, pose, vt, trs = setup(paths, B, rng)
    fleet = FleetRefTrajectory(paths, pid, traj_horizon=N)
    dev = fleet.device
    state = torch.zeros((B, 8), dtype=torch.float64, device=dev)
    state[:, 0:3] = torch.as_tensor(pose, device=dev)
    pose_d, vt_d = state[:, 0:3].contiguous(), torch.as_tensor(vt, device=dev)
    side = dict(status=torch.zeros(B, dtype=torch.int32, device=dev), iters=torch.full((B,), 5, dtype=torch.int32, device=dev),
                cmd=torch.zeros((B, 2), dtype=torch.float64, device=dev), stop_latch=torch.zeros(B, dtype=torch.uint8, device=dev))
    score, out = fresh_score(B, dev), {}
    ts, tw = [], []
    for _ in range(REPEATS):   # alternating
        ts.append(event_time(lambda: fleet.track_score_batch(state, score=score, out=out, **side), 200))
        tw.append(event_time(lambda: fleet.get_waypoints_batch(pose_d, vt_d), 200))
    say("1. per call at B = %d, paths of %s samples, ids interleaved, us (median [min, max] of %d repeats; device events around 200 back-to-back calls through the Python host)"
        % (B, ", ".join(str(len(t)) for t in trs), REPEATS))
    say("   kmpc_track_score_fleet (state [B,8], command side, record):  %7.1f [%7.1f, %7.1f]" % med(ts))
    say("   kmpc_waypoints_fleet (N = %d, target-velocity mode):           %7.1f [%7.1f, %7.1f]" % ((N,) + med(tw)))
    say("   ratio of the medians score / waypoints: %.2f" % (med(ts)[0] / med(tw)[0]))
    fleet.close()


def episodes(paths, steps=100):
    rng = np.random.default_rng(2)
    pid, pose, vt, _ = setup(paths, B, rng)

    def run_case(kind):
        loop = make_loop(paths, pid, pose, vt)
        loop.run(20, score=False)   # warm-up: caches, the solver's warm start
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "steps":
            for _ in range(steps):
                loop.step()
        else:
            loop.run(steps, score=kind == "scored")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        loop.grt.close()
        return dt / steps * 1e6   # us per period
    kinds = [("run(%d), scored" % steps, "scored"), ("run(%d), unscored" % steps, "unscored"), ("%d x step()" % steps, "steps")]
    res = {k: [] for k, _ in kinds}
    for _ in range(REPEATS):
        for name, kind in kinds:
            res[name].append(run_case(kind))
    say("2. one mixed ClosedLoop of %d vehicles, N = %d, after 20 warm-up periods: us per period, wall clock with a synchronisation at the end (median [min, max] of %d)" % (B, N, REPEATS))
    for name, _ in kinds:
        say("   %-22s %8.1f [%8.1f, %8.1f]" % ((name,) + med(res[name])))
    m = {k: med(res[n])[0] for n, k in kinds}
    say("   scored - unscored: %.1f us per period; unscored run / step() loop: %.3f" % (m["scored"] - m["unscored"], m["unscored"] / m["steps"]))
    say("   (the step() loop is THIS tree's: step() and run() share the period's body; it is not a measurement of the parent commit)")


def host_route(paths, nb=256, steps=100):
    rng = np.random.default_rng(3)
    pid, pose, vt, trs = setup(paths, nb, rng)

    def device_route():
        loop = make_loop(paths, pid, pose, vt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop.run(steps)
        sm = loop.score_summary()
        dt = time.perf_counter() - t0
        loop.grt.close()
        return dt, sm

    def host():
        loop = make_loop(paths, pid, pose, vt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = [loop.sim.state.cpu().numpy().copy()]
        for _ in range(steps):
            o = loop.step()
            o["cmd"].cpu(); o["status"].cpu(); loop.command_stop.cpu()
            st.append(loop.sim.state.cpu().numpy().copy())
        st = np.array(st)
        ect = np.stack([S.cross_track(trs[pid[b]][:, 4:6], st[:, b, 0], st[:, b, 1])[0] for b in range(nb)], 1)
        dt = time.perf_counter() - t0
        loop.grt.close()
        return dt, ect
    td, th = [], []
    for _ in range(REPEATS):
        a, sm = device_route()
        b, ect = host()
        td.append(a); th.append(b)
    say("3. %d vehicles, %d periods, from a fresh loop to the scores on the host: s (median [min, max] of %d)" % (nb, steps, REPEATS))
    say("   run(%d) scored on the device + one download of the record:        %8.3f [%8.3f, %8.3f]" % ((steps,) + med(td)))
    say("   step() + downloads + numpy cross_track per vehicle, every period:  %8.3f [%8.3f, %8.3f]" % med(th))
    say("   ratio of the medians host / device: %.1f; largest |max e_ct (device) - max e_ct (host)|: %.2e m" % (med(th)[0] / med(td)[0], np.abs(sm["max_ect"] - ect.max(0)).max()))


def main():
    paths = [path_dict(f) for f in FILES]
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    kernels(paths)
    episodes(paths)
    host_route(paths)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
