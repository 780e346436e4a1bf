"""Timing of the tracking-score kernel and of scored episodes on one MI355X (-> profiles/track_score_timing.txt).

  1. kmpc_track_score_fleet next to kmpc_waypoints_fleet at B = 4096 on the three fixture paths, path ids interleaved; the calls go through the Python
     host, so launch overhead is in.  The score call runs with its command side and the record, as in a scored period.
  2. ClosedLoop.run(100) of 4096 vehicles scored against the same run unscored (the kernel's cost inside the loop), and against 100 x step() of THIS tree
     (step() and run() share the period's body; the parent commit itself is not measured by this tool).
  3. a scored run(100) + ONE score download against the host route the tests took before: step(), a download of the state, the command, the status and the latch
     and numpy cross_track per vehicle every period (256 vehicles: the host route is slow).  Both routes are timed by the wall clock from a fresh loop to
     the scores on the host, once per repeat, in turn.
Method: tools/_timing.py.

usage: python tools/track_score_timing.py [out.txt]
"""
import sys
import time

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd import ClosedLoop, FleetRefTrajectory  # noqa: E402
from mkz_mpc_path_follower_amd.ref_traj import fresh_score, path_arrays  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator  # noqa: E402
import scenario as S  # noqa: E402

B, N = 4096, 8


def setup(paths, nb, rng):
    pid = (np.arange(nb) % len(paths)).astype(np.int32)
    trs = [np.column_stack(path_arrays(p["t"], p["lat"], p["lon"], p["psi"], p["lat0"], p["lon0"])) for p in paths]
    pose = T.scatter_fleet(trs, pid, rng, frac=0.5)
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
    res = T.rotate({"score": (lambda: fleet.track_score_batch(state, score=score, out=out, **side), 200),
                    "waypoints": (lambda: fleet.get_waypoints_batch(pose_d, vt_d), 200)})
    ts, tw = med(res["score"]), med(res["waypoints"])
    say("1. per call at B = %d, paths of %s samples, ids interleaved, us (median [min, max] of %d repeats; device events around 200 back-to-back calls through the Python host)"
        % (B, ", ".join(str(len(t)) for t in trs), T.REPEATS))
    say("   kmpc_track_score_fleet (state [B,8], command side, record):  %7.1f [%7.1f, %7.1f]" % ts)
    say("   kmpc_waypoints_fleet (N = %d, target-velocity mode):           %7.1f [%7.1f, %7.1f]" % ((N,) + tw))
    say("   ratio of the medians score / waypoints: %.2f" % (ts[0] / tw[0]))
    fleet.close()


def episodes(paths, steps=100):
    rng = np.random.default_rng(2)
    pid, pose, vt, _ = setup(paths, B, rng)
    kinds = {"run(%d), scored" % steps: "scored", "run(%d), unscored" % steps: "unscored", "%d x step()" % steps: "steps"}

    def make(name):             # warmed up here, by the unscored run() whatever the kind times (caches, the solver's warm start): loop_rates' warm = 0
        loop = make_loop(paths, pid, pose, vt)
        loop.run(20, score=False)
        return loop, kinds[name]

    def advance(case, n):
        loop, kind = case
        if n and kind == "steps":
            T.step_periods(loop, n)
        elif n:
            loop.run(n, score=kind == "scored")
    rates, _ = T.loop_rates(list(kinds), make, B, steps, warm=0, advance=advance, after=lambda case, last: case[0].grt.close())
    res = {name: [B / r for r in rates[name]] for name in kinds}     # M vehicle-steps/s -> us per period
    say("2. one mixed ClosedLoop of %d vehicles, N = %d, after 20 warm-up periods: us per period, wall clock with a synchronisation at the end (median [min, max] of %d)" % (B, N, T.REPEATS))
    for name in kinds:
        say("   %-22s %8.1f [%8.1f, %8.1f]" % ((name,) + med(res[name])))
    m = {kinds[name]: med(res[name])[0] for name in kinds}
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
    for _ in range(T.REPEATS):     # not T.loop_rates(): no warm-up belongs to either route, and what is timed ends on the host
        a, sm = device_route()
        b, ect = host()
        td.append(a); th.append(b)
    say("3. %d vehicles, %d periods, from a fresh loop to the scores on the host: s (median [min, max] of %d)" % (nb, steps, T.REPEATS))
    say("   run(%d) scored on the device + one download of the record:        %8.3f [%8.3f, %8.3f]" % ((steps,) + med(td)))
    say("   step() + downloads + numpy cross_track per vehicle, every period:  %8.3f [%8.3f, %8.3f]" % med(th))
    say("   ratio of the medians host / device: %.1f; largest |max e_ct (device) - max e_ct (host)|: %.2e m" % (med(th)[0] / med(td)[0], np.abs(sm["max_ect"] - ect.max(0)).max()))


def main():
    paths = [T.path_dict(f) for f in T.FILES]
    say(T.header())
    kernels(paths)
    episodes(paths)
    host_route(paths)
    T.finish(sys.argv)


if __name__ == "__main__":
    main()
