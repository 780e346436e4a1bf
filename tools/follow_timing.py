"""Timing of car following on one MI355X (-> profiles/follow_timing.txt).

  1. kmpc_follow_fleet next to kmpc_waypoints_fleet of the same build at B = 4096, 32768 and 262144 on the three fixture paths
     (tests/golden/path{1,2,3}_decimated.npz), path ids interleaved, random poses: a dense fleet, nearly every vehicle has a leader; device events
     around REPS back-to-back calls through the Python host, so launch overhead is in.  The stage is timed as the kernel alone (arclengths given) and as
     Follower.cap() (the geometry-only kmpc_track_score_fleet call, the on-the-road mask and the kernel); the score call is timed separately.
     The pair search is B^2 comparisons whatever the paths are: the number of paths changes how many candidates match, not how many are read.
  2. vehicle-steps per second of ONE ClosedLoop of 4096 vehicles without and with follower=: 512 platoons of eight, 20 m apart at 6 m/s, each on
     its own copy of a fixture path, so that the cap rarely binds and both loops solve the same problems.
  `python tools/follow_timing.py plain` prints the rate of the loop without follower= alone, five repeats: run alternately on this build and on
  the parent commit's (KMPC_TREE=<its checkout>), it shows that a loop without the stage costs what it cost.
Method of tools/fleet_paths_timing.py: the configurations of a group alternate inside one process, five repeats each, median
and range.

usage: python tools/follow_timing.py [plain | out.txt]
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("KMPC_TREE", HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "tests"))

from mkz_mpc_path_follower_amd import ClosedLoop, FleetRefTrajectory  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator  # noqa: E402
import scenario as S  # noqa: E402

REPEATS, N, PLATOON, SPACING = 5, 8, 8, 20.0
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


def setup(B, n_paths):
    """B vehicles in platoons of PLATOON on n_paths copies of the fixture paths (path p is fixture p % 3): platoon q on path q % n_paths, its
    vehicles SPACING m apart from 5 m + 170 m * (q // n_paths) on, first vehicle in front -> fleet, state [B,8] (host; at the samples' headings, 6 m/s)"""
    base = [path_dict(f) for f in FILES]
    fleet_paths = [base[p % 3] for p in range(n_paths)]
    q = np.arange(B) // PLATOON
    pid = (q % n_paths).astype(np.int32)
    fleet = FleetRefTrajectory(fleet_paths, pid, traj_horizon=N)
    state = np.zeros((B, 8))
    s_want = 5.0 + 170.0 * (q // n_paths) + SPACING * (PLATOON - 1 - np.arange(B) % PLATOON)
    for p in range(min(n_paths, 3)):
        tr = fleet.trajectories[p]
        sel = np.flatnonzero(pid % 3 == p)
        assert s_want[sel].max() < tr[-1, 6] - 60.0, "path %d is too short for %d platoons" % (p, q.max() // n_paths + 1)
        idx = np.searchsorted(tr[:, 6], s_want[sel])
        state[sel, 0], state[sel, 1], state[sel, 2] = tr[idx, 4], tr[idx, 5], tr[idx, 3]
    state[:, 3] = 6.0
    return fleet, state


def kernels(B, reps):
    """the three fixture paths, ids interleaved, poses within 1 m of a random sample of the vehicle's path, speeds U(2, 8): a dense fleet in which
    nearly every vehicle has a leader"""
    from mkz_mpc_path_follower_amd._stage import ptr, stream
    from mkz_mpc_path_follower_amd.ref_traj import Follower
    rng = np.random.default_rng(1)
    paths = [path_dict(f) for f in FILES]
    pid = np.arange(B) % 3
    fleet = FleetRefTrajectory(paths, pid, traj_horizon=N)
    state = np.zeros((B, 8))
    for p, tr in enumerate(fleet.trajectories):
        sel = np.where(pid == p)[0]
        idx = rng.integers(0, int(0.6 * len(tr)), len(sel))
        state[sel, 0], state[sel, 1], state[sel, 2] = tr[idx, 4] + rng.uniform(-1, 1, len(sel)), tr[idx, 5] + rng.uniform(-1, 1, len(sel)), tr[idx, 3]
    state[:, 3] = rng.uniform(2.0, 8.0, B)
    st = torch.as_tensor(state, device="cuda")
    pose = st[:, 0:3].contiguous()
    vt = torch.full((B,), 6.0, dtype=torch.float64, device="cuda")
    fo = Follower(fleet)
    out = torch.empty((B,), dtype=torch.float64, device="cuda")
    fo.cap(st, vt, out=out)
    torch.cuda.synchronize()
    with_leader = int((fo.leader >= 0).sum().item())
    err, dev = fo._track["err"], torch.device("cuda", 0)
    track = dict(fo._track)

    def kernel_alone():
        fleet._lib.kmpc_follow_fleet(0, B, ptr(err[:, 3]), 4, ptr(st[:, 3]), 8, ptr(fleet.path_id), None, ptr(fo.rows), ptr(vt), ptr(out),
                                     ptr(fo.gap_leader), ptr(fo.leader), ptr(fo.stat), stream(dev))
    tw, tk, tc, ts = [], [], [], []
    for _ in range(REPEATS):   # alternating
        tw.append(event_time(lambda: fleet.get_waypoints_batch(pose, vt), reps))
        tk.append(event_time(kernel_alone, reps))
        ts.append(event_time(lambda: fleet.track_score_batch(st, score=None, out=track), reps))
        tc.append(event_time(lambda: fo.cap(st, vt, out=out), reps))
    say("   B = %d (%d vehicles with a leader), %d calls per repeat:" % (B, with_leader, reps))
    say("     kmpc_waypoints_fleet, target-velocity mode:                  %10.1f [%10.1f, %10.1f]" % med(tw))
    say("     kmpc_follow_fleet alone (arclengths given):                  %10.1f [%10.1f, %10.1f]   %.3f x the waypoint call; %.4f ns per follower-candidate pair"
        % (med(tk) + (med(tk)[0] / med(tw)[0], med(tk)[0] * 1e3 / (float(B) * B))))
    say("     kmpc_track_score_fleet, geometry only (score = None):        %10.1f [%10.1f, %10.1f]" % med(ts))
    say("     Follower.cap(): score call + on-the-road mask + the kernel:  %10.1f [%10.1f, %10.1f]   %.3f x the waypoint call" % (med(tc) + (med(tc)[0] / med(tw)[0],)))


def make_loop(B, with_follower):
    fleet, state = setup(B, B // PLATOON)
    sim = VehicleSimulator(B, X0=state[:, 0], Y0=state[:, 1], Psi0=state[:, 2])
    sim.state[:, 3] = 6.0
    kw = {}
    if with_follower:
        from mkz_mpc_path_follower_amd.ref_traj import Follower
        kw["follower"] = Follower(fleet)
    return ClosedLoop(fleet, sim, N=N, target_vel=6.0, **kw)


def loop_rate(B, with_follower, steps):
    loop = make_loop(B, with_follower)
    for _w in range(20):
        loop.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _s in range(steps):
        o = loop.step()
    torch.cuda.synchronize()
    rate = B * steps / (time.perf_counter() - t0) / 1e6
    bound = int(loop.follower.summary()["n_bound"].sum()) if with_follower else 0
    return rate, int(o["status"].max().item()), float(o["iters"].double().mean().item()), bound


def loops(B=4096, steps=100):
    kinds = [("without follower=", False), ("with follower= (default rows)", True)]
    res = {k: [] for k, _ in kinds}
    last = {}
    for _ in range(REPEATS):
        for name, wf in kinds:
            r = loop_rate(B, wf, steps)
            res[name].append(r[0])
            last[name] = r[1:]
    say("2. ClosedLoop of %d vehicles in %d platoons of %d, %g m apart at 6 m/s, N = %d, %d steps per repeat after 20 warm-up steps: M vehicle-steps/s "
        "(median [min, max] of %d)" % (B, B // PLATOON, PLATOON, SPACING, N, steps, REPEATS))
    for name, _ in kinds:
        say("   %-32s %6.2f [%6.2f, %6.2f]   (worst status of the last step: %d; its mean solver iterations: %.2f; vehicle-periods in which the cap bound: %d)"
            % ((name,) + med(res[name]) + last[name]))
    say("   ratio of the medians with / without: %.3f" % (med(res[kinds[1][0]])[0] / med(res[kinds[0][0]])[0]))


def plain(B=4096, steps=100):
    rates = [loop_rate(B, False, steps)[0] for _ in range(REPEATS)]
    print("loop without follower=, %d vehicles, tree %s: M vehicle-steps/s %s, median %.2f" % (B, ROOT, " ".join("%.2f" % r for r in rates), med(rates)[0]),
          flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "plain":
        return plain()
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    say("1. per call, us (median [min, max] of %d repeats; device events around back-to-back calls through the Python host)" % REPEATS)
    kernels(4096, 200)
    kernels(32768, 50)
    kernels(262144, 5)
    loops()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
