"""The method of the tools/*_timing.py, once (tools/README.md, "The timing tools").

  per call   event_time(): WARM = 3 calls, a synchronisation, a device event, `reps` back-to-back calls, a device event, a synchronisation -> us per
             call.  rotate() takes the cases of a group in rotation inside one process, REPEATS = 5 times each; med() gives median [min, max].
  per loop   loop_rates(): the kinds of loop alternate, REPEATS times each; every loop is built afresh, advanced by 20 warm-up periods, synchronised,
             advanced by `steps` periods and synchronised again -> M vehicle-steps per second of wall clock.
  report     say() prints a line and keeps it, finish(sys.argv) writes the kept lines to argv[1] when there is one.
  inputs     the fixture paths (tests/golden/path{1,2,3}_decimated.npz) and the fleets on them that more than one tool times.  Every helper takes the
             generator it draws from and draws in one fixed order, so a tool's inputs are what its seed says.

Importing this module puts the tree under test and tests/ on sys.path and does nothing else; the tree is this checkout or, for A/B runs of one tool
against two trees, the one that KMPC_TREE names.  The package itself is imported where a helper needs it.
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

REPEATS, WARM = 5, 3
FILES = ("path1_decimated.npz", "path2_decimated.npz", "path3_decimated.npz")
N, PLATOON, SPACING = 8, 8, 20.0     # the platoon fleet: horizon, vehicles per platoon, metres between them
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def finish(argv):
    if len(argv) > 1:
        with open(argv[1], "w") as f:
            f.write("".join(s + "\n" for s in LINES))


def header():
    return "%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__)


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def event_time(fn, reps, warm=WARM):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps   # us per call


def rotate(cases, repeats=REPEATS, timer=event_time, before=None):
    """cases: name -> (fn, reps), in the order they take turns -> name -> [time per repeat].  before() runs at the start of every round (the tools
    whose kernels advance a state put it back there).  timer is an argument for the test of the order alone."""
    res = {k: [] for k in cases}
    for _ in range(repeats):
        if before is not None:
            before()
        for k, (fn, reps) in cases.items():
            res[k].append(timer(fn, reps))
    return res


def run_periods(loop, n):
    return loop.run(n, score=False)


def step_periods(loop, n):
    for _ in range(n):
        o = loop.step()
    return o


def loop_rates(kinds, make, B, steps, warm=20, advance=run_periods, after=None):
    """kinds: the names of the loops, in the order they alternate; make(name) -> a fresh loop; advance(loop, n) -> what the last period returned.
    -> name -> [M vehicle-steps/s per repeat], name -> [after(loop, last) per repeat] (what a tool prints next to the rate)"""
    rates, extras = {k: [] for k in kinds}, {k: [] for k in kinds}
    for _ in range(REPEATS):
        for k in kinds:
            loop = make(k)
            advance(loop, warm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = advance(loop, steps)
            torch.cuda.synchronize()
            rates[k].append(B * steps / (time.perf_counter() - t0) / 1e6)
            if after is not None:
                extras[k].append(after(loop, last))
    return rates, extras


def path_dict(name):
    import scenario as S
    arr, lat0, lon0 = S.path_arrays(name)
    return dict(arr, lat0=lat0, lon0=lon0)


def single_path(N, name=FILES[0]):
    """-> the waypoint helper of one fixture path at horizon N, its [M,7] trajectory array"""
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    p = path_dict(name)
    grt = GPSRefTrajectory(arrays=p, traj_horizon=N, traj_dt=0.2, lat0=p["lat0"], lon0=p["lon0"])
    return grt, grt.get_global_trajectory_reference()


def scatter(tr, n, rng, frac=0.5, jitter=(0.5, 0.5, 0.05)):
    """n poses at random samples of the first `frac` of the trajectory array tr, off them by U(-j, j) per coordinate -> [n,3] (X, Y, psi).
    Draws: the samples, X, Y, psi; a coordinate whose jitter is 0 takes no draw."""
    idx = rng.integers(0, int(frac * len(tr)), n)
    return np.stack([tr[idx, c] + rng.uniform(-j, j, n) if j else tr[idx, c] for c, j in zip((4, 5, 3), jitter)], 1)


def scatter_fleet(trs, pid, rng, frac=0.6, jitter=(1.0, 1.0, 0.2)):
    """scatter() path by path, in the order of the paths, for the vehicles that pid puts on each -> [B,3]"""
    pose = np.empty((len(pid), 3))
    for p, tr in enumerate(trs):
        sel = np.where(pid == p)[0]
        pose[sel] = scatter(tr, len(sel), rng, frac, jitter)
    return pose


def interleaved_fleet(paths, B, rng, frac=0.6, jitter=(1.0, 1.0, 0.2)):
    """B vehicles, path ids interleaved (0, 1, 2, 0, ...), scattered over the first `frac` of the vehicle's path -> fleet, pose [B,3] (host)"""
    from mkz_mpc_path_follower_amd import FleetRefTrajectory
    pid = np.arange(B) % len(paths)
    fleet = FleetRefTrajectory(paths, pid, traj_horizon=N)
    return fleet, scatter_fleet(fleet.trajectories, pid, rng, frac, jitter)


def dense_fleet(B, rng):
    """the three fixture paths, ids interleaved, poses within 1 m of a random sample of the vehicle's path at the sample's heading, speeds U(2, 8):
    a dense fleet in which nearly every vehicle has a leader -> fleet, state [B,8] (host)"""
    fleet, pose = interleaved_fleet([path_dict(f) for f in FILES], B, rng, jitter=(1.0, 1.0, 0.0))
    state = np.zeros((B, 8))
    state[:, 0:3] = pose
    state[:, 3] = rng.uniform(2.0, 8.0, B)
    return fleet, state


def platoons(B, n_paths):
    """B vehicles in platoons of PLATOON on n_paths copies of the fixture paths (path p is fixture p % 3): platoon q on path q % n_paths, its
    vehicles SPACING m apart from 5 m + 170 m * (q // n_paths) on, first vehicle in front -> fleet, state [B,8] (host; at the samples' headings, 6 m/s)"""
    from mkz_mpc_path_follower_amd import FleetRefTrajectory
    base = [path_dict(f) for f in FILES]
    q = np.arange(B) // PLATOON
    pid = (q % n_paths).astype(np.int32)
    fleet = FleetRefTrajectory([base[p % 3] for p in range(n_paths)], pid, traj_horizon=N)
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


def platoon_loop(fleet, state, **stages):
    """a ClosedLoop on what platoons() returned, with the given stages (follower=, lanes=)"""
    from mkz_mpc_path_follower_amd import ClosedLoop
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator
    B = state.shape[0]
    sim = VehicleSimulator(B, X0=state[:, 0], Y0=state[:, 1], Psi0=state[:, 2])
    sim.state[:, 3] = 6.0
    return ClosedLoop(fleet, sim, N=N, target_vel=6.0, **stages)
