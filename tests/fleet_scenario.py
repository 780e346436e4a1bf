"""A fleet that mixes recorded paths, tracking modes and target speeds (test helper; uses oracle/ -- test infrastructure).

The reference ships three recorded paths and two tracking modes and pairs each path with its own start pose (launch/sim_path_follow.launch:13, 22-30).  The
mixed fleet below puts six vehicles on each of the three fixture paths -- 18 in all, ordered so that the path ids are interleaved, not sorted:

  (a) time mode,               the launch pose of scenario.VARIANTS[path],                                      at rest
  (b) velocity mode, 4 m/s,    sample floor(0.1 M), offset (+0.3 m, -0.2 m, +0.05 rad),                         at rest
  (c) velocity mode, 6 m/s,    sample floor(0.3 M), same offset,                                                at rest
  (d) velocity mode, 8 m/s,    sample floor(0.5 M), same offset,                                                at rest
  (e) velocity mode, 6 m/s,    the first sample with s >= s_end - 25 m,                                         v0 = 6
  (f) time mode,               the first sample with t >= t_end - 4 s,                                          v0 = 2

(e) and (f) run off the end of their path and latch the stop flag.  The oracle loop (scenario.oracle_closed_loop: numpy waypoints + numpy plant + the C port of
the solver, one call per vehicle) is the expected behaviour; the GPU tests run all 18 through ONE ClosedLoop on a FleetRefTrajectory.
The time-mode vehicles carry target_vel = 1.0, the launch file's value (:9): the solver's v_des, weighted with C_v = 0 (mpc_cmd_pub.jl:49).
"""
import numpy as np

import scenario as S

NAMES = ("path1", "path2", "path3")
FILES = tuple(S.VARIANTS[n]["path"] for n in NAMES)
KINDS = "abcdef"
N, STEPS = 8, 60
OFFSET = (0.3, -0.2, 0.05)
# control period in which the oracle loop's stop flag latches (number of live periods before it), per kind and path; None: never within STEPS
LATCH = {"a": (None, None, None), "b": (None, None, None), "c": (None, None, None), "d": (None, None, None), "e": (22, 22, 22), "f": (32, 31, 26)}

_cache = {}


def trajectory(p):
    """[M,7] array of fixture path p (0, 1, 2), from the oracle's restatement of the constructor"""
    if ("traj", p) not in _cache:
        from oracle import waypoints as W
        arr, lat0, lon0 = S.path_arrays(FILES[p])
        _cache[("traj", p)] = W.build_trajectory(arr["t"], arr["lat"], arr["lon"], arr["psi"], lat0, lon0)
    return _cache[("traj", p)]


def path_dict(p, lo=None, hi=None):
    """what FleetRefTrajectory takes for one path: fixture path p, or its samples [lo:hi]"""
    arr, lat0, lon0 = S.path_arrays(FILES[p])
    d = {k: np.asarray(v)[lo:hi] for k, v in arr.items()}
    d.update(lat0=lat0, lon0=lon0)
    return d


def five_paths():
    """[path1, path1[0:2] (M = 2, the minimum), path2, path1[100:165] (M = 65, one more than a wave), path3]: the short paths between the long ones, so
    that an offset or lane-tail error reads a neighbour's samples"""
    return [path_dict(0), path_dict(0, 0, 2), path_dict(1), path_dict(0, 100, 165), path_dict(2)]


def vehicles():
    """the 18 vehicles, kind-major so that the path ids run 0, 1, 2, 0, 1, 2, ...: list of dict(kind, path, time_mode, target_vel, X0, Y0, Psi0, v0)"""
    out = []
    for kind in KINDS:
        for p, name in enumerate(NAMES):
            tr = trajectory(p)
            M = len(tr)
            v = dict(kind=kind, path=p, time_mode=kind in "af", target_vel=1.0, v0=0.0)
            if kind == "a":
                V = S.VARIANTS[name]
                v.update(X0=V["X0"], Y0=V["Y0"], Psi0=V["Psi0"], target_vel=V["target_vel"])
            elif kind in "bcd":
                i = int({"b": 0.1, "c": 0.3, "d": 0.5}[kind] * M)
                v.update(X0=tr[i, 4] + OFFSET[0], Y0=tr[i, 5] + OFFSET[1], Psi0=tr[i, 3] + OFFSET[2], target_vel={"b": 4.0, "c": 6.0, "d": 8.0}[kind])
            elif kind == "e":
                i = int(np.argmax(tr[:, 6] >= tr[-1, 6] - 25.0))
                v.update(X0=tr[i, 4], Y0=tr[i, 5], Psi0=tr[i, 3], target_vel=6.0, v0=6.0)
            else:
                i = int(np.argmax(tr[:, 0] >= tr[-1, 0] - 4.0))
                v.update(X0=tr[i, 4], Y0=tr[i, 5], Psi0=tr[i, 3], v0=2.0)
            out.append(v)
    return out


def oracle_fleet(O, steps=STEPS):
    """the oracle loop of every vehicle (computed once per process): list of scenario.oracle_closed_loop's dicts, in vehicles() order"""
    if ("oracle", steps) not in _cache:
        _cache[("oracle", steps)] = [S.oracle_closed_loop(O, steps, path=FILES[v["path"]], track_with_time=v["time_mode"], target_vel=v["target_vel"],
                                                          X0=v["X0"], Y0=v["Y0"], Psi0=v["Psi0"], N=N, v0=v["v0"]) for v in vehicles()]
    return _cache[("oracle", steps)]


def make_loop(vs, paths=None, path_ids=None, **kw):
    """ClosedLoop of the vehicles `vs` on a FleetRefTrajectory of `paths` (default: the three fixture paths, ids = the vehicles' own)"""
    import torch
    from mkz_mpc_path_follower_amd import ClosedLoop, FleetRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator
    paths = [path_dict(p) for p in range(3)] if paths is None else paths
    path_ids = [v["path"] for v in vs] if path_ids is None else path_ids
    grt = FleetRefTrajectory(paths, path_ids, time_mode=[int(v["time_mode"]) for v in vs], traj_horizon=N, traj_dt=0.2)
    sim = VehicleSimulator(len(vs), X0=np.array([v["X0"] for v in vs]), Y0=np.array([v["Y0"] for v in vs]), Psi0=np.array([v["Psi0"] for v in vs]))
    sim.state[:, 3] = torch.as_tensor([v["v0"] for v in vs], dtype=torch.float64, device=sim.device)
    return ClosedLoop(grt, sim, N=N, target_vel=[v["target_vel"] for v in vs], weights=S.WEIGHTS, **kw)


def run(loop, steps):
    """-> per-step numpy logs: state [steps+1,B,8], cmd [steps,B,2], status [steps,B], stop (latched) [steps,B]; plus fit_status where the loop has it"""
    import torch
    log = dict(state=[loop.sim.state.cpu().numpy().copy()], cmd=[], status=[], stop=[], fit_status=[])
    for _ in range(steps):
        o = loop.step()
        log["cmd"].append(o["cmd"].cpu().numpy().copy()); log["status"].append(o["status"].cpu().numpy().copy())
        log["stop"].append(loop.command_stop.cpu().numpy().copy()); log["state"].append(loop.sim.state.cpu().numpy().copy())
        if "fit_status" in o:
            log["fit_status"].append(o["fit_status"].cpu().numpy().copy())
    torch.cuda.synchronize()
    return {k: np.array(v) for k, v in log.items()}
