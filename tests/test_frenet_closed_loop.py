"""The Frenet node's loop (scripts/nodes_gazebo_sim/gazebo_sim_mpc_cmd_pub_frenet.jl:54-153) closed through the plant: on the CPU from the oracle's
restatements (frenet_scenario.oracle_frenet_loop) and on the device for a fleet (closed_loop.ClosedLoopFrenet: waypoints -> curvature fit ->
Frenet solve -> command stage -> plant, one kernel each), the two compared with each other and against what "follows the path" means here:
every solve Optimal, cross-track error <= 0.5 m from 6 s on (the settle bound of tests/scenario.py; path1 at 5 m/s -- on path2 at 12 m/s and over
path3's sharp corners at 8 m/s the kinematic Frenet model itself leaves metres, so tracking is not asserted there), rate limits respected."""
import numpy as np
import pytest

import frenet_scenario as FS

PATH, VT, N8 = "path1_decimated.npz", 5.0, 8
RELAX = 1e-8 + 1e-12   # Ipopt's bound_relax_factor on the first-step rate rows, + float slack of the subtraction


def _first_sample():
    from oracle import waypoints as W
    arr, lat0, lon0 = FS.path_arrays(PATH)
    return W.build_trajectory(arr["t"], arr["lat"], arr["lon"], arr["psi"], lat0, lon0)


# ---------------------------------------------------------------- CPU
def test_oracle_frenet_loop_follows_path1(oracle):
    """path1 at 5 m/s for 100 periods, started 0.3 m / 0.3 m / 0.1 rad off the first sample at 2.5 m/s (measured: cross-track 0.02 m from 6 s on)"""
    tr = _first_sample()
    r = FS.oracle_frenet_loop(oracle, 100, path=PATH, target_vel=VT, X0=tr[0, 4] + 0.3, Y0=tr[0, 5] + 0.3, Psi0=tr[0, 3] + 0.1, v0=2.5, N=N8)
    assert (r["status"] == 0).all() and not r["stop"].any(), np.bincount(r["status"] + 1)
    ect, _ = FS.cross_track(r["traj"][:, 4:6], r["state"][:, 0], r["state"][:, 1])
    print("oracle Frenet loop: cross-track from 6 s on %.4f m, final speed %.5f m/s, mean iters %.2f (max %d)"
          % (ect[60:].max(), r["state"][-1, 3], r["iters"].mean(), r["iters"].max()))
    assert ect[60:].max() <= 0.5
    assert abs(r["state"][-1, 3] - VT) <= 0.01
    d = np.abs(np.diff(np.vstack([[0.0, 0.0], r["cmd"]]), axis=0))
    assert d[:, 0].max() <= 0.15 + RELAX and d[:, 1].max() <= 0.05 + RELAX


# ---------------------------------------------------------------- GPU
def _fleet(N, B=64, seed=42, kernel_variant=None, frac=0.6):
    """B vehicles on the first 60 % of path1, +-1 m, +-0.2 rad, 0.3 ... 1.0 x the target speed -> (loop, start states [B,4], traj)"""
    import torch
    from mkz_mpc_path_follower_amd import ClosedLoopFrenet
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator
    arr, lat0, lon0 = FS.path_arrays(PATH)
    grt = GPSRefTrajectory(arrays=arr, traj_horizon=N, traj_dt=0.2, lat0=lat0, lon0=lon0)
    tr = grt.get_global_trajectory_reference()
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, int(frac * len(tr)), B)
    start = np.stack([tr[idx, 4] + rng.uniform(-1, 1, B), tr[idx, 5] + rng.uniform(-1, 1, B), tr[idx, 3] + rng.uniform(-0.2, 0.2, B),
                      VT * rng.uniform(0.3, 1.0, B)], 1)
    sim = VehicleSimulator(B, X0=start[:, 0], Y0=start[:, 1], Psi0=start[:, 2])
    sim.state[:, 3] = torch.as_tensor(start[:, 3], dtype=torch.float64, device=sim.device)
    opts = {} if kernel_variant is None else dict(kernel_variant=kernel_variant)
    return ClosedLoopFrenet(grt, sim, N, VT, **opts), start, tr


def _run(loop, steps):
    """-> per-step numpy logs: state [steps+1,B,8], cmd [steps,B,2], status, stop (latched), fit_status, k_poly"""
    import torch
    log = dict(state=[loop.sim.state.cpu().numpy().copy()], cmd=[], status=[], stop=[], fit_status=[], k_poly=[])
    for _ in range(steps):
        o = loop.step()
        log["cmd"].append(o["cmd"].cpu().numpy().copy()); log["status"].append(o["status"].cpu().numpy().copy())
        log["stop"].append(loop.command_stop.cpu().numpy().copy()); log["fit_status"].append(o["fit_status"].cpu().numpy().copy())
        log["k_poly"].append(o["k_poly"].cpu().numpy().copy()); log["state"].append(loop.sim.state.cpu().numpy().copy())
    torch.cuda.synchronize()
    out = {k: np.array(v) for k, v in log.items()}
    out["keys"] = set(o.keys())
    return out


@pytest.mark.gpu
def test_fleet_loop_matches_the_cpu_loop_and_follows_the_path(oracle):
    """64 vehicles, 100 periods, N = 8.  Vehicles 0 ... 3 against oracle_frenet_loop: positions within 1e-6 m, commands within 1e-6 (DESIGN section 6,
    launch-scenario row), same status and stop flags.  All 64: Optimal throughout, cross-track <= 0.5 m from 6 s on (CPU, 32 such starts: 0.24 m),
    published commands within the first-step rate limits."""
    loop, start, tr = _fleet(N8)
    g = _run(loop, 100)
    assert g["keys"] == {"k_poly", "fit_status", "ref", "cmd", "status", "iters", "cost", "solve_s"}   # ClosedLoop.step's dictionary + the fit
    for b in range(4):
        r = FS.oracle_frenet_loop(oracle, 100, path=PATH, target_vel=VT, X0=start[b, 0], Y0=start[b, 1], Psi0=start[b, 2], v0=start[b, 3], N=N8)
        dpos = np.abs(g["state"][:, b, 0:2] - r["state"][:, 0:2]).max()
        dcmd = np.abs(g["cmd"][:, b] - r["cmd"]).max()
        print("vehicle %d: max |dpos| = %.3e m, max |dcmd| = %.3e" % (b, dpos, dcmd))
        assert dpos <= 1e-6 and dcmd <= 1e-6
        assert (g["status"][:, b] == r["status"]).all() and (g["stop"][:, b] == r["stop"]).all()
    assert (g["status"] == 0).all() and (g["fit_status"] == 0).all() and not g["stop"].any()
    B = start.shape[0]
    ect = np.stack([FS.cross_track(tr[:, 4:6], g["state"][:, b, 0], g["state"][:, b, 1])[0] for b in range(B)], 1)
    print("fleet: cross-track from 6 s on %.4f m" % ect[60:].max())
    assert ect[60:].max() <= 0.5
    d = np.abs(np.diff(np.concatenate([np.zeros((1, B, 2)), g["cmd"]]), axis=0))
    assert d[..., 0].max() <= 0.15 + RELAX and d[..., 1].max() <= 0.05 + RELAX, (d[..., 0].max(), d[..., 1].max())


@pytest.mark.gpu
def test_back_ends_in_the_loop():
    """the same 64 vehicles for 30 periods on the four-problems-per-wave kernel (kernel_variant = 3, the fleet configuration) and at N = 20 (one wave per
    problem): all Optimal; variant 3 within 1e-6 m of variant 2"""
    runs = {}
    for key, N, kv in (("v2", N8, 2), ("v3", N8, 3), ("n20", 20, None)):
        loop, _, _ = _fleet(N, kernel_variant=kv)
        runs[key] = _run(loop, 30)
        assert (runs[key]["status"] == 0).all() and (runs[key]["fit_status"] == 0).all(), key
    d = np.abs(runs["v3"]["state"][:, :, 0:2] - runs["v2"]["state"][:, :, 0:2]).max()
    print("kernel_variant 3 vs 2: max |dpos| = %.3e m" % d)
    assert d <= 1e-6


@pytest.mark.gpu
def test_end_of_the_path():
    """vehicles started 20 m before path1's end: the stop flag latches, the command is (-1, 0) from then on, the fit is fed clamped (bunched) waypoints
    all the while and nothing non-finite appears anywhere, the cars stop"""
    import torch
    from mkz_mpc_path_follower_amd import ClosedLoopFrenet
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator
    B = 8
    arr, lat0, lon0 = FS.path_arrays(PATH)
    grt = GPSRefTrajectory(arrays=arr, traj_horizon=N8, traj_dt=0.2, lat0=lat0, lon0=lon0)
    tr = grt.get_global_trajectory_reference()
    i0 = int(np.searchsorted(tr[:, 6], tr[-1, 6] - 20.0))
    lat = np.linspace(-0.5, 0.5, B)
    sim = VehicleSimulator(B, X0=tr[i0, 4] - lat * np.sin(tr[i0, 3]), Y0=tr[i0, 5] + lat * np.cos(tr[i0, 3]), Psi0=tr[i0, 3])
    sim.state[:, 3] = VT
    g = _run(ClosedLoopFrenet(grt, sim, N8, VT), 120)
    for k in ("state", "cmd", "k_poly"):
        assert np.isfinite(g[k]).all(), k
    assert g["stop"][-1].all() and not g["stop"][0].any()
    assert (np.diff(g["stop"].astype(int), axis=0) >= 0).all()                       # latched: never released
    latched = g["stop"]
    assert (g["cmd"][latched] == np.array([-1.0, 0.0])).all()
    live = ~latched
    assert (g["status"][live] == 0).all() and (g["fit_status"][live] == 0).all()
    assert (g["state"][-1, :, 3] == 0.0).all()


@pytest.mark.gpu
def test_wrong_setups_are_refused():
    import torch
    from mkz_mpc_path_follower_amd import BatchMPC, ClosedLoopFrenet
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator
    arr, lat0, lon0 = FS.path_arrays(PATH)
    grt = GPSRefTrajectory(arrays=arr, traj_horizon=N8, traj_dt=0.2, lat0=lat0, lon0=lon0)
    sim = VehicleSimulator(4)
    with pytest.raises(ValueError, match="target-velocity"):
        ClosedLoopFrenet(grt, sim, N8, 0.0)
    with pytest.raises(ValueError, match="target-velocity"):
        ClosedLoopFrenet(grt, sim, N8, VT, track_with_time=True)
    with pytest.raises(ValueError, match="model=1"):
        ClosedLoopFrenet(grt, sim, N8, VT, mpc=BatchMPC(N=N8))                        # Cartesian solver
    with pytest.raises(ValueError, match="float64"):
        ClosedLoopFrenet(grt, sim, N8, VT, mpc=BatchMPC(N=N8, dtype=torch.float32, model=1))
    with pytest.raises(ValueError, match="horizon"):
        ClosedLoopFrenet(grt, sim, N8, VT, mpc=BatchMPC(N=12, model=1))
    ClosedLoopFrenet(grt, sim, N8, VT, mpc=BatchMPC(N=N8, model=1, kernel_variant=3))
