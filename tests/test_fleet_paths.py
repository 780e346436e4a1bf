"""Fleets on several recorded paths: a path and a tracking mode per vehicle (kmpc_pathset, kmpc_waypoints_fleet, ref_traj.FleetRefTrajectory and the
closed loops on it).

CPU: the C entry points' argument handling, and the mixed fleet of tests/fleet_scenario.py run by the oracle loop alone -- the expected behaviour.
GPU: the fleet kernel against the single-path kernel bit for bit and against the oracle; containment of bad path ids; the mixed fleet in ONE ClosedLoop
against the oracle loop; the same vehicles in per-path loops (the batch composition must not matter, Cartesian and Frenet); the host-side refusals.
The path set of the kernel tests is [path1, path1[0:2], path2, path1[100:165], path3]: M = 2235, 2, 2198, 65, 2209.
Measured figures of the GPU tests (each prints its own before it asserts): not measured yet -- DESIGN.md section 6 carries them once they are."""
import ctypes as C

import numpy as np
import pytest

import fleet_scenario as F

H = 8


# ---------------------------------------------------------------- CPU
def test_pathset_argument_handling():
    """KMPC_ERR_ARG before any device call; a valid call succeeds or, without a GPU, answers KMPC_ERR_NODEVICE"""
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    tr = F.trajectory(0)[:40]
    cols = [np.ascontiguousarray(np.concatenate([tr[:30, i], tr[30:40, i]])) for i in (0, 4, 5, 3, 6)]
    dp = [a.ctypes.data_as(C.POINTER(C.c_double)) for a in cols]
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    h = C.c_void_p()
    assert L.kmpc_pathset_create(0, 0, i32(30, 10), *dp, C.byref(h)) == -1                  # P = 0
    assert L.kmpc_pathset_create(0, 2, i32(39, 1), *dp, C.byref(h)) == -1                   # a path of one sample
    assert b"path 1" in L.kmpc_pathset_last_error(None)
    assert L.kmpc_pathset_create(0, 2, None, *dp, C.byref(h)) == -1                         # no sample counts
    for k in range(5):
        a = list(dp)
        a[k] = None
        assert L.kmpc_pathset_create(0, 2, i32(30, 10), *a, C.byref(h)) == -1, k             # a NULL array
    assert L.kmpc_pathset_create(0, 2, i32(30, 10), *dp, None) == -1
    assert L.kmpc_pathset_create(0, 3, i32(2**30, 2**30, 2), *dp, C.byref(h)) == -1          # 2^31 + 2 samples in all (nothing is read before the check)
    assert not h.value
    rc = L.kmpc_pathset_create(0, 2, i32(30, 10), *dp, C.byref(h))
    assert rc in (0, -3), rc
    if rc == 0:
        assert L.kmpc_waypoints_fleet(h, -1, H, 0.2, None, None, None, None, None, None, None, None) == -1
        assert L.kmpc_waypoints_fleet(h, 4, 64, 0.2, None, None, None, None, None, None, None, None) == -1
        assert L.kmpc_waypoints_fleet(h, 4, H, 0.0, None, None, None, None, None, None, None, None) == -1
        assert L.kmpc_waypoints_fleet(h, 4, H, 0.2, None, None, None, None, None, None, None, None) == -1 and b"null" in L.kmpc_pathset_last_error(h)
        assert L.kmpc_waypoints_fleet(h, 0, H, 0.2, None, None, None, None, None, None, None, None) == 0       # B = 0: no launch
        assert L.kmpc_pathset_destroy(h) == 0
    assert L.kmpc_waypoints_fleet(None, 4, H, 0.2, None, None, None, None, None, None, None, None) == -1
    assert L.kmpc_pathset_destroy(None) == 0


def test_mixed_fleet_cpu_oracle(oracle):
    """the 18 vehicles of fleet_scenario, each by the oracle loop alone: every live solve Optimal, (a)-(d) never latch, (e) latches in period 22 on all three
    paths, (f) in period 32 / 31 / 26"""
    vs, rs = F.vehicles(), F.oracle_fleet(oracle)
    assert [v["path"] for v in vs] == [0, 1, 2] * 6 and len(vs) == 18
    for v, r in zip(vs, rs):
        n = int((~r["stop"]).sum())
        print("(%s) path%d: %d live periods, mean iterations %.2f" % (v["kind"], v["path"] + 1, n, r["iters"][:n].mean()))
        assert (r["status"][:n] == 0).all(), (v["kind"], v["path"], np.bincount(r["status"][:n]))
        want = F.LATCH[v["kind"]][v["path"]]
        assert n == (F.STEPS if want is None else want), (v["kind"], v["path"], n)
        assert r["stop"][n:].all() and (r["cmd"][n:] == np.array([-1.0, 0.0])).all()


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def five():
    """the five-path set, 640 vehicles over it and the fleet kernel's answer -> dict"""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import FleetRefTrajectory
    paths = F.five_paths()
    rng = np.random.default_rng(11)
    B = 640
    pid = rng.integers(0, 5, B).astype(np.int32)
    tm = rng.integers(0, 2, B).astype(np.uint8)
    fleet = FleetRefTrajectory(paths, pid, tm, traj_horizon=H)
    assert [len(t) for t in fleet.trajectories] == [2235, 2, 2198, 65, 2209]
    pose = np.empty((B, 3))
    for p, tr in enumerate(fleet.trajectories):   # the recipe of test_waypoints.test_kernel_matches_oracle, per path
        sel = np.where(pid == p)[0]
        n, M = len(sel), len(tr)
        assert n >= 60
        idx = rng.integers(0, M, n)
        idx[:20] = np.maximum(M - 1 - np.arange(20), 0)     # the last 20 samples -> clamping / stop flag
        idx[20:40] = np.minimum(np.arange(20), M - 1)       # the first 20
        pose[sel] = np.stack([tr[idx, 4] + rng.normal(0, 1.5, n), tr[idx, 5] + rng.normal(0, 1.5, n),
                              tr[idx, 3] + rng.normal(0, 0.3, n) + rng.choice([0, 0, 0, 2 * np.pi, -2 * np.pi], n)], axis=1)
        pose[sel[40:42], :2] += 400.0                       # far away from the path (ten vehicles in all)
    vt = rng.uniform(0.5, 12.0, B)
    ref, stop, closest = fleet.get_waypoints_batch(pose, vt, want_closest=True)
    torch.cuda.synchronize()
    return dict(paths=paths, fleet=fleet, pid=pid, tm=tm, pose=pose, vt=vt, ref=ref, stop=stop, closest=closest)


@pytest.mark.gpu
def test_fleet_kernel_equals_the_single_path_kernel(five):
    """for every (path, mode) pair the fleet kernel's rows are torch.equal to GPSRefTrajectory.get_waypoints_batch on that path alone in that mode"""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    d = five
    seen = 0
    for p, src in enumerate(d["paths"]):
        g = GPSRefTrajectory(arrays=src, traj_horizon=H, lat0=src["lat0"], lon0=src["lon0"])
        assert np.array_equal(g.trajectory, d["fleet"].trajectories[p])
        for m in (0, 1):
            sel = np.where((d["pid"] == p) & (d["tm"] == m))[0]
            assert len(sel) >= 20, (p, m)
            r, s, c = g.get_waypoints_batch(d["pose"][sel], None if m else d["vt"][sel], want_closest=True)
            dsel = torch.as_tensor(sel, device=r.device)
            assert torch.equal(d["ref"][dsel], r) and torch.equal(d["stop"][dsel], s) and torch.equal(d["closest"][dsel], c), (p, m)
            seen += len(sel)
        g.close()
    assert seen == len(d["pid"])
    assert d["stop"].sum().item() > 0 and (d["stop"] == 0).sum().item() > 0


@pytest.mark.gpu
def test_fleet_kernel_matches_the_oracle(five):
    """against oracle.waypoints.get_waypoints on the vehicle's own path: closest index and stop flag exact, values <= 1e-12 (the bounds of DESIGN section 6, row f1)"""
    from oracle import waypoints as W
    d = five
    ref, stop, closest = d["ref"].cpu().numpy(), d["stop"].cpu().numpy(), d["closest"].cpu().numpy()
    worst = 0.0
    for b in range(len(d["pid"])):
        tr = d["fleet"].trajectories[d["pid"][b]]
        xi, yi, pi_, st, ci = W.get_waypoints(tr, d["pose"][b, 0], d["pose"][b, 1], d["pose"][b, 2], None if d["tm"][b] else d["vt"][b], traj_horizon=H)
        assert closest[b] == ci, (b, closest[b], ci)
        assert stop[b] == int(st), b
        e = max(np.abs(ref[b, :, 0] - xi).max(), np.abs(ref[b, :, 1] - yi).max(), np.abs(ref[b, :, 2] - pi_).max())
        worst = max(worst, e)
        assert e <= 1e-12, (b, e)
    print("fleet kernel vs oracle: max |d| = %.3e" % worst)


@pytest.mark.gpu
def test_time_mode_none_mirrors_the_single_path_call(five):
    """time_mode = None: every vehicle in target-velocity mode with v_target, every vehicle in time mode without"""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import FleetRefTrajectory
    d = five
    B = len(d["pid"])
    plain = FleetRefTrajectory(d["paths"], d["pid"], None, traj_horizon=H)
    assert plain.time_mode is None
    for with_vt in (True, False):
        a = plain.get_waypoints_batch(d["pose"], d["vt"] if with_vt else None, want_closest=True)
        moded = FleetRefTrajectory(d["paths"], d["pid"], np.full(B, 0 if with_vt else 1, dtype=np.uint8), traj_horizon=H)
        b = moded.get_waypoints_batch(d["pose"], d["vt"], want_closest=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), with_vt
        mixed_mode = torch.as_tensor(d["tm"] == (0 if with_vt else 1), device=a[0].device)   # the vehicles whose own mode this is: their rows of the mixed launch
        assert torch.equal(a[0][mixed_mode], d["ref"][mixed_mode]) and torch.equal(a[2][mixed_mode], d["closest"][mixed_mode])
        moded.close()
    with pytest.raises(ValueError, match="v_target"):
        d["fleet"].get_waypoints_batch(d["pose"], None)      # per-vehicle modes need v_target
    plain.close()


@pytest.mark.gpu
def test_bad_path_ids_are_contained():
    """path ids -1, P and 2^30 and a NaN pose on a valid path, between valid vehicles: the refused ones get stop 1, closest -1 and their own pose as every waypoint
    (a non-finite component as 0), the NaN pose gets closest 0, every output is finite and the neighbours equal a launch without the bad vehicles bit for bit"""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import FleetRefTrajectory
    paths = F.five_paths()
    P = len(paths)
    pid = np.array([0, -1, 2, P, 4, 2**30, 3, 3, -7, 1, 0], dtype=np.int32)
    tm = np.array([0, 1, 1, 0, 0, 1, 0, 1, 0, 1, 1], dtype=np.uint8)
    B = len(pid)
    fleet = FleetRefTrajectory(paths, pid, tm, traj_horizon=H)
    trs = fleet.trajectories
    rng = np.random.default_rng(5)
    pose = np.empty((B, 3))
    for b in range(B):
        tr = trs[pid[b]] if 0 <= pid[b] < P else trs[0]
        i = rng.integers(0, len(tr))
        pose[b] = (tr[i, 4] + 0.4, tr[i, 5] - 0.3, tr[i, 3] + 0.1)
    pose[6, 0] = np.nan                 # valid path, NaN pose
    pose[8, 1] = np.inf                 # refused AND non-finite
    vt = rng.uniform(2.0, 9.0, B)
    ref, stop, closest = fleet.get_waypoints_batch(pose, vt, want_closest=True)
    torch.cuda.synchronize()
    ref, stop, closest = ref.cpu().numpy(), stop.cpu().numpy(), closest.cpu().numpy()
    assert np.isfinite(ref).all()
    bad = [1, 3, 5, 8]
    for b in bad:
        want = np.where(np.isfinite(pose[b]), pose[b], 0.0)
        assert stop[b] == 1 and closest[b] == -1 and (ref[b] == want[None, :]).all(), b
    assert closest[6] == 0
    good = [b for b in range(B) if b not in bad]            # the NaN pose is a valid vehicle: it stays
    assert (closest[good] >= 0).all()
    alone = FleetRefTrajectory(paths, pid[good], tm[good], traj_horizon=H)
    r2, s2, c2 = alone.get_waypoints_batch(pose[good], vt[good], want_closest=True)
    assert np.array_equal(ref[good], r2.cpu().numpy()) and np.array_equal(stop[good], s2.cpu().numpy()) and np.array_equal(closest[good], c2.cpu().numpy())
    fleet.close(); alone.close()


@pytest.fixture(scope="module")
def mixed_run():
    """the 18 vehicles through ONE ClosedLoop on a FleetRefTrajectory of the three fixture paths, 60 control periods"""
    return F.run(F.make_loop(F.vehicles()), F.STEPS)


@pytest.mark.gpu
def test_mixed_fleet_matches_the_oracle_loop(oracle, mixed_run):
    """per vehicle against its oracle loop, up to the latch: positions <= 1e-6 m, other states and commands <= 1e-6 (launch-scenario row), status 0 on
    every live solve, the stop flag latched in the same control period"""
    g, vs, rs = mixed_run, F.vehicles(), F.oracle_fleet(oracle)
    worst_p = worst_o = 0.0
    for b, (v, r) in enumerate(zip(vs, rs)):
        n = int((~r["stop"]).sum())
        assert int((~g["stop"][:, b]).sum()) == n and g["stop"][n:, b].all(), (b, v["kind"], v["path"])
        assert (g["status"][:n, b] == 0).all() and (r["status"][:n] == 0).all(), (b, v["kind"], v["path"])
        dp = np.hypot(g["state"][:n + 1, b, 0] - r["state"][:n + 1, 0], g["state"][:n + 1, b, 1] - r["state"][:n + 1, 1]).max()
        do = max(np.abs(g["state"][:n + 1, b, 2:] - r["state"][:n + 1, 2:]).max(), np.abs(g["cmd"][:n, b] - r["cmd"][:n]).max())
        print("(%s) path%d: max |dpos| = %.3e m, other states and commands %.3e" % (v["kind"], v["path"] + 1, dp, do))
        worst_p, worst_o = max(worst_p, dp), max(worst_o, do)
        assert dp <= 1e-6 and do <= 1e-6, (b, v["kind"], v["path"], dp, do)
        assert (g["cmd"][n:, b] == np.array([-1.0, 0.0])).all()
    print("mixed fleet vs oracle loops: max |dpos| = %.3e m, max other = %.3e" % (worst_p, worst_o))


@pytest.mark.gpu
def test_batch_composition_does_not_matter(mixed_run):
    """the same 18 vehicles as three per-path loops (each on a FleetRefTrajectory of ONE path, modes mixed within it), 30 periods: state and command histories
    bit-identical to the mixed fleet's"""
    vs = F.vehicles()
    K = 30
    for p in range(3):
        sel = [b for b, v in enumerate(vs) if v["path"] == p]
        g = F.run(F.make_loop([vs[b] for b in sel], paths=[F.path_dict(p)], path_ids=[0] * len(sel)), K)
        assert np.array_equal(g["state"], mixed_run["state"][:K + 1, sel]) and np.array_equal(g["cmd"], mixed_run["cmd"][:K, sel]), p
        assert np.array_equal(g["status"], mixed_run["status"][:K, sel]) and np.array_equal(g["stop"], mixed_run["stop"][:K, sel]), p


@pytest.mark.gpu
def test_batch_composition_does_not_matter_frenet():
    """ClosedLoopFrenet, 8 vehicles, 30 periods: four on path1 at 5 m/s, four on path3 at 4 m/s, at rest on the path at floor(0.1 M) ... floor(0.4 M); the mixed loop
    equals the two per-path loops bit for bit, every solve Optimal.  (No tracking bound on path3: the kinematic Frenet model's limits there are a known limit.)"""
    import torch
    from mkz_mpc_path_follower_amd import ClosedLoopFrenet, FleetRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator
    K = 30
    vs = []
    for f in (0.1, 0.2, 0.3, 0.4):
        for p, vt in ((0, 5.0), (2, 4.0)):
            tr = F.trajectory(p)
            i = int(f * len(tr))
            vs.append(dict(path=p, vt=vt, pose=(tr[i, 4], tr[i, 5], tr[i, 3])))

    def run(sel, paths, ids):
        grt = FleetRefTrajectory(paths, ids, traj_horizon=F.N, traj_dt=0.2)
        pose = np.array([vs[b]["pose"] for b in sel])
        sim = VehicleSimulator(len(sel), X0=pose[:, 0], Y0=pose[:, 1], Psi0=pose[:, 2])
        return F.run(ClosedLoopFrenet(grt, sim, F.N, [vs[b]["vt"] for b in sel]), K)
    every = list(range(len(vs)))
    mixed = run(every, [F.path_dict(p) for p in range(3)], [v["path"] for v in vs])
    assert (mixed["status"] == 0).all() and (mixed["fit_status"] == 0).all() and not mixed["stop"].any()
    for p in (0, 2):
        sel = [b for b in every if vs[b]["path"] == p]
        g = run(sel, [F.path_dict(p)], [0] * len(sel))
        assert np.array_equal(g["state"], mixed["state"][:, sel]) and np.array_equal(g["cmd"], mixed["cmd"][:, sel]), p
        assert (g["status"] == 0).all()


@pytest.mark.gpu
def test_host_checks():
    import torch
    from mkz_mpc_path_follower_amd import ClosedLoop, ClosedLoopFrenet, FleetRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator
    paths = [F.path_dict(p) for p in range(3)]
    trs = [F.trajectory(p) for p in range(3)]
    B = 6
    pid = [0, 1, 2, 0, 1, 2]
    fleet = FleetRefTrajectory(paths, pid, [0, 0, 1, 0, 1, 0], traj_horizon=F.N)
    assert fleet.path_id.dtype == torch.int32 and fleet.time_mode.dtype == torch.uint8 and fleet.path_id.is_cuda
    sim = VehicleSimulator(B)
    with pytest.raises(ValueError, match="track_with_time"):
        ClosedLoop(fleet, sim, N=F.N, target_vel=5.0, track_with_time=True)
    with pytest.raises(ValueError, match="time mode"):
        ClosedLoopFrenet(fleet, sim, F.N, 5.0)
    with pytest.raises(ValueError, match="target_vel"):
        ClosedLoop(fleet, sim, N=F.N, target_vel=[5.0] * (B - 1))
    with pytest.raises(ValueError, match="target-velocity"):
        ClosedLoopFrenet(FleetRefTrajectory(paths, pid, traj_horizon=F.N), sim, F.N, [5.0, 4.0, 0.0, 5.0, 5.0, 5.0])
    loop = ClosedLoop(fleet, sim, N=F.N, target_vel=[5.0, -1.0, 0.0, 7.5, 2.0, 3.0])
    assert loop.v_target.tolist() == [5.0, 0.0, 0.0, 7.5, 2.0, 3.0] and loop.des_speed == (5.0, 0.0, 0.0, 7.5, 2.0, 3.0)
    assert ClosedLoop(fleet, sim, N=F.N, target_vel=6.0).des_speed == 6.0                     # a scalar keeps today's attributes
    # re-routing vehicle 3 between two calls changes its rows and nobody else's
    pose = np.array([[trs[p][300, 4] + 0.2, trs[p][300, 5] - 0.1, trs[p][300, 3]] for p in pid])
    vt = np.full(B, 5.0)
    r0, s0, c0 = fleet.get_waypoints_batch(pose, vt, want_closest=True)
    fleet.path_id[3] = 2
    r1, s1, c1 = fleet.get_waypoints_batch(pose, vt, want_closest=True)
    others = [0, 1, 2, 4, 5]
    assert torch.equal(r0[others], r1[others]) and torch.equal(c0[others], c1[others]) and torch.equal(s0[others], s1[others])
    assert not torch.equal(r0[3], r1[3])
    alone = FleetRefTrajectory(paths, [2], [0], traj_horizon=F.N)
    assert torch.equal(alone.get_waypoints_batch(pose[3:4], vt[3:4])[0][0], r1[3])
    fleet.close(); alone.close()
