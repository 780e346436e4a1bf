"""Grip and road on the device: kmpc_sim_advance_road against the queue kernel it extends (bit for bit with the neutral row), against the numpy
restatement tests/road_ref.py, word by word, under bad rows, and inside the closed loops (VehicleSimulator(road=)).

Tolerances.  Tests 1, 3, 4 and 5 are exact (torch.equal): a neutral row's arithmetic is the queue kernel's operation for operation, and no lane
reads another's row.  Test 2, one period against the restatement: the same operations in the same order, contraction off; what differs is the
device's atan2 / cos / sin against numpy's over 100 sub-steps.  The project's rule (tests/test_latency.py, tests/test_estimator.py): 10 x the value
measured on the MI355X, capped at the plant test's bounds 1e-9 m on X, Y and 1e-10 on the other states, utilisation capped at 1e-9 relative.
Measured: MEASURED_STEP below.  Test 6, the loop against the CPU loop: 10 x measured, capped at 1e-6 m (the existing loop tests' cap).  Measured:
MEASURED_LOOP below.  B = 300 unless a test says otherwise: two 256-thread blocks, the second partial, not a multiple of 64."""
import ctypes as C

import numpy as np
import pytest

import latency_ref as LR
import plant_ref as R
import road_ref as RR

pytestmark = pytest.mark.gpu

B0 = 300
# measured on the MI355X (2026-10-19): one period against the restatement, max over 300 vehicles of the position difference [m], of the difference in
# the other six states, and of the relative difference of the two utilisation maxima -- see test_one_period_matches_the_restatement's docstring.
# bound = 10 x measured, capped at 1e-9 m, 1e-10 and 1e-9; where the measured value is below the smallest difference the largest value of its column
# can show (one ulp of 500 m = 1.137e-13 for the positions, of 20 m/s = 3.553e-15 for the other states), 10 x that ulp, as tests/test_latency.py does
MEASURED_STEP = (4.441e-16, 2.220e-16, 8.029e-16)
TOL_STEP = np.array([1.2e-12, 3.6e-14, 8.1e-15])
# measured on the MI355X (2026-10-19): the neutral and mu = 0.5 vehicles of the 6-vehicle, 120-period loop against the CPU loop, largest position
# difference [m] and largest difference of the other states and the commands -- see test_loop_matches_the_cpu_loop's docstring; bound = 10 x, capped
# at 1e-6
MEASURED_LOOP = (4.764e-11, 4.855e-10)
TOL_LOOP = np.array([4.8e-10, 4.9e-9])


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64).cuda()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def lib():
    from mkz_mpc_path_follower_amd import _lib
    return _lib.load()


def advance(L, state, cmd, plant, road, delay, queue, depth, p, n, stat):
    assert L.kmpc_sim_advance_road(0, state.shape[0], ptr(state), ptr(cmd), ptr(plant), ptr(road), ptr(delay), ptr(queue), depth, p, n, ptr(stat), None) == 0


# ---------------------------------------------------------------- 1: the neutral row is the queue kernel
@pytest.mark.parametrize("n", [10, 7])
def test_neutral_row_is_the_queue_kernel_bit_for_bit(n):
    """300 vehicles with +-30 % plant rows, 6 periods, depth 4, delays 0 ... 30, fresh commands every period (tests/test_road_ref.py's case 3): with
    the neutral row in every vehicle the state after every period and the ring are kmpc_sim_advance_queue's on the same arguments, road_stat stays
    zero, and road_stat = NULL gives the same state"""
    import torch
    L, depth, periods = lib(), 4, 6
    s0, _, plant = R.spread_case()
    rng = np.random.default_rng(200 + n)
    delay = rng.integers(0, 31, B0)
    cmds = np.stack([rng.uniform(-1, 1, (periods, B0)), rng.uniform(-0.5, 0.5, (periods, B0))], 2)
    plant_d, delay_d, road_d = dev(plant), dev(delay, torch.int32), dev(RR.rows(B0))
    a, b, c = dev(s0), dev(s0), dev(s0)
    qa, qb, qc = (torch.full((depth, B0, 2), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3))
    stat = torch.zeros((B0, 4), dtype=torch.float64, device="cuda")
    for p in range(periods):
        cmd = dev(cmds[p])
        assert L.kmpc_sim_advance_queue(0, B0, ptr(a), ptr(cmd), ptr(plant_d), ptr(delay_d), ptr(qa), depth, p, n, None) == 0
        advance(L, b, cmd, plant_d, road_d, delay_d, qb, depth, p, n, stat)
        advance(L, c, cmd, plant_d, road_d, delay_d, qc, depth, p, n, None)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c), (n, p)
        assert torch.equal(qa[p % depth], qb[p % depth]) and torch.equal(qa[p % depth], qc[p % depth])
    assert torch.isfinite(a).all().item() and not stat.any().item()


# ---------------------------------------------------------------- 2: against the restatement
def test_one_period_matches_the_restatement():
    """one period, n = 10, spread_case() states and plant rows, road_ref.random_rows(): mu per axle +inf (half) or U(0.2, 1.2), A_LONG U(-1, 1),
    A_LAT U(-2, 2), DF_OFFSET U(-0.05, 0.05), ACC_GAIN U(0.7, 1.3).  Saturation counts are exact except for vehicles whose restated |F| / lim came
    within 1e-9 of 1 in some sub-step (none with the committed seed: tests/test_road_ref.py).
    Measured on the MI355X: positions within 4.441e-16 m, the other states within 2.220e-16, utilisation within 8.029e-16 relative (MEASURED_STEP),
    every saturation count exact (103 vehicles saturate at the front, 15 at the rear); bounds TOL_STEP, within the caps 1e-9 m / 1e-10 / 1e-9."""
    import torch
    L = lib()
    s0, cmd, plant = R.spread_case()
    road = RR.random_rows()
    near = np.zeros(B0, dtype=bool)
    exp, exp_stat = RR.update_road(s0, cmd, plant, road, n_updates=10, near=near)
    state, stat = dev(s0), torch.zeros((B0, 4), dtype=torch.float64, device="cuda")
    queue = torch.full((2, B0, 2), float("nan"), dtype=torch.float64, device="cuda")
    advance(L, state, dev(cmd), dev(plant), dev(road), None, queue, 2, 0, 10, stat)
    torch.cuda.synchronize()
    got, got_stat = state.cpu().numpy(), stat.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(got_stat).all()
    dpos = np.hypot(got[:, 0] - exp[:, 0], got[:, 1] - exp[:, 1]).max()
    d = np.abs(got[:, 2:] - exp[:, 2:])
    d[:, 0] = np.abs((got[:, 2] - exp[:, 2] + np.pi) % (2 * np.pi) - np.pi)
    dutil = (np.abs(got_stat[:, 2:4] - exp_stat[:, 2:4]) / np.maximum(exp_stat[:, 2:4], 1e-300)).max()
    print("one period against the restatement: max |dpos| %.3e m, other states %.3e, utilisation (relative) %.3e (bounds %s); vehicles near a limit %d, "
          "saturated front %d rear %d" % (dpos, d.max(), dutil, TOL_STEP, near.sum(), (exp_stat[:, 0] > 0).sum(), (exp_stat[:, 1] > 0).sum()))
    assert near.mean() <= 0.01 and (exp_stat[:, 0] > 0).sum() >= 10 and (exp_stat[:, 1] > 0).sum() >= 10
    assert np.array_equal(got_stat[~near, 0:2], exp_stat[~near, 0:2])
    assert (np.array([dpos, d.max(), dutil]) <= TOL_STEP).all() and (TOL_STEP <= np.array([1e-9, 1e-10, 1e-9])).all()


# ---------------------------------------------------------------- 3: every word acts, and only on its own vehicle
def test_every_word_acts_on_its_own_vehicle_only():
    """ten vehicles share spread_case()'s cornering vehicle 0 (8 m/s, vy 0.15, wz 0.08, d_f 0.2) and its command: 0 and 9 on the neutral row, 1 ... 6
    differing from it in word 0 ... 5 alone, 7 and 8 in the unread words 6 and 7.  The neutral pair and the two unread-word vehicles are identical
    bit for bit; each of the six differs from them in the state."""
    import torch
    L = lib()
    s0, cmd, plant = R.spread_case()
    s0, cmd, plant = np.tile(s0[0], (10, 1)), np.tile(cmd[0], (10, 1)), np.tile(R.DEFAULT_ROW, (10, 1))
    road = RR.rows(10)
    for w, v in enumerate((0.05, 0.05, -1.0, 1.5, 0.03, 0.8, 123.0, -7.0)):
        road[1 + w, w] = v
    state, stat = dev(s0), torch.zeros((10, 4), dtype=torch.float64, device="cuda")
    queue = torch.zeros((2, 10, 2), dtype=torch.float64, device="cuda")
    advance(L, state, dev(cmd), dev(plant), dev(road), None, queue, 2, 0, 10, stat)
    torch.cuda.synchronize()
    for b in (7, 8, 9):
        assert torch.equal(state[b], state[0]) and torch.equal(stat[b], stat[0]), b
    for b in range(1, 7):
        assert not torch.equal(state[b], state[0]), RR.FIELDS[b - 1]
    st = stat.cpu().numpy()
    assert st[1, 0] > 0 and st[1, 1] == 0 and st[2, 1] > 0 and not st[0].any() and torch.isfinite(state).all().item()


# ---------------------------------------------------------------- 4: containment
def test_a_bad_row_poisons_its_own_vehicle_alone():
    """one vehicle of 300 has NaN as MU_F, one MU_R = 0: every other vehicle's state and statistics equal a run without them, bit for bit (NaN
    arithmetic in one lane: no fault)"""
    import torch
    L = lib()
    s0, cmd, plant = R.spread_case()
    road = RR.random_rows()
    bad = road.copy()
    bad[17, 0], bad[200, 1] = np.nan, 0.0
    out = []
    for rows in (road, bad):
        state, stat = dev(s0), torch.zeros((B0, 4), dtype=torch.float64, device="cuda")
        queue = torch.zeros((2, B0, 2), dtype=torch.float64, device="cuda")
        for p in range(2):
            advance(L, state, dev(cmd), dev(plant), dev(rows), None, queue, 2, p, 10, stat)
        torch.cuda.synchronize()
        out.append((state.cpu().numpy(), stat.cpu().numpy()))
    keep = np.ones(B0, bool)
    keep[[17, 200]] = False
    assert np.array_equal(out[0][0][keep], out[1][0][keep]) and np.array_equal(out[0][1][keep], out[1][1][keep])
    assert np.isfinite(out[0][0]).all() and np.isfinite(out[0][1]).all()


# ---------------------------------------------------------------- 5: off means off in the loops
def _loop(kind, sim, grt):
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop, ClosedLoopFrenet
    sim.state[:, 3] = LR.VT
    if kind == "frenet":
        return ClosedLoopFrenet(grt, sim, 8, LR.VT)
    return ClosedLoop(grt, sim, N=8, target_vel=LR.VT)


@pytest.mark.parametrize("kind", ["cartesian", "frenet"])
def test_neutral_road_leaves_the_loops_as_they_are(kind):
    """12 vehicles on path1 at 6 m/s, 20 periods, with history: VehicleSimulator(road=road_params(B)) against VehicleSimulator(cmd_queue_depth=2) --
    states, commands, statuses and scores bit for bit, and no saturated sub-step"""
    import torch
    import scenario as S
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator, road_params
    arr, lat0, lon0 = S.path_arrays("path1_decimated.npz")
    grt = GPSRefTrajectory(arrays=arr, traj_horizon=8, traj_dt=0.2, lat0=lat0, lon0=lon0)
    X0, Y0, P0, _ = LR.starts(12)
    plain = _loop(kind, VehicleSimulator(12, X0=X0, Y0=Y0, Psi0=P0, cmd_queue_depth=2), grt)
    sim = VehicleSimulator(12, X0=X0, Y0=Y0, Psi0=P0, road=road_params(12))
    assert sim.cmd_queue_depth == 2 and tuple(sim.road_stat.shape) == (12, 4) and plain.sim.road is None and plain.sim.road_summary() is None
    a, b = plain.run(20, history=True), _loop(kind, sim, grt).run(20, history=True)
    torch.cuda.synchronize()
    for k in ("state", "cmd", "status", "latch", "score"):
        assert torch.equal(a[k], b[k]), k
    assert sim.period == 20 and (b["status"] == 0).all().item() and not sim.road_stat.any().item()
    assert not sim.road_summary()["sat_f"].any() and sim.road_summary()["util_f"].shape == (12,)


# ---------------------------------------------------------------- 6: the loop against the CPU loop
OFFSETS = (0.0, 0.3)


def test_loop_matches_the_cpu_loop(oracle):
    """six vehicles on path3 from 58 % of its length, already at 6 m/s, 120 periods: neutral, mu = 0.5 and mu = 0.35, each once on the path and once
    0.3 m to its left, against road_ref.cpu_loop (the oracle's waypoints and solver, the restated plant).
    Neutral and mu = 0.5: states and commands by the 10 x rule (MEASURED_LOOP, TOL_LOOP, cap 1e-6), saturation counts exact unless the restated
    force came within 1e-9 of its limit.  mu = 0.35 slides for seconds, which amplifies the last-ulp difference between the device's polynomials
    and libm: asserted on the physics only (front saturated, max |e_ct| more than twice its neutral twin's, every solve Optimal, every state
    finite), its difference from the CPU loop printed.
    Measured on the MI355X: neutral and mu = 0.5 positions within 4.764e-11 m, other states and commands within 4.855e-10 (MEASURED_LOOP), counts
    exact (front 0, 0, 890, 1024); the mu = 0.35 vehicles 1.166e-10 m and 4.855e-10 from the CPU loop, front saturated 3676 and 3895 sub-steps as there,
    max |e_ct| 3.288 and 3.478 m against their neutral twins' 0.621 and 0.636 m."""
    import torch
    import scenario as S
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator, road_params
    runs, tr = RR.cpu_loops(oracle, OFFSETS)
    X0, Y0, P0, _ = RR.loop_start(OFFSETS)
    order = [(ri, oi) for ri in range(3) for oi in range(2)]                      # vehicle b = 2 * road + offset
    mu = np.array([RR.LOOP_ROADS[ri].get("mu", np.inf) for ri, _ in order])
    arr, lat0, lon0 = S.path_arrays(RR.PATH)
    grt = GPSRefTrajectory(arrays=arr, traj_horizon=8, traj_dt=0.2, lat0=lat0, lon0=lon0)
    sim = VehicleSimulator(6, X0=X0[[oi for _, oi in order]], Y0=Y0[[oi for _, oi in order]], Psi0=P0[[oi for _, oi in order]],
                           road=road_params(6, mu=mu))
    sim.state[:, 3] = RR.VT
    out = ClosedLoop(grt, sim, N=8, target_vel=RR.VT).run(RR.PERIODS, history=True)
    torch.cuda.synchronize()
    g = {k: out[k].cpu().numpy() for k in ("state", "cmd", "status", "latch")}
    summary = sim.road_summary()
    assert (g["status"] == 0).all() and not g["latch"].any() and np.isfinite(g["state"]).all()
    ect = np.stack([S.cross_track(tr[:, 4:6], g["state"][:, b, 0], g["state"][:, b, 1])[0] for b in range(6)], 1)
    worst = np.zeros(2)
    for b, (ri, oi) in enumerate(order):
        r = runs[(ri, OFFSETS[oi])]
        assert (r["status"] == 0).all()
        dp = np.hypot(g["state"][:, b, 0] - r["state"][:, 0], g["state"][:, b, 1] - r["state"][:, 1]).max()
        do = max(np.abs(g["state"][:, b, 2:] - r["state"][:, 2:]).max(), np.abs(g["cmd"][:, b] - r["cmd"]).max())
        print("vehicle %d (mu %s, %.1f m beside the path) against the CPU loop: max |dpos| %.3e m, other states and commands %.3e; max |e_ct| %.3f m "
              "(CPU %.3f m); saturated front %d rear %d (CPU %d, %d)%s" % (b, mu[b], OFFSETS[oi], dp, do, ect[:, b].max(), r["ect"].max(), summary["sat_f"][b],
                                                                         summary["sat_r"][b], r["stat"][0], r["stat"][1], "; near a limit" if r["near"] else ""))
        if ri < 2:
            worst = np.maximum(worst, (dp, do))
            if not r["near"]:
                assert summary["sat_f"][b] == r["stat"][0] and summary["sat_r"][b] == r["stat"][1]
        else:
            assert summary["sat_f"][b] > 0 and ect[:, b].max() > 2.0 * ect[:, oi].max()
    assert summary["sat_f"][0] == 0 and summary["sat_f"][1] == 0 and summary["sat_f"][2] > 0 and summary["sat_f"][3] > 0
    print("worst of the neutral and mu = 0.5 vehicles: %s (bounds %s)" % (worst, TOL_LOOP))
    assert (worst <= TOL_LOOP).all() and TOL_LOOP.max() <= 1e-6
