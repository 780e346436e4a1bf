"""Monte-Carlo closed loops on the device: a plant per vehicle with a command delay (kmpc_sim_advance_plant), the measurement stage
(kmpc_sense_batch) and the loops' `sensor=` against the fixed kernel (bit for bit where nothing differs) and the numpy restatements of
tests/plant_ref.py.

Tolerances.  Per-vehicle rows against numpy: the existing kernel test's (tests/test_closed_loop.py) -- 1e-9 m on X / Y, 1e-10 on the rest, heading
modulo 2 pi: same arithmetic, same library calls, other constants.  Normals against numpy: 1e-13 (|n| < 6.8, one ulp there is 9e-16, log / sqrt / cos
within a few ulp each; measured 8.9e-16).  Everything else is torch.equal.  Measured against numpy for the rows: 5.6e-17 m, 0 rad, 4.4e-16.
B = 300 unless a test says otherwise: two 256-thread blocks, the second partial."""
import ctypes as C
import os

import numpy as np
import pytest

import plant_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
B0 = 300
pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64).cuda()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def advance_fixed(state, cmd, n):
    """kmpc_sim_advance_batch on a copy of `state` -> the new state"""
    import torch
    from mkz_mpc_path_follower_amd import _lib
    s = state.clone()
    assert _lib.load().kmpc_sim_advance_batch(0, s.shape[0], ptr(s), ptr(cmd), n, None) == 0
    torch.cuda.synchronize()
    return s


def advance_plant(state, cmd, rows, n, delay=None, held=None):
    """kmpc_sim_advance_plant on a copy of `state` (and of `held`) -> the new state, cmd_held after the call"""
    import torch
    from mkz_mpc_path_follower_amd import _lib
    s, h = state.clone(), None if held is None else held.clone()
    assert _lib.load().kmpc_sim_advance_plant(0, s.shape[0], ptr(s), ptr(cmd), ptr(rows), ptr(delay), ptr(h), n, None) == 0
    torch.cuda.synchronize()
    return s, h


def sense(state, rows, seed, period, id_base=0):
    import torch
    from mkz_mpc_path_follower_amd import _lib
    est = torch.full((state.shape[0], 4), 777.0, dtype=torch.float64, device="cuda")
    assert _lib.load().kmpc_sense_batch(0, state.shape[0], ptr(state), ptr(rows), seed, period, id_base, ptr(est), None) == 0
    torch.cuda.synchronize()
    return est


def heading_diff(a, b):
    return np.abs((a - b + np.pi) % (2 * np.pi) - np.pi)


# ---------------------------------------------------------------- 1-3: the plant kernel
def test_default_rows_are_the_fixed_kernel_bit_for_bit():
    import torch
    s0, cmd = R.draw_states(np.random.default_rng(5), B0)
    assert (s0[:, 3] == 0).sum() > 10                       # standing starts included
    s0, cmd, rows = dev(s0), dev(cmd), dev(np.tile(R.DEFAULT_ROW, (B0, 1)))
    want = advance_fixed(s0, cmd, 10)
    got, _ = advance_plant(s0, cmd, rows, 10)
    assert torch.equal(got, want) and not torch.equal(got, s0)
    # through the Python surface: plant_params' rows are kmpc_plant_default's, and a simulator without plant runs the fixed kernel
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator, plant_params
    assert torch.equal(plant_params(B0), rows)
    for kw in (dict(), dict(plant=plant_params(B0)), dict(cmd_delay=0)):
        sim = VehicleSimulator(B0, **kw)
        assert (sim.plant is None) == (not kw)
        sim.state.copy_(s0); sim.cmd.copy_(cmd)
        sim._update_vehicle_model(10)
        torch.cuda.synchronize()
        assert torch.equal(sim.state, want), kw
    sim.plant = sim.plant[:, :7]
    with pytest.raises(ValueError):
        sim._update_vehicle_model(10)


@pytest.mark.parametrize("gentle", [False, True])
def test_per_vehicle_rows_match_the_restatement(gentle):
    """rows within +-30 % of the defaults, vx in [2, 20] m/s (tests/test_plant_sensor_ref.py checks these inputs on the CPU); gentle: the case whose slip
    angles stay inside the polynomial range"""
    s0, cmd, rows = R.spread_case(gentle)
    exp, _ = R.update_plant(s0, cmd, rows, n_updates=10)
    got, _ = advance_plant(dev(s0), dev(cmd), dev(rows), 10)
    got = got.cpu().numpy()
    dxy, dpsi, drest = np.abs(got[:, 0:2] - exp[:, 0:2]).max(), heading_diff(got[:, 2], exp[:, 2]).max(), np.abs(got[:, 3:] - exp[:, 3:]).max()
    print("per-vehicle rows (gentle=%s): X/Y %.3e m, psi %.3e rad, rest %.3e" % (gentle, dxy, dpsi, drest))
    assert np.isfinite(got).all()
    assert dxy < 1e-9 and dpsi < 1e-10 and drest < 1e-10
    for w in range(8):   # one word off the default row: a swapped or ignored word would leave the vehicle on the default row's state
        assert not np.array_equal(got[291 + w], got[290]), R.FIELDS[w]
        assert np.abs(got[291 + w] - got[290]).max() > 1e-6, R.FIELDS[w]
    assert np.array_equal(got[290], got[299])


def test_delay_is_two_calls_of_the_fixed_kernel():
    import torch
    rng = np.random.default_rng(7)
    s0, cmd = R.draw_states(rng, B0)
    held = np.stack([rng.uniform(-1, 1, B0), rng.uniform(-0.5, 0.5, B0)], 1)
    delay = rng.choice([0, 3, 10, 25, -2], B0).astype(np.int32)
    assert all((delay == d).sum() > 20 for d in (0, 3, 10, 25, -2))
    s0, cmd, held, rows = dev(s0), dev(cmd), dev(held), dev(np.tile(R.DEFAULT_ROW, (B0, 1)))
    got, held_after = advance_plant(s0, cmd, rows, 10, dev(delay, torch.int32), held)
    for dl in (0, 3, 10, 25, -2):
        d = min(max(dl, 0), 10)
        want = advance_fixed(advance_fixed(s0, held, d), cmd, 10 - d)
        g = torch.as_tensor(delay == dl).cuda()
        assert torch.equal(got[g], want[g]), dl
    assert torch.equal(held_after, cmd)
    # the Python surface: cmd_held starts at 0, so a simulator with a full-period delay spends its first period on the zero command
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator
    sim = VehicleSimulator(B0, cmd_delay=10)
    assert sim.cmd_delay.dtype == torch.int32 and tuple(sim.cmd_delay.shape) == (B0,) and not sim.cmd_held.any().item()
    sim.state.copy_(s0); sim.cmd.copy_(cmd)
    sim._update_vehicle_model(10)
    torch.cuda.synchronize()
    assert torch.equal(sim.state, advance_fixed(s0, torch.zeros_like(cmd), 10)) and torch.equal(sim.cmd_held, cmd)


# ---------------------------------------------------------------- 4: the measurement stage
def test_sensor_without_noise_is_truth_plus_bias():
    import torch
    rng = np.random.default_rng(9)
    s0, _ = R.draw_states(rng, B0)
    rows = np.zeros((B0, 8))
    rows[:, 4:8] = rng.normal(0, 1, (B0, 4)) * [0.5, 0.5, 0.05, 0.3]
    rows[:10, 4:8] = 0.0
    # keep heading and speed inside their ranges for the bitwise part ...
    ok = (s0[:, 2] + rows[:, 6] >= -np.pi) & (s0[:, 2] + rows[:, 6] < np.pi) & (s0[:, 3] + rows[:, 7] >= 0)
    rows[~ok, 6:8] = 0.0
    st, rw = dev(s0), dev(rows)
    est = sense(st, rw, 99, 4)
    assert torch.equal(est, st[:, 0:4] + rw[:, 4:8])
    assert torch.equal(est[:10], st[:10, 0:4])
    # ... then push the heading past +-pi and the speed below 0
    s1 = s0.copy()
    s1[:, 2] = np.where(np.arange(B0) % 2 == 0, 3.0, -3.0)
    s1[:, 3] = 0.2
    rows[:, 6] = np.where(np.arange(B0) % 2 == 0, 0.5, -0.5)
    rows[:, 7] = -0.7
    est = sense(dev(s1), dev(rows), 99, 4).cpu().numpy()
    assert (est[:, 2] >= -np.pi).all() and (est[:, 2] < np.pi).all()
    assert heading_diff(est[:, 2], s1[:, 2] + rows[:, 6]).max() < 1e-14 and np.abs(est[:, 2]).max() < 2.8
    assert (est[:, 3] == 0.0).all()
    assert np.abs(est - R.sense(s1, rows, 99, 4)).max() < 1e-14


def test_sensor_normals_match_the_restatement():
    """state 0, sigma 1, bias 0: est IS the normals (heading wrapped, speed floored); a 64-bit seed with a non-zero high word and vehicle ids that
    cross 2^32, so both high words of key and counter are exercised.  A second state with v = 8 keeps the speed channel's negative normals."""
    seed, id_base = 0x9E3779B97F4A7C15, 2 ** 32 - 100
    rows = np.zeros((B0, 8)); rows[:, 0:4] = 1.0
    worst = 0.0
    for v in (0.0, 8.0):
        s0 = np.zeros((B0, 8)); s0[:, 3] = v
        for period in (0, 1, 2 ** 33 + 5):
            got = sense(dev(s0), dev(rows), seed, period, id_base).cpu().numpy()
            exp = R.sense(s0, rows, seed, period, id_base)
            worst = max(worst, np.abs(got - exp).max())
            assert np.isfinite(got).all() and np.abs(got[:, 0:2]).max() < 6.8
    print("normals against numpy: %.3e" % worst)
    assert worst < 1e-13


def test_sensor_noise_depends_on_vehicle_id_period_and_seed_only():
    import torch
    rng = np.random.default_rng(10)
    s0, _ = R.draw_states(rng, B0)
    rows = np.zeros((B0, 8)); rows[:, 0:4] = [0.2, 0.2, 0.01, 0.1]; rows[:, 4:8] = [0.1, -0.1, 0.0, 0.05]
    st, rw = dev(s0), dev(rows)
    whole = sense(st, rw, 5, 17, 0)
    part = sense(st[100:116].contiguous(), rw[100:116].contiguous(), 5, 17, 100)
    assert torch.equal(whole[100:116], part)
    for other in (sense(st, rw, 5, 18, 0), sense(st, rw, 6, 17, 0), sense(st, rw, 5 + 2 ** 32, 17, 0), sense(st, rw, 5, 17 + 2 ** 32, 0)):
        assert (other[:, 0:3] != whole[:, 0:3]).all().item()            # every row, every channel (the speed channel may sit on its floor)
    from mkz_mpc_path_follower_amd.vehicle_sim import SensorModel
    sm = SensorModel(B0, sigma=(0.2, 0.2, 0.01, 0.1), bias=(0.1, -0.1, 0.0, 0.05), seed=5)
    assert torch.equal(sm.sense(st, 17), whole)
    out = torch.empty_like(whole)
    assert sm.sense(st, 17, out=out) is out and torch.equal(out, whole)


# ---------------------------------------------------------------- 5-7: the loops
@pytest.fixture(scope="module")
def path1():
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    d = np.load(os.path.join(HERE, "golden", "path1_decimated.npz"))
    grt = GPSRefTrajectory(arrays=dict(t=d["t"], lat=d["lat"], lon=d["lon"], psi=d["psi"]), traj_horizon=8, traj_dt=0.2)
    return grt, grt.get_global_trajectory_reference()


def starts(tr, B, seed=11):
    """as tests/test_closed_loop.py::test_closed_loop_tracks_the_recorded_path: on / next to the first 60 % of the path, at rest -> X0, Y0, Psi0"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, int(0.6 * len(tr)), B)
    lat = rng.normal(0, 0.5, B)
    psi0 = tr[idx, 3]
    return tr[idx, 4] - lat * np.sin(psi0), tr[idx, 5] + lat * np.cos(psi0), psi0 + rng.normal(0, 0.05, B)


def make_loop(kind, grt, X0, Y0, P0, vt=8.0, sensor=None, **sim_kw):
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop, ClosedLoopFrenet
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator
    sim = VehicleSimulator(len(X0), X0=X0, Y0=Y0, Psi0=P0, **sim_kw)
    if kind == "frenet":
        return ClosedLoopFrenet(grt, sim, 8, vt, sensor=sensor)
    return ClosedLoop(grt, sim, N=8, target_vel=vt, sensor=sensor)


@pytest.mark.parametrize("kind", ["cartesian", "frenet"])
def test_loops_off_means_off(path1, kind):
    """a sensor without noise or bias, default plant rows and zero delay: the plain loop's states and commands, bit for bit"""
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import SensorModel, plant_params
    grt, tr = path1
    B, K = 64, 30
    X0, Y0, P0 = starts(tr, B)
    plain = make_loop(kind, grt, X0, Y0, P0).run(K, history=True)
    loop = make_loop(kind, grt, X0, Y0, P0, sensor=SensorModel(B, sigma=0.0, bias=0.0, seed=3), plant=plant_params(B), cmd_delay=0)
    full = loop.run(K, history=True)
    torch.cuda.synchronize()
    assert "est" not in plain and tuple(full["est"].shape) == (K, B, 4)
    assert torch.equal(full["state"], plain["state"]) and torch.equal(full["cmd"], plain["cmd"])
    assert torch.equal(full["status"], plain["status"]) and torch.equal(full["score"], plain["score"])
    assert torch.equal(full["est"], full["state"][:K, :, 0:4]) and torch.equal(loop.est, full["est"][K - 1])
    assert (full["state"][K, :, 3] > 1.0).all().item()                      # the cars did pull away
    with pytest.raises(ValueError):
        make_loop(kind, grt, X0, Y0, P0, sensor=SensorModel(B + 1))


def test_a_gps_bias_moves_the_car_by_the_bias(path1):
    """Loop A measures its position 0.3 m east and 0.4 m south of where it is; loop B, without a sensor, starts that much east and south of A.  Both
    controllers see the same, and the plant integrates X, Y and is translation-invariant: A's track + bias is B's track.
    Measured on the MI355X over all 40 periods: positions 2.274e-13 m, the other six states 8.034e-15 (bounds 1e-6: six orders under the 0.5 m the
    test exists to see, and the measured figure is well under the 1e-8 above which the difference would need an explanation)."""
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import SensorModel
    grt, tr = path1
    B, K = 64, 40
    bias = (0.3, -0.4)
    X0, Y0, P0 = starts(tr, B)
    a = make_loop("cartesian", grt, X0, Y0, P0, sensor=SensorModel(B, sigma=0.0, bias=(bias[0], bias[1], 0.0, 0.0))).run(K, history=True)
    b = make_loop("cartesian", grt, X0 + bias[0], Y0 + bias[1], P0).run(K, history=True)
    torch.cuda.synchronize()
    sa, sb = a["state"].cpu().numpy(), b["state"].cpu().numpy()
    dxy = np.abs(sa[:, :, 0:2] + np.array(bias) - sb[:, :, 0:2]).max()
    drest = max(heading_diff(sa[:, :, 2], sb[:, :, 2]).max(), np.abs(sa[:, :, 3:] - sb[:, :, 3:]).max())
    print("GPS bias: positions %.3e m, other states %.3e" % (dxy, drest))
    assert np.hypot(*(sa[K, :, 0:2] - sa[0, :, 0:2]).T).min() > 5.0          # the cars travelled
    assert dxy < 1e-6 and drest < 1e-6


def test_noise_and_mismatch_show_in_the_score_and_nothing_breaks(path1):
    """four groups of 64 in one loop: nominal; mass +30 % with both cornering stiffnesses -30 %; GPS sigma 0.2 m; commands 50 ms late.
    Medians of rms_ect measured on the MI355X (printed; DESIGN.md section 8a has them): 0.2129, 0.2328, 0.2254, 0.2139 m -- findings; only what follows
    without a measurement is asserted."""
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import SensorModel, plant_params
    grt, tr = path1
    G, K = 64, 120
    B = 4 * G
    x, y, p = starts(tr, G)
    X0, Y0, P0 = np.tile(x, 4), np.tile(y, 4), np.tile(p, 4)
    grp = np.repeat(np.arange(4), G)
    d = R.DEFAULT_ROW
    rows = plant_params(B, m=np.where(grp == 1, 1.3, 1.0) * d[2], C_alpha_f=np.where(grp == 1, 0.7, 1.0) * d[4], C_alpha_r=np.where(grp == 1, 0.7, 1.0) * d[5])
    sigma = np.zeros((B, 4)); sigma[grp == 2, 0:2] = 0.2
    loop = make_loop("cartesian", grt, X0, Y0, P0, sensor=SensorModel(B, sigma=sigma, seed=2024), plant=rows, cmd_delay=np.where(grp == 3, 5, 0))
    out = loop.run(K, history=True)
    plain = make_loop("cartesian", grt, x, y, p).run(K, history=True)
    torch.cuda.synchronize()
    assert torch.isfinite(out["state"]).all().item() and torch.isfinite(out["cmd"]).all().item()
    errors = (out["status"] == 3).sum(0).cpu().numpy()                       # periods that ended KMPC_NUMERICAL_ERROR, per vehicle
    for g in range(1, 4):
        assert errors[grp == g].max() <= errors[grp == 0].max(), (g, errors[grp == g].max(), errors[grp == 0].max())
    rms = loop.score_summary()["rms_ect"]
    med = [float(np.median(rms[grp == g])) for g in range(4)]
    print("median rms_ect [m]: nominal %.4f, heavy / soft tyres %.4f, GPS sigma 0.2 m %.4f, 50 ms delay %.4f" % tuple(med))
    assert med[2] > med[0]
    assert torch.equal(out["state"][:, :G], plain["state"]) and torch.equal(out["cmd"][:, :G], plain["cmd"])
    assert torch.equal(out["score"][:G], plain["score"])
