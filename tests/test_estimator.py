"""The state estimator on the device (kmpc_estimate_batch, vehicle_sim.Estimator, the loops' `estimator=`) against the numpy restatement of
tests/estimator_ref.py, against itself (fresh records, containment, run() == step()) and against a CPU loop made of the oracle's parts.

Tolerances.  Kernel against restatement: same operations in the same order, contraction off; what differs is the device library's tan / atan /
sin / cos / sqrt (a few ulp from numpy's).  The project's rule: 10 x the value measured on the MI355X, capped at 1e-9 (m, rad, m/s; relative to
the record's largest covariance word for P).  Measured on the MI355X, single call: record state and est 0 (bit-identical), P 2.318e-16 relative,
innov 9.992e-16; 100-call recursion: record state and est 5.684e-14, P 4.213e-16 relative, innov 2.688e-13.  Where the measurement is 0 the bound is
10 x the smallest difference the quantity can show, one ulp of x, y = 500 m (1.137e-13).  Bounds: TOL_* below.
Flags and the two counters are exact.
B = 300 unless a test says otherwise: two 256-thread blocks, the second partial."""
import ctypes as C
import os

import numpy as np
import pytest

import estimator_ref as E
import plant_ref as R
import scenario as S

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu

# 10 x measured (module docstring), capped at 1e-9
TOL_X, TOL_P, TOL_INNOV = 1.2e-12, 2.4e-15, 1.0e-14             # single call
TOL_RUN_X, TOL_RUN_P, TOL_RUN_INNOV = 5.7e-13, 4.3e-15, 2.7e-12  # 100-call recursion


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64).cuda()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def estimate(rec, z, u, params, gate=0.0, dt=0.1, u_stride=2):
    """kmpc_estimate_batch on a copy of `rec` (numpy in, numpy out) -> rec, est, innov, flags"""
    import torch
    from mkz_mpc_path_follower_amd import _lib
    B = len(rec)
    r, zz, uu, pp = dev(rec), dev(z), dev(u), dev(params)
    est = torch.full((B, 4), 777.0, dtype=torch.float64, device="cuda")
    innov = torch.full((B, 4), 777.0, dtype=torch.float64, device="cuda")
    flags = torch.full((B,), 777, dtype=torch.int32, device="cuda")
    assert _lib.load().kmpc_estimate_batch(0, B, ptr(r), ptr(zz), ptr(uu), u_stride, ptr(pp), dt, E.L_A, E.L_B, gate, ptr(est), ptr(innov), ptr(flags), None) == 0
    torch.cuda.synchronize()
    return r.cpu().numpy(), est.cpu().numpy(), innov.cpu().numpy(), flags.cpu().numpy()


def errors(got, exp):
    """(record / est state error with the heading modulo 2 pi, P error relative to the record's largest |P| word)"""
    dx = np.abs(got[..., 0:4] - exp[..., 0:4])
    dx[..., 2] = np.abs(E.wrap(got[..., 2] - exp[..., 2]))
    if got.shape[-1] == 4:
        return dx.max(), 0.0
    scale = np.maximum(np.abs(exp[..., 4:14]).max(-1, keepdims=True), 1e-300)
    return dx.max(), (np.abs(got[..., 4:14] - exp[..., 4:14]) / scale).max()


# ---------------------------------------------------------------- 1: one call against the restatement
def test_single_call_matches_the_restatement():
    """tests/estimator_ref.py::single_call_case (tests/test_estimator_ref.py checks its groups on the CPU): flags and both counters exact, the
    rest within TOL_*"""
    c = E.single_call_case()
    exp_rec, exp_est, exp_innov, exp_flags = E.estimate(c["rec"], c["z"], c["u"], c["params"], gate=c["gate"])
    rec, est, innov, flags = estimate(c["rec"], c["z"], c["u"], c["params"], gate=c["gate"])
    assert np.array_equal(flags, exp_flags)
    assert np.array_equal(rec[:, 14], exp_rec[:, 14]) and np.array_equal(rec[:, 15], exp_rec[:, 15])
    nanz = ~np.isfinite(c["z"]).all(1) & (exp_rec[:, 14] == 0)              # the two fresh vehicles with a non-finite measurement: est = z
    assert nanz.sum() == 2 and np.array_equal(est[nanz], c["z"][nanz], equal_nan=True) and not rec[nanz].any()
    ok = ~nanz
    dx, dP = errors(rec[ok], exp_rec[ok])
    de, _ = errors(est[ok], exp_est[ok])
    di = np.abs(innov - exp_innov).max()
    print("single call against numpy: record state %.3e, P %.3e (relative), est %.3e, innov %.3e" % (dx, dP, de, di))
    assert np.isfinite(rec).all() and np.isfinite(innov).all()
    assert dx <= TOL_X and de <= TOL_X and dP <= TOL_P and di <= TOL_INNOV
    assert np.array_equal(est[ok], rec[ok, 0:4])
    # u through a stride: the same (acc, d_f) as columns 6, 7 of a [B,8] state gives the same bits
    st8 = np.zeros((len(rec), 8)); st8[:, 6:8] = c["u"]
    import torch
    from mkz_mpc_path_follower_amd import _lib
    r2, s8, e2 = dev(c["rec"]), dev(st8), torch.empty((len(rec), 4), dtype=torch.float64, device="cuda")
    assert _lib.load().kmpc_estimate_batch(0, len(rec), ptr(r2), ptr(dev(c["z"])), C.c_void_p(s8.data_ptr() + 48), 8, ptr(dev(c["params"])), 0.1, E.L_A, E.L_B,
                                           c["gate"], ptr(e2), None, None, None) == 0      # and without innov / flags
    torch.cuda.synchronize()
    assert np.array_equal(r2.cpu().numpy(), rec) and np.array_equal(e2.cpu().numpy(), est, equal_nan=True)


# ---------------------------------------------------------------- 2: fresh and contained records
def test_fresh_record_takes_the_measurement_bit_for_bit():
    rng = np.random.default_rng(8)
    B = 300
    z = np.stack([rng.uniform(-500, 500, B), rng.uniform(-500, 500, B), rng.uniform(-np.pi, np.pi, B), rng.uniform(0, 20, B)], 1)
    params = np.concatenate([np.tile([0.02, 0.02, 0.01, 0.1], (B, 1)), np.array([0.2, 0.2, 0.02, 0.1]) * rng.uniform(0.5, 2, (B, 4))], 1)
    u = rng.uniform(-0.5, 0.5, (B, 2))
    rec, est, innov, flags = estimate(np.zeros((B, 16)), z, u, params, gate=3.0)
    assert np.array_equal(est, z) and np.array_equal(rec[:, 0:4], z)
    assert np.array_equal(rec[:, [4, 8, 11, 13]], params[:, 4:8] * params[:, 4:8]) and not rec[:, [5, 6, 7, 9, 10, 12]].any()
    assert (rec[:, 14] == 1).all() and not rec[:, 15].any() and (flags == E.INIT).all() and not innov.any()


def test_a_poisoned_neighbour_changes_nothing():
    """vehicle b alone, in the batch of 300, and next to a vehicle whose record is all NaN: bit-identical; the NaN vehicle comes back reset"""
    c = E.single_call_case()
    whole = estimate(c["rec"], c["z"], c["u"], c["params"], gate=c["gate"])
    for b in (0, 45, 123, 255, 256, 299):
        alone = estimate(c["rec"][b:b + 1], c["z"][b:b + 1], c["u"][b:b + 1], c["params"][b:b + 1], gate=c["gate"])
        pair = [np.stack([a[b], a[b]]) for a in (c["rec"], c["z"], c["u"], c["params"])]
        pair[0][0] = np.nan
        two = estimate(*pair, gate=c["gate"])
        for w, a, t in zip(whole, alone, two):
            assert np.array_equal(w[b], a[0], equal_nan=True) and np.array_equal(w[b], t[1], equal_nan=True), b
        assert two[3][0] & E.RESET and not two[0][0].any() and np.array_equal(two[1][0], c["z"][b], equal_nan=True) and not two[2][0].any()
    # NaN records, rows and measurements scattered through the batch: everybody else keeps their bits
    rec, params, z = c["rec"].copy(), c["params"].copy(), c["z"].copy()
    rec[5] = np.nan; rec[257, 9] = np.inf; params[7, 2] = np.nan; params[100, 1] = np.inf
    got = estimate(rec, z, c["u"], params, gate=c["gate"])
    bad = [5, 257, 7, 100]
    keep = np.setdiff1d(np.arange(300), bad)
    for w, g in zip(whole, got):
        assert np.array_equal(w[keep], g[keep], equal_nan=True)
    assert (got[3][bad] & E.RESET).all() and not got[0][bad].any() and np.array_equal(got[1][bad], z[bad])
    exp = E.estimate(rec, z, c["u"], params, gate=c["gate"])
    assert np.array_equal(got[3], exp[3])


# ---------------------------------------------------------------- 3, 4: consistency and coasting, open loop
@pytest.fixture(scope="module")
def consistency():
    """tests/estimator_ref.py::consistency_case through vehicle_sim.Estimator, 100 calls, next to the restatement's recursion"""
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import Estimator
    k = E.consistency_case()
    K, B = k["z"].shape[0], k["z"].shape[1]
    est = Estimator(B, q=E.CONS_Q, r=E.CONS_R)
    assert np.array_equal(est.params.cpu().numpy(), k["params"])
    z, u = dev(k["z"]), dev(k["u"])
    out = dict(rec=torch.empty((K, B, 16), dtype=torch.float64, device="cuda"), est=torch.empty((K, B, 4), dtype=torch.float64, device="cuda"),
               innov=torch.empty((K, B, 4), dtype=torch.float64, device="cuda"), flags=torch.empty((K, B), dtype=torch.int32, device="cuda"))
    for j in range(K):
        est.update(z[j], u, out=out["est"][j])
        out["rec"][j].copy_(est.record); out["innov"][j].copy_(est.innov); out["flags"][j].copy_(est.flags)
    torch.cuda.synchronize()
    return k, {n: t.cpu().numpy() for n, t in out.items()}, E.run_recursion(k["z"], k["u"], k["params"])


def test_recursion_follows_the_restatement(consistency):
    k, got, exp = consistency
    assert np.array_equal(got["flags"], exp["flags"]) and np.array_equal(got["rec"][:, :, 14:16], exp["rec"][:, :, 14:16])
    dx, dP = errors(got["rec"], exp["rec"])
    de, _ = errors(got["est"], exp["est"])
    di = np.abs(got["innov"] - exp["innov"]).max()
    print("100-call recursion against numpy: record state %.3e, P %.3e (relative), est %.3e, innov %.3e" % (dx, dP, de, di))
    assert dx <= TOL_RUN_X and de <= TOL_RUN_X and dP <= TOL_RUN_P and di <= TOL_RUN_INNOV


def test_filter_is_consistent_and_beats_the_measurement(consistency):
    """mean innov^2 per channel in [0.9, 1.1] (25 344 samples, standard error 0.009; the restatement gives 0.986, 1.004, 1.001, 1.004 with this
    seed); rms error against the truth below the measurement's on every channel and below half of it on x and y (restatement: 0.357, 0.354,
    0.631, 0.785 of it)"""
    k, got, _ = consistency
    assert (got["flags"][0] == E.INIT).all() and not got["flags"][1:].any()
    m = (got["innov"][1:] ** 2).mean((0, 1))
    d, dz = got["est"] - k["truth"], k["z"] - k["truth"]
    d[..., 2], dz[..., 2] = E.wrap(d[..., 2]), E.wrap(dz[..., 2])
    ratio = np.sqrt((d[1:] ** 2).mean((0, 1)) / (dz[1:] ** 2).mean((0, 1)))
    print("mean innov^2 %s over %d samples; rms error / measurement's %s" % (np.round(m, 4), got["innov"][1:, :, 0].size, np.round(ratio, 4)))
    assert got["innov"][1:, :, 0].size == 25344
    assert (m > 0.9).all() and (m < 1.1).all()
    assert (ratio < 1.0).all() and (ratio[0:2] < 0.5).all()


def test_filter_coasts_through_a_dropout():
    """NaN on x and y for 10 periods: P_xx and P_yy grow every period, est_out stays finite, bits 0 and 1 are set, word 15 rises by 20, and the
    filter re-converges (position covariance back near its value before the dropout, far below the coasting peak: the CPU test's criterion)"""
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import Estimator
    k = E.consistency_case()
    z = k["z"][:60, :16].copy()
    z[30:40, :, 0:2] = np.nan
    est = Estimator(16, q=E.CONS_Q, r=E.CONS_R)
    zd, u = dev(z), dev(k["u"][:16])
    rec, out, flags = [], [], []
    for j in range(60):
        out.append(est.update(zd[j], u).clone()); rec.append(est.record.clone()); flags.append(est.flags.clone())
    torch.cuda.synchronize()
    rec, out, flags = (torch.stack(t).cpu().numpy() for t in (rec, out, flags))
    assert np.isfinite(out).all() and np.isfinite(rec).all()
    assert (flags[30:40] == 3).all() and not flags[40:].any() and not flags[1:30].any()
    assert (np.diff(rec[29:40, :, 4], axis=0) > 0).all() and (np.diff(rec[29:40, :, 8], axis=0) > 0).all()
    assert (rec[29, :, 15] == 0).all() and (rec[-1, :, 15] == 20).all() and (rec[-1, :, 14] == 60).all()
    t = rec[:, :, 4] + rec[:, :, 8]
    assert (t[59] < 1.25 * t[29]).all() and (t[59] < 0.6 * t[39]).all()
    d = out - k["truth"][:60, :16]
    assert np.hypot(d[50:, :, 0], d[50:, :, 1]).mean() < np.hypot(*(k["z"][50:60, :16, 0:2] - k["truth"][50:60, :16, 0:2]).transpose(2, 0, 1)).mean()
    est.reset()
    assert not est.record.any().item() and not est.flags.any().item()


# ---------------------------------------------------------------- 5: the loops
SIGMA, SEED, VT, STEPS, NV, NIDS = (0.5, 0.5, 0.02, 0.1), 2024, 6.0, 150, 48, 16
CPU_VEHICLES, CPU_STEPS = (0, 16, 32), 60
# Estimate error, rms position error of est_filt / that of est per vehicle over the 150 periods.  The CPU loop (cpu_loop below, all 48 vehicles, 150
# periods) gave 0.161 ... 0.378; bound = min(0.8, 1.5 x 0.378) = 0.567.  The same CPU loops' median rms e_ct: 0.195 m with the filter, 0.240 m without
# (two of the three starts are 0.5 m beside the path, which both figures carry), every solve Optimal.
RATIO_BOUND = 0.567


def path1_arrays():
    return S.path_arrays("path1_decimated.npz")


def starts():
    """three starts on path1 (5 %, 25 % and 45 % along it), 0.5 m left / 0.5 m right / on it, heading off by +-0.05 rad, already at the target speed;
    vehicle b uses start b // 16 and noise id b -> X0, Y0, Psi0 [48]"""
    from oracle import waypoints as W
    arr, lat0, lon0 = path1_arrays()
    tr = W.build_trajectory(arr["t"], arr["lat"], arr["lon"], arr["psi"], lat0, lon0)
    idx = (np.array([0.05, 0.25, 0.45]) * len(tr)).astype(int)
    lat, dpsi = np.array([0.5, -0.5, 0.0]), np.array([0.05, -0.05, 0.0])
    psi0 = tr[idx, 3]
    X0, Y0, P0 = tr[idx, 4] - lat * np.sin(psi0), tr[idx, 5] + lat * np.cos(psi0), psi0 + dpsi
    return np.repeat(X0, NIDS), np.repeat(Y0, NIDS), np.repeat(P0, NIDS), tr


def make_loop(kind, estimator=True, estimator_input="actuator"):
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop, ClosedLoopFrenet
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import Estimator, SensorModel, VehicleSimulator
    arr, lat0, lon0 = path1_arrays()
    grt = GPSRefTrajectory(arrays=arr, traj_horizon=8, traj_dt=0.2, lat0=lat0, lon0=lon0)
    X0, Y0, P0, _ = starts()
    sim = VehicleSimulator(NV, X0=X0, Y0=Y0, Psi0=P0)
    sim.state[:, 3] = VT
    sensor = SensorModel(NV, sigma=SIGMA, seed=SEED)
    kw = dict(sensor=sensor)
    if estimator:
        kw.update(estimator=Estimator.from_sensor(sensor), estimator_input=estimator_input)
    if kind == "frenet":
        return ClosedLoopFrenet(grt, sim, 8, VT, **kw)
    return ClosedLoop(grt, sim, N=8, target_vel=VT, **kw)


def cpu_loop(O, b, steps, estimator=True):
    """tests/scenario.py::oracle_closed_loop in target-velocity mode with the measurement stage (plant_ref.sense: vehicle b's seeded noise) and the
    estimator (estimator_ref.estimate, predicting with the plant's actuator states) in front of the controller, for vehicle b of the fleet above
    -> dict of per-step arrays: state [steps+1,8], cmd [steps,2], est, est_filt [steps,4], status [steps]"""
    from oracle import waypoints as W, vehicle_sim as V
    X0, Y0, P0, traj = starts()
    p = O.params(8, S.WEIGHTS)
    s = V.initial_state(1, X0[b], Y0[b], P0[b])
    s[0, 3] = VT
    row = np.array([SIGMA + (0.0, 0.0, 0.0, 0.0)])
    par = np.array([(0.02, 0.02, 0.01, 0.1) + SIGMA])          # Estimator.from_sensor: r = sigma (all above the floor)
    rec = np.zeros((1, 16))
    u_prev, U_prev, have_warm, command_stop = np.zeros(2), None, False, False
    log = dict(state=[s[0].copy()], cmd=[], est=[], est_filt=[], status=[])
    for k in range(steps):
        z = R.sense(s, row, SEED, k, id_base=b)
        if estimator:
            rec, seen, _, _ = E.estimate(rec, z, s[:, 6:8], par, dt=0.1)
        else:
            seen = z
        x, y, psi, v = seen[0]
        xr, yr, pr, stop, _ci = W.get_waypoints(traj, x, y, psi, VT, traj_horizon=8)
        command_stop = command_stop or stop
        assert not command_stop
        q = O.problem(p, [x, y, psi, v], np.stack([xr, yr, pr], 1), VT, u_prev)
        r = O.solve_condensed(p, q, o=O.opts(warm=1) if have_warm else O.opts(), U0=U_prev)
        cmd = r["U"][0].copy()
        u_prev, U_prev, have_warm = cmd.copy(), r["U"].copy(), True
        log["status"].append(r["status"]); log["cmd"].append(cmd); log["est"].append(z[0].copy()); log["est_filt"].append(seen[0].copy())
        s = V.update_vehicle_model(s, cmd[None, :], n_updates=10)
        log["state"].append(s[0].copy())
    return {n: np.array(v) for n, v in log.items()}


def position_ratio(state, est, est_filt):
    """rms position error of est_filt against the truth / that of est, per vehicle: state [K+1,B,8], est, est_filt [K,B,4] -> [B]"""
    K = est.shape[0]
    ef = ((est_filt[:, :, 0:2] - state[:K, :, 0:2]) ** 2).sum(2).mean(0)
    er = ((est[:, :, 0:2] - state[:K, :, 0:2]) ** 2).sum(2).mean(0)
    return np.sqrt(ef / er)


@pytest.fixture(scope="module")
def cart_run():
    import torch
    loop = make_loop("cartesian")
    out = loop.run(STEPS, history=True)
    torch.cuda.synchronize()
    h = {k: out[k].cpu().numpy() for k in ("state", "cmd", "status", "latch", "est", "est_filt", "score")}
    h["record"], h["last_est"], h["last_est_filt"] = loop.estimator.record.cpu().numpy(), loop.est.cpu().numpy(), loop.est_filt.cpu().numpy()
    h["rms_ect"] = loop.score_summary()["rms_ect"]
    return h


@pytest.mark.parametrize("kind", ["cartesian", "frenet"])
def test_run_is_150_steps(kind, cart_run):
    """run(150, history=True) and 150 x step() are the same loop body: states, commands, measurements, estimates and the filter's records bit for bit"""
    import torch
    if kind == "cartesian":
        h = cart_run
    else:
        loop = make_loop(kind)
        out = loop.run(STEPS, history=True)
        torch.cuda.synchronize()
        h = {k: out[k].cpu().numpy() for k in ("state", "cmd", "status", "est", "est_filt")}
        h["record"] = loop.estimator.record.cpu().numpy()
        assert (h["status"] == 0).all() and np.isfinite(h["state"]).all() and np.isfinite(h["est_filt"]).all()
    assert h["est_filt"].shape == (STEPS, NV, 4) and h["est"].shape == (STEPS, NV, 4)
    loop = make_loop(kind)
    state, cmd, est, filt = [loop.sim.state.clone()], [], [], []
    for _ in range(STEPS):
        o = loop.step()
        state.append(loop.sim.state.clone()); cmd.append(o["cmd"].clone()); est.append(loop.est.clone()); filt.append(loop.est_filt.clone())
    torch.cuda.synchronize()
    for name, t in (("state", state), ("cmd", cmd), ("est", est), ("est_filt", filt)):
        assert np.array_equal(torch.stack(t).cpu().numpy(), h[name]), name
    assert np.array_equal(loop.estimator.record.cpu().numpy(), h["record"]) and (h["record"][:, 14] == STEPS).all()
    assert not np.array_equal(h["est"], h["est_filt"]) and np.array_equal(h["est"][0], h["est_filt"][0])     # the first period initialises from the measurement


def test_loop_options_are_checked():
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop
    from mkz_mpc_path_follower_amd.vehicle_sim import Estimator
    loop = make_loop("cartesian", estimator=False)
    assert loop.estimator is None and loop.est_filt is None
    with pytest.raises(ValueError):
        ClosedLoop(loop.grt, loop.sim, N=8, target_vel=VT, estimator=Estimator(NV + 1))
    with pytest.raises(ValueError):
        ClosedLoop(loop.grt, loop.sim, N=8, target_vel=VT, estimator=Estimator(NV), estimator_input="state")
    with pytest.raises(ValueError):
        Estimator(NV).update(loop.sim.state[:, 0:4], loop.sim.cmd)          # z must be contiguous
    with pytest.raises(ValueError):
        Estimator(NV).update(loop.sim.state[:, 0:4].contiguous(), loop.sim.state[:, 5:8:2])


def test_estimator_without_a_sensor_and_on_the_command(cart_run):
    """no sensor: the filter reads the truth (r = its floor); estimator_input="command": another prediction input, so other estimates -- and within
    the 0.8 that caps the estimate-error bound, though that bound itself was derived for the actuator-fed loop only"""
    import torch
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import Estimator, VehicleSimulator
    arr, lat0, lon0 = path1_arrays()
    X0, Y0, P0, _ = starts()
    sim = VehicleSimulator(NV, X0=X0, Y0=Y0, Psi0=P0)
    sim.state[:, 3] = VT
    loop = ClosedLoop(GPSRefTrajectory(arrays=arr, traj_horizon=8, traj_dt=0.2, lat0=lat0, lon0=lon0), sim, N=8, target_vel=VT,
                      estimator=Estimator(NV, r=(1e-3, 1e-3, 1e-4, 1e-3)))
    out = loop.run(40, history=True)
    torch.cuda.synchronize()
    assert "est" not in out and loop.est is None and tuple(out["est_filt"].shape) == (40, NV, 4)
    d = (out["est_filt"] - out["state"][:40, :, 0:4]).abs().amax((0, 1)).cpu().numpy()
    print("no sensor: |est_filt - truth| <= %s" % d)
    assert (d < [0.01, 0.01, 0.001, 0.01]).all() and (out["status"] == 0).all().item()
    h = make_loop("cartesian", estimator_input="command").run(STEPS, history=True)
    torch.cuda.synchronize()
    hc = {k: h[k].cpu().numpy() for k in ("state", "est", "est_filt", "status")}
    assert not np.array_equal(hc["est_filt"], cart_run["est_filt"]) and (hc["status"] == 0).all()
    rc, ra = position_ratio(hc["state"], hc["est"], hc["est_filt"]), position_ratio(cart_run["state"], cart_run["est"], cart_run["est_filt"])
    print("estimate error ratio, median: command-fed %.4f, actuator-fed %.4f" % (np.median(rc), np.median(ra)))
    assert rc.max() < 0.8


def test_loop_matches_the_cpu_loop(oracle, cart_run):
    """vehicles 0, 16, 32 (one per start) over 60 periods against cpu_loop: positions within 1e-6 m, the other states, the commands, the measurement
    and the estimate within 1e-6 (launch-scenario row)"""
    g = cart_run
    for b in CPU_VEHICLES:
        r = cpu_loop(oracle, b, CPU_STEPS)
        n = CPU_STEPS
        assert (r["status"] == 0).all()
        dp = np.hypot(g["state"][:n + 1, b, 0] - r["state"][:, 0], g["state"][:n + 1, b, 1] - r["state"][:, 1]).max()
        do = max(np.abs(g["state"][:n + 1, b, 2:] - r["state"][:, 2:]).max(), np.abs(g["cmd"][:n, b] - r["cmd"]).max())
        dz = max(np.abs(g["est"][:n, b] - r["est"]).max(), np.abs(g["est_filt"][:n, b] - r["est_filt"]).max())
        print("vehicle %d against the CPU loop: max |dpos| = %.3e m, other states and commands %.3e, measurement and estimate %.3e" % (b, dp, do, dz))
        assert dp <= 1e-6 and do <= 1e-6 and dz <= 1e-6, (b, dp, do, dz)


def test_filtered_loop_solves_estimates_and_tracks_better(cart_run):
    """every solve Optimal, every state finite; per vehicle the estimate's rms position error / the measurement's below RATIO_BOUND; the fleet's
    median rms e_ct below that of the same fleet, seeds and starts without estimator= (no per-vehicle assertion on e_ct: single vehicles can tie)"""
    import torch
    g = cart_run
    assert (g["status"] == 0).all() and np.isfinite(g["state"]).all() and np.isfinite(g["est_filt"]).all() and not g["latch"].any()
    assert np.array_equal(g["last_est"], g["est"][-1]) and np.array_equal(g["last_est_filt"], g["est_filt"][-1])
    ratio = position_ratio(g["state"], g["est"], g["est_filt"])
    print("estimate error ratio per vehicle: %.4f ... %.4f (bound %.2f)" % (ratio.min(), ratio.max(), RATIO_BOUND))
    assert ratio.max() < RATIO_BOUND
    raw = make_loop("cartesian", estimator=False)
    o = raw.run(STEPS, history=True)
    torch.cuda.synchronize()
    assert torch.equal(o["est"][0], torch.as_tensor(g["est"][0]).cuda())             # the same noise: same seed, ids and starts
    e_filt, e_raw = g["rms_ect"], raw.score_summary()["rms_ect"]           # scored on the device against the truth (ref_traj.track_score_batch)
    print("median rms e_ct [m]: filtered %.4f, unfiltered %.4f" % (np.median(e_filt), np.median(e_raw)))
    assert np.median(e_filt) < np.median(e_raw)
